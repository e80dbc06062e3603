"""Times trpx_decode_sum_labelled -- every input form, three label sets -- next to the route it replaces (trpx_decode_indexed, then
index_add_ of the widened pixels) and next to trpx_decode_sum of the same stack in groups of 4 (HIP events, warm-up, median) on the
stacks of DESIGN.md section 4.20, every result checked against the decoded pixels first.

    python tools/sum_labelled_time.py [--reps 20] [--stacks synth,poisson] [--forms index,offsets,free]

The label sets on a stack of ny x nx scan positions: bin2x2 (the 2 x 2 real-space binning: 4 frames an output, pairs nx apart),
classes (8 ragged, interleaved classes, seeded), hits (one output of a seeded third of the frames, the others masked).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trpx_amd import _lib, codec, workloads  # noqa: E402
from timing import median_ms  # noqa: E402

MASK = 0xFFFFFFFF


def stack(name):
    if name == "synth":
        return codec.synth(np.uint16, 0, 480, 512 * 512), (20, 24)
    if name == "poisson":
        return workloads.poisson_u16(3.0, 0, 480, 512 * 512), (20, 24)
    if name == "synth2000":
        return codec.synth(np.uint16, 0, 2000, 512 * 512), (40, 50)
    raise ValueError(name)


def label_sets(ny, nx):
    n = ny * nx
    y, x = np.divmod(np.arange(n), nx)
    rng = np.random.default_rng(20240807)
    hits = np.full(n, MASK, np.uint32)
    hits[rng.permutation(n)[: n // 3]] = 0
    return {"bin2x2": (((y // 2) * (nx // 2) + x // 2).astype(np.uint32), (ny // 2) * (nx // 2)),
            "classes": (rng.integers(0, 8, size=n).astype(np.uint32), 8),
            "hits": (hits, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stacks", default="synth,poisson")
    ap.add_argument("--forms", default="index,offsets,free")
    args = ap.parse_args()
    for name in args.stacks.split(","):
        px, (ny, nx) = stack(name)
        n, v = px.shape
        dt = px.dtype
        enc = codec.encode(px, index=True)
        enc.check()
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        pix = torch.empty((n, v), dtype=dt, device="cuda")
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        ws = codec.Workspace("cuda")
        ws.get(max(codec.decode_sum_labelled_workspace_bytes(s.numel(), v, n, dt, n), codec.decode_sum_workspace_bytes(s.numel(), v, n, dt, 4),
                   _lib.lib().trpx_decode_workspace_bytes(codec.dtype_code(dt), v, n, 12)))
        row = {"stack": name, "dtype": str(dt).split(".")[1], "frames": n, "values": v, "stream_bytes": s.numel(),
               "frames_per_chunk": _lib.lib().trpx_decode_sum_labelled_frames_per_chunk(codec.dtype_code(dt), v, n)}
        row["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, v, n, dt, out=pix, status=st, index=idx), args.reps)
        sums = torch.empty((n // 4, v), dtype=torch.int32, device="cuda")
        row["sum_g4_index_ms"] = median_ms(lambda: codec.decode_sum(s, offs, v, n, dt, 4, out=sums, index=idx, workspace=ws, status=st), args.reps)
        del sums
        for lname, (lab_np, n_out) in label_sets(ny, nx).items():
            labels = torch.from_numpy(lab_np.view(np.int32)).cuda()
            keep = torch.from_numpy(np.nonzero(lab_np < n_out)[0]).cuda()
            lab_long = torch.from_numpy(lab_np[lab_np < n_out].astype(np.int64)).cuda()
            out = torch.empty((n_out, v), dtype=torch.int32, device="cuda")
            old = torch.empty((n_out, v), dtype=torch.int32, device="cuda")

            def replaced():
                codec.decode(s, offs, v, n, dt, out=pix, status=st, index=idx)
                old.zero_()
                # (torch gathers no uint16 rows: through the int16 view of the same bits)
                old.index_add_(0, lab_long, (pix if keep.numel() == n else pix.view(torch.int16)[keep].view(dt)).to(torch.int32))
            replaced()
            row[f"{lname}_replaced_ms"] = median_ms(replaced, args.reps)
            for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                if form not in args.forms.split(","):
                    continue

                def call():
                    codec.decode_sum_labelled(s, o, v, n, dt, labels, n_out, out_dtype=torch.int32, out=out, index=i, workspace=ws, status=st)
                out.fill_(0x5A5A5A5A)
                call()
                torch.cuda.synchronize()
                assert int(st[0].item()) == 0 and torch.equal(out, old), (name, lname, form)
                row[f"{lname}_{form}_ms"] = median_ms(call, args.reps)
            del out, old
        print(json.dumps(row), flush=True)
        del px, enc, pix, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
