"""Times trpx_decode_reduce -- every op on every input form -- next to trpx_decode_sum of the same stack and group and next to
trpx_decode_indexed (HIP events, warm-up, median) on the stacks of DESIGN.md section 4.19, every result checked against the
decoded pixels first.

    python tools/reduce_time.py [--reps 20] [--stacks synth,poisson,c4] [--ops max,min,sumsq,count] [--forms index,offsets,free]
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

THRESHOLD = 4                                               # COUNT_GE: a level inside Poisson(3) and synth-v1 data


def stack(name):
    if name == "synth":
        return codec.synth(np.uint16, 0, 2000, 512 * 512)
    if name == "poisson":
        return workloads.poisson_u16(3.0, 0, 2000, 512 * 512)
    if name == "c4":
        return codec.synth(np.int32, 0, 8, 4096 * 4096)
    raise ValueError(name)


def truth(ref, group, op):
    """the op over groups of frames of ref (int64 pixels), as the bits of the element the call writes, in int64"""
    parts = []
    for j in range(0, ref.shape[0], group):
        p = ref[j:j + group]
        parts.append(p.amax(0) if op == "max" else p.amin(0) if op == "min" else (p * p).sum(0) if op == "sumsq" else (p >= THRESHOLD).sum(0))
    return torch.stack(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stacks", default="synth,poisson,c4")
    ap.add_argument("--ops", default="max,min,sumsq,count")
    ap.add_argument("--forms", default="index,offsets,free")
    args = ap.parse_args()
    for name in args.stacks.split(","):
        px = stack(name)
        n, v = px.shape
        dt = px.dtype
        enc = codec.encode(px, index=True)
        enc.check()
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        pix = torch.empty((n, v), dtype=dt, device="cuda")
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        groups = (10, n) if n >= 10 else (1, n)
        ws = codec.Workspace("cuda")
        ws.get(max([codec.decode_reduce_workspace_bytes(s.numel(), v, n, dt, g, "sumsq") for g in groups] +
                   [codec.decode_sum_workspace_bytes(s.numel(), v, n, dt, g) for g in groups] +
                   [_lib.lib().trpx_decode_workspace_bytes(codec.dtype_code(dt), v, n, 12)]))
        row = {"stack": name, "dtype": str(dt).split(".")[1], "frames": n, "values": v, "stream_bytes": s.numel()}
        row["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, v, n, dt, out=pix, status=st, index=idx), args.reps)
        ref = pix.to(torch.int64)
        for group in groups:
            n_out = -(-n // group)
            row[f"chunks_g{group}"] = _lib.lib().trpx_decode_reduce_chunks(codec.dtype_code(dt), v, n, group)
            sums = torch.empty((n_out, v), dtype=torch.int32, device="cuda")
            for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                if form in args.forms.split(","):
                    row[f"sum_g{group}_{form}_ms"] = median_ms(
                        lambda: codec.decode_sum(s, o, v, n, dt, group, out=sums, index=i, workspace=ws, status=st), args.reps)
            for op in args.ops.split(","):
                want = truth(ref, group, op)
                out = torch.empty((n_out, v), dtype=codec.reduce_out_dtype(dt, op), device="cuda")
                for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                    if form not in args.forms.split(","):
                        continue

                    def call():
                        codec.decode_reduce(s, o, v, n, dt, group, op, threshold=THRESHOLD, out=out, index=i, workspace=ws, status=st)
                    out.view(torch.uint8).fill_(0x5A)
                    call()
                    torch.cuda.synchronize()
                    assert int(st[0].item()) == 0, (name, group, op, form)
                    got = out.view(torch.int64) if op == "sumsq" else out.to(torch.int64)
                    assert torch.equal(got, want), (name, group, op, form)
                    row[f"{op}_g{group}_{form}_ms"] = median_ms(call, args.reps)
                del want, out
        print(json.dumps(row), flush=True)
        del px, enc, pix, ref, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
