"""Times trpx_decode_sparse next to trpx_decode_indexed / trpx_decode of the whole stack and next to what a caller pays
without it (the indexed decode + torch.nonzero + the gather of the values): HIP events, warm-up, median, on the stacks of
DESIGN.md section 4.12, the events checked against the decoded pixels first.

    python tools/sparse_time.py [--reps 20] [--cases synth:64,poisson:8,poisson:10] [--forms index,offsets,free]

One case and one form under a kernel trace shows the count / scan / write kernels alone.
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

N, V = 2000, 512 * 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="synth:64,poisson:8,poisson:10", help="stack:threshold, ...")
    ap.add_argument("--forms", default="index,offsets,free")
    ap.add_argument("--no-baselines", action="store_true", help="the sparse calls alone (under a kernel trace)")
    args = ap.parse_args()
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]
    for name in dict.fromkeys(c[0] for c in cases):
        px = codec.synth(np.uint16, 0, N, V) if name == "synth" else workloads.poisson_u16(3.0, 0, N, V)
        enc = codec.encode(px, index=True)
        enc.check()
        del px
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        pix = torch.empty((N, V), dtype=torch.uint16, device="cuda")
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        ws = codec.Workspace("cuda")
        ws.get(max(codec.decode_sparse_workspace_bytes(s.numel(), V, N, np.uint16), _lib.lib().trpx_decode_workspace_bytes(_lib.U16, V, N, 12)))
        codec.decode(s, offs, V, N, torch.uint16, out=pix, status=st, index=idx)
        p16 = pix.view(torch.int16)                         # (synth-v1 and Poisson(3) stay below 2^15: the signed view compares alike)
        assert int(p16.min().item()) >= 0
        base = {"stack": name, "frames": N, "values": V, "stream_bytes": s.numel(), "groups": N * _lib.lib().trpx_group_count(V, 12)}
        if not args.no_baselines:
            base["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, V, N, torch.uint16, out=pix, status=st, index=idx), args.reps)
            base["decode_ms"] = median_ms(lambda: codec.decode(s, offs, V, N, torch.uint16, out=pix, status=st, workspace=ws), args.reps)
        for _, t in (c for c in cases if c[0] == name):
            row = dict(base, threshold=t)
            nz = torch.nonzero(p16 >= t)
            want_val = p16[nz[:, 0], nz[:, 1]]
            total = nz.shape[0]
            row["events"] = total
            row["event_fraction"] = total / (N * V)
            if not args.no_baselines:
                row["nonzero_gather_ms"] = median_ms(lambda: (lambda z: p16[z[:, 0], z[:, 1]])(torch.nonzero(p16 >= t)), args.reps)
            rows = torch.empty(N + 1, dtype=torch.int64, device="cuda")
            pos = torch.empty(total, dtype=torch.uint32, device="cuda")
            val = torch.empty(total, dtype=torch.uint16, device="cuda")
            for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                if form not in args.forms.split(","):
                    continue

                def call():
                    codec.decode_sparse(s, o, V, N, torch.uint16, t, index=i, capacity=total, row_offsets=rows, positions=pos,
                                        values=val, workspace=ws, status=st)
                pos.zero_(); val.zero_()
                call()
                torch.cuda.synchronize()
                assert int(st[0].item()) == 0 and int(rows[-1].item()) == total, (name, t, form)
                assert torch.equal(pos.view(torch.int32).to(torch.int64), nz[:, 1]) and torch.equal(val.view(torch.int16), want_val), (name, t, form)
                row[f"sparse_{form}_ms"] = median_ms(call, args.reps)
            del nz, want_val
            print(json.dumps(row), flush=True)
        del enc, pix, p16, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
