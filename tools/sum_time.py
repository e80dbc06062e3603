"""Times trpx_decode_sum next to trpx_decode / trpx_decode_indexed (HIP events, warm-up, median) on the stacks of
DESIGN.md section 4.9, sums checked against the decoded pixels first.  Achieved bytes/s count the algorithmic bytes of the
summing decode: stream + decode index (when given) + sums.

    python tools/sum_time.py [--reps 20] [--stacks synth,poisson,wide,c4]
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


def stack(name):
    if name == "synth":
        return codec.synth(np.uint16, 0, 2000, 512 * 512)
    if name == "poisson":
        return workloads.poisson_u16(3.0, 0, 2000, 512 * 512)
    if name == "wide":
        return workloads.poisson_u16(3.0, 0, 200, 1030 * 1065)
    if name == "c4":
        return codec.synth(np.int32, 0, 8, 4096 * 4096)
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stacks", default="synth,poisson,wide,c4")
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
        ws = codec.Workspace("cuda")
        ws.get(max(codec.decode_sum_workspace_bytes(s.numel(), v, n, dt, n),
                   codec.decode_sum_workspace_bytes(s.numel(), v, n, dt, 1),
                   _lib.lib().trpx_decode_workspace_bytes(codec.dtype_code(dt), v, n, 12)))
        row = {"stack": name, "frames": n, "values": v, "stream_bytes": s.numel()}
        row["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, v, n, dt, out=pix, status=st, index=idx), args.reps)
        row["decode_ms"] = median_ms(lambda: codec.decode(s, offs, v, n, dt, out=pix, status=st, workspace=ws), args.reps)
        row["decode_free_ms"] = median_ms(lambda: codec.decode(s, None, v, n, dt, out=pix, status=st, workspace=ws), args.reps)
        ref = pix.to(torch.int64)
        for group in (10, n) if n >= 10 else (1, n):
            want = torch.stack([ref[j:j + group].sum(0) for j in range(0, n, group)])
            sums = torch.empty((-(-n // group), v), dtype=torch.int32, device="cuda")
            for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                codec.decode_sum(s, o, v, n, dt, group, out=sums, index=i, workspace=ws, status=st)
                torch.cuda.synchronize()
                assert int(st[0].item()) == 0, (name, group, form)
                assert torch.equal(sums.to(torch.int64), want.clamp(-(1 << 31), (1 << 31) - 1)), (name, group, form)
                ms = median_ms(lambda: codec.decode_sum(s, o, v, n, dt, group, out=sums, index=i, workspace=ws, status=st),
                               args.reps)
                blocks = -(-v // 12)
                index_bytes = n * blocks + 8 * n * -(-blocks // 256)       # widths + group offsets
                algo = s.numel() + (index_bytes if i is not None else 0) + sums.numel() * 4
                row[f"sum_g{group}_{form}_ms"] = ms
                row[f"sum_g{group}_{form}_GBps"] = algo / ms / 1e6
        print(json.dumps(row), flush=True)
        del px, enc, pix, ref, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
