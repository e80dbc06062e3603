"""Times trpx_encode_sparse next to trpx_encode of the resident dense pixels and next to the route it replaces (zero_ the dense
stack, index_put_ the events, trpx_encode): HIP events, warm-up, median, on the stacks of DESIGN.md section 4.14 -- the events
trpx_decode_sparse gives of them -- the bytes checked against the dense encode first.

    python tools/sparse_encode_time.py [--reps 20] [--cases synth:64,poisson:8,poisson:10,empty:1]

One case under a kernel trace shows the bounds / tile-bits / scan / validate / pack kernels alone (--no-baselines).
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
    ap.add_argument("--cases", default="synth:64,poisson:8,poisson:10,empty:1", help="stack:threshold, ...")
    ap.add_argument("--no-baselines", action="store_true", help="the sparse call alone (under a kernel trace)")
    args = ap.parse_args()
    tiles = N * _lib.lib().trpx_group_count(V, 12)
    for case in args.cases.split(","):
        name, t = case.split(":")[0], int(case.split(":")[1])
        px = codec.synth(np.uint16, 0, N, V) if name == "synth" else workloads.poisson_u16(3.0, 0, N, V) if name == "poisson" \
            else torch.zeros((N, V), dtype=torch.uint16, device="cuda")
        p16 = px.view(torch.int16)                          # (synth-v1 and Poisson(3) stay below 2^15: the signed view compares alike)
        assert int(p16.min().item()) >= 0
        p16.mul_(p16 >= t)                                  # the stack of the events: everything below the threshold is zero
        ws = codec.Workspace("cuda")
        enc = codec.encode(px, workspace=ws, index=True)
        enc.check()
        rows, pos, val, st = codec.decode_sparse(enc.stack(), enc.frame_offsets, V, N, torch.uint16, max(t, 1), index=enc.index)
        assert int(st[0].item()) == 0
        n_events = pos.numel()
        want, want_offs, pb = enc.stack().clone(), enc.frame_offsets.clone(), enc.prolix_bits()
        out, offs, status = torch.empty_like(enc.data), torch.empty_like(enc.frame_offsets), torch.empty(8, dtype=torch.int32, device="cuda")
        del enc
        # tiles of 3072 pixels without an event (both passes leave them after reading their bounds)
        hit = torch.zeros(tiles, dtype=torch.bool, device="cuda")
        if n_events:
            frame = torch.repeat_interleave(torch.arange(N, device="cuda"), rows[1:] - rows[:-1])
            col = pos.view(torch.int32).to(torch.int64)
            hit[frame * (tiles // N) + col // 3072] = True
        row = {"stack": name, "threshold": t, "frames": N, "values": V, "events": n_events, "event_fraction": n_events / (N * V),
               "stream_bytes": want.numel(), "tiles": tiles, "empty_tile_fraction": 1.0 - float(hit.sum().item()) / tiles,
               "bound_bytes": codec.encode_sparse_bound_bytes(torch.uint16, V, N, n_events)}
        sws = codec.Workspace("cuda")
        sout = torch.empty(row["bound_bytes"], dtype=torch.uint8, device="cuda")

        def sparse():
            codec.encode_sparse(rows, pos if n_events else None, val if n_events else None, V, N, torch.uint16, out=sout, workspace=sws,
                                frame_offsets=offs, status=status)
        sout.fill_(0xA5)
        sparse()
        torch.cuda.synchronize()
        assert int(status[0].item()) == 0 and int(status[1].item()) == pb, (name, t)
        assert torch.equal(offs, want_offs) and torch.equal(sout[:want.numel()], want), (name, t)
        row["encode_sparse_ms"] = median_ms(sparse, args.reps)
        if not args.no_baselines:
            def dense():
                codec.encode(px, out=out, workspace=ws, frame_offsets=offs, status=status)
            row["encode_dense_ms"] = median_ms(dense, args.reps)
            v16 = val.view(torch.int16)

            def replaced():
                p16.zero_()
                if n_events:
                    p16.index_put_((frame, col), v16)
                dense()
            row["zero_put_encode_ms"] = median_ms(replaced, args.reps)
            assert int(status[0].item()) == 0 and torch.equal(out[:want.numel()], want), (name, t)
            row["sparse_over_dense"] = row["encode_sparse_ms"] / row["encode_dense_ms"]
            row["sparse_over_replaced"] = row["encode_sparse_ms"] / row["zero_put_encode_ms"]
        print(json.dumps(row), flush=True)
        del px, p16, out, sout, want, hit, ws, sws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
