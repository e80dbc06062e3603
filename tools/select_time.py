"""Times trpx_select_frames next to two yardsticks measured in the same run: trpx_bench_stream mode 2 (a plain streaming copy)
over the same number of bytes -- the ceiling of a call that only moves bytes --, and the route the call replaces, built from the
entry points a caller had before it: trpx_decode_indexed of the whole stack, index_select on the pixels, trpx_encode.  HIP
events, warm-up, median of 20, on the stacks of DESIGN.md section 4.16; the replaced route's bytes are compared with the call's
first.

    python tools/select_time.py [--reps 20] [--frames 2000] [--stacks synth,poisson] [--lists identity,random10,random50,permutation]
                                [--with-index] [--no-baselines]

One stack and one list under a kernel trace shows the sizes / scan / verdict / copy kernels alone (--no-baselines).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trpx_amd import _lib, codec, workloads  # noqa: E402
from timing import median_ms, times_ms  # noqa: E402

SIDE = 512
V = SIDE * SIDE


def list_of(kind, n, rng):
    if kind == "identity":
        return np.arange(n)
    if kind == "permutation":
        return rng.permutation(n)
    share = {"random10": 0.1, "random50": 0.5}[kind]
    return np.sort(rng.choice(n, size=max(1, int(n * share)), replace=False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--stacks", default="synth,poisson")
    ap.add_argument("--lists", default="identity,random10,random50,permutation")
    ap.add_argument("--with-index", action="store_true", help="also carry the decode index (out_index)")
    ap.add_argument("--no-baselines", action="store_true", help="the select calls alone (under a kernel trace)")
    args = ap.parse_args()
    n = args.frames
    L = _lib.lib()
    rng = np.random.default_rng(20240807)
    for name in args.stacks.split(","):
        px = codec.synth(np.uint16, 0, n, V) if name == "synth" else workloads.poisson_u16(3.0, 0, n, V)
        enc = codec.encode(px, index=True)
        enc.check()
        del px
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        host_offs = offs.cpu().numpy()
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        ws, ws_enc = codec.Workspace("cuda"), codec.Workspace("cuda")
        for kind in args.lists.split(","):
            lst = list_of(kind, n, rng)
            k = lst.size
            frames = torch.from_numpy(lst.astype(np.int32)).cuda()
            total = int(np.diff(host_offs)[lst].sum())
            cap = (total + 15) // 16 * 16
            out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            out_offs = torch.empty(k + 1, dtype=torch.int64, device="cuda")
            row = {"stack": name, "frames": n, "values": V, "stream_bytes": s.numel(), "list": kind, "n_select": k, "selected_bytes": total}

            def call(index=None):
                return codec.select_frames(s, offs, frames, V, n, torch.uint16, index=index, out=out, workspace=ws, status=st, out_offsets=out_offs)
            call()
            torch.cuda.synchronize()
            assert int(st[0].item()) == 0 and int(out_offs[-1].item()) == total, (name, kind)
            if not args.no_baselines:
                # the copy ceiling: the same number of bytes through the streaming copy kernel
                src = s[:cap] if s.numel() >= cap else torch.empty(cap, dtype=torch.uint8, device="cuda")
                stream = torch.cuda.current_stream().cuda_stream
                row["copy_ceiling_ms"] = median_ms(lambda: _lib.check(L.trpx_bench_stream(2, src.data_ptr(), out.data_ptr(), cap, stream)), args.reps)
                call()                                       # (the ceiling wrote into `out`)
                # the replaced route: decode everything, pick the pixels, encode them
                pix = torch.empty((n, V), dtype=torch.uint16, device="cuda")
                picked_i = frames.to(torch.int64)
                out2 = torch.empty((k * codec.worst_case_bytes(np.uint16, V) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
                offs2 = torch.empty(k + 1, dtype=torch.int64, device="cuda")
                st2 = torch.empty(8, dtype=torch.int32, device="cuda")

                def replaced():
                    codec.decode(s, offs, V, n, torch.uint16, out=pix, status=st2, index=idx)
                    sel = pix.view(torch.int16).index_select(0, picked_i).view(torch.uint16)
                    return codec.encode(sel, out=out2, workspace=ws_enc, frame_offsets=offs2, status=st2)
                replaced()
                torch.cuda.synchronize()
                assert torch.equal(offs2, out_offs) and torch.equal(out2[:total], out[:total]), (name, kind)
                row["replaced_route_ms"] = median_ms(replaced, max(3, args.reps // 4), warm=1)
                del pix, out2
            ts = times_ms(call, args.reps)
            row["select_ms"], row["select_min_ms"], row["select_max_ms"] = statistics.median(ts), min(ts), max(ts)
            row["select_GBps"] = round(2 * total / row["select_ms"] / 1e6, 1)   # bytes read + bytes written
            if args.with_index:
                row["select_with_index_ms"] = median_ms(lambda: call(idx), args.reps)
            if not args.no_baselines:
                row["vs_copy_ceiling"] = round(row["select_ms"] / row["copy_ceiling_ms"], 2)
                row["vs_replaced_route"] = round(row["replaced_route_ms"] / row["select_ms"], 1)
            print(json.dumps(row), flush=True)
            del out
        del enc, ws, ws_enc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
