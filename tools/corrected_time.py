"""Times trpx_decode_corrected next to the three terms of its aim -- trpx_decode_indexed of the whole
stack, a fill of the uint16 frames and a fill of the float32 frames: t_aim = t(indexed) - t(fill u16) + t(fill f32), the indexed
decode with its store traffic swapped for the float stores --, next to the route the call replaces (the indexed decode, then
(pix.to(float32) - dark) * gain) and next to trpx_decode_sum(group = 1, F32) followed by the two torch passes: HIP events, warm-up,
median of 20, the frames compared bit for bit with the replaced route's first.

    python tools/corrected_time.py [--reps 20] [--frames 2000] [--stacks synth,poisson] [--forms index,offsets,free] [--no-baselines]

One stack and one form under a kernel trace shows k_decode_corrected alone (--no-baselines).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trpx_amd import codec, workloads  # noqa: E402
from timing import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--stacks", default="synth,poisson")
    ap.add_argument("--forms", default="index,offsets,free")
    ap.add_argument("--no-baselines", action="store_true", help="the corrected calls alone (under a kernel trace)")
    args = ap.parse_args()
    side, n, tdt, ndt = 512, args.frames, torch.uint16, np.uint16
    v = side * side
    k = torch.arange(v, device="cuda")
    dark = ((k * 7) % 41).to(torch.float32) + 0.5
    gain = torch.tensor([1.0, 1.25, -0.75, 0.0, 2.0], dtype=torch.float32, device="cuda")[k % 5].contiguous()
    for name in args.stacks.split(","):
        px = codec.synth(ndt, 0, n, v) if name == "synth" else workloads.poisson_u16(3.0, 0, n, v)
        enc = codec.encode(px, index=True)
        enc.check()
        del px
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        pix = torch.empty((n, v), dtype=tdt, device="cuda")
        out = torch.empty((n, v), dtype=torch.float32, device="cuda")
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        ws = codec.Workspace("cuda")
        ws.get(max(codec.decode_corrected_workspace_bytes(s.numel(), v, n, ndt), codec.decode_sum_workspace_bytes(s.numel(), v, n, ndt, 1)))
        row = {"stack": name, "dtype": np.dtype(ndt).name, "frames": n, "values": v, "stream_bytes": s.numel(), "out_bytes": 4 * n * v}

        def replaced():
            codec.decode(s, offs, v, n, tdt, out=pix, status=st, index=idx)
            return (pix.to(torch.float32) - dark) * gain
        want = replaced()
        if not args.no_baselines:
            row["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, v, n, tdt, out=pix, status=st, index=idx), args.reps)
            row["fill_u16_ms"] = median_ms(lambda: pix.view(torch.int16).fill_(1), args.reps)
            row["fill_f32_ms"] = median_ms(lambda: out.fill_(1.0), args.reps)
            row["aim_ms"] = row["decode_indexed_ms"] - row["fill_u16_ms"] + row["fill_f32_ms"]
            row["replaced_route_ms"] = median_ms(replaced, max(3, args.reps // 2), warm=1)

            def summed():
                codec.decode_sum(s, offs, v, n, tdt, 1, out_dtype=torch.float32, index=idx, out=out, workspace=ws, status=st)
                out.sub_(dark).mul_(gain)
            summed()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (name, "decode_sum route")
            row["sum_group1_then_torch_ms"] = median_ms(summed, max(3, args.reps // 2), warm=1)
        for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
            if form not in args.forms.split(","):
                continue

            def call(d=dark, g=gain):
                codec.decode_corrected(s, o, v, n, tdt, dark=d, gain=g, index=i, out=out, workspace=ws, status=st)
            out.fill_(float("nan"))
            call()
            torch.cuda.synchronize()
            assert int(st[0].item()) == 0 and torch.equal(out.view(torch.int32), want.view(torch.int32)), (name, form)   # (finite maps: no NaN)
            row[f"corrected_{form}_ms"] = median_ms(call, args.reps)
            if form == "index":
                row["corrected_index_no_maps_ms"] = median_ms(lambda: call(None, None), args.reps)
                if "aim_ms" in row:
                    row["ratio_to_aim"] = row["corrected_index_ms"] / row["aim_ms"]
                    row["replaced_over_corrected"] = row["replaced_route_ms"] / row["corrected_index_ms"]
        del want
        print(json.dumps(row), flush=True)
        del enc, pix, out, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
