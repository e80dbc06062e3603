"""Times trpx_decode_binned next to trpx_decode_indexed of the whole stack and next to what a caller pays without it (the indexed
decode, then view(n, out_h, bin_y, out_w, bin_x).sum((2, 4), dtype=int32) on the frames padded to multiples of the bin): HIP events,
warm-up, median of 20, on the stacks of DESIGN.md section 4.18, the sums checked against the replaced route's first.

    python tools/binned_time.py [--reps 20] [--frames 2000] [--stacks synth,poisson] [--bins 1,2,4,8] [--forms index,offsets,free]
                                [--detector] [--no-baselines]

--detector: 200 frames of 1030 x 1065 u16 (no multiple of the bin on either side) at bin 2 instead.
One stack, one bin and one form under a kernel trace shows k_binned_bands alone (--no-baselines).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--stacks", default="synth,poisson")
    ap.add_argument("--bins", default="1,2,4,8")
    ap.add_argument("--forms", default="index,offsets,free")
    ap.add_argument("--detector", action="store_true", help="200 frames of 1030 x 1065 at bin 2")
    ap.add_argument("--no-baselines", action="store_true", help="the binned calls alone (under a kernel trace)")
    args = ap.parse_args()
    h, w, n = (1030, 1065, 200) if args.detector else (512, 512, args.frames)
    bins = [2] if args.detector else [int(b) for b in args.bins.split(",")]
    v = h * w
    for name in args.stacks.split(","):
        px = codec.synth(np.uint16, 0, n, v) if name == "synth" else workloads.poisson_u16(3.0, 0, n, v)
        enc = codec.encode(px, index=True)
        enc.check()
        del px
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        pix = torch.empty((n, v), dtype=torch.uint16, device="cuda")
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        ws = codec.Workspace("cuda")
        ws.get(codec.decode_binned_workspace_bytes(s.numel(), v, n, np.uint16))
        base = {"stack": name, "dtype": "uint16", "frames": n, "height": h, "width": w, "stream_bytes": s.numel(),
                "lib": os.environ.get("TRPX_LIB", "product")}
        if not args.no_baselines:
            base["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, v, n, torch.uint16, out=pix, status=st, index=idx), args.reps)
        for b in bins:
            oh, ow = -(-h // b), -(-w // b)
            out = torch.empty((n, oh, ow), dtype=torch.int32, device="cuda")
            row = dict(base, bin=b, out_bytes=out.numel() * 4, bands_per_frame=_lib.lib().trpx_decode_binned_bands_per_frame(v, w, b, b, n))

            def replaced():
                codec.decode(s, offs, v, n, torch.uint16, out=pix, status=st, index=idx)
                frames = pix.view(n, h, w)
                if oh * b != h or ow * b != w:              # (edge bins: the frames padded with zeros first)
                    frames = torch.nn.functional.pad(frames.view(torch.int16), (0, ow * b - w, 0, oh * b - h)).view(torch.uint16)
                return frames.view(n, oh, b, ow, b).sum((2, 4), dtype=torch.int32)
            want = replaced()
            if not args.no_baselines:
                row["replaced_route_ms"] = median_ms(replaced, max(3, args.reps // 4), warm=1)
            for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                if form not in args.forms.split(","):
                    continue

                def call():
                    codec.decode_binned(s, o, v, n, torch.uint16, w, b, index=i, out=out, workspace=ws, status=st)
                out.fill_(-1)
                call()
                torch.cuda.synchronize()
                assert int(st[0].item()) == 0 and torch.equal(out, want), (name, b, form)
                row[f"binned_{form}_ms"] = median_ms(call, args.reps)
            del want, out
            print(json.dumps(row), flush=True)
        del enc, pix, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
