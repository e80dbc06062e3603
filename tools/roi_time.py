"""Times trpx_decode_roi next to trpx_decode_indexed / trpx_decode of the whole stack (HIP events, warm-up, median) on the
stacks of DESIGN.md section 4.10, the boxes checked against a crop of the decoded pixels first.

    python tools/roi_time.py [--reps 20] [--stacks synth,poisson] [--classes 64x64_per_frame,...]
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

N, H, W = 2000, 512, 512


def box_classes(rng):
    """name -> (box_h, box_w, int32 [n, 3] boxes)"""
    def per_frame(s):
        return np.stack([np.arange(N), rng.integers(H - s + 1, size=N), rng.integers(W - s + 1, size=N)], axis=1)
    frames = np.repeat(rng.choice(N, size=20, replace=False), 100)
    many = np.stack([frames, rng.integers(H - 63, size=2000), rng.integers(W - 63, size=2000)], axis=1)
    return {"64x64_per_frame": (64, 64, per_frame(64)), "256x256_per_frame": (256, 256, per_frame(256)),
            "100x64x64_in_20_frames": (64, 64, many)}


def crop(pix, boxes, bh, bw):
    b = torch.from_numpy(boxes.astype(np.int64)).cuda()
    rows = b[:, 1, None] + torch.arange(bh, device="cuda")[None, :]
    cols = b[:, 2, None] + torch.arange(bw, device="cuda")[None, :]
    return pix.view(torch.int16).view(N, H, W)[b[:, 0, None, None], rows[:, :, None], cols[:, None, :]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stacks", default="synth,poisson")
    ap.add_argument("--classes", default="", help="box classes to time (default: all); one class under a kernel trace shows its kernels alone")
    args = ap.parse_args()
    v = H * W
    for name in args.stacks.split(","):
        px = codec.synth(np.uint16, 0, N, v) if name == "synth" else workloads.poisson_u16(3.0, 0, N, v)
        enc = codec.encode(px, index=True)
        enc.check()
        del px
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        pix = torch.empty((N, v), dtype=torch.uint16, device="cuda")
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        ws = codec.Workspace("cuda")
        ws.get(max(codec.decode_roi_workspace_bytes(s.numel(), v, N, np.uint16),
                   _lib.lib().trpx_decode_workspace_bytes(_lib.U16, v, N, 12)))
        row = {"stack": name, "frames": N, "values": v, "stream_bytes": s.numel()}
        row["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, v, N, torch.uint16, out=pix, status=st, index=idx), args.reps)
        row["decode_ms"] = median_ms(lambda: codec.decode(s, offs, v, N, torch.uint16, out=pix, status=st, workspace=ws), args.reps)
        row["decode_free_ms"] = median_ms(lambda: codec.decode(s, None, v, N, torch.uint16, out=pix, status=st, workspace=ws), args.reps)
        for cls, (bh, bw, boxes) in box_classes(np.random.default_rng(1)).items():
            if args.classes and cls not in args.classes.split(","):
                continue
            want = crop(pix, boxes, bh, bw)
            d_boxes = torch.from_numpy(boxes.astype(np.int32)).cuda()
            out = torch.empty((len(boxes), bh, bw), dtype=torch.uint16, device="cuda")
            for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                def call():
                    codec.decode_roi(s, o, v, N, torch.uint16, W, d_boxes, (bh, bw), index=i, out=out, workspace=ws, status=st)
                out.zero_()
                call()
                torch.cuda.synchronize()
                assert int(st[0].item()) == 0, (name, cls, form)
                assert torch.equal(out.view(torch.int16), want), (name, cls, form)
                row[f"roi_{cls}_{form}_ms"] = median_ms(call, args.reps)
        print(json.dumps(row), flush=True)
        del enc, pix, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
