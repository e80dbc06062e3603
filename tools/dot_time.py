"""Times trpx_decode_dot next to trpx_decode_indexed of the whole stack and next to what a caller pays without it (the indexed
decode, the stack widened to int64, per map a multiply and a row sum -- torch has no integer matmul on the GPU): HIP events,
warm-up, median of 20, on the stacks of DESIGN.md section 4.15, the sums checked against the replaced route's first.

    python tools/dot_time.py [--reps 20] [--frames 2000] [--stacks synth,poisson] [--maps 1,3,16] [--kinds disc,ones,disc+xy]
                             [--forms index,offsets,free]

Map kinds: disc -- every map a multiple of a disc of radius 32 (few blocks are candidates); ones -- every map a multiple of the
all-ones map (every non-zero block is a candidate); disc+xy (three maps) -- the disc and the coordinate maps x, y.
One stack, one kind and one form under a kernel trace shows the support / runs / reduce kernels alone (--no-baselines).
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

SIDE = 512
V = SIDE * SIDE


def maps_of(kind, k):
    p = np.arange(V)
    disc = (((p % SIDE - SIDE // 2) ** 2 + (p // SIDE - SIDE // 2) ** 2) <= 32 * 32).astype(np.int32)
    if kind == "disc+xy":
        return np.stack([disc, (p % SIDE).astype(np.int32), (p // SIDE).astype(np.int32)])
    one = disc if kind == "disc" else np.ones(V, np.int32)
    return np.stack([one * (i + 1) for i in range(k)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--stacks", default="synth,poisson")
    ap.add_argument("--maps", default="1,3,16")
    ap.add_argument("--kinds", default="disc,ones,disc+xy")
    ap.add_argument("--forms", default="index,offsets,free")
    ap.add_argument("--no-baselines", action="store_true", help="the dot calls alone (under a kernel trace)")
    args = ap.parse_args()
    n = args.frames
    for name in args.stacks.split(","):
        px = codec.synth(np.uint16, 0, n, V) if name == "synth" else workloads.poisson_u16(3.0, 0, n, V)
        enc = codec.encode(px, index=True)
        enc.check()
        del px
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        pix = torch.empty((n, V), dtype=torch.uint16, device="cuda")
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        ws = codec.Workspace("cuda")
        ws.get(codec.decode_dot_workspace_bytes(s.numel(), V, n, np.uint16, 16))
        base = {"stack": name, "frames": n, "values": V, "stream_bytes": s.numel()}
        if not args.no_baselines:
            base["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, V, n, torch.uint16, out=pix, status=st, index=idx), args.reps)
        for kind in args.kinds.split(","):
            for k in ([3] if kind == "disc+xy" else [int(x) for x in args.maps.split(",")]):
                w = torch.from_numpy(maps_of(kind, k)).cuda()
                w64 = w.to(torch.int64)
                out = torch.empty((n, k), dtype=torch.int64, device="cuda")
                row = dict(base, maps=kind, n_maps=k)

                def replaced():
                    codec.decode(s, offs, V, n, torch.uint16, out=pix, status=st, index=idx)
                    p64 = pix.to(torch.int64)
                    return torch.stack([(p64 * w64[i]).sum(-1) for i in range(k)], dim=1)
                want = replaced()
                if not args.no_baselines:
                    row["replaced_route_ms"] = median_ms(replaced, max(3, args.reps // 4), warm=1)
                for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                    if form not in args.forms.split(","):
                        continue

                    def call():
                        codec.decode_dot(s, o, V, n, torch.uint16, w, index=i, out=out, workspace=ws, status=st)
                    out.zero_()
                    call()
                    torch.cuda.synchronize()
                    assert int(st[0].item()) == 0 and torch.equal(out, want), (name, kind, k, form)
                    row[f"dot_{form}_ms"] = median_ms(call, args.reps)
                del want, w64
                print(json.dumps(row), flush=True)
        del enc, pix, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
