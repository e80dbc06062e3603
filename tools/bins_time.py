"""Times trpx_decode_bins next to trpx_decode_indexed of the whole stack, next to trpx_decode_dot with one all-ones map (the same
extraction with a multiply instead of the LDS add) and next to what a caller pays without it (the indexed decode, the stack
widened to int64, index_add_ over the unmasked pixels): HIP events, warm-up, median of 20, on the stacks of DESIGN.md section
4.17, the sums checked against the replaced route's first.

    python tools/bins_time.py [--reps 20] [--frames 2000] [--stacks synth,poisson] [--maps radial16,radial256,radial4096,ring,mod256]
                              [--forms index,offsets,free] [--large] [--no-baselines]

Maps: radialN -- N rings over the 512 x 512 frame, the corners masked; ring -- one ring of width 8 at radius 100, everything else
masked (few blocks are candidates); modN -- p % N (no two neighbours share a label: the merge never merges).
--large: eight 4096 x 4096 int32 frames, 256 rings (many spans per frame, the partial sums and k_bins_reduce) instead.
TRPX_LIB=tools/variants/libtrpx_binsnomerge.so (make -C trpx_amd/csrc binsnomerge) times the kernel with the merge compiled out.
One stack, one map and one form under a kernel trace shows the support / spans / reduce kernels alone (--no-baselines).
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

MASKED = 0xFFFF


def map_of(kind, side):
    """(labels uint16 [side * side], n_bins)"""
    p = np.arange(side * side)
    r = np.sqrt((p % side - side // 2) ** 2 + (p // side - side // 2) ** 2)
    if kind.startswith("radial"):
        nb = int(kind[6:])
        ring = np.floor(r * nb / (side // 2)).astype(np.int64)
        return np.where(ring < nb, ring, MASKED).astype(np.uint16), nb
    if kind == "ring":
        return np.where((r >= 100) & (r < 108), 0, MASKED).astype(np.uint16), 1
    nb = int(kind[3:])
    return (p % nb).astype(np.uint16), nb


def to_dev16(a):
    return torch.from_numpy(a.view(np.uint8)).cuda().view(torch.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--stacks", default="synth,poisson")
    ap.add_argument("--maps", default="radial16,radial256,radial4096,ring,mod256")
    ap.add_argument("--forms", default="index,offsets,free")
    ap.add_argument("--large", action="store_true", help="eight 4096 x 4096 int32 frames")
    ap.add_argument("--no-baselines", action="store_true", help="the bins calls alone (under a kernel trace)")
    args = ap.parse_args()
    side, n, tdt, ndt = (4096, 8, torch.int32, np.int32) if args.large else (512, args.frames, torch.uint16, np.uint16)
    v = side * side
    for name in (["synth"] if args.large else args.stacks.split(",")):
        px = codec.synth(ndt, 0, n, v) if name == "synth" else workloads.poisson_u16(3.0, 0, n, v)
        enc = codec.encode(px, index=True)
        enc.check()
        del px
        s, offs, idx = enc.stack(), enc.frame_offsets, enc.index
        pix = torch.empty((n, v), dtype=tdt, device="cuda")
        st = torch.empty(8, dtype=torch.int32, device="cuda")
        ws = codec.Workspace("cuda")
        ws.get(max(codec.decode_bins_workspace_bytes(s.numel(), v, n, ndt, 4096), codec.decode_dot_workspace_bytes(s.numel(), v, n, ndt, 1)))
        base = {"stack": name, "dtype": np.dtype(ndt).name, "frames": n, "values": v, "stream_bytes": s.numel(),
                "spans_per_frame": _lib.lib().trpx_decode_bins_spans_per_frame(v, n), "lib": os.environ.get("TRPX_LIB", "product")}
        if not args.no_baselines:
            base["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, v, n, tdt, out=pix, status=st, index=idx), args.reps)
            ones = torch.ones((1, v), dtype=torch.int32, device="cuda")
            dots = torch.empty((n, 1), dtype=torch.int64, device="cuda")
            base["dot_ones_index_ms"] = median_ms(
                lambda: codec.decode_dot(s, offs, v, n, tdt, ones, index=idx, out=dots, workspace=ws, status=st), args.reps)
            del ones, dots
        for kind in args.maps.split(","):
            lab, nb = map_of(kind, side)
            lab_dev = to_dev16(lab)
            keep = torch.from_numpy(np.flatnonzero(lab < nb)).cuda()
            where = torch.from_numpy(lab[lab < nb].astype(np.int64)).cuda()
            out = torch.empty((n, nb), dtype=torch.int64, device="cuda")
            row = dict(base, map=kind, n_bins=nb, unmasked=int(keep.numel()))

            def replaced():
                codec.decode(s, offs, v, n, tdt, out=pix, status=st, index=idx)
                return torch.zeros((n, nb), dtype=torch.int64, device="cuda").index_add_(1, where, pix.to(torch.int64)[:, keep])
            want = replaced()
            if not args.no_baselines:
                row["replaced_route_ms"] = median_ms(replaced, max(3, args.reps // 4), warm=1)
            for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                if form not in args.forms.split(","):
                    continue

                def call():
                    codec.decode_bins(s, o, v, n, tdt, lab_dev, nb, index=i, out=out, workspace=ws, status=st)
                out.fill_(-1)
                call()
                torch.cuda.synchronize()
                assert int(st[0].item()) == 0 and torch.equal(out, want), (name, kind, form)
                row[f"bins_{form}_ms"] = median_ms(call, args.reps)
            del want, keep, where
            print(json.dumps(row), flush=True)
        del enc, pix, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
