"""Times trpx_decode_hist next to trpx_decode_indexed of the whole stack, next to trpx_decode_bins with the p % 256 map (the same
walk with twelve label loads and a support kernel) and next to what a caller pays without it (the indexed decode, widen, shift,
clamp, offset by group, torch.bincount): HIP events, warm-up, median of 20, on the stacks of DESIGN.md section 4.21, the
histograms checked against the replaced route's first.

    python tools/hist_time.py [--reps 20] [--frames 2000] [--stacks synth,poisson] [--rules frame256,stack4096,wide16]
                              [--forms index,offsets,free] [--large] [--no-baselines]

Rules: frame256 -- per-frame histograms of 256 unit bins from 0; stack4096 -- the stack's histogram (one group) of 4096 unit
bins; wide16 -- per frame, 16 bins of 16 counts (on Poisson(3) nearly every block lies in one bin and is counted from its width).
--large: eight 4096 x 4096 int32 frames, 256 unit bins, group 1 and 8 (many spans a group, the partial counts and k_reduce_parts)
instead.
TRPX_LIB=tools/variants/libtrpx_histnoskip.so (make -C trpx_amd/csrc histnoskip) times the kernel that extracts every block with
a width: the difference is what the one-bin skip buys.  One stack, one rule and one form under a kernel trace shows the spans /
reduce kernels alone (--no-baselines).
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


def rule_of(kind, n):
    """(group, lo, shift, n_bins)"""
    return {"frame256": (1, 0, 0, 256), "stack4096": (n, 0, 0, 4096), "wide16": (1, 0, 4, 16), "large1": (1, 0, 0, 256), "large8": (n, 0, 0, 256)}[kind]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--stacks", default="synth,poisson")
    ap.add_argument("--rules", default="frame256,stack4096,wide16")
    ap.add_argument("--forms", default="index,offsets,free")
    ap.add_argument("--large", action="store_true", help="eight 4096 x 4096 int32 frames")
    ap.add_argument("--no-baselines", action="store_true", help="the hist calls alone (under a kernel trace)")
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
        ws.get(max(codec.decode_hist_workspace_bytes(s.numel(), v, n, ndt, 4096, group=g) for g in (1, n))
               + codec.decode_bins_workspace_bytes(s.numel(), v, n, ndt, 256))
        base = {"stack": name, "dtype": np.dtype(ndt).name, "frames": n, "values": v, "stream_bytes": s.numel(),
                "lib": os.environ.get("TRPX_LIB", "product")}
        if not args.no_baselines:
            base["decode_indexed_ms"] = median_ms(lambda: codec.decode(s, offs, v, n, tdt, out=pix, status=st, index=idx), args.reps)
            lab = torch.from_numpy((np.arange(v) % 256).astype(np.int16)).cuda()                 # (labels < 2^15: the int16 view of uint16)
            sums = torch.empty((n, 256), dtype=torch.int64, device="cuda")
            base["bins_mod256_index_ms"] = median_ms(
                lambda: codec.decode_bins(s, offs, v, n, tdt, lab, 256, index=idx, out=sums, workspace=ws, status=st), args.reps)
            del lab, sums
        for kind in (["large1", "large8"] if args.large else args.rules.split(",")):
            group, lo, shift, nb = rule_of(kind, n)
            n_groups = -(-n // group)
            out = torch.empty((n_groups, nb), dtype=torch.int64, device="cuda")
            row = dict(base, rule=kind, group=group, lo=lo, shift=shift, n_bins=nb,
                       spans_per_group=_lib.lib().trpx_decode_hist_spans_per_group(v, n, group))
            group_base = (torch.arange(n, dtype=torch.int64, device="cuda") // group * nb)[:, None]

            def replaced():
                codec.decode(s, offs, v, n, tdt, out=pix, status=st, index=idx)
                want = torch.zeros(n_groups * nb, dtype=torch.int64, device="cuda")
                step = max(1, (1 << 27) // v)                                       # (the int64 copy a chunk of frames at a time: 1 GB)
                for f0 in range(0, n, step):
                    b = ((pix[f0: f0 + step].to(torch.int64) - lo) >> shift).clamp_(0, nb - 1)
                    b += group_base[f0: f0 + step]
                    want += torch.bincount(b.view(-1), minlength=n_groups * nb)
                return want.view(n_groups, nb)
            want = replaced()
            if not args.no_baselines:
                row["replaced_route_ms"] = median_ms(replaced, max(3, args.reps // 4), warm=1)
            for form, (o, i) in {"index": (offs, idx), "offsets": (offs, None), "free": (None, None)}.items():
                if form not in args.forms.split(","):
                    continue

                def call():
                    codec.decode_hist(s, o, v, n, tdt, nb, group=group, lo=lo, shift=shift, index=i, out=out, workspace=ws, status=st)
                out.fill_(-1)
                call()
                torch.cuda.synchronize()
                assert int(st[0].item()) == 0 and torch.equal(out, want), (name, kind, form)
                row[f"hist_{form}_ms"] = median_ms(call, args.reps)
            del want
            print(json.dumps(row), flush=True)
        del enc, pix, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
