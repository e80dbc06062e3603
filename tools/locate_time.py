"""HIP-event timing of trpx_locate_frames (decode_locate.hip) on index-free stacks, alone, followed by trpx_decode with the
offsets it wrote, and -- for comparison -- trpx_decode with frame_offsets = NULL (its own serial walk, then the basic
kernels) with the time of that walk alone (k_walk_serial, the width-storing serial walk trpx_frame_offsets_host ran before
trpx_locate_frames existed: stage 0 of trpx_profile_read).  One JSON line per stack; offsets and pixels are checked against
the encoder's before anything is timed.

    python tools/locate_time.py [--reps R] [--stacks synth,poisson3,poisson3_big,int32_4k]

The locator walks the frames one after another: seconds per 2000-frame Poisson(3) stack.  Run it under a timeout."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(kind, dev):
    from trpx_amd import codec, workloads
    if kind == "synth":
        return codec.synth(np.uint16, 0, 2000, 512 * 512, device=dev), np.uint16, "2000 x 512^2 synth-v1 u16"
    if kind == "poisson3":
        return workloads.poisson_u16(3.0, 0, 2000, 512 * 512, device=dev), np.uint16, "2000 x 512^2 Poisson(3) u16"
    if kind == "poisson3_big":
        return workloads.poisson_u16(3.0, 0, 200, 1030 * 1065, device=dev), np.uint16, "200 x (1030 x 1065) Poisson(3) u16"
    if kind == "int32_4k":
        return codec.synth(np.int32, 0, 8, 4096 * 4096, device=dev), np.int32, "8 x 4096^2 synth-v1 int32"
    raise ValueError(kind)


def main():
    import torch
    from trpx_amd import _lib, codec
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stacks", default="synth,poisson3,poisson3_big,int32_4k")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    for kind in a.stacks.split(","):
        px, dt, label = make(kind, dev)
        frames, n = px.shape[0], px[0].numel()
        enc = codec.encode(px)
        torch.cuda.synchronize()
        enc.check()
        stack = enc.stack().clone()
        want = enc.frame_offsets.clone()
        del enc
        max_bits = 8 * np.dtype(dt).itemsize
        ws_l, ws_d = codec.Workspace(dev), codec.Workspace(dev)
        lb = L.trpx_locate_workspace_bytes(stack.numel(), n, frames, 12)
        ws = ws_l.get(lb)
        offs = torch.empty(frames + 1, dtype=torch.int64, device=dev)
        st = torch.empty(8, dtype=torch.int32, device=dev)
        back = torch.empty_like(px)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def locate():
            _lib.check(L.trpx_locate_frames(stack.data_ptr(), stack.numel(), n, frames, 12, max_bits, offs.data_ptr(),
                                            st.data_ptr(), ws.data_ptr(), ws.numel(), stream))

        def timed(fn, reps):
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            return float(np.median(ts)), float(min(ts))

        locate()
        torch.cuda.synchronize()
        assert int(st[0].item()) == 0 and torch.equal(offs, want), f"{label}: offsets differ from the encoder's"
        reps = a.reps
        loc_med, loc_min = timed(locate, reps)

        def both():
            locate()
            codec.decode(stack, offs, n, frames, dt, out=back, workspace=ws_d, status=st)
        both()
        torch.cuda.synchronize()
        assert int(st[0].item()) == 0 and torch.equal(back.view(torch.uint8), px.view(torch.uint8)), f"{label}: pixels differ"
        both_med, both_min = timed(both, reps)

        def walk_decode():
            codec.decode(stack, None, n, frames, dt, out=back, workspace=ws_d, status=st)
        walk_decode()
        torch.cuda.synchronize()
        assert int(st[0].item()) == 0 and torch.equal(back.view(torch.uint8), px.view(torch.uint8)), f"{label}: pixels differ"
        walk_med, _ = timed(walk_decode, reps)
        stage = (C.c_float * 16)()
        walk_ms = []
        for _ in range(reps):
            L.trpx_profile_enable(1)
            walk_decode()
            got = L.trpx_profile_read(stage, 16)
            L.trpx_profile_enable(0)
            assert got >= 1
            walk_ms.append(stage[0])
        assert int(st[0].item()) == 0
        print(json.dumps({"stack": label, "frames": frames, "n_values": n,
                          "stack_bytes": stack.numel(), "locate_ms": round(loc_med, 3), "locate_min_ms": round(loc_min, 3),
                          "locate_decode_ms": round(both_med, 3), "decode_no_offsets_ms": round(walk_med, 3),
                          "k_walk_serial_ms": round(float(np.median(walk_ms)), 3),
                          "frames_per_s_locate": round(frames / loc_med * 1e3), "workspace_bytes": lb}), flush=True)
        del px, back, stack, ws_l, ws_d, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
