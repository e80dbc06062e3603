"""HIP-event timing of trpx_locate_frames (decode_locate.hip) on index-free stacks: the auto route (position-parallel) and the
serial route (trpx_set_locate_path(1), one timed call) side by side on the same stack, then the auto route followed by
trpx_decode with the offsets it wrote, trpx_decode with frame_offsets = NULL (which locates the same way, then takes the
tuned routes), and that call on the serial route (its own serial walk, then the basic kernels; one timed call).  One JSON
line per stack; offsets and pixels are checked against the encoder's before anything is timed.

    python tools/locate_time.py [--reps R] [--stacks synth,poisson3,poisson3_big,int32_4k]

The serial route and trpx_decode(frame_offsets = NULL) take seconds per 2000-frame Poisson(3) stack.  Run it under a timeout."""
import argparse
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
        L.trpx_set_locate_path(1)                              # the serial route on the same stack, same process
        try:
            locate()
            torch.cuda.synchronize()
            assert int(st[0].item()) == 0 and torch.equal(offs, want), f"{label}: serial offsets differ from the encoder's"
            ser_med, _ = timed(locate, 1)
        finally:
            L.trpx_set_locate_path(0)

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
        L.trpx_set_locate_path(1)                              # trpx_decode(NULL) as before the parallel locator: its serial walk
        try:
            ser_dec_med, _ = timed(walk_decode, 1)
        finally:
            L.trpx_set_locate_path(0)
        assert int(st[0].item()) == 0
        print(json.dumps({"stack": label, "frames": frames, "n_values": n,
                          "stack_bytes": stack.numel(), "locate_ms": round(loc_med, 3), "locate_min_ms": round(loc_min, 3),
                          "locate_serial_ms": round(ser_med, 3), "speedup": round(ser_med / loc_med, 1),
                          "locate_decode_ms": round(both_med, 3), "decode_no_offsets_ms": round(walk_med, 3),
                          "decode_no_offsets_serial_ms": round(ser_dec_med, 3),
                          "frames_per_s_locate": round(frames / loc_med * 1e3), "workspace_bytes": lb}), flush=True)
        del px, back, stack, ws_l, ws_d, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
