import sys
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from trpx_amd import codec, _lib, workloads
kind = sys.argv[1]
for n, frames in ((1030 * 1065, 5), (1300 * 1000, 3)):
    for data in ("poisson3", "synth"):
        px = workloads.poisson_u16(3.0, 0, frames, n, device="cuda") if data == "poisson3" else codec.synth(np.uint16, 3, frames, n, device="cuda")
        enc = codec.encode(px); torch.cuda.synchronize(); enc.check()
        back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, np.uint16)
        torch.cuda.synchronize()
        s = st.cpu().numpy()
        assert s[0] == 0 and torch.equal(back, px), (kind, data, n, s)
        if kind == "alldense": assert s[2] == frames, (kind, data, s)
        if kind == "segwgrounds": assert s[2] == (frames if data == "poisson3" else 0), (kind, data, s)
        if kind == "noclassify" and data == "synth": assert s[2] == 0, (kind, data, s)
        idx = codec.build_index(enc.stack(), enc.frame_offsets, n, frames, np.uint16)
        back2, st2 = codec.decode(enc.stack(), enc.frame_offsets, n, frames, np.uint16, index=idx)
        torch.cuda.synchronize()
        assert int(st2[0]) == 0 and torch.equal(back2, px), (kind, data, n)
print("OK")
