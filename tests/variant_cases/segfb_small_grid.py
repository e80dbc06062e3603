import sys
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from trpx_amd import codec, _lib, workloads
for route in (0, 2, 4):
    _lib.lib().trpx_set_decode_path(route)
    for n, frames in ((1030 * 1065, 5), (2048 * 520, 3)):
        px = workloads.poisson_u16(3.0, 0, frames, n, device="cuda")
        enc = codec.encode(px); torch.cuda.synchronize(); enc.check()
        back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, np.uint16)
        torch.cuda.synchronize()
        assert int(st[0]) == 0 and torch.equal(back.view(torch.int16), px.view(torch.int16)), (route, n, frames, st.tolist())
print("OK")
