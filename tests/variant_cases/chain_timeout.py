import sys
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from trpx_amd import codec, _lib, workloads
n, frames = 1030 * 1065, 6
for kind in ("poisson3", "synth"):
    px = workloads.poisson_u16(3.0, 0, frames, n, device="cuda") if kind == "poisson3" else codec.synth(np.uint16, 3, frames, n, device="cuda")
    enc = codec.encode(px); torch.cuda.synchronize(); enc.check()
    P = _lib.lib().trpx_decode_parts_per_frame(codec.dtype_code(np.uint16), n, frames, 12)
    assert P > 8, P
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, np.uint16)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    assert s[0] == 0 and torch.equal(back, px), (kind, s)
    assert 2 <= s[2] <= 3, (kind, s)          # frames 0 and 1 (and no others but by the data's own doing)
    idx = codec.build_index(enc.stack(), enc.frame_offsets, n, frames, np.uint16)
    back2, st2 = codec.decode(enc.stack(), enc.frame_offsets, n, frames, np.uint16, index=idx)
    torch.cuda.synchronize()
    assert int(st2[0]) == 0 and torch.equal(back2, px), kind
print("OK")
