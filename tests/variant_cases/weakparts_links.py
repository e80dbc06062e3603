import sys
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from trpx_amd import codec, _lib
rng = np.random.RandomState(5)
for dtype, n, frames in ((np.uint16, 1030 * 1065, 12), (np.int32, 2048 * 2048 + 5, 2)):
    a = rng.randint(0, 8, (frames, n)).astype(dtype)
    a[:, 0::192] = 9                                      # every 16th block is 4 bits wide
    if np.dtype(dtype).kind == "i":
        a[:, 1::384] = -9
    px = torch.from_numpy(a).cuda()
    enc = codec.encode(px); torch.cuda.synchronize(); enc.check()
    # the index route (default): no cut finds a run, no part warms up in this build -- every link between two parts is open and
    # repaired, and every repaired part's entries are spliced from the repair's and its own walk's (none is walked again)
    P = _lib.lib().trpx_decode_parts_per_frame(codec.dtype_code(dtype), n, frames, 12)
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dtype)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    assert s[0] == 0 and torch.equal(back, px), s
    # (a part of ~1000 blocks on a chain that has not merged with the frame's by its end leaves the NEXT repair a false start:
    # such a frame -- a few of them here, none with real cuts, which warm up -- is listed for the other route and still exact)
    assert P > 3 and s[4] == 0 and s[5] + s[6] == frames * (P - 2) and s[5] > 9 * s[6] and s[2] <= frames, (P, s)
    # round 4's parts route: plain guesses == repaired links; no fallback, no failed repair
    assert _lib.lib().trpx_set_decode_path(4) == 0
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dtype)
    torch.cuda.synchronize()
    _lib.lib().trpx_set_decode_path(0)
    s = st.cpu().numpy()
    assert s[0] == 0 and torch.equal(back, px), s
    assert s[2] == 0 and s[3] > 0 and s[5] == s[3] and s[6] == 0, s
print("OK")
