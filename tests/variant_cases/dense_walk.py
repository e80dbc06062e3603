import sys
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from trpx_amd import codec, _lib, workloads
_lib.lib().trpx_set_decode_path(5)
want_serial = sys.argv[1] == "all"
rng = np.random.RandomState(11)
total = 0
hits = []
for dtype, n, frames in ((np.uint16, 512 * 512, 9), (np.int8, 3000, 140), (np.uint16, 3000, 140), (np.int32, 40000, 6), (np.uint8, 12 * 300 + 7, 130)):
    dt = np.dtype(dtype)
    if dtype == np.uint16 and n == 512 * 512:
        px = workloads.poisson_u16(3.0, 0, frames, n, device="cuda")
    else:
        nblk = (n + 11) // 12
        top = 8 * dt.itemsize - (1 if dt.kind == "i" else 0)
        hi = rng.choice([0, 1, 2, 3, 5, min(9, top), top], size=(frames, nblk), p=[0.1, 0.2, 0.3, 0.2, 0.1, 0.07, 0.03])
        mag = (rng.rand(frames, nblk * 12) * (2.0 ** np.repeat(hi, 12, axis=1))).astype(np.int64)[:, :n]
        if dt.kind == "i":
            mag = np.clip(mag * rng.choice([-1, 1], size=mag.shape), np.iinfo(dt).min, np.iinfo(dt).max)
        px = torch.from_numpy(mag.astype(dt)).cuda()
    enc = codec.encode(px, index=True); torch.cuda.synchronize(); enc.check()
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dtype)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    assert s[0] == 0 and torch.equal(back.view(torch.uint8), px.view(torch.uint8)), (dtype, n, frames, s)
    walked = codec.build_index(enc.stack(), enc.frame_offsets, n, frames, dtype)
    nb = (n + 11) // 12; ng = (nb + 255) // 256; w_off = (8 * frames * ng + 15) // 16 * 16
    assert torch.equal(enc.index[: 8 * frames * ng], walked[: 8 * frames * ng]) and torch.equal(enc.index[w_off: w_off + frames * nb], walked[w_off: w_off + frames * nb]), (dtype, n, frames)
    total += int(s[2])
    hits.append(int(s[2]))
assert not want_serial or (total > 0 and sum(1 for h in hits if h > 0) >= 3), hits     # (every LISTED frame of the serial build; which frames are listed is the per-frame decoder's call)
print("OK", total)
