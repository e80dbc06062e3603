import sys, ctypes as C
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from trpx_amd import codec, _lib
from oracle import oracle as O
L = _lib.lib()
frames, n = 40, 512 * 512
px = codec.synth(np.uint16, 0, frames, n)
want, sizes, pb = O.encode_stack(px.cpu().numpy())
enc = codec.encode(px)
torch.cuda.synchronize()
assert int(enc.status[0]) == _lib.ERR_TIMEOUT, int(enc.status[0])       # the forced failure is really there
enc.check()                                                              # re-runs through trpx_encode_checked
assert int(enc.status[0]) == 0 and enc.prolix_bits() == pb
assert enc.stack().cpu().numpy().tobytes() == want.tobytes()
host = np.zeros(8, np.uint32)
ws = codec.Workspace("cuda")
enc2 = codec.encode(px, workspace=ws)
torch.cuda.synchronize()
w = ws.buf
rc = L.trpx_encode_checked(_lib.U16, px.data_ptr(), n, frames, 12, enc2.data.data_ptr(), enc2.data.numel(), enc2.frame_offsets.data_ptr(),
                           enc2.status.data_ptr(), None, w.data_ptr(), w.numel(), None, host.ctypes.data)
assert rc == 0 and host[0] == 0 and host[1] == pb and enc2.stack().cpu().numpy().tobytes() == want.tobytes()
out = np.zeros(want.size + 64, np.uint8); total = C.c_size_t(0); gpb = C.c_uint(0); offs = np.zeros(frames + 1, np.uint64)
hp = px.cpu().numpy()
_lib.check(L.trpx_encode_host(_lib.U16, hp.ctypes.data, n, frames, 12, out.ctypes.data, out.size, C.byref(total), offs.ctypes.data, C.byref(gpb), -1))
assert total.value == want.size and (out[: want.size] == want).all() and gpb.value == pb
print("OK")
