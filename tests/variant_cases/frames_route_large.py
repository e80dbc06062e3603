import sys, numpy as np, torch
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from trpx_amd import codec
px = codec.synth(np.int32, 5, 130, 1500 * 1500)
enc = codec.encode(px); torch.cuda.synchronize(); enc.check()
back, st = codec.decode(enc.stack(), enc.frame_offsets, 1500 * 1500, 130, np.int32); torch.cuda.synchronize()
assert int(st[0].item()) == 0 and torch.equal(back, px)
print('OK')
