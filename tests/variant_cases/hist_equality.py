"""trpx_decode_hist on the library TRPX_LIB names (the histnoskip build: every block with a width is extracted, none is counted
from its width) against the histograms the product build left in the file argv[1] (tests/test_gpu_decode_hist.py writes it), on
the same seeded stacks: a skipped block and an extracted one must count alike."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trpx_amd import codec
import gpu_support as G

want = np.load(sys.argv[1])
n_calls = 0
for key in want.files:
    what, dtname, n, v, group, lo, shift, n_bins = key.split("|")
    n, v, group, lo, shift, n_bins = (int(x) for x in (n, v, group, lo, shift, n_bins))
    dt = np.dtype(dtname)
    px = G.mixed(dt, (n, v), seed=v, zero_stretch=True) if what == "mixed" else G.ladder(dt, (n, v), seed=v)
    enc = G.encode(px)
    hist, st = codec.decode_hist(enc.stack(), enc.frame_offsets, v, n, G.torch_dt(dt), n_bins, group=group, lo=lo, shift=shift, index=enc.index)
    torch.cuda.synchronize()
    assert int(st[0].item()) == 0, key
    got = hist.cpu().numpy()
    assert got.shape == want[key].shape and np.array_equal(got, want[key]), key
    assert int(got.sum()) == n * v, key
    n_calls += 1
assert n_calls >= 2
print("OK", n_calls)
