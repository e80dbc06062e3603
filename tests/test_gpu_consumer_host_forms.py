"""GPU tests: the ten _host forms of the index consumers (trpx_decode_sum_host ... trpx_decode_sum_labelled_host), which share one
staged call (consumer_host, trpx_amd/csrc/api.hip): inputs and outputs as 16-byte aligned pieces of one device block.

The stack: 5 frames of 39 x 79 = 3081 pixels -- two tiles, a last block of 9 values, and no input whose byte size is a multiple
of 16 (maps of 2 x 3081 and 4 x 3081 bytes, 20 bytes of labels, 3 outputs, 3 maps, 37 bins), so a piece laid out unaligned, or
over its neighbour, shows --, once as uint16 and once as int8 (sparse values of one byte).  Every form is called through ctypes
with the frame offsets and with frame_offsets = NULL, into numpy buffers with one sentinel element in front of and behind every
output, and compared byte for byte with gpu_support.consumer_truths (plain torch in int64 on the original pixels) or, where that
has no entry (roi, hist, corrected), with the device-pointer call of trpx_amd.codec.  The list runs forward and then reversed in
one process: every call meets arena slots that a larger, differently laid out call left behind."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import ConsumerSpec, consumer_truths, encode, mixed, to_dev, to_np

pytestmark = pytest.mark.gpu

FRAMES, HEIGHT, WIDTH = 5, 39, 79
V = HEIGHT * WIDTH
GROUP, N_OUT, N_MAPS, N_BINS, BIN, BOX = 2, 3, 3, 37, (2, 3), (4, 5)
POISON = 0x5A


class Out:
    """A numpy output of `shape` and type `dt` with one sentinel element on either side, every byte POISON until written"""

    def __init__(self, shape, dt):
        self.n = int(np.prod(shape))
        self.whole = np.empty(self.n + 2, np.dtype(dt))
        self.whole.view(np.uint8)[:] = POISON
        self.ptr = self.whole.ctypes.data + self.whole.itemsize

    def bytes(self, what, count=None):
        """the output's bytes (of its first `count` elements), the sentinels checked"""
        raw = self.whole.view(np.uint8).reshape(self.n + 2, -1)
        assert (raw[0] == POISON).all() and (raw[-1] == POISON).all(), f"{what}: written outside the output"
        return self.whole[1:1 + (self.n if count is None else count)].tobytes()


def _case(dt):
    """The stack, what every consumer is asked, and every expected output as bytes -- once per pixel type"""
    import torch
    from trpx_amd import codec
    dt = np.dtype(dt)
    px = mixed(dt, (FRAMES, V), seed=20 + dt.itemsize)
    enc = encode(px)
    rng = np.random.default_rng(5)
    c = dict(dt=dt, stream=to_np(enc.stack()), offs=to_np(enc.frame_offsets).astype(np.uint64),
             threshold=100 if dt.kind == "u" else 50, shift=8 if dt.itemsize == 2 else 1, lo=0 if dt.kind == "u" else -128,
             frame_labels=np.array([1, 0, 0xFFFFFFFF, 1, 2], np.uint32),
             weights=rng.integers(-1000, 1001, size=(N_MAPS, V)).astype(np.int32),
             pixel_labels=rng.integers(0, N_BINS + 3, size=V).astype(np.uint16),        # (some pixels in no bin)
             boxes=np.array([[0, 0, 0], [4, HEIGHT - BOX[0], WIDTH - BOX[1]], [2, 10, 20]], np.uint32),
             dark=rng.random(V, np.float32) * 10, gain=rng.random(V, np.float32) + 0.5)
    lab = c["frame_labels"].astype(np.int64)
    spec = ConsumerSpec(GROUP, torch.from_numpy(np.where(lab < N_OUT, lab, -1)), N_OUT, torch.from_numpy(c["weights"].astype(np.int64)),
                        torch.from_numpy(c["pixel_labels"].astype(np.int64)), N_BINS, WIDTH, BIN, c["threshold"])
    t = {k: v.numpy() for k, v in consumer_truths(torch.from_numpy(px.astype(np.int64)), spec).items()}
    assert 0 < t["rows"][-1] < FRAMES * V and t["counts"].tolist() == [1, 2, 1]          # (events, but not everything; a masked frame)
    want = dict(sum=t["sum"], max=t["max"].astype(dt), sumsq=t["sumsq"].view(np.uint64), labelled=t["labelled"],
                counts=t["counts"].astype(np.uint32), dot=t["dot"], bins=t["bins"], binned=t["binned"],
                rows=t["rows"].astype(np.uint64), positions=t["positions"].astype(np.uint32), values=t["values"].astype(dt))
    # what the truths have no entry for: the device-pointer calls
    stack, offs, index = enc.stack(), enc.frame_offsets, enc.index
    dark, gain = to_dev(c["dark"]), to_dev(c["gain"])
    dev = dict(roi=codec.decode_roi(stack, offs, V, FRAMES, dt, WIDTH, to_dev(c["boxes"]), BOX, index=index),
               hist=codec.decode_hist(stack, offs, V, FRAMES, dt, N_BINS, group=GROUP, lo=c["lo"], shift=c["shift"], index=index))
    for d, g in ((True, True), (True, False), (False, True), (False, False)):
        dev[f"corrected{int(d)}{int(g)}"] = codec.decode_corrected(stack, offs, V, FRAMES, dt, dark if d else None, gain if g else None, index=index)
    torch.cuda.synchronize()
    for k, (got, status) in dev.items():
        assert int(status[0].item()) == 0, k
        want[k] = to_np(got)
    c["want"] = {k: np.ascontiguousarray(v).tobytes() for k, v in want.items()}
    c["total"] = int(t["rows"][-1])
    return c


def _calls(c):
    """[(name, run(offs pointer or None))]: every _host form once, and their optional arguments; run() asserts"""
    from trpx_amd import _lib
    from trpx_amd.terse import _code
    L = _lib.lib()
    dt, want, stream = c["dt"], c["want"], c["stream"]
    code, i64 = _code(dt), _code(np.int64, True)

    def front(o):
        return stream.ctypes.data, stream.size, o, V, FRAMES, 12

    def plain(name, key, shape, odt, call):
        def run(o):
            out = Out(shape, odt)
            _lib.check(call(o, out))
            assert out.bytes(name) == want[key], name
        return name, run

    def corrected(d, g):
        dark, gain = (c["dark"].ctypes.data if d else None), (c["gain"].ctypes.data if g else None)
        return plain(f"corrected dark={d} gain={g}", f"corrected{int(d)}{int(g)}", (FRAMES, V), np.float32,
                     lambda o, out: L.trpx_decode_corrected_host(code, _lib.F32, *front(o), dark, gain, out.ptr, -1))

    def labelled(with_counts):
        def run(o):
            sums, counts = Out((N_OUT, V), np.int64), Out(N_OUT, np.uint32)
            _lib.check(L.trpx_decode_sum_labelled_host(code, i64, *front(o), c["frame_labels"].ctypes.data, N_OUT, sums.ptr,
                                                       counts.ptr if with_counts else None, -1))
            assert sums.bytes("labelled sums") == want["labelled"]
            assert counts.bytes("labelled counts") == (want["counts"] if with_counts else bytes([POISON]) * 4 * N_OUT)
        return f"sum_labelled counts={with_counts}", run

    def sparse(capacity):
        """capacity None: the two-call protocol (sizes, then exactly as many); a number: one call with that capacity"""
        def call(o, rows, pos, val, cap, found):
            return L.trpx_decode_sparse_host(code, *front(o), c["threshold"], rows.ptr, pos and pos.ptr, val and val.ptr, cap, C.byref(found), -1)

        def run(o):
            total, found = c["total"], C.c_size_t(0)
            rows = Out(FRAMES + 1, np.uint64)
            if capacity is None:
                assert call(o, rows, None, None, 0, found) == _lib.ERR_CAPACITY and found.value == total    # (there are events)
                assert rows.bytes("sparse rows, sizes only") == want["rows"]
                rows = Out(FRAMES + 1, np.uint64)
            cap = total if capacity is None else capacity
            pos, val, found = Out(cap, np.uint32), Out(cap, dt), C.c_size_t(0)
            rc = call(o, rows, pos, val, cap, found)
            assert found.value == total and rows.bytes("sparse rows") == want["rows"]
            if cap < total:
                assert rc == _lib.ERR_CAPACITY
                pos.bytes("sparse positions"), val.bytes("sparse values")                                   # (the sentinels)
            else:
                _lib.check(rc)
                assert pos.bytes("sparse positions", total) == want["positions"] and val.bytes("sparse values", total) == want["values"]
        return f"sparse capacity={capacity}", run

    n_groups, oh, ow = -(-FRAMES // GROUP), -(-HEIGHT // BIN[0]), -(-WIDTH // BIN[1])
    return [
        plain("sum", "sum", (n_groups, V), np.int64, lambda o, out: L.trpx_decode_sum_host(code, i64, *front(o), GROUP, out.ptr, -1)),
        plain("roi", "roi", (len(c["boxes"]), *BOX), dt,
              lambda o, out: L.trpx_decode_roi_host(code, *front(o), WIDTH, c["boxes"].ctypes.data, len(c["boxes"]), *BOX, out.ptr, -1)),
        sparse(None), sparse(c["total"] - 1), sparse(c["total"] + 7),
        plain("dot", "dot", (FRAMES, N_MAPS), np.int64,
              lambda o, out: L.trpx_decode_dot_host(code, *front(o), c["weights"].ctypes.data, N_MAPS, out.ptr, -1)),
        plain("bins", "bins", (FRAMES, N_BINS), np.int64,
              lambda o, out: L.trpx_decode_bins_host(code, *front(o), c["pixel_labels"].ctypes.data, N_BINS, out.ptr, -1)),
        plain("hist", "hist", (n_groups, N_BINS), np.uint64,
              lambda o, out: L.trpx_decode_hist_host(code, *front(o), GROUP, c["lo"], c["shift"], N_BINS, out.ptr, -1)),
        corrected(True, True), corrected(True, False), corrected(False, True), corrected(False, False),
        plain("binned", "binned", (FRAMES, oh, ow), np.int64, lambda o, out: L.trpx_decode_binned_host(code, i64, *front(o), WIDTH, *BIN, out.ptr, -1)),
        plain("reduce max", "max", (n_groups, V), dt, lambda o, out: L.trpx_decode_reduce_host(code, _lib.REDUCE_MAX, *front(o), GROUP, 0, out.ptr, -1)),
        plain("reduce sumsq", "sumsq", (n_groups, V), np.uint64,
              lambda o, out: L.trpx_decode_reduce_host(code, _lib.REDUCE_SUMSQ, *front(o), GROUP, 0, out.ptr, -1)),
        labelled(True), labelled(False),
    ]


@pytest.mark.parametrize("dt", [np.uint16, np.int8], ids=lambda d: np.dtype(d).name)
def test_every_host_form_with_and_without_offsets_forward_and_reversed(dt):
    c = _case(dt)
    calls = _calls(c)
    for order in (calls, calls[::-1]):
        for name, run in order:
            for offs in (c["offs"].ctypes.data, None):
                try:
                    run(offs)
                except Exception as e:                      # (an assertion or a TrpxError: say which call it was)
                    raise AssertionError(f"{name}, {'offsets' if offs else 'no offsets'}, {'forward' if order is calls else 'reversed'}: {e}") from e
