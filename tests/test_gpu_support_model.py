"""CPU tier: tests/gpu_support.py can fail.  The transfer helpers round-trip every supported type byte for byte on CPU tensors,
a guarded output's check passes untouched and fails for one byte changed just in front of the view, just behind it and -- for
a null or short-capacity call -- at the stated element, and the data sets hold what the GPU tests rely on."""
import numpy as np
import pytest
import torch

from gpu_support import DTYPE_NAMES, GUARD, Guarded, input_forms, ladder, ladder_holds_every_width, mixed, status_block
from gpu_support import to_dev, to_np, torch_dt

CPU = "cpu"
INTS = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32]
N = 41                                                       # elements of the guarded views
SENTINELS = {"uint8": 0xA5, "int8": 0x5A, "uint16": 0x5A, "int16": 0x5A, "uint32": 0x5A5A5A5A, "int32": 0x5A,
             "int64": 0x5A5A5A5A5A5A5A5A}                    # the ones the GPU tests name, per type


@pytest.mark.parametrize("name", DTYPE_NAMES)
def test_transfer_round_trips_byte_for_byte(name):
    dt = np.dtype(name)
    raw = np.random.default_rng(3).integers(0, 256, size=3 * 5 * 7 * dt.itemsize, dtype=np.uint8)
    raw[: 2 * dt.itemsize] = 0xFF                            # the all-ones pattern: -1, the unsigned maximum, a NaN
    a = raw.view(dt).reshape(3, 5, 7)
    a.setflags(write=False)                                  # (shared cases are read-only: to_dev copies)
    t = to_dev(a, CPU)
    assert t.dtype == torch_dt(dt) and tuple(t.shape) == a.shape and t.device.type == "cpu"
    assert t.data_ptr() != a.ctypes.data
    back = to_np(t)
    assert back.dtype == dt and back.shape == a.shape and back.tobytes() == a.tobytes()
    part = to_np(t[1:, ::2])                                 # a view that is not contiguous
    assert part.dtype == dt and part.tobytes() == np.ascontiguousarray(a[1:, ::2]).tobytes()
    w = a.copy()                                             # a writable array is not copied on the host first, yet never aliased
    tw = to_dev(w, CPU)
    tw.view(torch.uint8).zero_()
    assert w.tobytes() == a.tobytes() and not to_np(tw).tobytes().strip(b"\0")
    empty = to_np(to_dev(np.zeros(0, dt), CPU))
    assert empty.dtype == dt and empty.shape == (0,)


def _byte(g, element):
    """(uint8 view of the whole allocation, position of the first byte of `element`, counted from the view's start)"""
    raw = g.whole.view(torch.uint8)
    return raw, (GUARD + element) * g.whole.element_size()


@pytest.mark.parametrize("name", sorted(SENTINELS))
def test_guarded_check_passes_untouched_and_fails_for_one_byte(name):
    dt, sentinel = np.dtype(name), SENTINELS[name]
    g = Guarded(N, dt, sentinel, CPU)
    assert g.view.dtype == torch_dt(dt) and g.view.numel() == N and g.whole.numel() == N + 2 * GUARD
    assert g.view.data_ptr() - g.whole.data_ptr() == GUARD * dt.itemsize
    assert (to_np(g.whole) == np.full(N + 2 * GUARD, sentinel, dt)).all()
    got = g.check("untouched", untouched_from=0)
    assert got.dtype == dt and got.shape == (N,) and (got == sentinel).all()
    g.view.copy_(to_dev(np.arange(N).astype(dt), CPU))       # "the call": writes the whole view, nothing else
    assert (g.check("written") == np.arange(N).astype(dt)).all()
    g.check("written up to N", untouched_from=N)
    raw, _ = _byte(g, 0)
    for what, pos in (("the byte in front of the view", _byte(g, 0)[1] - 1), ("the byte behind the view", _byte(g, N)[1]),
                      ("the first byte of the allocation", 0), ("the last byte of the allocation", raw.numel() - 1)):
        old = int(raw[pos])
        raw[pos] = old ^ 1
        with pytest.raises(AssertionError, match="written outside it"):
            g.check("it")
        raw[pos] = old
        g.check(what)


@pytest.mark.parametrize("name", sorted(SENTINELS))
def test_guarded_check_fails_for_one_byte_at_or_beyond_the_capacity(name):
    """A call given a capacity of k elements (k = 0: a null output) may write elements [0, k) of the view only."""
    dt = np.dtype(name)
    for k in (0, 7, N - 1):
        g = Guarded(N, dt, SENTINELS[name], CPU)
        raw, _ = _byte(g, 0)
        g.view[:k] = 1                                       # what the call may write
        g.check("out", untouched_from=k)
        for element in (k, N - 1):
            pos = _byte(g, element)[1] + dt.itemsize - 1     # the last byte of that element
            old = int(raw[pos])
            raw[pos] = old ^ 0x80
            g.check("out")                                   # inside the view: the guards alone do not see it
            with pytest.raises(AssertionError, match=f"out written at or behind element {k}"):
                g.check("out", untouched_from=k)
            raw[pos] = old
            g.check("out", untouched_from=k)


def test_status_block_and_input_forms():
    st = status_block(CPU)
    assert st.dtype == torch.int32 and st.tolist() == [77] * 8

    class Enc:
        frame_offsets, index = torch.arange(6), torch.zeros(3)
    offs, index = input_forms(Enc, "index")
    assert offs.data_ptr() == Enc.frame_offsets.data_ptr() and offs.numel() == 6 and index is Enc.index
    offs, index = input_forms(Enc, "offsets", first=2)
    assert offs.tolist() == [2, 3, 4, 5] and index is None
    assert input_forms(Enc, "none", first=2) == (None, None)
    with pytest.raises(AssertionError):
        input_forms(Enc, "both")


@pytest.mark.parametrize("dt", INTS, ids=lambda d: np.dtype(d).name)
def test_ladder_holds_every_width_at_three_turns(dt):
    px = ladder(dt, (3, 12 * 3 * 33), seed=5)
    assert px.dtype == dt and px.shape == (3, 12 * 3 * 33)
    ladder_holds_every_width(px)
    info = np.iinfo(dt)
    top = [0 if w == 0 else (1 << (w - (info.min < 0))) - 1 for w in range(info.bits + 1)]
    blocks = np.abs(px.astype(np.int64)).reshape(3, -1, 12).max(axis=2)
    assert blocks[0, : info.bits + 1].tolist() == top        # frame 0: block b is exactly b bits wide
    flat = px.copy()
    flat[px == info.max] = 0                                 # without the full-width blocks' top value the fixture check fails
    with pytest.raises(AssertionError):
        ladder_holds_every_width(flat)


@pytest.mark.parametrize("dt", INTS, ids=lambda d: np.dtype(d).name)
def test_mixed_with_a_zero_stretch_is_mixed_with_the_stretch_zeroed(dt):
    for shape in ((2, 7), (4, 1073), (3, 7000)):
        n, v = shape
        plain, stretch = mixed(dt, shape, 17), mixed(dt, shape, 17, zero_stretch=True)
        want = plain.copy()
        want[:, v // 2: v // 2 + v // 7] = 0
        assert stretch.dtype == plain.dtype == dt and stretch.tobytes() == want.tobytes()
        if v // 7:
            assert plain[:, v // 2: v // 2 + v // 7].any()
    cube = mixed(dt, (3, 70, 100), 17)                       # [frames, h, w]: the same values, reshaped
    assert cube.shape == (3, 70, 100) and cube.tobytes() == mixed(dt, (3, 7000), 17).tobytes()


@pytest.mark.parametrize("dt", [np.uint8, np.int32], ids=lambda d: np.dtype(d).name)
def test_the_generators_are_deterministic_in_their_seed(dt):
    shape = (3, 1200)
    for gen in (mixed, ladder):
        assert gen(dt, shape, 9).tobytes() == gen(dt, shape, 9).tobytes()
        assert gen(dt, shape, 9).tobytes() != gen(dt, shape, 10).tobytes()
