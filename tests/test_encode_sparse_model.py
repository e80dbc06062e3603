"""CPU tier: trpx_encode_sparse_bound_bytes against the oracle.  The bound is arithmetic on the event count alone (a block
without events costs 1 bit, 4 behind a block with events; a block with events at most 12 + 12 x bits(T); a pad byte per frame),
so it must hold for every placement and every value: oracle.encode_stack(dense).size <= bound <= the dense worst case."""
import numpy as np
import pytest

from trpx_amd import _lib

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32]
CODE = {np.dtype(np.uint8): _lib.U8, np.dtype(np.int8): _lib.I8, np.dtype(np.uint16): _lib.U16, np.dtype(np.int16): _lib.I16,
        np.dtype(np.uint32): _lib.U32, np.dtype(np.int32): _lib.I32}
N_FRAMES = 3


def _align16(x):
    return (x + 15) // 16 * 16


def _frames(dt, n_values, occupancy, seed):
    """N_FRAMES frames with events on `occupancy` of the pixels ("one": a single event in the stack): full-width values, the
    type's extremes (the minimum of signed types included) and small ones."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dt)
    px = np.zeros((N_FRAMES, n_values), dt)
    if occupancy == "one":
        px[rng.integers(N_FRAMES), rng.integers(n_values)] = info.min if info.min < 0 else info.max
        return px
    m = rng.random(px.shape) < occupancy
    vals = rng.integers(info.min, int(info.max) + 1, size=px.shape, dtype=np.int64)
    kind = rng.integers(0, 4, size=px.shape)
    vals = np.where(kind == 0, info.min if info.min < 0 else info.max, vals)
    vals = np.where(kind == 1, info.max, vals)
    vals = np.where(kind == 2, rng.integers(1, 4, size=px.shape), vals)
    px[m] = vals[m].astype(dt)
    return px


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n_values", [1, 11, 12, 13, 3071, 3072, 3073, 6149])
def test_bound_holds_and_stays_below_the_dense_worst_case(oracle, dt, n_values):
    L = _lib.lib()
    code = CODE[np.dtype(dt)]
    worst = N_FRAMES * L.trpx_worst_case_bytes(code, n_values, 12)
    for k, occupancy in enumerate((0.0, "one", 0.01, 1.0)):
        px = _frames(dt, n_values, occupancy, seed=1000 * n_values + k)
        n_events = int(np.count_nonzero(px))
        size = oracle.encode_stack(px)[0].size
        bound = L.trpx_encode_sparse_bound_bytes(code, n_values, N_FRAMES, n_events, 12)
        # (the bound is clamped to the worst case and THEN rounded up to 16, like the capacity trpx_encode's callers allocate: at
        # frames of a few values the rounding alone exceeds n_frames x worst_case, so that is the ceiling it is held to)
        assert bound % 16 == 0 and size <= bound <= _align16(worst), (np.dtype(dt).name, n_values, occupancy, n_events, size, bound, worst)
        if worst % 16 == 0:                                  # where the rounding cannot add anything the bound is the issue's own
            assert bound <= worst
        assert bound - worst < 16                            # ... and elsewhere the excess is the rounding alone
        # explicit zeros are events too: the bound of a longer list is no smaller
        assert L.trpx_encode_sparse_bound_bytes(code, n_values, N_FRAMES, n_events + 7, 12) >= bound
        if occupancy == 0.0:
            assert bound - size <= 16 * N_FRAMES            # an empty stack: tight


def test_bound_of_the_headline_empty_stack(oracle):
    """2000 empty 512 x 512 u16 frames: 21 846 one-bits and a pad byte each, and a bound within 16 bytes per frame of it."""
    L = _lib.lib()
    frame = oracle.encode_stack(np.zeros((1, 512 * 512), np.uint16))[0].size
    assert frame == 1 + 21846 // 8
    bound = L.trpx_encode_sparse_bound_bytes(_lib.U16, 512 * 512, 2000, 0, 12)
    assert 2000 * frame <= bound <= 2000 * (frame + 16)
    # at 1 % occupancy the bound is far below the dense worst case: that is what it is for
    events = 2000 * 512 * 512 // 100
    assert L.trpx_encode_sparse_bound_bytes(_lib.U16, 512 * 512, 2000, events, 12) < 2000 * L.trpx_worst_case_bytes(_lib.U16, 512 * 512, 12) // 5
