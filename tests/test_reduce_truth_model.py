"""CPU tier: the truths of tests/reduce_truth.py on hand-written arrays, each against numbers worked out by hand -- and each check
shown to fail on a wrong answer, so that the GPU tier's comparisons mean something."""
import numpy as np
import pytest

import reduce_truth as R

PX = np.array([[1, -2, 0, 7],
               [3, -5, 0, 7],
               [-4, -1, 0, 6],
               [2, -9, 5, -128],
               [0, 0, 0, 127]], np.int8)


def test_groups_and_the_short_last_group():
    assert R.max_truth(PX, 2).tolist() == [[3, -2, 0, 7], [2, -1, 5, 6], [0, 0, 0, 127]]
    assert R.min_truth(PX, 2).tolist() == [[1, -5, 0, 7], [-4, -9, 0, -128], [0, 0, 0, 127]]
    assert R.max_truth(PX, 5).tolist() == [[3, 0, 5, 127]] == R.max_truth(PX, 9).tolist()      # a group beyond the stack
    assert R.min_truth(PX, 1).tolist() == PX.tolist()
    assert R.max_truth(PX, 2).dtype == np.int8 and R.min_truth(PX, 2).dtype == np.int8
    assert R.max_truth(PX, 2).tolist() != R.max_truth(PX, 3).tolist()                            # (the group matters)


def test_blank_frame_takes_part():
    neg = np.array([[-3, -1], [-7, -2]], np.int16)
    assert R.max_truth(neg, 2).tolist() == [[-3, -1]]
    with_blank = np.vstack([neg, np.zeros((1, 2), np.int16)])
    assert R.max_truth(with_blank, 3).tolist() == [[0, 0]]
    pos = np.array([[3, 1], [7, 2]], np.uint16)
    assert R.min_truth(pos, 2).tolist() == [[3, 1]]
    assert R.min_truth(np.vstack([pos, np.zeros((1, 2), np.uint16)]), 3).tolist() == [[0, 0]]


def test_sumsq_small_and_exact():
    got = R.sumsq_truth(PX, 2)
    assert got.dtype == np.uint64
    assert got.tolist() == [[10, 29, 0, 98], [20, 82, 25, 36 + 16384], [0, 0, 0, 16129]]
    assert got.tolist() == R.sumsq_exact(PX, 2)
    assert R.sumsq_truth(PX, 5).tolist() == [[30, 111, 25, 98 + 36 + 16384 + 16129]]


@pytest.mark.parametrize("dt", [np.uint32, np.int32])
def test_sumsq_wraps_modulo_2_64(dt):
    info = np.iinfo(dt)
    px = np.array([[info.max, info.min, 5]] * 5, dt)
    got = R.sumsq_truth(px, 5)
    exact = R.sumsq_exact(px, 5)
    assert [int(v) for v in got[0]] == [e % (1 << 64) for e in exact[0]]
    big = max(abs(int(info.max)), abs(int(info.min)))
    assert 5 * big * big >= 1 << 64 and int(got[0][0 if dt == np.uint32 else 1]) != 5 * big * big    # it did wrap
    assert int(got[0][2]) == 125
    if dt == np.int32:
        assert int(R.sumsq_truth(px[:1], 1)[0][1]) == 1 << 62                                          # INT32_MIN squared


def test_count_and_thresholds_beyond_the_type():
    assert R.count_truth(PX, 2, 0).tolist() == [[2, 0, 2, 2], [1, 0, 2, 1], [1, 1, 1, 1]]
    assert R.count_truth(PX, 2, 1).tolist() == [[2, 0, 0, 2], [1, 0, 1, 1], [0, 0, 0, 1]]
    assert R.count_truth(PX, 5, 7).tolist() == [[0, 0, 0, 3]]
    assert R.count_truth(PX, 2, 0).dtype == np.uint32
    every, none = [[2] * 4, [2] * 4, [1] * 4], [[0] * 4] * 3
    assert R.count_truth(PX, 2, -128).tolist() == every == R.count_truth(PX, 2, -129).tolist()
    assert R.count_truth(PX, 2, 127).tolist() == [[0] * 4, [0] * 4, [0, 0, 0, 1]]
    assert R.count_truth(PX, 2, 128).tolist() == none == R.count_truth(PX, 2, 1 << 40).tolist()
    u = np.array([[0, 255], [255, 254]], np.uint8)
    assert R.count_truth(u, 2, 255).tolist() == [[1, 1]] and R.count_truth(u, 2, 256).tolist() == [[0, 0]]
    assert R.count_truth(u, 2, 0).tolist() == [[2, 2]] == R.count_truth(u, 2, -1).tolist()


def test_truth_dispatch_out_dtype_and_thresholds():
    for op in R.OPS:
        t = R.truth(PX, 2, op, threshold=1)
        assert t.shape == (3, 4) and t.dtype == R.out_dtype(np.int8, op)
    assert R.truth(PX, 2, "count", threshold=1).tolist() == R.count_truth(PX, 2, 1).tolist() != R.count_truth(PX, 2, 0).tolist()
    assert R.out_dtype(np.uint16, "max") == np.uint16 and R.out_dtype(np.uint16, "sumsq") == np.uint64 and R.out_dtype(np.int32, "count") == np.uint32
    assert R.thresholds(np.int16) == [0, 1, 10922, -32768, -32769, 32767, 32768]
    assert R.thresholds(np.uint32) == [0, 1, 1431655765, 0, -1, 4294967295, 4294967296]
    with pytest.raises(AssertionError):
        R.truth(PX, 2, "median")
    with pytest.raises(AssertionError):
        R.truth(PX, 0, "max")
