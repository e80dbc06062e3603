"""The truths of trpx_decode_reduce: numpy on the ORIGINAL pixels (the codec is lossless, so no decoder is trusted).  px is
[frames, values]; every function returns [ceil(frames / group), values] of the element the op writes.  No library, no GPU:
tests/test_reduce_truth_model.py runs them on hand-written arrays."""
import numpy as np

OPS = ("max", "min", "sumsq", "count")


def out_dtype(dt, op):
    """the element the op writes: the pixel type for max / min, uint64 for sumsq, uint32 for count"""
    assert op in OPS, op
    return np.dtype(np.uint64) if op == "sumsq" else np.dtype(np.uint32) if op == "count" else np.dtype(dt)


def _groups(px, group):
    n = px.shape[0]
    assert px.ndim == 2 and n >= 1 and group >= 1
    return [px[j:j + group] for j in range(0, n, group)]   # a short last group: the frames that exist


def max_truth(px, group):
    return np.stack([p.max(axis=0) for p in _groups(px, group)])


def min_truth(px, group):
    return np.stack([p.min(axis=0) for p in _groups(px, group)])


def sumsq_truth(px, group):
    """sum of (int64)v * (int64)v modulo 2^64.  numpy's int64 product wraps (two's complement) and its bits are the unsigned
    product's; the sum is taken in uint64, which wraps by definition."""
    with np.errstate(over="ignore"):
        return np.stack([(p.astype(np.int64) ** 2).astype(np.uint64).sum(axis=0, dtype=np.uint64) for p in _groups(px, group)])


def sumsq_exact(px, group):
    """the same sum in Python integers, unbounded: [outputs][values] lists (for the model test and the wrap assertion)"""
    return [[sum(int(v) * int(v) for v in p[:, i]) for i in range(px.shape[1])] for p in _groups(px, group)]


def count_truth(px, group, threshold):
    """frames with (int64)v >= threshold; the threshold is any int64 (beyond the type's limits: every frame / none)"""
    t = np.int64(threshold)
    return np.stack([(p.astype(np.int64) >= t).sum(axis=0).astype(np.uint32) for p in _groups(px, group)])


def truth(px, group, op, threshold=0):
    assert op in OPS, op
    if op == "max":
        return max_truth(px, group)
    if op == "min":
        return min_truth(px, group)
    if op == "sumsq":
        return sumsq_truth(px, group)
    return count_truth(px, group, threshold)


def thresholds(dt):
    """the COUNT_GE thresholds of the exactness matrix: 0, 1, a mid value, the type's minimum and minimum - 1, its maximum and
    maximum + 1"""
    info = np.iinfo(dt)
    return [0, 1, int(info.max) // 3, int(info.min), int(info.min) - 1, int(info.max), int(info.max) + 1]
