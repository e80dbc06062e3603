"""What the tests of trpx_decode_sum_labelled share: the truth -- numpy on the ORIGINAL pixels, never a decoder -- and the launch
plan restated (trpx_amd/csrc/label_runs.hpp, decode_sum_labelled.hpp).  No fixtures, no library, no GPU."""
import numpy as np

MASK = 0xFFFFFFFF                                           # the conventional "in no sum" label
MAX_OUT = 1 << 20
TARGET_CHUNKS, SUB_TILES = 1024, 2                          # chunks a launch aims at, 256-block groups per tile (decode_sum.hpp)
SMALL_FRAMES, SMALL_OUT = 4096, 8192                        # up to here one workgroup orders the frames in LDS


def truth(px: np.ndarray, labels: np.ndarray, n_out: int, out_dt=np.int64):
    """(sums [n_out, values] of out_dt, counts uint32 [n_out]): np.add.at in int64, then gpu_support.sum_truth's conversion
    (32-bit integers clamp, the others astype: floats round once to nearest even)."""
    n = px.shape[0]
    labels = np.asarray(labels).astype(np.uint64)
    assert labels.shape == (n,)
    keep = labels < n_out
    acc = np.zeros((n_out, int(np.prod(px.shape[1:]))), np.int64)
    np.add.at(acc, labels[keep].astype(np.int64), px.reshape(n, -1)[keep].astype(np.int64))
    counts = np.bincount(labels[keep].astype(np.int64), minlength=n_out).astype(np.uint32)
    o = np.dtype(out_dt)
    if o.kind in "iu" and o.itemsize == 4:
        info = np.iinfo(o)
        return np.clip(acc, info.min, info.max).astype(o), counts
    return acc.astype(o), counts


def plan(itemsize: int, n_values: int, n_frames: int):
    """(frames per chunk, chunks, tiles per frame) of the call's launch plan"""
    n_blocks = -(-n_values // 12)
    tpf = -(-n_blocks // (SUB_TILES * 256))
    chunks = max(-(-TARGET_CHUNKS // tpf), 1)
    if tpf > 1:                                             # frames of more than one tile: fill the last round of resident workgroups
        places = 256 * (3 if itemsize < 4 else 2)
        chunks = -(-chunks * tpf // places) * places // tpf
    chunks = min(chunks, n_frames)
    fpc = -(-n_frames // chunks)
    if itemsize < 4:
        fpc = min(fpc, 65535)
    return fpc, -(-n_frames // fpc), tpf


def own_bytes(itemsize: int, n_values: int, n_frames: int, n_out: int) -> int:
    """the call's scratch behind the consumers' front: counts (and the merge list's length), cursors, starts, the merge's list,
    the order, the partial slab"""
    def up(x, a):
        return -(-x // a) * a
    fpc, chunks, _ = plan(itemsize, n_values, n_frames)
    cursor = up(4 * (n_out + 1), 8)
    starts = up(cursor + 4 * n_out, 8)
    todo = up(starts + 4 * (n_out + 1), 8)
    order = up(todo + 4 * n_out, 8)
    slab = up(order + 8 * n_frames, 256)
    return slab + chunks * 2 * up(n_values, 64) * (8 if itemsize == 4 else 4)
