"""The model behind the converting-decode edge tests (test_convert_edges_model.py, test_gpu_convert_edges.py): the values at
which a conversion can go wrong, stacks that carry them through every position of a block, and the expected output computed
from the ORIGINAL pixels in integer arithmetic.  The codec is lossless, so no decoder is trusted.  Plain module, no tests."""
import zlib

import numpy as np

SRCS = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
DSTS = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64, np.float32, np.float64]
SUM_SRCS = [np.uint16, np.int16, np.uint32, np.int32]
SUM_OUTS = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
N_DEFAULT = 12 * 256 + 5                                   # two 256-block groups and a 5-value last block

# float32 ties and their neighbours below 2^32 (24 significant bits: from 2^24 on not every integer is a float)
F32_EDGES = [2**24 - 1, 2**24, 2**24 + 1, 2**24 + 2, 2**24 + 3, 2**25 + 2, 2**25 + 6, 2**31 - 65, 2**31 - 64,
             2**32 - 129, 2**32 - 128, 2**32 - 1]
F64_EDGES = [2**53 - 1, 2**53, 2**53 + 1, 2**53 + 2, 2**53 + 3, 2**61 + 2**8, 2**61 + 2**8 + 1]


def legal(src, dst) -> bool:
    """A signed stream into an unsigned container is refused (Terse.hpp:356-357)."""
    return not (np.dtype(src).kind == "i" and np.dtype(dst).kind == "u")


def src_range(src):
    """(min, max) of a pixel type; 64-bit types: the project's domain D3 (unsigned < 2^63, |signed| < 2^62)."""
    src = np.dtype(src)
    if src.itemsize == 8:
        return (0, 2**63 - 1) if src.kind == "u" else (-(2**62 - 1), 2**62 - 1)
    info = np.iinfo(src)
    return int(info.min), int(info.max)


def rne(v: int, mant_bits: int) -> int:
    """The integer nearest to v with at most mant_bits significant bits, ties to the even one: what a conversion of v to a
    binary float of that precision yields (24: float32, 53: float64; no exponent limit is in reach).  Integers only."""
    a = -v if v < 0 else v
    drop = a.bit_length() - mant_bits
    if drop <= 0:
        return v
    q, rest, half = a >> drop, a & ((1 << drop) - 1), 1 << (drop - 1)
    if rest > half or (rest == half and (q & 1)):
        q += 1
    return -(q << drop) if v < 0 else q << drop


def _as_int64(px) -> np.ndarray:
    a = np.asarray(px)
    if a.dtype == np.uint64:
        assert a.size == 0 or int(a.max()) < 2**63, "outside the domain D3"
    return a.astype(np.int64)                              # (object arrays / lists of Python integers: exact or OverflowError)


def truth(px, dst) -> np.ndarray:
    """What decoding `px` (the original pixels: an integer array or Python integers, below 2^63 in magnitude) into `dst`
    must give: clamped to dst's range for an integral dst, rounded once to nearest even for a floating one."""
    dst = np.dtype(dst)
    a = _as_int64(px)
    if dst.kind in "iu":
        info = np.iinfo(dst)
        return np.clip(a, max(int(info.min), -2**63), min(int(info.max), 2**63 - 1)).astype(dst)
    mant = 24 if dst == np.float32 else 53
    uniq, inv = np.unique(a, return_inverse=True)
    # rne leaves at most 53 significant bits: float() of it is exact, and so is the cast to float32 of a 24-bit one
    vals = np.array([float(rne(int(u), mant)) for u in uniq], np.float64).astype(dst)
    return vals[inv.reshape(-1)].reshape(a.shape)


def edge_values(src, dst) -> list:
    """The values of src's range at which a conversion into dst can go wrong, as sorted Python integers."""
    src, dst = np.dtype(src), np.dtype(dst)
    lo, hi = src_range(src)
    vals = {0, 1, -1, lo, lo + 1, hi - 1, hi}
    if dst.kind in "iu":
        d = np.iinfo(dst)
        vals |= {int(d.min) - 1, int(d.min), int(d.min) + 1, int(d.max) - 1, int(d.max), int(d.max) + 1}
    elif dst == np.float32:
        vals |= set(F32_EDGES)
        if src.itemsize == 8:
            # around both kinds of tie at 2^40, 2^53 and 2^61, one below and ONE BIT ABOVE the halfway point: there a
            # conversion through double (exact at 2^40, a rounding of its own at 2^53 and 2^61) differs from a single one
            for k in (40, 53, 61):
                h = 1 << (k - 24)
                vals |= {(1 << k) + m * h + e for m in (1, 3) for e in (-1, 0, 1)}
    elif src.itemsize == 8:
        vals |= set(F64_EDGES)
    if src.kind == "i":
        vals |= {-v for v in vals}
    return sorted(v for v in vals if lo <= v <= hi)


def edge_stack(src, dst, n: int = N_DEFAULT, frames: int = 3, block: int = 12) -> np.ndarray:
    """[frames', n'] pixels of type src that carry every edge_values(src, dst):
      * at every position 0 .. block-1 of a block of its own whose other values are small (the edge sets the width),
      * inside a run of three blocks of one width (repeat-width headers),
      * in the short last block of a frame,
    between small seeded noise and a stretch of zero blocks.  n' = n plus whole 256-block groups and frames' >= frames where
    the edges do not fit otherwise (the last blocks of `frames` frames hold frames * (n % block) values only)."""
    src = np.dtype(src)
    edges = edge_values(src, dst)
    rng = np.random.RandomState(zlib.crc32(f"{src.name}>{np.dtype(dst).name}/{block}".encode()) & 0x7FFFFFFF)
    while n % block == 0:
        n += 12 * 256
    tail = n % block
    frames = max(frames, -(-len(edges) // tail))
    per = -(-len(edges) // frames)                         # edges laid out per frame
    need = 2 + per * (block + 4) + 4                       # blocks: lead-in noise, the sections, the zeros
    while n // block < need or n % block == 0:
        n += 12 * 256
    tail = n % block
    small_lo = -3 if src.kind == "i" else 0
    px = [[int(x) for x in rng.randint(small_lo, 4, size=n)] for _ in range(frames)]
    for f in range(frames):
        b = 2
        for i in range(f, len(edges), frames):
            e = edges[i]
            for pos in range(block):                       # a block of its own, the edge at every position
                px[f][b * block + pos] = e
                b += 1
            b += 1                                         # (a noise block between the sections)
            for k in range(3):                             # a run of equal-width blocks
                px[f][b * block + (i + 5 * k) % block] = e
                b += 1
        b += 1
        for k in range(b * block, (b + 3) * block):        # a stretch of zeros: blocks of width 0
            px[f][k] = 0
        assert b + 3 <= n // block
        for k, i in enumerate(range(f * tail, min((f + 1) * tail, len(edges)))):
            px[f][n - tail + k] = edges[i]                 # the short last block
    return np.array(px, dtype=object).astype(src)


# ---- designed sums (trpx_decode_sum) ----------------------------------------------------------------------------------
I32_MAX, I32_MIN, U32_MAX = 2**31 - 1, -2**31, 2**32 - 1
SUM_TARGETS = [I32_MAX - 1, I32_MAX, I32_MAX + 1, I32_MIN + 1, I32_MIN, I32_MIN - 1, U32_MAX, U32_MAX + 1, 0] + F32_EDGES


def sum_targets(src, terms: int) -> list:
    """The targets a sum of `terms` values of type src can land on (negative ones for signed sources only), and the
    negatives of the float32 list for signed sources."""
    lo, hi = src_range(src)
    t = list(SUM_TARGETS) + ([-v for v in F32_EDGES] if lo < 0 else [])
    t += [1, terms * hi, terms * hi - 1] + ([-1, terms * lo, terms * lo + 1] if lo < 0 else [])   # (the ends of what is in reach)
    return [v for v in dict.fromkeys(t) if terms * lo <= v <= terms * hi]


def split_sum(target: int, terms: int, src, rng) -> list:
    """`terms` integers inside src's range that add up to `target` exactly: seeded random terms, the rest spread greedily."""
    lo, hi = src_range(src)
    assert terms * lo <= target <= terms * hi
    out, left = [], target
    for k in range(terms, 0, -1):
        a, b = max(lo, left - (k - 1) * hi), min(hi, left - (k - 1) * lo)    # what keeps the rest reachable
        v = a if k == 1 else int(rng.randint(0, 2**31 - 1)) % (b - a + 1) + a
        if k > 1 and rng.rand() < 0.25:
            v = b if rng.rand() < 0.5 else a               # and often a term at the end of its range
        out.append(v)
        left -= v
    assert left == 0 and sum(out) == target
    return out


def sum_stack(src, frames: int, n: int, group: int, seed: int) -> np.ndarray:
    """[frames, n] pixels of type src whose sums over each group of `group` consecutive frames land on sum_targets, column
    after column (a short last group takes the targets it can reach)."""
    src = np.dtype(src)
    rng = np.random.RandomState(seed)
    px = np.zeros((frames, n), dtype=object)
    for g0 in range(0, frames, group):
        terms = min(group, frames - g0)
        tg = sum_targets(src, terms)
        for col in range(n):
            px[g0:g0 + terms, col] = split_sum(tg[(col + g0) % len(tg)], terms, src, rng)
    return px.astype(src)


def sum_truth(px, group: int, dst) -> np.ndarray:
    """truth() of the exact integer sums of each group of frames."""
    a = _as_int64(px)
    return truth(np.stack([a[j:j + group].sum(axis=0) for j in range(0, a.shape[0], group)]), dst)
