"""What the GPU tests of the entry points share: stacks, guarded outputs and timing.  One copy of each, so that a test module
takes its helpers from here, not from another test module, and an edit to one consumer's helper cannot change another
consumer's data.

  * torch_dt / to_dev / to_np: numpy <-> torch for every integer container and float32 / float64, through bytes, so the
    unsigned wide types need no special case;
  * encode: codec.encode + check() + synchronise;
  * mixed / ladder / ladder_holds_every_width: the seeded data sets;
  * Guarded / status_block / input_forms: an output between two bands of a sentinel, the poisoned status words, the three
    ways a call can be given a stack;
  * events_median: HIP-event timing (tools/timing.py holds the same loop for the scripts under tools/, which do not import
    from tests/);
  * sum_truth / sparse_truth: the numpy truths more than one module compares with.

No fixtures, no library at import; everything but encode() works on CPU tensors: tests/test_gpu_support_model.py runs it there
and shows that each check can fail."""
import statistics

import numpy as np

GUARD = 64                                                  # sentinel elements on either side of a guarded output
OK, INVALID_ARG, CAPACITY, CORRUPT = 0, 1, 3, 5              # status word 0 (include/trpx_hip.h)

DTYPE_NAMES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64", "float32", "float64")


# ---- dtype mapping and transfer ------------------------------------------------------------------------------------------------
def torch_dt(dt):
    import torch
    name = np.dtype(dt).name
    assert name in DTYPE_NAMES, name
    return getattr(torch, name)


def to_dev(a: np.ndarray, device="cuda"):
    """A numpy array as an (aligned) tensor of the same type and shape on `device`."""
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:                                         # (no bytes to view)
        return torch.empty(a.shape, dtype=torch_dt(a.dtype), device=device)
    if not a.flags.writeable:                               # (torch.from_numpy wants a writable array; shared cases are read-only)
        a = a.copy()
    raw = torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device, copy=True)     # (copy: never an alias of `a`, on the CPU either)
    return raw.view(torch_dt(a.dtype)).view(a.shape)


def to_np(t) -> np.ndarray:
    """A tensor as a numpy array of the same type and shape on the host."""
    import torch
    name = str(t.dtype).split(".")[1]                       # torch.uint16 -> uint16
    assert name in DTYPE_NAMES, name
    dt = np.dtype(name)
    if t.numel() == 0:
        return np.empty(tuple(t.shape), dt)
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().view(dt).reshape(tuple(t.shape))


# ---- encode --------------------------------------------------------------------------------------------------------------------
def encode(px, index=True, block=12):
    """codec.encode of pixels, checked and synchronised.  px: a numpy array [frames, values] or [frames, h, w], uploaded as
    [frames, values]; or a tensor already on the device, handed to codec.encode as it is (which takes either shape).
    index: also keep the decode index."""
    import torch
    from trpx_amd import codec
    if isinstance(px, np.ndarray):
        px = to_dev(px.reshape(px.shape[0], -1))
    enc = codec.encode(px, block=block, index=True if index else None)
    enc.check()
    torch.cuda.synchronize()
    return enc


# ---- generators ----------------------------------------------------------------------------------------------------------------
def mixed(dt, shape, seed, zero_stretch=False):
    """Mixed magnitudes, [frames, values] or [frames, h, w]: small values (narrow blocks) and full-range runs (wide blocks;
    32-bit types: blocks of width 32).  zero_stretch: values [v // 2, v // 2 + v // 7) of every frame are zero (width-0 blocks)."""
    n, v = shape[0], int(np.prod(shape[1:]))
    rng = np.random.default_rng(seed)
    info = np.iinfo(dt)
    big = rng.integers(info.min, int(info.max) + 1, size=(n, v), dtype=np.int64)
    small = rng.integers(-3 if info.min < 0 else 0, 4, size=(n, v), dtype=np.int64)
    sel = (np.arange(v) // 97) % 3 == 0
    out = np.where(sel[None, :], big, small)
    if zero_stretch:
        out[:, v // 2: v // 2 + v // 7] = 0
    return out.astype(dt).reshape(shape)


def ladder(dt, shape, seed):
    """A width ladder: block b holds one value of exactly 2^w - 1 (signed: 2^(w - 1) - 1, and -2^(w - 1) + 1 as well) at
    position b % 12 and nothing larger in magnitude, w cycling through 0 .. bits: the largest value a block of every width can
    hold is there in some block, which is where a skip rule's boundary lies."""
    n, v = shape
    rng = np.random.default_rng(seed)
    info = np.iinfo(dt)
    nblk = -(-v // 12)
    b = np.arange(nblk)
    out = np.empty((n, nblk, 12), np.int64)
    for f in range(n):
        w = (b + 5 * f) % (info.bits + 1)
        hi = np.where(w == 0, 0, (1 << np.maximum(w - (1 if info.min < 0 else 0), 0).astype(np.int64)) - 1).astype(np.int64)
        r = rng.random((nblk, 12))
        if info.min < 0:
            vals = np.floor((2 * r - 1) * hi[:, None]).astype(np.int64)
            vals[b, (b + 5) % 12] = -hi
        else:
            vals = np.floor(r * hi[:, None]).astype(np.int64)
        vals = np.clip(vals, -hi[:, None], hi[:, None])
        vals[b, b % 12] = hi
        out[f] = vals
    return np.ascontiguousarray(out.reshape(n, nblk * 12)[:, :v]).astype(dt)


def ladder_holds_every_width(px):
    """The ladder data set does what it is for (a check of the fixture, not of the code): for every width w the largest value a
    w-bit block can hold is there.  Holds from three turns of the ladder on: 12 * 3 * 33 values a frame."""
    info = np.iinfo(px.dtype)
    for w in range(1, info.bits + 1):
        top = (1 << (w - 1 if info.min < 0 else w)) - 1
        assert (px == top).any() and (info.min == 0 or (px == -top).any()), (px.dtype, w)


# ---- guarded outputs -----------------------------------------------------------------------------------------------------------
class Guarded:
    """An output of a call in the middle of a larger allocation: `view` is n elements of `dt`, with GUARD elements on either
    side, all of it filled with `sentinel`."""

    def __init__(self, n: int, dt, sentinel: int, device="cuda"):
        self.n = n
        self.fill = np.full(1, sentinel, dt)[0]
        self.whole = to_dev(np.full(n + 2 * GUARD, sentinel, dt), device)
        self.view = self.whole[GUARD:GUARD + n]

    def check(self, what: str, untouched_from=None) -> np.ndarray:
        """Raises if an element outside the view is not the sentinel -- or, for a call that was given a null pointer or a
        capacity short of n, an element of the view at or behind `untouched_from`.  Returns the view on the host."""
        a = to_np(self.whole)
        assert (a[:GUARD] == self.fill).all() and (a[GUARD + self.n:] == self.fill).all(), f"written outside {what}"
        if untouched_from is not None:
            assert (a[GUARD + untouched_from:] == self.fill).all(), f"{what} written at or behind element {untouched_from}"
        return a[GUARD:GUARD + self.n]


def status_block(device="cuda"):
    """The status words of a call, prefilled with what no call writes."""
    import torch
    return torch.full((8,), 77, dtype=torch.int32, device=device)


def input_forms(enc, mode, first=0):
    """(frame_offsets, index) to pass for the frames from `first` on: "index" = both, "offsets" = no index, "none" = neither."""
    assert mode in ("index", "offsets", "none")
    return (None if mode == "none" else enc.frame_offsets[first:]), (enc.index if mode == "index" else None)


# ---- timing --------------------------------------------------------------------------------------------------------------------
def events_median(fn, reps, warm=3):
    """Median over `reps` calls of fn, in ms between two HIP events, after `warm` untimed calls."""
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


# ---- shared truths: numpy on the original pixels ---------------------------------------------------------------------------------
def sum_truth(px: np.ndarray, group: int, out_dt) -> np.ndarray:
    """trpx_decode_sum: the sums of `group` consecutive frames in int64, clamped (32-bit outputs) or rounded once"""
    n = px.shape[0]
    p64 = px.reshape(n, -1).astype(np.int64)
    s = np.stack([p64[j:j + group].sum(axis=0) for j in range(0, n, group)])
    o = np.dtype(out_dt)
    if o.kind in "iu" and o.itemsize == 4:
        info = np.iinfo(o)
        return np.clip(s, info.min, info.max).astype(o)
    return s.astype(o)


def sparse_truth(px: np.ndarray, t: int):
    """trpx_decode_sparse: (row_offsets int64 [n + 1], positions uint32, values) of px [n, v] at threshold t"""
    info = np.iinfo(px.dtype)
    if t <= info.min:
        m = np.ones(px.shape, bool)
    elif t > info.max:
        m = np.zeros(px.shape, bool)
    else:
        m = px >= px.dtype.type(t)
    rows = np.concatenate([[0], np.cumsum(m.sum(axis=1))]).astype(np.int64)
    return rows, np.nonzero(m)[1].astype(np.uint32), px[m]
