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
  * sum_truth / sparse_truth: the numpy truths more than one module compares with;
  * selected: a route or path setter (trpx_set_decode_path / _encode_path / _locate_path) for a block, auto behind it;
  * index_layout / index_parts / assert_same_index: the two defined parts of a decode index;
  * assert_round_trip: status 0 and the pixels back, byte for byte;
  * host_encode / host_decode: trpx_encode_host / trpx_decode_host on numpy arrays, into poisoned buffers;
  * fuzz_stack, ALL_DTYPES, ROUTES: the width patterns, pixel types and forced decode routes of the route tests;
  * run_case / run_variant: a program of tests/variant_cases/ in a child python, on the product or on a test build of the library;
  * large stacks (tests/test_gpu_large_stacks.py): crossing_frames picks the frames around a boundary of a running total,
    assert_stream_is_chunks compares a stack with the concatenation of encodes of its chunks, DeviceGuarded is Guarded for outputs
    too large for the host, wide / frame_chunks / ConsumerSpec / consumer_truths are every consumer written with plain torch in
    int64, chunk by chunk, from the pixels; need_device_memory fails (never skips) where the device has too little free.

No fixtures, no library at import; everything but encode(), the host_ calls and the child programs works on CPU tensors:
tests/test_gpu_support_model.py and tests/test_support_checks_model.py run it there and show that each check can fail."""
import contextlib
import ctypes as C
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                                                  # sentinel elements on either side of a guarded output
OK, INVALID_ARG, CAPACITY, CORRUPT = 0, 1, 3, 5              # status word 0 (include/trpx_hip.h)

DTYPE_NAMES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64", "float32", "float64")
ALL_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32]          # the pixel types of the tuned kernels
# trpx_set_decode_path (0 = auto).  4: large frames by round 4's parts route instead of the index route; = auto for small frames;
# 5: auto with the listed frames' index by the dense walk, decode_dense.hip
ROUTES = {"basic": 1, "tiles": 2, "frames": 3, "parts": 4, "dense": 5}


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


# ---- routes and paths ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def selected(setter: str, value: int, lib=None):
    """trpx_set_decode_path / _encode_path / _locate_path for the block, 0 (auto) behind it -- also when the block raises: a
    route left set makes every later test of the process fail for the wrong reason.  lib: the library (a stub in the CPU tier)."""
    if lib is None:
        from trpx_amd import _lib
        lib = _lib.lib()
    fn = getattr(lib, setter)
    rc = fn(value)
    assert rc == 0, (setter, value, rc)
    try:
        yield
    finally:
        fn(0)


# ---- the decode index ------------------------------------------------------------------------------------------------------------
def index_layout(n_values, n_frames):
    """(bytes of group offsets, byte at which the widths start, bytes of widths) of a decode index at block 12: one 8-byte
    offset per group of 256 blocks, padding up to a multiple of 16, one byte per block."""
    nb = (n_values + 11) // 12
    ng = (nb + 255) // 256
    return 8 * n_frames * ng, (8 * n_frames * ng + 15) // 16 * 16, n_frames * nb


def index_parts(index, n_values, n_frames):
    """(group-offset bytes, width bytes) of a decode index, tensor or array.  The index is defined only where a group / a block
    exists: the padding between the two parts belongs to neither."""
    g, w_off, w = index_layout(n_values, n_frames)
    return index[:g], index[w_off: w_off + w]


def _same(a, b):
    """Byte equality of two tensors (compared where they are) or of a tensor / an array and an array (on the host)."""
    if not isinstance(a, np.ndarray) and not isinstance(b, np.ndarray):
        import torch
        return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    a, b = (x if isinstance(x, np.ndarray) else to_np(x) for x in (a, b))
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


def assert_same_index(a, b, n_values, n_frames, ctx):
    """Two decode indices agree in their group offsets and in their widths."""
    for what, pa, pb in zip(("group offsets", "widths"), index_parts(a, n_values, n_frames), index_parts(b, n_values, n_frames)):
        assert _same(pa, pb), (ctx, what)


# ---- round trip ------------------------------------------------------------------------------------------------------------------
def assert_round_trip(back, status, px, ctx):
    """What a decode returned: status word 0 is 0, `back` has the type and the number of elements of `px` and holds its bytes
    (through uint8, so that the unsigned wide types need no special case; [frames, values] against [frames, h, w] is the same
    stack).  Tensors or arrays; the caller has synchronised."""
    assert int(status[0]) == 0, (ctx, "status", int(status[0]))
    kind = [str(x.dtype).split(".")[-1] for x in (back, px)]                # torch.uint16 / dtype('uint16') -> uint16
    assert kind[0] == kind[1] and int(np.prod(back.shape)) == int(np.prod(px.shape)), (ctx, "type or size differ", kind, back.shape, px.shape)
    assert _same(back, px), (ctx, "pixels differ")


# ---- child programs --------------------------------------------------------------------------------------------------------------
VARIANT_CASES = os.path.join(ROOT, "tests", "variant_cases")
VARIANTS = os.path.join(ROOT, "tools", "variants")


def run_case(case, *args, **env):
    """tests/variant_cases/`case` (or a path) in a fresh child python with `env` added to the environment: it must exit 0 and
    print OK within 600 s."""
    r = subprocess.run([sys.executable, os.path.join(VARIANT_CASES, case), *args], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **env))
    assert r.returncode == 0 and "OK" in r.stdout, (case, args, env, r.stdout[-2000:], r.stderr[-3000:])


def run_variant(name, case, *args, variants=VARIANTS):
    """The case on the test build tools/variants/libtrpx_`name`.so (TRPX_LIB); skips where that build is absent -- looked for
    when its turn comes, so that a failure on one build is not turned into a skip by the absence of the next."""
    import pytest
    variant = os.path.join(variants, f"libtrpx_{name}.so")
    if not os.path.exists(variant):
        pytest.skip(f"test variant not built (make -C trpx_amd/csrc {name})")
    run_case(case, *args, TRPX_LIB=variant)


# ---- the host entry points and the fuzz generator ----------------------------------------------------------------------------------
def host_encode(px2d, block=12):
    """[frames, n] numpy -> (stream bytes, offsets, prolix_bits) through trpx_encode_host."""
    from trpx_amd import _lib
    from trpx_amd.terse import _code
    L = _lib.lib()
    px2d = np.ascontiguousarray(px2d)
    f, n = px2d.shape
    cap = f * L.trpx_worst_case_bytes(_code(px2d.dtype), n, block)
    out = np.full(cap, 0xAA, np.uint8)     # poisoned: every output byte must be written
    total, pb = C.c_size_t(0), C.c_uint(0)
    offs = np.zeros(f + 1, np.uint64)
    _lib.check(L.trpx_encode_host(_code(px2d.dtype), px2d.ctypes.data, n, f, block, out.ctypes.data, cap,
                                  C.byref(total), offs.ctypes.data, C.byref(pb), -1))
    return out[: total.value].copy(), offs, int(pb.value)


def host_decode(stream, offs, n, frames, dtype, block=12, stream_signed=None):
    from trpx_amd import _lib
    from trpx_amd.terse import _code
    L = _lib.lib()
    out = np.full((frames, n), 0x55, np.dtype(dtype))
    stream = np.ascontiguousarray(stream)
    _lib.check(L.trpx_decode_host(int(np.dtype(dtype).kind == "i") if stream_signed is None else int(stream_signed),
                                  _code(dtype, True), stream.ctypes.data, stream.size,
                                  offs.ctypes.data if offs is not None else None, n, frames, block,
                                  out.ctypes.data, -1))
    return out


def fuzz_stack(rng, dt, kind, n, frames):
    """tools/fuzz_paths.py's generator: width patterns that exercise runs, outliers, flips and long runs (inside D3)."""
    top = 8 * dt.itemsize - (2 if dt.kind == "i" else (1 if dt.itemsize == 4 else 0))
    nblk = (n + 11) // 12
    if kind == 0:
        hi = np.full((frames, nblk), rng.randint(0, top + 1))                                          # one width
    elif kind == 1:
        hi = rng.randint(0, top + 1, size=(frames, nblk))                                              # every block its own width
    elif kind == 2:
        hi = np.where(rng.rand(frames, nblk) < 0.02, rng.randint(0, top + 1, size=(frames, nblk)), 3 if top >= 3 else 1)   # runs + outliers
    elif kind == 3:
        hi = np.where(rng.rand(frames, nblk) < 0.5, 2, 3 if top >= 3 else 1)                          # flips every other block
    elif kind == 5:                                                                                    # payloads of one bits: a header position
        hi = np.repeat(rng.randint(0, min(top, 12) + 1, size=(frames, (nblk + 39) // 40)), 40, axis=1)[:, :nblk]   # may read 0xFFFFFFFF
        sat = np.repeat(hi, 12, axis=1)[:, :n]
        mag = np.where(rng.rand(frames, n) < 0.97, (1 << sat) - 1, 0).astype(np.int64)
        mag[:, n // 2: n // 2 + n // 5] = 0                                                             # and a run of empty blocks
        if dt.kind == "i":
            return np.where(mag > 0, -1, 0).astype(dt) * (rng.rand(frames, n) < 0.9) + (rng.randint(-40, 40, size=(frames, n)) * (rng.rand(frames, n) < 0.01)).astype(dt)
        return mag.astype(dt)
    else:
        hi = np.repeat(rng.randint(0, top + 1, size=(frames, (nblk + 299) // 300)), 300, axis=1)[:, :nblk]   # long runs of changing widths
    mag = (rng.rand(frames, nblk * 12) * (2.0 ** np.repeat(hi, 12, axis=1))).astype(np.int64)[:, :n]
    if kind % 2 == 0:
        mag[:, : n // 3] = 0                                                                          # empty stretches
    if dt.kind == "i":
        mag = mag * rng.choice([-1, 1], size=mag.shape)
    return mag.astype(dt)


# ---- large stacks: the frames around a boundary, chunk-wise encodes, guarded outputs on the device, torch truths ---------------------
def need_device_memory(need: int, what: str):
    """Fails -- never skips -- where the device has less than `need` bytes free (after handing torch's cache back)."""
    import torch
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    assert free >= need, f"{what} needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB are free"


def crossing_frames(offs, boundaries):
    """offs [n + 1]: what lies in front of every frame (bytes, bits, values), tensor or array.  Returns ({boundary: the frame k
    that holds it, offs[k] <= boundary < offs[k + 1]}, the frames to sample: the first, the last and k - 1, k, k + 1 of every
    boundary).  A boundary the stack does not reach is an error: a test of a crossing must not pass without one."""
    o = (offs if isinstance(offs, np.ndarray) else to_np(offs)).astype(np.int64)
    n = o.size - 1
    at, picks = {}, {0, n - 1}
    for b in boundaries:
        assert o[0] <= b < o[-1], f"boundary {b} is not crossed: the stack ends at {int(o[-1])}"
        k = int(np.searchsorted(o, b, side="right")) - 1
        at[b] = k
        picks.update(f for f in (k - 1, k, k + 1) if 0 <= f < n)
    return at, sorted(picks)


def _i64(x):
    if isinstance(x, np.ndarray):
        return x.astype(np.int64)
    import torch
    return x.view(torch.int64) if str(x.dtype) == "torch.uint64" else x.to(torch.int64)


def assert_stream_is_chunks(stream, offs, n_frames, encode_chunk, chunk=256, ctx=""):
    """Frames are independent and start on a byte: `stream` with offsets `offs` [n_frames + 1] must be, byte for byte, what
    encode_chunk(f0, f1) -> (bytes, offsets [f1 - f0 + 1]) gives for the frames [f0, f1) of every chunk of `chunk` frames, one
    behind the other, and `offs` the running sums.  Tensors (compared where they are) or arrays."""
    assert int(offs[0]) == 0 and offs.shape[0] == n_frames + 1, (ctx, "offsets")
    at = 0
    for f0 in range(0, n_frames, chunk):
        f1 = min(f0 + chunk, n_frames)
        cs, co = encode_chunk(f0, f1)
        co = _i64(co)
        assert int(co[0]) == 0 and co.shape[0] == f1 - f0 + 1, (ctx, "chunk offsets", f0)
        assert _same(_i64(offs[f0:f1 + 1]), co + at), (ctx, f"offsets of frames {f0}..{f1} are not the running sums", at)
        size = int(co[-1])
        assert at + size <= stream.shape[0], (ctx, f"the stream ends inside frames {f0}..{f1}")
        assert _same(stream[at:at + size], cs[:size]), (ctx, f"bytes of frames {f0}..{f1} (from byte {at}) differ")
        at += size
    assert at == int(offs[n_frames]) == stream.shape[0], (ctx, "total", at, int(offs[n_frames]), stream.shape[0])


class DeviceGuarded:
    """Guarded for an output too large to build or to check on the host: `view` has `shape` and type `tdt` (a torch dtype), with
    GUARD elements on either side, every byte of the allocation 0xA5 until something writes it; checked where it lies."""
    BYTE = 0xA5

    def __init__(self, shape, tdt, device="cuda"):
        import torch
        self.n = int(np.prod(shape))
        self.whole = torch.empty(self.n + 2 * GUARD, dtype=tdt, device=device)
        self.view = self.whole[GUARD:GUARD + self.n].view(shape)
        self.poison()

    def poison(self):
        import torch
        self.whole.view(torch.uint8).fill_(self.BYTE)

    def check(self, what: str):
        import torch
        lo, hi = self.whole[:GUARD].view(torch.uint8), self.whole[GUARD + self.n:].view(torch.uint8)
        assert bool((lo == self.BYTE).all()) and bool((hi == self.BYTE).all()), f"written outside {what}"
        return self.view


def wide(x):
    """An integer tensor as int64 with the same values (torch has few operators for the unsigned wide types)."""
    import torch
    name = str(x.dtype)
    if name == "torch.uint16":
        return x.view(torch.int16).to(torch.int64) & 0xFFFF
    if name == "torch.uint32":
        return x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if name == "torch.uint64":
        return x.view(torch.int64)                          # (the same bits: equal where the values are)
    return x.to(torch.int64)


def signed_view(x):
    """The same bits as the signed type of the same size (for torch.where and friends on the unsigned wide types)"""
    import torch
    return x.view({"torch.uint16": torch.int16, "torch.uint32": torch.int32, "torch.uint64": torch.int64}.get(str(x.dtype), x.dtype))


def keep_from(x, threshold):
    """x with every value below `threshold` set to 0: the frames whose events trpx_decode_sparse returns at that threshold"""
    import torch
    s = signed_view(x)
    return torch.where(wide(x) >= threshold, s, torch.zeros_like(s)).view(x.dtype)


same_bytes = _same


def frame_chunks(f0, f1, n_values, elems=1 << 25):
    """[f0, f1) in runs of frames of at most `elems` values (one int64 copy of a run: 8 * elems bytes)"""
    step = max(1, elems // n_values)
    for a in range(f0, f1, step):
        yield a, min(a + step, f1)


class ConsumerSpec:
    """What the consumers of one large-stack test are asked: group (trpx_decode_sum / _reduce), frame_labels int64 [frames] with
    n_out (a label outside 0 .. n_out - 1 masks the frame; _sum_labelled), weights int64 [K, n_values] (_dot), pixel_labels int64
    [n_values] with n_bins (_bins), width and bin = (bin_y, bin_x) (_binned), threshold (_sparse)."""

    def __init__(self, group, frame_labels, n_out, weights, pixel_labels, n_bins, width, bin, threshold):
        self.group, self.frame_labels, self.n_out, self.weights = group, frame_labels, n_out, weights
        self.pixel_labels, self.n_bins, self.width, self.bin, self.threshold = pixel_labels, n_bins, width, bin, threshold


def consumer_truths(px, spec, elems=1 << 25):
    """Every consumer from the pixels px [frames, n_values], in int64 on px's device, a run of frames at a time: a dict of
      sum, max, sumsq [ceil(frames / group), n_values] (sumsq modulo 2^64, as int64 bits);
      labelled [n_out, n_values], counts [n_out];  dot [frames, K];  bins [frames, n_bins];  binned [frames, oh, ow];
      rows [frames + 1], positions, values: the events with value >= threshold, by frame and ascending position."""
    import torch
    F, n = px.shape
    dev, i64 = px.device, torch.int64
    g, by, bx = spec.group, spec.bin[0], spec.bin[1]
    W = spec.width
    H = n // W
    oh, ow = -(-H // by), -(-W // bx)
    n_g = -(-F // g)
    t = dict(sum=torch.zeros((n_g, n), dtype=i64, device=dev), max=torch.full((n_g, n), -2 ** 63, dtype=i64, device=dev),
             sumsq=torch.zeros((n_g, n), dtype=i64, device=dev), labelled=torch.zeros((spec.n_out, n), dtype=i64, device=dev),
             counts=torch.zeros(spec.n_out, dtype=i64, device=dev), dot=torch.zeros((F, spec.weights.shape[0]), dtype=i64, device=dev),
             bins=torch.zeros((F, spec.n_bins), dtype=i64, device=dev), binned=torch.zeros((F, oh, ow), dtype=i64, device=dev))
    rows, pos, val = [torch.zeros(1, dtype=i64, device=dev)], [], []
    for j in range(n_g):
        for a, b in frame_chunks(j * g, min((j + 1) * g, F), n, elems):
            x = wide(px[a:b])
            t["sum"][j] += x.sum(0)
            t["max"][j] = torch.maximum(t["max"][j], x.amax(0))
            t["sumsq"][j] += (x * x).sum(0)
            lab = spec.frame_labels[a:b]
            ok = (lab >= 0) & (lab < spec.n_out)
            t["labelled"].index_add_(0, lab[ok], x[ok])
            t["counts"] += torch.bincount(lab[ok], minlength=spec.n_out)
            for k in range(spec.weights.shape[0]):
                t["dot"][a:b, k] = (x * spec.weights[k]).sum(1)
            for k in range(spec.n_bins):
                t["bins"][a:b, k] = (x * (spec.pixel_labels == k)).sum(1)
            img = torch.zeros((b - a, oh * by, ow * bx), dtype=i64, device=dev)
            img[:, :H, :W] = x.view(b - a, H, W)
            t["binned"][a:b] = img.view(b - a, oh, by, ow, bx).sum((2, 4))
            m = x >= spec.threshold
            rows.append(m.sum(1))
            pos.append(m.nonzero()[:, 1])
            val.append(x[m])
            del x, img, m
    t["rows"] = torch.cumsum(torch.cat(rows), 0)
    t["positions"], t["values"] = torch.cat(pos), torch.cat(val)
    return t
