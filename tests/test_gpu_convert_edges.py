"""GPU tests: the converting and narrowing decodes at their value edges, on every route.

The truth is tests/convert_edges.py: the ORIGINAL pixels, clamped or rounded once in integer arithmetic -- the codec is lossless,
so no decoder is trusted.  Every comparison is byte for byte; every device output is the middle of an allocation with GUARD
sentinel elements on either side, checked after the call."""
import functools

import numpy as np
import pytest

import convert_edges as ce
from gpu_support import selected, to_dev, torch_dt
from gpu_support import ROUTES as FORCED_ROUTES

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A
CORRUPT = 5
_name = lambda d: np.dtype(d).name
PAIRS = [(s, d) for s in ce.SRCS for d in ce.DSTS if ce.legal(s, d)]
_pair_id = lambda p: f"{_name(p[0])}-{_name(p[1])}"


# ---- plumbing -----------------------------------------------------------------------------------------------------------
def _stream_dev(stream: np.ndarray):
    """The stack in device memory, padded to whole dwords (the decoders read aligned 32-bit words)."""
    buf = np.zeros((stream.size + 3) // 4 * 4 + 16, np.uint8)
    buf[: stream.size] = stream
    return to_dev(buf)


class _Guarded:
    """n elements of dtype `dt` in device memory between two guard bands."""

    def __init__(self, n: int, dt):
        import torch
        self.n, self.dt = n, np.dtype(dt)
        self.raw = torch.full(((n + 2 * GUARD) * self.dt.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.ptr = self.raw.data_ptr() + GUARD * self.dt.itemsize

    def tensor(self, shape):
        a, b = GUARD * self.dt.itemsize, (GUARD + self.n) * self.dt.itemsize
        return self.raw[a:b].view(torch_dt(self.dt)).view(*shape)

    def check(self):
        a, b = GUARD * self.dt.itemsize, (GUARD + self.n) * self.dt.itemsize
        lo, hi = self.raw[:a].cpu().numpy(), self.raw[b:].cpu().numpy()
        assert (lo == SENTINEL).all() and (hi == SENTINEL).all(), "written outside the output"

    def numpy(self, shape):
        a, b = GUARD * self.dt.itemsize, (GUARD + self.n) * self.dt.itemsize
        return self.raw[a:b].cpu().numpy().view(self.dt).reshape(shape)


def _device_decode(entry: str, stream_signed: bool, dst, d_stream, terse_bytes: int, offs, n: int, frames: int, block: int = 12,
                   want_pixels: bool = True):
    """trpx_decode / trpx_decode_convert on device memory into a guarded output.  Returns (status word 0, pixels or None)
    after checking the return code and the guards."""
    import torch
    from trpx_amd import _lib
    from trpx_amd.terse import _code
    L = _lib.lib()
    out = _Guarded(frames * n, dst)
    st = torch.full((_lib.STATUS_WORDS,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    ws_bytes = max(L.trpx_decode_workspace_bytes(c, n, frames, block) for c in (_lib.U8, _lib.U32, _lib.U64))
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    d_offs = to_dev(np.asarray(offs, np.uint64)) if offs is not None else None
    rc = getattr(L, entry)(int(stream_signed), _code(dst, True), d_stream.data_ptr(), terse_bytes,
                           d_offs.data_ptr() if d_offs is not None else None, n, frames, block, out.ptr, st.data_ptr(),
                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, (entry, rc, L.trpx_last_error_string())
    out.check()
    return int(st[0].item()), (out.numpy((frames, n)) if want_pixels else None)


def _host_decode(stream, offs, n, frames, dst, stream_signed, block=12):
    from trpx_amd import _lib
    from trpx_amd.terse import _code
    dst = np.dtype(dst)
    whole = np.full((frames * n + 2 * GUARD) * dst.itemsize, SENTINEL, np.uint8)
    out = whole[GUARD * dst.itemsize: (GUARD + frames * n) * dst.itemsize]
    stream = np.ascontiguousarray(stream)
    offs = np.ascontiguousarray(offs, np.uint64) if offs is not None else None
    _lib.check(_lib.lib().trpx_decode_host(int(stream_signed), _code(dst, True), stream.ctypes.data, stream.size,
                                           offs.ctypes.data if offs is not None else None, n, frames, block, out.ctypes.data, -1))
    assert (whole[: GUARD * dst.itemsize] == SENTINEL).all() and (whole[(GUARD + frames * n) * dst.itemsize:] == SENTINEL).all()
    return out.view(dst).reshape(frames, n)


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


@functools.lru_cache(maxsize=None)
def _edge_case(src, dst, block):
    """(pixels, oracle stream, offsets, truth) of one pair: computed once, shared by the tests, never written to."""
    from oracle import oracle as O
    px = ce.edge_stack(src, dst, block=block)
    stream, sizes, _ = O.encode_stack(px, block)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    want = ce.truth(px, dst)
    for a in (px, stream, offs, want):
        a.setflags(write=False)
    return px, stream, offs, want


# ---- a. trpx_decode_convert on device memory ------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_decode_convert_on_device_memory(gpu, oracle, pair):
    import torch
    from trpx_amd import codec
    src, dst = pair
    signed = np.dtype(src).kind == "i"
    for block in (12, 7):
        px, stream, offs, want = _edge_case(src, dst, block)
        frames, n = px.shape
        enc = codec.encode(to_dev(px), block=block)
        torch.cuda.synchronize()
        enc.check()
        assert enc.stack().cpu().numpy().tobytes() == stream.tobytes(), ("encode", _pair_id(pair), block)
        assert (enc.frame_offsets.cpu().numpy() == offs.astype(np.int64)).all()
        d_stream = _stream_dev(stream)
        for given in (offs, None):
            code, got = _device_decode("trpx_decode_convert", signed, dst, d_stream, stream.size, given, n, frames, block)
            assert code == 0, (_pair_id(pair), block, given is not None)
            assert _same(got, want), (_pair_id(pair), block, given is not None, px.reshape(-1)[(got != want).reshape(-1)][:8])


# ---- b. the host surface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=_pair_id)
def test_decode_host_every_pair(gpu, oracle, pair):
    src, dst = pair
    signed = np.dtype(src).kind == "i"
    for block, with_offsets in ((12, True), (12, False), (7, True), (7, False)):
        px, stream, offs, want = _edge_case(src, dst, block)
        frames, n = px.shape
        got = _host_decode(stream, offs if with_offsets else None, n, frames, dst, signed, block)
        assert _same(got, want), (_pair_id(pair), block, with_offsets, px.reshape(-1)[(got != want).reshape(-1)][:8])


@pytest.mark.parametrize("src", [np.uint16, np.int64], ids=_name)
def test_terse_class_containers(gpu, oracle, src):
    from trpx_amd import Terse, _lib
    for dst in (np.int32, np.uint8, np.float32, np.float64):
        px = ce.edge_stack(src, dst if ce.legal(src, dst) else np.int8)
        frames, n = px.shape
        if np.dtype(src).itemsize == 8:
            assert int(np.abs(px).max()) > 2**32                                  # wide values: the stream holds 64-bit pixels
        t = Terse()
        t.push_back_stack(px)
        if not ce.legal(src, dst):                                                # Terse.hpp:356-357
            with pytest.raises(ValueError):
                t.prolix(np.empty(n, dst), 0)
            continue
        want = ce.truth(px, dst)
        assert _same(t.prolix_stack(dst), want), (_name(src), _name(dst), "prolix_stack")
        for f in (0, frames - 1, 1):
            assert _same(t.prolix(np.empty(n, dst), f), want[f]), (_name(src), _name(dst), "prolix", f)
    _lib.lib().trpx_host_release()


# ---- c. narrowing through the tuned routes --------------------------------------------------------------------------------
NARROW = [(np.uint16, np.uint8), (np.int16, np.int8), (np.uint32, np.uint16), (np.int32, np.int16), (np.uint32, np.uint8),
          (np.int32, np.int8)]
ROUTES = {"auto": 0, **FORCED_ROUTES}
GEOMETRIES = [("flips", 3000, 140), ("runs", 40000, 130), ("runs", 12 * 34000 + 3, 3), ("dense", 256 * 512, 6)]


def _narrow_stack(src, dst, kind, n, frames, seed):
    """A stack of type src whose every value fits dst, in the width patterns of the route matrix (flips, runs with outliers)
    and of test_width_changes_every_block_position_parallel_walk (dense: no two neighbouring blocks share a width), the widths
    capped to the container's."""
    dst = np.dtype(dst)
    rng = np.random.RandomState(seed)
    top = 8 * dst.itemsize - (1 if dst.kind == "i" else 0)                        # bits of magnitude
    nblk = (n + 11) // 12
    if kind == "flips":
        hi = np.where(rng.rand(frames, nblk) < 0.5, 2, 3)
    elif kind == "runs":
        hi = np.where(rng.rand(frames, nblk) < 0.02, rng.randint(0, top + 1, size=(frames, nblk)), 3)
    else:
        choices = np.array(sorted({1, 2, 3, 4, 6, min(8, top), top}))
        step = rng.randint(1, len(choices), size=(frames, nblk))                  # never 0: the next block's width differs
        hi = choices[np.cumsum(step, axis=1) % len(choices)]
    mag = (rng.rand(frames, nblk * 12) * (2.0 ** np.repeat(hi, 12, axis=1))).astype(np.int64)
    if kind == "dense":
        mag[:, ::12] = 2 ** hi - 1                                                # the block's width is exactly hi (signed: + 1)
    mag = mag[:, :n]
    if dst.kind == "i":
        mag = mag * rng.choice([-1, 1], size=mag.shape)
    info = np.iinfo(dst)
    assert mag.min() >= info.min and mag.max() <= info.max
    return mag.astype(src)


@functools.lru_cache(maxsize=1)
def _narrow_cases(src, dst):
    """Per geometry: (pixels, the frames' oracle streams, px.astype(dst)); computed once per pair and shared by its routes."""
    from oracle import oracle as O
    cases = []
    for g, (kind, n, frames) in enumerate(GEOMETRIES):
        px = _narrow_stack(src, dst, kind, n, frames, seed=100 * g + ce.SRCS.index(src) + 10 * ce.DSTS.index(dst))
        streams = [O.encode(px[f])[0] for f in range(frames)]
        want = px.astype(dst)
        px.setflags(write=False)
        cases.append((px, streams, want))
    return cases


def _block_bit_positions(O, frame_px):
    """First bit of every block of one frame (header lengths as Terse.hpp:520-541 writes them)."""
    w = O.widths(frame_px).astype(np.int64)
    prev = np.concatenate([[0], w[:-1]])
    hl = np.where(w == prev, 1, np.where(w < 7, 4, np.where(w < 10, 6, 12)))
    nv = np.full(w.size, 12, np.int64)
    nv[-1] = frame_px.size - (w.size - 1) * 12
    return np.concatenate([[0], np.cumsum(hl + nv * w)])


def _placements(O, L, route, px, streams, dst_code):
    """(frame, block) of the one wide block, in turn: block 0 of frame 0, both sides of the first group seam of a middle
    frame, the short last block of the last frame and, where the route cuts the frames into parts, the first block that
    starts behind the first cut of a middle frame (decode_part.hip: cuts at multiples of L bits of the frame)."""
    frames, n = px.shape
    nblk = (n + 11) // 12
    mid = frames // 2
    where = [(0, 0)] + [(mid, b) for b in (255, 256) if b < nblk - 1] + [(frames - 1, nblk - 1)]
    P = L.trpx_decode_parts_per_frame(dst_code, n, frames, 12)
    if P > 1:
        limit = 8 * streams[mid].size
        if route == "parts":
            cut = ((limit + P - 1) // P + 127) & ~127
        else:
            tail = 2048 if limit > 16 * 2048 else limit // 16
            cut = (limit - tail + P - 2) // (P - 1)
        pos = _block_bit_positions(O, px[mid])
        where.append((mid, min(int(np.searchsorted(pos[:-1], cut)), nblk - 2)))
    return where, P


@pytest.mark.parametrize("pair,route", [(p, r) for p in NARROW for r in ROUTES], ids=lambda v: v if isinstance(v, str) else _pair_id(v))
def test_narrowing_through_the_tuned_routes(gpu, oracle, pair, route):
    """decode_any (api.hip) runs the tuned decoder for a same-signedness request and relies on its TRPX_ERR_CORRUPT for a block
    wider than the container to fall back to the converting decoder.  So: a stack that fits decodes on every route; the same
    stack with ONE block one bit too wide -- a legitimate stream of the wider type -- is reported by every route, wherever the
    block sits, with offsets and without, nothing is written outside the output, and the host entry point returns the clamped
    pixels."""
    from trpx_amd import _lib, codec
    L = _lib.lib()
    src, dst = (np.dtype(x) for x in pair)
    signed = dst.kind == "i"
    bits = 8 * dst.itemsize
    info = np.iinfo(dst)
    cases = _narrow_cases(pair[0], pair[1])
    try:
        with selected("trpx_set_decode_path", ROUTES[route]):
            saw_parts = False
            for (kind, n, frames), (px, streams, want) in zip(GEOMETRIES, cases):
                nblk = (n + 11) // 12
                sizes = np.array([s.size for s in streams], np.uint64)
                offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
                stream = np.concatenate(streams)
                d_stream = _stream_dev(stream)
                # fits: the tuned decoders take the stream of the wider type into the narrow container
                for given in (offs, None):
                    code, got = _device_decode("trpx_decode", signed, dst, d_stream, stream.size, given, n, frames)
                    assert code == 0, ("fits", route, kind, n, given is not None, code)
                    assert _same(got, want), ("fits", route, kind, n, given is not None)
                where, P = _placements(oracle, L, route, px, streams, codec.dtype_code(dst))
                saw_parts = saw_parts or P > 1
                for k, (f, b) in enumerate(where):
                    # one value of the block needs one bit more than the container has: it clamps to the container's end
                    v = 1 << (bits - 1) if signed else 1 << bits
                    if signed and k % 2:
                        v = -v - 1
                    i = b * 12 + (k * 5) % (min(12, n - b * 12))
                    frame_px = px[f].copy()
                    frame_px[i] = v
                    w = oracle.widths(frame_px)
                    assert (w > bits).sum() == 1 and w[b] == bits + 1                 # exactly one block, one bit wider
                    wide = oracle.encode(frame_px)[0]
                    parts = streams[:f] + [wide] + streams[f + 1:]
                    stream_w = np.concatenate(parts)
                    offs_w = np.concatenate([[0], np.cumsum([s.size for s in parts])]).astype(np.uint64)
                    d_wide = _stream_dev(stream_w)
                    for given in (offs_w, None):
                        code, _ = _device_decode("trpx_decode", signed, dst, d_wide, stream_w.size, given, n, frames, want_pixels=False)
                        assert code == CORRUPT, ("one wide block", route, kind, n, (f, b), given is not None, code)
                    got = _host_decode(stream_w, offs_w, n, frames, dst, signed)
                    keep = want[f, i]
                    want[f, i] = info.max if v > 0 else info.min                     # truth of the one changed pixel
                    try:
                        assert want[f, i] == ce.truth(np.array([v]), dst)[0]
                        assert _same(got, want), ("one wide block", route, kind, n, (f, b), "host")
                    finally:
                        want[f, i] = keep
            assert saw_parts                                                          # the large-frame geometry is cut into parts
    finally:
        L.trpx_host_release()


# ---- d. trpx_decode_sum on designed sums ----------------------------------------------------------------------------------
SUM_SHAPES = [(6, 12 * 37 + 5, (2, 3, 6)),
              (300, 60, (300,))]          # a single output: the frames of the group are split into chunks with partial slabs


@pytest.mark.parametrize("src", ce.SUM_SRCS, ids=_name)
def test_decode_sum_on_designed_sums(gpu, oracle, src):
    """Column sums built to land on INT32_MAX +- 1, INT32_MIN +- 1, UINT32_MAX (+ 1), 0, the float32 ties and the ends of
    what the source type reaches (the ties beyond 2^53: test_decode_sum_ties_beyond_2_53)."""
    import torch
    from trpx_amd import codec
    for frames, n, groups in SUM_SHAPES:
        for group in groups:
            px = ce.sum_stack(src, frames, n, group, seed=group)
            want_stream, sizes, _ = oracle.encode_stack(px)
            enc = codec.encode(to_dev(px), index=True)
            torch.cuda.synchronize()
            enc.check()
            assert enc.stack().cpu().numpy().tobytes() == want_stream.tobytes()
            n_out = -(-frames // group)
            for dst in ce.SUM_OUTS:
                if not ce.legal(src, dst):
                    continue
                want = ce.sum_truth(px, group, dst)
                for mode in ("index", "offsets", "none"):
                    out = _Guarded(n_out * n, dst)
                    _, st = codec.decode_sum(enc.stack(), None if mode == "none" else enc.frame_offsets, n, frames, src, group,
                                             out_dtype=torch_dt(dst), index=enc.index if mode == "index" else None,
                                             out=out.tensor((n_out, n)))
                    torch.cuda.synchronize()
                    out.check()
                    assert int(st[0].item()) == 0, (_name(src), frames, group, _name(dst), mode)
                    got = out.numpy((n_out, n))
                    assert _same(got, want), (_name(src), frames, group, _name(dst), mode)


BIG_FRAMES = 2**21 + 8                    # 2^53 / (2^32 - 1) < 2^21 + 1: the fewest frames of 32-bit pixels that sum to 2^53, and a few
BIG_TARGETS = [2**53 + 1, 2**53 + 3,      # float64 ties: down to even, up to even
               2**53 + 2**29 + 1,         # ONE BIT above a float32 halfway point no double holds: through double it is a tie
               2**53 + 3 * 2**29 + 1, 2**53 + 2**29 - 1, 2**53 + 2**29, 2**53, 2**53 - 1, 2**53 + 2, 2**52 + 2**28 + 1, 7, 0]


@pytest.mark.parametrize("src", [np.uint32, np.int32], ids=_name)
def test_decode_sum_ties_beyond_2_53(gpu, src):
    """A sum needs 54 bits before its conversion to double rounds at all, and before a conversion to float THROUGH double can
    differ from a single rounding: one group of 2^21 + 8 frames of 12 values (one block) of 32-bit pixels, every column's
    terms spread evenly so that the sum is the target exactly.  The stream comes from the GPU encoder (two million
    single-frame encodes by the oracle take minutes); the truth does not depend on it.  i32 pixels reach 2^52 only: their
    columns land on the targets halved where those are out of reach."""
    import torch
    from trpx_amd import codec
    lo, hi = ce.src_range(src)
    targets = [t if t <= BIG_FRAMES * hi else t // 2 for t in BIG_TARGETS]
    px = np.empty((BIG_FRAMES, len(targets)), np.int64)
    for c, t in enumerate(targets):
        base, rest = divmod(t, BIG_FRAMES)
        px[:, c] = base
        px[c: c + 2 * rest: 2, c] += 1                                            # (rest < frames / 2 for every target here)
        assert base + 1 <= hi and int(px[:, c].sum()) == t
    px = px.astype(src)
    n = px.shape[1]
    enc = codec.encode(to_dev(px), index=True)
    torch.cuda.synchronize()
    enc.check()
    for dst in (np.float32, np.float64, np.int64, np.int32):
        want = ce.truth(np.array([targets], dtype=object), dst)
        for mode in ("index", "offsets", "none"):
            out = _Guarded(n, dst)
            _, st = codec.decode_sum(enc.stack(), None if mode == "none" else enc.frame_offsets, n, BIG_FRAMES, src, BIG_FRAMES,
                                     out_dtype=torch_dt(dst), index=enc.index if mode == "index" else None, out=out.tensor((1, n)))
            torch.cuda.synchronize()
            out.check()
            assert int(st[0].item()) == 0, (_name(src), _name(dst), mode)
            assert _same(out.numpy((1, n)), want), (_name(src), _name(dst), mode, out.numpy((1, n)), want)
