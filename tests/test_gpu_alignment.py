"""GPU tests: every entry point at the weakest pointer alignment include/trpx_hip.h allows.

The header promises: pixels and pixels_out "aligned to T", terse "4-byte aligned", the consumers' outputs "aligned to their
type".  The kernels branch on the alignment they find (misalignment() -> plan_stack / plan_indexed, store_group_lines' c =
address & 127, k_encode_fused_mis2 from pixels & 2, vec in encode.hip / decode.hip, base16 in the stream windows, whole16 on
the dot maps), and every tensor of torch's allocator is 256-byte aligned: without these tests each branch is seen from one side.
Here every pointer is a view carved out of a larger tensor (tests/alignment.py) at the residues mod 128 where those branches
turn, with guards around it: 0xFF around what a call reads -- behind a stream from align4(total) on --, a position-dependent
pattern in and around what it writes.

The truth is always the original pixels and numpy on them (the codec is lossless); for encoded bytes it is oracle.encode_stack.
No GPU decoder is trusted, every comparison is exact.  The streams the decoders are given are the ORACLE's bytes; the decode
index is the GPU encoder's, whose stream has been compared with the oracle's first.

The routes (decode_plan.hpp; F = frames, S = 12 * 1024 + 5; every frame here has < 2^26 bits).  3 frames are fewer than the
position-parallel locator takes (4), so the form without offsets is Walk::kSerial + Extract::kBasic under every selector:

  stack                      form      selector      DecodePlan
  (3, S), (3, 12 * 1024)     offsets   0, 3, 4, 5    walk kNone, extract kFrames, defer, misaligned = frame bytes % 128 != 0
                                                     || out % 128 != 0 -- for (3, 12 * 1024) the output pointer ALONE (k_decode_frames
                                                     <T, LINES = true>); 5: dense = true.  Frames 1 (mod 4) change width on every
                                                     block: the walker lists them, launch_decode_deferred decodes them
                             offsets   1             walk kHeaders, extract kBasic
                             offsets   2             walk kSeg, extract kTiled
                             index     3             walk kCallers, extract kFramesIndexed
                             index     0, 1, 2, 4, 5 walk kCallers, extract kTiled (fewer than 1024 frames)
                             none      all           walk kSerial, extract kBasic
  (1024, 4096) 16 / 32 bit   index     0             walk kCallers, extract kFrames, misaligned, defer (frame bytes are a multiple of
                                                     128: the output pointer alone sends the stack to the walking decoder and
                                                     its hand-over list); residue 0 would be kFramesIndexed
  3 x (1030 x 1065)          offsets   0             walk kChain, extract kChainTiles (91 413 blocks < 2^18), parts > 1, defer,
  u16, i32                                           narrow for u16
                             offsets   2             walk kSeg, extract kTiled
                             offsets   4             walk kNone, extract kParts, parts > 1, defer
                             index     0, 2, 4       walk kCallers, extract kTiled
                             none      0, 2, 4       walk kSerial, extract kBasic
  2 x 2048^2 u8              offsets   0             walk kChain, extract kChainUnits (349 526 blocks >= 2^18, 1-byte pixels), narrow
                             offsets   2, 4          as above
                             index     0, 2, 4       walk kCallers, extract kUnitsIndexed (no selector moves large frames
                                                     of 8- / 16-bit pixels off it)
                             none      0, 2, 4       walk kSerial, extract kBasic
  64-bit containers, trpx_decode_convert             walk kHeaders, extract kConvert
  build_index                (3, ..): walk kFrames (selector 2: kSeg); large frames: walk kChain; check_index
  sum / roi / sparse / dot   index given: their own kernels alone; otherwise plan_index as build_index (and the serial locator)

The stream-base tests run the same calls with the stream at 4, 8, 12 and 68 mod 128 (mod 16: 4, 8, 12, 4) and an aligned
output, so that (base & 15) != 0 takes the guarded dword fills of every window (decode_frame.hip, part_walk.hpp, walk_lds.hpp,
unpack_tile.hpp) in place of the LDS-DMA / 16-byte ones."""
import functools

import numpy as np
import pytest

from alignment import RESIDUES, STREAM_RESIDUES, align_up, carve, carve_copy, carve_stream, same_bytes, to_bytes
from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import selected, to_dev, torch_dt

pytestmark = pytest.mark.gpu

S = 12 * 1024 + 5
WIDE = [np.uint64, np.int64]
SMALL = [(3, S), (3, 12 * 1024), (1, 3072 + 12), (2, 7), (2, 12)]
ROWS = {S: 647, 12 * 1024: 128, 1030 * 1065: 1065, 4096: 64, 2048 * 2048: 2048}      # row length of a frame, for the boxes
LARGE = [(np.uint16, 3, 1030 * 1065), (np.int32, 3, 1030 * 1065), (np.uint8, 2, 2048 * 2048)]
FORMS = ("offsets", "index", "none")
_name = lambda d: np.dtype(d).name


def large_residues(dtype):
    size = np.dtype(dtype).itemsize
    return (RESIDUES[size][0], 64 + size) if np.dtype(dtype) == np.uint8 else RESIDUES[size]


def ladder(dtype, frames: int, n: int) -> np.ndarray:
    """[frames, n] pixels: a width ladder per block, 0 up to the type's full width, both signs for signed types.  A block's
    first value is an extreme of its width (of either sign), so the width is exactly the ladder's.  Frames 1 (mod 4)
    change width on every block -- more than the walker's hand-over line of 2 changes in 9 blocks --, the others keep a width
    for 5 to 9 blocks.  Every frame's first and last pixel is an extreme of the type."""
    dt = np.dtype(dtype)
    bits, signed = 8 * dt.itemsize, dt.kind == "i"
    rng = np.random.default_rng(1000003 * bits + 7919 * frames + n + signed)
    nblk = -(-n // 12)
    b = np.arange(nblk)
    level = np.empty((frames, nblk), np.int64)
    minimum = np.empty((frames, nblk), bool)                 # signed: the block's first value is its width's minimum, else maximum
    for f in range(frames):
        if f % 4 == 1:
            level[f] = np.cumsum(rng.integers(1, bits + 1, size=nblk)) % (bits + 1)      # (a step is never 0 mod bits + 1)
            minimum[f] = b % 2 == 1
        else:
            run = (b + 2 * f) // (5 + f % 5)
            level[f] = run % (bits + 1)
            minimum[f] = (run // (bits + 1)) % 2 == 1        # one turn of the ladder with maxima, the next with minima
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    mask = np.where(level > 0, ones >> (64 - np.maximum(level, 1)).astype(np.uint64), np.uint64(0))     # level low bits
    sign = np.where(level > 0, np.uint64(1) << (np.maximum(level, 1) - 1).astype(np.uint64), np.uint64(0))
    r = rng.integers(0, 1 << 64, size=(frames, nblk, 12), dtype=np.uint64) & mask[:, :, None]
    if signed:
        r[:, :, 0] = np.where(minimum, sign, mask >> np.uint64(1))           # the width's maximum / minimum
        r = (r ^ sign[:, :, None]) - sign[:, :, None]                                    # sign extension (wraps mod 2^64)
    else:
        r[:, :, 0] = mask
    px = r.reshape(frames, nblk * 12)[:, :n].astype(np.dtype(f"u{dt.itemsize}")).view(dt).copy()
    info = np.iinfo(dt)
    px[0::2, 0], px[1::2, 0] = info.max, info.min if signed else info.max
    px[0::2, -1], px[1::2, -1] = info.min if signed else info.max, info.max
    px.setflags(write=False)
    return px


class Stack:
    """One stack of the tests: its pixels, the oracle's stream of it, and both on the device.  Made once, never changed."""

    def __init__(self, dtype, frames, n):
        from oracle import oracle as O
        self.dtype, self.frames, self.n = np.dtype(dtype), frames, n
        self.tdt = torch_dt(dtype)
        self.px = ladder(dtype, frames, n)
        self.O = O
        self._enc = {}
        self._dev = None

    def encoded(self, block=12):
        """(bytes, offsets int64 [frames + 1], prolix_bits): oracle.encode_stack."""
        if block not in self._enc:
            want, sizes, pb = self.O.encode_stack(self.px, block)
            offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))]).astype(np.int64)
            assert offs[-1] == want.size
            self._enc[block] = (want, offs, pb)
        return self._enc[block]

    @property
    def d_px(self):
        self.dev()
        return self._dev["px"]

    def dev(self):
        """{px, stream, offs, index} on the device, at the allocator's alignment.  index: the GPU encoder's own, None for
        64-bit containers; its stream is compared with the oracle's here."""
        if self._dev is None:
            import torch
            from trpx_amd import codec
            want, offs, pb = self.encoded()
            d = {"px": to_dev(self.px), "stream": to_dev(want), "offs": to_dev(offs), "index": None}
            if self.dtype.itemsize < 8:
                enc = codec.encode(d["px"], index=True)
                torch.cuda.synchronize()
                enc.check()
                same_bytes(enc.stack(), want, "the encoder's stream of the stack")
                d["index"] = enc.index
            self._dev = d
        return self._dev


@functools.lru_cache(maxsize=None)
def _stack(name, frames, n):
    return Stack(np.dtype(name), frames, n)


def stack(dtype, frames, n) -> Stack:
    return _stack(np.dtype(dtype).name, frames, n)


def _ok(status, what):
    import torch
    torch.cuda.synchronize()
    assert int(status[0].item()) == 0, (what, "status", int(status[0].item()))


def _mark(mark, label):
    if mark is not None:
        mark(label)


# ---- a. encoder input ---------------------------------------------------------------------------------------------------------
ENCODE_PATHS = {"single": ("trpx_set_encode_path", 0, 12), "twopass": ("trpx_set_encode_path", 1, 12),
                "generic": ("trpx_set_encode_path", 0, 7)}


def encode_cases(gpu, dtype, path, shapes=SMALL, residues=None, mark=None):
    import torch
    from trpx_amd import codec
    setter, value, block = ENCODE_PATHS[path]
    size = np.dtype(dtype).itemsize
    ws = codec.Workspace(gpu)
    with selected(setter, value):
        for frames, n in shapes:
            st = stack(dtype, frames, n)
            want, offs, pb = st.encoded(block)
            for off in residues or RESIDUES[size]:
                what = f"encode {path} {_name(dtype)} ({frames}, {n}) pixels at {off} mod 128"
                px, room, check = carve_copy(st.d_px, off)
                assert px.data_ptr() % 128 == off and px.is_contiguous()
                _mark(mark, what)
                enc = codec.encode(px, block=block, workspace=ws)
                torch.cuda.synchronize()
                enc.check()
                assert enc.total_bytes() == want.size, what
                same_bytes(enc.frame_offsets, offs, what + ": frame offsets")
                same_bytes(enc.stack(), want, what + ": stream")
                assert enc.prolix_bits() == pb, what
                check(what)
                same_bytes(px, st.px, what + ": the pixels themselves")


@pytest.mark.parametrize("path", sorted(ENCODE_PATHS))
@pytest.mark.parametrize("dtype", DTYPES + WIDE, ids=_name)
def test_encoder_input_at_every_residue(gpu, oracle, dtype, path):
    """The pixels at every residue of their type (64-bit containers: 8), 0xFF around them, through the single-pass encoder
    (k_encode_fused; 16-bit pixels at 2 mod 4 with more than one frame: k_encode_fused_mis2, whose realigned loads read the
    dword in front of a block -- at the stack's first pixel that dword is guard), the two-pass pipeline (vec = n % 4 == 0 &&
    pixels % 16 == 0 is cleared by the pointer alone for n = 12 * 1024) and the generic kernels (block 7; 64-bit containers
    under every path).  (1, 3084): one frame, so mis2 is off and the plain loads run at 2 mod 4.  Stream, frame offsets and
    prolix_bits against the oracle."""
    encode_cases(gpu, dtype, path)


def encode_exact_capacity(gpu, dtype, path, shape=(3, S), residues=(16, 112), mark=None):
    import torch
    from trpx_amd import codec
    setter, value, block = ENCODE_PATHS[path]
    st = stack(dtype, *shape)
    want, offs, pb = st.encoded(block)
    total = want.size
    with selected(setter, value):
        roomy = codec.encode(st.d_px, block=block)
        torch.cuda.synchronize()
        roomy.check()
        assert roomy.total_bytes() == total
        for off in residues:
            what = f"encode {path} {_name(dtype)} {shape} out at {off} mod 128, capacity align4({total})"
            out, room, check = carve(align_up(total, 4), torch.uint8, off, gpu)
            _mark(mark, what)
            enc = codec.encode(st.d_px, out=out, block=block)
            torch.cuda.synchronize()
            assert int(enc.status[0].item()) == 0, what
            enc.check()
            same_bytes(enc.frame_offsets, offs, what + ": frame offsets")
            same_bytes(out[:total], want, what + ": stream")
            assert not to_bytes(out[total:]).any(), what + ": bytes [total, align4(total)) are zeroed"
            assert enc.prolix_bits() == pb, what
            check(what)


@pytest.mark.parametrize("path", sorted(ENCODE_PATHS))
def test_encoder_output_of_exactly_the_stacks_size(gpu, oracle, path):
    """out at 16 and 112 mod 128 with out_capacity = align_up(total, 4) exactly, total from a first, roomy call: status 0, the
    oracle's bytes, and "nothing beyond out_capacity is ever touched" -- the fitting side of
    test_capacity_error_and_sizes_only_query."""
    for dtype in (np.uint16, np.int32, np.uint8):
        encode_exact_capacity(gpu, dtype, path)


# ---- b. / c. decoder output and stream base ------------------------------------------------------------------------------------
def decode_cases(gpu, dtype, sel, shapes, carved, forms=FORMS, residues=None, mark=None):
    """codec.decode under selector `sel`, in the input forms `forms`, with the output (carved = "out") or the stream (carved =
    "stream") at every residue and the other one at residue 0; both lie in carved rooms."""
    from trpx_amd import codec
    size = np.dtype(dtype).itemsize
    ws = codec.Workspace(gpu)
    with selected("trpx_set_decode_path", sel):
        for frames, n in shapes:
            st = stack(dtype, frames, n)
            d = st.dev()
            for off in residues or (RESIDUES[size] if carved == "out" else STREAM_RESIDUES):
                terse, _, tcheck = carve_stream(d["stream"], off if carved == "stream" else 0)
                for form in forms:
                    what = f"decode selector {sel} {form} {_name(dtype)} ({frames}, {n}) {carved} at {off} mod 128"
                    out, room, check = carve(st.px.nbytes, st.tdt, off if carved == "out" else 0, gpu)
                    _mark(mark, what)
                    back, status = codec.decode(terse, None if form == "none" else d["offs"], n, frames, st.tdt, out=out,
                                                workspace=ws, index=d["index"] if form == "index" else None)
                    _ok(status, what)
                    same_bytes(out, st.px, what)
                    check(what)
                tcheck(f"stream of {_name(dtype)} ({frames}, {n}) at {off}")


@pytest.mark.parametrize("sel", range(6))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_decoder_output_at_every_residue(gpu, oracle, dtype, sel):
    """pixels_out at every residue of its type, prefilled with the pattern like its guards: every pixel, and nothing else,
    written.  (3, S): frames start inside a line; (3, 12 * 1024): out_misaligned alone decides (the table above)."""
    decode_cases(gpu, dtype, sel, [(3, S), (3, 12 * 1024)], "out")


@pytest.mark.parametrize("sel", range(6))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_stream_base_at_every_residue(gpu, oracle, dtype, sel):
    """terse at 4, 8, 12 and 68 mod 128 with 0xFF from align4(total) on: the dword fills of every stream window, and no
    dependence on a byte behind the stream."""
    decode_cases(gpu, dtype, sel, [(3, S), (3, 12 * 1024)], "stream")


@pytest.mark.parametrize("carved", ["out", "stream"])
@pytest.mark.parametrize("dtype", [np.uint16, np.int16, np.uint32, np.int32], ids=_name)
def test_a_thousand_frames_with_the_index(gpu, oracle, dtype, carved):
    """(1024, 4096) through trpx_decode_indexed under selector 0: the n_frames >= 1024 line of plan_indexed.  Frame bytes are a
    multiple of 128, so a misaligned output alone moves the stack onto the walking decoder and its hand-over list (every
    fourth frame is listed); with the stream carved the output is aligned and k_decode_frames_indexed runs."""
    decode_cases(gpu, dtype, 0, [(1024, 4096)], carved, forms=("index",))


@pytest.mark.parametrize("carved", ["out", "stream"])
@pytest.mark.parametrize("sel", [0, 2, 4])
@pytest.mark.parametrize("dtype,frames,n", LARGE, ids=lambda v: _name(v) if isinstance(v, type) else str(v))
def test_large_frames(gpu, oracle, dtype, frames, n, sel, carved):
    """Frames of more than 32 K blocks (Walk::kChain + kChainTiles; 2 x 2048^2 u8, at least 2^18 blocks: kChainUnits /
    kUnitsIndexed -- two residues there), the tiled route and round 4's parts route."""
    residues = large_residues(dtype) if carved == "out" else (STREAM_RESIDUES if np.dtype(dtype) != np.uint8 else (4, 68))
    decode_cases(gpu, dtype, sel, [(frames, n)], carved, residues=residues)


CONVERT = [("uint16", "float32", 4), ("uint16", "float64", 8), ("uint16", "uint8", 1), ("int64", "int64", 8)]


def convert_case(gpu, src, dst, off, stream_off=0, mark=None):
    import torch
    from trpx_amd import _lib, codec
    L = _lib.lib()
    st = stack(src, 3, S)
    d = st.dev()
    code = {"float32": _lib.F32, "float64": _lib.F64, "uint8": _lib.U8, "int64": _lib.I64}[dst]
    ddt = np.dtype(dst)
    want = st.px.astype(ddt) if ddt.kind == "f" or ddt.itemsize >= st.dtype.itemsize \
        else np.clip(st.px, np.iinfo(ddt).min, np.iinfo(ddt).max).astype(ddt)
    what = f"convert {src} -> {dst} out at {off}, stream at {stream_off} mod 128"
    terse, _, tcheck = carve_stream(d["stream"], stream_off)
    out, room, check = carve(want.nbytes, torch_dt(dst), off, gpu)
    status = torch.empty(_lib.STATUS_WORDS, dtype=torch.int32, device=gpu)
    ws_bytes = max(L.trpx_decode_workspace_bytes(c, S, 3, 12) for c in (_lib.U8, _lib.U32, _lib.U64))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
    signed = int(st.dtype.kind == "i")
    _mark(mark, what)
    if src == dst:       # a 64-bit container through trpx_decode
        _lib.check(L.trpx_decode(signed, code, terse.data_ptr(), terse.numel(), d["offs"].data_ptr(), S, 3, 12, out.data_ptr(),
                                 status.data_ptr(), ws.data_ptr(), ws.numel(), codec._stream_ptr(terse)))
    else:
        _lib.check(L.trpx_decode_convert(signed, code, terse.data_ptr(), terse.numel(), d["offs"].data_ptr(), S, 3, 12,
                                         out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), codec._stream_ptr(terse)))
    _ok(status, what)
    same_bytes(out, want, what)
    check(what)
    tcheck(what)


@pytest.mark.parametrize("src,dst,off", CONVERT, ids=[f"{a}-{b}" for a, b, _ in CONVERT])
def test_converting_decode_and_64_bit_containers(gpu, oracle, src, dst, off):
    """trpx_decode_convert of a u16 stream into f32 at 4, f64 at 8 and u8 (clamped) at 1, and an i64 stream into i64 at 8: with
    the output carved, then with the stream at each of its residues (walk kHeaders, extract kConvert)."""
    convert_case(gpu, src, dst, off)
    for stream_off in STREAM_RESIDUES:
        convert_case(gpu, src, dst, 0, stream_off)


def index_region(st: Stack, index) -> np.ndarray:
    """The index proper: 8 bytes per 256-block group, then (16-byte aligned) a width byte per block.  What lies behind is the
    scratch of whatever wrote it."""
    nblk = -(-st.n // 12)
    groups = 8 * st.frames * (-(-nblk // 256))
    b = to_bytes(index)
    w = align_up(groups, 16)
    return np.concatenate([b[:groups], b[w: w + st.frames * nblk]])


INDEX_STACKS = [(dt, 3, S) for dt in DTYPES] + [(dt, 3, 12 * 1024) for dt in DTYPES] + [(np.uint16, 3, 1030 * 1065),
                                                                                       (np.int32, 3, 1030 * 1065)]


def build_index_cases(gpu, stacks=INDEX_STACKS, residues=STREAM_RESIDUES, sels=(0, 2), mark=None):
    import torch
    from trpx_amd import codec
    for dtype, frames, n in stacks:
        st = stack(dtype, frames, n)
        d = st.dev()
        want = index_region(st, d["index"])
        widths = np.stack([st.O.widths(st.px[f]) for f in range(frames)]).astype(np.uint8).reshape(-1)
        assert np.array_equal(want[-widths.size:], widths), "the encoder's own index against oracle.widths"
        for off in residues:
            terse, _, tcheck = carve_stream(d["stream"], off)
            for sel in sels:
                what = f"build_index selector {sel} {_name(dtype)} ({frames}, {n}) stream at {off} mod 128"
                with selected("trpx_set_decode_path", sel):
                    _mark(mark, what)
                    got = codec.build_index(terse, d["offs"], n, frames, st.tdt)
                    torch.cuda.synchronize()
                same_bytes(index_region(st, got), want, what)
            tcheck(what)


def test_build_index_from_a_stream_at_every_residue(gpu, oracle):
    """trpx_build_index (walk kFrames; selector 2: kSeg; large frames: kChain) against the encoder's own index -- group
    offsets and widths, the widths also against oracle.widths."""
    build_index_cases(gpu)


LOCATE_STACKS = [(np.uint8, 3, S), (np.int16, 3, S), (np.int32, 3, 12 * 1024), (np.uint16, 1024, 4096), (np.int32, 1024, 4096),
                 (np.uint16, 3, 1030 * 1065)]


def locate_cases(gpu, stacks=LOCATE_STACKS, residues=STREAM_RESIDUES, mark=None):
    from trpx_amd import codec
    for dtype, frames, n in stacks:
        st = stack(dtype, frames, n)
        d = st.dev()
        _, offs, _ = st.encoded()
        for off in residues:
            terse, _, tcheck = carve_stream(d["stream"], off)
            for path in (0, 1):
                what = f"locate_frames path {path} {_name(dtype)} ({frames}, {n}) stream at {off} mod 128"
                out, room, check = carve(8 * (frames + 1), torch_dt(np.int64), 8, gpu)
                with selected("trpx_set_locate_path", path):
                    _mark(mark, what)
                    _, status = codec.locate_frames(terse, n, frames, st.tdt, out=out)
                    _ok(status, what)
                same_bytes(out, offs, what)
                check(what)
            tcheck(what)


def test_locate_frames_in_a_stream_at_every_residue(gpu, oracle):
    """trpx_locate_frames on both paths (0: position-parallel from 4 frames and 8 KB on -- the (1024, 4096) stacks, whose
    16-byte loads start at whatever base they are given; 1: the serial walk), offsets written at 8 mod 128, against the
    oracle's frame sizes."""
    locate_cases(gpu)


# ---- consumers -----------------------------------------------------------------------------------------------------------------
def sum_truth(px, group):
    p = px.astype(np.int64)
    return np.stack([p[j: j + group].sum(axis=0) for j in range(0, px.shape[0], group)])


def boxes_of(st: Stack):
    """Boxes at the frames' corners: the first rows of frame 0 and the last rows of the last frame included."""
    w = ROWS[st.n]
    h = st.n // w
    bh, bw = min(3, h), min(37, w)
    rows = [(0, 0, 0), (st.frames - 1, h - bh, w - bw), (1 % st.frames, h // 2, (w - bw) // 2), (st.frames - 1, h - bh, 0)]
    return np.array(rows, np.int32), (bh, bw), w


def roi_truth(st: Stack, rows, shape, w):
    bh, bw = shape
    return np.stack([st.px[f].reshape(-1, w)[y: y + bh, x: x + bw] for f, y, x in rows])


def threshold_of(st: Stack) -> int:
    return 1 << (8 * st.dtype.itemsize - 2)


def sparse_truth(st: Stack, thr):
    pos = [np.flatnonzero(st.px[f].astype(np.int64) >= thr) for f in range(st.frames)]
    rows = np.concatenate([[0], np.cumsum([p.size for p in pos])]).astype(np.int64)
    return rows, np.concatenate(pos).astype(np.uint32), np.concatenate([st.px[f][p] for f, p in enumerate(pos)])


def maps_of(st: Stack) -> np.ndarray:
    rng = np.random.default_rng(st.n)
    m = rng.integers(-3, 4, size=(3, st.n)).astype(np.int32)
    m[1] = np.arange(st.n) % ROWS[st.n]                      # the x map of a centre of mass
    m[:, 0], m[:, -1] = 1, -1                                # the frames' extreme first and last pixels count
    return m


def dot_truth(st: Stack, m):
    with np.errstate(over="ignore"):
        return (st.px.astype(np.int64)[:, None, :] * m.astype(np.int64)[None, :, :]).sum(axis=2)


def _form(d, form):
    return (None if form == "none" else d["offs"]), (d["index"] if form == "index" else None)


def consumer_cases(gpu, dtype, frames, n, stream_residues, out_residues, mark=None):
    """decode_sum / _roi / _sparse / _dot in their three input forms: the stream at each of `stream_residues`, the outputs at the
    residues `out_residues` = (the type's, 4, 8) -- 0: aligned.  Every output lies in a carved room."""
    import torch
    from trpx_amd import codec
    st = stack(dtype, frames, n)
    d = st.dev()
    t_off, off4, off8 = out_residues
    ws = codec.Workspace(gpu)
    sums = {np.int64: sum_truth(st.px, 2)}
    info = np.iinfo(np.int32)
    sums[np.int32] = np.clip(sums[np.int64], info.min, info.max).astype(np.int32)
    rows, box_shape, width = boxes_of(st)
    boxes = to_dev(rows)
    roi = roi_truth(st, rows, box_shape, width)
    thr = threshold_of(st)
    s_rows, s_pos, s_val = sparse_truth(st, thr)
    n_ev = int(s_rows[-1])
    assert 0 < n_ev < st.px.size
    maps = maps_of(st)
    d_maps = to_dev(maps)
    dots = dot_truth(st, maps)
    for s_off in stream_residues:
        terse, _, tcheck = carve_stream(d["stream"], s_off)
        for form in FORMS:
            offs, index = _form(d, form)
            tag = f"{form} {_name(dtype)} ({frames}, {n}) stream at {s_off}, outputs at {out_residues} mod 128"
            for odt, o_off in ((np.int32, off4), (np.int64, off8)):
                what = f"decode_sum into {_name(odt)} {tag}"
                out, room, check = carve(sums[odt].nbytes, torch_dt(odt), o_off, gpu)
                _mark(mark, what)
                _, status = codec.decode_sum(terse, offs, n, frames, st.tdt, 2, out_dtype=torch_dt(odt), index=index, out=out, workspace=ws)
                _ok(status, what)
                same_bytes(out, sums[odt], what)
                check(what)
            what = f"decode_roi {tag}"
            out, room, check = carve(roi.nbytes, st.tdt, t_off, gpu)
            _mark(mark, what)
            _, status = codec.decode_roi(terse, offs, n, frames, st.tdt, width, boxes, box_shape, index=index,
                                         out=out.view(roi.shape), workspace=ws)
            _ok(status, what)
            same_bytes(out, roi, what)
            check(what)
            what = f"decode_sparse {tag}"
            r_out, _, r_check = carve(s_rows.nbytes, torch_dt(np.int64), off8, gpu)
            p_out, _, p_check = carve(4 * n_ev, torch_dt(np.uint32), off4, gpu)
            v_out, _, v_check = carve(s_val.nbytes, st.tdt, t_off, gpu)
            _mark(mark, what)
            _, _, _, status = codec.decode_sparse(terse, offs, n, frames, st.tdt, thr, index=index, capacity=n_ev, row_offsets=r_out,
                                                  positions=p_out, values=v_out, workspace=ws)
            _ok(status, what)
            for got, want, chk, part in ((r_out, s_rows, r_check, "row_offsets"), (p_out, s_pos, p_check, "positions"),
                                         (v_out, s_val, v_check, "values")):
                same_bytes(got, want, f"{what}: {part}")
                chk(f"{what}: {part}")
            what = f"decode_dot {tag}"
            out, room, check = carve(dots.nbytes, torch_dt(np.int64), off8, gpu)
            _mark(mark, what)
            _, status = codec.decode_dot(terse, offs, n, frames, st.tdt, d_maps, index=index, out=out.view(dots.shape), workspace=ws)
            _ok(status, what)
            same_bytes(out, dots, what)
            check(what)
        tcheck(f"stream of {tag}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_consumers_on_a_stream_at_every_residue(gpu, oracle, dtype):
    """decode_sum, decode_roi, decode_sparse and decode_dot on (3, S) with the stream at 4, 8, 12 and 68 mod 128."""
    consumer_cases(gpu, dtype, 3, S, STREAM_RESIDUES, (0, 0, 0))


def test_consumers_on_large_frames_at_every_stream_residue(gpu, oracle):
    """The same on 3 x (1030 x 1065) u16: the index is built by the chain walk where none is given."""
    consumer_cases(gpu, np.uint16, 3, 1030 * 1065, STREAM_RESIDUES, (0, 0, 0))


@pytest.mark.parametrize("dtype", [np.uint16, np.int32], ids=_name)
def test_consumer_outputs_at_the_alignment_of_their_type(gpu, oracle, dtype):
    """(3, S): decode_sum into int32 at 4 and int64 at 8, decode_roi's out and decode_sparse's values at the pixel type's
    smallest residue, its positions at 4, its row_offsets and decode_dot's out at 8 mod 128."""
    consumer_cases(gpu, dtype, 3, S, (0,), (RESIDUES[np.dtype(dtype).itemsize][0], 4, 8))


def encode_sparse_case(gpu, dtype, mark=None):
    import torch
    from trpx_amd import codec
    st = stack(dtype, 3, S)
    thr = threshold_of(st)
    spx = np.where(st.px.astype(np.int64) >= thr, st.px, 0).astype(st.dtype)      # what the events stand for
    s_rows, s_pos, s_val = sparse_truth(st, thr)
    want, sizes, pb = st.O.encode_stack(spx)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))]).astype(np.int64)
    t_off = RESIDUES[st.dtype.itemsize][0]
    what = f"encode_sparse {_name(dtype)} (3, {S}): row_offsets at 8, positions at 4, values at {t_off} mod 128"
    rows, _, r_check = carve_copy(to_dev(s_rows), 8)
    pos, _, p_check = carve_copy(to_dev(s_pos), 4)
    val, _, v_check = carve_copy(to_dev(s_val), t_off)
    assert rows.data_ptr() % 128 == 8 and pos.data_ptr() % 128 == 4 and val.data_ptr() % 128 == t_off
    _mark(mark, what)
    enc = codec.encode_sparse(rows, pos, val, S, 3, st.tdt)
    torch.cuda.synchronize()
    enc.check()
    assert enc.total_bytes() == want.size, what
    same_bytes(enc.frame_offsets, offs, what + ": frame offsets")
    same_bytes(enc.stack(), want, what + ": stream")
    assert enc.prolix_bits() == pb, what
    for chk in (r_check, p_check, v_check):
        chk(what)


@pytest.mark.parametrize("dtype", [np.uint16, np.int32], ids=_name)
def test_encode_sparse_from_events_at_the_alignment_of_their_type(gpu, oracle, dtype):
    """trpx_encode_sparse with 0xFF around its three lists: the stream of the events' dense frames, from the oracle."""
    encode_sparse_case(gpu, dtype)
