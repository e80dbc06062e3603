"""CPU tier: trpx_decode_reduce's four symbols are exported and bound, its workspace size and its chunk count are arithmetic
(trpx_decode_sum's launch plan), its argument errors are return codes decided before any device call (the pointers below are
fake, aligned addresses: a call that reached the device would fail differently), and what the op decides
(trpx_amd/csrc/reduce_ops.hpp) is clean under ASan + UBSan in a stand-alone CPU program."""
import ctypes as C
import os
import subprocess

import pytest

from trpx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VALUES, N_FRAMES, TERSE_BYTES = 512 * 512, 8, 1 << 20
TERSE, OFFS, INDEX, OUT, STATUS, WS = 0x10000, 0x20000, 0x30000, 0x50000, 0x70000, 0x80000
OPS = (_lib.REDUCE_MAX, _lib.REDUCE_MIN, _lib.REDUCE_SUMSQ, _lib.REDUCE_COUNT_GE)
STREAM_DTYPES = (_lib.U8, _lib.I8, _lib.U16, _lib.I16, _lib.U32, _lib.I32)
TARGET_UNITS, SUB_TILES = 1024, 2                           # workgroups a launch aims at, 256-block groups per tile (decode_sum.hpp)


def L():
    return _lib.lib()


def _reduce(dtype=_lib.U16, op=_lib.REDUCE_MAX, terse=TERSE, terse_bytes=TERSE_BYTES, offs=OFFS, index=INDEX, n_values=N_VALUES,
            n_frames=N_FRAMES, block=12, group=2, threshold=0, out=OUT, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_reduce(dtype, op, terse, terse_bytes, offs, index, n_values, n_frames, block, group, threshold, out, status,
                                  ws, ws_bytes, None)


def _sum_plan(dtype, n_values, n_frames, group):
    """(chunks, frames per chunk, tiles per frame, outputs) of trpx_decode_sum's launch plan"""
    n_blocks = -(-n_values // 12)
    tpf = -(-n_blocks // (SUB_TILES * 256))
    n_out = -(-n_frames // group)
    per_group = min(group, n_frames)
    units = n_out * tpf
    chunks = min(-(-TARGET_UNITS // units) if units < TARGET_UNITS else 1, per_group)
    fpc = min(-(-per_group // chunks), 0xFFFFFFFF if dtype >= _lib.U32 else 65535)
    return -(-per_group // fpc), fpc, tpf, n_out


def test_symbols_are_exported_and_bound():
    names = ("trpx_decode_reduce_workspace_bytes", "trpx_decode_reduce_chunks", "trpx_decode_reduce", "trpx_decode_reduce_host")
    for name in names:
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L(), name).restype == _lib.SYMBOLS[name][0]
    _P, _SZ, _U, _I, _I64 = C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_int64
    assert _lib.SYMBOLS["trpx_decode_reduce_workspace_bytes"] == (_SZ, [_I, _I, _SZ, _SZ, _SZ, _U, _U])
    assert _lib.SYMBOLS["trpx_decode_reduce_chunks"] == (_U, [_I, _SZ, _SZ, _U])
    assert _lib.SYMBOLS["trpx_decode_reduce"] == (_I, [_I, _I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _U, _I64, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_reduce_host"] == (_I, [_I, _I, _P, _SZ, _P, _SZ, _SZ, _U, _U, _I64, _P, _I])
    assert OPS == (0, 1, 2, 3)
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_header_declares_them_and_lists_the_call_under_restated_widths():
    text = open(os.path.join(ROOT, "include", "trpx_hip.h")).read()
    for name in ("size_t trpx_decode_reduce_workspace_bytes(", "unsigned trpx_decode_reduce_chunks(", "int trpx_decode_reduce(",
                 "int trpx_decode_reduce_host(",
                 "TRPX_REDUCE_MAX = 0, TRPX_REDUCE_MIN = 1, TRPX_REDUCE_SUMSQ = 2, TRPX_REDUCE_COUNT_GE = 3"):
        assert name in text
    top = text[text.index("Restated widths."):text.index("Status 0 with pixels that are not the stream's")]
    assert "trpx_decode_reduce" in top
    assert "#define TRPX_ABI_VERSION 3" in text


def test_workspace_bytes_is_arithmetic():
    f = L().trpx_decode_reduce_workspace_bytes
    for op in OPS:
        n = f(_lib.U16, op, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 2)
        assert n > 0 and n % 8 == 0
        assert n >= L().trpx_index_bytes(_lib.U16, N_VALUES, N_FRAMES, 12)        # (index built in the workspace)
        assert f(_lib.U16, op, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 0) == 0        # group 0
        assert f(_lib.U16, op, TERSE_BYTES, N_VALUES, N_FRAMES, 7, 2) == 0         # block 7
        assert f(_lib.U64, op, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 2) == 0        # 64-bit container
        assert f(_lib.F32, op, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 2) == 0        # not a stream type
        assert f(_lib.U16, op, 0, N_VALUES, N_FRAMES, 12, 2) == 0
        # few outputs: the frames are split into chunks, whose partial accumulators need room
        assert f(_lib.U16, op, TERSE_BYTES, N_VALUES, 2000, 12, 2000) > f(_lib.U16, op, TERSE_BYTES, N_VALUES, 2000, 12, 1)
    assert f(_lib.U16, 4, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 2) == 0             # unknown op
    assert f(_lib.U16, -1, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 2) == 0
    # one chunk: the front alone, whatever the op; split: 64-bit accumulators need twice the slab of 32-bit ones
    front = L().trpx_decode_roi_workspace_bytes(_lib.U16, TERSE_BYTES, N_VALUES, 2000, 12)
    assert all(f(_lib.U16, op, TERSE_BYTES, N_VALUES, 2000, 12, 1) == front for op in OPS)
    chunks = L().trpx_decode_reduce_chunks(_lib.U16, N_VALUES, 2000, 2000)
    assert chunks > 1
    slab32, slab64 = (f(_lib.U16, op, TERSE_BYTES, N_VALUES, 2000, 12, 2000) - front for op in (_lib.REDUCE_MAX, _lib.REDUCE_SUMSQ))
    assert slab32 == -(-chunks * N_VALUES * 4 // 256) * 256 and slab64 == -(-chunks * N_VALUES * 8 // 256) * 256
    assert f(_lib.U16, _lib.REDUCE_SUMSQ, TERSE_BYTES, N_VALUES, 2000, 12, 2000) >= f(_lib.U16, _lib.REDUCE_MAX, TERSE_BYTES, N_VALUES, 2000, 12, 2000)
    assert f(_lib.U16, _lib.REDUCE_MIN, TERSE_BYTES, N_VALUES, 2000, 12, 2000) == f(_lib.U16, _lib.REDUCE_COUNT_GE, TERSE_BYTES, N_VALUES, 2000, 12, 2000)


# (frames, values), group, chunks: the plan paths and the empty-chunk case of the GPU tier, the flagship stack, a frame of many tiles
@pytest.mark.parametrize("shape, group, want", [
    ((2100, 40), 2, 1),                                     # 1050 units: one chunk of two frames
    ((2100, 40), 2100, 700),                                # one output: 700 chunks of 3
    ((40, 6144 * 30), 40, 20),                              # 30 full tiles: 20 chunks of 2
    ((11, 7), 10, 10),                                      # 10 chunks of one frame; the last output has nine empty ones
    ((2000, 512 * 512), 10, 1), ((2000, 512 * 512), 2000, 24), ((500, 512 * 512), 10, 1), ((9, 7), 3, 3), ((3, 6144 + 3072 + 5), 4, 3),
    ((2, 4096 * 4096), 2, 1), ((1, 13), 1, 1),
])
def test_chunks_are_the_summing_decode_s_plan(shape, group, want):
    for dtype in STREAM_DTYPES:
        chunks, fpc, tpf, n_out = _sum_plan(dtype, shape[1], shape[0], group)
        assert L().trpx_decode_reduce_chunks(dtype, shape[1], shape[0], group) == chunks == want, (dtype, fpc, tpf, n_out)
    chunks, fpc, _, _ = _sum_plan(_lib.U16, shape[1], shape[0], group)
    assert (chunks - 1) * fpc < min(group, shape[0]) <= chunks * fpc           # every chunk of a full group has a frame


def test_chunks_is_zero_for_sizes_no_call_takes():
    f = L().trpx_decode_reduce_chunks
    assert f(_lib.U16, 0, 8, 2) == 0 and f(_lib.U16, N_VALUES, 0, 2) == 0 and f(_lib.U16, N_VALUES, 8, 0) == 0
    assert f(_lib.U64, N_VALUES, 8, 2) == 0 and f(_lib.F32, N_VALUES, 8, 2) == 0 and f(42, N_VALUES, 8, 2) == 0 and f(-1, N_VALUES, 8, 2) == 0
    assert f(_lib.U32, 1 << 28, 1, 1) == 0                  # frames of >= 2^32 bits
    assert f(_lib.U16, N_VALUES, 8, 2) > 0


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(block=0), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U32, n_values=1 << 28), _lib.ERR_UNSUPPORTED),              # frames of >= 2^32 bits
    # TRPX_ERR_INVALID_ARG
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),            # float dtype: not a stream type
    (dict(dtype=_lib.F64), _lib.ERR_INVALID_ARG),
    (dict(dtype=42), _lib.ERR_INVALID_ARG),                  # unknown dtype
    (dict(dtype=-1), _lib.ERR_INVALID_ARG),
    (dict(op=4), _lib.ERR_INVALID_ARG),                      # unknown op
    (dict(op=-1), _lib.ERR_INVALID_ARG),
    (dict(op=42), _lib.ERR_INVALID_ARG),
    (dict(group=0), _lib.ERR_INVALID_ARG),
    (dict(n_values=0), _lib.ERR_INVALID_ARG),                # bad sizes
    (dict(n_frames=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=4, n_frames=5), _lib.ERR_INVALID_ARG), # more frames than bytes
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(out=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 1), _lib.ERR_INVALID_ARG),                                   # u16 elements at an odd byte
    (dict(out=OUT + 2, dtype=_lib.I32), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 2, dtype=_lib.U8, op=_lib.REDUCE_COUNT_GE), _lib.ERR_INVALID_ARG),   # uint32 counts
    (dict(out=OUT + 4, dtype=_lib.U8, op=_lib.REDUCE_SUMSQ), _lib.ERR_INVALID_ARG),      # uint64 sums
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    (dict(index=None, ws=None), _lib.ERR_INVALID_ARG),       # a form that needs a workspace, without one
    (dict(offs=None, index=None, ws=None), _lib.ERR_INVALID_ARG),
    (dict(n_frames=2000, group=2000, ws=None, ws_bytes=1 << 40), _lib.ERR_INVALID_ARG),   # an index given, but the plan splits
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),       # workspace too small for the index
    (dict(ws_bytes=0, index=None, offs=None), _lib.ERR_CAPACITY),
    (dict(n_frames=2000, group=2000, ws_bytes=0), _lib.ERR_CAPACITY),            # ... for the partial slab
])
def test_argument_errors_are_return_codes(kw, code):
    assert _reduce(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_reduce")


def test_legal_calls_pass_every_check():
    # every check passed: the first thing to fail is the workspace of the form without an index, which is one word long
    for dtype in STREAM_DTYPES:
        for op in OPS:
            for thr in (0, -(1 << 63), (1 << 63) - 1):
                assert _reduce(dtype=dtype, op=op, threshold=thr, index=None, ws_bytes=8) == _lib.ERR_CAPACITY, (dtype, op)
    es = {_lib.U8: 1, _lib.I8: 1, _lib.U16: 2, _lib.I16: 2, _lib.U32: 4, _lib.I32: 4}
    for dtype in STREAM_DTYPES:                             # aligned to the element only
        assert _reduce(dtype=dtype, out=OUT + es[dtype], index=None, ws_bytes=8) == _lib.ERR_CAPACITY
        assert _reduce(dtype=dtype, op=_lib.REDUCE_COUNT_GE, out=OUT + 4, index=None, ws_bytes=8) == _lib.ERR_CAPACITY
        assert _reduce(dtype=dtype, op=_lib.REDUCE_SUMSQ, out=OUT + 8, index=None, ws_bytes=8) == _lib.ERR_CAPACITY
    for kw in (dict(group=1), dict(group=N_FRAMES + 5), dict(group=0xFFFFFFFF), dict(n_values=7), dict(n_values=1030 * 1065)):
        assert _reduce(index=None, ws_bytes=8, **kw) == _lib.ERR_CAPACITY, kw


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n_values, n_frames, group", [(N_VALUES, N_FRAMES, 2), (N_VALUES, 2000, 2000), (122880, 3, 3)])
def test_workspace_one_word_short(op, n_values, n_frames, group):
    need = L().trpx_decode_reduce_workspace_bytes(_lib.U16, op, TERSE_BYTES, n_values, n_frames, 12, group)
    kw = dict(op=op, n_values=n_values, n_frames=n_frames, group=group)
    assert _reduce(offs=None, index=None, ws_bytes=need - 8, **kw) == _lib.ERR_CAPACITY      # without offsets: the whole need
    assert L().trpx_last_error_string().startswith(b"trpx_decode_reduce")
    # with offsets given less is needed, and the call checks against its own form's need: the index has to fit
    idx = L().trpx_index_bytes(_lib.U16, n_values, n_frames, 12)
    assert 0 < idx <= need
    assert _reduce(index=None, ws_bytes=idx // 2, **kw) == _lib.ERR_CAPACITY


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    out = (C.c_uint64 * 64)()

    def host(dtype=_lib.U16, op=_lib.REDUCE_MAX, block=12, n_values=12, group=1, out=out, terse=buf, terse_bytes=64, n_frames=2):
        return L().trpx_decode_reduce_host(dtype, op, terse, terse_bytes, None, n_values, n_frames, block, group, 0, out, -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=_lib.U32, n_values=1 << 28, terse_bytes=1 << 30), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(op=4), _lib.ERR_INVALID_ARG), (dict(op=-1), _lib.ERR_INVALID_ARG), (dict(group=0), _lib.ERR_INVALID_ARG),
                     (dict(n_values=0), _lib.ERR_INVALID_ARG), (dict(n_frames=0), _lib.ERR_INVALID_ARG), (dict(n_frames=65), _lib.ERR_INVALID_ARG),
                     (dict(out=None), _lib.ERR_INVALID_ARG), (dict(terse=None), _lib.ERR_INVALID_ARG), (dict(terse_bytes=0), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_decode_reduce_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device


def test_ops_under_the_sanitizers():
    """reduce_ops.hpp -- the text the kernels run -- for every (pixel type, op): a model of the call over heap arrays of exactly
    the partial slab's and the output's elements, every chunk split including chunks without frames, the type's minimum and
    maximum, INT32_MIN squared, sums of squares that wrap 2^64, thresholds at and beyond the type's limits, against a direct
    loop in 128-bit arithmetic, under ASan + UBSan (a stand-alone CPU program)."""
    exe = os.path.join(ROOT, "tests", "cpp", "reduce_sanitize")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "reduce_example.mk", "reduce_sanitize"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK reduce_sanitize" in r.stdout, r.stdout + r.stderr
