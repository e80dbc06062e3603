"""CPU tier: trpx_decode_sum_labelled's four symbols are exported and bound, its workspace size and its frames per chunk are
arithmetic (restated in tests/labelled_truth.py), its argument errors are return codes decided before any device call, in
trpx_decode_sum's order (the pointers below are fake, aligned addresses: a call that reached the device would fail
differently), and what it decides about runs (trpx_amd/csrc/label_runs.hpp) is clean under ASan + UBSan in a stand-alone
CPU program."""
import ctypes as C
import os
import subprocess

import pytest

import labelled_truth as T
from trpx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VALUES, N_FRAMES, TERSE_BYTES, N_OUT = 512 * 512, 8, 1 << 20, 3
TERSE, OFFS, INDEX, OUT, STATUS, WS, LABELS, COUNTS = 0x10000, 0x20000, 0x30000, 0x50000, 0x70000, 0x80000, 0x90000, 0xA0000
STREAM_DTYPES = (_lib.U8, _lib.I8, _lib.U16, _lib.I16, _lib.U32, _lib.I32)
OUT_DTYPES = (_lib.I32, _lib.U32, _lib.I64, _lib.U64, _lib.F32, _lib.F64)
ITEMSIZE = {_lib.U8: 1, _lib.I8: 1, _lib.U16: 2, _lib.I16: 2, _lib.U32: 4, _lib.I32: 4}


def L():
    return _lib.lib()


def _call(dtype=_lib.U16, out_dtype=_lib.I64, terse=TERSE, terse_bytes=TERSE_BYTES, offs=OFFS, index=INDEX, n_values=N_VALUES,
          n_frames=N_FRAMES, block=12, labels=LABELS, n_out=N_OUT, out=OUT, counts=COUNTS, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_sum_labelled(dtype, out_dtype, terse, terse_bytes, offs, index, n_values, n_frames, block, labels, n_out, out,
                                        counts, status, ws, ws_bytes, None)


def test_symbols_are_exported_and_bound():
    names = ("trpx_decode_sum_labelled_workspace_bytes", "trpx_decode_sum_labelled_frames_per_chunk", "trpx_decode_sum_labelled",
             "trpx_decode_sum_labelled_host")
    for name in names:
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L(), name).restype == _lib.SYMBOLS[name][0]
    _P, _SZ, _U, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert _lib.SYMBOLS["trpx_decode_sum_labelled_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U, _SZ])
    assert _lib.SYMBOLS["trpx_decode_sum_labelled_frames_per_chunk"] == (_U, [_I, _SZ, _SZ])
    assert _lib.SYMBOLS["trpx_decode_sum_labelled"] == (_I, [_I, _I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _P, _SZ, _P, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_sum_labelled_host"] == (_I, [_I, _I, _P, _SZ, _P, _SZ, _SZ, _U, _P, _SZ, _P, _P, _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_header_declares_them_and_lists_the_call_under_restated_widths():
    text = open(os.path.join(ROOT, "include", "trpx_hip.h")).read()
    for name in ("size_t trpx_decode_sum_labelled_workspace_bytes(", "unsigned trpx_decode_sum_labelled_frames_per_chunk(",
                 "int trpx_decode_sum_labelled(", "int trpx_decode_sum_labelled_host(", "A MASKED FRAME IS NEVER READ AND NEVER VALIDATED"):
        assert name in text
    top = text[text.index("Restated widths."):text.index("Status 0 with pixels that are not the stream's")]
    assert "trpx_decode_sum_labelled" in top
    assert "#define TRPX_ABI_VERSION 3" in text


GRID_VALUES = (7, 449, 6144, 6145, 512 * 512, 4096 * 4096)
GRID_FRAMES = (1, 3, 1024, 1025, 5000, 70_000_000)


@pytest.mark.parametrize("dtype", STREAM_DTYPES)
def test_workspace_bytes_and_frames_per_chunk_are_arithmetic(dtype):
    ws, per_chunk, front = L().trpx_decode_sum_labelled_workspace_bytes, L().trpx_decode_sum_labelled_frames_per_chunk, L().trpx_decode_roi_workspace_bytes
    taken = 0
    for n_values in GRID_VALUES:
        for n_frames in GRID_FRAMES:
            terse_bytes = max(n_frames, TERSE_BYTES)
            fr = front(dtype, terse_bytes, n_values, n_frames, 12)                 # the consumers' front alone; 0: sizes no call takes
            fpc, chunks, _ = T.plan(ITEMSIZE[dtype], n_values, n_frames)
            assert per_chunk(dtype, n_values, n_frames) == (fpc if fr else 0), (n_values, n_frames)
            for n_out in (1, 1 << 20):
                got = ws(dtype, terse_bytes, n_values, n_frames, 12, n_out)
                assert got == (fr + T.own_bytes(ITEMSIZE[dtype], n_values, n_frames, n_out) if fr else 0), (n_values, n_frames, n_out)
                assert got % 8 == 0
            taken += bool(fr)
            if fr:
                assert (chunks - 1) * fpc < n_frames <= chunks * fpc               # every chunk has a frame
    assert taken >= 30                                                             # (the 4096^2 x 70 000 000 corner is what no call takes)
    # the 65 535 cap binds for 8/16-bit types, not for 32-bit ones
    assert per_chunk(dtype, 7, 70_000_000) == (65535 if ITEMSIZE[dtype] < 4 else 68360)
    assert per_chunk(dtype, 7, 2500) == 3 and per_chunk(dtype, 449, 5000) == 5 and per_chunk(dtype, 7, 600) == 1
    # 43 tiles a frame: 24 chunks would be 1032 units, two rounds of the resident workgroups, which hold 35 chunks (1505 units)
    assert per_chunk(dtype, 512 * 512, 480) == 14


def test_arithmetic_is_zero_for_what_no_call_takes():
    ws, per_chunk = L().trpx_decode_sum_labelled_workspace_bytes, L().trpx_decode_sum_labelled_frames_per_chunk
    assert ws(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, N_OUT) > 0
    assert ws(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 0) == 0               # no outputs
    assert ws(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, (1 << 20) + 1) == 0   # too many
    assert ws(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7, N_OUT) == 0            # block 7
    assert ws(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12, N_OUT) == 0           # 64-bit container
    assert ws(_lib.F32, TERSE_BYTES, N_VALUES, N_FRAMES, 12, N_OUT) == 0           # not a stream type
    assert ws(_lib.U16, 0, N_VALUES, N_FRAMES, 12, N_OUT) == 0
    assert ws(_lib.U16, TERSE_BYTES, 0, N_FRAMES, 12, N_OUT) == 0 and ws(_lib.U16, TERSE_BYTES, N_VALUES, 0, 12, N_OUT) == 0
    assert per_chunk(_lib.U16, 0, 8) == 0 and per_chunk(_lib.U16, N_VALUES, 0) == 0
    assert per_chunk(_lib.U64, N_VALUES, 8) == 0 and per_chunk(_lib.F32, N_VALUES, 8) == 0 and per_chunk(42, N_VALUES, 8) == 0
    assert per_chunk(-1, N_VALUES, 8) == 0
    assert per_chunk(_lib.U32, 1 << 28, 1) == 0             # frames of >= 2^32 bits
    # the order needs room whatever the form: more outputs, more frames -> more scratch
    assert ws(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 1000) > ws(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 1)


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(block=0), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U32, n_values=1 << 28), _lib.ERR_UNSUPPORTED),              # frames of >= 2^32 bits
    (dict(dtype=_lib.I16, out_dtype=_lib.U32), _lib.ERR_UNSUPPORTED),            # a signed stream into an unsigned output
    (dict(dtype=_lib.I8, out_dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(n_out=(1 << 20) + 1), _lib.ERR_UNSUPPORTED),
    (dict(n_out=1 << 40), _lib.ERR_UNSUPPORTED),
    # TRPX_ERR_INVALID_ARG
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),            # float dtype: not a stream type
    (dict(dtype=_lib.F64), _lib.ERR_INVALID_ARG),
    (dict(dtype=42), _lib.ERR_INVALID_ARG),                  # unknown dtype
    (dict(dtype=-1), _lib.ERR_INVALID_ARG),
    (dict(out_dtype=_lib.U16), _lib.ERR_INVALID_ARG),        # none of the six
    (dict(out_dtype=_lib.I8), _lib.ERR_INVALID_ARG),
    (dict(out_dtype=42), _lib.ERR_INVALID_ARG),
    (dict(n_out=0), _lib.ERR_INVALID_ARG),
    (dict(n_values=0), _lib.ERR_INVALID_ARG),                # bad sizes
    (dict(n_frames=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=4, n_frames=5), _lib.ERR_INVALID_ARG), # more frames than bytes
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(out=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(labels=None), _lib.ERR_INVALID_ARG),
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(labels=LABELS + 2), _lib.ERR_INVALID_ARG),         # labels at an address = 2 mod 4
    (dict(labels=LABELS + 1), _lib.ERR_INVALID_ARG),
    (dict(counts=COUNTS + 2), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 4), _lib.ERR_INVALID_ARG),               # int64 sums at 4 mod 8
    (dict(out=OUT + 2, out_dtype=_lib.I32), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 4, out_dtype=_lib.F64), _lib.ERR_INVALID_ARG),
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    (dict(ws=None), _lib.ERR_INVALID_ARG),                   # the order of the frames lives in the workspace: every form needs one
    (dict(index=None, ws=None), _lib.ERR_INVALID_ARG),
    (dict(offs=None, index=None, ws=None), _lib.ERR_INVALID_ARG),
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0), _lib.ERR_CAPACITY),                   # ... and room, with an index too
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),
    (dict(ws_bytes=0, index=None, offs=None), _lib.ERR_CAPACITY),
])
def test_argument_errors_are_return_codes(kw, code):
    assert _call(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_sum_labelled")


@pytest.mark.parametrize("kw, code", [
    # trpx_decode_sum's order: 64-bit container -> unknown dtype -> out_dtype -> block -> signedness -> [n_out] -> sizes -> null ->
    # index without offsets -> misaligned -> frames of >= 2^32 bits -> workspace
    (dict(dtype=_lib.U64, out_dtype=42, block=7, n_out=0), _lib.ERR_UNSUPPORTED),
    (dict(dtype=42, out_dtype=42, block=7), _lib.ERR_INVALID_ARG),
    (dict(out_dtype=42, block=7), _lib.ERR_INVALID_ARG),
    (dict(block=7, n_out=0, n_values=0), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I16, out_dtype=_lib.U32, n_out=0), _lib.ERR_UNSUPPORTED),     # signedness in front of the outputs' count
    (dict(n_out=0, n_values=0, terse=None), _lib.ERR_INVALID_ARG),
    (dict(n_out=(1 << 20) + 1, n_values=0, terse=None), _lib.ERR_UNSUPPORTED),     # the outputs' count in front of the sizes
    (dict(n_out=0, block=7), _lib.ERR_UNSUPPORTED),                                # ... and behind the block size
    (dict(n_values=0, ws_bytes=0), _lib.ERR_INVALID_ARG),
    (dict(terse=None, ws_bytes=0), _lib.ERR_INVALID_ARG),
    (dict(labels=LABELS + 2, ws_bytes=0), _lib.ERR_INVALID_ARG),                   # pointers in front of the capacity
    (dict(labels=LABELS + 2, dtype=_lib.U32, n_values=1 << 28), _lib.ERR_INVALID_ARG),   # ... and of the frame-size limit
    (dict(dtype=_lib.U32, n_values=1 << 28, ws_bytes=0), _lib.ERR_UNSUPPORTED),
    (dict(ws=None, ws_bytes=0), _lib.ERR_INVALID_ARG),                             # a null workspace in front of its size
])
def test_order_of_the_checks(kw, code):
    assert _call(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_sum_labelled")


def test_legal_calls_pass_every_check():
    # every check passed: the first thing to fail is the workspace, which is one word long
    for dtype in STREAM_DTYPES:
        for out_dtype in OUT_DTYPES:
            if dtype & 1 and out_dtype in (_lib.U32, _lib.U64):
                continue
            for index in (INDEX, None):
                assert _call(dtype=dtype, out_dtype=out_dtype, index=index, ws_bytes=8) == _lib.ERR_CAPACITY, (dtype, out_dtype)
    for kw in (dict(n_out=1), dict(n_out=1 << 20), dict(n_out=N_FRAMES + 5), dict(counts=None), dict(labels=LABELS + 4), dict(counts=COUNTS + 4),
               dict(out=OUT + 8), dict(out=OUT + 4, out_dtype=_lib.F32), dict(n_values=7), dict(n_values=1030 * 1065)):
        assert _call(ws_bytes=8, **kw) == _lib.ERR_CAPACITY, kw


@pytest.mark.parametrize("n_values, n_frames, n_out", [(N_VALUES, N_FRAMES, 3), (N_VALUES, 2000, 2000), (122880, 3, 1 << 20)])
def test_workspace_one_word_short(n_values, n_frames, n_out):
    need = L().trpx_decode_sum_labelled_workspace_bytes(_lib.U16, TERSE_BYTES, n_values, n_frames, 12, n_out)
    kw = dict(n_values=n_values, n_frames=n_frames, n_out=n_out)
    assert _call(offs=None, index=None, ws_bytes=need - 8, **kw) == _lib.ERR_CAPACITY        # without offsets: the whole need
    # with more given less is needed, and the call checks against its own form's need
    own = T.own_bytes(2, n_values, n_frames, n_out)
    idx = L().trpx_index_bytes(_lib.U16, n_values, n_frames, 12)
    assert 0 < own < need and idx + own <= need
    assert _call(ws_bytes=own - 8, **kw) == _lib.ERR_CAPACITY                                # an index given: the order and the slab
    assert _call(index=None, ws_bytes=own + idx // 2, **kw) == _lib.ERR_CAPACITY            # offsets only: the index has to fit too


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    out = (C.c_uint64 * 64)()
    lab = (C.c_uint32 * 64)()
    cnt = (C.c_uint32 * 64)()

    def host(dtype=_lib.U16, out_dtype=_lib.I64, block=12, n_values=12, n_out=2, out=out, terse=buf, terse_bytes=64, n_frames=2, labels=lab,
             counts=cnt):
        return L().trpx_decode_sum_labelled_host(dtype, out_dtype, terse, terse_bytes, None, n_values, n_frames, block, labels, n_out, out,
                                                 counts, -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=_lib.U32, n_values=1 << 28, terse_bytes=1 << 30), _lib.ERR_UNSUPPORTED),
                     (dict(n_out=(1 << 20) + 1), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.I16, out_dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(out_dtype=_lib.U16), _lib.ERR_INVALID_ARG), (dict(n_out=0), _lib.ERR_INVALID_ARG),
                     (dict(n_values=0), _lib.ERR_INVALID_ARG), (dict(n_frames=0), _lib.ERR_INVALID_ARG), (dict(n_frames=65), _lib.ERR_INVALID_ARG),
                     (dict(out=None), _lib.ERR_INVALID_ARG), (dict(terse=None), _lib.ERR_INVALID_ARG), (dict(labels=None), _lib.ERR_INVALID_ARG),
                     (dict(terse_bytes=0), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_decode_sum_labelled_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device
        assert host(counts=None) == _lib.ERR_NO_DEVICE


def test_run_rules_under_the_sanitizers():
    """label_runs.hpp -- the text the kernels run: a model of the call over heap arrays of exactly the ordered frames', the
    partial slab's and the output's elements; chunks of 1, 2, 5 and 65535 positions; all one label, all masked, every frame its
    own label, f % 3, boundaries exactly on the cuts, one label over three and more chunks between short ones, more outputs than
    frames, seeded random labels.  Equal to the direct sums, every output written exactly once (direct xor merged), no slot used
    twice, every partial added once; under ASan + UBSan (a stand-alone CPU program)."""
    exe = os.path.join(ROOT, "tests", "cpp", "sum_labelled_sanitize")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "sum_labelled_example.mk", "sum_labelled_sanitize"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK sum_labelled_sanitize" in r.stdout, r.stdout + r.stderr
