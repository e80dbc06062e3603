"""CPU tier: trpx_decode_corrected's three symbols are exported and bound, its workspace size is arithmetic, its argument errors
are return codes decided before any device call (the pointers below are fake, aligned addresses: a call that reached the device
would fail differently), and the pixel rule and the store step's index arithmetic (trpx_amd/csrc/correct_px.hpp) are clean under
ASan + UBSan in a stand-alone CPU program."""
import ctypes as C
import os
import subprocess

import pytest

from trpx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VALUES, N_FRAMES, TERSE_BYTES = 512 * 512, 8, 1 << 20
TERSE, OFFS, INDEX, OUT, STATUS, WS, DARK, GAIN = 0x10000, 0x20000, 0x30000, 0x50000, 0x70000, 0x80000, 0x90000, 0xA0000


def L():
    return _lib.lib()


def _call(dtype=_lib.U16, out_dtype=_lib.F32, terse=TERSE, terse_bytes=TERSE_BYTES, offs=OFFS, index=INDEX, n_values=N_VALUES, n_frames=N_FRAMES,
          block=12, dark=DARK, gain=GAIN, out=OUT, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_corrected(dtype, out_dtype, terse, terse_bytes, offs, index, n_values, n_frames, block, dark, gain, out, status, ws,
                                     ws_bytes, None)


def test_symbols_are_exported_and_bound():
    names = ("trpx_decode_corrected_workspace_bytes", "trpx_decode_corrected", "trpx_decode_corrected_host")
    for name in names:
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L(), name).restype == _lib.SYMBOLS[name][0]
    _P, _SZ, _U, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert _lib.SYMBOLS["trpx_decode_corrected_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U])
    assert _lib.SYMBOLS["trpx_decode_corrected"] == (_I, [_I, _I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _P, _P, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_corrected_host"] == (_I, [_I, _I, _P, _SZ, _P, _SZ, _SZ, _U, _P, _P, _P, _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_header_declares_them_and_lists_the_call_under_restated_widths():
    text = open(os.path.join(ROOT, "include", "trpx_hip.h")).read()
    for name in ("size_t trpx_decode_corrected_workspace_bytes(", "int trpx_decode_corrected(", "int trpx_decode_corrected_host("):
        assert name in text
    top = text[text.index("Restated widths."):text.index("Status 0 with pixels that are not the stream's")]
    assert "trpx_decode_corrected" in top
    assert "#define TRPX_ABI_VERSION 3" in text
    doc = text[text.index("Corrected decode:"):text.index("size_t trpx_decode_corrected_workspace_bytes(")]
    assert "SUBNORMAL" in doc and "unspecified" in doc       # the one case the result is not pinned for
    assert "Terse.hpp:352-389" in doc and "src/prolix.cpp:69-92" in doc
    # the declared parameter lists have as many parameters as the binding table
    for ret, name in (("size_t", "trpx_decode_corrected_workspace_bytes"), ("int", "trpx_decode_corrected"), ("int", "trpx_decode_corrected_host")):
        decl = text[text.index(f"\n{ret} {name}("):]
        assert decl[:decl.index(");")].count(",") + 1 == len(_lib.SYMBOLS[name][1]), name


@pytest.mark.parametrize("dtype", [_lib.U8, _lib.I8, _lib.U16, _lib.I16, _lib.U32, _lib.I32])
@pytest.mark.parametrize("n_values, n_frames", [(N_VALUES, N_FRAMES), (N_VALUES, 2000), (1, 1), (13, 3), (2 * 12288 + 67, 3), (4096 * 4096, 8)])
def test_workspace_bytes_is_what_the_index_needs(dtype, n_values, n_frames):
    terse_bytes = max(TERSE_BYTES, n_frames)
    n = L().trpx_decode_corrected_workspace_bytes(dtype, terse_bytes, n_values, n_frames, 12)
    assert n > 0 and n % 8 == 0
    assert n == L().trpx_decode_roi_workspace_bytes(dtype, terse_bytes, n_values, n_frames, 12)


def test_workspace_bytes_is_zero_for_what_the_call_does_not_take():
    f = L().trpx_decode_corrected_workspace_bytes
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7) == 0                  # block 7
    assert f(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12) == 0                 # 64-bit container
    assert f(_lib.F32, TERSE_BYTES, N_VALUES, N_FRAMES, 12) == 0                 # not a stream type
    assert f(42, TERSE_BYTES, N_VALUES, N_FRAMES, 12) == 0
    assert f(_lib.U16, TERSE_BYTES, 0, N_FRAMES, 12) == 0
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, 0, 12) == 0
    assert f(_lib.U16, 0, N_VALUES, N_FRAMES, 12) == 0
    assert f(_lib.U16, 4, N_VALUES, N_FRAMES, 12) == 0                           # fewer bytes than frames
    assert f(_lib.U32, TERSE_BYTES, 1 << 28, 1, 12) == 0                         # frames of >= 2^32 bits
    assert f(_lib.U8, 1 << 25, 8, (1 << 24) + 3, 12) == 0                        # more groups of 256 blocks than one call takes
    assert f(_lib.U8, 1 << 25, 8, (1 << 24) - 1, 12) > 0                         # ... and the most it takes


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(block=0), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),            # a 64-bit container
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
    (dict(out_dtype=_lib.F64), _lib.ERR_UNSUPPORTED),        # only float32 frames
    (dict(out_dtype=_lib.U16), _lib.ERR_UNSUPPORTED),
    (dict(out_dtype=_lib.I32), _lib.ERR_UNSUPPORTED),
    (dict(out_dtype=42), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U32, n_values=1 << 28), _lib.ERR_UNSUPPORTED),              # frames of >= 2^32 bits
    (dict(dtype=_lib.U8, n_values=8, n_frames=(1 << 24) + 3, terse_bytes=1 << 25), _lib.ERR_UNSUPPORTED),   # more groups than one call takes
    # TRPX_ERR_INVALID_ARG
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),            # float dtype: not a stream type
    (dict(dtype=_lib.F64), _lib.ERR_INVALID_ARG),
    (dict(dtype=42), _lib.ERR_INVALID_ARG),                  # unknown dtype
    (dict(dtype=-1), _lib.ERR_INVALID_ARG),
    (dict(n_values=0), _lib.ERR_INVALID_ARG),                # zero sizes
    (dict(n_frames=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=4), _lib.ERR_INVALID_ARG),             # fewer bytes than frames
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(out=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 2), _lib.ERR_INVALID_ARG),
    (dict(dark=DARK + 2), _lib.ERR_INVALID_ARG),
    (dict(gain=GAIN + 1), _lib.ERR_INVALID_ARG),
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    (dict(index=None, ws=None), _lib.ERR_INVALID_ARG),       # no workspace where the index is built
    (dict(offs=None, index=None, ws=None), _lib.ERR_INVALID_ARG),
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),       # workspace too small for the index
    (dict(ws_bytes=0, index=None, offs=None), _lib.ERR_CAPACITY),
])
def test_argument_errors_are_return_codes(kw, code):
    assert _call(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_corrected")


@pytest.mark.parametrize("kw", [dict(), dict(dark=None), dict(gain=None), dict(dark=None, gain=None), dict(out=OUT + 4), dict(out=OUT + 12),
                                dict(dark=DARK + 4, gain=GAIN + 8), dict(n_values=13, n_frames=3), dict(dtype=_lib.I32)])
def test_legal_corners_pass_every_check(kw):
    # absent maps and every 4-byte alignment are legal: the first thing to fail is the workspace that is one byte short
    args = dict(n_values=N_VALUES, n_frames=N_FRAMES, dtype=_lib.U16)
    args.update({k: v for k, v in kw.items() if k in args})
    need = L().trpx_decode_corrected_workspace_bytes(args["dtype"], TERSE_BYTES, args["n_values"], args["n_frames"], 12)
    assert need > 0
    assert _call(offs=None, index=None, ws_bytes=need - 1, **kw) == _lib.ERR_CAPACITY
    assert L().trpx_last_error_string().startswith(b"trpx_decode_corrected: workspace")
    assert _call(index=None, ws_bytes=0, **kw) == _lib.ERR_CAPACITY              # offsets only needs less, but not nothing


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    frames = (C.c_float * 24)()
    dark = (C.c_float * 12)()

    def host(dtype=_lib.U16, out_dtype=_lib.F32, block=12, n_values=12, out=frames, terse=buf, dark=dark, gain=None):
        return L().trpx_decode_corrected_host(dtype, out_dtype, terse, 64, None, n_values, 2, block, dark, gain, out, -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(out_dtype=_lib.F64), _lib.ERR_UNSUPPORTED), (dict(out_dtype=_lib.U16), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(n_values=0), _lib.ERR_INVALID_ARG), (dict(out=None), _lib.ERR_INVALID_ARG), (dict(terse=None), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_decode_corrected_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device
        assert host(dark=None) == _lib.ERR_NO_DEVICE         # ... absent maps included


def test_rule_and_store_step_under_the_sanitizers():
    """correct_px.hpp -- the text the kernel runs: whole frames of 1, 11, 12, 13, 767, 769 and 12 288 + 67 values stored on the host
    with every (lane, round) of the store step, output and maps 0, 4, 8 and 12 bytes behind a 16-byte boundary: every pixel owned
    exactly once, no index outside its array, the 16-byte path exactly where all three addresses allow it, and the pixel rule
    equal to a plain float loop at the edges of every type; under ASan + UBSan (a stand-alone CPU program)."""
    exe = os.path.join(ROOT, "tests", "cpp", "corrected_sanitize")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "corrected_example.mk", "corrected_sanitize"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK corrected_sanitize" in r.stdout, r.stdout + r.stderr
