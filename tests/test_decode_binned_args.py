"""CPU tier: trpx_decode_binned's four symbols are exported and bound, its workspace size and its bands per frame are arithmetic,
its argument errors are return codes decided before any device call (the pointers below are fake, aligned addresses: a call that
reached the device would fail differently), and what a lane does with a block (trpx_amd/csrc/binned_map.hpp) is clean under
ASan + UBSan in a stand-alone CPU program."""
import ctypes as C
import os
import subprocess

import pytest

from trpx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH = 512
N_VALUES, N_FRAMES, TERSE_BYTES = WIDTH * WIDTH, 8, 1 << 20
TERSE, OFFS, INDEX, OUT, STATUS, WS = 0x10000, 0x20000, 0x30000, 0x50000, 0x70000, 0x80000
ACCS, TARGET, RUN = 8192, 1536, 8                           # accumulators of a band, workgroups a launch aims at, groups per run


def L():
    return _lib.lib()


def _binned(dtype=_lib.U16, out_dtype=_lib.I32, terse=TERSE, terse_bytes=TERSE_BYTES, offs=OFFS, index=INDEX, n_values=N_VALUES,
            n_frames=N_FRAMES, block=12, width=WIDTH, bin_y=2, bin_x=2, out=OUT, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_binned(dtype, out_dtype, terse, terse_bytes, offs, index, n_values, n_frames, block, width, bin_y, bin_x, out,
                                  status, ws, ws_bytes, None)


def _bands(n_values, width, bin_y, bin_x, n_frames):
    """rows = ceil(out_h / want), bands = ceil(out_h / rows), want = min(out_h, max(what the accumulators force, min(what the
    frames leave room for, the frame's runs)))"""
    out_h, out_w = -(-(n_values // width) // bin_y), -(-width // bin_x)
    by_lds = -(-out_h // max(1, ACCS // out_w))
    by_frames = -(-TARGET // n_frames)
    by_runs = -(-L().trpx_group_count(n_values, 12) // RUN)
    want = min(out_h, max(by_lds, min(by_frames, by_runs)))
    rows = -(-out_h // want)
    return -(-out_h // rows)


def test_symbols_are_exported_and_bound():
    names = ("trpx_decode_binned_workspace_bytes", "trpx_decode_binned_bands_per_frame", "trpx_decode_binned", "trpx_decode_binned_host")
    for name in names:
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L(), name).restype == _lib.SYMBOLS[name][0]
    _P, _SZ, _U, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert _lib.SYMBOLS["trpx_decode_binned_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U])
    assert _lib.SYMBOLS["trpx_decode_binned_bands_per_frame"] == (_U, [_SZ, _SZ, _U, _U, _SZ])
    assert _lib.SYMBOLS["trpx_decode_binned"] == (_I, [_I, _I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _SZ, _U, _U, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_binned_host"] == (_I, [_I, _I, _P, _SZ, _P, _SZ, _SZ, _U, _SZ, _U, _U, _P, _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_header_declares_them_and_lists_the_call_under_restated_widths():
    text = open(os.path.join(ROOT, "include", "trpx_hip.h")).read()
    for name in ("size_t trpx_decode_binned_workspace_bytes(", "unsigned trpx_decode_binned_bands_per_frame(", "int trpx_decode_binned(",
                 "int trpx_decode_binned_host("):
        assert name in text
    top = text[text.index("Restated widths."):text.index("Status 0 with pixels that are not the stream's")]
    assert "trpx_decode_binned" in top
    assert "#define TRPX_ABI_VERSION 3" in text


@pytest.mark.parametrize("n_values, width, bin_y, bin_x, n_frames, want", [
    (512 * 512, 512, 2, 2, 2000, 8),                        # the flagship stack: 32 output rows of 256 sums a band
    (512 * 512, 512, 1, 1, 2000, 32), (512 * 512, 512, 4, 4, 2000, 2), (512 * 512, 512, 8, 8, 2000, 1), (512 * 512, 512, 64, 64, 2000, 1),
    (512 * 512, 512, 64, 64, 1, 8),                         # one frame: cut for the GPU's sake, down to one output row
    (512 * 512, 512, 8, 8, 500, 4),                         # ceil(1536 / 500)
    (1030 * 1065, 1065, 2, 2, 200, 35),                     # 15 rows of 533 sums
    (331 * 371, 371, 1, 1, 3, 16), (331 * 371, 371, 13, 13, 3, 5), (331 * 371, 371, 64, 64, 3, 3),
    (5 * 37, 37, 2, 2, 1, 1), (1, 1, 1, 1, 1, 1), (13, 1, 1, 1, 5, 1), (13, 13, 1, 1, 5, 1),
    (2 * 8192, 8192, 1, 1, 1, 2),                           # the widest output row: a band is one row
])
def test_bands_per_frame_is_arithmetic(n_values, width, bin_y, bin_x, n_frames, want):
    assert L().trpx_decode_binned_bands_per_frame(n_values, width, bin_y, bin_x, n_frames) == want == _bands(n_values, width, bin_y, bin_x, n_frames)


def test_bands_per_frame_is_zero_for_sizes_no_call_takes():
    f = L().trpx_decode_binned_bands_per_frame
    assert f(0, 512, 2, 2, 8) == 0
    assert f(N_VALUES, 512, 2, 2, 0) == 0
    assert f(N_VALUES, 0, 2, 2, 8) == 0
    assert f(N_VALUES, 500, 2, 2, 8) == 0                   # a width that does not divide
    assert f(N_VALUES, 512, 0, 2, 8) == 0 and f(N_VALUES, 512, 2, 0, 8) == 0
    assert f(N_VALUES, 512, 65, 2, 8) == 0 and f(N_VALUES, 512, 2, 65, 8) == 0
    assert f(4 * 512, 512, 5, 2, 8) == 0                    # a bin higher than the frame
    assert f(8 * 8, 8, 2, 9, 8) == 0                        # ... wider
    assert f(2 * 8193, 8193, 1, 1, 8) == 0                  # more than 8192 sums in a row
    assert f(1 << 29, 512, 2, 2, 1) == 0                    # frames of >= 2^32 bits
    assert f(2 * 8192, 8192, 1, 1, 8) > 0 and f(2 * 8193, 8193, 1, 2, 8) > 0


@pytest.mark.parametrize("dtype", [_lib.U8, _lib.I8, _lib.U16, _lib.I16, _lib.U32, _lib.I32])
@pytest.mark.parametrize("n_values, n_frames", [(N_VALUES, N_FRAMES), (N_VALUES, 2000), (122893, 3), (4096 * 4096, 8), (13, 1)])
def test_workspace_bytes_is_the_box_decode_s(dtype, n_values, n_frames):
    terse_bytes = max(TERSE_BYTES, n_frames)
    n = L().trpx_decode_binned_workspace_bytes(dtype, terse_bytes, n_values, n_frames, 12)
    assert n > 0 and n == L().trpx_decode_roi_workspace_bytes(dtype, terse_bytes, n_values, n_frames, 12)   # no scratch of its own


def test_workspace_bytes_is_zero_for_what_the_call_does_not_support():
    f = L().trpx_decode_binned_workspace_bytes
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7) == 0                  # block 7
    assert f(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12) == 0                 # 64-bit container
    assert f(_lib.F32, TERSE_BYTES, N_VALUES, N_FRAMES, 12) == 0                 # not a stream type
    assert f(_lib.U16, TERSE_BYTES, 0, N_FRAMES, 12) == 0
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, 0, 12) == 0
    assert f(_lib.U16, 0, N_VALUES, N_FRAMES, 12) == 0


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(block=0), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U32, n_values=1 << 28), _lib.ERR_UNSUPPORTED),              # frames of >= 2^32 bits
    (dict(dtype=_lib.I16, out_dtype=_lib.U32), _lib.ERR_UNSUPPORTED),            # a signed stream into an unsigned output
    (dict(dtype=_lib.I8, out_dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I32, out_dtype=_lib.U32), _lib.ERR_UNSUPPORTED),
    (dict(n_values=4 * 8193, width=8193, bin_x=1), _lib.ERR_UNSUPPORTED),        # more than 8192 sums in a row
    (dict(n_values=4 * 16386, width=16386, bin_x=2), _lib.ERR_UNSUPPORTED),
    # TRPX_ERR_INVALID_ARG
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),            # float dtype: not a stream type
    (dict(dtype=_lib.F64), _lib.ERR_INVALID_ARG),
    (dict(dtype=42), _lib.ERR_INVALID_ARG),                  # unknown dtype
    (dict(dtype=-1), _lib.ERR_INVALID_ARG),
    (dict(out_dtype=_lib.U8), _lib.ERR_INVALID_ARG),         # an output type that is none of the six
    (dict(out_dtype=_lib.I16), _lib.ERR_INVALID_ARG),
    (dict(out_dtype=42), _lib.ERR_INVALID_ARG),
    (dict(out_dtype=-1), _lib.ERR_INVALID_ARG),
    (dict(n_values=0), _lib.ERR_INVALID_ARG),                # zero sizes
    (dict(n_frames=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=0), _lib.ERR_INVALID_ARG),
    (dict(width=0), _lib.ERR_INVALID_ARG),
    (dict(width=500), _lib.ERR_INVALID_ARG),                 # a width that does not divide n_values
    (dict(width=N_VALUES + 1), _lib.ERR_INVALID_ARG),
    (dict(bin_y=0), _lib.ERR_INVALID_ARG),                   # the bin
    (dict(bin_x=0), _lib.ERR_INVALID_ARG),
    (dict(bin_y=65), _lib.ERR_INVALID_ARG),
    (dict(bin_x=65), _lib.ERR_INVALID_ARG),
    (dict(n_values=4 * 512, bin_y=5), _lib.ERR_INVALID_ARG),           # higher than the frame
    (dict(width=8, bin_x=9), _lib.ERR_INVALID_ARG),                    # wider than the frame
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(out=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 2), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 2, out_dtype=_lib.F32), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 4, out_dtype=_lib.I64), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 4, out_dtype=_lib.U64), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 4, out_dtype=_lib.F64), _lib.ERR_INVALID_ARG),
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    (dict(index=None, ws=None), _lib.ERR_INVALID_ARG),       # a form that needs a workspace, without one
    (dict(offs=None, index=None, ws=None), _lib.ERR_INVALID_ARG),
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),       # workspace too small for the index
    (dict(ws_bytes=0, index=None, offs=None), _lib.ERR_CAPACITY),
])
def test_argument_errors_are_return_codes(kw, code):
    assert _binned(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_binned")


def test_legal_bins_and_outputs_pass_every_check():
    # every check passed: the first thing to fail is the workspace of the form without an index, which is one word long
    for kw in (dict(bin_y=1, bin_x=1), dict(bin_y=64, bin_x=64), dict(bin_y=1, bin_x=64), dict(bin_y=3, bin_x=5),
               dict(n_values=1030 * 1065, width=1065), dict(n_values=7, width=7, bin_y=1, bin_x=7), dict(n_values=7, width=1, bin_y=7, bin_x=1),
               dict(n_values=4 * 8192, width=8192, bin_x=1), dict(dtype=_lib.I16, out_dtype=_lib.I64), dict(dtype=_lib.U32, out_dtype=_lib.U64)):
        assert _binned(index=None, ws_bytes=8, **kw) == _lib.ERR_CAPACITY, kw
    for out_dtype, size in ((_lib.I32, 4), (_lib.U32, 4), (_lib.F32, 4), (_lib.I64, 8), (_lib.U64, 8), (_lib.F64, 8)):
        assert _binned(out_dtype=out_dtype, out=OUT + size, index=None, ws_bytes=8) == _lib.ERR_CAPACITY     # aligned to its type only


@pytest.mark.parametrize("n_values, n_frames", [(N_VALUES, N_FRAMES), (N_VALUES, 2000), (122880, 3)])
def test_workspace_one_word_short(n_values, n_frames):
    need = L().trpx_decode_binned_workspace_bytes(_lib.U16, TERSE_BYTES, n_values, n_frames, 12)
    kw = dict(n_values=n_values, n_frames=n_frames)
    assert _binned(offs=None, index=None, ws_bytes=need - 8, **kw) == _lib.ERR_CAPACITY      # without offsets: the whole need
    assert L().trpx_last_error_string().startswith(b"trpx_decode_binned")
    # with offsets given less is needed, and the call checks against its own form's need: the index has to fit
    idx = L().trpx_index_bytes(_lib.U16, n_values, n_frames, 12)
    assert 0 < idx <= need
    assert _binned(index=None, ws_bytes=idx // 2, **kw) == _lib.ERR_CAPACITY


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    out = (C.c_int64 * 64)()

    def host(dtype=_lib.U16, out_dtype=_lib.I32, block=12, n_values=12, width=4, bin_y=2, bin_x=2, out=out, terse=buf):
        return L().trpx_decode_binned_host(dtype, out_dtype, terse, 64, None, n_values, 2, block, width, bin_y, bin_x, out, -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=_lib.I16, out_dtype=_lib.U32), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(out_dtype=_lib.U16), _lib.ERR_INVALID_ARG), (dict(n_values=0), _lib.ERR_INVALID_ARG),
                     (dict(out=None), _lib.ERR_INVALID_ARG), (dict(terse=None), _lib.ERR_INVALID_ARG),
                     (dict(width=5), _lib.ERR_INVALID_ARG), (dict(width=0), _lib.ERR_INVALID_ARG),
                     (dict(bin_y=0), _lib.ERR_INVALID_ARG), (dict(bin_y=4), _lib.ERR_INVALID_ARG), (dict(bin_x=5), _lib.ERR_INVALID_ARG),
                     (dict(bin_x=65), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_decode_binned_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device


def test_block_map_under_the_sanitizers():
    """binned_map.hpp -- the text the kernel runs -- band by band into heap arrays of exactly a band's accumulators: width 1,
    widths around 12, bins larger than a block, partial edge bins, a partial last block, every band split of a frame, the values
    0, the type's minimum and maximum and stretches that sum to zero, against a plain double loop, under ASan + UBSan (a
    stand-alone CPU program)."""
    exe = os.path.join(ROOT, "tests", "cpp", "binned_sanitize")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "binned_example.mk", "binned_sanitize"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK binned_sanitize" in r.stdout, r.stdout + r.stderr
