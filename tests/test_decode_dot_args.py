"""CPU tier: trpx_decode_dot's three symbols are exported and bound, its workspace size is arithmetic, and its argument errors are
return codes decided before any device call (the pointers below are fake, aligned addresses: a call that reached the device
would fail differently)."""
import ctypes as C

import pytest

from trpx_amd import _lib

N_VALUES, N_FRAMES, TERSE_BYTES, N_MAPS = 512 * 512, 8, 1 << 20, 3
TERSE, OFFS, INDEX, WEIGHTS, DOTS, STATUS, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x70000, 0x80000
RUN = 8                                                     # groups per run (one wavefront's unit of work)


def L():
    return _lib.lib()


def _dot(dtype=_lib.U16, terse=TERSE, terse_bytes=TERSE_BYTES, offs=OFFS, index=INDEX, n_values=N_VALUES, n_frames=N_FRAMES, block=12,
         weights=WEIGHTS, n_maps=N_MAPS, dots=DOTS, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_dot(dtype, terse, terse_bytes, offs, index, n_values, n_frames, block, weights, n_maps, dots, status, ws,
                               ws_bytes, None)


def _runs(n_values=N_VALUES, n_frames=N_FRAMES):
    return n_frames * -(-L().trpx_group_count(n_values, 12) // RUN)


def _support_bytes(n_values=N_VALUES):
    return 4 * -(-(-(-n_values // 12)) // 32)


def test_symbols_are_exported_and_bound():
    for name in ("trpx_decode_dot_workspace_bytes", "trpx_decode_dot", "trpx_decode_dot_host"):
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L(), name).restype == _lib.SYMBOLS[name][0]
    _P, _SZ, _U, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert _lib.SYMBOLS["trpx_decode_dot_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U, _U])
    assert _lib.SYMBOLS["trpx_decode_dot"] == (_I, [_I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _P, _U, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_dot_host"] == (_I, [_I, _P, _SZ, _P, _SZ, _SZ, _U, _P, _U, _P, _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_header_declares_them_and_lists_the_call_under_restated_widths():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trpx_hip.h")).read()
    for name in ("trpx_decode_dot_workspace_bytes(", "int trpx_decode_dot(", "int trpx_decode_dot_host("):
        assert name in text
    top = text[text.index("Restated widths."):text.index("Status 0 with pixels that are not the stream's")]
    assert "trpx_decode_dot" in top
    assert "#define TRPX_ABI_VERSION 3" in text


@pytest.mark.parametrize("n_maps", [1, 2, 3, 16])
def test_workspace_bytes_is_arithmetic(n_maps):
    f = L().trpx_decode_dot_workspace_bytes
    n = f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, n_maps)
    assert n > 0 and n % 8 == 0
    assert n >= L().trpx_index_bytes(_lib.U16, N_VALUES, N_FRAMES, 12)          # (index built in the workspace)
    # beyond what the index and the locator need: 8 bytes per (run, map), the support words, a small constant -- nothing of the
    # size of n_frames x n_values
    extra = n - L().trpx_decode_roi_workspace_bytes(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12)
    assert 0 < extra <= 8 * n_maps * _runs() + _support_bytes() + 16
    assert extra < N_FRAMES * N_VALUES // 64


def test_workspace_bytes_is_zero_for_what_the_call_does_not_support():
    f = L().trpx_decode_dot_workspace_bytes
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7, 3) == 0               # block 7
    assert f(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 3) == 0              # 64-bit container
    assert f(_lib.F32, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 3) == 0              # not a stream type
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 0) == 0              # no maps
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 17) == 0             # too many maps
    assert f(_lib.U16, TERSE_BYTES, 0, N_FRAMES, 12, 3) == 0
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, 0, 12, 3) == 0
    assert f(_lib.U16, 0, N_VALUES, N_FRAMES, 12, 3) == 0
    for dt in (_lib.U8, _lib.I8, _lib.U16, _lib.I16, _lib.U32, _lib.I32):
        assert f(dt, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 16) > 0


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
    (dict(n_values=0), _lib.ERR_INVALID_ARG),                # zero sizes
    (dict(n_frames=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=0), _lib.ERR_INVALID_ARG),
    (dict(n_maps=0), _lib.ERR_INVALID_ARG),                  # the number of maps
    (dict(n_maps=17), _lib.ERR_INVALID_ARG),
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(weights=None), _lib.ERR_INVALID_ARG),
    (dict(dots=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(weights=WEIGHTS + 2), _lib.ERR_INVALID_ARG),
    (dict(dots=DOTS + 4), _lib.ERR_INVALID_ARG),
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    (dict(ws=None), _lib.ERR_INVALID_ARG),                   # no workspace: the support bits and partial sums live there
    (dict(offs=None, index=None, ws=None), _lib.ERR_INVALID_ARG),
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0), _lib.ERR_CAPACITY),                   # workspace too small for the partial sums
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),       # ... and for the index
])
def test_argument_errors_are_return_codes(kw, code):
    assert _dot(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_dot")


def test_weights_need_only_four_byte_alignment():
    # 4-byte aligned maps pass every check: the first thing to fail is the workspace that is one word short
    assert _dot(weights=WEIGHTS + 4, ws_bytes=8) == _lib.ERR_CAPACITY


@pytest.mark.parametrize("n_maps", [1, 3, 16])
def test_workspace_one_word_short(n_maps):
    need = L().trpx_decode_dot_workspace_bytes(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, n_maps)
    assert _dot(offs=None, index=None, n_maps=n_maps, ws_bytes=need - 8) == _lib.ERR_CAPACITY   # without offsets: the whole need
    assert L().trpx_last_error_string().startswith(b"trpx_decode_dot")
    # with offsets and index given less is needed, and the call checks against its own form's need: the support words, 8 bytes
    # per (run, map)
    own = (_support_bytes() + 7) // 8 * 8 + 8 * n_maps * _runs()
    assert own < need
    assert _dot(n_maps=n_maps, ws_bytes=own - 8) == _lib.ERR_CAPACITY
    assert L().trpx_last_error_string().startswith(b"trpx_decode_dot")


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    w = (C.c_int32 * 48)()
    dots = (C.c_int64 * 8)()

    def host(dtype=_lib.U16, block=12, n_values=12, weights=w, n_maps=2, out=dots, terse=buf):
        return L().trpx_decode_dot_host(dtype, terse, 64, None, n_values, 2, block, weights, n_maps, out, -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(n_values=0), _lib.ERR_INVALID_ARG), (dict(weights=None), _lib.ERR_INVALID_ARG),
                     (dict(out=None), _lib.ERR_INVALID_ARG), (dict(terse=None), _lib.ERR_INVALID_ARG),
                     (dict(n_maps=0), _lib.ERR_INVALID_ARG), (dict(n_maps=17), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_decode_dot_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device
