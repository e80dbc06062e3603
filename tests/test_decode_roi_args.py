"""CPU tier: trpx_decode_roi's three symbols are exported and bound, and its argument errors are return codes decided before
any device call (the pointers below are fake, aligned addresses: a call that reached the device would fail differently)."""
import ctypes as C

import pytest

from trpx_amd import _lib

WIDTH, HEIGHT = 512, 512
N_VALUES, N_FRAMES, TERSE_BYTES = WIDTH * HEIGHT, 8, 1 << 20
TERSE, OFFS, INDEX, OUT, STATUS, WS, BOXES = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


def L():
    return _lib.lib()


def _roi(dtype=_lib.U16, terse=TERSE, offs=OFFS, index=INDEX, n_values=N_VALUES, n_frames=N_FRAMES, block=12, width=WIDTH,
         boxes=BOXES, n_boxes=5, box_h=64, box_w=48, out=OUT, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_roi(dtype, terse, TERSE_BYTES, offs, index, n_values, n_frames, block, width, boxes, n_boxes, box_h,
                               box_w, out, status, ws, ws_bytes, None)


def test_symbols_are_exported_and_bound():
    for name in ("trpx_decode_roi_workspace_bytes", "trpx_decode_roi", "trpx_decode_roi_host"):
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
    _P, _SZ, _U, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert _lib.SYMBOLS["trpx_decode_roi_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U])
    assert _lib.SYMBOLS["trpx_decode_roi"] == (_I, [_I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _SZ, _P, _SZ, _U, _U, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_roi_host"] == (_I, [_I, _P, _SZ, _P, _SZ, _SZ, _U, _SZ, _P, _SZ, _U, _U, _P, _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_workspace_bytes_is_arithmetic():
    f = L().trpx_decode_roi_workspace_bytes
    n = f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12)
    assert n > 0 and n % 8 == 0
    assert n >= L().trpx_index_bytes(_lib.U16, N_VALUES, N_FRAMES, 12)          # (index built in the workspace)
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7) == 0                  # block 7
    assert f(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12) == 0                 # 64-bit container


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U32, n_values=1 << 28, width=1 << 14), _lib.ERR_UNSUPPORTED),   # frames of >= 2^32 bits
    # TRPX_ERR_INVALID_ARG
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),            # unknown dtype: not a stream type
    (dict(dtype=42), _lib.ERR_INVALID_ARG),
    (dict(width=0), _lib.ERR_INVALID_ARG),
    (dict(width=500), _lib.ERR_INVALID_ARG),                 # does not divide n_values
    (dict(box_h=0), _lib.ERR_INVALID_ARG),
    (dict(box_w=0), _lib.ERR_INVALID_ARG),
    (dict(box_h=HEIGHT + 1), _lib.ERR_INVALID_ARG),
    (dict(box_w=WIDTH + 1), _lib.ERR_INVALID_ARG),
    (dict(n_boxes=0), _lib.ERR_INVALID_ARG),
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(boxes=None), _lib.ERR_INVALID_ARG),
    (dict(out=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(offs=None, index=None, ws=None, ws_bytes=1 << 40), _lib.ERR_INVALID_ARG),   # a workspace is needed and there is none
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(boxes=BOXES + 2), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 1), _lib.ERR_INVALID_ARG),               # (u16 pixels)
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),       # workspace too small for the index
])
def test_argument_errors_are_return_codes(kw, code):
    assert _roi(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_roi")


def test_workspace_too_small_without_offsets():
    need = L().trpx_decode_roi_workspace_bytes(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12)
    assert _roi(offs=None, index=None, ws_bytes=need - 8) == _lib.ERR_CAPACITY
    assert L().trpx_last_error_string().startswith(b"trpx_decode_roi")


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    out = (C.c_uint16 * 64)()
    good = (C.c_uint32 * 3)(0, 0, 0)
    outside = (C.c_uint32 * 3)(0, 2, 0)                      # y0 + box_h = 4 > height 3

    def host(n_values=12, width=4, boxes=good, box_h=2, box_w=2):
        return L().trpx_decode_roi_host(_lib.U16, buf, 64, None, n_values, 2, 12, width, boxes, 1, box_h, box_w, out, -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    assert host(boxes=outside) == _lib.ERR_INVALID_ARG
    assert L().trpx_last_error_string().startswith(b"trpx_decode_roi")
    assert host(width=5) == _lib.ERR_INVALID_ARG
    assert L().trpx_last_error_string().startswith(b"trpx_decode_roi")
    assert host(box_h=4) == _lib.ERR_INVALID_ARG             # taller than the frame
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device
