"""CPU tier: trpx_decode_sum's three symbols are exported and bound, and its argument errors are return codes decided before
any device call (the pointers below are fake, aligned addresses: a call that reached the device would fail differently)."""
import ctypes as C

import pytest

from trpx_amd import _lib

N_VALUES, N_FRAMES, TERSE_BYTES = 512 * 512, 8, 1 << 20
TERSE, OFFS, INDEX, SUMS, STATUS, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


def L():
    return _lib.lib()


def _sum(dtype=_lib.U16, out=_lib.I32, offs=OFFS, index=INDEX, block=12, group=2, ws=WS, ws_bytes=1 << 40, sums=SUMS):
    return L().trpx_decode_sum(dtype, out, TERSE, TERSE_BYTES, offs, index, N_VALUES, N_FRAMES, block, group, sums, STATUS,
                               ws, ws_bytes, None)


def test_symbols_are_exported_and_bound():
    for name in ("trpx_decode_sum_workspace_bytes", "trpx_decode_sum", "trpx_decode_sum_host"):
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]


def test_workspace_bytes_is_arithmetic():
    f = L().trpx_decode_sum_workspace_bytes
    n = f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 2)
    assert n > 0 and n % 8 == 0
    assert n >= L().trpx_index_bytes(_lib.U16, N_VALUES, N_FRAMES, 12)          # (index built in the workspace)
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 0) == 0              # group 0
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7, 2) == 0               # block 7
    assert f(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 2) == 0              # 64-bit container
    # few outputs: the frames are split into chunks, whose partial sums need room
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, 2000, 12, 2000) > f(_lib.U16, TERSE_BYTES, N_VALUES, 2000, 12, 1)


@pytest.mark.parametrize("kw, code", [
    (dict(group=0), _lib.ERR_INVALID_ARG),
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I16, out=_lib.U32), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I32, out=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                # an index without its offsets
    (dict(out=_lib.U16), _lib.ERR_INVALID_ARG),             # unknown out_dtype
    (dict(out=42), _lib.ERR_INVALID_ARG),
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),           # not a stream type
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),      # workspace too small for the index
    (dict(sums=SUMS + 2), _lib.ERR_INVALID_ARG),            # sums misaligned for their type
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(sums=None), _lib.ERR_INVALID_ARG),
])
def test_argument_errors_are_return_codes(kw, code):
    assert _sum(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_sum")


def test_workspace_too_small_without_offsets():
    need = L().trpx_decode_sum_workspace_bytes(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 2)
    assert _sum(offs=None, index=None, ws_bytes=need - 8) == _lib.ERR_CAPACITY


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    out = (C.c_int32 * 64)()
    if L().trpx_device_count() == 0:
        assert L().trpx_decode_sum_host(_lib.U16, _lib.I32, buf, 64, None, 7, 2, 12, 1, out, -1) == _lib.ERR_NO_DEVICE
    else:
        assert L().trpx_decode_sum_host(_lib.U16, _lib.I32, buf, 64, None, 7, 2, 12, 0, out, -1) == _lib.ERR_INVALID_ARG
        assert L().trpx_decode_sum_host(_lib.U16, _lib.I32, buf, 64, None, 7, 2, 7, 1, out, -1) == _lib.ERR_UNSUPPORTED
