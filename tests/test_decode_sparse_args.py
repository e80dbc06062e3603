"""CPU tier: trpx_decode_sparse's three symbols are exported and bound, and its argument errors are return codes decided before
any device call (the pointers below are fake, aligned addresses: a call that reached the device would fail differently)."""
import ctypes as C

import pytest

from trpx_amd import _lib

N_VALUES, N_FRAMES, TERSE_BYTES = 512 * 512, 8, 1 << 20
TERSE, OFFS, INDEX, ROWS, POS, VALS, STATUS, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000


def L():
    return _lib.lib()


def _sparse(dtype=_lib.U16, terse=TERSE, offs=OFFS, index=INDEX, n_values=N_VALUES, n_frames=N_FRAMES, block=12, threshold=8,
            rows=ROWS, pos=POS, vals=VALS, capacity=100, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_sparse(dtype, terse, TERSE_BYTES, offs, index, n_values, n_frames, block, threshold, rows, pos, vals,
                                  capacity, status, ws, ws_bytes, None)


def test_symbols_are_exported_and_bound():
    for name in ("trpx_decode_sparse_workspace_bytes", "trpx_decode_sparse", "trpx_decode_sparse_host"):
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
    _P, _SZ, _U, _I, _I64 = C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_int64
    assert _lib.SYMBOLS["trpx_decode_sparse_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U])
    assert _lib.SYMBOLS["trpx_decode_sparse"] == (_I, [_I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _I64, _P, _P, _P, _SZ, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_sparse_host"] == (_I, [_I, _P, _SZ, _P, _SZ, _SZ, _U, _I64, _P, _P, _P, _SZ, C.POINTER(_SZ), _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_workspace_bytes_is_arithmetic():
    f = L().trpx_decode_sparse_workspace_bytes
    n = f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12)
    assert n > 0 and n % 8 == 0
    assert n >= L().trpx_index_bytes(_lib.U16, N_VALUES, N_FRAMES, 12)          # (index built in the workspace)
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7) == 0                  # block 7
    assert f(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12) == 0                 # 64-bit container
    # per group: counts + flags + base, 40 bytes; nothing of the size of n_frames x n_values beyond what the index needs
    groups = N_FRAMES * L().trpx_group_count(N_VALUES, 12)
    assert n - L().trpx_decode_roi_workspace_bytes(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12) <= 40 * groups + 4 * N_FRAMES + 16


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U32, n_values=1 << 28), _lib.ERR_UNSUPPORTED),              # frames of >= 2^32 bits
    # TRPX_ERR_INVALID_ARG
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),            # unknown dtype: not a stream type
    (dict(dtype=42), _lib.ERR_INVALID_ARG),
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(rows=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(rows=ROWS + 4), _lib.ERR_INVALID_ARG),
    (dict(pos=POS + 2), _lib.ERR_INVALID_ARG),
    (dict(vals=VALS + 1), _lib.ERR_INVALID_ARG),             # (u16 values)
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(pos=None), _lib.ERR_INVALID_ARG),                  # values without positions
    (dict(vals=None), _lib.ERR_INVALID_ARG),                 # positions without values
    (dict(pos=None, vals=None, capacity=5), _lib.ERR_INVALID_ARG),   # NULL outputs with a capacity
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    (dict(ws=None), _lib.ERR_INVALID_ARG),                   # no workspace: the counts live there, index given or not
    (dict(offs=None, index=None, ws=None), _lib.ERR_INVALID_ARG),
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0), _lib.ERR_CAPACITY),                   # workspace too small for the counts
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),       # ... and for the index
])
def test_argument_errors_are_return_codes(kw, code):
    assert _sparse(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_sparse")


def test_sizes_only_query_is_legal_as_far_as_the_arguments_go():
    # NULL outputs with capacity 0 pass every check: the first thing to fail is the workspace that is one word short
    assert _sparse(pos=None, vals=None, capacity=0, ws_bytes=8) == _lib.ERR_CAPACITY


def test_workspace_one_word_short():
    need = L().trpx_decode_sparse_workspace_bytes(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12)
    assert _sparse(offs=None, index=None, ws_bytes=need - 8) == _lib.ERR_CAPACITY           # without offsets: the whole need
    assert L().trpx_last_error_string().startswith(b"trpx_decode_sparse")
    # with offsets and index given less is needed, and the call checks against its own form's need: 40 bytes per group, 4 per frame
    groups = N_FRAMES * L().trpx_group_count(N_VALUES, 12)
    own = (40 * groups + 4 * N_FRAMES + 7) // 8 * 8
    assert own < need
    assert _sparse(ws_bytes=own - 8) == _lib.ERR_CAPACITY
    assert L().trpx_last_error_string().startswith(b"trpx_decode_sparse")


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    rows = (C.c_uint64 * 3)()
    pos = (C.c_uint32 * 24)()
    vals = (C.c_uint16 * 24)()
    found = C.c_size_t(0)

    def host(dtype=_lib.U16, block=12, n_values=12, positions=pos, values=vals, capacity=24, row_offsets=rows):
        return L().trpx_decode_sparse_host(dtype, buf, 64, None, n_values, 2, block, 1, row_offsets, positions, values, capacity,
                                           C.byref(found), -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(n_values=0), _lib.ERR_INVALID_ARG),
                     (dict(row_offsets=None), _lib.ERR_INVALID_ARG), (dict(positions=None), _lib.ERR_INVALID_ARG),
                     (dict(values=None), _lib.ERR_INVALID_ARG), (dict(positions=None, values=None, capacity=5), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_decode_sparse")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device
        assert host(positions=None, values=None, capacity=0) == _lib.ERR_NO_DEVICE
