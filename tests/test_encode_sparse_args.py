"""CPU tier: trpx_encode_sparse's four symbols are exported and bound, its argument errors are return codes decided before any
device call (the pointers below are fake, aligned addresses: a call that reached the device would fail differently), and the
host form validates its arguments and the event lists before a device is looked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from trpx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VALUES, N_FRAMES, N_EVENTS = 512 * 512, 8, 1000
ROWS, POS, VALS, OUT, OFFS, STATUS, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000


def L():
    return _lib.lib()


def _encode(dtype=_lib.U16, rows=ROWS, pos=POS, vals=VALS, n_events=N_EVENTS, n_values=N_VALUES, n_frames=N_FRAMES, block=12,
            out=OUT, capacity=1 << 20, offs=OFFS, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_encode_sparse(dtype, rows, pos, vals, n_events, n_values, n_frames, block, out, capacity, offs, status, ws,
                                  ws_bytes, None)


def test_symbols_are_exported_and_bound():
    names = ("trpx_encode_sparse_workspace_bytes", "trpx_encode_sparse_bound_bytes", "trpx_encode_sparse", "trpx_encode_sparse_host")
    for name in names:
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
    _P, _SZ, _U, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert _lib.SYMBOLS["trpx_encode_sparse_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _U])
    assert _lib.SYMBOLS["trpx_encode_sparse_bound_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U])
    assert _lib.SYMBOLS["trpx_encode_sparse"] == (_I, [_I, _P, _P, _P, _SZ, _SZ, _SZ, _U, _P, _SZ, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_encode_sparse_host"] == (_I, [_I, _P, _P, _P, _SZ, _SZ, _SZ, _U, _P, _SZ, C.POINTER(_SZ), _P,
                                                          C.POINTER(_U), _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_workspace_bytes_is_arithmetic():
    f = L().trpx_encode_sparse_workspace_bytes
    n = f(_lib.U16, N_VALUES, N_FRAMES, 12)
    assert n > 0 and n % 8 == 0
    assert f(_lib.U16, N_VALUES, N_FRAMES, 7) == 0          # block 7
    assert f(_lib.U64, N_VALUES, N_FRAMES, 12) == 0 and f(_lib.I64, N_VALUES, N_FRAMES, 12) == 0
    assert f(_lib.F32, N_VALUES, N_FRAMES, 12) == 0 and f(42, N_VALUES, N_FRAMES, 12) == 0
    assert f(_lib.U16, 0, N_FRAMES, 12) == 0 and f(_lib.U16, N_VALUES, 0, 12) == 0
    assert f(_lib.U8, 1 << 32, 1, 12) == 0                  # positions are 32-bit
    # 16 bytes per 256-block tile (offset, bits, first event) and 8 per frame; nothing per pixel, whatever the type
    for dt in (_lib.U8, _lib.I16, _lib.U32):
        for n_values, n_frames in ((1, 1), (3072, 5), (3073, 5), (N_VALUES, N_FRAMES), (12 * 65536 + 1, 3), ((1 << 32) - 1, 2)):
            tiles = n_frames * L().trpx_group_count(n_values, 12)
            need = f(dt, n_values, n_frames, 12)
            assert 0 < need <= 16 * tiles + 8 * n_frames + 8, (dt, n_values, n_frames)
            assert need == f(_lib.U8, n_values, n_frames, 12)
    assert f(_lib.U16, 3072 * 100, 7, 12) == f(_lib.U16, 3072 * 99 + 1, 7, 12)   # grows with tiles, not with n_values


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(block=0), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U8, n_values=1 << 32, n_frames=1), _lib.ERR_UNSUPPORTED),   # positions are 32-bit
    # TRPX_ERR_INVALID_ARG
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),            # float and unknown dtypes
    (dict(dtype=_lib.F64), _lib.ERR_INVALID_ARG),
    (dict(dtype=42), _lib.ERR_INVALID_ARG),
    (dict(dtype=-1), _lib.ERR_INVALID_ARG),
    (dict(n_values=0), _lib.ERR_INVALID_ARG),                # zero sizes
    (dict(n_frames=0), _lib.ERR_INVALID_ARG),
    (dict(rows=None), _lib.ERR_INVALID_ARG),                 # null pointers
    (dict(offs=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(ws=None), _lib.ERR_INVALID_ARG),
    (dict(rows=ROWS + 4), _lib.ERR_INVALID_ARG),             # misaligned pointers
    (dict(pos=POS + 2), _lib.ERR_INVALID_ARG),
    (dict(vals=VALS + 1), _lib.ERR_INVALID_ARG),             # (u16 values)
    (dict(out=OUT + 8), _lib.ERR_INVALID_ARG),
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(pos=None), _lib.ERR_INVALID_ARG),                  # values without positions
    (dict(vals=None), _lib.ERR_INVALID_ARG),                 # positions without values
    (dict(pos=None, vals=None), _lib.ERR_INVALID_ARG),       # events without lists
    (dict(pos=None, n_events=0), _lib.ERR_INVALID_ARG),      # one NULL without the other, no events
    (dict(out=None), _lib.ERR_INVALID_ARG),                  # out NULL with a capacity
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0), _lib.ERR_CAPACITY),                   # workspace too small
])
def test_argument_errors_are_return_codes(kw, code):
    assert _encode(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_encode_sparse")


def test_legal_forms_pass_the_argument_checks():
    # a sizes-only query and a stack of empty frames pass every check: the first thing to fail is the workspace that is one word short
    need = L().trpx_encode_sparse_workspace_bytes(_lib.U16, N_VALUES, N_FRAMES, 12)
    assert _encode(out=None, capacity=0, ws_bytes=need - 8) == _lib.ERR_CAPACITY
    assert _encode(pos=None, vals=None, n_events=0, ws_bytes=need - 8) == _lib.ERR_CAPACITY
    assert _encode(dtype=_lib.I32, vals=VALS + 4, ws_bytes=need - 8) == _lib.ERR_CAPACITY
    assert L().trpx_last_error_string().startswith(b"trpx_encode_sparse")


def test_bound_bytes_of_what_is_not_supported():
    f = L().trpx_encode_sparse_bound_bytes
    assert f(_lib.U16, N_VALUES, N_FRAMES, N_EVENTS, 12) > 0
    assert f(_lib.U16, N_VALUES, N_FRAMES, N_EVENTS, 7) == 0
    assert f(_lib.U64, N_VALUES, N_FRAMES, N_EVENTS, 12) == 0 and f(_lib.F32, N_VALUES, N_FRAMES, N_EVENTS, 12) == 0
    assert f(_lib.U16, 0, N_FRAMES, N_EVENTS, 12) == 0 and f(_lib.U16, N_VALUES, 0, N_EVENTS, 12) == 0
    assert f(_lib.U8, 1 << 32, 1, 0, 12) == 0


def test_host_wrapper_checks_arguments_and_events_before_the_device():
    n_values = 6149
    rows = np.array([2, 6, 6, 9], np.uint64)                # 4, 0 and 3 events behind two events of no frame
    pos = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0, 11, 3072, 6148, 5, 6, 7], np.uint32)
    vals = np.arange(9, dtype=np.uint16)
    out = np.zeros(4096, np.uint8)
    total, pb = C.c_size_t(0), C.c_uint(0)

    def host(dtype=_lib.U16, rows=rows, pos=pos, vals=vals, n_events=9, n_values=n_values, n_frames=3, block=12, out=out,
             total=total):
        p = lambda a: a.ctypes.data if a is not None else None
        return L().trpx_encode_sparse_host(dtype, p(rows), p(pos), p(vals), n_events, n_values, n_frames, block, p(out),
                                           out.size if out is not None else 0, C.byref(total) if total is not None else None, None,
                                           C.byref(pb), -1)

    def bent(i, v, what=pos):
        a = what.copy()
        a[i] = v
        return a

    # the same answers with and without a GPU: nothing below gets as far as looking for one
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(n_values=1 << 32), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(n_values=0), _lib.ERR_INVALID_ARG), (dict(n_frames=0), _lib.ERR_INVALID_ARG),
                     (dict(rows=None), _lib.ERR_INVALID_ARG), (dict(out=None), _lib.ERR_INVALID_ARG), (dict(total=None), _lib.ERR_INVALID_ARG),
                     (dict(pos=None), _lib.ERR_INVALID_ARG), (dict(vals=None), _lib.ERR_INVALID_ARG),
                     (dict(pos=None, vals=None), _lib.ERR_INVALID_ARG),
                     # the events
                     (dict(pos=bent(5, n_values)), _lib.ERR_INVALID_ARG),              # out of range
                     (dict(pos=bent(8, 0xFFFFFFFF)), _lib.ERR_INVALID_ARG),
                     (dict(pos=bent(3, 3072)), _lib.ERR_INVALID_ARG),                  # a duplicate
                     (dict(pos=bent(4, 5)), _lib.ERR_INVALID_ARG),                     # unsorted
                     (dict(rows=bent(2, 5, rows)), _lib.ERR_INVALID_ARG),              # a decreasing row
                     (dict(rows=bent(3, 10, rows)), _lib.ERR_INVALID_ARG),             # ends beyond the events
                     (dict(n_events=8), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_encode_sparse_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device
        assert host(rows=np.zeros(4, np.uint64), pos=None, vals=None, n_events=0) == _lib.ERR_NO_DEVICE


def test_host_checks_under_the_sanitizers():
    """The event validation and the bound on lists in exact-size allocations, under ASan + UBSan (a stand-alone CPU program)."""
    exe = os.path.join(ROOT, "tests", "cpp", "encode_sparse_sanitize")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "encode_sparse_example.mk", "encode_sparse_sanitize"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK encode sparse host checks" in r.stdout, r.stdout + r.stderr
