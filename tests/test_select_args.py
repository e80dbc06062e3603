"""CPU tier: trpx_select_frames' three symbols are exported and bound, its workspace size is arithmetic, its argument errors are
return codes decided before any device call (the pointers below are fake, aligned addresses: a call that reached the device
would fail differently), the host form judges the list before it looks for a device, and the output map the copy kernel runs
(trpx_amd/csrc/select_map.hpp) holds under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from trpx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VALUES, N_FRAMES, N_SELECT, TERSE_BYTES = 512 * 512, 8, 5, 1 << 20
TERSE, OFFS, INDEX, FRAMES, OUT, OUT_OFFS, OUT_INDEX, STATUS, WS = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000,
                                                                    0x80000, 0x90000)


def L():
    return _lib.lib()


def _select(dtype=_lib.U16, terse=TERSE, terse_bytes=TERSE_BYTES, offs=OFFS, index=None, n_values=N_VALUES, n_frames=N_FRAMES, block=12,
            frames=FRAMES, n_select=N_SELECT, out=OUT, cap=1 << 20, out_offs=OUT_OFFS, out_index=None, status=STATUS, ws=WS,
            ws_bytes=1 << 40):
    return L().trpx_select_frames(dtype, terse, terse_bytes, offs, index, n_values, n_frames, block, frames, n_select, out, cap, out_offs,
                                  out_index, status, ws, ws_bytes, None)


def test_symbols_are_exported_and_bound():
    for name in ("trpx_select_frames_workspace_bytes", "trpx_select_frames", "trpx_select_frames_host"):
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L(), name).restype == _lib.SYMBOLS[name][0]
    _P, _SZ, _U, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert _lib.SYMBOLS["trpx_select_frames_workspace_bytes"] == (_SZ, [_SZ, _SZ])
    assert _lib.SYMBOLS["trpx_select_frames"] == (_I, [_I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _P, _SZ, _P, _SZ, _P, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_select_frames_host"] == (_I, [_I, _P, _SZ, _P, _SZ, _SZ, _U, _P, _SZ, _P, _SZ, _P, C.POINTER(_SZ), _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "trpx_hip.h")).read()
    for name in ("trpx_select_frames_workspace_bytes(", "int trpx_select_frames(", "int trpx_select_frames_host("):
        assert name in text
    doc = text[text.index("Select frames of a stack"):text.index("size_t trpx_select_frames_workspace_bytes(")]
    assert "Terse.hpp:502-505" in doc and "MUST NOT OVERLAP" in doc
    assert "#define TRPX_ABI_VERSION 3" in text


@pytest.mark.parametrize("n_select", [1, 5, 256, 257, 2000, 1 << 20])
def test_workspace_bytes_is_arithmetic(n_select):
    f = L().trpx_select_frames_workspace_bytes
    n = f(N_FRAMES, n_select)
    # the selected sizes (8 bytes each) and one verdict word per 256 entries: nothing in proportion to the bytes moved
    assert n % 8 == 0 and 8 * n_select + 4 * -(-n_select // 256) <= n <= 8 * n_select + 4 * -(-n_select // 256) + 8
    assert f(1, n_select) == n and f(1 << 30, n_select) == n                     # the source's size adds nothing


def test_workspace_bytes_is_zero_for_what_the_call_refuses():
    f = L().trpx_select_frames_workspace_bytes
    assert f(0, 5) == 0 and f(8, 0) == 0 and f(8, 1 << 31) == 0


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=0), _lib.ERR_UNSUPPORTED),
    (dict(block=4097), _lib.ERR_UNSUPPORTED),
    (dict(block=7, index=INDEX, out_index=OUT_INDEX), _lib.ERR_UNSUPPORTED),     # an index needs block 12 ...
    (dict(dtype=_lib.U64, index=INDEX, out_index=OUT_INDEX), _lib.ERR_UNSUPPORTED),   # ... and pixels of <= 32 bits
    (dict(dtype=_lib.I64, index=INDEX, out_index=OUT_INDEX), _lib.ERR_UNSUPPORTED),
    # TRPX_ERR_INVALID_ARG
    (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),            # float dtype: not a stream type
    (dict(dtype=42), _lib.ERR_INVALID_ARG),                  # unknown dtype
    (dict(dtype=-1), _lib.ERR_INVALID_ARG),
    (dict(n_values=0), _lib.ERR_INVALID_ARG),                # zero sizes
    (dict(n_frames=0), _lib.ERR_INVALID_ARG),
    (dict(terse_bytes=0), _lib.ERR_INVALID_ARG),
    (dict(n_select=0), _lib.ERR_INVALID_ARG),
    (dict(n_frames=9, terse_bytes=8), _lib.ERR_INVALID_ARG),   # more frames than bytes
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # frame_offsets is mandatory
    (dict(frames=None), _lib.ERR_INVALID_ARG),
    (dict(out_offs=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(ws=None), _lib.ERR_INVALID_ARG),
    (dict(out=None), _lib.ERR_INVALID_ARG),                  # out NULL with a capacity
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(frames=FRAMES + 2), _lib.ERR_INVALID_ARG),
    (dict(out=OUT + 8), _lib.ERR_INVALID_ARG),
    (dict(out_offs=OUT_OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8, out_index=OUT_INDEX), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX, out_index=OUT_INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(out_index=OUT_INDEX), _lib.ERR_INVALID_ARG),       # out_index without index
    (dict(index=INDEX), _lib.ERR_INVALID_ARG),               # ... and the other way round: they go together
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0), _lib.ERR_CAPACITY),
    (dict(ws_bytes=8 * N_SELECT), _lib.ERR_CAPACITY),        # the sizes fit, the verdict word does not
])
def test_argument_errors_are_return_codes(kw, code):
    assert _select(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_select_frames")


def test_weakest_alignments_and_every_block_and_dtype_pass_the_checks():
    # what the header allows passes every check: the first thing to fail is the workspace that is one word short
    short = L().trpx_select_frames_workspace_bytes(N_FRAMES, N_SELECT) - 8
    assert _select(terse=TERSE + 4, frames=FRAMES + 4, out=OUT + 16, offs=OFFS + 8, out_offs=OUT_OFFS + 8, ws_bytes=short) == _lib.ERR_CAPACITY
    for block in (1, 7, 12, 4096):
        assert _select(block=block, ws_bytes=short) == _lib.ERR_CAPACITY
    for dt in (_lib.U8, _lib.I8, _lib.U16, _lib.I16, _lib.U32, _lib.I32, _lib.U64, _lib.I64):
        assert _select(dtype=dt, ws_bytes=short) == _lib.ERR_CAPACITY
    assert _select(out=None, cap=0, ws_bytes=short) == _lib.ERR_CAPACITY         # the sizes-only query
    assert _select(n_select=100, ws_bytes=8 * 100) == _lib.ERR_CAPACITY          # a list longer than the stack
    assert _select(index=INDEX, out_index=OUT_INDEX, ws_bytes=short) == _lib.ERR_CAPACITY


def test_host_wrapper_checks_arguments_and_list_before_the_device():
    buf = (C.c_uint8 * 64)()
    offs = np.array([0, 10, 30, 64], np.uint64)
    out = (C.c_uint8 * 256)()
    out_offs = np.zeros(8, np.uint64)
    total = C.c_size_t(0)

    def host(dtype=_lib.U16, block=12, n_values=12, terse=buf, terse_bytes=64, o=offs, frames=(2, 0), dst=out, cap=256, tot=total):
        fr = np.array(frames, np.uint32)
        return L().trpx_select_frames_host(dtype, terse, terse_bytes, o.ctypes.data if o is not None else None, n_values, 3, block,
                                           fr.ctypes.data if fr.size else None, fr.size, dst, cap, out_offs.ctypes.data,
                                           C.byref(tot) if tot is not None else None, -1)

    beyond, decreasing = offs.copy(), offs.copy()
    beyond[3] = 65
    decreasing[1], decreasing[2] = 30, 10
    # the same answers with and without a GPU
    for kw, code in [(dict(block=0), _lib.ERR_UNSUPPORTED), (dict(block=4097), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(n_values=0), _lib.ERR_INVALID_ARG), (dict(terse=None), _lib.ERR_INVALID_ARG),
                     (dict(o=None), _lib.ERR_INVALID_ARG), (dict(dst=None), _lib.ERR_INVALID_ARG), (dict(tot=None), _lib.ERR_INVALID_ARG),
                     (dict(frames=()), _lib.ERR_INVALID_ARG), (dict(terse_bytes=2), _lib.ERR_INVALID_ARG),
                     (dict(frames=(0, 3)), _lib.ERR_INVALID_ARG),               # the list: an entry equal to n_frames ...
                     (dict(frames=(0xFFFFFFFF,)), _lib.ERR_INVALID_ARG),         # ... and far outside
                     (dict(o=beyond, frames=(2,)), _lib.ERR_CORRUPT),            # offsets that leave the stream
                     (dict(o=decreasing, frames=(0, 1)), _lib.ERR_CORRUPT),      # ... or decrease
                     (dict(frames=(2, 2, 2, 2, 2, 2, 2, 2), cap=200), _lib.ERR_CAPACITY)]:   # 8 x 34 bytes
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_select_frames_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device
        assert host(o=beyond, frames=(0, 1)) == _lib.ERR_NO_DEVICE               # only selected frames are judged
        assert host(block=7, dtype=_lib.I64) == _lib.ERR_NO_DEVICE               # bytes only: every block, every container


def test_output_map_under_the_sanitizers():
    """select_map.hpp -- the text the copy kernel runs -- writing every line of every GPU-tier shape into exact-size heap arrays,
    at the capacity edges and with bad lists and offsets, under ASan + UBSan (a stand-alone CPU program)."""
    exe = os.path.join(ROOT, "tests", "cpp", "select_sanitize")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "select_example.mk", "select_sanitize"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK select map checks" in r.stdout, r.stdout + r.stderr
