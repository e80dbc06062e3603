"""CPU tier: trpx_decode_bins's four symbols are exported and bound, its workspace size and its spans per frame are arithmetic,
its argument errors are return codes decided before any device call (the pointers below are fake, aligned addresses: a call that
reached the device would fail differently), and what a lane does with a block (trpx_amd/csrc/bins_merge.hpp) is clean under
ASan + UBSan in a stand-alone CPU program."""
import ctypes as C
import os
import subprocess

import pytest

from trpx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VALUES, N_FRAMES, TERSE_BYTES, N_BINS = 512 * 512, 8, 1 << 20, 256
TERSE, OFFS, INDEX, LABELS, BINS, STATUS, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x70000, 0x80000
RUN, WAVES, TARGET = 8, 4, 1536                            # groups per run, wavefronts per workgroup, workgroups a launch aims at


def L():
    return _lib.lib()


def _bins(dtype=_lib.U16, terse=TERSE, terse_bytes=TERSE_BYTES, offs=OFFS, index=INDEX, n_values=N_VALUES, n_frames=N_FRAMES, block=12,
          labels=LABELS, n_bins=N_BINS, bins=BINS, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_bins(dtype, terse, terse_bytes, offs, index, n_values, n_frames, block, labels, n_bins, bins, status, ws,
                                ws_bytes, None)


def _spans(n_values, n_frames):
    """min(ceil(runs per frame / 4), max(1, ceil(TARGET / n_frames)))"""
    runs = -(-L().trpx_group_count(n_values, 12) // RUN)
    return min(-(-runs // WAVES), max(1, -(-TARGET // n_frames)))


def _support_bytes(n_values=N_VALUES):
    return (4 * -(-(-(-n_values // 12)) // 32) + 7) // 8 * 8


def test_symbols_are_exported_and_bound():
    names = ("trpx_decode_bins_workspace_bytes", "trpx_decode_bins_spans_per_frame", "trpx_decode_bins", "trpx_decode_bins_host")
    for name in names:
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L(), name).restype == _lib.SYMBOLS[name][0]
    _P, _SZ, _U, _I = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
    assert _lib.SYMBOLS["trpx_decode_bins_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U, _U])
    assert _lib.SYMBOLS["trpx_decode_bins_spans_per_frame"] == (_U, [_SZ, _SZ])
    assert _lib.SYMBOLS["trpx_decode_bins"] == (_I, [_I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _P, _U, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_bins_host"] == (_I, [_I, _P, _SZ, _P, _SZ, _SZ, _U, _P, _U, _P, _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_header_declares_them_and_lists_the_call_under_restated_widths():
    text = open(os.path.join(ROOT, "include", "trpx_hip.h")).read()
    for name in ("trpx_decode_bins_workspace_bytes(", "unsigned trpx_decode_bins_spans_per_frame(", "int trpx_decode_bins(",
                 "int trpx_decode_bins_host("):
        assert name in text
    top = text[text.index("Restated widths."):text.index("Status 0 with pixels that are not the stream's")]
    assert "trpx_decode_bins" in top
    assert "#define TRPX_ABI_VERSION 3" in text


@pytest.mark.parametrize("n_values, n_frames, want", [
    (512 * 512, 2000, 1),                                   # the flagship stack: a workgroup per frame
    (122893, 1, 2), (122893, 3, 2), (122893, 5, 2),         # five runs and a tail: two spans (the GPU tier's reduce case)
    (4096 * 4096, 8, 171),                                  # 683 runs: ceil(683 / 4) = 171 < ceil(1536 / 8) = 192
    (4096 * 4096, 64, 24),                                  # ... and bounded by the frames: ceil(1536 / 64)
    (4096 * 4096, 1536, 1), (4096 * 4096, 1537, 1),
    (1, 1, 1), (12, 7, 1), (24577, 1, 1), (24576 * 4, 1, 1), (24576 * 4 + 1, 1, 2),    # up to four runs (of 8 x 256 x 12 values): one span
])
def test_spans_per_frame_is_arithmetic(n_values, n_frames, want):
    assert L().trpx_decode_bins_spans_per_frame(n_values, n_frames) == want == _spans(n_values, n_frames)


def test_spans_per_frame_is_zero_for_sizes_no_call_takes():
    assert L().trpx_decode_bins_spans_per_frame(0, 8) == 0
    assert L().trpx_decode_bins_spans_per_frame(N_VALUES, 0) == 0


@pytest.mark.parametrize("n_bins", [1, 37, 256, 4096])
@pytest.mark.parametrize("n_values, n_frames", [(N_VALUES, N_FRAMES), (N_VALUES, 2000), (122893, 3), (4096 * 4096, 8), (13, 1)])
def test_workspace_bytes_is_arithmetic(n_bins, n_values, n_frames):
    terse_bytes = max(TERSE_BYTES, n_frames)
    n = L().trpx_decode_bins_workspace_bytes(_lib.U16, terse_bytes, n_values, n_frames, 12, n_bins)
    front = L().trpx_decode_roi_workspace_bytes(_lib.U16, terse_bytes, n_values, n_frames, 12)
    assert front > 0 and n % 8 == 0
    spans = L().trpx_decode_bins_spans_per_frame(n_values, n_frames)
    # beyond the front: the support words, and the spans' partial sums where a frame is more than one span -- nothing otherwise
    assert n - front == _support_bytes(n_values) + (8 * n_bins * n_frames * spans if spans > 1 else 0)


def test_workspace_bytes_is_zero_for_what_the_call_does_not_support():
    f = L().trpx_decode_bins_workspace_bytes
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7, 3) == 0               # block 7
    assert f(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 3) == 0              # 64-bit container
    assert f(_lib.F32, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 3) == 0              # not a stream type
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 0) == 0              # no bins
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 4097) == 0           # too many bins
    assert f(_lib.U16, TERSE_BYTES, 0, N_FRAMES, 12, 3) == 0
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, 0, 12, 3) == 0
    assert f(_lib.U16, 0, N_VALUES, N_FRAMES, 12, 3) == 0
    for dt in (_lib.U8, _lib.I8, _lib.U16, _lib.I16, _lib.U32, _lib.I32):
        assert f(dt, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 4096) > 0


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
    (dict(n_bins=0), _lib.ERR_INVALID_ARG),                  # the number of bins
    (dict(n_bins=4097), _lib.ERR_INVALID_ARG),
    (dict(n_bins=0xFFFF), _lib.ERR_INVALID_ARG),
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(labels=None), _lib.ERR_INVALID_ARG),
    (dict(bins=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(labels=LABELS + 1), _lib.ERR_INVALID_ARG),
    (dict(bins=BINS + 4), _lib.ERR_INVALID_ARG),
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    (dict(ws=None), _lib.ERR_INVALID_ARG),                   # no workspace: the support bits live there
    (dict(offs=None, index=None, ws=None), _lib.ERR_INVALID_ARG),
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0), _lib.ERR_CAPACITY),                   # workspace too small for the support words
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),       # ... and for the index
])
def test_argument_errors_are_return_codes(kw, code):
    assert _bins(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_bins")


def test_labels_need_only_two_byte_alignment():
    # 2-byte aligned labels pass every check: the first thing to fail is the workspace that is one word short
    for shift in (2, 4, 6):
        assert _bins(labels=LABELS + shift, ws_bytes=8) == _lib.ERR_CAPACITY


@pytest.mark.parametrize("n_bins", [1, 256, 4096])
@pytest.mark.parametrize("n_values, n_frames", [(N_VALUES, N_FRAMES), (N_VALUES, 2000), (122893, 3)])
def test_workspace_one_word_short(n_bins, n_values, n_frames):
    need = L().trpx_decode_bins_workspace_bytes(_lib.U16, TERSE_BYTES, n_values, n_frames, 12, n_bins)
    kw = dict(n_values=n_values, n_frames=n_frames, n_bins=n_bins)
    assert _bins(offs=None, index=None, ws_bytes=need - 8, **kw) == _lib.ERR_CAPACITY        # without offsets: the whole need
    assert L().trpx_last_error_string().startswith(b"trpx_decode_bins")
    # with offsets and index given less is needed, and the call checks against its own form's need: the support words and, with
    # more than one span per frame, the partial sums
    spans = L().trpx_decode_bins_spans_per_frame(n_values, n_frames)
    own = _support_bytes(n_values) + (8 * n_bins * n_frames * spans if spans > 1 else 0)
    assert own < need
    assert _bins(ws_bytes=own - 8, **kw) == _lib.ERR_CAPACITY
    assert L().trpx_last_error_string().startswith(b"trpx_decode_bins")


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    lab = (C.c_uint16 * 12)()
    bins = (C.c_int64 * 8)()

    def host(dtype=_lib.U16, block=12, n_values=12, labels=lab, n_bins=4, out=bins, terse=buf):
        return L().trpx_decode_bins_host(dtype, terse, 64, None, n_values, 2, block, labels, n_bins, out, -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(n_values=0), _lib.ERR_INVALID_ARG), (dict(labels=None), _lib.ERR_INVALID_ARG),
                     (dict(out=None), _lib.ERR_INVALID_ARG), (dict(terse=None), _lib.ERR_INVALID_ARG),
                     (dict(n_bins=0), _lib.ERR_INVALID_ARG), (dict(n_bins=4097), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_decode_bins_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device


def test_block_merge_under_the_sanitizers():
    """bins_merge.hpp -- the text the kernels run -- over exact-size heap arrays: every block length 1 .. 12, labels all equal,
    all different, changing at every position, the edge labels n_bins - 1, n_bins and 0xFFFF first and last, the values 0, the
    type's minimum and maximum, at every 2-byte alignment of the map, against a plain per-pixel loop, under ASan + UBSan (a
    stand-alone CPU program)."""
    exe = os.path.join(ROOT, "tests", "cpp", "bins_sanitize")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "bins_example.mk", "bins_sanitize"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK bins_sanitize" in r.stdout, r.stdout + r.stderr
