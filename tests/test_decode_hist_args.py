"""CPU tier: trpx_decode_hist's four symbols are exported and bound, its workspace size and its spans per group are arithmetic,
its argument errors are return codes decided before any device call (the pointers below are fake, aligned addresses: a call that
reached the device would fail differently), and the bin rule (trpx_amd/csrc/hist_bin.hpp) is clean under ASan + UBSan in a
stand-alone CPU program."""
import ctypes as C
import os
import subprocess

import pytest

from trpx_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_VALUES, N_FRAMES, TERSE_BYTES, N_BINS = 512 * 512, 8, 1 << 20, 256
TERSE, OFFS, INDEX, HIST, STATUS, WS = 0x10000, 0x20000, 0x30000, 0x50000, 0x70000, 0x80000
RUN, WAVES, TARGET, MAX_SPAN_RUNS = 8, 4, 1536, 1 << 17    # groups per run, wavefronts per workgroup, workgroups aimed at, runs a span may hold


def L():
    return _lib.lib()


def _hist(dtype=_lib.U16, terse=TERSE, terse_bytes=TERSE_BYTES, offs=OFFS, index=INDEX, n_values=N_VALUES, n_frames=N_FRAMES, block=12,
          group=1, lo=0, shift=0, n_bins=N_BINS, hist=HIST, status=STATUS, ws=WS, ws_bytes=1 << 40):
    return L().trpx_decode_hist(dtype, terse, terse_bytes, offs, index, n_values, n_frames, block, group, lo, shift, n_bins, hist, status,
                                ws, ws_bytes, None)


def _spans(n_values, n_frames, group):
    """max(ceil(R / 2^17), min(ceil(R / 4), max(1, ceil(TARGET / G)))), R the runs of a full group, G the groups"""
    frames = min(group, n_frames)
    n_groups = -(-n_frames // frames)
    runs = frames * -(-L().trpx_group_count(n_values, 12) // RUN)
    return max(-(-runs // MAX_SPAN_RUNS), min(-(-runs // WAVES), max(1, -(-TARGET // n_groups))))


def test_symbols_are_exported_and_bound():
    names = ("trpx_decode_hist_workspace_bytes", "trpx_decode_hist_spans_per_group", "trpx_decode_hist", "trpx_decode_hist_host")
    for name in names:
        assert name in _lib.SYMBOLS
        assert getattr(L(), name).argtypes == _lib.SYMBOLS[name][1]
        assert getattr(L(), name).restype == _lib.SYMBOLS[name][0]
    _P, _SZ, _U, _I, _I64 = C.c_void_p, C.c_size_t, C.c_uint, C.c_int, C.c_int64
    assert _lib.SYMBOLS["trpx_decode_hist_workspace_bytes"] == (_SZ, [_I, _SZ, _SZ, _SZ, _U, _SZ, _U])
    assert _lib.SYMBOLS["trpx_decode_hist_spans_per_group"] == (_U, [_SZ, _SZ, _SZ])
    assert _lib.SYMBOLS["trpx_decode_hist"] == (_I, [_I, _P, _SZ, _P, _P, _SZ, _SZ, _U, _SZ, _I64, _U, _U, _P, _P, _P, _SZ, _P])
    assert _lib.SYMBOLS["trpx_decode_hist_host"] == (_I, [_I, _P, _SZ, _P, _SZ, _SZ, _U, _SZ, _I64, _U, _U, _P, _I])
    assert L().trpx_abi_version() == 3                      # symbols added, no layout changed


def test_header_declares_them_and_lists_the_call_under_restated_widths():
    text = open(os.path.join(ROOT, "include", "trpx_hip.h")).read()
    for name in ("trpx_decode_hist_workspace_bytes(", "unsigned trpx_decode_hist_spans_per_group(", "int trpx_decode_hist(",
                 "int trpx_decode_hist_host("):
        assert name in text
    top = text[text.index("Restated widths."):text.index("Status 0 with pixels that are not the stream's")]
    assert "trpx_decode_hist" in top
    assert "#define TRPX_ABI_VERSION 3" in text


@pytest.mark.parametrize("n_values, n_frames, group, want", [
    (512 * 512, 2000, 1, 1),                                # the flagship stack per frame: a workgroup per frame, nothing through the workspace
    (512 * 512, 2000, 2000, 1536),                          # ... and as one group: 22000 runs, not one workgroup
    (512 * 512, 2000, 5000, 1536),                          # (a group larger than the stack: one group)
    (512 * 512, 2000, 2, 2),                                # 1000 groups: ceil(1536 / 1000)
    (122893, 1, 1, 2), (122893, 3, 1, 2), (122893, 5, 1, 2),    # five runs and a tail: two spans (the GPU tier's reduce case)
    (122893, 5, 2, 3), (122893, 5, 5, 8),                   # ceil(12 / 4), ceil(30 / 4)
    (4096 * 4096, 8, 1, 171), (4096 * 4096, 8, 8, 1366),    # 683 runs a frame: ceil(683 / 4) < ceil(1536 / 8); ceil(5464 / 4) < 1536
    (1, 1, 1, 1), (12, 7, 1, 1), (12, 7, 7, 2), (24577, 1, 1, 1), (24576 * 4, 1, 1, 1), (24576 * 4 + 1, 1, 1, 2),
    (8, (1 << 24) - 1, (1 << 24) - 1, 1536),                # 2^24 - 1 runs in one group: 128 spans would keep the counters, 1536 are aimed at
])
def test_spans_per_group_is_arithmetic(n_values, n_frames, group, want):
    assert L().trpx_decode_hist_spans_per_group(n_values, n_frames, group) == want == _spans(n_values, n_frames, group)


def test_a_span_holds_fewer_than_2_32_values():
    # the 32-bit counters in LDS: runs of 8 x 256 x 12 values, at most 2^17 of them
    assert MAX_SPAN_RUNS * RUN * 256 * 12 < 1 << 32
    for n_values, n_frames, group in [(8, (1 << 24) - 1, (1 << 24) - 1), (512 * 512, 2000, 2000), (1 << 28, 15, 15)]:
        spans = L().trpx_decode_hist_spans_per_group(n_values, n_frames, group)
        runs = min(group, n_frames) * -(-L().trpx_group_count(n_values, 12) // RUN)
        assert spans >= 1 and -(-runs // spans) <= MAX_SPAN_RUNS


def test_spans_per_group_is_zero_for_sizes_no_call_takes():
    f = L().trpx_decode_hist_spans_per_group
    assert f(0, 8, 1) == 0
    assert f(N_VALUES, 0, 1) == 0
    assert f(N_VALUES, 8, 0) == 0
    assert f(8, (1 << 24) + 3, 1) == 0 and f(8, 1 << 30, 1 << 20) == 0          # more groups of 256 blocks than one call takes
    assert f(8, (1 << 24) - 1, 1) == 1                                           # ... and the most it takes


@pytest.mark.parametrize("n_bins", [1, 37, 256, 4096])
@pytest.mark.parametrize("n_values, n_frames, group", [(N_VALUES, N_FRAMES, 1), (N_VALUES, 2000, 1), (N_VALUES, 2000, 2000), (122893, 5, 2),
                                                       (4096 * 4096, 8, 8), (13, 1, 1)])
def test_workspace_bytes_is_arithmetic(n_bins, n_values, n_frames, group):
    terse_bytes = max(TERSE_BYTES, n_frames)
    n = L().trpx_decode_hist_workspace_bytes(_lib.U16, terse_bytes, n_values, n_frames, 12, group, n_bins)
    front = L().trpx_decode_roi_workspace_bytes(_lib.U16, terse_bytes, n_values, n_frames, 12)
    assert front > 0 and n % 8 == 0
    spans = L().trpx_decode_hist_spans_per_group(n_values, n_frames, group)
    n_groups = -(-n_frames // min(group, n_frames))
    # beyond the front: the spans' partial counts where a group is more than one span -- nothing otherwise
    assert n - front == (8 * n_bins * n_groups * spans if spans > 1 else 0)


def test_workspace_bytes_is_zero_for_what_the_call_does_not_support():
    f = L().trpx_decode_hist_workspace_bytes
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 7, 1, 3) == 0            # block 7
    assert f(_lib.U64, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 1, 3) == 0           # 64-bit container
    assert f(_lib.F32, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 1, 3) == 0           # not a stream type
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 1, 0) == 0           # no bins
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 1, 4097) == 0        # too many bins
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 0, 3) == 0           # no group
    assert f(_lib.U16, TERSE_BYTES, 0, N_FRAMES, 12, 1, 3) == 0
    assert f(_lib.U16, TERSE_BYTES, N_VALUES, 0, 12, 1, 3) == 0
    assert f(_lib.U16, 0, N_VALUES, N_FRAMES, 12, 1, 3) == 0
    assert f(_lib.U8, 1 << 25, 8, (1 << 24) + 3, 12, 1, 3) == 0                  # more groups of 256 blocks than one call takes
    assert f(_lib.U8, 1 << 25, 8, (1 << 24) - 1, 12, 1, 3) > 0
    for dt in (_lib.U8, _lib.I8, _lib.U16, _lib.I16, _lib.U32, _lib.I32):
        assert f(dt, TERSE_BYTES, N_VALUES, N_FRAMES, 12, 1, 4096) > 0


@pytest.mark.parametrize("kw, code", [
    # TRPX_ERR_UNSUPPORTED
    (dict(block=7), _lib.ERR_UNSUPPORTED),
    (dict(block=0), _lib.ERR_UNSUPPORTED),
    (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),            # a 64-bit dtype
    (dict(dtype=_lib.I64), _lib.ERR_UNSUPPORTED),
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
    (dict(n_bins=0), _lib.ERR_INVALID_ARG),                  # the number of bins
    (dict(n_bins=4097), _lib.ERR_INVALID_ARG),
    (dict(shift=33), _lib.ERR_INVALID_ARG),                  # the bin width
    (dict(lo=(1 << 32) + 1), _lib.ERR_INVALID_ARG),          # the first bin's edge
    (dict(lo=-(1 << 32) - 1), _lib.ERR_INVALID_ARG),
    (dict(lo=-(1 << 63)), _lib.ERR_INVALID_ARG),
    (dict(group=0), _lib.ERR_INVALID_ARG),                   # what trpx_decode_sum refuses of a group
    (dict(terse=None), _lib.ERR_INVALID_ARG),                # null pointers
    (dict(hist=None), _lib.ERR_INVALID_ARG),
    (dict(status=None), _lib.ERR_INVALID_ARG),
    (dict(terse=TERSE + 2), _lib.ERR_INVALID_ARG),           # misaligned pointers
    (dict(offs=OFFS + 4), _lib.ERR_INVALID_ARG),
    (dict(index=INDEX + 8), _lib.ERR_INVALID_ARG),
    (dict(hist=HIST + 4), _lib.ERR_INVALID_ARG),
    (dict(status=STATUS + 4), _lib.ERR_INVALID_ARG),
    (dict(ws=WS + 4), _lib.ERR_INVALID_ARG),
    (dict(offs=None), _lib.ERR_INVALID_ARG),                 # an index without its offsets
    (dict(index=None, ws=None), _lib.ERR_INVALID_ARG),       # no workspace where the index is built
    (dict(offs=None, index=None, ws=None), _lib.ERR_INVALID_ARG),
    (dict(group=N_FRAMES, ws=None), _lib.ERR_INVALID_ARG),   # ... or where the spans' partial counts go
    # TRPX_ERR_CAPACITY
    (dict(ws_bytes=0, index=None), _lib.ERR_CAPACITY),       # workspace too small for the index
    (dict(ws_bytes=0, group=N_FRAMES), _lib.ERR_CAPACITY),   # ... and for the partial counts
])
def test_argument_errors_are_return_codes(kw, code):
    assert _hist(**kw) == code
    assert L().trpx_last_error_string().startswith(b"trpx_decode_hist")


@pytest.mark.parametrize("kw", [dict(n_bins=1), dict(n_bins=4096), dict(shift=0), dict(shift=32), dict(lo=1 << 32), dict(lo=-(1 << 32)),
                                dict(n_bins=4096, shift=32, lo=-(1 << 32)), dict(group=1), dict(group=3), dict(group=1 << 40)])
def test_legal_corners_pass_every_check(kw):
    # the first thing to fail is the workspace that is one byte short (the form without offsets and index needs one whatever the group)
    need = L().trpx_decode_hist_workspace_bytes(_lib.U16, TERSE_BYTES, N_VALUES, N_FRAMES, 12, kw.get("group", 1), kw.get("n_bins", N_BINS))
    assert need > 0
    assert _hist(offs=None, index=None, ws_bytes=need - 1, **kw) == _lib.ERR_CAPACITY
    assert L().trpx_last_error_string().startswith(b"trpx_decode_hist: workspace")


@pytest.mark.parametrize("n_bins", [1, 256, 4096])
@pytest.mark.parametrize("n_values, n_frames, group", [(N_VALUES, N_FRAMES, N_FRAMES), (N_VALUES, 2000, 2000), (122893, 3, 1), (122893, 5, 2)])
def test_workspace_one_byte_short(n_bins, n_values, n_frames, group):
    need = L().trpx_decode_hist_workspace_bytes(_lib.U16, TERSE_BYTES, n_values, n_frames, 12, group, n_bins)
    kw = dict(n_values=n_values, n_frames=n_frames, n_bins=n_bins, group=group)
    assert _hist(offs=None, index=None, ws_bytes=need - 1, **kw) == _lib.ERR_CAPACITY        # without offsets: the whole need
    assert L().trpx_last_error_string().startswith(b"trpx_decode_hist")
    # with offsets and index given less is needed, and the call checks against its own form's need: the partial counts
    spans = L().trpx_decode_hist_spans_per_group(n_values, n_frames, group)
    assert spans > 1
    own = 8 * n_bins * -(-n_frames // group) * spans
    assert own < need
    assert _hist(ws_bytes=own - 1, **kw) == _lib.ERR_CAPACITY
    assert L().trpx_last_error_string().startswith(b"trpx_decode_hist")


def test_host_wrapper_checks_before_the_device():
    buf = (C.c_uint8 * 64)()
    hist = (C.c_uint64 * 8)()

    def host(dtype=_lib.U16, block=12, n_values=12, group=1, lo=0, shift=0, n_bins=4, out=hist, terse=buf):
        return L().trpx_decode_hist_host(dtype, terse, 64, None, n_values, 2, block, group, lo, shift, n_bins, out, -1)

    # the argument checks come before the device is looked for: the same answers with and without a GPU
    for kw, code in [(dict(block=7), _lib.ERR_UNSUPPORTED), (dict(dtype=_lib.U64), _lib.ERR_UNSUPPORTED),
                     (dict(dtype=42), _lib.ERR_INVALID_ARG), (dict(dtype=_lib.F32), _lib.ERR_INVALID_ARG),
                     (dict(n_values=0), _lib.ERR_INVALID_ARG), (dict(out=None), _lib.ERR_INVALID_ARG), (dict(terse=None), _lib.ERR_INVALID_ARG),
                     (dict(n_bins=0), _lib.ERR_INVALID_ARG), (dict(n_bins=4097), _lib.ERR_INVALID_ARG), (dict(shift=33), _lib.ERR_INVALID_ARG),
                     (dict(lo=(1 << 32) + 1), _lib.ERR_INVALID_ARG), (dict(lo=-(1 << 32) - 1), _lib.ERR_INVALID_ARG),
                     (dict(group=0), _lib.ERR_INVALID_ARG)]:
        assert host(**kw) == code, kw
        assert L().trpx_last_error_string().startswith(b"trpx_decode_hist_host")
    if L().trpx_device_count() == 0:
        assert host() == _lib.ERR_NO_DEVICE                  # a legal call gets as far as the device


def test_bin_rule_under_the_sanitizers():
    """hist_bin.hpp -- the text the kernel runs: for both signednesses, every width 0 .. 32 and a fixed list of (lo, shift, n_bins)
    -- lo at each type's minimum and maximum and at +-2^32, shift 0 / 1 / 31 / 32, 1 / 2 / 4096 bins -- hist_block_one_bin is
    true exactly when the two ends of the width's range share a bin; for widths <= 8 every value of the range lands in the
    promised bin; the merged lane count of random blocks of 1 .. 12 values equals a plain loop; under ASan + UBSan (a stand-alone
    CPU program)."""
    exe = os.path.join(ROOT, "tests", "cpp", "hist_sanitize")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "hist_example.mk", "hist_sanitize"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK hist_sanitize" in r.stdout, r.stdout + r.stderr
