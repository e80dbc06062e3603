"""CPU tier: the checks of tests/gpu_support.py that the parity tests lean on can fail.  assert_round_trip sees one wrong byte,
another type or size and a non-zero status, and passes unsigned wide data with the top bit set; assert_same_index sees a planted group
offset and a planted width, not the padding between the two parts; run_variant skips for an absent build, fails for a child
that exits non-zero or does not print OK; selected puts 0 back when its block raises; fuzz_stack is seeded."""
import numpy as np
import pytest
import torch

from gpu_support import assert_round_trip, assert_same_index, fuzz_stack, index_layout, index_parts, run_variant, selected, to_dev

N, FRAMES = 12 * 300 + 5, 3                                  # 301 blocks, two groups of 256 a frame: 48 offset bytes, widths from 48 on


# ---- assert_round_trip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.uint16, np.uint32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("as_tensor", [True, False], ids=["tensor", "array"])
def test_round_trip_passes_unsigned_wide_data_with_the_top_bit_set(dt, as_tensor):
    px = np.arange(2 * 41, dtype=np.int64).reshape(2, 41).astype(dt) | dt(1 << (8 * np.dtype(dt).itemsize - 1))
    back = to_dev(px.reshape(-1), "cpu") if as_tensor else px.copy()
    ok = torch.zeros(8, dtype=torch.int32) if as_tensor else np.zeros(8, np.int32)
    assert_round_trip(back, ok, to_dev(px, "cpu") if as_tensor else px, "top bit")        # (tensor against tensor, array against array)
    assert_round_trip(back, ok, px, "top bit")                                           # (and either against the array)


def test_round_trip_fails_for_one_wrong_byte_in_the_last_element():
    px = np.arange(2 * 41, dtype=np.uint16).reshape(2, 41)
    ok = torch.zeros(8, dtype=torch.int32)
    for high in (False, True):
        bad = px.copy()
        bad.view(np.uint8).reshape(-1)[-1 if high else -2] ^= 1
        for back, truth in ((bad, px), (to_dev(bad, "cpu"), px), (to_dev(bad, "cpu"), to_dev(px, "cpu"))):
            with pytest.raises(AssertionError, match="pixels differ"):
                assert_round_trip(back, ok, truth, ("ctx", 7))
    with pytest.raises(AssertionError, match="type or size differ"):                       # a frame short
        assert_round_trip(px[:1], ok, px, "short")
    with pytest.raises(AssertionError, match="type or size differ"):                       # the same bytes in another type
        assert_round_trip(px.view(np.int16), ok, px, "signed")
    assert_round_trip(px.reshape(-1), ok, px, "flat")                                      # the same stack, another shape


def test_round_trip_fails_for_a_status_with_correct_pixels():
    px = np.arange(2 * 41, dtype=np.uint16).reshape(2, 41)
    st = torch.zeros(8, dtype=torch.int32)
    st[0] = 5
    with pytest.raises(AssertionError, match="status"):
        assert_round_trip(px.copy(), st, px, "corrupt")
    st[0], st[2] = 0, 3                                       # (the other status words are the caller's)
    assert_round_trip(px.copy(), st, px, "listed frames")


# ---- the decode index ------------------------------------------------------------------------------------------------------------
def _index(as_tensor):
    g, w_off, w = index_layout(N, FRAMES)
    assert (g, w_off, w) == (8 * FRAMES * 2, 48, FRAMES * 301)
    a = np.random.default_rng(5).integers(0, 256, size=w_off + w + 16, dtype=np.uint8)
    return to_dev(a, "cpu") if as_tensor else a


@pytest.mark.parametrize("as_tensor", [True, False], ids=["tensor", "array"])
def test_same_index_sees_offsets_and_widths_and_not_the_padding(as_tensor):
    n, frames = 12 * 100, 3                                   # one group a frame: 24 offset bytes, padding 24 .. 31, widths from 32
    g, w_off, w = index_layout(n, frames)
    assert (g, w_off, w) == (24, 32, 300)
    a = np.random.default_rng(6).integers(0, 256, size=w_off + w + 16, dtype=np.uint8)
    a = to_dev(a, "cpu") if as_tensor else a
    b = a.clone() if as_tensor else a.copy()
    assert_same_index(a, b, n, frames, "same")
    offsets, widths = index_parts(b, n, frames)
    assert len(offsets) == g and len(widths) == w
    for pos in range(g, w_off):                               # the padding, and what lies behind the widths: not compared
        b[pos] ^= 0xFF
    b[w_off + w] ^= 0xFF
    assert_same_index(a, b, n, frames, "padding differs")
    for pos, what in ((0, "group offsets"), (g - 1, "group offsets"), (w_off, "widths"), (w_off + w - 1, "widths")):
        b[pos] ^= 1
        with pytest.raises(AssertionError, match=what):
            assert_same_index(a, b, n, frames, ("ctx", pos))
        b[pos] ^= 1
    assert_same_index(a, b, n, frames, "restored")


def test_index_layout_of_a_stack_with_two_groups_a_frame():
    idx = _index(False)
    offsets, widths = index_parts(idx, N, FRAMES)
    assert offsets.tobytes() == idx[:48].tobytes() and widths.tobytes() == idx[48: 48 + 903].tobytes()


# ---- run_variant -----------------------------------------------------------------------------------------------------------------
def _case(tmp_path, body):
    p = tmp_path / "case.py"
    p.write_text(body)
    return str(p)


def test_run_variant_skips_for_an_absent_build_and_runs_a_present_one(tmp_path):
    case = _case(tmp_path, "import os, sys\nassert os.environ['TRPX_LIB'].endswith('libtrpx_standin.so') and sys.argv[1:] == ['all']\nprint('OK')\n")
    with pytest.raises(pytest.skip.Exception, match=r"test variant not built \(make -C trpx_amd/csrc standin\)"):
        run_variant("standin", case, "all", variants=str(tmp_path))
    (tmp_path / "libtrpx_standin.so").write_bytes(b"never loaded")
    run_variant("standin", case, "all", variants=str(tmp_path))


def test_run_variant_fails_for_a_child_that_exits_non_zero_or_prints_no_ok(tmp_path):
    (tmp_path / "libtrpx_standin.so").write_bytes(b"never loaded")
    with pytest.raises(AssertionError, match="boom"):                                      # (the tail of stderr is shown)
        run_variant("standin", _case(tmp_path, "print('OK')\nraise SystemExit('boom')\n"), variants=str(tmp_path))
    with pytest.raises(AssertionError, match="done"):
        run_variant("standin", _case(tmp_path, "print('done')\n"), variants=str(tmp_path))


# ---- selected --------------------------------------------------------------------------------------------------------------------
class _Lib:
    def __init__(self, refuse=None):
        self.calls, self.refuse = [], refuse

    def trpx_set_decode_path(self, value):
        self.calls.append(value)
        return 1 if value == self.refuse else 0


def test_selected_restores_auto_when_its_block_raises():
    lib = _Lib()
    with selected("trpx_set_decode_path", 3, lib=lib):
        assert lib.calls == [3]
    assert lib.calls == [3, 0]
    with pytest.raises(ZeroDivisionError):
        with selected("trpx_set_decode_path", 2, lib=lib):
            1 / 0
    assert lib.calls == [3, 0, 2, 0]
    refusing = _Lib(refuse=9)
    with pytest.raises(AssertionError):                        # a value the library refuses: the block does not run
        with selected("trpx_set_decode_path", 9, lib=refusing):
            refusing.calls.append("ran")
    assert refusing.calls == [9]


# ---- fuzz_stack ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(6))
def test_fuzz_stack_is_seeded_and_of_its_type(kind):
    for dt in (np.dtype(np.uint8), np.dtype(np.int32)):
        a = fuzz_stack(np.random.RandomState(11), dt, kind, 12 * 50 + 7, 3)
        b = fuzz_stack(np.random.RandomState(11), dt, kind, 12 * 50 + 7, 3)
        assert a.dtype == dt and a.shape == (3, 607) and a.tobytes() == b.tobytes()
