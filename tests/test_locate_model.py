"""CPU tier: the model of the position-parallel frame locator (tools/locate_parallel_model.py, the scheme of decode_locate.hip)
with scaled-down windows and chunks, on small oracle-encoded stacks and on streams built to defeat chain merging.  Its offsets
and status must equal the encoder's offsets, or, for hand-edited streams, those of the plain serial walk."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("locate_parallel_model", os.path.join(ROOT, "tools", "locate_parallel_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))])


def _encode(oracle, px):
    stream, sizes, _ = oracle.encode_stack(px)
    return stream, _offsets(sizes)


SCALES = [(256, 4), (512, 8), (1024, 16)]


@pytest.mark.parametrize("win_bits,win_per_chunk", SCALES)
@pytest.mark.parametrize("data", ["synth", "poisson3"])
def test_model_matches_encoder(oracle, model, data, win_bits, win_per_chunk):
    from trpx_amd import workloads
    n, frames = 96 * 96, 6
    px = oracle.synth(np.uint16, 0, frames, n) if data == "synth" else workloads.poisson_u16_np(3.0, 0, frames, n)
    stream, want = _encode(oracle, px)
    offs, st, stats = model.locate(stream, n, frames, 16, win_bits, win_per_chunk)
    assert st == 0 and np.array_equal(offs, want), stats
    assert stats["repair_free"] == 1.0, stats             # an encoder-written stack needs no repair


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint32])
def test_model_odd_sizes(oracle, model, dtype):
    rng = np.random.default_rng(4)
    bits = 8 * np.dtype(dtype).itemsize
    for n, frames in [(5, 200), (13, 120), (12 * 9 + 7, 60), (64 * 64 + 3, 5)]:
        w = rng.integers(0, bits + 1, size=(frames, (n + 11) // 12)).repeat(12, axis=1)[:, :n]
        v = (rng.integers(0, 2**62, size=(frames, n), dtype=np.int64) & ((1 << w) - 1)).astype(np.int64)
        px = (v & ((1 << bits) - 1)).astype(np.dtype(dtype).newbyteorder("=").str.replace("i", "u")).view(dtype)
        stream, want = _encode(oracle, px)
        offs, st, _ = model.locate(stream, n, frames, bits, 256, 4)
        assert st == 0 and np.array_equal(offs, want), (n, frames)


def test_model_adversarial_streams(oracle, model):
    from trpx_amd import workloads
    n, frames = 48 * 48, 12
    rng = np.random.default_rng(9)
    cases = {
        "const_w9": (rng.integers(0, 512, size=(frames, n)) | 256).astype(np.uint16),
        "periodic": np.tile((np.arange(n) % 24 * 997).astype(np.uint16), (frames, 1)),
        "alternating": np.where((np.arange(frames) % 2 == 0)[:, None], workloads.poisson_u16_np(10.0, 0, frames, n), 0).astype(np.uint16),
        "blank": np.zeros((frames, n), np.uint16),
    }
    for label, px in cases.items():
        stream, want = _encode(oracle, px)
        offs, st, stats = model.locate(stream, n, frames, 16, 256, 4)
        assert st == 0 and np.array_equal(offs, want), (label, stats)


def test_model_hostile_streams_equal_serial(oracle, model):
    from trpx_amd import workloads
    n, frames = 48 * 48, 10
    stream, offs = _encode(oracle, workloads.poisson_u16_np(3.0, 2, frames, n))
    cases = {"truncated": (stream[: offs[frames // 2] + 5], frames), "too_many": (stream, frames + 1),
             "too_few": (stream, frames - 1)}
    garbage = stream.copy()
    for k in range(1, frames):
        garbage[offs[k] - 1] |= 0xF0
    cases["garbage_pad"] = (garbage, frames)
    wide = stream.copy()                                   # a 12-bit header of width 73 on a true block start deep inside frame 3
    st, pos, w, nb = model.Stream(stream), 8 * int(offs[3]), 0, (n + 11) // 12
    for _ in range(nb // 2):
        x = st.peek(pos)
        if x & 1:
            pos += 1 + 12 * w
        else:
            w, hl = model.header(x)
            pos += hl + 12 * w
    for i, bit in enumerate([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]):
        byte, sh = divmod(pos + i, 8)
        wide[byte] = (wide[byte] & ~np.uint8(1 << sh)) | np.uint8(bit << sh)
    cases["wide"] = (wide, frames)
    rng = np.random.default_rng(12)
    for t in range(12):
        bent = stream.copy()
        k = int(rng.integers(1, frames))
        bent[offs[k] - 1] ^= np.uint8(rng.integers(1, 256))
        cases[f"bent{t}"] = (bent, frames)
    for label, (s, f) in cases.items():
        want, want_st = model.serial_locate(s, n, f, 16)
        got, st, _ = model.locate(s, n, f, 16, 256, 4)
        assert st == want_st, label
        if label == "wide":
            assert st == 5
        if want_st == 0:
            assert np.array_equal(got, want), label
