"""CPU tier: the helpers of tests/test_gpu_large_stacks.py can fail, and its cases cross what they say they cross.

The helpers run on small numpy / CPU-tensor stand-ins with the boundary as a parameter (a "crossing" at byte 2^12): the picker
finds the frames around a boundary and refuses a boundary that is not crossed; the chunk comparison rejects one changed byte
and one offset off by one behind the boundary; every torch truth equals plain numpy on the pixels and disagrees with an output
in which the frames behind the boundary were swapped or their frame number was wrapped.  The sizing arithmetic of cases A - E
is checked with the oracle's bytes per value on a few frames."""
import numpy as np
import pytest
import torch

from gpu_support import ConsumerSpec, DeviceGuarded, GUARD, assert_stream_is_chunks, consumer_truths, crossing_frames, frame_chunks, keep_from
from gpu_support import signed_view, sparse_truth, sum_truth, to_dev, to_np, wide

BOUNDARY = 1 << 12
N512 = 512 * 512


# ---- the picker ----------------------------------------------------------------------------------------------------------------
def test_picker_finds_the_frames_around_a_boundary():
    offs = np.arange(0, 31) * 300                            # 30 frames of 300 bytes: byte 4096 lies in frame 13
    at, picks = crossing_frames(offs, [BOUNDARY])
    assert at == {BOUNDARY: 13} and offs[13] <= BOUNDARY < offs[14]
    assert picks == [0, 12, 13, 14, 29]
    at, picks = crossing_frames(to_dev(offs.astype(np.int64), "cpu"), [BOUNDARY, 2 * BOUNDARY])     # a tensor; two boundaries
    assert at == {BOUNDARY: 13, 2 * BOUNDARY: 27} and picks == [0, 12, 13, 14, 26, 27, 28, 29]
    assert crossing_frames(offs, [3900])[0] == {3900: 13}    # a boundary on a frame's first byte belongs to that frame
    assert crossing_frames(offs, [0])[1] == [0, 1, 29]       # the neighbours stay inside the stack


def test_picker_refuses_a_boundary_that_is_not_crossed():
    offs = np.arange(0, 14) * 300                            # 13 frames: 3900 bytes
    for b in (BOUNDARY, 3900):                               # the end itself is not inside the stack
        with pytest.raises(AssertionError, match="not crossed"):
            crossing_frames(offs, [b])
    crossing_frames(offs, [3899])


# ---- the chunk comparison ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_stack(oracle):
    px = np.random.default_rng(5).integers(0, 256, size=(37, 301), dtype=np.uint8)
    stream, sizes, _ = oracle.encode_stack(px)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert offs[-1] > BOUNDARY + 600

    def chunk(f0, f1):
        s, z, _ = oracle.encode_stack(px[f0:f1])
        return s, np.concatenate([[0], np.cumsum(z)]).astype(np.uint64)
    return px, stream, offs, chunk


@pytest.mark.parametrize("as_tensor", [False, True])
def test_chunk_comparison_accepts_the_stack_and_rejects_one_byte_and_one_offset(small_stack, as_tensor):
    px, stream, offs, chunk = small_stack
    conv = (lambda a: to_dev(a, "cpu")) if as_tensor else (lambda a: a.copy())
    if as_tensor:
        inner = chunk
        chunk = lambda f0, f1: tuple(to_dev(x.astype(np.int64) if x.dtype == np.uint64 else x, "cpu") for x in inner(f0, f1))   # noqa: E731
    for size in (5, 256):
        assert_stream_is_chunks(conv(stream), conv(offs), 37, chunk, size)
    k = crossing_frames(offs, [BOUNDARY])[0][BOUNDARY]
    bad = stream.copy()
    bad[BOUNDARY + 300] ^= 1                                 # one bit of one byte behind the boundary
    with pytest.raises(AssertionError, match="bytes of frames"):
        assert_stream_is_chunks(conv(bad), conv(offs), 37, chunk, 5)
    shifted = offs.copy()
    shifted[k + 2:] += 1                                     # the table off by one behind the boundary
    with pytest.raises(AssertionError, match="running sums"):
        assert_stream_is_chunks(conv(stream), conv(shifted), 37, chunk, 5)
    with pytest.raises(AssertionError):                      # a stream that ends early; one with a byte too many
        assert_stream_is_chunks(conv(stream[:-1]), conv(offs), 37, chunk, 5)
    with pytest.raises(AssertionError):
        assert_stream_is_chunks(conv(np.concatenate([stream, [0]]).astype(np.uint8)), conv(offs), 37, chunk, 5)


# ---- the guarded device output ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", [torch.uint8, torch.uint16, torch.uint32, torch.int64, torch.uint64])
def test_device_guarded_passes_untouched_and_fails_for_one_byte(tdt):
    g = DeviceGuarded((3, 7), tdt, "cpu")
    assert g.view.shape == (3, 7) and g.whole.numel() == 21 + 2 * GUARD and (g.whole.view(torch.uint8) == 0xA5).all()
    g.view.view(torch.uint8).zero_()
    assert not g.check("written").view(torch.uint8).any()
    raw = g.whole.view(torch.uint8)
    size = g.whole.element_size()
    for pos in (GUARD * size - 1, (GUARD + 21) * size, 0, raw.numel() - 1):
        raw[pos] ^= 0x10
        with pytest.raises(AssertionError, match="written outside"):
            g.check("it")
        raw[pos] ^= 0x10
    g.poison()
    assert (g.view.view(torch.uint8) == 0xA5).all()


# ---- the torch truths ----------------------------------------------------------------------------------------------------------------
F, W, H = 23, 8, 6
N = W * H


def _spec(group=5, threshold=200):
    f = torch.arange(F, dtype=torch.int64)
    labels = (f * 7) % 4                                     # n_out = 3: label 3 masks the frame
    p = torch.arange(N, dtype=torch.int64)
    weights = torch.stack([torch.ones(N, dtype=torch.int64), p % W - 4, (p * 37) % 11 - 5]).to(torch.int32)
    return ConsumerSpec(group, labels, 3, weights, ((p // 5) % 4).to(torch.int16), 3, W, (4, 3), threshold)


def _pixels(dt, seed=7):
    info = np.iinfo(dt)
    return np.random.default_rng(seed).integers(0, int(info.max) + 1, size=(F, N), dtype=np.uint64).astype(dt)


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.uint32])
def test_torch_truths_are_plain_numpy_on_the_pixels(dt):
    px = _pixels(dt)
    spec = _spec(threshold=int(np.iinfo(dt).max * 0.8))
    t = {k: v.numpy() for k, v in consumer_truths(to_dev(px, "cpu"), spec, elems=3 * N).items()}      # (runs of three frames)
    p64 = px.astype(np.int64)
    groups = [p64[j:j + 5] for j in range(0, F, 5)]
    assert (t["sum"] == sum_truth(px, 5, np.int64)).all()
    assert (t["max"] == np.stack([g.max(0) for g in groups])).all()
    sq = np.stack([(g.astype(object) ** 2).sum(0) % (1 << 64) for g in groups])
    assert (t["sumsq"].view(np.uint64).astype(object) == sq).all()
    lab = spec.frame_labels.numpy()
    assert (t["labelled"] == np.stack([p64[lab == k].sum(0) for k in range(3)])).all()
    assert (t["counts"] == [(lab == k).sum() for k in range(3)]).all()
    assert (t["dot"] == p64 @ spec.weights.numpy().astype(np.int64).T).all()
    pl = spec.pixel_labels.numpy()
    assert (t["bins"] == np.stack([p64[:, pl == k].sum(1) for k in range(3)], axis=1)).all()
    img = p64.reshape(F, H, W)
    want = np.zeros((F, 2, 3), np.int64)                     # bins of 4 x 3 in frames of 6 x 8: edge bins sum what exists
    for y in range(2):
        for x in range(3):
            want[:, y, x] = img[:, 4 * y:4 * y + 4, 3 * x:3 * x + 3].sum((1, 2))
    assert (t["binned"] == want).all()
    rows, pos, val = sparse_truth(px, spec.threshold)
    assert (t["rows"] == rows).all() and (t["positions"] == pos).all() and (t["values"] == val.astype(np.int64)).all()
    assert rows[-1] > F                                      # (there are events)


@pytest.mark.parametrize("dt", [np.uint8, np.uint32])
def test_every_truth_disagrees_with_swapped_or_wrapped_frames(dt):
    """The outputs a kernel with a wrapped frame number would give: frames behind the "boundary" (frame 16 of 23) read from
    frame number modulo 16, or two frames on either side of it exchanged."""
    px = _pixels(dt)
    spec = _spec(threshold=int(np.iinfo(dt).max * 0.8))
    t = consumer_truths(to_dev(px, "cpu"), spec)
    wrapped = px[np.arange(F) % 16]
    swapped = px.copy()
    swapped[[14, 17]] = px[[17, 14]]                         # (frames of different groups, labels and rows)
    for what, wrong in (("wrapped", wrapped), ("swapped", swapped)):
        w = consumer_truths(to_dev(wrong, "cpu"), spec)
        for key in t:
            if key in ("counts", "rows", "values"):          # (frames per label: no function of the pixels; the events: below)
                continue
            assert t[key].shape != w[key].shape or not torch.equal(t[key], w[key]), (what, key)
        assert any(t[k].shape != w[k].shape or not torch.equal(t[k], w[k]) for k in ("rows", "values")), (what, "events")


def test_wide_and_keep_from_hold_the_values_of_the_unsigned_types():
    for dt in (np.uint8, np.uint16, np.uint32, np.uint64, np.int16):
        info = np.iinfo(dt)
        a = np.array([0, 1, int(info.max) // 2 + 1, int(info.max)], dtype=dt)
        w = wide(to_dev(a, "cpu"))
        assert w.dtype == torch.int64 and (w.numpy().view(np.uint64 if dt == np.uint64 else np.int64) == a).all()
        assert signed_view(to_dev(a, "cpu")).element_size() == a.itemsize
    for dt in (np.uint8, np.uint16, np.uint32):
        a = np.array([[0, 5, 6, int(np.iinfo(dt).max)]], dtype=dt)
        assert (to_np(keep_from(to_dev(a, "cpu"), 6)) == np.array([[0, 0, 6, np.iinfo(dt).max]], dtype=dt)).all()
    assert list(frame_chunks(3, 11, 10, 30)) == [(3, 6), (6, 9), (9, 11)] and list(frame_chunks(0, 2, 100, 30)) == [(0, 1), (1, 2)]


# ---- the sizing of the cases ------------------------------------------------------------------------------------------------------------
def _bytes_per_value(oracle, px):
    return oracle.encode_stack(px)[0].size / px.size


def test_case_a_crosses_stream_bit_2_32(oracle):
    from trpx_amd import workloads
    rng = np.random.default_rng(1)
    u8 = _bytes_per_value(oracle, rng.integers(0, 256, size=(2, N512), dtype=np.uint8))
    assert 1.0100 < u8 < 1.0108                              # 8 bits a value, a 1-bit header a block, a few wider ones
    assert 8 * 2100 * N512 * u8 > 1.02 * 2 ** 32
    p3 = _bytes_per_value(oracle, workloads.poisson_u16_np(3.0, 0, 2, N512))
    assert 0.40 < p3 < 0.43                                 # the header-dense flavour: 4200 frames of it fall short of bit 2^32 ...
    assert 8 * 4200 * N512 * p3 < 2 ** 32 < 8 * 5100 * N512 * p3 / 1.02      # ... so the case has 5100


def test_case_b_crosses_stream_and_pixel_byte_2_32(oracle):
    rng = np.random.default_rng(2)
    u32 = _bytes_per_value(oracle, rng.integers(0, 1 << 32, size=(2, N512), dtype=np.uint64).astype(np.uint32))
    assert 4.0100 < u32 < 4.0108
    assert 4160 * N512 * u32 > 1.01 * 2 ** 32 and 4160 * N512 * 4 > 2 ** 32 > 4095 * N512 * 4


def test_cases_c_and_d_cross_their_boundaries():
    from trpx_amd import _lib
    L = _lib.lib()
    assert 16500 * N512 > 2 ** 32 > 2 ** 31 > 8000 * N512 and 16384 * N512 == 2 ** 32
    assert 70001 > 65535
    assert L.trpx_group_count(8, 12) == 1 and L.trpx_group_count(40, 12) == 1 and L.trpx_group_count(N512, 12) == 86
    assert (2 ** 24 + 3) * 256 >= 2 ** 32 > (2 ** 24 - 1) * 256      # one workgroup of 256 threads per tile


def test_case_e_lies_on_either_side_of_the_32_bit_frame_line(oracle):
    from trpx_amd import _lib
    L = _lib.lib()
    for side, below in ((11008, True), (11100, False), (11600, False)):
        n = side * side
        worst = 8 * L.trpx_worst_case_bytes(_lib.U32, n, 12)
        assert 33 * n <= worst < 33 * n + 64                 # 32 bits a value and 12 header bits a block of 12
        assert (worst < 0xF0000000) == below and (33 * n < 0xF0000000) == below
    rng = np.random.default_rng(3)
    u32 = _bytes_per_value(oracle, rng.integers(0, 1 << 32, size=(1, 1 << 20), dtype=np.uint64).astype(np.uint32))
    assert 8 * u32 * 11600 ** 2 > 1.004 * 2 ** 32 and 3.85e9 < 8 * u32 * 11008 ** 2 < 2 ** 32
