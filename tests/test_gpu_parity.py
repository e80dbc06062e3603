"""GPU parity tests (-m gpu): the encoders and every decode route, called through the C ABI, against the CPU oracle.  (Frames
of more than 32 K blocks: tests/test_gpu_large_frames.py; the Terse class, the C++ examples, the *_host and sharded calls:
tests/test_gpu_host_surface.py.)

Bar: bit-exact streams, frame sizes and prolix_bits on encode; pixel-exact on decode, and a damaged stream or a wrong index
reported, never decoded into garbage silently.  Small cases: golden fixtures made by the real reference + seeded differential
runs against the oracle.  Full BASELINE sizes: synth-v1 anchors (FNV hashes / byte totals computed with the real reference)
and size-independent properties (encode -> decode round trip, stack == concatenation of single-frame encodes, sizes == prefix
differences).

Reached, encoders: trpx_encode / trpx_encode_indexed / trpx_encode_checked / trpx_encode_host, the single-pass encoder and its
two chains (encode_fused.hip: k_encode_fused, k_encode_fused_mis2, k_stitch), the two-pass pipeline behind
trpx_set_encode_path(1) (encode.hip), the generic kernels of any block size, the synth-v1 generator, the workspace register,
and the look-back timeout in its test build (force_timeout).
Reached, decoders: trpx_decode / trpx_decode_convert / trpx_decode_indexed / trpx_build_index / trpx_decode_host along every
route of trpx_set_decode_path -- the basic kernels (decode.hip), the position-parallel walk + tiled extraction (decode_seg.hip),
the per-frame decoder and its index writers (decode_frame.hip: k_decode_frames, k_index_frames), round 4's parts route, the
dense walk of listed frames (decode_dense.hip) in the product and in its two test builds (denseserial, densetiny)."""
import os

import numpy as np
import pytest

from gpu_support import (ALL_DTYPES, ROOT, ROUTES, assert_round_trip, assert_same_index, encode, fuzz_stack, host_decode, host_encode,
                         index_layout, index_parts, run_variant, selected, to_dev)

pytestmark = pytest.mark.gpu


def test_golden_fixtures_through_c_abi(gpu, golden):
    n_checked = 0
    for c in golden["cases"]:
        px = np.array(c["pixels"], np.dtype(c["dtype"]))
        s, offs, pb = host_encode(px.reshape(1, -1), c["block"])
        assert s.tobytes().hex() == c["stream"], c["name"]
        assert pb == c["prolix_bits"], c["name"]
        assert int(offs[1]) == len(c["stream"]) // 2
        want = np.frombuffer(bytes.fromhex(c["stream"]), np.uint8)
        assert (host_decode(want, None, px.size, 1, px.dtype, c["block"])[0] == px).all(), c["name"]
        n_checked += 1
    assert n_checked >= 36 and any(c["block"] != 12 for c in golden["cases"])


def test_golden_stack_layout(gpu, golden):
    st = golden["stack"]
    px = np.array(st["pixels"], np.uint16)
    s, offs, pb = host_encode(px)
    assert s.tobytes().hex() == st["stream"]
    assert [int(x) for x in np.diff(offs)] == st["frame_sizes"]
    # decode with the offsets, and without (serial walk, the .trpx file case)
    assert (host_decode(s, offs, px.shape[1], 3, np.uint16) == px).all()
    assert (host_decode(s, None, px.shape[1], 3, np.uint16) == px).all()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_differential_vs_oracle_all_dtypes(gpu, oracle, dtype):
    rng = np.random.RandomState(11)
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    top = bits - 1 if dt.kind == "i" else bits            # full width incl. cases outside the reference's D3 domain
    for n in (1, 5, 12, 13, 255 * 12, 256 * 12, 256 * 12 + 1, 3073, 7000, 12289):
        for frames in (1, 3):
            for hi in (0, 2, 7, min(top, 10), top):
                mag = rng.randint(0, 1 << hi, size=(frames, n), dtype=np.int64) if hi else np.zeros((frames, n), np.int64)
                if dt.kind == "i":
                    mag = mag * rng.choice([-1, 1], size=(frames, n))
                px = mag.astype(dt)
                if hi and rng.rand() < 0.5:                # blocks of zeros / runs of equal widths
                    px[:, : n // 2] = 0
                want, sizes, pb = oracle.encode_stack(px)
                got, offs, gpb = host_encode(px)
                assert got.size == want.size and (np.diff(offs).astype(np.uint64) == sizes).all(), (dtype, n, frames, hi)
                assert (got == want).all(), (dtype, n, frames, hi)
                assert gpb == pb
                assert (host_decode(want, offs, n, frames, dt) == px).all(), (dtype, n, frames, hi)


def test_type_extremes_round_trip(gpu, oracle):
    # outside the reference's validity domain (D3): oracle == GPU == mathematically consistent extension
    # (42 values: a partial last block of 6; 48 and 4800: whole blocks -- -INT32_MIN once overflowed in the single-pass encoder's
    #  width computation and came out as a 33-bit block, which the 42-value case never saw while sizes that are no multiples
    #  of 4 still took the two-pass pipeline)
    for dt in (np.int16, np.int32, np.int8):
        info = np.iinfo(dt)
        for reps in (7, 8, 800):
            px = np.array([info.min, info.max, -1, 0, 1, info.min + 1] * reps, dt).reshape(1, -1)
            want, sizes, pb = oracle.encode_stack(px)
            got, offs, gpb = host_encode(px)
            assert (got == want).all() and gpb == pb == info.bits, (dt, reps)
            assert (host_decode(got, offs, px.shape[1], 1, dt) == px).all(), (dt, reps)
    px = np.array([0xFFFFFFFF, 0x80000000, 1, 0] * 5, np.uint32).reshape(1, -1)
    got, offs, gpb = host_encode(px)
    assert gpb == 32 and (got == oracle.encode_stack(px)[0]).all()
    assert (host_decode(got, offs, px.shape[1], 1, np.uint32) == px).all()


def test_frame_sizes_that_are_no_multiples_of_four(gpu, oracle):
    # n % 4 != 0 -> frames start at any element; since round 3 they run on the tuned kernels too (the route matrix forces the others)
    rng = np.random.RandomState(3)
    for n in (13, 4097, 10001):
        px = rng.poisson(5, size=(4, n)).astype(np.uint16)
        want, sizes, pb = oracle.encode_stack(px)
        got, offs, _ = host_encode(px)
        assert (got == want).all()
        assert (host_decode(got, offs, n, 4, np.uint16) == px).all()
        assert (host_decode(got, None, n, 4, np.uint16) == px).all()


def test_synth_generator_matches_oracle(gpu, oracle):
    from trpx_amd import codec
    for dt, n in ((np.uint16, 512 * 512), (np.int32, 300 * 300)):
        dev = codec.synth(dt, 5, 3, n, device=gpu).cpu().numpy()
        assert (dev == oracle.synth(dt, 5, 3, n)).all()


def _synth_anchors():
    import json
    return json.load(open(os.path.join(ROOT, "tests", "golden", "synth_anchors.json")))["anchors"]


def test_synth_anchors_u16_512(gpu, golden):
    """configs[1]/[2] data: GPU stream of frames 0..2 hashes to what the REAL reference produced."""
    import torch
    from trpx_amd import codec
    from oracle import oracle as O
    n = 512 * 512
    px = codec.synth(np.uint16, 0, 16, n, device=gpu)
    enc = encode(px, index=False)
    offs = enc.frame_offsets.cpu().numpy()
    data = enc.stack().cpu().numpy()
    assert int(offs[-1]) == golden["synth_u16_first16_total_bytes"]
    assert enc.prolix_bits() == 12
    for a in golden["anchors"]:
        if a["dtype"] != "uint16":
            continue
        f = a["frame"]
        s = data[offs[f]:offs[f + 1]]
        assert s.size == a["size"]
        assert f"{O.fnv1a64(s):016x}" == a["stream_fnv"]
        assert s[:16].tobytes().hex() == a["first16"]
    back, status = codec.decode(enc.stack(), enc.frame_offsets, n, 16, np.uint16)
    torch.cuda.synchronize()
    assert_round_trip(back, status, px, "u16 512 x 512")


def test_synth_anchor_i32_4096(gpu, golden):
    """configs[3]: 4096x4096 int32 with sparse peaks (wide bit-width / 12-bit header path)."""
    import torch
    from trpx_amd import codec
    from oracle import oracle as O
    a = [x for x in golden["anchors"] if x["dtype"] == "int32"][0]
    n = a["n"]
    # ... and frames 1 .. 7 -- the eight frames bench.py times -- from tests/golden/synth_anchors.json (the real reference again:
    # tests/golden/make_anchors.py)
    more = [x for x in _synth_anchors() if x["dtype"] == "int32"]
    assert [x["frame"] for x in more] == list(range(1, 8))
    px = codec.synth(np.int32, 0, 8, n, device=gpu)
    enc = encode(px, index=False)
    offs = enc.frame_offsets.cpu().numpy()
    for x in [a] + more:
        f = x["frame"]
        s = enc.data[offs[f]: offs[f + 1]].cpu().numpy()
        assert s.size == x["size"] and enc.prolix_bits() == x["prolix_bits"], f
        assert f"{O.fnv1a64(s):016x}" == x["stream_fnv"] and s[:16].tobytes().hex() == x["first16"], f
    back, status = codec.decode(enc.stack(), enc.frame_offsets, n, 8, np.int32)
    torch.cuda.synchronize()
    assert_round_trip(back, status, px, "i32 4096 x 4096")


def test_full_stack_2000_frames_properties(gpu):
    """configs[1]+[2] at full size: total bytes == the reference's 203 596 114, round trip exact,
    every frame of the stack == its own single-frame encode (checked on a sample)."""
    import torch
    from trpx_amd import codec
    n, frames = 512 * 512, 2000
    px = codec.synth(np.uint16, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    assert enc.total_bytes() == 203596114          # SURVEY.md section 8 row d, computed with the real reference
    assert enc.prolix_bits() == 12
    offs = enc.frame_offsets
    assert int(offs[0].item()) == 0 and bool((offs[1:] > offs[:-1]).all())
    back, status = codec.decode(enc.stack(), offs, n, frames, np.uint16)
    torch.cuda.synchronize()
    assert_round_trip(back, status, px, "2000 frames")
    for f in (0, 1, 999, 1999):
        single = codec.encode(px[f:f + 1])
        torch.cuda.synchronize()
        a, b = int(offs[f].item()), int(offs[f + 1].item())
        assert single.total_bytes() == b - a
        assert torch.equal(single.stack(), enc.data[a:b])
    # frames 1000 and 1999 against what the REAL reference made of them (tests/golden/synth_anchors.json)
    from oracle import oracle as O
    for x in [x for x in _synth_anchors() if x["dtype"] == "uint16"]:
        f = x["frame"]
        a, b = int(offs[f].item()), int(offs[f + 1].item())
        s = enc.data[a:b].cpu().numpy()
        assert s.size == x["size"] and f"{O.fnv1a64(s):016x}" == x["stream_fnv"] and s[:16].tobytes().hex() == x["first16"], f
        assert f"{O.fnv1a64(px[f].cpu().numpy()):016x}" == x["pixels_fnv"], f


def test_capacity_error_and_sizes_only_query(gpu):
    import torch
    from trpx_amd import codec, _lib
    px = codec.synth(np.uint16, 0, 4, 512 * 512, device=gpu)
    full = codec.encode(px)
    torch.cuda.synchronize()
    for path in (0, 1):                                    # single-pass and two-pass encoders
        with selected("trpx_set_encode_path", path):
            big = torch.full((1 << 20,), 7, dtype=torch.uint8, device=gpu)
            enc = codec.encode(px, out=big[:150000])        # room for one frame, not for four
            torch.cuda.synchronize()
            assert int(enc.status[0].item()) == _lib.ERR_CAPACITY
            assert bool((big[150000:] == 7).all()), "nothing beyond out_capacity may ever be touched"
            assert torch.equal(full.frame_offsets, enc.frame_offsets), "sizes must still be reported"


def test_single_pass_and_two_pass_encoders_agree(gpu):
    import torch
    from trpx_amd import codec
    for dt, n, frames in ((np.uint16, 512 * 512, 24), (np.int32, 1000 * 1000, 3), (np.uint16, 12 * 1024 * 5 + 8, 7)):
        px = codec.synth(dt, 3, frames, n, device=gpu)
        a = codec.encode(px)
        with selected("trpx_set_encode_path", 1):
            b = codec.encode(px)
        torch.cuda.synchronize()
        a.check(); b.check()
        assert torch.equal(a.frame_offsets, b.frame_offsets)
        assert a.prolix_bits() == b.prolix_bits()
        assert torch.equal(a.stack(), b.stack())


def test_corrupt_and_truncated_streams_are_detected(gpu, oracle):
    from trpx_amd import _lib, TrpxError
    rng = np.random.RandomState(5)
    px = rng.poisson(4, size=(2, 5000)).astype(np.uint16)
    s, offs, _ = host_encode(px)
    with pytest.raises(TrpxError) as e:                    # truncated
        host_decode(s[: s.size - 40], None, 5000, 2, np.uint16)
    assert e.value.code == _lib.ERR_CORRUPT
    bad_offs = offs.copy()
    bad_offs[1] -= 3                                       # frame boundary in the wrong place
    with pytest.raises(TrpxError):
        host_decode(s, bad_offs, 5000, 2, np.uint16)


def test_decode_index_side_channel(gpu, oracle):
    """the encoder's decode index == the index the header walk builds from the stream, and
    walk-free decode with it is pixel-identical (u16 1024-block tiles, int32 512-block tiles, ragged frame end,
    both encoder paths)."""
    import torch
    from trpx_amd import codec, _lib
    # (frames of more than 32 K blocks: trpx_build_index takes the index route's one walk of many short parts, decode_part.hip)
    for dt, n, frames in ((np.uint16, 512 * 512, 9), (np.int32, 700 * 700, 3), (np.uint16, 12 * 1024 * 3 + 16, 5),
                          (np.int32, 1030 * 1065, 4), (np.uint16, 1500 * 1500 + 7, 3)):
        px = codec.synth(dt, 11, frames, n, device=gpu)
        for path in (0, 1):
            with selected("trpx_set_encode_path", path):
                enc = codec.encode(px, index=True)
            torch.cuda.synchronize()
            enc.check()                                      # (behind the block: a re-run after a timeout takes the auto path)
            walked =codec.build_index(enc.stack(), enc.frame_offsets, n, frames, dt)
            torch.cuda.synchronize()
            # the index buffers are only defined where a block / group exists: compare through a decode and bytewise
            assert_same_index(enc.index, walked, n, frames, (dt, n, path))
            back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt, index=enc.index)
            torch.cuda.synchronize()
            assert_round_trip(back, st, px, (dt, n, path))
    # a wrong index is rejected, not decoded into garbage silently: by the tiled kernel (route 2) and by the per-frame
    # decoder with the widths given (route 3; a wrong group offset, a width that is not the stream's, a width wider than the type)
    px = codec.synth(np.uint16, 0, 2, 512 * 512, device=gpu)
    enc = codec.encode(px, index=True)
    nb = (512 * 512 + 11) // 12
    _, w_off, _ = index_layout(512 * 512, 2)
    for route in (2, 3):
        with selected("trpx_set_decode_path", route):
            spoils = [("offset", slice(0, 8), 255)] if route == 2 else \
                     [("offset", slice(8, 9), 1), ("width", slice(w_off + 5000, w_off + 5001), 1), ("wide", slice(w_off + nb + 77, w_off + nb + 78), 17)]
            for what, where, val in spoils:
                bad = enc.index.clone()
                bad[where] = (bad[where] + val) if what != "wide" else val
                back, st = codec.decode(enc.stack(), enc.frame_offsets, 512 * 512, 2, np.uint16, index=bad)
                torch.cuda.synchronize()
                assert int(st[0].item()) == _lib.ERR_CORRUPT, (route, what)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_many_small_frames_take_the_per_frame_decoder(gpu, oracle, dtype):
    """Stacks of small frames select k_decode_frames at any frame count (walker wave + extraction waves per workgroup): differential test
    against the oracle for every pixel type, mixed widths, partial last blocks, tiny and multi-super-step frames."""
    rng = np.random.RandomState(23)
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    top = bits - 1 if dt.kind == "i" else bits
    for n, frames in ((1, 130), (11, 130), (388, 150), (12 * 768 + 4, 140), (9216 * 3 + 8, 129)):
        hi = rng.randint(0, top + 1, size=(frames, (n + 11) // 12))            # a width for every block
        hi[rng.rand(*hi.shape) < 0.6] = 3 if top >= 3 else 1                    # long runs of one width + outliers
        mag = np.zeros((frames, n), np.int64)
        for k in range(12):
            cols = np.arange(k, n, 12)
            h = hi[:, : cols.size]
            mag[:, cols] = (rng.rand(frames, cols.size) * (2.0 ** h)).astype(np.int64)
        if dt.kind == "i":
            mag = mag * rng.choice([-1, 1], size=mag.shape)
            mag = np.clip(mag, np.iinfo(dt).min, np.iinfo(dt).max)
        px = mag.astype(dt)
        want, sizes, pb = oracle.encode_stack(px)
        got, offs, gpb = host_encode(px)
        assert got.size == want.size and (got == want).all() and gpb == pb, (dtype, n)
        assert (np.diff(offs).astype(np.uint64) == sizes).all()
        assert (host_decode(want, offs, n, frames, dt) == px).all(), (dtype, n)
    # a corrupt stack is reported, not decoded
    from trpx_amd import _lib, TrpxError
    bad = want.copy()
    bad[int(offs[5]) : int(offs[5]) + 6] ^= 0xFF
    try:
        out = host_decode(bad, offs, n, frames, dt)
        assert not (out == px).all()          # (flipping payload bits may still parse: then pixels differ)
    except TrpxError as e:
        assert e.code == _lib.ERR_CORRUPT


@pytest.mark.parametrize("block", [1, 3, 7, 16, 100, 4096])
def test_any_block_size_generic_kernels(gpu, oracle, block):
    """The `block` argument of Terse(Iterator, size, block) (Terse.hpp:263-270): every size other than the tuned
    default 12 goes through the generic kernels; differential test against the oracle."""
    rng = np.random.RandomState(block)
    for dt in (np.uint8, np.int16, np.uint16, np.int32):
        info = np.iinfo(dt)
        for n, frames in ((1, 2), (block, 1), (block * 3 + 1, 3), (5000, 2), (70001, 2)):
            hi = rng.randint(0, info.bits - (1 if dt().dtype.kind == "i" else 0) + 1)
            mag = (rng.rand(frames, n) * (2.0 ** hi)).astype(np.int64)
            mag[:, : n // 3] = 0
            if np.dtype(dt).kind == "i":
                mag = np.clip(mag * rng.choice([-1, 1], size=mag.shape), info.min, info.max)
            px = mag.astype(dt)
            parts = [oracle.encode(px[f], block) for f in range(frames)]
            want = np.concatenate([p[0] for p in parts])
            got, offs, gpb = host_encode(px, block)
            assert got.size == want.size and (got == want).all(), (block, dt, n)
            assert gpb == max(p[1] for p in parts)
            assert [int(x) for x in np.diff(offs)] == [p[0].size for p in parts]
            assert (host_decode(want, offs, n, frames, dt, block) == px).all(), (block, dt, n)
            assert (host_decode(want, None, n, frames, dt, block) == px).all(), (block, dt, n)


def test_converting_decode_cross_type_and_float(gpu, oracle):
    """Rows a9 (clamping into narrower types, Bit_pointer.hpp:747-763) and a10 (float / double output,
    Terse.hpp:379-383): trpx_decode_convert against the oracle's value semantics."""
    rng = np.random.RandomState(41)
    for src in (np.uint16, np.int16, np.int32, np.uint32):
        s_signed = np.dtype(src).kind == "i"
        info = np.iinfo(src)
        n, frames = 5003, 3
        mag = (rng.rand(frames, n) * (2.0 ** rng.randint(1, info.bits - (1 if s_signed else 0), size=(frames, 1)))).astype(np.int64)
        mag[:, ::7] = 0
        if s_signed:
            mag = np.clip(mag * rng.choice([-1, 1], size=mag.shape), info.min, info.max)
        px = mag.astype(src)
        stream, sizes, pb = oracle.encode_stack(px)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        for dst in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64):
            if s_signed and np.dtype(dst).kind == "u":
                continue                                   # the reference asserts against it (Terse.hpp:356-357)
            got = host_decode(stream, offs, n, frames, dst, stream_signed=s_signed)
            if np.dtype(dst).kind == "f":
                want = px.astype(dst)                      # exact: |v| < 2^32 fits double; float32 rounds like a cast
            else:
                di = np.iinfo(dst)
                want = np.clip(px.astype(np.int64), di.min, di.max).astype(dst)
            # the oracle's own decode path into the same output type (float / double: Terse.hpp:379-383)
            chk = np.stack([oracle.decode(stream[int(offs[f]):int(offs[f + 1])], n, dst, stream_signed=s_signed) for f in range(frames)])
            assert (chk == want).all(), (src, dst)
            assert (got == chk).all(), (src, dst)
    # the class surface: decode a u16 object into int32 / float64 containers
    from trpx_amd import Terse
    px = rng.randint(0, 60000, size=4000).astype(np.uint16)
    t = Terse(px)
    assert (t.prolix(np.empty(4000, np.int32)) == px.astype(np.int32)).all()
    assert (t.prolix(np.empty(4000, np.float64)) == px.astype(np.float64)).all()
    assert (t.prolix(np.empty(4000, np.uint8)) == np.minimum(px, 255).astype(np.uint8)).all()


@pytest.mark.parametrize("dtype", [np.uint16, np.int32, np.uint8])
def test_encoder_chains_across_many_tiles_and_frames(gpu, oracle, dtype):
    """Stresses the single-pass encoder's two chains (encode_fused.hip): one-tile frames in their hundreds (the frame
    chain beyond one 64-frame look-back window, first tile == last tile), frames of a few tiles with a partial last
    tile, and frames of more than 64 tiles (tile look-back beyond one window); widths vary from block to block so
    that tile boundaries fall on arbitrary bits.  Vector-aligned sizes only (n % 4 == 0) -- the fused path."""
    rng = np.random.RandomState(7)
    dt = np.dtype(dtype)
    tile_values = (1024 if dt.itemsize <= 2 else 768) * 12
    top = 8 * dt.itemsize - (1 if dt.kind == "i" else 0)
    for frames, n in ((700, 1000), (200, 4), (130, 2 * tile_values + 40), (3, 70 * tile_values + 8), (67, tile_values)):
        # per-block magnitude: mostly narrow, some wide, so that widths change almost every block
        nblk = (n + 11) // 12
        hi = rng.choice([0, 1, 2, 3, 5, min(9, top), top], size=(frames, nblk), p=[0.1, 0.2, 0.3, 0.2, 0.1, 0.07, 0.03])
        mag = (rng.rand(frames, nblk * 12) * (2.0 ** np.repeat(hi, 12, axis=1))).astype(np.int64)[:, :n]
        if dt.kind == "i":
            mag = np.clip(mag * rng.choice([-1, 1], size=mag.shape), np.iinfo(dt).min, np.iinfo(dt).max)
        px = mag.astype(dt)
        want, sizes, pb = oracle.encode_stack(px)
        got, offs, gpb = host_encode(px)
        assert (np.diff(offs).astype(np.uint64) == sizes).all(), (dtype, frames, n)
        assert got.size == want.size and (got == want).all(), (dtype, frames, n)
        assert gpb == pb
        assert (host_decode(got, offs, n, frames, dt) == px).all(), (dtype, frames, n)
        assert (host_decode(got, None, n, frames, dt) == px).all(), (dtype, frames, n)   # frames located by the device walk


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_two_pass_pipeline_and_basic_decoder_all_dtypes(gpu, oracle, dtype):
    """The fallback pipelines (two-pass encode: encode.hip; basic walk + unpack: decode.hip) against the oracle for every
    pixel type, with widths that change from block to block, three times over (a byte-packing code path of the basic
    8-bit unpack kernel once gave run-to-run different pixels)."""
    import torch
    from trpx_amd import codec
    rng = np.random.RandomState(5)
    dt = np.dtype(dtype)
    top = 8 * dt.itemsize - (1 if dt.kind == "i" else 0)
    frames, n = 150, 1000
    nblk = (n + 11) // 12
    hi = rng.choice([0, 1, 2, 3, 5, min(9, top), top], size=(frames, nblk), p=[0.1, 0.2, 0.3, 0.2, 0.1, 0.07, 0.03])
    mag = (rng.rand(frames, nblk * 12) * (2.0 ** np.repeat(hi, 12, axis=1))).astype(np.int64)[:, :n]
    if dt.kind == "i":
        mag = np.clip(mag * rng.choice([-1, 1], size=mag.shape), np.iinfo(dt).min, np.iinfo(dt).max)
    px = mag.astype(dt)
    want, sizes, pb = oracle.encode_stack(px)
    with selected("trpx_set_encode_path", 1):
        enc = codec.encode(to_dev(px))
        torch.cuda.synchronize()
    enc.check()                                              # (behind the block: a re-run after a timeout takes the auto path)
    assert enc.stack().cpu().numpy().tobytes() == want.tobytes()
    assert enc.prolix_bits() == pb
    for _ in range(3):
        back, st = codec.decode(enc.stack(), None, n, frames, dt)        # no offsets: serial walk + basic unpack
        torch.cuda.synchronize()
        assert_round_trip(back, st, px, dtype)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_every_decode_path_every_dtype_block_to_block_width_changes(gpu, oracle, dtype):
    """One noisy stack per pixel type (the width changes with almost every block, including the type's full width),
    encoded by the single-pass encoder with the decode index, then decoded along every route the library has:
    per-frame decoder (auto), tiled decoder (forced), walk-free indexed decoder, serial walk without offsets."""
    import torch
    from trpx_amd import codec
    rng = np.random.RandomState(99)
    dt = np.dtype(dtype)
    top = 8 * dt.itemsize - (1 if dt.kind == "i" else 0)
    for frames, n in ((140, 3000), (6, 40000)):
        nblk = (n + 11) // 12
        hi = rng.choice([0, 1, 2, 3, 5, min(9, top), top], size=(frames, nblk), p=[0.1, 0.2, 0.3, 0.2, 0.1, 0.07, 0.03])
        mag = (rng.rand(frames, nblk * 12) * (2.0 ** np.repeat(hi, 12, axis=1))).astype(np.int64)[:, :n]
        if dt.kind == "i":
            mag = np.clip(mag * rng.choice([-1, 1], size=mag.shape), np.iinfo(dt).min, np.iinfo(dt).max)
        px = mag.astype(dt)
        want, sizes, pb = oracle.encode_stack(px)
        enc = encode(px)
        assert enc.stack().cpu().numpy().tobytes() == want.tobytes(), (dtype, frames)
        for kind in ("offsets", "index", "walk"):
            back, st = codec.decode(enc.stack(), None if kind == "walk" else enc.frame_offsets, n, frames, dt,
                                    index=enc.index if kind == "index" else None)
            torch.cuda.synchronize()
            assert_round_trip(back, st, px, (dtype, frames, kind))


def test_more_frames_than_one_grid_slice(gpu, oracle):
    """The single-pass encoder's grid is (tiles per frame, frames in slices of 32768): 40 000 tiny frames cross into
    the second slice (and give the frame chain ~600 look-back windows)."""
    rng = np.random.RandomState(17)
    frames, n = 40000, 48
    px = (rng.rand(frames, n) * (2.0 ** rng.randint(0, 12, size=(frames, 1)))).astype(np.uint16)
    want, sizes, pb = oracle.encode_stack(px)
    got, offs, gpb = host_encode(px)
    assert (np.diff(offs).astype(np.uint64) == sizes).all()
    assert got.size == want.size and (got == want).all() and gpb == pb
    assert (host_decode(got, offs, n, frames, np.uint16) == px).all()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_width_changes_every_block_position_parallel_walk(gpu, oracle, dtype):
    """Streams with an explicit header on EVERY block (no two neighbouring blocks share a width; Terse.hpp:360-372 makes
    the header chain one dependent step per block) for all six pixel types, against the oracle:
    a 130-frame stack (per-frame decoder -> its walker defers such frames to the position-parallel walk, decode_seg.hip:
    one wavefront per frame, several LDS windows per segment) and three large frames (tiled decoder: several wavefronts
    per frame, links between them closed by k_seg_resolve).  Also the walk's product itself -- width[b] of every block --
    against oracle.widths(), for the encoder's index and for the index rebuilt from the stream."""
    import torch
    from trpx_amd import codec
    rng = np.random.RandomState(7)
    dt = np.dtype(dtype)
    top = 8 * dt.itemsize - (1 if dt.kind == "i" else 0)
    choices = np.array([1, 2, 3, 4, 6, min(8, top), top])
    for frames, n in ((130, 256 * 512), (3, 1024 * 1024 + 4)):
        nblk = (n + 11) // 12
        step = rng.randint(1, len(choices), size=(frames, nblk))             # never 0: the next block's width differs
        hi = choices[np.cumsum(step, axis=1) % len(choices)]
        mag = (rng.rand(frames, nblk * 12) * (2.0 ** np.repeat(hi, 12, axis=1))).astype(np.int64)
        mag[:, ::12] = (2 ** np.minimum(hi, 62) - 1)                          # the block's width is exactly hi (signed: + 1)
        mag = mag[:, :n]
        if dt.kind == "i":
            mag = np.minimum(mag, 2 ** (top - 1) - 1) * rng.choice([-1, 1], size=mag.shape)
        px = mag.astype(dt)
        want, sizes, pb = oracle.encode_stack(px)
        enc = encode(px)
        assert enc.stack().cpu().numpy().tobytes() == want.tobytes(), (dtype, frames)
        back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt)
        torch.cuda.synchronize()
        assert_round_trip(back, st, px, (dtype, frames))
        walked = codec.build_index(enc.stack(), enc.frame_offsets, n, frames, dt)
        torch.cuda.synchronize()
        want_w = np.stack([oracle.widths(px[f]) for f in range(frames)]).astype(np.uint8)
        for name, idx in (("encoder", enc.index), ("walk", walked)):
            got_w = index_parts(idx, n, frames)[1].cpu().numpy().reshape(frames, nblk)
            assert (got_w == want_w).all(), (dtype, frames, name)


def test_lookback_timeout_falls_back_to_two_pass(gpu, oracle):
    """A look-back wait of the single-pass encoder that gives up (TRPX_ERR_TIMEOUT) must not cost the caller the stack:
    in a test build of the library whose waits give up at once (make force_timeout: -DTRPX_FORCE_TIMEOUT) the plain
    stream-ordered call reports status 7, and trpx_encode_checked / Encoded.check() / trpx_encode_host end with status 0
    and the oracle's bytes (re-run through the two-pass pipeline)."""
    run_variant("force_timeout", "lookback_timeout.py")


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_build_index_of_many_small_frames(gpu, oracle, dtype):
    """trpx_build_index on a stack of frames of < 2^26 bits runs the per-frame walker with index writers in place of the extraction
    (k_index_frames; header-dense frames go to the position-parallel walk): the index must equal the one the encoder writes as a
    by-product, block for block and group for group, and decode the stack (Terse.hpp:360-372 has one chain per frame)."""
    import torch
    from trpx_amd import codec
    dt = np.dtype(dtype)
    rng = np.random.RandomState(4242 + ALL_DTYPES.index(dtype))
    for kind, n, frames in ((2, 40000, 130), (3, 12 * 1024 + 8, 140), (1, 3000, 200), (5, 50000, 131), (0, 52, 129),
                            (3, 12 * 34000, 4), (2, 12 * 34000 + 4, 3),           # (> 32 K blocks: dense frames go through several wavefronts each)
                            (2, 513 * 7, 131), (3, 1030 * 53 + 1, 3)):            # (no multiples of 4)
        px = fuzz_stack(rng, dt, kind, n, frames)
        enc = encode(px)
        walked = codec.build_index(enc.stack(), enc.frame_offsets, n, frames, dt)
        torch.cuda.synchronize()
        assert_same_index(enc.index, walked, n, frames, (dtype, kind, n, frames))
        back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt, index=walked)
        torch.cuda.synchronize()
        assert_round_trip(back, st, px, (dtype, kind, n, frames))


@pytest.mark.parametrize("route", ["auto", "tiles", "frames", "parts", "dense", "basic"])
def test_fuzz_slice_every_route(gpu, oracle, route):
    """A bounded, seeded slice of tools/fuzz_paths.py inside the tier the driver runs: random pixel types, frame sizes (small,
    512 x 512, detector sizes beyond 32 K blocks), frame counts and width patterns (runs, flips, pedestals, Poisson counts, type
    extremes), encoded by the GPU (== the oracle's bytes), decoded along the forced route (== the pixels), the decode index
    three ways.  The slice is the first _FUZZ_SLICE cases of the seed's sequence that stay within max_pixels: the same cases on
    every machine (the time budget is a safety cap far above what they take, 6 - 10 s per route); the long runs stay with the
    tool (profiles/rNN_fuzz.txt).  Then valid streams no encoder writes -- restated widths, tests/noncanonical.py K1 and K3 --
    along the same route: exact or refused, as tests/noncanonical_dev.py pins it."""
    import importlib.util
    import noncanonical as nc
    import noncanonical_dev as nd
    spec = importlib.util.spec_from_file_location("fuzz_paths", os.path.join(ROOT, "tools", "fuzz_paths.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    code = {"auto": 0, **ROUTES}[route]
    with selected("trpx_set_decode_path", code):
        n_run, n_large, n_fb = fz.run(60, seed=600 + code, basic=route == "basic", budget_s=300.0, quiet=True, max_run=_FUZZ_SLICE,
                                      max_pixels=1 << (21 if route in ("basic", "frames") else 23))
        for kind in ("K1", "K3"):
            for dt, shape in ((np.uint16, (3, 7000)), (np.int32, (4, 1073))):
                v = nd.Dev(nc.make(dt, shape, kind)).decode("offsets")
                assert v in (nd.EXACT, nd.REFUSED) and v == nd.pinned(f"decode|offsets|{code}", kind, shape, dt), (route, kind, dt, shape, v)
    assert n_run == _FUZZ_SLICE, n_run


_FUZZ_SLICE = 10     # cases per route (>= 8); every route's seed has more than that within its max_pixels among its 60


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_decode_route_matrix(gpu, oracle, route, dtype):
    """Each decode route forced through trpx_set_decode_path (the basic kernels, the position-parallel walk + tiled
    extraction, the per-frame decoder for any number of frames) must give the oracle's pixels for every pixel type:
    Terse.hpp:352-389 has one answer whatever the route."""
    import torch
    from trpx_amd import codec, _lib
    L = _lib.lib()
    dt = np.dtype(dtype)
    rng = np.random.RandomState(1000 * ROUTES[route] + ALL_DTYPES.index(dtype))
    cases = [(0, 4096, 3), (1, 12 * 768 + 4, 17), (2, 40000, 130), (3, 3000, 140), (4, 131072, 3), (2, 388, 129), (1, 52, 2),
             (5, 50000, 131), (5, 262144, 4), (2, 12 * 40000 + 8, 3),      # (> 32 K blocks: several wavefronts per frame on the tiled route,
             (3, 12 * 34000, 5),                                            #  and the per-frame decoder's hand-over of dense frames through them)
             (2, 12 * 300 + 7, 130), (1, 2463 * 3, 4), (3, 1030 * 53 + 1, 3), (2, 12 * 34000 + 3, 3)]   # pixel counts that are no multiples of 4:
    #                                                                            frames start at any element (1030 x 1065, 2463 x 2527 detectors)
    assert L.trpx_set_decode_path(9) != 0                                    # out of range: refused
    with selected("trpx_set_decode_path", ROUTES[route]):
        for kind, n, frames in cases:
            px = fuzz_stack(rng, dt, kind, n, frames)
            want, sizes, pb = oracle.encode_stack(px)
            enc = encode(px)
            assert enc.stack().cpu().numpy().tobytes() == want.tobytes() and enc.prolix_bits() == pb, ("encode", route, dtype, kind, n, frames)
            back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt)
            torch.cuda.synchronize()
            assert_round_trip(back, st, px, (route, dtype, kind, n, frames))
            if enc.index is not None and route != "basic":       # walk-free: tiled kernel / per-frame decoder with the widths given
                back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt, index=enc.index)
                torch.cuda.synchronize()
                assert_round_trip(back, st, px, ("index", route, dtype, kind, n, frames))


@pytest.mark.parametrize("dtype,frames", [(np.uint16, 3000), (np.int32, 1537), (np.uint8, 4100)])
def test_stacks_larger_than_one_round_of_workgroups(gpu, oracle, dtype, frames):
    """The per-frame decoder runs one workgroup per frame, 2048 resident at a time for 8/16-bit pixels, 1536 for 32-bit:
    stacks past one round (prolix.cpp:69-92 loops over any number of frames).  Full size, so checked through properties:
    sizes == prefix differences, round trip pixel-identical, and a sample of frames -- the first, the last and the ones
    around the round's edge -- byte-identical to the oracle's single-frame encodes."""
    import torch
    from trpx_amd import codec
    n = 512 * 512
    dt = np.dtype(dtype)
    if dtype == np.uint8:                                                    # synth-v1 exists for u16 / i32: fold the u16 frames into bytes
        px = (codec.synth(np.uint16, 0, frames, n, device=gpu).view(torch.int16) & 0xFF).to(torch.uint8)
    else:
        px = codec.synth(dtype, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    offs = enc.frame_offsets.cpu().numpy()
    assert offs[0] == 0 and (np.diff(offs.astype(np.int64)) > 0).all() and int(offs[-1]) == enc.total_bytes()
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt)
    torch.cuda.synchronize()
    assert_round_trip(back, st, px, (dtype, frames))
    edge = 2048 if dt.itemsize < 4 else 1536
    stream = enc.stack().cpu().numpy()
    for f in sorted(x for x in {0, 1, edge - 1, edge, edge + 1, frames - 1} if x < frames):
        want = oracle.encode(px[f].cpu().numpy().view(dt))[0]
        got = stream[int(offs[f]): int(offs[f + 1])]
        assert got.size == want.size and (got == want).all(), (dtype, f)


def test_dense_walk_last_resort_and_stress(gpu, oracle):
    """The dense walk of listed frames (decode_dense.hip, route 5) in two test builds.  `denseserial` (-DTRPX_DENSE_FORCE_SERIAL):
    every listed frame skips its write pass and is walked by one lane from (0, 0) -- the last resort a frame takes when its
    speculative walks do not close.  `densetiny` (-DTRPX_DENSE_SEG_BLOCKS=1): regions of a few blocks, so that link walks cross
    dozens of regions, deep records collide and the write pass's checks (end state AND block count of every region) have to
    catch what the records got wrong -- frames that do not close end in the serial walk, none may be wrong (with 128-byte windows
    most frames did; a region is at least one 224-byte window now, and few do).  status[2] counts those frames."""
    for name, arg in (("denseserial", "all"), ("densetiny", "some")):
        run_variant(name, "dense_walk.py", arg)


def test_encoder_workspace_between_calls(gpu, oracle):
    """The single-pass encoder's descriptor words are cleared by the call's last kernel, and the library skips the clearing
    launch for a workspace it remembers as clean (include/trpx_hip.h, "Workspaces between calls").  Same workspace call after
    call, another geometry in between, the decoder given the same memory (the library forgets it by itself), a foreign
    write announced with trpx_workspace_invalidate -- the stream is the oracle's every time; a foreign write that is NOT
    announced (here: the whole workspace zeroed, tag included) is caught by the first tile's tag check: the call reports
    TRPX_ERR_TIMEOUT and Encoded.check() answers with the two-pass pipeline (Terse.hpp:500-549: identical bytes)."""
    import torch
    from trpx_amd import codec, _lib
    L = _lib.lib()
    n, frames = 512 * 512, 24
    px = codec.synth(np.uint16, 7, frames, n, device=gpu)
    want = oracle.encode_stack(px.cpu().numpy())[0]
    ws = codec.Workspace(gpu)

    def enc(p=px, w=want):
        e = codec.encode(p, workspace=ws)
        torch.cuda.synchronize()
        code = int(e.status[0].item())
        e.check()
        assert e.stack().cpu().numpy().tobytes() == w.tobytes()
        return code

    assert enc() == 0 and enc() == 0 and enc() == 0                       # unknown -> clean -> clean
    px2 = codec.synth(np.uint16, 90, 5, 300 * 300, device=gpu)             # another geometry in the same memory
    want2 = oracle.encode_stack(px2.cpu().numpy())[0]
    assert enc(px2, want2) == 0 and enc() == 0 and enc(px2, want2) == 0 and enc(px2, want2) == 0
    assert enc() == 0
    back, st = codec.decode(torch.from_numpy(want).to(gpu), codec.encode(px).frame_offsets, n, frames, np.uint16, workspace=ws)
    torch.cuda.synchronize()                                               # the decoder scribbles over the same workspace ...
    assert_round_trip(back, st, px, "the encoder's workspace given to the decoder")
    assert enc() == 0 and enc() == 0                                       # ... and the library knows
    ws.buf.fill_(0xA5)                                                     # a foreign write, announced
    L.trpx_workspace_invalidate(ws.buf.data_ptr(), ws.buf.numel())
    assert enc() == 0 and enc() == 0
    ws.buf.zero_()                                                         # a foreign write, NOT announced: the tag is gone
    assert enc() == _lib.ERR_TIMEOUT                                       # reported by the first tile; check() re-ran the call (two-pass)
    assert enc() == 0 and enc() == 0


@pytest.mark.parametrize("dtype", [np.uint16, np.int16])
def test_encoder_frames_two_bytes_behind_a_dword(gpu, oracle, dtype):
    """Stacks of 16-bit frames with an odd pixel count (513 x 511, ...): every second frame starts 2 bytes behind a dword
    boundary and is loaded through k_encode_fused_mis2's realigned loads (dword-aligned loads from the dword in front + funnel
    shifts, encode_fused.hip: load_raw_mis2); and a stack whose FIRST pixel sits there (every frame but the first realigned).
    Byte-identical to the oracle (Terse.hpp:500-549), incl. frames with a partial last block and tiles' halo blocks."""
    import torch
    rng = np.random.RandomState(3)
    for n, frames, shift in ((513 * 511, 9, 0), (12 * 1024 * 3 + 7, 6, 0), (300 * 300, 5, 1), (12 * 2048 + 1, 4, 1)):
        a = rng.poisson(2.0, (frames, n)).astype(np.int64)
        a[:, ::4099] = 3000
        if np.dtype(dtype).kind == "i":
            a = a - 2
        a = a.astype(dtype)
        want = oracle.encode_stack(a)[0]
        flat = torch.zeros(frames * n + 8, dtype=torch.int16, device=gpu)
        flat[shift: shift + frames * n] = torch.from_numpy(a.view(np.int16).reshape(-1)).to(gpu)
        px = flat[shift: shift + frames * n].view(frames, n)
        px = px.view(torch.uint16) if np.dtype(dtype).kind == "u" else px
        assert px.data_ptr() % 4 == 2 * shift
        enc = encode(px, index=False)
        assert enc.stack().cpu().numpy().tobytes() == want.tobytes(), (dtype, n, frames, shift)


def test_default_workspace_is_not_remembered(gpu, oracle):
    """codec.encode() without workspace= allocates its scratch itself and lets it die with the Encoded object: the library
    must not remember that memory as a clean workspace (torch's allocator hands the block to the next tensor).  Encode, drop,
    scribble over what comes back from the allocator -- all but the last words, where the tag sits --, encode the same
    geometry again: status 0 at the first attempt, the oracle's bytes."""
    import torch, gc
    from trpx_amd import codec
    n, frames = 512 * 512, 24
    px = codec.synth(np.uint16, 11, frames, n, device=gpu)
    want = oracle.encode_stack(px.cpu().numpy())[0].tobytes()
    for _ in range(3):
        e = codec.encode(px)
        torch.cuda.synchronize()
        assert int(e.status[0].item()) == 0 and e.stack().cpu().numpy().tobytes() == want
        ws_bytes = e._retry[1].numel()
        del e
        gc.collect()
        junk = torch.empty(ws_bytes - 4096, dtype=torch.uint8, device=gpu)  # (same size class: the caching allocator's block)
        junk.fill_(0x5A)
        torch.cuda.synchronize()
        del junk


@pytest.mark.parametrize("shape,frames,victim,route", [((512, 512), 70, 10, 0), ((1030, 1065), 5, 2, 0), ((512, 512), 70, 10, 5)])
def test_header_dense_hostile_streams(gpu, oracle, shape, frames, victim, route):
    """The same for the routes header-dense frames take -- Poisson(3) counts, a width change on one block in four: stacks of
    512 x 512 frames are handed over by the per-frame decoder to the position-parallel walk with one wavefront per frame
    (70 frames: the hand-over is decided by the stack's statistics), frames of 1030 x 1065 are voted header-dense by the index
    route's walkers (the victim's own vote may be garbage) and walked one workgroup per frame (k_seg_wg, decode_seg.hip).  Both
    count their blocks from states that are guesses until the
    links close, in passes that do not check widths against the pixel type: a damaged frame must end in TRPX_ERR_CORRUPT or,
    where only payload bits changed, in status 0 with every other frame exact.  route 5: the listed frames through the dense walk
    (decode_dense.hip: one speculative pass, link walks, a verified write pass, the serial walk as the last resort)."""
    with selected("trpx_set_decode_path", route):
        _header_dense_hostile(gpu, oracle, shape, frames, victim)


def _header_dense_hostile(gpu, oracle, shape, frames, victim):
    import torch
    from trpx_amd import codec, _lib, workloads
    n = shape[0] * shape[1]
    px = workloads.poisson_u16(3.0, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    good = enc.stack().clone()
    offs = enc.frame_offsets.clone()
    o = offs.cpu().numpy()
    lo, hi = int(o[victim]), int(o[victim + 1])
    want, _ = oracle.encode(px[victim].cpu().numpy())
    assert good[lo:hi].cpu().numpy().tobytes() == want.tobytes()
    ws = codec.Workspace(gpu)
    others = [f for f in range(frames) if f != victim]

    def run(stream):
        back, st = codec.decode(stream, offs, n, frames, np.uint16, workspace=ws)
        torch.cuda.synchronize()
        return back, int(st[0].item())

    def clean_call_still_works(after):
        back, s = run(good)
        assert s == 0 and torch.equal(back.view(torch.int16), px.view(torch.int16)), f"the workspace does not serve a clean call after: {after}"

    clean_call_still_works("nothing")
    g = torch.Generator().manual_seed(20260105)
    gross = {"ones": lambda b: b[lo:hi].fill_(0xFF), "zeroes": lambda b: b[lo:hi].zero_(),
             "noise": lambda b: b[lo:hi].copy_(torch.randint(0, 256, (hi - lo,), generator=g, dtype=torch.uint8).to(gpu)),
             "burst": lambda b: b[(lo + hi) // 2: (lo + hi) // 2 + 2048].copy_(torch.randint(0, 256, (2048,), generator=g, dtype=torch.uint8).to(gpu))}
    for what, spoil in gross.items():
        bad = good.clone()
        spoil(bad)
        back, s = run(bad)
        assert s == _lib.ERR_CORRUPT, (what, s)
        clean_call_still_works(what)
    seen = {0: 0, _lib.ERR_CORRUPT: 0}
    for k, p in enumerate([lo, hi - 1] + [int(q) for q in torch.randint(lo, hi, (22,), generator=g)]):
        bad = good.clone()
        bad[p] ^= 1 << (k % 8)
        back, s = run(bad)
        assert s in (0, _lib.ERR_CORRUPT), (p - lo, s)
        seen[s] += 1
        if s == 0:
            for f in others:
                assert torch.equal(back[f].view(torch.int16), px[f].view(torch.int16)), f"a flip in frame {victim} (byte {p - lo}) changed frame {f}"
    assert seen[_lib.ERR_CORRUPT] > 0 and seen[0] > 0, seen
    clean_call_still_works("single flips")
