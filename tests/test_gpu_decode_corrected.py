"""GPU tests: trpx_decode_corrected (decode_corrected.hip).  The truth is numpy on the ORIGINAL pixels, all
float32: (px.astype(np.float32) - dark[None]) * gain[None] -- three IEEE operations, each rounded once -- and the outputs are
compared as uint32 BIT PATTERNS wherever the truth is not NaN, by isnan where it is.  The codec is lossless, so no decoder is
trusted and no tolerance is needed.  Results that are subnormal are unspecified (include/trpx_hip.h): the fixtures hold none, and
a test says so.  Every output sits in the middle of a guarded allocation."""
import dataclasses
import json
import os
import statistics
import subprocess

import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import CORRUPT, GUARD, OK, Guarded, encode, input_forms, ladder, ladder_holds_every_width, mixed, status_block, to_dev, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_FILL = 0x7FC5A5A5                                       # a NaN no float operation of the call yields: "never written"
F32_TINY = np.finfo(np.float32).tiny


def truth(px, dark=None, gain=None):
    """[frames, n_values] float32: the issue's expression; an absent map is an absent operation"""
    x = px.reshape(px.shape[0], -1).astype(np.float32)
    with np.errstate(all="ignore"):
        if dark is not None:
            x = x - dark[None]
        if gain is not None:
            x = x * gain[None]
    assert x.dtype == np.float32
    return x


def make_maps(v, seed=0):
    """(dark, gain) float32 [v]: fractional darks k + 0.5, gains with fractions, negative and zero entries, and -- where the frame has
    room -- +-inf and NaN in both and one huge dark (1e30).  |gain| is 0 or at least 0.75 and every finite difference is 0 or at
    least 0.5 in magnitude: no product is subnormal."""
    k = np.arange(v)
    dark = ((k * 7 + seed) % 41).astype(np.float32) + np.float32(0.5)
    gain = np.array([1.0, 1.25, -0.75, 0.0, 2.0, 1.0009765625, -1.0, 3.0], np.float32)[(k * 5 + k // 3 + seed) % 8]
    for at, d, g in ((3, np.inf, None), (17, -np.inf, None), (29, np.nan, None), (41, None, np.inf), (53, None, -np.inf), (67, None, np.nan),
                     (71, 1e30, None), (83, np.inf, 0.0), (v - 2, np.nan, np.inf), (v - 1, 1e30, -0.75)):
        if 0 <= at < v and v > 90:
            if d is not None:
                dark[at] = d
            if g is not None:
                gain[at] = g
    return dark, gain


def finite_maps(v, seed=0):
    k = np.arange(v)
    return ((k * 7 + seed) % 41).astype(np.float32) + np.float32(0.5), np.array([1.0, 1.25, -0.75, 0.0, 2.0], np.float32)[(k + seed) % 5]


def assert_bits(got, want, ctx):
    """got / want float32 of one shape: NaN where the truth is NaN, the truth's bits everywhere else"""
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, ctx
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (ctx, "NaN positions differ")
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError((ctx, f"{bad.size} elements differ, the first at non-NaN element {int(bad[0])}: {g[bad[0]]:#x} != {w[bad[0]]:#x}"))


def assert_no_subnormal(want, ctx):
    a = np.abs(want[np.isfinite(want)])
    assert not ((a > 0) & (a < F32_TINY)).any(), (ctx, "the fixture holds a subnormal result: unspecified, not to be tested")


# ---- the call ----------------------------------------------------------------------------------------------------------------
def _lib_():
    from trpx_amd import codec                              # (torch first, as in every other GPU test: the library is loaded behind it)
    return codec.lib()


def _ws(enc, n_frames):
    from trpx_amd import codec
    import torch
    need = codec.decode_corrected_workspace_bytes(enc.data.numel(), enc.n_values, n_frames, enc.dtype)
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda")


def _corr(enc, dt, dark, gain, mode="index", first=0, n_frames=None, ws=None, out_ptr=None):
    """One trpx_decode_corrected call into a guarded allocation prefilled with NAN_FILL (or to out_ptr).  dark / gain: device
    tensors or None.  Returns (out [frames, n_values] float32 on the host -- None with out_ptr --, status word 0) after checking
    the guards."""
    from trpx_amd import _lib
    from trpx_amd.codec import dtype_code
    import torch
    n_frames = enc.n_frames - first if n_frames is None else n_frames
    out = Guarded(n_frames * enc.n_values, np.uint32, NAN_FILL) if out_ptr is None else None
    status = status_block()
    if ws is None and mode != "index":
        ws = _ws(enc, n_frames)
    stack = enc.stack()
    offs, index = input_forms(enc, mode, first)
    rc = _lib_().trpx_decode_corrected(dtype_code(np.dtype(dt)), _lib.F32, stack.data_ptr(), stack.numel(), offs.data_ptr() if offs is not None else None,
                                       index.data_ptr() if index is not None else None, enc.n_values, n_frames, 12,
                                       dark.data_ptr() if dark is not None else None, gain.data_ptr() if gain is not None else None,
                                       out.view.data_ptr() if out_ptr is None else out_ptr, status.data_ptr(),
                                       ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib_().trpx_last_error_string()
    torch.cuda.synchronize()
    got = out.check("out").view(np.float32).reshape(n_frames, enc.n_values) if out is not None else None
    return got, int(status[0].item())


def _check(enc, px, dark, gain, mode="index", what="", **kw):
    want = truth(px, dark, gain)
    got, status = _corr(enc, px.dtype, to_dev(dark) if dark is not None else None, to_dev(gain) if gain is not None else None, mode, **kw)
    ctx = (what, mode, px.dtype, px.shape, dark is not None, gain is not None)
    assert status == OK, ctx
    assert_bits(got, want, ctx)
    return got


def big(dt):
    """two whole tiles (1024 blocks, 512 for 32-bit pixels), five blocks and a partial block of 7: odd, so frames 1 and 2 start off a
    16-byte boundary"""
    return (2 * 12288 if np.dtype(dt).itemsize <= 2 else 2 * 6144) + 5 * 12 + 7


def with_edges(px):
    """the 32-bit stacks hold the values whose conversion rounds: 2^24 + 1 (down) and 2^24 + 3 (up), and the types' ends"""
    dt = px.dtype
    if dt.itemsize == 4:
        vals = [(1 << 24) + 1, (1 << 24) + 3, (1 << 24) - 1, (1 << 25) + 2, np.iinfo(dt).max, np.iinfo(dt).min]
        if dt.kind == "i":
            vals += [-(1 << 24) - 1, -(1 << 24) - 3]
        flat = px.reshape(px.shape[0], -1)
        for f in range(flat.shape[0]):
            for i, val in enumerate(vals):
                at = (13 + 101 * i + 7 * f) % flat.shape[1]
                flat[f, at] = val
    return px


def test_the_edge_values_round_as_the_issue_says():
    """a check of the truth itself: numpy's conversion rounds to nearest even"""
    a = np.array([(1 << 24) + 1, (1 << 24) + 3, np.iinfo(np.uint32).max], np.uint32).astype(np.float32)
    assert a.tolist() == [16777216.0, 16777220.0, 4294967296.0]
    b = np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max], np.int32).astype(np.float32)
    assert b.tolist() == [-2147483648.0, 2147483648.0]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_exactness_matrix(dt):
    """ladder stacks (every width) and mixed stacks with zero stretches, maps with fractions, negative and zero gains, +-inf, NaN
    and 1e30; each map absent against the all-zero / all-one map; no result of the fixture is subnormal"""
    n, v = 3, big(dt)
    dark, gain = make_maps(v, seed=np.dtype(dt).itemsize)
    assert np.isinf(dark).any() and np.isnan(dark).any() and np.isinf(gain).any() and np.isnan(gain).any() and (dark == np.float32(1e30)).any()
    assert (gain < 0).any() and (gain == 0).any()
    zeros, ones = np.zeros(v, np.float32), np.ones(v, np.float32)
    for what, px in (("mixed", with_edges(mixed(dt, (n, v), seed=v % 1000, zero_stretch=True))), ("ladder", with_edges(ladder(dt, (n, v), seed=v)))):
        if what == "ladder":
            ladder_holds_every_width(ladder(dt, (n, v), seed=v))
        if np.dtype(dt).itemsize == 4:
            assert (px == (1 << 24) + 1).any() and (px == (1 << 24) + 3).any() and (px == np.iinfo(dt).max).any() and (px == np.iinfo(dt).min).any()
        enc = encode(px)
        for d, g in ((dark, gain), (None, gain), (dark, None), (None, None)):
            assert_no_subnormal(truth(px, d, g), (what, dt))
        both = _check(enc, px, dark, gain, what=what)
        assert np.isnan(both).any()
        # NULL dark / NULL gain: exactly the results of an all +0.0f / an all 1.0f map
        for d, g, d_map, g_map in ((None, gain, zeros, gain), (dark, None, dark, ones), (None, None, zeros, ones)):
            absent = _check(enc, px, d, g, what=f"{what} / absent map")
            present = _check(enc, px, d_map, g_map, what=f"{what} / neutral map")
            assert_bits(absent, present, (what, dt, "absent map != neutral map"))
        plain = _check(enc, px, None, None, what=f"{what} / plain float decode")
        assert np.array_equal(plain, px.astype(np.float32))


@pytest.mark.parametrize("dt", [np.uint16, np.int8, np.int32, np.uint32], ids=lambda d: np.dtype(d).name)
def test_shapes(dt):
    """the smallest frames that reach each path, 3 frames each: one value, a wavefront that is not full, exactly one full wavefront,
    the tile edge, and two tiles + five blocks + a partial block; 769: odd, one full wavefront and one value"""
    for v in sorted({1, 100, 768, 769, 6144 if np.dtype(dt).itemsize == 4 else 12288, 12288, big(dt)}):
        px = mixed(dt, (3, v), seed=v, zero_stretch=True)
        enc = encode(px)
        dark, gain = make_maps(v, seed=1)
        assert_no_subnormal(truth(px, dark, gain), (dt, v))
        _check(enc, px, dark, gain, what=f"v = {v}")
        _check(enc, px, None, None, what=f"v = {v}, no maps")


def test_large_frames_of_more_than_32k_blocks():
    v = 640 * 640
    assert -(-v // 12) > 32768
    px = mixed(np.uint16, (2, v), seed=5, zero_stretch=True)
    dark, gain = make_maps(v, seed=2)
    _check(encode(px), px, dark, gain, what="640 x 640")


def _pattern(n, seed):
    return (np.arange(n, dtype=np.uint64) * 2654435761 + seed).astype(np.uint32) | np.uint32(0x7F800001)      # position-dependent NaNs


@pytest.mark.parametrize("dt, v", [(np.uint16, 2 * 12288 + 67), (np.int32, 769), (np.uint8, 868)], ids=["uint16", "int32", "uint8"])
def test_alignment(dt, v):
    """out, dark and gain carved out of larger tensors 0, 4, 8 and 12 bytes past a 16-byte boundary, independently: a position-
    dependent pattern around the output is intact afterwards, and 0xFF bytes (NaN) around the maps would show in the result if a
    map were read outside [0, n_values).  868 values: a multiple of 4 with one full wavefront, so every frame takes the staged
    16-byte path where the three residues are 0 and the 4-byte one elsewhere; the odd sizes mix both within one stack."""
    import torch
    n = 3
    px = mixed(dt, (n, v), seed=v, zero_stretch=True)
    enc = encode(px)
    dark, gain = finite_maps(v, seed=3)
    want = truth(px, dark, gain)
    assert not np.isnan(want).any()
    for ko in range(4):
        for kd in range(4):
            for kg in range(4):
                if v > 1000 and (ko + kd + kg) % 3 and not ko == kd == kg:       # (the large frame: a third of the 64 triples)
                    continue
                before = _pattern(n * v + 2 * GUARD + 4, ko)
                whole = to_dev(before)
                maps = []
                for k, m in ((kd, dark), (kg, gain)):
                    host = np.full(v + 2 * GUARD + 4, 0xFFFFFFFF, np.uint32)
                    host[GUARD + k: GUARD + k + v] = m.view(np.uint32)
                    t = to_dev(host)
                    assert t.data_ptr() % 16 == 0
                    maps.append(t[GUARD + k: GUARD + k + v].view(torch.float32))
                assert whole.data_ptr() % 16 == 0 and maps[0].data_ptr() % 16 == 4 * kd and maps[1].data_ptr() % 16 == 4 * kg
                view = whole[GUARD + ko: GUARD + ko + n * v]
                _, status = _corr(enc, dt, maps[0], maps[1], out_ptr=view.data_ptr())
                after = to_np(whole)
                ctx = (dt, v, ko, kd, kg)
                assert status == OK, ctx
                assert np.array_equal(after[:GUARD + ko], before[:GUARD + ko]) and np.array_equal(after[GUARD + ko + n * v:], before[GUARD + ko + n * v:]), \
                    (ctx, "written outside out")
                assert_bits(after[GUARD + ko: GUARD + ko + n * v].view(np.float32).reshape(n, v), want, ctx)


@pytest.mark.parametrize("dt", [np.uint16, np.int32], ids=lambda d: np.dtype(d).name)
def test_input_forms_and_sub_stacks_agree(dt):
    n, v = 5, big(dt)
    px = mixed(dt, (n, v), seed=17, zero_stretch=True)
    enc = encode(px)
    dark, gain = make_maps(v, seed=4)
    outs = [_check(enc, px, dark, gain, mode, what="forms") for mode in ("index", "offsets", "none")]
    outs.append(_check(enc, px, dark, gain, "index", what="second run"))
    for o in outs[1:]:
        assert o.tobytes() == outs[0].tobytes()
    for a, b in ((0, n), (1, n - 1), (n - 1, n), (1, 2)):     # frames [a, b) alone: frame_offsets + a, n_frames = b - a, no index
        sub = _check(enc, px[a:b], dark, gain, "offsets", what=f"frames [{a}, {b})", first=a, n_frames=b - a)
        assert sub.tobytes() == outs[0][a:b].tobytes()


@pytest.mark.parametrize("dt, v", [(np.uint16, 2 * 12288 + 67), (np.uint8, 13), (np.int32, 6144 + 1)], ids=["uint16", "uint8", "int32"])
def test_every_element_is_written(dt, v):
    """out is prefilled with a NaN pattern (_corr); with finite maps no element keeps it, whichever maps are present"""
    px = mixed(dt, (3, v), seed=v, zero_stretch=True)
    enc = encode(px)
    dark, gain = finite_maps(v)
    for d, g in ((dark, gain), (None, gain), (dark, None), (None, None)):
        for mode in ("index", "none"):
            got = _check(enc, px, d, g, mode, what="prefilled")
            assert not np.isnan(got).any() and not (got.view(np.uint32) == NAN_FILL).any()


def _noncanonical_fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "noncanonical.json")) as f:
        fx = json.load(f)["fixtures"]
    return [e for e in fx if e["block"] == 12 and np.dtype(e["dtype"]).itemsize <= 4]


@pytest.mark.parametrize("dtname", [np.dtype(d).name for d in DTYPES])
def test_noncanonical_streams(dtname):
    """Valid streams no encoder here writes (tests/noncanonical.py; the reference decodes every one: tests/golden/
    noncanonical.json), through tests/noncanonical_dev.py.  Padded widths decode on every form.  Restated widths without an
    index: CORRUPT.  Status 0 with wrong pixels: never, and nothing is written outside the output."""
    import torch
    import noncanonical as nc
    import noncanonical_dev as ncd
    from oracle import oracle as O
    from trpx_amd import _lib
    fixtures = [e for e in _noncanonical_fixtures() if e["dtype"] == dtname]
    assert sorted(e["kind"] for e in fixtures) == sorted(nc.KINDS)
    L = _lib_()
    for e in fixtures:
        S = nc.make(np.dtype(dtname), tuple(e["shape"]), e["kind"], e["variant"], 12)
        assert f"{O.fnv1a64(S.stream):016x}" == e["stream"] and f"{O.fnv1a64(S.px):016x}" == e["pixels"] and e["ref_decodes"]
        D = ncd.Dev(S)
        built, idx, _ = D.build_index()
        have_index = built == ncd.EXACT
        padded = e["kind"] in ("K0", "K2")
        if padded:
            assert have_index
        dark, gain = finite_maps(D.n, seed=5)
        want = truth(S.px, dark, gain)
        d_dark, d_gain = to_dev(dark), to_dev(gain)
        ws = torch.empty(L.trpx_decode_corrected_workspace_bytes(D.code, D.nbytes, D.n, D.frames, 12) + 256, dtype=torch.uint8, device="cuda")
        for mode in ("index", "offsets", "none"):
            if mode == "index" and not have_index:
                continue
            out, st = ncd.dev_buf(want.nbytes), status_block()
            offs, index = D._forms(mode, idx)
            rc = L.trpx_decode_corrected(D.code, _lib.F32, D.terse.data_ptr(), D.nbytes, offs, index, D.n, D.frames, 12, d_dark.data_ptr(),
                                         d_gain.data_ptr(), ncd.inner_ptr(out), st.data_ptr(), ws.data_ptr(), ws.numel(), ncd.stream_ptr())
            torch.cuda.synchronize()
            verdict = ncd.verdict(rc, int(st[0].item()), [ncd.dev_read(out, want.nbytes) + (want,)])
            ctx = (dtname, e["kind"], e["shape"], mode, verdict)
            assert verdict in (ncd.EXACT, ncd.REFUSED), ctx                      # never status 0 with wrong pixels, never a write outside
            if padded:
                assert verdict == ncd.EXACT, ctx                                 # padded widths decode everywhere
            elif mode != "index":
                assert verdict == ncd.REFUSED, ctx                               # restated widths have no index


def test_corrupt_index_and_short_offsets_are_rejected():
    """Every tile of every frame is validated against what follows it: a tile offset that is off by 12 bits is found whichever
    tile it is, and so is a frame-offset table whose end is short.  Status CORRUPT, nothing written outside out (checked in
    _corr).  (The kernel reads the offset of a tile's first group of 256 blocks: those are the entries bent.)"""
    import torch
    n, v = 3, 2 * 12288 + 67                                # u16: 3 tiles of 4 groups a frame, 9 groups
    groups, per_tile = 9, 4
    px = mixed(np.uint16, (n, v), seed=31, zero_stretch=True)
    enc = encode(px)
    dark, gain = (to_dev(m) for m in finite_maps(v))
    assert _corr(enc, px.dtype, dark, gain)[1] == OK
    for f in range(n):
        for t in range(0, groups, per_tile):
            bent = dataclasses.replace(enc, index=enc.index.clone())
            bent.index[: 8 * n * groups].view(torch.int64)[f * groups + t] += 12     # (the index starts with the group offsets)
            assert _corr(bent, px.dtype, dark, gain)[1] == CORRUPT, (f, t)
    wide = dataclasses.replace(enc, index=enc.index.clone())
    wide.index[(8 * n * groups + 15) // 16 * 16 + 5] = 17                            # a width above the type's
    assert _corr(wide, px.dtype, dark, gain)[1] == CORRUPT
    short = dataclasses.replace(enc, frame_offsets=enc.frame_offsets.clone())
    short.frame_offsets[-1] -= 1
    assert _corr(short, px.dtype, dark, gain)[1] == CORRUPT
    assert _corr(short, px.dtype, dark, gain, mode="offsets")[1] == CORRUPT


def test_graph_capture_replays_with_new_maps():
    from trpx_amd import codec
    import torch
    n, v = 4, 511 * 513
    px = mixed(np.uint16, (n, v), seed=9, zero_stretch=True)
    enc = encode(px)
    maps = [finite_maps(v, seed=s) for s in (1, 2)]
    dark, gain = to_dev(maps[0][0]), to_dev(maps[0][1])
    out = torch.zeros((n, v), dtype=torch.float32, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")
    stack = enc.stack()

    def call():
        codec.decode_corrected(stack, enc.frame_offsets, v, n, torch.uint16, dark=dark, gain=gain, index=enc.index, out=out, status=status)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # warm-up outside the capture
        call()
    torch.cuda.synchronize()
    assert_bits(out.cpu().numpy(), truth(px, *maps[0]), "warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                     # one stream, no parallel branches
        call()
    for d, gn in maps[::-1]:
        dark.copy_(to_dev(d)), gain.copy_(to_dev(gn))        # the same buffers, other maps
        out.fill_(float("nan"))
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status[0].item()) == OK
        assert_bits(out.cpu().numpy(), truth(px, d, gn), "replay")
    assert not np.array_equal(truth(px, *maps[0]), truth(px, *maps[1]))


def test_python_surfaces_and_the_host_form():
    from trpx_amd import _lib, codec
    from trpx_amd.terse import Terse
    import torch
    rng = np.random.default_rng(43)
    n, v = 5, 20 * 35
    px = (rng.integers(0, 3000, size=(n, v)) - 700).astype(np.int16)
    px[:, 100:240] = rng.integers(-32768, 32768, size=(n, 140))
    enc = encode(px)
    dark, gain = make_maps(v, seed=6)
    t = Terse()
    t.push_back_stack(px)
    stream = enc.stack().cpu().numpy()
    offs_h = enc.frame_offsets.cpu().numpy().astype(np.uint64)
    for d, g in ((dark, gain), (None, gain), (dark, None), (None, None)):
        want = truth(px, d, g)
        dd, dg = (to_dev(m) if m is not None else None for m in (d, g))
        # the device-resident wrapper: index given, offsets only, neither
        for offs, index in ((enc.frame_offsets, enc.index), (enc.frame_offsets, None), (None, None)):
            out, st = codec.decode_corrected(enc.stack(), offs, v, n, torch.int16, dark=dd, gain=dg, index=index)
            torch.cuda.synchronize()
            assert int(st[0].item()) == OK and out.dtype == torch.float32 and tuple(out.shape) == (n, v)
            assert_bits(out.cpu().numpy(), want, "codec.decode_corrected")
        # the host class, whole and a sub-stack
        got = t.prolix_corrected(dark=d, gain=g)
        assert got.dtype == np.float32 and got.shape == (n, v)
        assert_bits(got, want, "Terse.prolix_corrected")
        assert_bits(t.prolix_corrected(dark=d, gain=g, first=1, n=3), want[1:4], "Terse.prolix_corrected [1, 4)")
        # the _host form of the C ABI: offsets given and not
        for o in (offs_h.ctypes.data, None):
            out = np.full(want.size + 2, NAN_FILL, np.uint32)
            rc = _lib_().trpx_decode_corrected_host(codec.dtype_code(torch.int16), _lib.F32, stream.ctypes.data, stream.size, o, v, n, 12,
                                                    d.ctypes.data if d is not None else None, g.ctypes.data if g is not None else None,
                                                    out[1:].ctypes.data, -1)
            assert rc == 0, _lib_().trpx_last_error_string()
            assert out[0] == NAN_FILL and out[-1] == NAN_FILL
            assert_bits(out[1:-1].view(np.float32).reshape(n, v), want, "trpx_decode_corrected_host")
    assert codec.decode_corrected_workspace_bytes(enc.stack().numel(), v, n, torch.int16) > 0
    assert t.prolix_corrected(first=n).shape == (0, v)
    assert Terse().prolix_corrected().shape[0] == 0
    for kw in (dict(dark=dark[:-1]), dict(gain=np.zeros(v + 1, np.float32)), dict(first=n + 1), dict(first=2, n=n)):
        with pytest.raises(ValueError):
            t.prolix_corrected(**kw)
    with pytest.raises(ValueError):
        codec.decode_corrected(enc.stack(), enc.frame_offsets, v, n, torch.int16, dark=to_dev(dark[:-1]))
    with pytest.raises(ValueError):
        codec.decode_corrected(enc.stack(), enc.frame_offsets, v, n, torch.int16, gain=to_dev(gain.astype(np.float64)))


def test_cpp_class_prolix_corrected():
    exe = os.path.join(ROOT, "tests", "cpp", "corrected_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "corrected_example.mk", "corrected_example"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK corrected example" in r.stdout, r.stdout + r.stderr


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_faster_than_decoding_and_correcting():
    """500 x 512^2 u16 synth-v1 with the encoder's index, resident.  The baseline is what a caller pays without this entry point:
    trpx_decode_indexed of the stack, then (pix.to(torch.float32) - dark) * gain -- in the same process, repetitions interleaved,
    medians.  The two outputs are first shown equal bit for bit.  No margin: the call must only never be slower than the route it
    replaces.  (Measured on an MI355X: DESIGN.md section 4.22.)"""
    from trpx_amd import codec
    import torch
    n, side = 500, 512
    v = side * side
    px = codec.synth(np.uint16, 0, n, v)
    enc = codec.encode(px, index=True)
    enc.check()
    stack = enc.stack()
    d_h, g_h = finite_maps(v, seed=7)
    dark, gain = to_dev(d_h), to_dev(g_h)
    pix = torch.empty((n, v), dtype=torch.uint16, device="cuda")
    st = torch.empty(8, dtype=torch.int32, device="cuda")
    out = torch.empty((n, v), dtype=torch.float32, device="cuda")
    base = [None]

    def corrected():
        codec.decode_corrected(stack, enc.frame_offsets, v, n, torch.uint16, dark=dark, gain=gain, index=enc.index, out=out, status=st)

    def replaced():
        codec.decode(stack, enc.frame_offsets, v, n, torch.uint16, out=pix, status=st, index=enc.index)
        base[0] = (pix.to(torch.float32) - dark) * gain

    for _ in range(2):
        corrected()
        replaced()
    torch.cuda.synchronize()
    assert int(st[0].item()) == OK
    assert torch.equal(pix.view(torch.int16), px.view(torch.int16))
    assert torch.equal(out.view(torch.int32), base[0].view(torch.int32))         # the two routes agree, bit for bit (finite maps: no NaN)
    t_new, t_old = [], []
    for _ in range(9):
        t_new.append(_event_ms(corrected))
        t_old.append(_event_ms(replaced))
    assert int(st[0].item()) == OK
    m_new, m_old = statistics.median(t_new), statistics.median(t_old)
    print(f"\n500 x 512^2 u16 synth-v1, dark and gain: decode_corrected {m_new:.4f} ms, decode_indexed + to(float32) - dark * gain "
          f"{m_old:.4f} ms, ratio {m_old / m_new:.2f}")
    assert m_new <= m_old, (m_new, m_old)
