"""GPU tests: trpx_decode_binned (decode_binned.hip).  The truth is numpy on the ORIGINAL pixels -- the
frame padded with zeros to multiples of the bin, reshape(F, out_h, bin_y, out_w, bin_x).sum((2, 4)) in int64, converted as
gpu_support.sum_truth converts -- compared for equality: the codec is lossless and the sums are integers, so no decoder is trusted
and no tolerance is needed.  Every output sits in the middle of a guarded allocation, 64 sentinel elements on either side."""
import dataclasses
import json
import os
import statistics
import subprocess

import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import (CORRUPT, GUARD, OK, Guarded, encode, input_forms, ladder, ladder_holds_every_width, mixed, status_block, sum_truth,
                         to_dev, to_np, torch_dt)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A
OUT_DTYPES = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
UNSUPPORTED = 2
GROUP = 3072                                                # values of a 256-block group
ACCS, TARGET, RUN = 8192, 1536, 8                           # accumulators of a band, workgroups a launch aims at, groups per run


def truth(px: np.ndarray, bin_y: int, bin_x: int, out_dt) -> np.ndarray:
    """[frames, out_h, out_w] of out_dt from px [frames, h, w]"""
    f, h, w = px.shape
    oh, ow = -(-h // bin_y), -(-w // bin_x)
    pad = np.zeros((f, oh * bin_y, ow * bin_x), np.int64)
    pad[:, :h, :w] = px
    s = pad.reshape(f, oh, bin_y, ow, bin_x).sum((2, 4))
    return sum_truth(s, 1, out_dt).reshape(f, oh, ow)


def out_types_for(dt):
    """the output types a stream of dt may be summed into"""
    return [o for o in OUT_DTYPES if not (np.dtype(dt).kind == "i" and np.dtype(o).kind == "u")]


# ---- the call ----------------------------------------------------------------------------------------------------------------
def _lib_():
    from trpx_amd import codec                              # (torch first, as in every other GPU test: the library is loaded behind it)
    return codec.lib()


def _out_code(out_dt):
    from trpx_amd.terse import _code
    return _code(out_dt, True)                              # (the output types include float32 / float64)


def _ws(enc, n_frames):
    from trpx_amd import codec
    import torch
    need = codec.decode_binned_workspace_bytes(enc.data.numel(), enc.n_values, n_frames, enc.dtype)
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda")


def _plan(h, w, bin_y, bin_x, n_frames):
    """(output rows per band, bands per frame): the header's formula; the bands are checked against the library's answer"""
    out_h, out_w = -(-h // bin_y), -(-w // bin_x)
    by_lds = -(-out_h // max(1, ACCS // out_w))
    by_runs = -(-(-(-(-(-h * w // 12)) // 256)) // RUN)
    want = min(out_h, max(by_lds, min(-(-TARGET // n_frames), by_runs)))
    rows = -(-out_h // want)
    bands = -(-out_h // rows)
    assert _lib_().trpx_decode_binned_bands_per_frame(h * w, w, bin_y, bin_x, n_frames) == bands, (h, w, bin_y, bin_x, n_frames)
    return rows, bands


def _binned(enc, dt, width, bin_y, bin_x, out_dt=np.int32, mode="index", first=0, n_frames=None, ws=None, expect_rc=0):
    """One trpx_decode_binned call into a guarded allocation.  Returns (binned [n_frames, out_h, out_w] on the host, status word
    0) after checking the guards."""
    from trpx_amd.codec import dtype_code
    import torch
    dt, out_dt = np.dtype(dt), np.dtype(out_dt)
    n_frames = enc.n_frames - first if n_frames is None else n_frames
    oh, ow = -(-(enc.n_values // width) // bin_y), -(-width // bin_x)
    out = Guarded(n_frames * oh * ow, out_dt, SENTINEL)
    status = status_block()
    stack = enc.stack()
    offs, index = input_forms(enc, mode, first)
    if ws is None and mode != "index":
        ws = _ws(enc, n_frames)
    rc = _lib_().trpx_decode_binned(dtype_code(dt), _out_code(out_dt), stack.data_ptr(),
                                    stack.numel(), offs.data_ptr() if offs is not None else None,
                                    index.data_ptr() if index is not None else None, enc.n_values, n_frames, 12, width, bin_y, bin_x,
                                    out.view.data_ptr(), status.data_ptr(), ws.data_ptr() if ws is not None else None,
                                    ws.numel() if ws is not None else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == expect_rc, _lib_().trpx_last_error_string()
    torch.cuda.synchronize()
    got = out.check("binned_out", untouched_from=0 if rc else None)
    return got.reshape(n_frames, oh, ow).copy(), int(status[0].item())


def _check(enc, px, bin_y, bin_x, out_dt=np.int32, mode="index", what="", **kw):
    want = truth(px, bin_y, bin_x, out_dt)
    got, status = _binned(enc, px.dtype, px.shape[2], bin_y, bin_x, out_dt, mode, **kw)
    ctx = (what, mode, px.dtype, px.shape, (bin_y, bin_x), np.dtype(out_dt).name)
    assert status == OK, ctx
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), ctx
    return got


# the frames at which each mechanism can fail: one pixel, a block, a block and a pixel, width 1, rows that are no multiple of 12,
# one value short of a group and the group edge, the run edge (8 groups) and a frame a row and a column larger, five runs and a tail
FRAMES = [(1, 1), (1, 12), (1, 13), (13, 1), (5, 37), (83, 37), (64, 48), (96, 256), (97, 257), (331, 371)]
FRAME_COUNTS = [1, 3, 5]
BINS = [(1, 1), (2, 2), (3, 5), (1, 7), (7, 1), (13, 13), (64, 64), "frame"]


def bins_for(h, w):
    out = []
    for b in BINS:
        by, bx = (h, w) if b == "frame" else b
        if by <= min(h, 64) and bx <= min(w, 64) and (by, bx) not in out:
            out.append((by, bx))
    return out


def frames_for(dt, hw):
    return FRAME_COUNTS[(FRAMES.index(hw) + DTYPES.index(dt)) % 3]         # (every size with every count over the six types)


def test_the_matrix_runs_one_band_and_interior_bands_with_edges_inside_groups():
    """Arithmetic on the matrix below (through trpx_decode_binned_bands_per_frame): some case is one band, and some case has at
    least three bands with an interior band whose two edges fall inside 256-block groups -- both of its edge groups are shared
    with a neighbour, also inside a block."""
    one, interior = [], []
    for dt in DTYPES:
        for h, w in FRAMES:
            n = frames_for(dt, (h, w))
            for by, bx in bins_for(h, w):
                rows, bands = _plan(h, w, by, bx, n)
                if bands == 1:
                    one.append((h, w, by, bx, n))
                lo, hi = rows * by * w, 2 * rows * by * w   # band 1
                if bands >= 3 and lo % GROUP and hi % GROUP and lo % 12 and hi % 12:
                    interior.append((h, w, by, bx, n, bands))
    assert one and interior
    assert any(c[:2] == (331, 371) for c in interior) and any(c[:2] == (97, 257) for c in interior)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("hw", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exactness_matrix(dt, hw):
    h, w = hw
    n = frames_for(dt, hw)
    outs = out_types_for(dt)
    for what, px in (("mixed", mixed(dt, (n, h, w), seed=n * 1000 + h * w % 1000, zero_stretch=True)),
                     ("ladder", ladder(dt, (n, h * w), seed=h * w).reshape(n, h, w))):
        if what == "ladder" and h * w >= 12 * 3 * 33:        # (three cycles of the widths 0 .. 32)
            ladder_holds_every_width(px.reshape(n, -1))
        enc = encode(px)
        for k, (by, bx) in enumerate(bins_for(h, w)):
            _plan(h, w, by, bx, n)
            _check(enc, px, by, bx, outs[(k + FRAMES.index(hw)) % len(outs)], what=what)
            if (by, bx) in ((1, 1), (2, 2)):                 # ... and into the type the sums never clamp in
                _check(enc, px, by, bx, np.int64, what=what)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_output_type(dt):
    h, w, n = 83, 37, 3
    px = mixed(dt, (n, h, w), seed=7, zero_stretch=True)
    enc = encode(px)
    for out_dt in OUT_DTYPES:
        if out_dt in out_types_for(dt):
            for by, bx in ((1, 1), (3, 5), (64, 37)):
                _check(enc, px, by, bx, out_dt, what="output types")
        else:                                               # a signed stream into an unsigned output: refused, nothing written
            _binned(enc, dt, w, 3, 5, out_dt, expect_rc=UNSUPPORTED)


def test_value_edges_clamp_keep_and_round_once():
    """64 x 64 bins (and their partial neighbours: a 70 x 66 frame) of INT32_MIN / INT32_MAX / UINT32_MAX: 4096 times the value
    leaves 32 bits (clamped), is kept in 64 bits, and is rounded once into float32 (2^44 - 2^12 needs 32 bits of mantissa)."""
    h, w = 70, 66
    for dt, pv in ((np.int32, -(1 << 31)), (np.int32, (1 << 31) - 1), (np.uint32, 0xFFFFFFFF)):
        px = np.full((2, h, w), pv, dt)
        enc = encode(px)
        for out_dt in out_types_for(dt):
            got = _check(enc, px, 64, 64, out_dt, what="edges")
            o = np.dtype(out_dt)
            if o.kind in "iu" and o.itemsize == 4:
                assert got[0, 0, 0] == (np.iinfo(o).min if pv < 0 else np.iinfo(o).max)          # clamped
            elif o.kind in "iu":
                assert int(got[0, 0, 0]) == 4096 * pv                                            # exact
            else:
                assert float(got[0, 0, 0]) == float(o.type(4096 * pv))                           # rounded once
            assert int(got[0, 1, 1]) == int(truth(px, 64, 64, out_dt)[0, 1, 1]) and (h - 64) * (w - 64) * abs(pv) < 2 ** 53
    px = np.full((1, h, w), -(1 << 31), np.int32)
    _binned(encode(px), np.int32, w, 64, 64, np.uint32, expect_rc=UNSUPPORTED)


def test_the_widest_output_row():
    """8192 sums in a row: a band is one output row, 64 KB of 64-bit accumulators for a 32-bit type"""
    for dt in (np.uint32, np.uint16):
        px = mixed(dt, (2, 3, 8192), seed=3, zero_stretch=True)
        enc = encode(px)
        assert _plan(3, 8192, 1, 1, 2) == (1, 3) and _plan(3, 8192, 2, 1, 2) == (1, 2)
        _check(enc, px, 1, 1, np.int64, what="widest row")
        _check(enc, px, 2, 1, np.float64, what="widest row")


@pytest.mark.parametrize("dt", [np.uint16, np.int32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("hw, n", [((97, 257), 5), ((331, 371), 3)])
def test_input_forms_runs_and_sub_stacks_agree(dt, hw, n):
    h, w = hw
    px = mixed(dt, (n, h, w), seed=17, zero_stretch=True)
    enc = encode(px)
    pairs = ((0, n), (1, n - 1), (n - 1, n), (1, 2))
    for by, bx in ((1, 1), (2, 2), (13, 13)):
        outs = [_check(enc, px, by, bx, np.int64, mode, what="forms") for mode in ("index", "offsets", "none")]
        outs.append(_check(enc, px, by, bx, np.int64, "index", what="second run"))
        for o in outs[1:]:
            assert o.tobytes() == outs[0].tobytes(), (dt, by, bx)
        for a, b in pairs:                                  # frames [a, b) alone: frame_offsets + a, n_frames = b - a, no index
            sub = _check(enc, px[a:b], by, bx, np.int64, "offsets", what=f"frames [{a}, {b})", first=a, n_frames=b - a)
            assert sub.tobytes() == outs[0][a:b].tobytes()


def test_agrees_with_decode_bins_with_one_bin():
    """a bin of the whole frame is trpx_decode_bins with one bin"""
    from trpx_amd import codec
    import torch
    n, h, w = 3, 64, 48
    for dt in (np.int16, np.uint32):
        px = mixed(dt, (n, h, w), seed=5, zero_stretch=True)
        enc = encode(px)
        bins, st = codec.decode_bins(enc.stack(), enc.frame_offsets, h * w, n, torch_dt(dt), to_dev(np.zeros(h * w, np.uint16)), 1, index=enc.index)
        torch.cuda.synchronize()
        assert int(st[0].item()) == OK
        got = _check(enc, px, h, w, np.int64, what="one bin")
        assert np.array_equal(got.reshape(n, 1), bins.cpu().numpy())


@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.uint32], ids=lambda d: np.dtype(d).name)
def test_agrees_with_decode_sum_with_group_one(dt):
    """a bin of one pixel is trpx_decode_sum with group 1, for every output type"""
    from trpx_amd import codec
    import torch
    n, h, w = 3, 97, 257
    px = mixed(dt, (n, h, w), seed=6, zero_stretch=True)
    enc = encode(px)
    for out_dt in out_types_for(dt):
        sums, st = codec.decode_sum(enc.stack(), enc.frame_offsets, h * w, n, torch_dt(dt), 1, out_dtype=torch_dt(out_dt), index=enc.index)
        torch.cuda.synchronize()
        assert int(st[0].item()) == OK
        got = _check(enc, px, 1, 1, out_dt, what="group 1")
        assert got.tobytes() == to_np(sums).tobytes()


def test_outputs_aligned_to_their_type_only_and_the_stream_to_four_bytes():
    """binned_out at odd element offsets inside a larger tensor (4-byte types at 4 mod 8, 8-byte types at 8 mod 16), the stream at
    4 mod 8 with other bytes around it"""
    from trpx_amd.codec import dtype_code
    import torch
    n, h, w = 3, 83, 37
    px = mixed(np.uint16, (n, h, w), seed=11, zero_stretch=True)
    enc = encode(px)
    nbytes = enc.stack().numel()
    for shift in (4, 12):
        host = np.full(shift + (nbytes + 3) // 4 * 4 + 64, 0xFF, np.uint8)
        host[shift: shift + nbytes] = to_np(enc.stack())
        host[shift + nbytes: shift + (nbytes + 3) // 4 * 4] = 0
        terse = to_dev(host)[shift: shift + nbytes]
        assert terse.data_ptr() % 16 == shift
        for out_dt in OUT_DTYPES:
            o = np.dtype(out_dt)
            for by, bx in ((2, 2), (1, 1)):
                oh, ow = -(-h // by), -(-w // bx)
                count = n * oh * ow
                for odd in (1, 3):
                    whole = to_dev(np.full(count + 2 * GUARD + odd, SENTINEL, o))
                    view = whole[GUARD + odd: GUARD + odd + count]
                    assert view.data_ptr() % (2 * o.itemsize) == o.itemsize
                    status = status_block()
                    rc = _lib_().trpx_decode_binned(dtype_code(np.dtype(np.uint16)), _out_code(o),
                                                    terse.data_ptr(), nbytes, enc.frame_offsets.data_ptr(), enc.index.data_ptr(), h * w, n, 12,
                                                    w, by, bx, view.data_ptr(), status.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, _lib_().trpx_last_error_string()
                    torch.cuda.synchronize()
                    a = to_np(whole)
                    fill = np.full(1, SENTINEL, o)[0]
                    assert int(status[0].item()) == OK
                    assert (a[:GUARD + odd] == fill).all() and (a[GUARD + odd + count:] == fill).all(), (out_dt, odd)
                    assert a[GUARD + odd: GUARD + odd + count].tobytes() == truth(px, by, bx, o).tobytes(), (out_dt, odd, shift)


def test_width_zero_groups_are_still_validated():
    """Group 1 of every frame holds nothing but width-0 blocks: nothing is fetched from it.  One bent group offset in front of it
    is found all the same, on a call that is well-formed in every other respect; and so is a frame-offset table whose end is
    short."""
    import torch
    n, h, w = 3, 96, 96                                     # three groups a frame
    px = mixed(np.uint16, (n, h, w), seed=31)
    px.reshape(n, -1)[:, GROUP - 24: 2 * GROUP + 24] = 0
    enc = encode(px)
    groups, blocks = 3, 768
    w_at = (8 * n * groups + 15) // 16 * 16                 # (the index: the group offsets, then the widths)
    widths = enc.index[w_at: w_at + n * blocks].cpu().numpy().reshape(n, blocks)
    assert not widths[:, 256:512].any() and widths[:, :254].any() and widths[:, 514:].any()
    for mode in ("index", "offsets", "none"):
        for by, bx in ((1, 1), (2, 2), (64, 64)):
            _check(enc, px, by, bx, mode=mode, what="width 0")
    for frame, group in ((1, 1), (0, 2), (2, 1)):
        bent = dataclasses.replace(enc, index=enc.index.clone())
        offs64 = bent.index[: 8 * n * groups].view(torch.int64)
        offs64[frame * groups + group] += 1
        for by, bx in ((1, 1), (2, 2), (64, 64)):
            assert _binned(bent, px.dtype, w, by, bx)[1] == CORRUPT, (frame, group, by, bx)
    short = dataclasses.replace(enc, frame_offsets=enc.frame_offsets.clone())
    short.frame_offsets[-1] -= 1
    assert _binned(short, px.dtype, w, 2, 2)[1] == CORRUPT
    assert _binned(short, px.dtype, w, 2, 2, mode="offsets")[1] == CORRUPT
    assert _binned(enc, px.dtype, w, 2, 2)[1] == OK


def _noncanonical_fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "noncanonical.json")) as f:
        fx = json.load(f)["fixtures"]
    return [e for e in fx if e["block"] == 12 and np.dtype(e["dtype"]).itemsize <= 4]


@pytest.mark.parametrize("dtname", [np.dtype(d).name for d in DTYPES])
def test_noncanonical_streams(dtname):
    """Valid streams no encoder here writes (tests/noncanonical.py; the reference decodes every one: tests/golden/
    noncanonical.json).  Padded widths: exact on every form.  Restated widths without an index: CORRUPT (trpx_build_index's
    verdict).  Status 0 with wrong sums: never."""
    import torch
    import noncanonical as nc
    from oracle import oracle as O
    from trpx_amd import codec
    from trpx_amd.codec import dtype_code
    fixtures = [e for e in _noncanonical_fixtures() if e["dtype"] == dtname]
    assert sorted(e["kind"] for e in fixtures) == sorted(nc.KINDS)
    for e in fixtures:
        S = nc.make(np.dtype(dtname), tuple(e["shape"]), e["kind"], e["variant"], 12)
        assert f"{O.fnv1a64(S.stream):016x}" == e["stream"] and f"{O.fnv1a64(S.px):016x}" == e["pixels"] and e["ref_decodes"]
        n, v = S.shape
        w = next(d for d in (37, 16, 12, 7, 5, 3, 2, 1) if v % d == 0)
        h = v // w
        px = S.px.reshape(n, h, w)
        host = np.zeros(S.stream.size + 16, np.uint8)
        host[: S.stream.size] = S.stream
        terse, nbytes = torch.from_numpy(host).cuda(), int(S.stream.size)
        offs = torch.from_numpy(S.offsets.astype(np.int64)).cuda()
        code = dtype_code(np.dtype(dtname))
        index = torch.zeros(codec.index_bytes(np.dtype(dtname), v, n), dtype=torch.uint8, device="cuda")
        st = status_block()
        assert _lib_().trpx_build_index(code, terse.data_ptr(), nbytes, offs.data_ptr(), v, n, 12, index.data_ptr(), st.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        have_index = int(st[0].item()) == OK
        if e["kind"] in ("K0", "K2"):
            assert have_index
        enc = dataclasses.make_dataclass("Stack", ["data", "frame_offsets", "index", "n_values", "n_frames", "dtype", "stack"])(
            terse, offs, index, v, n, torch_dt(dtname), lambda: terse[:nbytes])
        for by, bx in ((1, 1), (min(2, h), min(3, w))):
            want = truth(px, by, bx, np.int64)
            for mode in ("index", "offsets", "none"):
                if mode == "index" and not have_index:
                    continue
                got, status = _binned(enc, dtname, w, by, bx, np.int64, mode)
                ctx = (dtname, e["kind"], mode, by, bx)
                assert status in (OK, CORRUPT), ctx
                assert status == CORRUPT or np.array_equal(got, want), ctx       # never status 0 with wrong sums
                if e["kind"] in ("K0", "K2"):
                    assert status == OK, ctx                                     # padded widths decode everywhere
                elif mode != "index":
                    assert status == CORRUPT, ctx                                # restated widths have no index


def test_graph_capture_replays_on_a_second_stack():
    """one capture, replayed after a second stack of the same geometry has been written into the same buffers"""
    from trpx_amd import codec
    import torch
    n, h, w = 6, 331, 371
    v = h * w
    stacks = [mixed(np.uint16, (n, h, w), seed=s, zero_stretch=(s == 9)) for s in (9, 10)]
    encs = [encode(px) for px in stacks]
    cap = max(e.stack().numel() for e in encs)
    terse = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    offs = torch.zeros_like(encs[0].frame_offsets)
    index = torch.zeros_like(encs[0].index)
    assert encs[1].index.numel() == index.numel()

    def load(e):
        terse.zero_()
        terse[: e.stack().numel()].copy_(e.stack())
        offs.copy_(e.frame_offsets)
        index.copy_(e.index)
    out = torch.zeros((n, -(-h // 2), -(-w // 2)), dtype=torch.int32, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")

    def call():
        codec.decode_binned(terse[:cap], offs, v, n, torch.uint16, w, 2, index=index, out=out, status=status)
    load(encs[0])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # warm-up outside the capture
        call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), truth(stacks[0], 2, 2, np.int32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                     # one stream, no parallel branches
        call()
    for e, px in ((encs[1], stacks[1]), (encs[0], stacks[0])):
        load(e)
        out.fill_(SENTINEL)
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status[0].item()) == OK
        assert np.array_equal(out.cpu().numpy(), truth(px, 2, 2, np.int32))


def test_python_surfaces():
    from trpx_amd import codec
    from trpx_amd.terse import Terse
    import torch
    rng = np.random.default_rng(43)
    n, h, wd = 3, 20, 35
    px = rng.integers(0, 3000, size=(n, h, wd)).astype(np.uint16)
    px[:, 3:7] = rng.integers(0, 65536, size=(n, 4, wd))
    enc = encode(px)
    abi, status = _binned(enc, px.dtype, wd, 3, 4)
    assert status == OK and np.array_equal(abi, truth(px, 3, 4, np.int32))
    # the device-resident wrapper: an int bin and a pair, every input form, an output of the caller's
    got, st = codec.decode_binned(enc.stack(), enc.frame_offsets, h * wd, n, torch.uint16, wd, (3, 4), index=enc.index)
    torch.cuda.synchronize()
    assert int(st[0].item()) == OK and got.dtype == torch.int32 and tuple(got.shape) == (n, 7, 9) and np.array_equal(got.cpu().numpy(), abi)
    got, st = codec.decode_binned(enc.stack(), enc.frame_offsets, h * wd, n, torch.uint16, wd, 2, out_dtype=torch.float64)
    assert int(st[0].item()) == OK and tuple(got.shape) == (n, 10, 18) and np.array_equal(got.cpu().numpy(), truth(px, 2, 2, np.float64))
    mine = torch.zeros(n * 7 * 9, dtype=torch.int64, device="cuda")
    got, st = codec.decode_binned(enc.stack(), None, h * wd, n, torch.uint16, wd, (3, 4), out_dtype=torch.int64, out=mine)   # frames located, index built
    assert int(st[0].item()) == OK and got.data_ptr() == mine.data_ptr() and np.array_equal(got.cpu().numpy(), abi)
    assert codec.decode_binned_workspace_bytes(enc.stack().numel(), h * wd, n, torch.uint16) > 0
    with pytest.raises(TypeError):
        codec.decode_binned(enc.stack(), enc.frame_offsets, h * wd, n, torch.uint16, wd, 2, out_dtype=torch.int16)
    for bad in (0, 65, (21, 1), (1, 36)):
        with pytest.raises(ValueError):
            codec.decode_binned(enc.stack(), enc.frame_offsets, h * wd, n, torch.uint16, wd, bad)
    with pytest.raises(ValueError):
        codec.decode_binned(enc.stack(), enc.frame_offsets, h * wd, n, torch.uint16, 34, 2)
    with pytest.raises(ValueError):
        codec.decode_binned(enc.stack(), enc.frame_offsets, h * wd, n, torch.uint16, wd, 2, out=mine)
    # the host class
    t = Terse()
    t.push_back_stack(px)
    with pytest.raises(ValueError):
        t.prolix_binned(2)                                  # no dim() yet
    t.dim([wd, h])
    got = t.prolix_binned((3, 4))
    assert got.dtype == np.int32 and got.shape == (n, 7, 9) and np.array_equal(got, abi)
    got = t.prolix_binned(2, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, truth(px, 2, 2, np.float32))
    assert np.array_equal(t.prolix_binned(1, np.uint64), px.astype(np.uint64))
    for bad in (0, 65, (21, 1), (1, 36)):
        with pytest.raises(ValueError):
            t.prolix_binned(bad)
    s = Terse()
    s.push_back_stack(px.astype(np.int16))
    s.dim([wd, h])
    with pytest.raises(ValueError):
        s.prolix_binned(2, np.uint32)                       # signed data into an unsigned output


def test_cpp_class_prolix_binned():
    exe = os.path.join(ROOT, "tests", "cpp", "binned_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "binned_example.mk", "binned_example"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK binned example" in r.stdout, r.stdout + r.stderr


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_faster_than_decoding_and_summing():
    """500 x 512^2 u16 synth-v1 with the encoder's index, resident, binned 2 x 2 into int32.  The baseline is what a caller pays
    without this entry point: trpx_decode_indexed of the stack, then pix.view(n, 256, 2, 256, 2).sum((2, 4), dtype=int32) -- in
    the same process, repetitions interleaved, medians.  No margin: the call must only be no slower than the route it replaces."""
    from trpx_amd import codec
    import torch
    n, side = 500, 512
    v = side * side
    px = codec.synth(np.uint16, 0, n, v)
    enc = codec.encode(px, index=True)
    enc.check()
    stack = enc.stack()
    pix = torch.empty((n, v), dtype=torch.uint16, device="cuda")
    st = torch.empty(8, dtype=torch.int32, device="cuda")
    out = torch.empty((n, side // 2, side // 2), dtype=torch.int32, device="cuda")
    base = [None]

    def binned():
        codec.decode_binned(stack, enc.frame_offsets, v, n, torch.uint16, side, (2, 2), index=enc.index, out=out, status=st)

    def replaced():
        codec.decode(stack, enc.frame_offsets, v, n, torch.uint16, out=pix, status=st, index=enc.index)
        base[0] = pix.view(n, side // 2, 2, side // 2, 2).sum((2, 4), dtype=torch.int32)

    for _ in range(2):
        binned()
        replaced()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(9):
        t_new.append(_event_ms(binned))
        t_old.append(_event_ms(replaced))
    assert int(st[0].item()) == OK
    assert torch.equal(pix.view(torch.int16), px.view(torch.int16))
    assert torch.equal(out, base[0])                        # the two routes agree, value for value
    m_new, m_old = statistics.median(t_new), statistics.median(t_old)
    print(f"\n500 x 512^2 u16 synth-v1, 2 x 2 into int32: decode_binned {m_new:.4f} ms, decode_indexed + view.sum {m_old:.4f} ms, "
          f"ratio {m_old / m_new:.2f}")
    assert m_new <= m_old, (m_new, m_old)
