"""GPU tests: trpx_decode_reduce (decode_reduce.hip).  The truth is numpy on the ORIGINAL pixels
(tests/reduce_truth.py): the codec is lossless, so no decoder is trusted.  Every result is compared byte for byte, and every
output of a device call lies between two bands of a sentinel that must stay intact."""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import reduce_truth as R
from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import CORRUPT, GUARD, OK, encode, events_median, input_forms, mixed, status_block, to_dev, to_np, torch_dt
from tiff_layout import parse_tiff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 77
SIGNED = [d for d in DTYPES if np.dtype(d).kind == "i"]
UNSIGNED = [d for d in DTYPES if np.dtype(d).kind == "u"]


def _name(dt):
    return np.dtype(dt).name


def _chunks(dt, n_frames, n_values, group):
    from trpx_amd import _lib
    from trpx_amd.codec import dtype_code
    return _lib.lib().trpx_decode_reduce_chunks(dtype_code(np.dtype(dt)), n_values, n_frames, group)


def _reduce(enc, dt, group, op, threshold=0, mode="index", first=0, n_frames=None, odd=0, stack=None, index=None, what="", at=None):
    """One call into a guarded output that starts `odd` elements behind the guard: (result on the host, status word 0).  The
    sentinels around the output are checked whatever the status.  at: (remainder, modulus) the output's address must have."""
    from trpx_amd import codec
    import torch
    n = enc.n_frames - first if n_frames is None else n_frames
    odt = R.out_dtype(dt, op)
    count = -(-n // group) * enc.n_values
    whole = to_dev(np.full(count + 2 * GUARD + odd, SENTINEL, odt))
    view = whole[GUARD + odd: GUARD + odd + count]
    assert view.data_ptr() % odt.itemsize == 0 and (at is None or view.data_ptr() % at[1] == at[0]), (view.data_ptr(), at)
    offs, idx = input_forms(enc, mode, first)
    st = status_block()
    out, st2 = codec.decode_reduce(enc.stack() if stack is None else stack, offs, enc.n_values, n, torch_dt(dt), group, op, threshold=threshold,
                                   out=view, index=idx if index is None else index, status=st)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr() and st2.data_ptr() == st.data_ptr()
    a = to_np(whole)
    fill = np.full(1, SENTINEL, odt)[0]
    assert (a[:GUARD + odd] == fill).all() and (a[GUARD + odd + count:] == fill).all(), ("written outside the output", what, _name(dt), op, group, mode)
    return a[GUARD + odd: GUARD + odd + count].reshape(-1, enc.n_values), int(st[0].item())


def _check(px, enc, group, op, threshold=0, mode="index", **kw):
    got, code = _reduce(enc, px.dtype, group, op, threshold, mode, **kw)
    ctx = (_name(px.dtype), px.shape, group, op, threshold, mode)
    assert code == OK, ctx
    want = R.truth(px, group, op, threshold)
    assert got.shape == want.shape and got.dtype == want.dtype, ctx
    assert got.tobytes() == want.tobytes(), ctx


def _every_op(px, enc, group, mode="index", thresholds=None, **kw):
    for op in ("max", "min", "sumsq"):
        _check(px, enc, group, op, mode=mode, **kw)
    for t in (R.thresholds(px.dtype) if thresholds is None else thresholds):
        _check(px, enc, group, "count", t, mode, **kw)


# (3, 6144 + 3072 + 5): a tile, a sub-tile and a partial block; (5, 513 * 511): frames start inside a cache line
SHAPES = [(9, 7), (11, 12 * 37 + 5), (3, 6144 + 3072 + 5), (5, 513 * 511), (6, 512 * 512)]


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exactness_matrix(dt, shape):
    n, v = shape
    px = mixed(dt, shape, seed=n * 1000 + v)
    enc = encode(px)
    for group in sorted({1, 3, n - 1, n, n + 5}):           # (n - 1: a group that does not divide n)
        _every_op(px, enc, group)
    if np.dtype(dt).itemsize == 4 and shape == (11, 12 * 37 + 5):
        # the fixture does what it is for: the true sums of squares of 32-bit mixed data pass 2^64, and the result is the wrapped one
        exact = R.sumsq_exact(px, n)[0]
        wrapped = R.sumsq_truth(px, n)[0]
        assert max(exact) >= 1 << 64 and [int(x) for x in wrapped] == [e % (1 << 64) for e in exact]
        assert any(int(w) != e for w, e in zip(wrapped, exact))


def _one_sign(dt, shape, seed, sign):
    """every pixel strictly negative (sign = -1: signed types) or strictly positive, small and large magnitudes"""
    info = np.iinfo(dt)
    rng = np.random.default_rng(seed)
    top = int(info.max) if sign > 0 else -int(info.min)
    mag = np.where(rng.random(shape) < 0.3, rng.integers(1, top + 1, size=shape, dtype=np.int64), rng.integers(1, 6, size=shape, dtype=np.int64))
    mag.reshape(-1)[::1009] = top                           # the type's minimum / maximum itself
    return (sign * mag).astype(dt)


@pytest.mark.parametrize("dt", [np.int16, np.int32], ids=_name)
def test_max_of_negative_frames_and_a_blank_one(dt):
    """The accumulators start at the type's minimum, not at zero -- and the zeros of width-0 blocks take part: one blank frame
    lifts every maximum to 0."""
    n, v = 6, 6144 + 3072 + 5
    px = _one_sign(dt, (n, v), 21, -1)
    assert (px < 0).all() and (px == np.iinfo(dt).min).any()
    blank = px.copy()
    blank[4] = 0
    for data in (px, blank):
        enc = encode(data)
        for group in (1, 2, 4, n):
            for mode in ("index", "offsets"):
                _check(data, enc, group, "max", mode=mode)
    assert (R.max_truth(px, n) < 0).all() and (R.max_truth(blank, n) == 0).all() and (R.max_truth(blank, 4)[0] < 0).all()


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.uint32, np.int16, np.int32], ids=_name)
def test_min_of_positive_frames_and_a_blank_one(dt):
    n, v = 6, 6144 + 3072 + 5
    px = _one_sign(dt, (n, v), 22, +1)
    assert (px > 0).all() and (px == np.iinfo(dt).max).any()
    blank = px.copy()
    blank[1] = 0
    for data in (px, blank):
        enc = encode(data)
        for group in (1, 2, 4, n):
            for mode in ("index", "offsets"):
                _check(data, enc, group, "min", mode=mode)
    assert (R.min_truth(px, n) > 0).all() and (R.min_truth(blank, n) == 0).all() and (R.min_truth(blank, 4)[1] > 0).all()


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_empty_chunks_leave_the_identity(dt):
    """(11, 7) with group 10: ten chunks of one frame, and the last output -- one frame -- has nine chunks without frames.  What
    they leave in the partial slab must not move the merge: with all pixels of one sign, zeros there would show in max or min."""
    n, v, group = 11, 7, 10
    assert _chunks(dt, n, v, group) == 10
    signs = (-1, +1) if np.dtype(dt).kind == "i" else (+1,)
    for sign in signs:
        px = _one_sign(dt, (n, v), 23, sign)
        enc = encode(px)
        for mode in ("index", "offsets", "none"):
            _every_op(px, enc, group, mode)
        assert (R.max_truth(px, group)[1] < 0).all() if sign < 0 else (R.min_truth(px, group)[1] > 0).all()


# the launch plan's paths on tiny stacks (the chunk count is asserted: if the plan changes, pick shapes by the same criteria)
@pytest.mark.parametrize("shape, group, chunks", [
    ((2100, 40), 2, 1),                                     # 1050 units of one chunk of two frames: the pipelined loop alone
    ((2100, 40), 2100, 700),                                # 700 chunks of 3
    ((40, 6144 * 30), 40, 20),                              # chunks > 1 and more than one frame a chunk, on full tiles
], ids=["one-chunk", "700-chunks", "chunks-of-2-full-tiles"])
@pytest.mark.parametrize("dt", [np.int16, np.uint32], ids=_name)
def test_plan_paths(dt, shape, group, chunks):
    n, v = shape
    assert _chunks(dt, n, v, group) == chunks
    px = mixed(dt, shape, seed=7 + n, zero_stretch=True)
    enc = encode(px)
    _every_op(px, enc, group, thresholds=(1, int(np.iinfo(dt).max) // 3))
    _check(px, enc, group, "max", mode="offsets")


def test_input_forms_agree():
    px = mixed(np.uint16, (40, 513 * 511), seed=3)
    enc = encode(px)
    for op, group, t in (("max", 7, 0), ("min", 40, 0), ("sumsq", 7, 0), ("count", 9, 3)):
        outs = [_reduce(enc, np.uint16, group, op, t, mode) for mode in ("index", "offsets", "none")]
        assert all(code == OK for _, code in outs)
        assert all(outs[0][0].tobytes() == o.tobytes() for o, _ in outs)
        assert outs[0][0].tobytes() == R.truth(px, group, op, t).tobytes()


def test_sub_range():
    px = mixed(np.int16, (30, 5000), seed=11)
    enc = encode(px)
    for a, b in ((0, 30), (5, 17), (29, 30), (3, 4)):
        for op, t in (("max", 0), ("min", 0), ("sumsq", 0), ("count", -2)):
            got, code = _reduce(enc, np.int16, 4, op, t, mode="offsets", first=a, n_frames=b - a)
            assert code == OK and got.tobytes() == R.truth(px[a:b], 4, op, t).tobytes(), (a, b, op)


def test_large_int32_frames():
    """Two 4096^2 int32 frames: the index comes from the large-frame walk."""
    rng = np.random.default_rng(7)
    v = 4096 * 4096
    px = (rng.poisson(3.0, size=(2, v)) - 1).astype(np.int32)
    px[1, : v // 3] = rng.integers(-(1 << 31), (1 << 31) - 1, size=v // 3, dtype=np.int64).astype(np.int32)
    enc = encode(px)
    for op in ("max", "sumsq"):
        for mode in ("index", "offsets", "none"):
            _check(px, enc, 2, op, mode=mode)
        _check(px, enc, 1, op)


@pytest.mark.parametrize("dt, at", [(np.uint8, (1, 2)), (np.int8, (1, 2)), (np.uint16, (2, 128)), (np.int16, (2, 128)), (np.uint32, (4, 8)),
                                    (np.int32, (4, 8))], ids=lambda x: _name(x) if isinstance(x, type) else "")
def test_outputs_aligned_to_their_element_only(dt, at):
    """max / min of T at an address that is aligned to T only (u8 at an odd byte, u16 at 2 mod 128, 32-bit types at 4 mod 8),
    counts at 4 mod 8, sums of squares at 8 mod 16; the sentinels on both sides stay intact (_reduce checks them)."""
    px = mixed(dt, (5, 6144 + 3072 + 5), seed=31, zero_stretch=True)
    enc = encode(px)
    for group in (1, 2, 5):
        for mode in ("index", "offsets"):
            _check(px, enc, group, "max", mode=mode, odd=1, at=at)
            _check(px, enc, group, "min", mode=mode, odd=1, at=at)
            _check(px, enc, group, "count", 1, mode, odd=1, at=(4, 8))
            _check(px, enc, group, "sumsq", mode=mode, odd=1, at=(8, 16))


def test_corruption():
    """status 5, and nothing written outside the output (the guards are checked in _reduce)"""
    px = mixed(np.uint16, (12, 513 * 511), seed=13)
    enc = encode(px)
    bad_index = enc.index.clone().fill_(0xFF)
    total = enc.total_bytes()
    cut = enc.stack()[: total // 2].clone()
    for op in R.OPS:
        for group in (3, 12):                               # one chunk a group / a partial slab
            assert _reduce(enc, np.uint16, group, op, 1, index=bad_index, what="index of 0xFF")[1] == CORRUPT
            # a truncated stream: the last frames' chains run past the buffer
            assert _reduce(enc, np.uint16, group, op, 1, mode="offsets", stack=cut, what="cut, offsets")[1] == CORRUPT
            assert _reduce(enc, np.uint16, group, op, 1, mode="none", stack=cut, what="cut, no offsets")[1] == CORRUPT
    _check(px, enc, 3, "max")


def _noncanonical_fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "noncanonical.json")) as f:
        fx = json.load(f)["fixtures"]
    return [e for e in fx if e["block"] == 12 and np.dtype(e["dtype"]).itemsize <= 4]


@pytest.mark.parametrize("dtname", [_name(d) for d in DTYPES])
def test_noncanonical_streams(dtname):
    """Valid streams no encoder here writes (tests/noncanonical.py; the reference decodes every one: tests/golden/
    noncanonical.json).  Padded widths: exact on every form.  Restated widths without an index: CORRUPT (trpx_build_index's
    verdict).  Status 0 with wrong values: never."""
    import torch
    import noncanonical as nc
    from oracle import oracle as O
    from trpx_amd import _lib, codec
    from trpx_amd.codec import dtype_code
    fixtures = [e for e in _noncanonical_fixtures() if e["dtype"] == dtname]
    assert sorted(e["kind"] for e in fixtures) == sorted(nc.KINDS)
    for e in fixtures:
        S = nc.make(np.dtype(dtname), tuple(e["shape"]), e["kind"], e["variant"], 12)
        assert f"{O.fnv1a64(S.stream):016x}" == e["stream"] and f"{O.fnv1a64(S.px):016x}" == e["pixels"] and e["ref_decodes"]
        n, v = S.shape
        host = np.zeros(S.stream.size + 16, np.uint8)
        host[: S.stream.size] = S.stream
        terse, nbytes = torch.from_numpy(host).cuda(), int(S.stream.size)
        offs = torch.from_numpy(S.offsets.astype(np.int64)).cuda()
        index = torch.zeros(codec.index_bytes(np.dtype(dtname), v, n), dtype=torch.uint8, device="cuda")
        st = status_block()
        assert _lib.lib().trpx_build_index(dtype_code(np.dtype(dtname)), terse.data_ptr(), nbytes, offs.data_ptr(), v, n, 12, index.data_ptr(),
                                           st.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        have_index = int(st[0].item()) == OK
        if e["kind"] in ("K0", "K2"):
            assert have_index
        enc = dataclasses.make_dataclass("Stack", ["data", "frame_offsets", "index", "n_values", "n_frames", "dtype", "stack"])(
            terse, offs, index, v, n, torch_dt(dtname), lambda: terse[:nbytes])
        for op, group, t in (("max", n, 0), ("min", 2, 0), ("sumsq", n, 0), ("count", 2, 1)):
            want = R.truth(S.px, group, op, t)
            for mode in ("index", "offsets", "none"):
                if mode == "index" and not have_index:
                    continue
                got, status = _reduce(enc, np.dtype(dtname), group, op, t, mode)
                ctx = (dtname, e["kind"], mode, op)
                assert status in (OK, CORRUPT), ctx
                assert status == CORRUPT or got.tobytes() == want.tobytes(), ctx     # never status 0 with wrong values
                if e["kind"] in ("K0", "K2"):
                    assert status == OK, ctx                                         # padded widths reduce exactly everywhere
                elif mode != "index":
                    assert status == CORRUPT, ctx                                    # restated widths have no index


@pytest.mark.parametrize("mode", ["offsets", "none"])
@pytest.mark.parametrize("op, group", [("max", 64), ("sumsq", 8)])
def test_graph_capture(mode, op, group):
    """(group 64: one output, a partial slab and the merge inside the capture; group 8: one chunk)"""
    from trpx_amd import codec
    import torch
    px = mixed(np.uint16, (64, 513 * 511), seed=9)
    enc = encode(px)
    stack = enc.stack()
    offs = enc.frame_offsets if mode == "offsets" else None
    ws = codec.Workspace(stack.device)
    ws.get(codec.decode_reduce_workspace_bytes(stack.numel(), enc.n_values, enc.n_frames, np.uint16, group, op))
    out = torch.empty((64 // group, enc.n_values), dtype=codec.reduce_out_dtype(np.uint16, op), device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")

    def call():
        codec.decode_reduce(stack, offs, enc.n_values, enc.n_frames, np.uint16, group, op, out=out, workspace=ws, status=status)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # warm-up outside the capture
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                     # one stream, no parallel branches
        call()
    out.view(torch.uint8).zero_()
    status.fill_(77)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert int(status[0].item()) == OK
    assert to_np(out).tobytes() == R.truth(px, group, op).tobytes()


def test_python_surfaces(tmp_path):
    """Terse.prolix_reduce on an object and on a file read back; codec.decode_reduce's own checks"""
    from trpx_amd import codec
    from trpx_amd.terse import Terse
    import torch
    for dt in (np.uint16, np.int16, np.uint8, np.int32):
        px = mixed(dt, (10, 48 * 64), seed=17)
        t = Terse()
        t.push_back_stack(px)
        path = tmp_path / f"s_{_name(dt)}.trpx"
        with open(path, "wb") as f:
            t.write(f)
        with open(path, "rb") as f:
            r = Terse.read(f)
        for obj in (t, r):
            for group in (None, 1, 4):
                for op, thr in (("max", 0), ("min", 0), ("sumsq", 0), ("count", 2)):
                    got = obj.prolix_reduce(op, group, thr)
                    want = R.truth(px, group or 10, op, thr)
                    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (_name(dt), group, op)
        with pytest.raises(ValueError):
            t.prolix_reduce("median")
        with pytest.raises(ValueError):
            t.prolix_reduce("max", 0)
    px = mixed(np.uint16, (10, 48 * 64), seed=17)
    enc = encode(px)
    got, st = codec.decode_reduce(enc.stack(), None, enc.n_values, 10, torch.uint16, 4, "count", threshold=3)   # frames located, index built
    torch.cuda.synchronize()
    assert int(st[0].item()) == OK and got.dtype == torch.uint32 and tuple(got.shape) == (3, 48 * 64)
    assert to_np(got).tobytes() == R.count_truth(px, 4, 3).tobytes()
    got, st = codec.decode_reduce(enc.stack(), enc.frame_offsets, enc.n_values, 10, torch.uint16, 4, codec.REDUCE_OPS["max"], index=enc.index)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint16 and to_np(got).tobytes() == R.max_truth(px, 4).tobytes()
    with pytest.raises(ValueError):
        codec.decode_reduce(enc.stack(), enc.frame_offsets, enc.n_values, 10, torch.uint16, 4, "mean")
    with pytest.raises(ValueError):
        codec.decode_reduce(enc.stack(), enc.frame_offsets, enc.n_values, 10, torch.uint16, 4, "sumsq", out=got)   # uint16 is not what sumsq writes
    assert codec.decode_reduce_workspace_bytes(enc.stack().numel(), enc.n_values, 10, torch.uint16, 4, "min") > 0


def test_cli_max(tmp_path):
    """prolix -max N writes the per-pixel maxima of N consecutive frames as a TIFF stack of the frames' own type; its -max path is
    the C++ Terse::prolix_reduce."""
    from trpx_amd.terse import Terse
    prolix = os.path.join(ROOT, "trpx_amd", "bin", "prolix")
    assert os.path.exists(prolix), "build() builds the CLI tools"
    for dt in (np.uint16, np.int16):
        px = mixed(dt, (10, 64 * 48), seed=17).reshape(10, 48, 64)
        t = Terse()
        t.push_back_stack(px.reshape(10, -1))
        t.dim([64, 48])
        path = tmp_path / f"s_{_name(dt)}.trpx"
        with open(path, "wb") as f:
            t.write(f)
        r = subprocess.run([prolix, "-max", "4", str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = parse_tiff(str(tmp_path / f"s_{_name(dt)}.tif"))
        want = R.max_truth(px.reshape(10, -1), 4)
        assert got.dtype == np.dtype(dt) and got.shape == (3, 48, 64) and got.reshape(3, -1).tobytes() == want.tobytes()
        both = subprocess.run([prolix, "-max", "4", "-sum", "4", str(path)], capture_output=True, text=True, timeout=300)
        assert both.returncode != 0 and "-sum and -max" in both.stderr
    assert "-max N" in subprocess.run([prolix, "-help"], capture_output=True, text=True, timeout=60).stdout


def test_cpp_class_prolix_reduce():
    exe = os.path.join(ROOT, "tests", "cpp", "reduce_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "reduce_example.mk", "reduce_example"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK reduce example" in r.stdout, r.stdout + r.stderr


# The ceiling on t_reduce / t_sum: what was measured on an MI355X with room for the run-to-run spread of the repetitions.  Four
# processes on two machines gave 0.931, 0.921, 0.925 and 0.921 (0.104 against 0.112-0.113 ms; the replaced route 0.149-0.153 ms, so
# reduce / replaced 0.68-0.70): the reduce does trpx_decode_sum's walk and writes int16 where the sum writes int32 (DESIGN.md
# section 4.19).
RATIO_CEILING = 1.10


def test_speed_against_the_route_it_replaces():
    """500 x 512^2 int16 (synth-v1, clipped to the type) with the encoder's index, resident, max over groups of 10.  The route the
    call replaces is trpx_decode_indexed of the stack, then pix.view(n // g, g, v).amax(1) -- int16, which torch reduces
    natively, so the baseline pays no widening copy.  A call slower than that has no reason to exist: no margin.  Beside it,
    trpx_decode_sum of the same stack and group into int32: the same walk."""
    from trpx_amd import codec
    import torch
    n, v, group = 500, 512 * 512, 10
    px = codec.synth(np.uint16, 0, n, v).to(torch.int32).clamp_(max=32767).to(torch.int16)
    enc = codec.encode(px, index=True)
    enc.check()
    torch.cuda.synchronize()
    stack = enc.stack()
    pix = torch.empty((n, v), dtype=torch.int16, device="cuda")
    out = torch.empty((n // group, v), dtype=torch.int16, device="cuda")
    sums = torch.empty((n // group, v), dtype=torch.int32, device="cuda")
    st = torch.empty(8, dtype=torch.int32, device="cuda")
    ws = codec.Workspace(stack.device)
    ws.get(max(codec.decode_reduce_workspace_bytes(stack.numel(), v, n, np.int16, group, "max"),
               codec.decode_sum_workspace_bytes(stack.numel(), v, n, np.int16, group)))

    def replaced():
        codec.decode(stack, enc.frame_offsets, v, n, torch.int16, out=pix, status=st, index=enc.index)
        return pix.view(n // group, group, v).amax(1)

    def reduce():
        codec.decode_reduce(stack, enc.frame_offsets, v, n, np.int16, group, "max", out=out, index=enc.index, workspace=ws, status=st)
    want = replaced()
    reduce()
    torch.cuda.synchronize()
    assert int(st[0].item()) == OK and torch.equal(out, want) and torch.equal(pix, px)
    t_old = events_median(replaced, 15)
    t_new = events_median(reduce, 15)
    t_sum = events_median(lambda: codec.decode_sum(stack, enc.frame_offsets, v, n, np.int16, group, out=sums, index=enc.index, workspace=ws,
                                                   status=st), 15)
    print(f"\nmax of 10 x 50: decode_indexed + amax {t_old:.4f} ms, decode_reduce {t_new:.4f} ms, decode_sum {t_sum:.4f} ms, "
          f"reduce / replaced {t_new / t_old:.3f}, reduce / sum {t_new / t_sum:.3f}")
    assert t_new <= t_old, (t_new, t_old)
    assert t_new <= RATIO_CEILING * t_sum, (t_new, t_sum)
