"""GPU tests: trpx_decode_hist (decode_hist.hip).  The truth is numpy on the ORIGINAL pixels,
np.bincount(np.clip((px.astype(np.int64) - lo) >> shift, 0, n_bins - 1)) per group, compared for equality: the codec is lossless
and the counts are integers, so no decoder is trusted and no tolerance is needed.  Every output sits in the middle of a guarded
allocation, 64 sentinel elements on either side."""
import dataclasses
import json
import os
import statistics
import subprocess
import tempfile

import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import (CAPACITY, CORRUPT, OK, Guarded, encode, input_forms, ladder, ladder_holds_every_width, mixed, run_variant, status_block,
                         torch_dt)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A


def truth(px: np.ndarray, group: int, lo: int, shift: int, n_bins: int) -> np.ndarray:
    """[ceil(frames / group), n_bins] int64: numpy on the original pixels (>> is arithmetic: values below lo floor)"""
    px = px.reshape(px.shape[0], -1)
    bins = np.clip((px.astype(np.int64) - lo) >> shift, 0, n_bins - 1)
    return np.stack([np.bincount(bins[f0: f0 + group].ravel(), minlength=n_bins) for f0 in range(0, px.shape[0], group)]).astype(np.int64)


def rules(dt):
    """(name, lo, shift, n_bins) for a pixel type: the fixed list of bin rules every stack of the matrix is counted under"""
    info = np.iinfo(dt)
    edge = 100 if info.bits == 8 else 1000                  # the first edge of the 4096 bins: inside the type's range
    out = [("one bin", 0, 0, 1), ("unit bins from 0", 0, 0, 256), ("shift 4", 0, 4, 16),
           ("shift 32, one bin holds everything", int(info.min), 32, 2), ("shift 32, two bins", -(1 << 32) if info.min < 0 else 0, 32, 2),
           ("lo at the minimum", int(info.min), 1, 64), ("lo at the maximum", int(info.max), 0, 3),
           ("4096 bins", -edge if info.min < 0 else edge, 0, 4096),
           # lo further than 2^30 from 0: the 64-bit form of the bin rule for the 8- and 16-bit types too (decode_hist.hip: kNarrow)
           ("lo far above", 1 << 32, 0, 5), ("lo far below", -(1 << 30) - 1, 18, 4096)]
    if info.min < 0:
        out.append(("negative floors", -37, 3, 16))
    return out


# ---- the call ----------------------------------------------------------------------------------------------------------------
def _lib_():
    from trpx_amd import codec                              # (torch first, as in every other GPU test: the library is loaded behind it)
    return codec.lib()


def _spans(v, n, group=1):
    return _lib_().trpx_decode_hist_spans_per_group(v, n, group)


def _ws(enc, n_frames, group=1, n_bins=4096):
    from trpx_amd import codec
    import torch
    need = max(codec.decode_hist_workspace_bytes(enc.data.numel(), enc.n_values, n_frames, enc.dtype, n_bins, group=g) for g in {1, group})
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda")


def _hist(enc, dt, group, lo, shift, n_bins, mode="index", first=0, n_frames=None, ws=None):
    """One trpx_decode_hist call into a guarded allocation.  Returns (hist [groups, n_bins] int64 on the host, status word 0)
    after checking the guards."""
    from trpx_amd.codec import dtype_code
    import torch
    dt = np.dtype(dt)
    n_frames = enc.n_frames - first if n_frames is None else n_frames
    n_groups = -(-n_frames // min(group, n_frames))
    out = Guarded(n_groups * n_bins, np.uint64, SENTINEL)
    status = status_block()
    ws = _ws(enc, n_frames, group, n_bins) if ws is None else ws
    stack = enc.stack()
    offs, index = input_forms(enc, mode, first)
    rc = _lib_().trpx_decode_hist(dtype_code(dt), stack.data_ptr(), stack.numel(), offs.data_ptr() if offs is not None else None,
                                  index.data_ptr() if index is not None else None, enc.n_values, n_frames, 12, group, lo, shift, n_bins,
                                  out.view.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib_().trpx_last_error_string()
    torch.cuda.synchronize()
    return out.check("hist_out").reshape(n_groups, n_bins).astype(np.int64), int(status[0].item())


def _check(enc, px, group, lo, shift, n_bins, mode="index", what="", want=None, **kw):
    want = truth(px, group, lo, shift, n_bins) if want is None else want
    got, status = _hist(enc, px.dtype, group, lo, shift, n_bins, mode, **kw)
    ctx = (what, mode, px.dtype, px.shape, group, lo, shift, n_bins)
    assert status == OK, ctx
    assert got.shape == want.shape and np.array_equal(got, want), ctx
    return got


# the frame sizes at which each mechanism can fail: a partial and a whole last block, the group edge (256 blocks), the run edge
# (8 groups), two runs and a tail -- and five runs and a tail: two spans per frame, the partial counts and k_reduce_parts
N_VALUES = [1, 11, 12, 13, 3071, 3072, 3073, 24575, 24576, 24577, 49157, 122893]
FRAME_COUNTS = [1, 3, 5]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("v", N_VALUES)
def test_exactness_matrix(dt, v):
    n = FRAME_COUNTS[(N_VALUES.index(v) + DTYPES.index(dt)) % 3]           # (every size with every count over the six types)
    info = np.iinfo(dt)
    assert (_spans(v, n) > 1) == (v == 122893)              # the partials and k_reduce_parts are known to run there, and only there
    assert _spans(v, n) == (2 if v == 122893 else 1)
    for what, px in (("mixed", mixed(dt, (n, v), seed=n * 1000 + v % 1000, zero_stretch=True)), ("ladder", ladder(dt, (n, v), seed=v))):
        if what == "ladder" and v >= 12 * 3 * 33:            # (three cycles of the widths 0 .. 32)
            ladder_holds_every_width(px)
        enc = encode(px)
        ws = _ws(enc, n)
        for name, lo, shift, n_bins in rules(dt):
            got = _check(enc, px, 1, lo, shift, n_bins, what=f"{what} / {name}", ws=ws)
            assert (got.sum(axis=1) == v).all(), (what, name)                   # every pixel exactly once
            if name == "4096 bins" and v >= 3071:
                # pixels beyond BOTH clamped ends -- where the type has them: an 8-bit type spans 256 values, fewer than 4096 bins
                # of any power-of-two width cover, so only its lower end is clamped
                assert (px < lo).any() and got[:, 0].all(), (what, name)
                if info.bits > 8:
                    assert (px.astype(np.int64) >= lo + 4096).any() and got[:, -1].all(), (what, name)
            if name == "lo far above":
                assert (got[:, 0] == v).all()
            if name == "lo far below" and info.bits <= 16:  # (v + 2^30 + 1) >> 18 = 4096 for every pixel of these types
                assert (got[:, -1] == v).all()
            if name == "shift 32, one bin holds everything":
                assert (got[:, 0] == v).all()
            if name == "shift 32, two bins" and info.min < 0 and v >= 3071:
                assert got[:, 0].all() and got[:, 1].all()   # the negative pixels and the others


@pytest.mark.parametrize("dt, v", [(np.uint16, 13), (np.int8, 3073), (np.int32, 24577), (np.uint8, 49157), (np.int16, 122893)],
                         ids=lambda x: str(x) if isinstance(x, int) else np.dtype(x).name)
def test_groups(dt, v):
    """group 1, 2 (a ragged last group of one frame), the stack's, and a group larger than the stack, on five frames: each is the
    truth, and the sum of the per-frame rows."""
    n = 5
    px = mixed(dt, (n, v), seed=v, zero_stretch=True)
    enc = encode(px)
    some_spans = set()
    for name, lo, shift, n_bins in [r for r in rules(dt) if r[0] in ("unit bins from 0", "shift 4", "4096 bins", "negative floors")]:
        rows = _check(enc, px, 1, lo, shift, n_bins, what=name)
        for group in (2, 3, n, n + 2):
            some_spans.add(_spans(v, n, group) > 1)
            got = _check(enc, px, group, lo, shift, n_bins, what=f"{name} / group {group}")
            per = min(group, n)
            assert np.array_equal(got, np.stack([rows[f0: f0 + per].sum(axis=0) for f0 in range(0, n, per)]))
            last = n - (got.shape[0] - 1) * per
            assert got.sum(axis=1).tolist() == [per * v] * (got.shape[0] - 1) + [last * v]
    assert True in some_spans                                # (spans that cross frames, through the partials)


@pytest.mark.parametrize("dt", [np.uint16, np.int32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("v, n", [(49157, 5), (122893, 3)])
def test_input_forms_runs_and_sub_stacks_agree(dt, v, n):
    px = mixed(dt, (n, v), seed=17, zero_stretch=True)
    enc = encode(px)
    pairs = ((0, n), (1, n - 1), (n - 1, n), (1, 2))
    for name, lo, shift, n_bins in [r for r in rules(dt) if r[0] in ("unit bins from 0", "shift 4", "4096 bins")]:
        outs = [_check(enc, px, 1, lo, shift, n_bins, mode, what=f"forms / {name}") for mode in ("index", "offsets", "none")]
        outs.append(_check(enc, px, 1, lo, shift, n_bins, "index", what="second run"))
        for o in outs[1:]:
            assert o.tobytes() == outs[0].tobytes(), (dt, name)
        for a, b in pairs:                                  # frames [a, b) alone: frame_offsets + a, n_frames = b - a, no index
            sub = _check(enc, px[a:b], 1, lo, shift, n_bins, "offsets", what=f"frames [{a}, {b})", first=a, n_frames=b - a)
            assert sub.tobytes() == outs[0][a:b].tobytes()
            whole = _check(enc, px[a:b], b - a, lo, shift, n_bins, "offsets", what=f"frames [{a}, {b}) as one group", first=a, n_frames=b - a)
            assert np.array_equal(whole[0], outs[0][a:b].sum(axis=0))


@pytest.mark.parametrize("dt, lo, shift, n_bins", [(np.uint16, 0, 2, 64), (np.int16, -50, 3, 40)], ids=["uint16", "int16"])
def test_tail_sums_are_the_siblings_counts(dt, lo, shift, n_bins):
    """For k = 1 .. n_bins - 1 the pixels in the bins from k on are the pixels >= lo + k * 2^shift: the row counts of a sizes-only
    trpx_decode_sparse at that threshold."""
    from trpx_amd import codec
    from trpx_amd.codec import dtype_code
    import torch
    n, v = 3, 3073
    px = mixed(dt, (n, v), seed=23, zero_stretch=True)
    enc = encode(px)
    hist = _check(enc, px, 1, lo, shift, n_bins, what="sibling")
    stack = enc.stack()
    ws = torch.empty(codec.decode_sparse_workspace_bytes(stack.numel(), v, n, torch_dt(dt)), dtype=torch.uint8, device="cuda")
    for k in range(1, n_bins):
        rows = Guarded(n + 1, np.uint64, SENTINEL)
        st = status_block()
        rc = _lib_().trpx_decode_sparse(dtype_code(np.dtype(dt)), stack.data_ptr(), stack.numel(), enc.frame_offsets.data_ptr(), enc.index.data_ptr(), v, n,
                                        12, lo + (k << shift), rows.view.data_ptr(), None, None, 0, st.data_ptr(), ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib_().trpx_last_error_string()
        torch.cuda.synchronize()
        assert int(st[0].item()) in (OK, CAPACITY), k        # (sizes only: CAPACITY says there are events, the row offsets are valid)
        counts = np.diff(rows.check("row_offsets").astype(np.int64))
        assert np.array_equal(hist[:, k:].sum(axis=1), counts), (k, lo + (k << shift))


def _noncanonical_fixtures():
    with open(os.path.join(ROOT, "tests", "golden", "noncanonical.json")) as f:
        fx = json.load(f)["fixtures"]
    return [e for e in fx if e["block"] == 12 and np.dtype(e["dtype"]).itemsize <= 4]


@pytest.mark.parametrize("dtname", [np.dtype(d).name for d in DTYPES])
def test_noncanonical_streams(dtname):
    """Valid streams no encoder here writes (tests/noncanonical.py; the reference decodes every one: tests/golden/
    noncanonical.json), through tests/noncanonical_dev.py.  Padded widths: the same histogram on every form -- the one-bin rule
    must hold where a width is wider than its values need.  Restated widths without an index: CORRUPT (trpx_build_index's
    verdict).  Status 0 with wrong counts: never."""
    import torch
    import noncanonical as nc
    import noncanonical_dev as ncd
    from oracle import oracle as O
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
        ws = torch.empty(L.trpx_decode_hist_workspace_bytes(D.code, D.nbytes, D.n, D.frames, 12, 1, 4096) + 256, dtype=torch.uint8, device="cuda")
        for name, lo, shift, n_bins in [r for r in rules(np.dtype(dtname)) if r[0] in ("unit bins from 0", "shift 4", "4096 bins", "negative floors")]:
            want = truth(S.px, 1, lo, shift, n_bins).astype(np.uint64)
            for mode in ("index", "offsets", "none"):
                if mode == "index" and not have_index:
                    continue
                out, st = ncd.dev_buf(want.nbytes), status_block()
                offs, index = D._forms(mode, idx)
                rc = L.trpx_decode_hist(D.code, D.terse.data_ptr(), D.nbytes, offs, index, D.n, D.frames, 12, 1, lo, shift, n_bins, ncd.inner_ptr(out),
                                        st.data_ptr(), ws.data_ptr(), ws.numel(), ncd.stream_ptr())
                torch.cuda.synchronize()
                verdict = ncd.verdict(rc, int(st[0].item()), [ncd.dev_read(out, want.nbytes) + (want,)])
                ctx = (dtname, e["kind"], e["shape"], mode, name, verdict)
                assert verdict in (ncd.EXACT, ncd.REFUSED), ctx                  # never status 0 with wrong counts, never a write outside
                if padded:
                    assert verdict == ncd.EXACT, ctx                             # padded widths decode everywhere
                elif mode != "index":
                    assert verdict == ncd.REFUSED, ctx                           # restated widths have no index


def test_corrupt_index_and_short_offsets_are_rejected():
    """The whole stack is validated, also where no block is fetched (one bin: every block is counted from its width): a group
    offset that is off by 12 bits is found whichever group it is, and so is a frame-offset table whose end is short.  Status
    CORRUPT, nothing written outside hist_out (checked in _hist)."""
    import torch
    n, v, groups = 3, 7000, 3                               # ceil(ceil(7000 / 12) / 256)
    px = mixed(np.uint16, (n, v), seed=31, zero_stretch=True)
    enc = encode(px)
    for lo, shift, n_bins in ((0, 0, 1), (0, 0, 256)):
        _check(enc, px, 1, lo, shift, n_bins)
        for g in range(n * groups):
            bent = dataclasses.replace(enc, index=enc.index.clone())
            bent.index[: 8 * n * groups].view(torch.int64)[g] += 12              # (the index starts with the group offsets)
            assert _hist(bent, px.dtype, 1, lo, shift, n_bins)[1] == CORRUPT, g
            assert _hist(bent, px.dtype, n, lo, shift, n_bins)[1] == CORRUPT, g
        short = dataclasses.replace(enc, frame_offsets=enc.frame_offsets.clone())
        short.frame_offsets[-1] -= 1
        assert _hist(short, px.dtype, 1, lo, shift, n_bins)[1] == CORRUPT
        assert _hist(short, px.dtype, 1, lo, shift, n_bins, mode="offsets")[1] == CORRUPT


def test_the_build_without_the_skip_counts_alike():
    """The histnoskip build (make -C trpx_amd/csrc histnoskip: every block with a width is extracted) in a child python, against
    the product's histograms of the same seeded stacks: one mixed and one ladder stack, bins wide enough that the product counts
    most blocks from their width."""
    cases = {}
    for what, dt, n, v in (("mixed", np.int16, 3, 24577), ("ladder", np.uint32, 2, 122893)):
        px = mixed(dt, (n, v), seed=v, zero_stretch=True) if what == "mixed" else ladder(dt, (n, v), seed=v)
        enc = encode(px)
        for group, lo, shift, n_bins in ((1, -37 if what == "mixed" else 0, 4, 16), (n, 0, 0, 256), (1, 0, 12, 4096)):
            cases[f"{what}|{np.dtype(dt).name}|{n}|{v}|{group}|{lo}|{shift}|{n_bins}"] = _check(enc, px, group, lo, shift, n_bins, what=what)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "product.npz")
        np.savez(path, **cases)
        run_variant("histnoskip", "hist_equality.py", path)


def test_graph_capture_replays_with_new_stacks():
    from trpx_amd import codec
    import torch
    n, v, n_bins = 6, 511 * 513, 64
    stacks = [mixed(np.uint16, (n, v), seed=s, zero_stretch=True) for s in (9, 10)]
    encs = [encode(px) for px in stacks]
    data, offs, index = encs[0].data.clone(), encs[0].frame_offsets.clone(), encs[0].index.clone()   # (capacity-sized: one geometry)
    out = torch.zeros((2, n_bins), dtype=torch.int64, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")
    ws = codec.Workspace("cuda")
    nbytes = max(e.total_bytes() for e in encs)

    def call():
        codec.decode_hist(data[:nbytes], offs, v, n, torch.uint16, n_bins, group=3, lo=0, shift=10, index=index, out=out, workspace=ws, status=status)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # warm-up outside the capture
        call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), truth(stacks[0], 3, 0, 10, n_bins))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                     # one stream, no parallel branches
        call()
    for px, e in zip(stacks[::-1], encs[::-1]):
        data.copy_(e.data), offs.copy_(e.frame_offsets), index.copy_(e.index)    # the same buffers, another stack
        out.fill_(SENTINEL)
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status[0].item()) == OK
        assert np.array_equal(out.cpu().numpy(), truth(px, 3, 0, 10, n_bins))


def test_python_surfaces_and_the_host_form():
    from trpx_amd import codec
    from trpx_amd.terse import Terse
    import ctypes as C
    import torch
    rng = np.random.default_rng(43)
    n, v = 5, 20 * 35
    px = (rng.integers(0, 3000, size=(n, v)) - 700).astype(np.int16)
    px[:, 100:240] = rng.integers(-32768, 32768, size=(n, 140))
    enc = encode(px)
    for group, lo, shift, n_bins in ((1, 0, 0, 256), (2, -37, 3, 16), (n, -1000, 5, 4096), (n + 1, 0, 32, 2)):
        want = truth(px, group, lo, shift, n_bins)
        abi, status = _hist(enc, px.dtype, group, lo, shift, n_bins)
        assert status == OK and np.array_equal(abi, want)
        # the device-resident wrapper: index given, offsets only, neither
        for offs, index in ((enc.frame_offsets, enc.index), (enc.frame_offsets, None), (None, None)):
            hist, st = codec.decode_hist(enc.stack(), offs, v, n, torch.int16, n_bins, group=group, lo=lo, shift=shift, index=index)
            torch.cuda.synchronize()
            assert int(st[0].item()) == OK and hist.dtype == torch.int64 and tuple(hist.shape) == want.shape
            assert np.array_equal(hist.cpu().numpy(), want)
        # the host class
        t = Terse()
        t.push_back_stack(px)
        got = t.prolix_hist(group=group, lo=lo, shift=shift, n_bins=n_bins)
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
        # the _host form of the C ABI: offsets given and not
        stream = enc.stack().cpu().numpy()
        offs_h = enc.frame_offsets.cpu().numpy().astype(np.uint64)
        for o in (offs_h.ctypes.data, None):
            out = np.full(want.size + 2, SENTINEL, np.uint64)
            rc = _lib_().trpx_decode_hist_host(codec.dtype_code(torch.int16), stream.ctypes.data, stream.size, o, v, n, 12, group, lo, shift, n_bins,
                                               out[1:].ctypes.data, -1)
            assert rc == 0, _lib_().trpx_last_error_string()
            assert out[0] == SENTINEL and out[-1] == SENTINEL and np.array_equal(out[1:-1].astype(np.int64).reshape(want.shape), want)
    assert codec.decode_hist_workspace_bytes(enc.stack().numel(), v, n, torch.int16, 256) > 0
    assert np.array_equal(Terse().prolix_hist(n_bins=4), np.zeros((0, 4), np.int64))
    for kw in (dict(n_bins=0), dict(n_bins=4097), dict(n_bins=16, shift=33), dict(n_bins=16, lo=(1 << 32) + 1), dict(n_bins=16, group=0)):
        with pytest.raises(ValueError):
            codec.decode_hist(enc.stack(), enc.frame_offsets, v, n, torch.int16, **kw)
        with pytest.raises(ValueError):
            t.prolix_hist(**kw)


def test_cpp_class_prolix_hist():
    exe = os.path.join(ROOT, "tests", "cpp", "hist_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "hist_example.mk", "hist_example"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK hist example" in r.stdout, r.stdout + r.stderr


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_faster_than_decoding_and_counting():
    """500 x 512^2 u16 synth-v1 with the encoder's index, resident; per-frame histograms of 256 unit bins from 0.  The baseline
    is what a caller pays without this entry point: trpx_decode_indexed of the stack, then widen, shift, clamp, offset by frame
    and torch.bincount -- in the same process, repetitions interleaved, medians.  No margin: the call must only be no slower than
    the route it replaces.  (Measured on an MI355X: DESIGN.md section 4.21.)"""
    from trpx_amd import codec
    import torch
    n, side, n_bins, lo, shift = 500, 512, 256, 0, 0
    v = side * side
    px = codec.synth(np.uint16, 0, n, v)
    enc = codec.encode(px, index=True)
    enc.check()
    stack = enc.stack()
    pix = torch.empty((n, v), dtype=torch.uint16, device="cuda")
    st = torch.empty(8, dtype=torch.int32, device="cuda")
    out = torch.empty((n, n_bins), dtype=torch.int64, device="cuda")
    ws = codec.Workspace("cuda")
    frame_base = (torch.arange(n, dtype=torch.int64, device="cuda") * n_bins)[:, None]
    base = [None]

    def hist():
        codec.decode_hist(stack, enc.frame_offsets, v, n, torch.uint16, n_bins, group=1, lo=lo, shift=shift, index=enc.index, out=out, workspace=ws,
                          status=st)

    def replaced():
        codec.decode(stack, enc.frame_offsets, v, n, torch.uint16, out=pix, status=st, index=enc.index)
        b = ((pix.to(torch.int64) - lo) >> shift).clamp_(0, n_bins - 1)
        b += frame_base
        base[0] = torch.bincount(b.view(-1), minlength=n * n_bins).view(n, n_bins)

    for _ in range(2):
        hist()
        replaced()
    torch.cuda.synchronize()
    t_hist, t_old = [], []
    for _ in range(9):
        t_hist.append(_event_ms(hist))
        t_old.append(_event_ms(replaced))
    assert int(st[0].item()) == OK
    assert torch.equal(pix.view(torch.int16), px.view(torch.int16))
    assert torch.equal(out, base[0])                        # the two routes agree, value for value
    assert bool((out.sum(dim=1) == v).all())
    m_hist, m_old = statistics.median(t_hist), statistics.median(t_old)
    print(f"\n500 x 512^2 u16 synth-v1, 256 unit bins per frame: decode_hist {m_hist:.4f} ms, decode_indexed + widen / shift / clamp / bincount "
          f"{m_old:.4f} ms, ratio {m_old / m_hist:.2f}")
    assert m_hist <= m_old, (m_hist, m_old)
