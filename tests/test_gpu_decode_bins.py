"""GPU tests: trpx_decode_bins (decode_bins.hip).  The truth is numpy on the ORIGINAL pixels, np.add.at in
int64 over the unmasked pixels, compared for equality: the codec is lossless and the sums are integers, so no decoder is trusted
and no tolerance is needed.  Every output sits in the middle of a guarded allocation, 64 sentinel elements on either side."""
import dataclasses
import json
import os
import statistics
import subprocess

import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import CORRUPT, OK, Guarded, encode, input_forms, ladder, ladder_holds_every_width, mixed, status_block, to_dev, torch_dt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A
MASKED = 0xFFFF
WIDTH = 37                                                  # the row length the 2-D maps use: no multiple or divisor of 12


def truth(px: np.ndarray, labels: np.ndarray, n_bins: int) -> np.ndarray:
    """[frames, n_bins] int64: numpy on the original pixels, the pixels whose label is no bin left out"""
    px = px.reshape(px.shape[0], -1)
    keep = labels < n_bins
    idx = labels[keep].astype(np.int64)
    out = np.zeros((px.shape[0], n_bins), np.int64)
    for f in range(px.shape[0]):
        np.add.at(out[f], idx, px[f, keep].astype(np.int64))
    return out


# ---- the maps --------------------------------------------------------------------------------------------------------------------
def rings(v, n_bins, width=WIDTH, scale=None):
    """Rings about the middle of a frame of rows of `width`; what lies further out than n_bins rings is masked."""
    y, x = np.arange(v) // width, np.arange(v) % width
    h = -(-v // width)
    r = np.sqrt((x - width // 2) ** 2 + (y - h // 2) ** 2)
    scale = max(1.0, float(r.max()) / (n_bins + 3)) if scale is None else scale
    ring = np.floor(r / scale).astype(np.int64)
    return np.where(ring < n_bins, ring, MASKED).astype(np.uint16)


def label_sets(v, seed):
    """(name, labels [v] uint16, n_bins): n_bins in {1, 2, 37, 4096}"""
    rng = np.random.default_rng(seed)
    p = np.arange(v)
    first, last = np.full(v, MASKED, np.uint16), np.full(v, MASKED, np.uint16)
    first[0], last[v - 1] = 1, 0
    rnd = rng.integers(0, 4200, size=v).astype(np.uint16)   # (some labels behind the last bin)
    rnd[rng.integers(0, v, size=8)] = MASKED
    rnd[v - 1] = 4095                                       # the last bin ...
    if v > 1:
        rnd[rng.integers(0, v - 1)] = 4096                  # ... and the first label that is none
        assert (rnd == 4095).any() and (rnd == 4096).any()
    return [("one bin", np.zeros(v, np.uint16), 1), ("p % 37", (p % 37).astype(np.uint16), 37), ("p % 2", (p % 2).astype(np.uint16), 2),
            ("rings", rings(v, 37), 37), ("masked", np.full(v, MASKED, np.uint16), 2), ("first pixel", first, 2), ("last pixel", last, 2),
            ("random4096", rnd, 4096)]


# ---- the call ----------------------------------------------------------------------------------------------------------------
def _lib_():
    from trpx_amd import codec                              # (torch first, as in every other GPU test: the library is loaded behind it)
    return codec.lib()


def _ws(enc, n_frames, n_bins=4096):
    from trpx_amd import codec
    import torch
    need = codec.decode_bins_workspace_bytes(enc.data.numel(), enc.n_values, n_frames, enc.dtype, n_bins)
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda")


def _bins(enc, dt, labels, n_bins, mode="index", first=0, n_frames=None, ws=None, lab_dev=None):
    """One trpx_decode_bins call into a guarded allocation; labels: [n_values] uint16 on the host (lab_dev: the device tensor to
    pass instead).  Returns (bins [n_frames, n_bins] on the host, status word 0) after checking the guards."""
    from trpx_amd.codec import dtype_code
    import torch
    dt = np.dtype(dt)
    n_frames = enc.n_frames - first if n_frames is None else n_frames
    if lab_dev is None:
        lab_dev = to_dev(np.ascontiguousarray(labels, dtype=np.uint16))
    out = Guarded(n_frames * n_bins, np.int64, SENTINEL)
    status = status_block()
    ws = _ws(enc, n_frames) if ws is None else ws
    stack = enc.stack()
    offs, index = input_forms(enc, mode, first)
    rc = _lib_().trpx_decode_bins(dtype_code(dt), stack.data_ptr(), stack.numel(), offs.data_ptr() if offs is not None else None,
                                  index.data_ptr() if index is not None else None, enc.n_values, n_frames, 12, lab_dev.data_ptr(), n_bins,
                                  out.view.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib_().trpx_last_error_string()
    torch.cuda.synchronize()
    return out.check("bins_out").reshape(n_frames, n_bins).copy(), int(status[0].item())


def _check(enc, px, labels, n_bins, mode="index", what="", want=None, **kw):
    want = truth(px, labels, n_bins) if want is None else want
    got, status = _bins(enc, px.dtype, labels, n_bins, mode, **kw)
    ctx = (what, mode, px.dtype, px.shape, n_bins)
    assert status == OK, ctx
    assert got.dtype == np.int64 and np.array_equal(got, want), ctx
    return got


# the frame sizes at which each mechanism can fail: a partial and a whole last block, the group edge (256 blocks), the run edge
# (8 groups), two runs and a tail -- and five runs and a tail: two spans per frame, the partial sums and k_bins_reduce
N_VALUES = [1, 11, 12, 13, 3071, 3072, 3073, 24575, 24576, 24577, 49157, 122893]
FRAME_COUNTS = [1, 3, 5]


def _two_spans(v, n):
    return _lib_().trpx_decode_bins_spans_per_frame(v, n) == 2


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("v", N_VALUES)
def test_exactness_matrix(dt, v):
    n = FRAME_COUNTS[(N_VALUES.index(v) + DTYPES.index(dt)) % 3]           # (every size with every count over the six types)
    sets = label_sets(v, seed=v)
    assert sorted({nb for _, _, nb in sets}) == [1, 2, 37, 4096]
    assert _two_spans(v, n) == (v == 122893)                # the reduce path is known to run there, and only there
    for what, px in (("mixed", mixed(dt, (n, v), seed=n * 1000 + v % 1000, zero_stretch=True)), ("ladder", ladder(dt, (n, v), seed=v))):
        if what == "ladder" and v >= 12 * 3 * 33:            # (three cycles of the widths 0 .. 32)
            ladder_holds_every_width(px)
        enc = encode(px)
        ws = _ws(enc, n)
        for name, lab, nb in sets:
            got = _check(enc, px, lab, nb, what=f"{what} / {name}", ws=ws)
            if name == "masked":
                assert not got.any()                        # (status 0 was asserted: the stack was still walked and validated)


@pytest.mark.parametrize("v", N_VALUES)
def test_every_frame_count_on_every_size(v):
    for n in FRAME_COUNTS:
        if v == 122893 and n in (1, 3):
            assert _two_spans(v, n)
        px = mixed(np.int16 if v % 2 else np.uint32, (n, v), seed=n, zero_stretch=True)
        enc = encode(px)
        for name, lab, nb in label_sets(v, seed=n):
            _check(enc, px, lab, nb, what=name)


def test_signed_extremes_into_one_bin():
    v = 3073
    for dt, pv in ((np.int32, -(1 << 31)), (np.uint32, 0xFFFFFFFF)):
        px = np.full((2, v), pv, dt)
        enc = encode(px)
        want = np.full((2, 1), v * pv, np.int64)
        assert np.array_equal(want, truth(px, np.zeros(v, np.uint16), 1))
        for mode in ("index", "offsets", "none"):
            _check(enc, px, np.zeros(v, np.uint16), 1, mode, what="extremes", want=want)


@pytest.mark.parametrize("dt", [np.uint16, np.int32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("v, n", [(49157, 5), (122893, 3)])
def test_input_forms_runs_and_sub_stacks_agree(dt, v, n):
    px = mixed(dt, (n, v), seed=17, zero_stretch=True)
    enc = encode(px)
    pairs = ((0, n), (1, n - 1), (n - 1, n), (1, 2))
    for name, lab, nb in [s for s in label_sets(v, seed=17) if s[0] in ("rings", "p % 37", "random4096")]:
        outs = [_check(enc, px, lab, nb, mode, what=f"forms / {name}") for mode in ("index", "offsets", "none")]
        outs.append(_check(enc, px, lab, nb, "index", what="second run"))
        for o in outs[1:]:
            assert o.tobytes() == outs[0].tobytes(), (dt, name)
        for a, b in pairs:                                  # frames [a, b) alone: frame_offsets + a, n_frames = b - a, no index
            sub = _check(enc, px[a:b], lab, nb, "offsets", what=f"frames [{a}, {b})", first=a, n_frames=b - a)
            assert sub.tobytes() == outs[0][a:b].tobytes()


def test_labels_at_two_four_and_eight_byte_alignment():
    """The map carved out of a larger tensor at addresses 2, 4 and 8 mod 16, labels of bin 0 around it (a read outside the map
    would change a sum): the label-by-label path and the 8-byte path."""
    n = 3
    for v in (3072 * 2, 3073):
        px = mixed(np.uint16, (n, v), seed=5, zero_stretch=True)
        enc = encode(px)
        for name, lab, nb in label_sets(v, seed=5):
            want = truth(px, lab, nb)
            for shift in (1, 2, 4):
                host = np.zeros(v + 16, np.uint16)
                host[shift: shift + v] = lab
                lab_dev = to_dev(host)[shift: shift + v]
                assert lab_dev.data_ptr() % 16 == 2 * shift
                _check(enc, px, lab, nb, what=f"shift {shift} / {name}", want=want, lab_dev=lab_dev)


@pytest.mark.parametrize("v", [13, 3073, 24577])
def test_labels_behind_the_map_are_never_read(v):
    """The map and a guard row of valid labels behind it in one allocation: the sums depend on the map alone -- a read behind
    labels[n_values) (the partial last block) would pick up the guard's labels of a bin."""
    n = 3
    px = mixed(np.uint16, (n, v), seed=v, zero_stretch=True)
    px[:, -1] = 65535
    enc = encode(px)
    for name, lab, nb in label_sets(v, seed=v):
        want = truth(px, lab, nb)
        for guard in (0, nb - 1):
            both = to_dev(np.concatenate([lab, np.full(v, guard, np.uint16)]))
            _check(enc, px, lab, nb, what=f"guard row {guard} / {name}", want=want, lab_dev=both)


def _group_bits(widths, n_values, lo, hi):
    """Bits of the blocks [lo, hi) of one frame under the layout rule (1 header bit where the width repeats, else 4 / 6 / 12)."""
    w = widths.astype(np.int64)
    prev = np.concatenate([[0], w[:-1]])
    hl = np.where(w == prev, 1, np.where(w < 7, 4, np.where(w < 10, 6, 12)))
    cnt = np.full(w.size, 12)
    cnt[-1] = n_values - 12 * (w.size - 1)
    return int((hl + cnt * w)[lo:hi].sum())


def test_masking_does_not_skip_validation():
    """Every label but those of one block is masked: the sums are exact on every form, and damage in the part of the stack no
    block is fetched from -- a width byte of the index, a frame-offset table whose end is short -- is still found."""
    n, v = 3, 7000
    px = mixed(np.uint16, (n, v), seed=31, zero_stretch=True)
    px[:, :12] = np.arange(1, 13)                           # (the one block the map sees holds something)
    enc = encode(px)
    lab = np.full(v, MASKED, np.uint16)
    lab[:12] = [0, 0, 1, 1, 1, 2, 2, 2, 2, 0, 3, 3]
    for mode in ("index", "offsets", "none"):
        _check(enc, px, lab, 4, mode, what="one block")
    groups, blocks = 3, 584                                 # ceil(7000 / 12), ceil(584 / 256)
    w_at = (8 * n * groups + 15) // 16 * 16                 # (the index: the group offsets, then the widths)
    widths = enc.index[w_at: w_at + n * blocks].cpu().numpy().reshape(n, blocks)
    for frame, block in ((1, 300), (0, 583), (2, 256)):     # blocks of groups 1 and 2, where every label is masked
        assert (lab[12 * block: 12 * block + 12] == MASKED).all()
        bent_w = widths[frame].astype(np.int64)
        bent_w[block] += 1 if bent_w[block] < 16 else -1
        lo, hi = block // 256 * 256, min(block // 256 * 256 + 256, blocks)
        assert _group_bits(bent_w, v, lo, hi) != _group_bits(widths[frame], v, lo, hi)   # (the fixture: the damage moves the group's end)
        bent = dataclasses.replace(enc, index=enc.index.clone())
        bent.index[w_at + frame * blocks + block] = int(bent_w[block])
        assert _bins(bent, px.dtype, lab, 4)[1] == CORRUPT, (frame, block)
    short = dataclasses.replace(enc, frame_offsets=enc.frame_offsets.clone())
    short.frame_offsets[-1] -= 1
    assert _bins(short, px.dtype, lab, 4)[1] == CORRUPT
    assert _bins(short, px.dtype, lab, 4, mode="offsets")[1] == CORRUPT
    masked = np.full(v, MASKED, np.uint16)
    assert _bins(enc, px.dtype, masked, 4)[1] == OK                              # (the intact stack under an all-masked map)
    assert _bins(short, px.dtype, masked, 4)[1] == CORRUPT                       # ... validated where nothing at all is fetched
    assert _bins(short, px.dtype, masked, 4, mode="offsets")[1] == CORRUPT


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
        for name, lab, nb in [s for s in label_sets(v, seed=3) if s[0] in ("rings", "p % 37", "random4096")]:
            want = truth(S.px, lab, nb)
            for mode in ("index", "offsets", "none"):
                if mode == "index" and not have_index:
                    continue
                got, status = _bins(enc, dtname, lab, nb, mode)
                ctx = (dtname, e["kind"], mode, name)
                assert status in (OK, CORRUPT), ctx
                assert status == CORRUPT or np.array_equal(got, want), ctx       # never status 0 with wrong sums
                if e["kind"] in ("K0", "K2"):
                    assert status == OK, ctx                                     # padded widths decode everywhere
                elif mode != "index":
                    assert status == CORRUPT, ctx                                # restated widths have no index


def test_graph_capture_replays_with_new_maps():
    from trpx_amd import codec
    import torch
    n, v, nb = 6, 511 * 513, 64
    px = mixed(np.uint16, (n, v), seed=9, zero_stretch=True)
    enc = encode(px)
    maps = [rings(v, nb, 513), (np.arange(v) % nb).astype(np.uint16), np.full(v, MASKED, np.uint16), rings(v, nb, 513, scale=1.5)]
    lab_dev = to_dev(maps[0])
    out = torch.zeros((n, nb), dtype=torch.int64, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")
    ws = codec.Workspace("cuda")
    stack = enc.stack()

    def call():
        codec.decode_bins(stack, enc.frame_offsets, v, n, torch.uint16, lab_dev, nb, index=enc.index, out=out, workspace=ws, status=status)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # warm-up outside the capture
        call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), truth(px, maps[0], nb))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                     # one stream, no parallel branches
        call()
    for lab in maps[1:]:
        lab_dev.view(torch.uint8).copy_(to_dev(lab).view(torch.uint8))           # the same buffer, a new map
        out.fill_(SENTINEL)
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status[0].item()) == OK
        assert np.array_equal(out.cpu().numpy(), truth(px, lab, nb))


def test_python_surfaces():
    from trpx_amd import codec
    from trpx_amd.terse import Terse
    import torch
    rng = np.random.default_rng(43)
    h, wd, nb = 20, 35, 8
    px = rng.integers(0, 3000, size=(3, h * wd)).astype(np.uint16)
    px[:, 100:240] = rng.integers(0, 65536, size=(3, 140))
    lab = rings(h * wd, nb, wd, scale=2.0)
    assert (lab == MASKED).any() and (lab == 0).any()
    want = truth(px, lab, nb)
    enc = encode(px)
    abi, status = _bins(enc, px.dtype, lab, nb)
    assert status == OK and np.array_equal(abi, want)
    # the device-resident wrapper, [n_values] and [H, W], uint16 and int16-viewed
    for shape in ((h * wd,), (h, wd)):
        for view in (torch.uint16, torch.int16):
            bins, st = codec.decode_bins(enc.stack(), enc.frame_offsets, h * wd, 3, torch.uint16, to_dev(lab.reshape(shape)).view(view), nb, index=enc.index)
            torch.cuda.synchronize()
            assert int(st[0].item()) == OK and bins.dtype == torch.int64 and tuple(bins.shape) == (3, nb)
            assert np.array_equal(bins.cpu().numpy(), abi)
    bins, st = codec.decode_bins(enc.stack(), None, h * wd, 3, torch.uint16, to_dev(lab), nb)      # frames located, index built
    assert int(st[0].item()) == OK and np.array_equal(bins.cpu().numpy(), abi)
    assert codec.decode_bins_workspace_bytes(enc.stack().numel(), h * wd, 3, torch.uint16, nb) > 0
    with pytest.raises(TypeError):
        codec.decode_bins(enc.stack(), enc.frame_offsets, h * wd, 3, torch.uint16, torch.from_numpy(lab.astype(np.int32)).cuda(), nb)
    with pytest.raises(ValueError):
        codec.decode_bins(enc.stack(), enc.frame_offsets, h * wd, 3, torch.uint16, to_dev(lab[:-1]), nb)
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            codec.decode_bins(enc.stack(), enc.frame_offsets, h * wd, 3, torch.uint16, to_dev(lab), bad)
    # the host class
    t = Terse()
    t.push_back_stack(px)
    for shape in ((h * wd,), (h, wd)):
        got = t.prolix_bins(lab.reshape(shape), nb)
        assert got.dtype == np.int64 and got.shape == (3, nb) and np.array_equal(got, abi)
    assert np.array_equal(t.prolix_bins(lab.astype(np.int64), nb), abi)
    with pytest.raises(ValueError):
        t.prolix_bins(np.zeros(5, np.uint16), nb)
    with pytest.raises(ValueError):
        t.prolix_bins(lab, 4097)
    with pytest.raises(TypeError):
        t.prolix_bins(np.zeros(h * wd, np.float32), nb)
    with pytest.raises(TypeError):
        t.prolix_bins(np.full(h * wd, 70000), nb)


def test_cpp_class_prolix_bins():
    exe = os.path.join(ROOT, "tests", "cpp", "bins_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "bins_example.mk", "bins_example"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK bins example" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("nb", [1, 2, 16])
def test_agrees_with_decode_dot_on_one_hot_maps(nb):
    """For up to 16 bins the sibling computes the same numbers from one one-hot map per bin."""
    from trpx_amd import codec
    import torch
    n, v = 3, 24577
    px = mixed(np.int16, (n, v), seed=nb, zero_stretch=True)
    enc = encode(px)
    lab = rings(v, nb)
    one_hot = np.stack([(lab == b) for b in range(nb)]).astype(np.int32)
    dots, st = codec.decode_dot(enc.stack(), enc.frame_offsets, v, n, torch.int16, torch.from_numpy(one_hot).cuda(), index=enc.index)
    torch.cuda.synchronize()
    assert int(st[0].item()) == OK
    got = _check(enc, px, lab, nb, what="one-hot")
    assert np.array_equal(got, dots.cpu().numpy())


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_faster_than_decoding_and_scattering():
    """500 x 512^2 u16 synth-v1 with the encoder's index, resident; a radial map of 256 bins over the 512 x 512 frame, the corners
    masked.  The baseline is what a caller pays without this entry point: trpx_decode_indexed of the stack, then index_add_ on
    int64, the exact integer scatter torch offers on the GPU -- in the same process, repetitions interleaved, medians.  No
    margin: the call must only be no slower than the route it replaces."""
    from trpx_amd import codec
    import torch
    n, side, nb = 500, 512, 256
    v = side * side
    px = codec.synth(np.uint16, 0, n, v)
    enc = codec.encode(px, index=True)
    enc.check()
    lab = rings(v, nb, side, scale=1.0)
    assert (lab == MASKED).any() and (lab == nb - 1).any()
    lab_dev = to_dev(lab)
    keep = torch.from_numpy(np.flatnonzero(lab < nb)).cuda()
    idx = torch.from_numpy(lab[lab < nb].astype(np.int64)).cuda()
    stack = enc.stack()
    pix = torch.empty((n, v), dtype=torch.uint16, device="cuda")
    st = torch.empty(8, dtype=torch.int32, device="cuda")
    out = torch.empty((n, nb), dtype=torch.int64, device="cuda")
    ws = codec.Workspace("cuda")
    base = [None]

    def bins():
        codec.decode_bins(stack, enc.frame_offsets, v, n, torch.uint16, lab_dev, nb, index=enc.index, out=out, workspace=ws, status=st)

    def replaced():
        codec.decode(stack, enc.frame_offsets, v, n, torch.uint16, out=pix, status=st, index=enc.index)
        p64 = pix.to(torch.int64)
        base[0] = torch.zeros((n, nb), dtype=torch.int64, device="cuda").index_add_(1, idx, p64[:, keep])

    for _ in range(2):
        bins()
        replaced()
    torch.cuda.synchronize()
    t_bins, t_old = [], []
    for _ in range(9):
        t_bins.append(_event_ms(bins))
        t_old.append(_event_ms(replaced))
    assert int(st[0].item()) == OK
    assert torch.equal(pix.view(torch.int16), px.view(torch.int16))
    assert torch.equal(out, base[0])                        # the two routes agree, value for value
    m_bins, m_old = statistics.median(t_bins), statistics.median(t_old)
    print(f"\n500 x 512^2 u16 synth-v1, 256 radial bins, corners masked: decode_bins {m_bins:.4f} ms, decode_indexed + int64 index_add_ "
          f"{m_old:.4f} ms, ratio {m_old / m_bins:.2f}")
    assert m_bins <= m_old, (m_bins, m_old)
