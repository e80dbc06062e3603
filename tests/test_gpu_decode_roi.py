"""GPU tests: trpx_decode_roi (decode_roi.hip).  The truth is the numpy crop of the ORIGINAL pixels,
compared byte for byte: the codec is lossless, so no decoder is trusted."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import Guarded, encode, events_median, input_forms, mixed, to_np, torch_dt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def truth(px, boxes, bh, bw):
    return np.stack([px[f, y:y + bh, x:x + bw] for f, y, x in boxes])


def _boxes_dev(boxes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(boxes, dtype=np.int64).reshape(-1, 3).astype(np.int32))).cuda()


def _roi(enc, px, boxes, bh, bw, mode="index", first=0, n_frames=None):
    """Decodes into the middle of a guarded allocation; returns (pixels, status word 0) after checking the guards."""
    from trpx_amd import codec
    import torch
    guarded = Guarded(len(boxes) * bh * bw, px.dtype, 0x5A)
    offs, index = input_forms(enc, mode, first)
    n_frames = enc.n_frames - first if n_frames is None else n_frames
    got, st = codec.decode_roi(enc.stack(), offs, enc.n_values, n_frames, torch_dt(px.dtype), px.shape[2], _boxes_dev(boxes), (bh, bw),
                               index=index, out=guarded.view.view(len(boxes), bh, bw))
    torch.cuda.synchronize()
    guarded.check("pixels_out")
    return to_np(got), int(st[0].item())


def _check(enc, px, boxes, bh, bw, mode="index", what=""):
    got, code = _roi(enc, px, boxes, bh, bw, mode)
    assert code == 0, (what, mode, px.dtype, px.shape)
    want = truth(px, boxes, bh, bw)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (what, mode, px.dtype, px.shape, bh, bw)


def box_sets(shape, seed=1):
    """The issue's boxes for a stack of `shape`: (what, box_h, box_w, [(frame, y0, x0), ...]), one call per entry."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    frames = list(range(n))
    sets = [("corners", 1, 1, [(f, y, x) for f in frames for y in (0, h - 1) for x in (0, w - 1)]),
            ("whole frame", h, w, [(f, 0, 0) for f in reversed(frames)]),
            ("full row", 1, w, [(f, y, 0) for f in frames for y in sorted({0, h // 2, h - 1})]),
            ("full column", h, 1, [(f, 0, x) for f in frames for x in sorted({0, w // 2, w - 1})])]
    th, tw = min(h, 3), min(w, 5)
    sets.append(("ends in the last pixel", th, tw, [(f, h - th, w - tw) for f in frames]))
    # rows that start inside a block and end inside one; where the frame has more than one group, a row segment of the box
    # crosses the first group seam (pixel 3072) so that it starts in one group and ends in the next
    mh, mw = max(1, 3 * h // 5), max(2, w // 2) if w > 1 else 1
    y0, x0 = (h - mh) // 2, min(w - mw, 7)
    if h * w > 3072:
        ys, xs = divmod(3072, w)                            # the seam's row and column
        mw = min(mw, 200)
        x0 = min(max(xs - mw // 2, 0), w - mw)
        if x0 % 12 == 0 and 0 < x0 < w - mw:
            x0 += 5
        y0 = min(max(ys - mh // 2, 0), h - mh)
        assert y0 <= ys < y0 + mh and (xs == 0 or x0 < xs < x0 + mw)
    sets.append(("mid-block rows", mh, mw, [(f, y0, x0) for f in frames]))
    rh, rw = min(h, 5), min(w, 9)
    rnd = [(int(rng.integers(n)), int(rng.integers(h - rh + 1)), int(rng.integers(w - rw + 1))) for _ in range(170)]
    rnd += rnd[:20] + [(f, y, min(w - rw, x + 2)) for f, y, x in rnd[:10]]     # repeated and overlapping entries
    order = rng.permutation(len(rnd))                                         # shuffled frame order
    sets.append(("200 random", rh, rw, [rnd[i] for i in order]))
    assert len(sets[-1][3]) == 200
    return sets


# frames x height x width: the smallest at which each mechanism can fail
SHAPES = [(3, 70, 100),     # 7000 pixels: three groups, the last one short, blocks straddle rows
          (4, 29, 37),      # 1073 = 89 * 12 + 5: a short last block, frames that start at odd bytes
          (2, 300, 5),      # rows shorter than a block: many rows per block
          (2, 3, 4000),     # a row longer than a group: units with no box pixels
          (2, 1, 7),        # a frame smaller than a block
          (5, 511, 513)]    # the project's odd-size case, 86 groups


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exactness_matrix(dt, shape):
    px = mixed(dt, shape, seed=shape[0] * 1000 + shape[1])
    enc = encode(px)
    for what, bh, bw, boxes in box_sets(shape):
        _check(enc, px, boxes, bh, bw, what=what)


@pytest.mark.parametrize("dt", [np.uint16, np.int32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(3, 70, 100), (5, 511, 513)], ids=lambda s: "x".join(map(str, s)))
def test_input_forms_agree(dt, shape):
    px = mixed(dt, shape, seed=17)
    enc = encode(px)
    for what, bh, bw, boxes in box_sets(shape, seed=2):
        outs = []
        for mode in ("index", "offsets", "none"):
            got, code = _roi(enc, px, boxes, bh, bw, mode)
            assert code == 0, (what, mode)
            outs.append(got)
        assert np.array_equal(outs[0].view(np.uint8), truth(px, boxes, bh, bw).view(np.uint8)), what
        assert all(np.array_equal(outs[0].view(np.uint8), o.view(np.uint8)) for o in outs[1:]), what


def test_sub_stack():
    """Frames [a, b) alone: frame_offsets + a, n_frames = b - a, no index; box frame numbers are relative to a."""
    shape = (9, 70, 100)
    px = mixed(np.int16, shape, seed=11)
    enc = encode(px)
    rng = np.random.default_rng(5)
    for a, b in ((0, 9), (2, 7), (8, 9), (3, 4)):
        boxes = [(int(rng.integers(b - a)), int(rng.integers(70 - 20 + 1)), int(rng.integers(100 - 33 + 1))) for _ in range(40)]
        got, code = _roi(enc, px, boxes, 20, 33, mode="offsets", first=a, n_frames=b - a)
        assert code == 0, (a, b)
        assert np.array_equal(got, truth(px[a:b], boxes, 20, 33)), (a, b)


@pytest.mark.parametrize("kind", ["synth", "poisson", "blank", "extremes"])
def test_data_kinds(kind):
    from trpx_amd import codec, workloads
    n, h, w = 17, 511, 513
    v = h * w
    dt = np.uint16
    if kind == "synth":
        px = to_np(codec.synth(np.uint16, 0, n, v))
    elif kind == "poisson":
        px = workloads.poisson_u16_np(3.0, 0, n, v).astype(dt)
    elif kind == "blank":
        px = np.zeros((n, v), dt)
    else:
        info = np.iinfo(dt)
        px = np.where((np.arange(v) % 2 == 0)[None, :], info.max, info.min).astype(dt).repeat(n, axis=0).reshape(n, v)
    px = np.ascontiguousarray(px).reshape(n, h, w)
    enc = encode(px)
    rng = np.random.default_rng(23)
    boxes = [(int(rng.integers(n)), int(rng.integers(h - 32 + 1)), int(rng.integers(w - 48 + 1))) for _ in range(50)]
    _check(enc, px, boxes, 32, 48, what=kind)
    _check(enc, px, boxes, 32, 48, mode="offsets", what=kind)


def test_large_int32_frames():
    """Two 4096^2 int32 frames: the index comes from the large-frame walk.  Boxes on the seams of the 256-block groups (every
    3072 pixels: three quarters of a row) and of the walk's parts (16384 blocks: 48 rows)."""
    rng = np.random.default_rng(7)
    h = w = 4096
    px = (rng.poisson(3.0, size=(2, h, w)) - 1).astype(np.int32)
    px[1, : h // 3] = rng.integers(-(1 << 31), (1 << 31) - 1, size=(h // 3, w), dtype=np.int64).astype(np.int32)
    enc = encode(px)
    boxes = [(f, y, x) for f in (0, 1) for y in (0, 48 - 64 + 48, 48 * 20 - 64, 48 * 43 - 127, h - 128)
             for x in (0, 3072 - 64, w - 128)]
    boxes += [(int(rng.integers(2)), int(rng.integers(h - 127)), int(rng.integers(w - 127))) for _ in range(64 - len(boxes))]
    assert len(boxes) == 64
    for mode in ("index", "offsets", "none"):
        _check(enc, px, boxes, 128, 128, mode=mode, what="large frames")


def test_bad_boxes_are_reported_and_the_others_are_exact():
    shape = (3, 70, 100)
    px = mixed(np.uint16, shape, seed=29)
    enc = encode(px)
    bh, bw = 9, 14
    rng = np.random.default_rng(3)
    good = [(int(rng.integers(3)), int(rng.integers(70 - bh + 1)), int(rng.integers(100 - bw + 1))) for _ in range(30)]
    boxes = good[:10] + [(3, 0, 0)] + good[10:20] + [(1, 5, 100 + 1 - bw)] + good[20:]   # frame == n_frames; x0 + box_w == width + 1
    for mode in ("index", "offsets"):
        got, code = _roi(enc, px, boxes, bh, bw, mode)      # (the guards are checked in there)
        assert code == 1, mode                              # TRPX_ERR_INVALID_ARG
        keep = [i for i in range(len(boxes)) if i not in (10, 21)]
        assert np.array_equal(got[keep], truth(px, good, bh, bw)), mode


def test_corrupt_index_and_short_offsets_are_rejected():
    """Inconsistent inputs the kernel has to reject by its own checks: a group offset that is off by 12 bits, a frame-offset
    table whose end is short.  Status CORRUPT, nothing written outside pixels_out."""
    from trpx_amd import codec
    import torch
    shape = (3, 70, 100)
    px = mixed(np.uint16, shape, seed=31)
    enc = encode(px)
    groups = 3                                              # ceil(ceil(7000 / 12) / 256)
    boxes = [(f, 0, 0) for f in range(3)]                   # whole frames: every group is touched
    got, code = _roi(enc, px, boxes, 70, 100)
    assert code == 0 and np.array_equal(got, px)

    bent = dataclasses.replace(enc, index=enc.index.clone())
    bent.index[: 8 * 3 * groups].view(torch.int64)[1 * groups + 1] += 12      # frame 1, group 1 (the index starts with the group offsets)
    _, code = _roi(bent, px, boxes, 70, 100)
    assert code == 5
    _, code = _roi(bent, px, [(0, 0, 0), (2, 60, 90)], 10, 10)              # boxes that do not touch the bent group
    assert code == 0

    short = dataclasses.replace(enc, frame_offsets=enc.frame_offsets.clone())
    short.frame_offsets[-1] -= 1
    _, code = _roi(short, px, boxes, 70, 100)
    assert code == 5
    _, code = _roi(short, px, [(2, 60, 90)], 10, 10)                         # the last group of the last frame alone
    assert code == 5


def test_graph_capture_replays_with_new_boxes():
    from trpx_amd import codec
    import torch
    shape = (6, 511, 513)
    px = mixed(np.uint16, shape, seed=9)
    enc = encode(px)
    stack = enc.stack()
    rng = np.random.default_rng(41)
    bh, bw, nb = 24, 40, 60
    lists = [[(int(rng.integers(6)), int(rng.integers(511 - bh + 1)), int(rng.integers(513 - bw + 1))) for _ in range(nb)]
             for _ in range(3)]
    boxes = _boxes_dev(lists[0])
    out = torch.zeros((nb, bh, bw), dtype=torch.uint16, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")

    def call():
        codec.decode_roi(stack, enc.frame_offsets, enc.n_values, enc.n_frames, torch.uint16, 513, boxes, (bh, bw), index=enc.index,
                         out=out, status=status)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # warm-up outside the capture
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for lst in lists[1:]:
        boxes.copy_(_boxes_dev(lst))
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status[0].item()) == 0
        assert np.array_equal(to_np(out), truth(px, lst, bh, bw))


def test_python_host_surface():
    from trpx_amd.terse import Terse
    rng = np.random.default_rng(43)
    px = rng.integers(0, 3000, size=(3, 20, 35)).astype(np.uint16)           # 3 frames of 35 x 20 (width x height)
    px[:, 5:9] = rng.integers(0, 65536, size=(3, 4, 35))
    t = Terse()
    t.push_back_stack(px.reshape(3, -1))
    with pytest.raises(ValueError):
        t.prolix_roi(2, 3, 4, 5)                            # dim() never set
    t.dim([35, 20])
    got = t.prolix_roi(2, 3, 11, 17)
    assert got.dtype == np.uint16 and np.array_equal(got, px[:, 2:13, 3:20])
    assert np.array_equal(t.prolix_roi(16, 30, 4, 5, frames=[2, 0]), px[[2, 0], 16:20, 30:35])
    boxes = [(2, 0, 0), (0, 13, 28), (1, 7, 9), (2, 0, 0), (1, 8, 10)]
    assert np.array_equal(t.prolix_boxes(boxes, (7, 7)), truth(px, boxes, 7, 7))
    with pytest.raises(ValueError):
        t.prolix_boxes([(0, 14, 0)], (7, 7))                # y0 + h > height
    with pytest.raises(ValueError):
        t.prolix_boxes([(3, 0, 0)], (7, 7))                 # frame == number_of_frames
    one_d = Terse()
    one_d.push_back_stack(px.reshape(3, -1))
    one_d.dim([700])
    with pytest.raises(ValueError):
        one_d.prolix_roi(0, 0, 1, 1)                        # not 2-D


def test_cpp_class_prolix_roi():
    exe = os.path.join(ROOT, "tests", "cpp", "roi_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "roi_example.mk"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK roi example" in r.stdout, r.stdout + r.stderr


def test_faster_than_decoding_everything():
    """2000 x 512^2 u16 synth-v1 with the encoder's index, resident; one 64 x 64 box per frame.  The baseline is what a caller
    has to run without this entry point, before any cropping: trpx_decode_indexed of the same stack, in the same process."""
    from trpx_amd import codec
    import torch
    n, h, w = 2000, 512, 512
    v = h * w
    px = codec.synth(np.uint16, 0, n, v)
    enc = codec.encode(px, index=True)
    enc.check()
    del px
    torch.cuda.synchronize()
    stack = enc.stack()
    rng = np.random.default_rng(47)
    boxes = _boxes_dev([(f, int(rng.integers(h - 63)), int(rng.integers(w - 63))) for f in range(n)])
    pix = torch.empty((n, v), dtype=torch.uint16, device="cuda")
    out = torch.empty((n, 64, 64), dtype=torch.uint16, device="cuda")
    st = torch.empty(8, dtype=torch.int32, device="cuda")
    t_full = events_median(lambda: codec.decode(stack, enc.frame_offsets, v, n, torch.uint16, out=pix, status=st, index=enc.index), 20)
    assert int(st[0].item()) == 0
    t_roi = events_median(lambda: codec.decode_roi(stack, enc.frame_offsets, v, n, torch.uint16, w, boxes, (64, 64), index=enc.index,
                                                   out=out, status=st), 20)
    assert int(st[0].item()) == 0
    b = boxes.cpu().numpy()
    rows = torch.from_numpy(b[:, 1].astype(np.int64)).cuda()[:, None] + torch.arange(64, device="cuda")[None, :]
    cols = torch.from_numpy(b[:, 2].astype(np.int64)).cuda()[:, None] + torch.arange(64, device="cuda")[None, :]
    want = pix.view(torch.int16).view(n, h, w)[torch.arange(n, device="cuda")[:, None, None], rows[:, :, None], cols[:, None, :]]
    assert torch.equal(out.view(torch.int16), want)
    print(f"\n2000 x 512^2 u16 synth, one 64 x 64 box per frame: decode_indexed {t_full:.4f} ms, decode_roi {t_roi:.4f} ms, "
          f"ratio {t_roi / t_full:.3f}")
    assert t_roi < t_full, (t_roi, t_full)
