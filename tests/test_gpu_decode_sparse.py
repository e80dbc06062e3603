"""GPU tests: trpx_decode_sparse (decode_sparse.hip).  The truth is numpy on the ORIGINAL pixels,
compared byte for byte: the codec is lossless, so no decoder is trusted.  Every output sits in the middle of a guarded
allocation, 64 sentinel elements on either side of row_offsets, positions and values."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import CAPACITY, CORRUPT, OK, Guarded, encode, events_median, input_forms, ladder, ladder_holds_every_width, mixed
from gpu_support import sparse_truth as truth
from gpu_support import status_block, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_SENTINEL, POS_SENTINEL, VAL_SENTINEL = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A


def thresholds(dt):
    info = np.iinfo(dt)
    lo, hi, bits = int(info.min), int(info.max), info.bits
    ts = [lo, lo + 1, 0, 1, hi, hi + 1]
    for k in (1, 3, 7, bits - 1):
        ts += [(1 << k) - 1, 1 << k, (1 << k) + 1]
        if lo < 0:
            ts.append(-(1 << k))
    if lo < 0:
        ts.append(-1)
    return sorted({min(max(t, lo), hi + 1) for t in ts})


def _ws(enc, n_frames):
    from trpx_amd import codec
    import torch
    need = codec.decode_sparse_workspace_bytes(enc.data.numel(), enc.n_values, n_frames, enc.dtype)
    return torch.empty(need, dtype=torch.uint8, device="cuda")


def _sparse(enc, dt, t, mode="index", capacity=0, null_outputs=False, first=0, n_frames=None, ws=None):
    """One trpx_decode_sparse call into guarded allocations; returns (row_offsets, positions, values, status word 0) on the
    host after checking the guards and that nothing at or beyond `capacity` was touched."""
    from trpx_amd import _lib
    from trpx_amd.codec import dtype_code
    import torch
    dt = np.dtype(dt)
    n_frames = enc.n_frames - first if n_frames is None else n_frames
    rows = Guarded(n_frames + 1, np.int64, ROW_SENTINEL)
    pos, val = Guarded(capacity, np.uint32, POS_SENTINEL), Guarded(capacity, dt, VAL_SENTINEL)
    status = status_block()
    ws = _ws(enc, n_frames) if ws is None else ws
    stack = enc.stack()
    offs, index = input_forms(enc, mode, first)
    rc = _lib.lib().trpx_decode_sparse(dtype_code(dt), stack.data_ptr(), stack.numel(), offs.data_ptr() if offs is not None else None,
                                       index.data_ptr() if index is not None else None, enc.n_values, n_frames, 12, int(t),
                                       rows.view.data_ptr(), None if null_outputs else pos.view.data_ptr(),
                                       None if null_outputs else val.view.data_ptr(), capacity, status.data_ptr(), ws.data_ptr(),
                                       ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().trpx_last_error_string()
    torch.cuda.synchronize()
    untouched = 0 if null_outputs else None
    return (rows.check("row_offsets"), pos.check("positions", untouched), val.check("values", untouched), int(status[0].item()))


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _check(enc, px, t, mode="index", what="", **kw):
    rows, pos, val = truth(px, t)
    total = int(rows[-1])
    got = _sparse(enc, px.dtype, t, mode, capacity=total, null_outputs=total == 0, **kw)
    ctx = (what, mode, px.dtype, px.shape, t, total)
    assert got[3] == OK, ctx
    assert np.array_equal(got[0], rows), ctx
    assert _same(got[1], pos) and _same(got[2], val), ctx
    return got


# frames x values: the smallest at which each mechanism can fail
SHAPES = [(3, 7000),        # three groups, the last one short
          (4, 1073),        # 89 * 12 + 5: a short last block, frames that start at odd bytes
          (2, 7),           # a frame smaller than a block
          (3, 3072),        # exactly one group
          (2, 3073),        # one value into the second group
          (5, 511 * 513)]   # 86 groups, the project's odd size


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exactness_matrix(dt, shape):
    for what, px in (("mixed", mixed(dt, shape, seed=shape[0] * 1000 + shape[1] % 1000)), ("ladder", ladder(dt, shape, seed=shape[1]))):
        if what == "ladder" and shape[1] >= 12 * 3 * 33:     # (three cycles of the widths 0 .. 32)
            ladder_holds_every_width(px)
        enc = encode(px)
        ws = _ws(enc, enc.n_frames)
        for t in thresholds(dt):
            _check(enc, px, t, what=what, ws=ws)


def test_capacity():
    shape = (3, 7000)
    px = mixed(np.uint16, shape, seed=3)
    enc = encode(px)
    t = 2
    rows, pos, val = truth(px, t)
    total = int(rows[-1])
    assert total > 100
    r, _, _, code = _sparse(enc, px.dtype, t, capacity=total - 1)            # (the guards are checked in there)
    assert code == CAPACITY and np.array_equal(r, rows)
    r, _, _, code = _sparse(enc, px.dtype, t, capacity=0, null_outputs=True)  # sizes only
    assert code == CAPACITY and np.array_equal(r, rows)
    r, p, v, code = _sparse(enc, px.dtype, t, capacity=total + 5)
    assert code == OK and np.array_equal(r, rows)
    assert _same(p[:total], pos) and _same(v[:total], val)
    assert (p[total:] == POS_SENTINEL).all() and (v[total:] == np.full(1, VAL_SENTINEL, px.dtype)[0]).all()   # the surplus is untouched


@pytest.mark.parametrize("dt", [np.uint16, np.int32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(3, 7000), (5, 511 * 513)], ids=lambda s: "x".join(map(str, s)))
def test_input_forms_agree(dt, shape):
    px = mixed(dt, shape, seed=17)
    enc = encode(px)
    for t in (1, 1 << 7):
        outs = [_check(enc, px, t, mode, what="forms") for mode in ("index", "offsets", "none")]
        outs.append(_check(enc, px, t, "index", what="second run"))
        for o in outs[1:]:
            assert all(_same(a, b) for a, b in zip(outs[0][:3], o[:3])), (dt, shape, t)


def test_sub_stack():
    """Frames [a, b) alone: frame_offsets + a, n_frames = b - a, no index."""
    px = mixed(np.int16, (9, 7000), seed=11)
    enc = encode(px)
    for a, b in ((0, 9), (2, 7), (8, 9), (3, 4)):
        _check(enc, px[a:b], 3, "offsets", what=f"frames [{a}, {b})", first=a, n_frames=b - a)


@pytest.mark.parametrize("kind", ["synth", "poisson", "blank", "extremes"])
def test_data_kinds(kind):
    from trpx_amd import codec, workloads
    n, v = 17, 511 * 513
    dt = np.uint16
    info = np.iinfo(dt)
    if kind == "synth":
        px, ts = to_np(codec.synth(np.uint16, 0, n, v)), [64]
    elif kind == "poisson":
        px, ts = workloads.poisson_u16_np(3.0, 0, n, v).astype(dt), [8]
    elif kind == "blank":
        px, ts = np.zeros((n, v), dt), [0, 1]                                 # all pixels (width-0 blocks report their zeros), none
    else:
        px, ts = np.where((np.arange(v) % 2 == 0)[None, :], info.max, info.min).astype(dt).repeat(n, axis=0).reshape(n, v), [info.max]
    px = np.ascontiguousarray(px)
    enc = encode(px)
    for t in ts:
        _check(enc, px, t, what=kind)


def test_large_int32_frames():
    """Two 4096^2 int32 frames (the data of test_gpu_decode_roi.test_large_int32_frames): the index comes from the large-frame walk."""
    rng = np.random.default_rng(7)
    h = w = 4096
    px = (rng.poisson(3.0, size=(2, h, w)) - 1).astype(np.int32)
    px[1, : h // 3] = rng.integers(-(1 << 31), (1 << 31) - 1, size=(h // 3, w), dtype=np.int64).astype(np.int32)
    px = px.reshape(2, -1)
    enc = encode(px)
    for mode in ("index", "offsets", "none"):
        _check(enc, px, 1 << 30, mode, what="large frames")


def test_corrupt_index_and_short_offsets_are_rejected():
    """The whole stack is validated: a group offset that is off by 12 bits is found whichever group it is, and so is a
    frame-offset table whose end is short.  Status CORRUPT, nothing written outside the outputs (checked in _sparse)."""
    import torch
    shape = (3, 7000)
    px = mixed(np.uint16, shape, seed=31)
    enc = encode(px)
    groups = 3                                              # ceil(ceil(7000 / 12) / 256)
    rows, _, _ = truth(px, 2)
    total = int(rows[-1])
    _check(enc, px, 2)
    for g in range(3 * groups):
        bent = dataclasses.replace(enc, index=enc.index.clone())
        bent.index[: 8 * 3 * groups].view(torch.int64)[g] += 12               # (the index starts with the group offsets)
        assert _sparse(bent, px.dtype, 2, capacity=total)[3] == CORRUPT, g
        assert _sparse(bent, px.dtype, 2, capacity=total // 2)[3] == CORRUPT, g   # CORRUPT wins over CAPACITY
    short = dataclasses.replace(enc, frame_offsets=enc.frame_offsets.clone())
    short.frame_offsets[-1] -= 1
    assert _sparse(short, px.dtype, 2, capacity=total)[3] == CORRUPT
    assert _sparse(short, px.dtype, 2, mode="offsets", capacity=total)[3] == CORRUPT


def test_graph_capture_replays_with_new_stacks():
    from trpx_amd import codec
    import torch
    shape = (6, 511 * 513)
    t = 3
    stacks = [mixed(np.uint16, shape, seed=s) for s in (9, 10, 12)]
    encs = [encode(px) for px in stacks]
    truths = [truth(px, t) for px in stacks]
    capacity = max(int(tr[0][-1]) for tr in truths) + 7
    data, offs, index = encs[0].data.clone(), encs[0].frame_offsets.clone(), encs[0].index.clone()   # (capacity-sized: one geometry)
    rows = torch.zeros(shape[0] + 1, dtype=torch.int64, device="cuda")
    pos = torch.zeros(capacity, dtype=torch.uint32, device="cuda")
    val = torch.zeros(capacity, dtype=torch.uint16, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")
    ws = codec.Workspace("cuda")

    def call():
        codec.decode_sparse(data, offs, shape[1], shape[0], torch.uint16, t, index=index, capacity=capacity, row_offsets=rows,
                            positions=pos, values=val, workspace=ws, status=status)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # warm-up outside the capture
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for enc, (r, p, v) in zip(encs[1:], truths[1:]):
        data.copy_(enc.data)
        offs.copy_(enc.frame_offsets)
        index.copy_(enc.index)
        rows.zero_(); pos.zero_(); val.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        total = int(r[-1])
        assert int(status[0].item()) == OK
        assert np.array_equal(rows.cpu().numpy(), r)
        assert _same(to_np(pos)[:total], p) and _same(to_np(val)[:total], v)


def test_python_surfaces():
    from trpx_amd import codec
    from trpx_amd.terse import Terse
    import torch
    rng = np.random.default_rng(43)
    px = rng.integers(0, 3000, size=(3, 700)).astype(np.uint16)
    px[:, 100:240] = rng.integers(0, 65536, size=(3, 140))
    t = Terse()
    t.push_back_stack(px)
    r, p, v = t.prolix_sparse(2500)
    tr = truth(px, 2500)
    assert r.dtype == np.int64 and p.dtype == np.uint32 and v.dtype == np.uint16
    assert np.array_equal(r, tr[0]) and _same(p, tr[1]) and _same(v, tr[2])
    r, p, v = t.prolix_sparse(2500, frames=[2, 0])
    tr = truth(px[[2, 0]], 2500)
    assert np.array_equal(r, tr[0]) and _same(p, tr[1]) and _same(v, tr[2])
    r, p, v = t.prolix_sparse(1 << 20)                      # above the type's range: no events
    assert np.array_equal(r, np.zeros(4, np.int64)) and p.size == 0 and v.size == 0 and v.dtype == np.uint16
    r, p, v = t.prolix_sparse(-7)                           # below it: every pixel
    assert np.array_equal(p, np.tile(np.arange(700, dtype=np.uint32), 3)) and _same(v, px.reshape(-1))
    with pytest.raises(ValueError):
        t.prolix_sparse(1, frames=[3])
    # the device-resident wrapper, sizing its outputs itself (synchronises)
    enc = encode(px)
    r, p, v, st = codec.decode_sparse(enc.stack(), enc.frame_offsets, 700, 3, torch.uint16, 2500, index=enc.index)
    tr = truth(px, 2500)
    assert int(st[0].item()) == OK and p.numel() == int(tr[0][-1])
    assert np.array_equal(r.cpu().numpy(), tr[0]) and _same(to_np(p), tr[1]) and _same(to_np(v), tr[2])
    r, p, v, st = codec.decode_sparse(enc.stack(), None, 700, 3, torch.uint16, 70000)
    assert int(st[0].item()) == OK and p.numel() == 0 and v.numel() == 0 and int(r[-1].item()) == 0


def test_cpp_class_prolix_sparse():
    exe = os.path.join(ROOT, "tests", "cpp", "sparse_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "sparse_example.mk"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK sparse example" in r.stdout, r.stdout + r.stderr


def test_faster_than_decoding_and_compacting():
    """2000 x 512^2 u16 Poisson(3) with the encoder's index, resident, threshold 8.  The baseline is what a caller pays without
    this entry point: trpx_decode_indexed of the stack, then torch.nonzero(pix >= 8) and the gather of the values on the decoded
    tensor -- in the same process, so no margin is needed."""
    from trpx_amd import codec, workloads
    import torch
    n, v, t = 2000, 512 * 512, 8
    px = workloads.poisson_u16(3.0, 0, n, v)
    enc = codec.encode(px, index=True)
    enc.check()
    del px
    torch.cuda.synchronize()
    stack = enc.stack()
    pix = torch.empty((n, v), dtype=torch.uint16, device="cuda")
    st = torch.empty(8, dtype=torch.int32, device="cuda")
    ws = codec.Workspace("cuda")
    t_decode = events_median(lambda: codec.decode(stack, enc.frame_offsets, v, n, torch.uint16, out=pix, status=st, index=enc.index), 20)
    assert int(st[0].item()) == OK
    p16 = pix.view(torch.int16)                             # (values stay below 4096: the signed view compares alike)
    assert int(p16.max().item()) < 4096
    total = int((p16 >= t).sum().item())
    rows = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    pos = torch.empty(total, dtype=torch.uint32, device="cuda")
    val = torch.empty(total, dtype=torch.uint16, device="cuda")

    def sparse():
        codec.decode_sparse(stack, enc.frame_offsets, v, n, torch.uint16, t, index=enc.index, capacity=total, row_offsets=rows,
                            positions=pos, values=val, workspace=ws, status=st)
    t_sparse = events_median(sparse, 20)
    assert int(st[0].item()) == OK
    assert int(rows[-1].item()) == total

    def compact():
        nz = torch.nonzero(p16 >= t)
        return nz, p16[nz[:, 0], nz[:, 1]]
    t_compact = events_median(compact, 20)
    nz, vals = compact()
    assert torch.equal(pos.view(torch.int32).to(torch.int64), nz[:, 1])
    assert torch.equal(val.view(torch.int16), vals)
    assert torch.equal(rows[1:], torch.cumsum(torch.bincount(nz[:, 0], minlength=n), 0))
    print(f"\n2000 x 512^2 u16 Poisson(3), t = 8, {total} events: decode_sparse {t_sparse:.4f} ms, decode_indexed {t_decode:.4f} ms, "
          f"nonzero + gather {t_compact:.4f} ms, t_sparse / t_decode {t_sparse / t_decode:.3f}")
    assert t_sparse < t_decode + t_compact, (t_sparse, t_decode, t_compact)
