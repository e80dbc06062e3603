"""GPU tests: trpx_select_frames (select_frames.hip).  The truth is numpy on the SOURCE BYTES --
b"".join(src[off[f]:off[f + 1]] for f in frames), the cumulative sizes for the offsets --, so no encoder or decoder is trusted
for the bytes.  Every buffer is a view carved out of a larger tensor at the weakest alignment the header allows (terse 4 mod 16,
frames 4 mod 8, out 16 mod 128; tests/alignment.py): 0xFF surrounds what is read, a position-dependent pattern lies in and
around what is written, and every case ends with the guards intact."""
import io
import os
import subprocess

import numpy as np
import pytest

from alignment import align_up, carve, carve_copy, carve_stream, same_bytes, to_bytes
from gpu_support import CAPACITY, CORRUPT, INVALID_ARG, OK, encode, mixed, to_dev, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096                                                # bytes of `out` a wavefront owns at a time (kSelChunk, select_map.hpp)
LINE = 16                                                   # bytes of an output line
MISALIGN_SEED = 0                                           # chosen with the oracle encoder: see test_misalignment


def _code(dt):
    from trpx_amd import codec
    return codec.dtype_code(dt)


def _encode(px, block=12, index=None):
    """codec.encode of [frames, values] pixels: (stream bytes, offsets int64 [frames + 1], Encoded), on the host."""
    enc = encode(px, index=index, block=block)
    return enc.stack().cpu().numpy().copy(), enc.frame_offsets.cpu().numpy().copy(), enc


def truth(src, off, frames, n_frames=None, terse_bytes=None):
    """(bytes, offsets) of the selected stack from the source bytes alone; an entry that is no frame, or whose offsets decrease
    or leave the stream, is an empty frame."""
    n_frames = len(off) - 1 if n_frames is None else n_frames
    terse_bytes = src.size if terse_bytes is None else terse_bytes
    parts = []
    for f in frames:
        f = int(f)
        good = f < n_frames and int(off[f]) <= int(off[f + 1]) <= terse_bytes
        parts.append(src[int(off[f]):int(off[f + 1])].tobytes() if good else b"")
    sizes = np.array([len(p) for p in parts], np.int64)
    return np.frombuffer(b"".join(parts), np.uint8), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def select(src, off, frames, n_values, dt, *, block=12, cap="fit", expect=OK, index=None, n_frames=None, terse_bytes=None):
    """One trpx_select_frames call on carved buffers, checked against truth(): status, out_offsets, the bytes, the zero pad, the
    pattern behind align4(total) and every guard.  cap: "fit" = align4(total), an int, or None for the sizes-only query.
    Returns (out view, out_offsets view, out_index or None, total) for what a case checks beyond that."""
    import torch
    from trpx_amd import _lib, codec
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n_frames = len(off) - 1 if n_frames is None else n_frames
    terse_bytes = src.size if terse_bytes is None else terse_bytes
    frames = np.ascontiguousarray(frames, dtype=np.uint32)
    want, want_off = truth(src, off, frames, n_frames, terse_bytes)
    total = want.size
    if cap == "fit":
        cap = align_up(total, 4)
    room_bytes = align_up(max(total, 1), LINE) + 64 if cap is None else cap
    d_terse, _, ck_terse = carve_stream(torch.from_numpy(src.copy()).to(dev), 4)
    d_off, _, ck_off = carve_copy(torch.from_numpy(np.asarray(off, np.int64).copy()).to(dev), 8)
    d_frames, _, ck_frames = carve_copy(torch.from_numpy(frames.view(np.int32).copy()).to(dev), 4)
    d_out, _, ck_out = carve(room_bytes, torch.uint8, 16, dev)
    d_out_off, _, ck_out_off = carve(8 * (frames.size + 1), torch.int64, 8, dev)
    d_status, _, ck_status = carve(32, torch.int32, 8, dev)
    assert d_terse.data_ptr() % 16 == 4 and d_frames.data_ptr() % 8 == 4 and d_out.data_ptr() % 128 == 16
    before = to_bytes(d_out).copy()
    ws = torch.empty(max(L.trpx_select_frames_workspace_bytes(n_frames, frames.size), 8), dtype=torch.uint8, device=dev)
    d_index = None
    if index is not None:
        d_index = torch.empty(codec.index_bytes(dt, n_values, frames.size, block), dtype=torch.uint8, device=dev)
    rc = L.trpx_select_frames(_code(dt), d_terse.data_ptr(), terse_bytes, d_off.data_ptr(), index.data_ptr() if index is not None else None,
                              n_values, n_frames, block, d_frames.data_ptr(), frames.size, d_out.data_ptr() if cap is not None else None,
                              cap or 0, d_out_off.data_ptr(), d_index.data_ptr() if d_index is not None else None, d_status.data_ptr(),
                              ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.trpx_last_error_string()
    torch.cuda.synchronize()
    status = d_status.cpu().numpy()
    print(f"select: n_select={frames.size} total={total} cap={cap} status={status[:2].tolist()}")
    if cap is None and expect == OK:
        expect = CAPACITY                                   # the sizes-only query answers as trpx_encode's does
    assert status[0] == expect and status[1] == 0, (status, expect)
    assert np.array_equal(d_out_off.cpu().numpy(), want_off), "out_offsets"
    got = to_bytes(d_out)
    written = align_up(total, 4) if expect == OK else 0
    same_bytes(got[:min(written, total)], want[:min(written, total)], "the selected stack")
    assert not got[total:written].any(), "bytes [total, align4(total)) are zeroed"
    same_bytes(got[written:], before[written:], "the pattern behind align4(total)")
    for ck, what in ((ck_terse, "terse"), (ck_off, "frame_offsets"), (ck_frames, "frames"), (ck_out, "out"), (ck_out_off, "out_offsets"),
                     (ck_status, "status")):
        ck(what)
    return d_out, d_out_off, d_index, total


def _lists(n, seed):
    rng = np.random.default_rng(seed + 1000)
    return {"identity": np.arange(n), "reverse": np.arange(n)[::-1].copy(), "every_third": np.arange(0, n, 3),
            "repeats": rng.integers(0, n, size=n + n // 2 + 5)}


# ---- misalignment: every (source residue, destination residue) pair ----------------------------------------------------------
@pytest.fixture(scope="module")
def small_u8(gpu):
    px = mixed(np.uint8, (48, 100), MISALIGN_SEED, zero_stretch=True)
    src, off, _ = _encode(px)
    return px, src, off


def _pairs(off, frames):
    sizes = np.diff(off)[frames]
    dst = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    return set(zip((off[frames] % 4).tolist(), (dst % 4).tolist()))


def test_misalignment_fixture_holds_every_residue_pair(small_u8):
    """A condition of the test, not a measurement: MISALIGN_SEED was chosen on the CPU with the oracle encoder (frames of 99 to
    102 bytes) so that the list with repeats alone meets all 16 pairs (source offset mod 4, destination offset mod 4)."""
    _, src, off = small_u8
    lists = _lists(48, MISALIGN_SEED)
    assert len(_pairs(off, lists["repeats"])) == 16
    assert len(set().union(*(_pairs(off, l) for l in lists.values()))) == 16
    assert lists["repeats"].size > 48 and np.unique(lists["repeats"]).size < lists["repeats"].size


@pytest.mark.parametrize("which", ["identity", "reverse", "every_third", "repeats"])
def test_misalignment(small_u8, which):
    _, src, off = small_u8
    select(src, off, _lists(48, MISALIGN_SEED)[which], 100, np.uint8)


# ---- tiny frames: many boundaries per 16-byte line ---------------------------------------------------------------------------
def test_tiny_frames(gpu):
    rng = np.random.default_rng(5)
    top = np.array([1, 4, 8])[rng.integers(0, 3, size=300)]  # zeros, 2-bit and 3-bit values: streams of 1, 2 and 3 bytes
    px = (rng.integers(0, 1 << 30, size=(300, 5)) % top[:, None]).astype(np.uint8)
    px[top > 1, 0] = top[top > 1] - 1
    src, off, _ = _encode(px)
    assert set(np.diff(off).tolist()) == {1, 2, 3}
    select(src, off, np.arange(300), 5, np.uint8)
    select(src, off, np.arange(0, 300, 3), 5, np.uint8)
    select(src, off, rng.integers(0, 300, size=3000), 5, np.uint8)              # more than a chunk of them


def test_one_byte_frames(gpu):
    src, off, _ = _encode(np.zeros((300, 5), np.uint8))
    assert src.size == 300 and (np.diff(off) == 1).all()     # sixteen boundaries in a line
    select(src, off, np.arange(300)[::-1], 5, np.uint8)
    select(src, off, np.random.default_rng(6).integers(0, 300, size=CHUNK + 37), 5, np.uint8)


# ---- large frames: every stream longer than two chunks -----------------------------------------------------------------------
def test_large_frames(gpu):
    px = np.random.default_rng(7).integers(0, 65536, size=(3, 64 * 1024)).astype(np.uint16)
    src, off, _ = _encode(px)
    assert (np.diff(off) > 2 * CHUNK).all()
    select(src, off, [2, 0, 2], 64 * 1024, np.uint16)


# ---- every container -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32])
def test_every_container(gpu, oracle, dt):
    """Besides the bytes: the result is what codec.encode writes for px[frames] -- stream, offsets and pad bytes --, and the
    oracle's decoders (the project's own; the reference's where it is built) turn it into px[frames]."""
    import torch
    frames = np.array([6, 1, 1, 4, 0])
    px = mixed(dt, (7, 1000), 11, zero_stretch=True)
    if np.dtype(dt).itemsize == 4:
        # the reference's own decoder does not expand 32-bit wide fields (on the encoder's source stream either: checked with
        # oracle/_ref on the CPU), so the 32-bit containers carry values of up to 31 significant bits here
        lim = 1 << (31 - (np.dtype(dt).kind == "i"))
        q = px.astype(np.int64)
        px = np.where(np.abs(q) >= lim, q % lim, q).astype(dt)
    src, off, _ = _encode(px)
    d_out, d_out_off, _, total = select(src, off, frames, 1000, dt)
    _, _, direct = _encode(px[frames])
    assert direct.total_bytes() == total
    assert torch.equal(direct.frame_offsets, d_out_off)
    pad = align_up(total, 4)
    assert torch.equal(direct.data[:pad], d_out[:pad]) and not d_out[total:pad].any()
    got, got_off = d_out.cpu().numpy(), d_out_off.cpu().numpy()
    for i, f in enumerate(frames):
        frame = got[got_off[i]:got_off[i + 1]]
        assert np.array_equal(oracle.decode(frame, 1000, dt), px[f])
        if oracle.have_ref():
            assert np.array_equal(oracle.ref_decode(frame, 1000, dt, direct.prolix_bits()), px[f])


def test_int64_and_block_7_are_bytes_only(gpu):
    """Only bytes move: a stack of 64-bit pixels and one with block 7 succeed with index = NULL."""
    px64 = np.random.default_rng(12).integers(-(1 << 50), 1 << 50, size=(7, 1000)).astype(np.int64)
    src, off, _ = _encode(px64)
    select(src, off, [3, 3, 0, 6], 1000, np.int64)
    px = mixed(np.uint16, (7, 1000), 13, zero_stretch=True)
    src, off, _ = _encode(px, block=7)
    select(src, off, [5, 2, 6, 6, 0], 1000, np.uint16, block=7)


# ---- capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity_edges(small_u8):
    _, src, off = small_u8
    frames = _lists(48, MISALIGN_SEED)["every_third"]
    total = truth(src, off, frames)[0].size
    assert total % 4                                         # (the pad is there to be checked)
    select(src, off, frames, 100, np.uint8, cap=align_up(total, 4))
    select(src, off, frames, 100, np.uint8, cap=align_up(total, 4) - 4, expect=CAPACITY)
    select(src, off, frames, 100, np.uint8, cap=None)        # sizes only: out = NULL, capacity 0


# ---- bad inputs: checks of the range guards (everything stays inside owned memory by construction of the carve) ---------------
@pytest.mark.parametrize("bad", [48, 0xFFFFFFFF])
def test_bad_list_entry(small_u8, bad):
    _, src, off = small_u8
    frames = np.array([3, 7, bad, 11, 2], np.uint32)
    select(src, off, frames, 100, np.uint8, cap=4096, expect=INVALID_ARG)
    select(src, off, frames, 100, np.uint8, cap=16, expect=INVALID_ARG)         # wins over CAPACITY


def test_bad_offsets(small_u8):
    _, src, off = small_u8
    dec = off.copy()
    dec[20], dec[21] = off[21], off[20]                      # frame 20 runs backwards
    select(src, off=dec, frames=np.arange(48), n_values=100, dt=np.uint8, cap=8192, expect=CORRUPT)
    select(src, off=dec, frames=[5, 30], n_values=100, dt=np.uint8)               # (only selected frames are judged)
    beyond = off.copy()
    beyond[48] = src.size + 1
    select(src, off=beyond, frames=[0, 47], n_values=100, dt=np.uint8, cap=8192, expect=CORRUPT)
    select(src, off=beyond, frames=[47, 48], n_values=100, dt=np.uint8, cap=16, expect=CORRUPT)   # over INVALID_ARG and CAPACITY


# ---- the decode index travels with the frames ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.uint16, np.int32])
def test_index(gpu, dt):
    import torch
    from trpx_amd import _lib, codec
    L = _lib.lib()
    n = 7000                                                 # 584 blocks (rows end inside 16-byte lines), 3 groups
    frames = np.array([6, 1, 1, 4, 0, 6, 2, 3, 5])
    px = mixed(dt, (7, n), 21, zero_stretch=True)
    src, off, enc = _encode(px, index=True)
    d_out, d_out_off, d_index, total = select(src, off, frames, n, dt, index=enc.index)
    stack = d_out[:align_up(total, 4)].clone()               # (a fresh tensor: 256-byte aligned)
    back, st = codec.decode(stack[:total], d_out_off.clone(), n, frames.size, dt, index=d_index)
    torch.cuda.synchronize()
    assert int(st[0].item()) == OK and np.array_equal(to_np(back), px[frames])
    built = codec.build_index(stack[:total], d_out_off.clone(), n, frames.size, dt)
    groups = L.trpx_group_count(n, 12)
    states = [torch.zeros(frames.size * groups, dtype=torch.int64, device=gpu) for _ in range(2)]
    for idx, s in zip((d_index, built), states):
        assert L.trpx_index_group_states(idx.data_ptr(), n, frames.size, 12, s.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(states[0], states[1])
    w = np.random.default_rng(22).integers(-5, 6, size=(2, n)).astype(np.int32)
    dots, st = codec.decode_dot(stack[:total], d_out_off.clone(), n, frames.size, dt, to_dev(w), index=d_index)
    torch.cuda.synchronize()
    assert int(st[0].item()) == OK
    assert np.array_equal(dots.cpu().numpy(), (px[frames].astype(np.int64)[:, None, :] * w.astype(np.int64)[None]).sum(-1))


# ---- stream ordered: one captured call, replayed with another list in the same buffer ------------------------------------------
def test_graph_replay_with_a_new_list(small_u8, gpu):
    import torch
    from trpx_amd import codec
    _, src, off = small_u8
    lists = _lists(48, MISALIGN_SEED)
    first, second = lists["repeats"], lists["repeats"][::-1].copy()
    terse, offs = torch.from_numpy(src).to(gpu), torch.from_numpy(off).to(gpu)
    frames = torch.from_numpy(first.astype(np.int32)).to(gpu)
    out = torch.empty(16384, dtype=torch.uint8, device=gpu)
    out_offs = torch.empty(first.size + 1, dtype=torch.int64, device=gpu)
    status = torch.empty(8, dtype=torch.int32, device=gpu)
    ws = codec.Workspace(gpu)
    ws.get(codec.select_frames_workspace_bytes(48, first.size))
    kw = dict(out=out, workspace=ws, status=status, out_offsets=out_offs)
    codec.select_frames(terse, offs, frames, 100, 48, np.uint8, **kw)           # eager
    torch.cuda.synchronize()
    want, want_off = truth(src, off, first)
    assert np.array_equal(out_offs.cpu().numpy(), want_off) and np.array_equal(out[:want.size].cpu().numpy(), want)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            codec.select_frames(terse, offs, frames, 100, 48, np.uint8, **kw)
    for lst in (second, first):
        frames.copy_(torch.from_numpy(lst.astype(np.int32)))
        out.zero_(); out_offs.zero_()
        g.replay()
        torch.cuda.synchronize()
        want, want_off = truth(src, off, lst)
        assert int(status[0].item()) == OK
        assert np.array_equal(out_offs.cpu().numpy(), want_off) and np.array_equal(out[:want.size].cpu().numpy(), want)


# ---- upper layers ----------------------------------------------------------------------------------------------------------------
def test_codec_select_frames_sizes_itself(small_u8, gpu):
    import torch
    from trpx_amd import _lib, codec
    px, src, off = small_u8
    terse, offs = torch.from_numpy(src).to(gpu), torch.from_numpy(off).to(gpu)
    frames = np.array([40, 2, 2, 17])
    sel = codec.select_frames(terse, offs, torch.from_numpy(frames.astype(np.int32)).to(gpu), 100, 48, np.uint8)
    sel.check()
    want, want_off = truth(src, off, frames)
    assert sel.n_frames == 4 and sel.total_bytes() == want.size and sel.prolix_bits() == 0
    assert np.array_equal(sel.stack().cpu().numpy(), want) and np.array_equal(sel.frame_offsets.cpu().numpy(), want_off)
    back, st = codec.decode(sel.stack(), sel.frame_offsets, 100, 4, np.uint8)
    torch.cuda.synchronize()
    assert int(st[0].item()) == OK and np.array_equal(back.cpu().numpy(), px[frames])
    bad = codec.select_frames(terse, offs, torch.tensor([1, 48], dtype=torch.int32, device=gpu), 100, 48, np.uint8)
    with pytest.raises(_lib.TrpxError) as e:
        bad.check()
    assert e.value.code == INVALID_ARG


def test_terse_select_with_a_mask_and_round_trip(gpu):
    from trpx_amd import Terse
    px = mixed(np.uint16, (9, 35 * 20), 31, zero_stretch=True)
    t = Terse()
    t.dim([35, 20])
    t.push_back_stack(px)
    mask = np.array([1, 0, 0, 1, 1, 0, 1, 0, 1], bool)
    kept = t.select(mask)
    assert kept.number_of_frames() == 5 and kept.dim() == [35, 20] and kept.size() == 700 and not kept.is_signed()
    assert kept.bits_per_val() == t.bits_per_val()           # kept from the source: an upper bound
    assert np.array_equal(kept.prolix_stack(np.uint16), px[mask])
    direct = Terse()
    direct.push_back_stack(px[mask])
    assert kept.data() == direct.data() and kept.frame_sizes() == direct.frame_sizes()
    order = [8, 0, 0, 3, 8, 8, 1, 2, 4, 5, 6, 7]             # longer than the stack
    assert np.array_equal(t.select(order).prolix_stack(np.uint16), px[order])
    for frame_index in (False, True):
        f = io.BytesIO()
        kept.write(f, frame_index=frame_index)
        f.seek(0)
        again = Terse.read(f)
        assert again.number_of_frames() == 5 and np.array_equal(again.prolix_stack(np.uint16), px[mask])
    assert t.select([]).number_of_frames() == 0
    for bad in ([9], [-1], np.ones(8, bool)):
        with pytest.raises(ValueError):
            t.select(bad)


def test_cpp_class_select():
    exe = os.path.join(ROOT, "tests", "cpp", "select_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "select_example.mk", "select_example"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK select example" in r.stdout, r.stdout + r.stderr
