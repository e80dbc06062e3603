"""GPU tests: trpx_decode_dot (decode_dot.hip).  The truth is numpy on the ORIGINAL pixels, in int64
with wrap, compared for equality: the codec is lossless and the sums are integers, so no decoder is trusted and no tolerance is
needed.  Every output sits in the middle of a guarded allocation, 64 sentinel elements on either side."""
import dataclasses
import json
import os
import statistics
import subprocess

import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import CORRUPT, OK, Guarded, encode, input_forms, ladder, ladder_holds_every_width, mixed, status_block, torch_dt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
WIDTH = 37                                                  # the row length the 2-D maps use: no multiple or divisor of 12


def truth(px: np.ndarray, w: np.ndarray) -> np.ndarray:
    """[frames, K] int64, with wrap: numpy on the original pixels"""
    with np.errstate(over="ignore"):
        return (px.astype(np.int64)[:, None, :] * w.astype(np.int64)[None]).sum(-1)


def truth_mod64(px: np.ndarray, w: np.ndarray) -> np.ndarray:
    """The same with Python integers mod 2^64 (the wrap cases)"""
    out = np.empty((px.shape[0], w.shape[0]), np.int64)
    for f in range(px.shape[0]):
        for k in range(w.shape[0]):
            s = sum(int(a) * int(b) for a, b in zip(px[f].tolist(), w[k].tolist())) % (1 << 64)
            out[f, k] = s - (1 << 64) if s >= (1 << 63) else s
    return out


# ---- the maps --------------------------------------------------------------------------------------------------------------------
def disc_map(v, width=WIDTH, radius=None):
    y, x = np.arange(v) // width, np.arange(v) % width
    h = -(-v // width)
    r = radius if radius is not None else max(1, min(width, h) // 3)
    return (((x - width // 2) ** 2 + (y - h // 2) ** 2) <= r * r).astype(np.int32)[None]


def map_sets(v, seed):
    """(name, weights [K, v] int32): K in {1, 2, 3, 16}"""
    rng = np.random.default_rng(seed)
    single = np.zeros((2, v), np.int32)
    single[0, v - 1] = 1
    single[1, 0] = 1
    p = np.arange(v)
    com = np.stack([p % WIDTH, p // WIDTH, np.ones(v, np.int64)]).astype(np.int32)
    rnd = rng.integers(I32_MIN, I32_MAX + 1, size=(16, v), dtype=np.int64)
    rnd[rng.integers(0, 16, size=8), rng.integers(0, v, size=8)] = I32_MIN
    rnd[rng.integers(0, 16, size=8), rng.integers(0, v, size=8)] = I32_MAX
    rnd[0, 0], rnd[15, v - 1] = I32_MIN, I32_MAX
    rnd[3] = 0                                              # one map of the sixteen is blank
    rnd[5, : v // 2] = 0                                    # ... and one is zero on half the frame
    return [("ones", np.ones((1, v), np.int32)), ("zeros", np.zeros((2, v), np.int32)), ("single", single), ("disc", disc_map(v)),
            ("x, y, 1", com), ("random16", rnd.astype(np.int32))]


# ---- the call ----------------------------------------------------------------------------------------------------------------
def _ws(enc, n_frames, n_maps=16):
    from trpx_amd import codec
    import torch
    need = codec.decode_dot_workspace_bytes(enc.data.numel(), enc.n_values, n_frames, enc.dtype, n_maps)
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda")


def _dot(enc, dt, w, mode="index", first=0, n_frames=None, ws=None, w_dev=None):
    """One trpx_decode_dot call into a guarded allocation; w: [K, n_values] int32 on the host (w_dev: the device tensor to
    pass instead).  Returns (dots [n_frames, K] on the host, status word 0) after checking the guards."""
    from trpx_amd import _lib
    from trpx_amd.codec import dtype_code
    import torch
    dt = np.dtype(dt)
    n_frames = enc.n_frames - first if n_frames is None else n_frames
    k = w.shape[0]
    if w_dev is None:
        w_dev = torch.from_numpy(np.ascontiguousarray(w, dtype=np.int32)).cuda()
    out = Guarded(n_frames * k, np.int64, SENTINEL)
    status = status_block()
    ws = _ws(enc, n_frames) if ws is None else ws
    stack = enc.stack()
    offs, index = input_forms(enc, mode, first)
    rc = _lib.lib().trpx_decode_dot(dtype_code(dt), stack.data_ptr(), stack.numel(), offs.data_ptr() if offs is not None else None,
                                    index.data_ptr() if index is not None else None, enc.n_values, n_frames, 12, w_dev.data_ptr(), k,
                                    out.view.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().trpx_last_error_string()
    torch.cuda.synchronize()
    return out.check("dots_out").reshape(n_frames, k).copy(), int(status[0].item())


def _check(enc, px, w, mode="index", what="", want=None, **kw):
    want = truth(px, w) if want is None else want
    got, status = _dot(enc, px.dtype, w, mode, **kw)
    ctx = (what, mode, px.dtype, px.shape, w.shape)
    assert status == OK, ctx
    assert got.dtype == np.int64 and np.array_equal(got, want), ctx
    return got


# the frame sizes at which each mechanism can fail: a partial and a whole last block, the group edge (256 blocks), the run edge
# (8 groups), two runs and a tail
N_VALUES = [1, 11, 12, 13, 3071, 3072, 3073, 24575, 24576, 24577, 49157]
FRAME_COUNTS = [1, 3, 5]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("v", N_VALUES)
def test_exactness_matrix(dt, v):
    n = FRAME_COUNTS[(N_VALUES.index(v) + DTYPES.index(dt)) % 3]           # (every size with every count over the six types)
    sets = map_sets(v, seed=v)
    assert sorted({w.shape[0] for _, w in sets}) == [1, 2, 3, 16]
    for what, px in (("mixed", mixed(dt, (n, v), seed=n * 1000 + v % 1000, zero_stretch=True)), ("ladder", ladder(dt, (n, v), seed=v))):
        if what == "ladder" and v >= 12 * 3 * 33:            # (three cycles of the widths 0 .. 32)
            ladder_holds_every_width(px)
        enc = encode(px)
        ws = _ws(enc, n)
        for name, w in sets:
            got = _check(enc, px, w, what=f"{what} / {name}", ws=ws)
            if name == "zeros":
                assert not got.any()                        # (status 0 was asserted: the stack was still walked and validated)


@pytest.mark.parametrize("v", N_VALUES)
def test_every_frame_count_on_every_size(v):
    for n in FRAME_COUNTS:
        px = mixed(np.int16 if v % 2 else np.uint32, (n, v), seed=n, zero_stretch=True)
        enc = encode(px)
        for name, w in map_sets(v, seed=n):
            _check(enc, px, w, what=name)


def test_wrap_is_modulo_two_to_the_64():
    v = 3073
    for dt, pv, wv in ((np.uint32, 0xFFFFFFFF, I32_MAX), (np.int32, I32_MIN, I32_MIN)):
        px = np.full((2, v), pv, dt)
        w = np.full((2, v), wv, np.int32)
        w[1, ::2] = 1                                       # (a second map whose sum does not wrap the same way)
        assert v * abs(pv) * abs(wv) > (1 << 63)            # the sum leaves int64
        want = truth_mod64(px, w)
        assert np.array_equal(want, truth(px, w))           # numpy's int64 arithmetic wraps alike
        enc = encode(px)
        for mode in ("index", "offsets", "none"):
            _check(enc, px, w, mode, what="wrap", want=want)


def test_maps_that_are_four_byte_aligned_only():
    """Maps at an address that is 4 but not 16 bytes aligned, with n_values % 4 == 0: the value-by-value path alone."""
    import torch
    v, n = 3072 * 2, 3
    px = mixed(np.uint16, (n, v), seed=5, zero_stretch=True)
    enc = encode(px)
    sets = map_sets(v, seed=5)
    for name, w in sets:
        buf = torch.zeros(w.size + 8, dtype=torch.int32, device="cuda")
        w_dev = buf[1:1 + w.size]
        w_dev.copy_(torch.from_numpy(np.ascontiguousarray(w).reshape(-1)).cuda())
        assert w_dev.data_ptr() % 16 == 4
        _check(enc, px, w, what=f"unaligned / {name}", w_dev=w_dev)


@pytest.mark.parametrize("dt", [np.uint16, np.int32], ids=lambda d: np.dtype(d).name)
def test_input_forms_runs_and_sub_stacks_agree(dt):
    n, v = 5, 49157
    px = mixed(dt, (n, v), seed=17, zero_stretch=True)
    enc = encode(px)
    for name, w in map_sets(v, seed=17)[3:]:
        outs = [_check(enc, px, w, mode, what=f"forms / {name}") for mode in ("index", "offsets", "none")]
        outs.append(_check(enc, px, w, "index", what="second run"))
        for o in outs[1:]:
            assert o.tobytes() == outs[0].tobytes(), (dt, name)
        for a, b in ((0, 5), (1, 4), (4, 5), (2, 3)):        # frames [a, b) alone: frame_offsets + a, n_frames = b - a, no index
            sub = _check(enc, px[a:b], w, "offsets", what=f"frames [{a}, {b})", first=a, n_frames=b - a)
            assert sub.tobytes() == outs[0][a:b].tobytes()


def _group_bits(widths, n_values, lo, hi):
    """Bits of the blocks [lo, hi) of one frame under the layout rule (1 header bit where the width repeats, else 4 / 6 / 12)."""
    w = widths.astype(np.int64)
    prev = np.concatenate([[0], w[:-1]])
    hl = np.where(w == prev, 1, np.where(w < 7, 4, np.where(w < 10, 6, 12)))
    cnt = np.full(w.size, 12)
    cnt[-1] = n_values - 12 * (w.size - 1)
    return int((hl + cnt * w)[lo:hi].sum())


def test_support_rule_does_not_skip_validation():
    """Every map is zero on all but one block: the sums are exact on every form, and damage in the part of the stack no block
    is fetched from -- a width byte of the index, a frame-offset table whose end is short -- is still found."""
    import torch
    n, v = 3, 7000
    px = mixed(np.uint16, (n, v), seed=31, zero_stretch=True)
    px[:, :12] = np.arange(1, 13)                           # (the one block the maps see holds something)
    enc = encode(px)
    w = np.zeros((3, v), np.int32)
    w[0, 5], w[1, 0], w[2, 11] = 7, -3, I32_MIN
    for mode in ("index", "offsets", "none"):
        _check(enc, px, w, mode, what="one block")
    groups, blocks = 3, 584                                 # ceil(7000 / 12), ceil(584 / 256)
    w_at = (8 * n * groups + 15) // 16 * 16                 # (the index: the group offsets, then the widths)
    widths = enc.index[w_at: w_at + n * blocks].cpu().numpy().reshape(n, blocks)
    for frame, block in ((1, 300), (0, 583), (2, 256)):     # blocks of groups 1 and 2, where every map is zero
        assert not w[:, 12 * block: 12 * block + 12].any()
        bent_w = widths[frame].astype(np.int64)
        bent_w[block] += 1 if bent_w[block] < 16 else -1
        lo, hi = block // 256 * 256, min(block // 256 * 256 + 256, blocks)
        assert _group_bits(bent_w, v, lo, hi) != _group_bits(widths[frame], v, lo, hi)   # (the fixture: the damage moves the group's end)
        bent = dataclasses.replace(enc, index=enc.index.clone())
        bent.index[w_at + frame * blocks + block] = int(bent_w[block])
        assert _dot(bent, px.dtype, w)[1] == CORRUPT, (frame, block)
    short = dataclasses.replace(enc, frame_offsets=enc.frame_offsets.clone())
    short.frame_offsets[-1] -= 1
    assert _dot(short, px.dtype, w)[1] == CORRUPT
    assert _dot(short, px.dtype, w, mode="offsets")[1] == CORRUPT
    assert _dot(enc, px.dtype, np.zeros((1, v), np.int32))[1] == OK              # (and the intact stack under an all-zero map)
    assert _dot(short, px.dtype, np.zeros((1, v), np.int32))[1] == CORRUPT       # ... validated where nothing at all is fetched


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
        code = dtype_code(np.dtype(dtname))
        index = torch.zeros(codec.index_bytes(np.dtype(dtname), v, n), dtype=torch.uint8, device="cuda")
        st = status_block()
        assert _lib.lib().trpx_build_index(code, terse.data_ptr(), nbytes, offs.data_ptr(), v, n, 12, index.data_ptr(), st.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        have_index = int(st[0].item()) == OK
        if e["kind"] in ("K0", "K2"):
            assert have_index
        enc = dataclasses.make_dataclass("Stack", ["data", "frame_offsets", "index", "n_values", "n_frames", "dtype", "stack"])(
            terse, offs, index, v, n, torch_dt(dtname), lambda: terse[:nbytes])
        for name, w in map_sets(v, seed=3)[3:]:
            want = truth(S.px, w)
            for mode in ("index", "offsets", "none"):
                if mode == "index" and not have_index:
                    continue
                got, status = _dot(enc, dtname, w, mode)
                ctx = (dtname, e["kind"], mode, name)
                assert status in (OK, CORRUPT), ctx
                assert status == CORRUPT or np.array_equal(got, want), ctx       # never status 0 with wrong sums
                if e["kind"] in ("K0", "K2"):
                    assert status == OK, ctx                                     # padded widths decode everywhere
                elif mode != "index":
                    assert status == CORRUPT, ctx                                # restated widths have no index


@pytest.mark.parametrize("v", [13, 3073, 24576])
def test_weights_behind_the_maps_are_never_read(v):
    """K maps and a guard map of large weights behind them in one allocation: the sums depend on the K maps alone -- a read
    behind a map's n_values (the partial last block) would pick up the next map's head, or the guard's."""
    import torch
    n = 3
    px = mixed(np.uint16, (n, v), seed=v, zero_stretch=True)
    px[:, -1] = 65535
    enc = encode(px)
    rng = np.random.default_rng(v)
    for k in (1, 2, 16):
        w = rng.integers(I32_MIN, I32_MAX + 1, size=(k, v), dtype=np.int64).astype(np.int32)
        for guard in (I32_MAX, I32_MIN):
            both = torch.from_numpy(np.concatenate([w, np.full((1, v), guard, np.int32)])).cuda()
            _check(enc, px, w, what=f"guard map {guard}", w_dev=both)


def test_graph_capture_replays_with_new_maps():
    from trpx_amd import codec
    import torch
    n, v = 6, 511 * 513
    px = mixed(np.uint16, (n, v), seed=9, zero_stretch=True)
    enc = encode(px)
    maps = [np.concatenate([disc_map(v, 513, 40), np.stack([np.arange(v) % 513, np.arange(v) // 513]).astype(np.int32)]),
            np.concatenate([disc_map(v, 513, 90) * -5, np.stack([np.arange(v) // 513, np.ones(v, np.int64)]).astype(np.int32)]),
            np.zeros((3, v), np.int32)]
    w_dev = torch.from_numpy(maps[0]).cuda()
    out = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")
    ws = codec.Workspace("cuda")
    stack = enc.stack()

    def call():
        codec.decode_dot(stack, enc.frame_offsets, v, n, torch.uint16, w_dev, index=enc.index, out=out, workspace=ws, status=status)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                              # warm-up outside the capture
        call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), truth(px, maps[0]))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                     # one stream, no parallel branches
        call()
    for w in maps[1:] + maps[:1]:
        w_dev.copy_(torch.from_numpy(w).cuda())             # the same buffer, new maps
        out.fill_(SENTINEL)
        status.fill_(77)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(status[0].item()) == OK
        assert np.array_equal(out.cpu().numpy(), truth(px, w))


def test_python_surfaces():
    from trpx_amd import codec
    from trpx_amd.terse import Terse
    import torch
    rng = np.random.default_rng(43)
    h, wd = 20, 35
    px = rng.integers(0, 3000, size=(3, h * wd)).astype(np.uint16)
    px[:, 100:240] = rng.integers(0, 65536, size=(3, 140))
    w = np.concatenate([disc_map(h * wd, wd, 6), np.stack([np.arange(h * wd) % wd, np.arange(h * wd) // wd]).astype(np.int32)])
    want = truth(px, w)
    enc = encode(px)
    abi, status = _dot(enc, px.dtype, w)
    assert status == OK and np.array_equal(abi, want)
    # the device-resident wrapper, [K, n_values] and [K, H, W]
    for shape in ((3, h * wd), (3, h, wd)):
        dots, st = codec.decode_dot(enc.stack(), enc.frame_offsets, h * wd, 3, torch.uint16, torch.from_numpy(w.reshape(shape)).cuda(), index=enc.index)
        torch.cuda.synchronize()
        assert int(st[0].item()) == OK and dots.dtype == torch.int64 and tuple(dots.shape) == (3, 3)
        assert np.array_equal(dots.cpu().numpy(), abi)
    dots, st = codec.decode_dot(enc.stack(), None, h * wd, 3, torch.uint16, torch.from_numpy(w).cuda())      # frames located, index built
    assert int(st[0].item()) == OK and np.array_equal(dots.cpu().numpy(), abi)
    assert codec.decode_dot_workspace_bytes(enc.stack().numel(), h * wd, 3, torch.uint16, 3) > 0
    with pytest.raises(TypeError):
        codec.decode_dot(enc.stack(), enc.frame_offsets, h * wd, 3, torch.uint16, torch.from_numpy(w.astype(np.int64)).cuda())
    with pytest.raises(ValueError):
        codec.decode_dot(enc.stack(), enc.frame_offsets, h * wd, 3, torch.uint16, torch.zeros((17, h * wd), dtype=torch.int32, device="cuda"))
    # the host class
    t = Terse()
    t.push_back_stack(px)
    for shape in ((3, h * wd), (3, h, wd)):
        got = t.prolix_dot(w.reshape(shape))
        assert got.dtype == np.int64 and np.array_equal(got, abi)
    assert np.array_equal(t.prolix_dot(w[0]), abi[:, :1])    # one map
    with pytest.raises(ValueError):
        t.prolix_dot(np.zeros((2, 5), np.int32))
    with pytest.raises(TypeError):
        t.prolix_dot(np.zeros((1, h * wd), np.float32))


def test_cpp_class_prolix_dot():
    exe = os.path.join(ROOT, "tests", "cpp", "dot_example")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "dot_example.mk"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK dot example" in r.stdout, r.stdout + r.stderr


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def test_faster_than_decoding_and_reducing():
    """500 x 512^2 u16 synth-v1 with the encoder's index, resident; three maps: a disc of radius 32, x and y.  The baseline is
    what a caller pays without this entry point: trpx_decode_indexed of the stack, then per map (px.to(int64) * w[k].to(int64))
    .sum(-1), the exact integer reduction torch offers on the GPU -- in the same process, repetitions interleaved, medians.  No
    margin: the call must only be no slower than the route it replaces."""
    from trpx_amd import codec
    import torch
    n, side = 500, 512
    v = side * side
    px = codec.synth(np.uint16, 0, n, v)
    enc = codec.encode(px, index=True)
    enc.check()
    p = np.arange(v)
    w = np.concatenate([disc_map(v, side, 32), np.stack([p % side, p // side]).astype(np.int32)])
    w_dev = torch.from_numpy(w).cuda()
    w64 = w_dev.to(torch.int64)
    stack = enc.stack()
    pix = torch.empty((n, v), dtype=torch.uint16, device="cuda")
    st = torch.empty(8, dtype=torch.int32, device="cuda")
    out = torch.empty((n, 3), dtype=torch.int64, device="cuda")
    ws = codec.Workspace("cuda")
    base = [None]

    def dot():
        codec.decode_dot(stack, enc.frame_offsets, v, n, torch.uint16, w_dev, index=enc.index, out=out, workspace=ws, status=st)

    def replaced():
        codec.decode(stack, enc.frame_offsets, v, n, torch.uint16, out=pix, status=st, index=enc.index)
        p64 = pix.to(torch.int64)
        base[0] = torch.stack([(p64 * w64[k]).sum(-1) for k in range(3)], dim=1)

    for _ in range(2):
        dot()
        replaced()
    torch.cuda.synchronize()
    t_dot, t_old = [], []
    for _ in range(9):
        t_dot.append(_event_ms(dot))
        t_old.append(_event_ms(replaced))
    assert int(st[0].item()) == OK
    assert torch.equal(pix.view(torch.int16), px.view(torch.int16))
    assert torch.equal(out, base[0])                        # the two routes agree, value for value
    m_dot, m_old = statistics.median(t_dot), statistics.median(t_old)
    print(f"\n500 x 512^2 u16 synth-v1, 3 maps (disc 32, x, y): decode_dot {m_dot:.4f} ms, decode_indexed + int64 reduction {m_old:.4f} ms, "
          f"ratio {m_old / m_dot:.2f}")
    assert m_dot <= m_old, (m_dot, m_old)
