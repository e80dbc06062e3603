"""GPU tests: the position-parallel route of trpx_locate_frames (decode_locate.hip).  The truth is the
encoder's frame_offsets; for hand-edited streams it is the serial route of the same call (trpx_set_locate_path(1)), whose
status and offsets the parallel route must reproduce in every case.  trpx_decode(frame_offsets = NULL) locates the frames the
same way and decodes them on the tuned routes.  The speed ceilings are what the serial route cannot meet (0.7 s and 5.3 s for
the two 2000-frame stacks, 5.9 s for the decode without offsets)."""
import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import encode, selected

pytestmark = pytest.mark.gpu


def _lib():
    from trpx_amd import _lib
    return _lib.lib()


def _locate(stack, n, frames, dtype, serial=False, first_bad=None):
    """stack: uint8 tensor on the GPU or numpy bytes -> (offsets np.int64, status word 0).  first_bad (a list): gets the
    first frame the parallel route handed to its serial repair (workspace word 0; -1: none)."""
    import torch
    from trpx_amd import codec
    if isinstance(stack, np.ndarray):
        stack = torch.from_numpy(np.ascontiguousarray(stack, dtype=np.uint8)).to("cuda:0")
    ws = codec.Workspace(stack.device)
    with selected("trpx_set_locate_path", 1 if serial else 0):
        ws.get(256)[:4].fill_(0xEE)
        offs, st = codec.locate_frames(stack, n, frames, dtype, workspace=ws)
        torch.cuda.synchronize()
    if first_bad is not None:
        first_bad.append(int(ws.get(256)[:4].view(torch.int32).item()))
    return offs.cpu().numpy(), int(st[0].item())


def _walk_block_starts(stack, fo, n, max_w):
    """The bit positions (from the stack's start) of every block start of the frame at byte fo: a CPU walk, Terse.hpp:360-372."""
    bits = np.unpackbits(np.concatenate([np.asarray(stack, np.uint8), np.zeros(8, np.uint8)]), bitorder="little")
    nb = (n + 11) // 12
    pos, w, starts = 8 * fo, 0, []
    for b in range(nb):
        starts.append(pos)
        x = int(np.packbits(bits[pos:pos + 16], bitorder="little").view("<u2")[0])
        nv = n - 12 * (nb - 1) if b == nb - 1 else 12
        if x & 1:
            pos += 1 + nv * w
            continue
        w, hl = (x >> 1) & 7, 4
        if w == 7:
            w += (x >> 4) & 3
            hl = 6
            if w == 10:
                w += (x >> 6) & 63
                hl = 12
        assert w <= max_w
        pos += hl + nv * w
    return starts


def _random_widths(dtype, frames, n, seed, gpu, keep_p=0.5):
    """Blocks of random widths (a share keep_p of them keeps the previous block's width)."""
    import torch
    from trpx_amd import codec
    g = torch.Generator(device=gpu).manual_seed(seed)
    bits = 8 * np.dtype(dtype).itemsize
    nb = (n + 11) // 12
    w = torch.randint(0, bits + 1, (frames, nb), generator=g, device=gpu)
    keep = torch.rand((frames, nb), generator=g, device=gpu) < keep_p
    idx = torch.arange(nb, device=gpu).expand(frames, nb)
    src = torch.where(keep, torch.zeros_like(idx), idx).cummax(dim=1).values
    w = torch.gather(w, 1, src)
    wv = w.repeat_interleave(12, dim=1)[:, :n]
    v = torch.randint(0, 2**62, (frames, n), generator=g, device=gpu, dtype=torch.int64)
    v = v & ((torch.ones_like(wv) << wv) - 1)
    tdt = codec.torch_dtype(dtype)
    if tdt in (torch.uint8, torch.uint16, torch.uint32):
        return (v & ((1 << bits) - 1)).to(tdt)
    v = v & ((1 << bits) - 1)
    return (v - ((v >> (bits - 1)) << bits)).to(tdt)


def _check_exact(px, dtype):
    n, frames = px[0].numel(), px.shape[0]
    enc = encode(px, index=False)
    offs, st = _locate(enc.stack(), n, frames, dtype)
    assert st == 0, (n, frames, st)
    assert np.array_equal(offs, enc.frame_offsets.cpu().numpy()), (n, frames)
    return enc


# ---- exactness: the auto route against the encoder ------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_parallel_locate_matches_encoder(gpu, dtype):
    cases = [(5, 3000), (13, 2000), (12 * 37 + 5, 400), (512 * 512, 9), (64 * 64 + 7, 200), (1, 2), (7, 1), (600, 2)]
    for i, (n, frames) in enumerate(cases):
        _check_exact(_random_widths(dtype, frames, n, 7000 + 100 * i + DTYPES.index(dtype), gpu), dtype)


def test_parallel_locate_2000_frames_and_drifting_sizes(gpu):
    import torch
    from trpx_amd import codec, workloads
    _check_exact(codec.synth(np.uint16, 0, 2000, 256 * 256, device=gpu), np.uint16)
    _check_exact(workloads.poisson_u16(3.0, 0, 2000, 128 * 128, device=gpu), np.uint16)
    # frame sizes that drift strongly: Poisson means from 0.01 to 300 over the stack
    lam = torch.logspace(-2, np.log10(300.0), 300, device=gpu).unsqueeze(1)
    g = torch.Generator(device=gpu).manual_seed(5)
    px = torch.poisson(lam.expand(300, 96 * 96).contiguous(), generator=g).clamp(max=65535).to(torch.int32).to(torch.uint16)
    _check_exact(px, np.uint16)


def test_parallel_locate_blank_and_dense_frames(gpu):
    import torch
    from trpx_amd import workloads
    n = 256 * 256
    dense = workloads.poisson_u16(10.0, 3, 64, n, device=gpu)
    px = torch.zeros((128, n), dtype=torch.uint16, device=gpu)
    px[1::2] = dense                                       # all-zero frames (1 byte each) between header-dense ones
    _check_exact(px, np.uint16)
    # a whole pad byte: all-one u8 frames of 108 values are 16 + 8 * 13 = 120 bits (bits % 8 == 0); beside them other sizes
    for n in (108, 95, 84, 100):
        _check_exact(torch.ones((500, n), dtype=torch.uint8, device=gpu), np.uint8)


def test_parallel_locate_large_frames(gpu):
    from trpx_amd import codec, workloads
    _check_exact(workloads.poisson_u16(3.0, 0, 6, 1030 * 1065, device=gpu), np.uint16)
    _check_exact(codec.synth(np.int32, 0, 4, 2048 * 2048, device=gpu), np.int32)


# ---- streams built to defeat chain merging: equal to the serial route ----------------------------------------------------

def _vs_serial(stack, n, frames, dtype, label):
    fb = []
    got = _locate(stack, n, frames, dtype, first_bad=fb)
    want = _locate(stack, n, frames, dtype, serial=True)
    print(f"{label}: {'no frame' if fb[0] < 0 else f'frames {fb[0]} ..'} of {frames} handed to the serial repair")
    assert got[1] == want[1], (label, got[1], want[1])
    if want[1] == 0:
        assert np.array_equal(got[0], want[0]), label
    return got


def test_parallel_locate_adversarial_streams(gpu):
    import torch
    from trpx_amd import workloads
    n = 128 * 128
    cases = {}
    # long runs of one constant non-zero width with random payload: chains a block apart never meet
    g = torch.Generator(device=gpu).manual_seed(11)
    cases["const_w9"] = torch.randint(256, 512, (64, n), generator=g, device=gpu, dtype=torch.int32).to(torch.uint16)
    # periodic payloads
    cases["periodic"] = (torch.arange(n, device=gpu, dtype=torch.int32) % 24 * 997).to(torch.uint16).repeat(64, 1)
    # frames alternating blank and Poisson(10)
    alt = torch.zeros((64, n), dtype=torch.uint16, device=gpu)
    alt[::2] = workloads.poisson_u16(10.0, 0, 32, n, device=gpu)
    cases["alternating"] = alt
    for label, px in cases.items():
        enc = encode(px.contiguous(), index=False)
        got = _vs_serial(enc.stack(), n, px.shape[0], np.uint16, label)
        assert got[1] == 0 and np.array_equal(got[0], enc.frame_offsets.cpu().numpy()), label
    # pad bits set to garbage: the stack is no longer the encoder's, the serial route is the truth
    px = workloads.poisson_u16(3.0, 1, 64, n, device=gpu)
    enc = encode(px, index=False)
    stack = enc.stack().cpu().numpy().copy()
    offs = enc.frame_offsets.cpu().numpy()
    rng = np.random.default_rng(3)
    for k in range(1, 64):
        stack[offs[k] - 1] |= np.uint8(rng.integers(0, 256)) & np.uint8(0xF0)
    _vs_serial(stack, n, 64, np.uint16, "garbage_pad")


def test_parallel_locate_hostile_streams(gpu):
    from trpx_amd import workloads
    n, frames = 128 * 128, 48
    enc = encode(workloads.poisson_u16(3.0, 2, frames, n, device=gpu), index=False)
    stack = enc.stack().cpu().numpy()
    offs = enc.frame_offsets.cpu().numpy()
    _vs_serial(stack[: offs[frames // 2] + 10], n, frames, np.uint16, "truncated")
    _vs_serial(stack, n, frames + 1, np.uint16, "one too many")
    got = _vs_serial(stack, n, frames - 1, np.uint16, "one too few")
    assert got[1] == 0 and np.array_equal(got[0], offs[:frames])
    bad = stack.copy()
    k = frames // 3
    starts = _walk_block_starts(stack, int(offs[k]), n, 16)
    pos = starts[len(starts) // 2]                         # a true block start deep inside frame k: a 12-bit header of width 73
    for i, bit in enumerate([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]):
        byte, sh = divmod(pos + i, 8)
        bad[byte] = (bad[byte] & ~np.uint8(1 << sh)) | np.uint8(bit << sh)
    got = _vs_serial(bad, n, frames, np.uint16, "wide header")
    assert got[1] == 5                                     # TRPX_ERR_CORRUPT
    rng = np.random.default_rng(12)
    for trial in range(12):                                # bent frame ends
        bent = stack.copy()
        k = int(rng.integers(1, frames))
        for j in range(int(rng.integers(1, 4))):
            bent[int(offs[k]) - 1 - j] ^= np.uint8(rng.integers(1, 256))
        _vs_serial(bent, n, frames, np.uint16, f"bent {trial}")


# ---- graph capture --------------------------------------------------------------------------------------------------------

def test_parallel_locate_graph_capture(gpu):
    import torch
    from trpx_amd import codec, workloads
    n, frames = 128 * 128, 2000
    px_a = workloads.poisson_u16(3.0, 0, frames, n, device=gpu)
    px_b = px_a.flip(0).contiguous()                       # the same frames reversed: a different stack of the same length
    a, b = encode(px_a, index=False), encode(px_b, index=False)
    assert a.stack().numel() == b.stack().numel()
    buf = a.stack().clone()
    offs = torch.empty(frames + 1, dtype=torch.int64, device=gpu)
    st = torch.empty(8, dtype=torch.int32, device=gpu)
    out = torch.empty((frames, n), dtype=torch.uint16, device=gpu)
    ws, wd = codec.Workspace(gpu), codec.Workspace(gpu)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))

    def body():
        codec.locate_frames(buf, n, frames, np.uint16, workspace=ws, status=st, out=offs)
        codec.decode(buf, offs, n, frames, np.uint16, out=out, workspace=wd, status=st)

    with torch.cuda.stream(s):
        body()                                             # warm-up: workspaces allocated outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        body()
    for enc, px in ((a, px_a), (b, px_b), (a, px_a)):
        buf.copy_(enc.stack())
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert int(st[0].item()) == 0
        assert torch.equal(offs, enc.frame_offsets)
        assert torch.equal(out, px)


# ---- speed ceilings (the serial route takes 0.7 s and 5.3 s) -------------------------------------------------------------

@pytest.mark.parametrize("kind", ["synth", "poisson3"])
def test_parallel_locate_speed_ceiling(gpu, kind):
    import torch
    from trpx_amd import codec, workloads
    n, frames = 512 * 512, 2000
    px = codec.synth(np.uint16, 0, frames, n, device=gpu) if kind == "synth" else workloads.poisson_u16(3.0, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    stack = enc.stack().clone()
    want = enc.frame_offsets.clone()
    del enc, px
    ws = codec.Workspace(gpu)
    offs = torch.empty(frames + 1, dtype=torch.int64, device=gpu)
    st = torch.empty(8, dtype=torch.int32, device=gpu)

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        codec.locate_frames(stack, n, frames, np.uint16, workspace=ws, status=st, out=offs)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    warm = once()
    assert int(st[0].item()) == 0 and torch.equal(offs, want)
    assert warm < 1000.0, f"{kind}: warm-up locate took {warm:.0f} ms"
    ms = float(np.median([once() for _ in range(3)]))
    print(f"locate {kind} 2000 x 512^2: {ms:.2f} ms")
    assert ms <= 100.0, f"{kind}: {ms:.1f} ms > 100 ms"


# ---- trpx_decode(frame_offsets = NULL): located in parallel, decoded on the tuned routes ---------------------------------

@pytest.mark.parametrize("shape", [(2000, 512 * 512), (200, 1030 * 1065)])
def test_decode_without_offsets_exact(gpu, shape):
    import torch
    from trpx_amd import codec, workloads
    frames, n = shape
    px = workloads.poisson_u16(3.0, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    stack = enc.stack().clone()
    del enc
    back, st = codec.decode(stack, None, n, frames, np.uint16)
    torch.cuda.synchronize()
    assert int(st[0].item()) == 0
    assert torch.equal(back.view(frames, n), px)


def test_decode_without_offsets_corrupt(gpu):
    import torch
    from trpx_amd import codec, workloads
    n, frames = 128 * 128, 48
    enc = encode(workloads.poisson_u16(3.0, 4, frames, n, device=gpu), index=False)
    offs = enc.frame_offsets.cpu().numpy()
    truncated = enc.stack()[: int(offs[frames // 2]) + 10].clone()
    _, st = codec.decode(truncated, None, n, frames, np.uint16)
    torch.cuda.synchronize()
    assert int(st[0].item()) == 5                          # TRPX_ERR_CORRUPT, as the serial walk reports
    _, st = codec.decode(enc.stack(), None, n, frames - 1, np.uint16)
    torch.cuda.synchronize()
    assert int(st[0].item()) == 0                          # fewer frames than present: no error


def test_decode_without_offsets_speed_ceiling(gpu):
    import torch
    from trpx_amd import codec, workloads
    n, frames = 512 * 512, 2000
    px = workloads.poisson_u16(3.0, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    stack = enc.stack().clone()
    del enc
    ws = codec.Workspace(gpu)
    out = torch.empty((frames, n), dtype=torch.uint16, device=gpu)
    st = torch.empty(8, dtype=torch.int32, device=gpu)

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        codec.decode(stack, None, n, frames, np.uint16, out=out, workspace=ws, status=st)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    warm = once()
    assert int(st[0].item()) == 0 and torch.equal(out, px)
    assert warm < 1000.0, f"warm-up decode without offsets took {warm:.0f} ms"
    ms = float(np.median([once() for _ in range(3)]))
    print(f"decode without offsets, 2000 x 512^2 Poisson(3): {ms:.2f} ms")
    assert ms <= 150.0, f"{ms:.1f} ms > 150 ms"
