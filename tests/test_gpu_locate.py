"""GPU tests: trpx_locate_frames / codec.locate_frames -- the frames of an index-free stack located on the device
(decode_locate.hip) exactly where the serial walk of Terse.hpp:562-585 finds them.  The truth is the encoder's own offsets;
for hand-edited streams it is a serial locate on the CPU (the oracle's frame_bytes, or a plain Python port of the walk that
also applies max_bits and the stream's end, as the device walk does)."""
import ctypes as C
import io

import numpy as np
import pytest

from gpu_support import ALL_DTYPES as DTYPES
from gpu_support import encode

pytestmark = pytest.mark.gpu


def _locate(stack, n, frames, dtype):
    """stack: uint8 tensor on the GPU or numpy bytes -> (offsets np.int64, status np.int32)"""
    import torch
    from trpx_amd import codec
    if isinstance(stack, np.ndarray):
        stack = torch.from_numpy(np.ascontiguousarray(stack, dtype=np.uint8)).to("cuda:0")
    offs, st = codec.locate_frames(stack, n, frames, dtype)
    torch.cuda.synchronize()
    return offs.cpu().numpy(), st.cpu().numpy()


def _random_widths(dtype, frames, n, seed, gpu):
    """Blocks of random widths (half of them keep the previous block's width: explicit and implicit headers)."""
    import torch
    g = torch.Generator(device=gpu).manual_seed(seed)
    bits = 8 * np.dtype(dtype).itemsize
    nb = (n + 11) // 12
    w = torch.randint(0, bits + 1, (frames, nb), generator=g, device=gpu)
    keep = torch.rand((frames, nb), generator=g, device=gpu) < 0.5
    idx = torch.arange(nb, device=gpu).expand(frames, nb)
    src = torch.where(keep, torch.zeros_like(idx), idx).cummax(dim=1).values
    w = torch.gather(w, 1, src)
    wv = w.repeat_interleave(12, dim=1)[:, :n]
    v = torch.randint(0, 2**62, (frames, n), generator=g, device=gpu, dtype=torch.int64)
    v = v & ((torch.ones_like(wv) << wv) - 1)
    from trpx_amd import codec
    tdt = codec.torch_dtype(dtype)
    if tdt in (torch.uint8, torch.uint16, torch.uint32):
        return (v & ((1 << bits) - 1)).to(tdt)
    return _wrap_signed(v, bits).to(tdt)


def _wrap_signed(v, bits):
    v = v & ((1 << bits) - 1)
    return v - ((v >> (bits - 1)) << bits)


def py_locate(stream, n, frames, max_w, block=12):
    """The serial walk (Terse.hpp:360-372 per frame, S_f = 1 + bits/8) in Python: offsets, or None where the device walk reports
    TRPX_ERR_CORRUPT (a header past the stream, a width above max_w, a frame end past the stream)."""
    stream = np.asarray(stream, np.uint8)
    L = 8 * stream.size
    nb = (n + block - 1) // block
    nlast = n - (nb - 1) * block
    pad = np.concatenate([stream, np.zeros(8, np.uint8)])
    bitarr = np.unpackbits(pad, bitorder="little")

    def peek(p):
        return int(np.packbits(bitarr[p:p + 16], bitorder="little").view("<u2")[0])

    offs, fo = [0], 0
    for _ in range(frames):
        if fo >= stream.size:
            return None
        pos, w = 8 * fo, 0
        for b in range(nb):
            if pos >= L:
                return None
            x = peek(pos)
            nv = nlast if b == nb - 1 else block
            if x & 1:
                pos += 1 + nv * w
                continue
            nw, hl = (x >> 1) & 7, 4
            if nw == 7:
                nw += (x >> 4) & 3
                hl = 6
                if nw == 10:
                    nw += (x >> 6) & 63
                    hl = 12
            if nw > max_w:
                return None
            pos += hl + nv * nw
            w = nw
        bits = pos - 8 * fo
        if bits > L - 8 * fo or fo + 1 + bits // 8 > stream.size:
            return None
        fo += 1 + bits // 8
        offs.append(fo)
    return np.array(offs, np.int64)


# ---- 1. exactness across shapes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_locate_matches_encoder_across_shapes(gpu, dtype):
    cases = [(1, 300), (5, 300), (12, 300), (13, 300), (12 * 37 + 5, 300), (12 * 37 + 5, 7), (512 * 512, 7),
             (1030 * 1065, 2), (1, 1), (5, 2), (13, 7), (512 * 512, 1)]
    for i, (n, frames) in enumerate(cases):
        px = _random_widths(dtype, frames, n, 1000 * i + DTYPES.index(dtype), gpu)
        enc = encode(px, index=False)
        offs, st = _locate(enc.stack(), n, frames, dtype)
        assert st[0] == 0, (n, frames, st)
        assert (offs == enc.frame_offsets.cpu().numpy()).all(), (n, frames)


# ---- 2. adversarial content ------------------------------------------------------------------------------------------------

def test_locate_all_zero_and_saturated_frames(gpu):
    import torch
    n, frames = 512 * 512, 40
    for fill in (0, -1):
        px = torch.full((frames, n), fill, dtype=torch.int16, device=gpu).view(torch.uint16)
        enc = encode(px, index=False)
        offs, st = _locate(enc.stack(), n, frames, np.uint16)
        assert st[0] == 0 and (offs == enc.frame_offsets.cpu().numpy()).all(), fill


def test_locate_tiny_frames_between_header_dense_ones(gpu):
    import torch
    for n in (12 * 37 + 5, 512 * 512):
        frames = 60
        px = _random_widths(np.uint16, frames, n, 77, gpu)
        px.view(torch.int16)[0::2] = 0                                    # every other frame compresses to ~1 bit per block
        enc = encode(px, index=False)
        offs, st = _locate(enc.stack(), n, frames, np.uint16)
        assert st[0] == 0 and (offs == enc.frame_offsets.cpu().numpy()).all(), n


def test_locate_frames_with_a_whole_pad_byte(gpu):
    """Frames whose bit count is a multiple of 8 end in a zero byte of their own (S_f = 1 + bits/8)."""
    from oracle import oracle as O
    n, frames = 12 * 37 + 5, 200
    px = _random_widths(np.uint16, frames, n, 5, gpu)
    host = px.cpu().numpy()
    w = np.stack([O.widths(host[f]) for f in range(frames)]).astype(np.int64)
    wp = np.concatenate([np.zeros((frames, 1), np.int64), w[:, :-1]], axis=1)
    hl = np.where(w == wp, 1, np.where(w < 7, 4, np.where(w < 10, 6, 12)))
    nv = np.full(w.shape[1], 12)
    nv[-1] = n - 12 * (w.shape[1] - 1)
    bits = (hl + nv[None, :] * w).sum(axis=1)
    assert (bits % 8 == 0).sum() >= 5
    enc = encode(px, index=False)
    offs, st = _locate(enc.stack(), n, frames, np.uint16)
    assert st[0] == 0 and (offs == enc.frame_offsets.cpu().numpy()).all()


def test_locate_with_pad_bits_set(gpu):
    """Pad bits set to 1 where the frame still decodes the same: the pad is never read, the offsets stay the encoder's."""
    from oracle import oracle as O
    n, frames = 12 * 37 + 5, 120
    px = _random_widths(np.uint16, frames, n, 9, gpu)
    enc = encode(px, index=False)
    stack = enc.stack().cpu().numpy().copy()
    offs = enc.frame_offsets.cpu().numpy()
    host = px.cpu().numpy()
    changed = 0
    for f in range(frames):
        fr = stack[offs[f]:offs[f + 1]].copy()
        fr[-1] |= 0x80
        if O.frame_bytes(fr, n) == fr.size and (O.decode(fr, n, np.uint16) == host[f]).all():
            stack[offs[f + 1] - 1] |= 0x80
            changed += 1
    assert changed > frames // 4
    got, st = _locate(stack, n, frames, np.uint16)
    assert st[0] == 0 and (got == offs).all()


# ---- 3. full size ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["synth", "poisson3"])
def test_locate_full_size_stacks(gpu, kind):
    import torch
    from trpx_amd import codec, workloads
    n, frames = 512 * 512, 2000
    px = codec.synth(np.uint16, 0, frames, n, device=gpu) if kind == "synth" else workloads.poisson_u16(3.0, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    stack = enc.stack()
    offs, st = codec.locate_frames(stack, n, frames, np.uint16)
    torch.cuda.synchronize()
    assert int(st[0].item()) == 0
    assert torch.equal(offs, enc.frame_offsets)
    back, st_d = codec.decode(stack, offs, n, frames, np.uint16)
    torch.cuda.synchronize()
    assert int(st_d[0].item()) == 0 and torch.equal(back.view(torch.int16), px.view(torch.int16))


# ---- 4. hostile streams ----------------------------------------------------------------------------------------------------

def test_locate_hostile_streams(gpu):
    from trpx_amd import _lib
    n, frames = 12 * 85 + 7, 40
    px = _random_widths(np.uint16, frames, n, 21, gpu)
    enc = encode(px, index=False)
    stack = enc.stack().cpu().numpy().copy()
    offs = enc.frame_offsets.cpu().numpy()
    # truncated
    _, st = _locate(stack[: offs[-1] - 100], n, frames, np.uint16)
    assert st[0] == _lib.ERR_CORRUPT
    # a header bent to a width above max_bits (first block of frame 5: code 7 + 3 + 63 -> 73)
    bent = stack.copy()
    bent[offs[5]] = 0xFE
    bent[offs[5] + 1] |= 0x0F
    assert py_locate(bent, n, frames, 16) is None
    _, st = _locate(bent, n, frames, np.uint16)
    assert st[0] == _lib.ERR_CORRUPT
    # one more frame than present / one fewer
    _, st = _locate(stack, n, frames + 1, np.uint16)
    assert st[0] == _lib.ERR_CORRUPT
    got, st = _locate(stack, n, frames - 1, np.uint16)
    assert st[0] == 0 and (got == offs[:frames]).all()
    # bent frame ends in the middle of the stack: whatever the serial walk makes of them
    rng = np.random.default_rng(3)
    for trial in range(12):
        bent = stack.copy()
        f = int(rng.integers(10, 30))
        at = int(offs[f + 1]) - 1 - int(rng.integers(0, 6))
        bent[at] ^= np.uint8(1 << int(rng.integers(0, 8)))
        want = py_locate(bent, n, frames, 16)
        got, st = _locate(bent, n, frames, np.uint16)
        if want is None:
            assert st[0] == _lib.ERR_CORRUPT, trial
        else:
            assert st[0] == 0 and (got == want).all(), trial


# ---- 5. host and file paths ------------------------------------------------------------------------------------------------

def test_host_locate_and_stack_open_without_offsets(gpu):
    from trpx_amd import _lib
    L = _lib.lib()
    n, frames = 12 * 300 + 1, 300
    px = _random_widths(np.uint16, frames, n, 31, gpu)
    enc = encode(px, index=False)
    stack = np.ascontiguousarray(enc.stack().cpu().numpy())
    want = enc.frame_offsets.cpu().numpy().astype(np.uint64)
    got = np.zeros(frames + 1, np.uint64)
    _lib.check(L.trpx_frame_offsets_host(stack.ctypes.data, stack.size, n, frames, 12, 16, got.ctypes.data, 0))
    assert (got == want).all()
    h = C.c_void_p()
    _lib.check(L.trpx_stack_open(C.byref(h), 0, stack.ctypes.data, stack.size, None, None, n, frames, 12, 16, 0))
    try:
        host = px.cpu().numpy()
        out = np.zeros(n, np.uint16)
        for f in (0, 1, frames // 2, frames - 1):
            _lib.check(L.trpx_stack_read(h, f, _lib.U16, out.ctypes.data))
            assert (out == host[f]).all(), f
    finally:
        L.trpx_stack_close(h)


def test_index_free_file_reads_back(gpu):
    from trpx_amd.terse import Terse
    from trpx_amd import codec
    n, frames = 256 * 256, 64
    px = codec.synth(np.uint16, 3, frames, n, device=gpu).cpu().numpy().reshape(frames, 256, 256)
    t = Terse()
    t.push_back_stack(px)
    buf = io.BytesIO()
    t.write(buf, frame_index=False)
    buf.seek(0)
    back = Terse.read(buf)
    assert back.number_of_frames() == frames
    assert (back.prolix_stack(np.uint16).reshape(px.shape) == px).all()


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------

def test_locate_and_decode_capture_into_hip_graph(gpu):
    import torch
    from trpx_amd import codec, _lib
    n, frames = 512 * 512, 64
    px = codec.synth(np.uint16, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    stack = enc.stack().clone()
    ws_l, ws_d = codec.Workspace(gpu), codec.Workspace(gpu)
    L = _lib.lib()
    ws_l.get(L.trpx_locate_workspace_bytes(stack.numel(), n, frames, 12))
    ws_d.get(L.trpx_decode_workspace_bytes(_lib.U16, n, frames, 12))
    offs = torch.empty(frames + 1, dtype=torch.int64, device=gpu)
    st_l = torch.empty(8, dtype=torch.int32, device=gpu)
    st_d = torch.empty(8, dtype=torch.int32, device=gpu)
    back = torch.empty((frames, n), dtype=torch.uint16, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            codec.locate_frames(stack, n, frames, np.uint16, workspace=ws_l, status=st_l, out=offs)
            codec.decode(stack, offs, n, frames, np.uint16, out=back, workspace=ws_d, status=st_d)
    offs.zero_(); back.zero_(); st_l.fill_(-1); st_d.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert int(st_l[0].item()) == 0 and int(st_d[0].item()) == 0
    assert torch.equal(offs, enc.frame_offsets)
    assert torch.equal(back.view(torch.int16), px.view(torch.int16))
    offs.zero_(); back.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(offs, enc.frame_offsets) and torch.equal(back.view(torch.int16), px.view(torch.int16))
