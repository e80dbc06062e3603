"""GPU tests: every entry point across the 32-bit boundaries of a large stack ("Size limits").

Each case is the smallest stack that crosses its boundary, generated on the device from a seed, and each test first asserts
that the crossing happened.  Nothing is compared with itself:
  * decode: the pixels, byte for byte over the whole stack, on the device;
  * encode: frames are independent and start on a byte, so the stream must be the concatenation of encodes of chunks of at most
    256 frames (a size the parity tests pin to the oracle) and the offsets their running sums; the oracle's bytes for the first
    and the last frame and the frames on either side of every crossing;
  * consumers: the same operation in plain torch, int64, from the pixels (gpu_support.consumer_truths), every element;
  * every output lies in a guarded allocation (gpu_support.DeviceGuarded) and every call's status word 0 is checked.
A test computes its need of device memory and FAILS where less is free; it frees its tensors at its end.

  A   2100 x 512^2 uint8 uniform, 5100 x 512^2 uint16 Poisson(3)      stream bit 2^32 (0.41 bytes a value: 4200 fall short)
  B   4160 x 512^2 uint32 uniform                                       stream byte 2^31 and 2^32, pixel byte 2^32
  C   16 500 x 512^2 uint8, sparse                                      value index 2^31 and 2^32
  D1  70 001 frames of 40 uint8                                         frame count above 16-bit grid dimensions
  D2  2^24 + 3 frames of 8 uint8: refused by every entry point          tile count 2^24 = 2^32 threads (TRPX_MAX_TILES_PER_CALL)
  E1  2 x 11 008^2 uint32 uniform                                       just below frame_bits_fit_32: in-frame positions to 3.9 Gbit
  E2  2 x 11 100^2, E3  2 x 11 600^2                                    above it; real frame bits > 2^32

Wall time of each test on an MI355X (pytest --durations, the call alone): D1 2.1 s, A uint8 4.0 s, A uint16 3.6 s, A host round
trip 0.8 s, E1 4.6 s, E2 2.1 s, E3 2.3 s, B 2.3 s, C 1.3 s, D2 under a second.

What these tests found.  Fixed with them: the two-pass encoder (trpx_set_encode_path(1), encode.hip) wrote a wrong stream for
8-bit stacks of a few hundred tiles and more -- right offsets, wrong bytes at block and tile edges, differently from run to run
(40 x 512^2 uint8: 176 916 of 10 594 982 bytes; 70 001 x 40: 1652 bytes in 636 frames); D1, A uint8 and C check it in
check_two_pass.  And a stack of 2^24 tiles or more reached launches the device cannot start (D2).

And the serial walker of a frame's headers (walk_lds.hpp: the walk of the frames whose position-parallel walk does not converge)
tested its window in 32 signed bits: for this pair of 11 008^2 uint32 frames (seed 11039; 3 887 757 296 bits a frame) trpx_decode
answered status 5 (TRPX_ERR_CORRUPT) and no pixels on the auto, frames, dense and tiles routes and trpx_build_index answered 5,
while the same geometry from seed 11008, whose walks all converge, decoded on every route (E1).
"""
import numpy as np
import pytest

from gpu_support import ROUTES, ConsumerSpec, DeviceGuarded, assert_same_index, assert_stream_is_chunks, consumer_truths, crossing_frames
from gpu_support import encode, frame_chunks, host_decode, host_encode, input_forms, keep_from, need_device_memory, same_bytes, selected
from gpu_support import signed_view, status_block, to_np, wide

pytestmark = pytest.mark.gpu

GiB = 1 << 30
N512 = 512 * 512
UNSUPPORTED = 2


# ---- the stacks, on the device ----------------------------------------------------------------------------------------------------
def _gen(gpu, seed):
    import torch
    g = torch.Generator(device=gpu)
    g.manual_seed(seed)
    return g


def uniform(gpu, tdt, frames, n, seed):
    """Uniform over the whole range of an unsigned type: random bytes, viewed"""
    import torch
    size = torch.empty(0, dtype=tdt).element_size()
    return torch.randint(0, 256, (frames, n * size), dtype=torch.uint8, device=gpu, generator=_gen(gpu, seed)).view(tdt)


def sparse_counts(gpu, frames, n, seed):
    """uint8 Poisson(0.05) by inverse CDF, one pixel in 4096 bright (200 + frame % 50): a small stream for many values"""
    import torch
    g = _gen(gpu, seed)
    out = torch.empty((frames, n), dtype=torch.uint8, device=gpu)
    cdf = np.cumsum([np.exp(-0.05) * 0.05 ** k / np.prod(np.arange(1, k + 1)) for k in range(4)])
    for a in range(0, frames, 128):
        b = min(a + 128, frames)
        r = torch.rand((b - a, n), device=gpu, generator=g)
        v = sum((r >= float(c)).to(torch.uint8) for c in cdf)
        bright = (200 + torch.arange(a, b, device=gpu) % 50).to(torch.uint8)[:, None].expand(b - a, n)
        out[a:b] = torch.where(r < 2.0 ** -12, bright, v)
    return out


# ---- one stack and what is asked of it -------------------------------------------------------------------------------------------
class Stack:
    def __init__(self, gpu, px, width, label):
        import torch
        self.gpu, self.px, self.width, self.label = gpu, px, width, label
        self.F, self.n = px.shape
        self.tdt = px.dtype
        self.enc = encode(px, index=True)                    # trpx_encode_indexed, the single-pass path
        self.stack, self.offs = self.enc.stack(), self.enc.frame_offsets
        torch.cuda.synchronize()

    def cross(self, offs, boundaries):
        """The crossing frames (gpu_support.crossing_frames; raises where there is no crossing)"""
        self.at, self.picks = crossing_frames(offs, boundaries)
        return self.at


def _ok(status, what):
    import torch
    torch.cuda.synchronize()
    assert int(status[0]) == 0, (what, "status", int(status[0]))


def check_encode(S, oracle, chunk=256, oracle_frames=None, chunk_fn=None):
    """The stream against chunk-wise encodes and the oracle."""

    def enc_chunk(f0, f1):
        e = encode(S.px[f0:f1], index=False)
        return e.stack(), e.frame_offsets
    assert_stream_is_chunks(S.stack, S.offs, S.F, chunk_fn or enc_chunk, chunk, S.label)
    offs = to_np(S.offs)
    for f in S.picks if oracle_frames is None else oracle_frames:
        want, _ = oracle.encode(to_np(S.px[f]))
        got = to_np(S.stack[int(offs[f]):int(offs[f + 1])])
        assert got.size == want.size and (got == want).all(), (S.label, "frame", f, "differs from the oracle's bytes")


def check_two_pass(S):
    """The two-pass encoder (trpx_set_encode_path(1)) and the index it builds: the bytes check_encode has compared."""
    import torch
    from trpx_amd import codec
    with selected("trpx_set_encode_path", 1):
        two = codec.encode(S.px, index=True if S.enc.index is not None else None)
        torch.cuda.synchronize()
    assert torch.equal(two.frame_offsets, S.offs), (S.label, "two-pass offsets")
    assert same_bytes(two.stack(), S.stack), (S.label, "two-pass stream")
    two.check()
    assert two.prolix_bits() == S.enc.prolix_bits()
    if S.enc.index is not None and two.index is not None:
        assert_same_index(two.index, S.enc.index, S.n, S.F, (S.label, "two-pass index"))
    del two


def check_decode(S, routes=ROUTES, indexed=True, locator=False):
    """trpx_decode on auto and every forced route, trpx_decode_indexed and trpx_build_index: the pixels back, whole stack."""
    import torch
    from trpx_amd import codec
    out = DeviceGuarded((S.F, S.n), S.tdt, S.gpu)
    ws = codec.Workspace(S.gpu)
    for name, value in [("auto", 0)] + sorted(routes.items()):
        out.poison()
        st = status_block()
        with selected("trpx_set_decode_path", value):
            codec.decode(S.stack, S.offs, S.n, S.F, S.tdt, out=out.view, status=st, workspace=ws)
            _ok(st, (S.label, "decode", name))
        assert same_bytes(out.check(f"decode {name}"), S.px), (S.label, "decode", name, "pixels differ")
    if locator:                                              # frame_offsets = NULL: the frames are located first
        out.poison()
        st = status_block()
        codec.decode(S.stack, None, S.n, S.F, S.tdt, out=out.view, status=st, workspace=ws)
        _ok(st, (S.label, "decode without offsets"))
        assert same_bytes(out.check("decode without offsets"), S.px), (S.label, "decode without offsets")
    if indexed:
        built = codec.build_index(S.stack, S.offs, S.n, S.F, S.tdt)
        torch.cuda.synchronize()
        for what, index in (("the encoder's index", S.enc.index), ("trpx_build_index", built)):   # each index decodes to the pixels
            out.poison()
            st = status_block()
            codec.decode(S.stack, S.offs, S.n, S.F, S.tdt, out=out.view, status=st, index=index)
            _ok(st, (S.label, "decode_indexed", what))
            assert same_bytes(out.check(what), S.px), (S.label, "decode_indexed", what)
        assert_same_index(built, S.enc.index, S.n, S.F, (S.label, "build_index"))
        del built
    ws.release()
    del out


def check_convert(S, out_tdt):
    """trpx_decode_convert into a wider type: the values, whole stack."""
    import torch
    from trpx_amd import _lib
    from trpx_amd.codec import dtype_code
    L = _lib.lib()
    out = DeviceGuarded((S.F, S.n), out_tdt, S.gpu)
    ws = torch.empty(L.trpx_decode_workspace_bytes(dtype_code(out_tdt), S.n, S.F, 12), dtype=torch.uint8, device=S.gpu)
    st = status_block()
    _lib.check(L.trpx_decode_convert(0, dtype_code(out_tdt), S.stack.data_ptr(), S.stack.numel(), S.offs.data_ptr(), S.n, S.F, 12,
                                     out.view.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    _ok(st, (S.label, "decode_convert"))
    got = out.check("decode_convert")
    for a, b in frame_chunks(0, S.F, S.n):
        assert torch.equal(wide(got[a:b]), wide(S.px[a:b])), (S.label, "decode_convert", "frames", a, b)
    del out, ws


def check_select(S):
    """trpx_select_frames: frames from both sides of every crossing, out of order, one twice -- the encode of those pixels."""
    import torch
    from trpx_amd import codec
    ks = sorted(S.at.values())
    want = [min(ks[-1] + 1, S.F - 1), 0, max(ks[0] - 1, 0), S.F - 1] + ks + [min(ks[-1] + 1, S.F - 1)]
    frames = torch.tensor(want, dtype=torch.int32, device=S.gpu)
    sel = codec.select_frames(S.stack, S.offs, frames, S.n, S.F, S.tdt, index=S.enc.index)
    sel.check()
    ref = encode(signed_view(S.px)[frames.to(torch.int64)].contiguous().view(S.tdt), index=True)
    assert torch.equal(sel.frame_offsets, ref.frame_offsets), (S.label, "select offsets", want)
    assert same_bytes(sel.stack(), ref.stack()), (S.label, "select bytes", want)
    assert_same_index(sel.index, ref.index, S.n, len(want), (S.label, "select index"))


def spec_for(S, group, n_out=4, n_maps=3, n_bins=5, bin=(8, 8), threshold=255):
    import torch
    dev, n = S.gpu, S.n
    f = torch.arange(S.F, dtype=torch.int64, device=dev)
    labels = (f * 7 + f // max(1, S.F // 3)) % (n_out + 1)   # label n_out: the frame is in no sum
    labels[-1] = 0                                           # the last frame is in one
    p = torch.arange(n, dtype=torch.int64, device=dev)
    maps = [torch.ones(n, dtype=torch.int64, device=dev), p % S.width - S.width // 2, (p * 2654435761 >> 7) % 2001 - 1000]
    weights = torch.stack(maps[:n_maps]).to(torch.int32)
    pixel_labels = ((p // 5) % (n_bins + 1)).to(torch.int16)  # label n_bins: the pixel is in no bin
    return ConsumerSpec(group, labels, n_out, weights, pixel_labels, n_bins, S.width, bin, threshold)


ALL = ("sum", "reduce", "sum_labelled", "roi", "sparse", "dot", "bins", "binned", "encode_sparse")


def check_consumers(S, spec, forms, box=(16, 16), which=ALL):
    """Every consumer in every input form against consumer_truths; roi and sparse have boxes and events on both sides of every
    crossing and in the last frame (asserted); trpx_encode_sparse from the events must give the stack of the kept pixels."""
    import torch
    from trpx_amd import codec
    i64, F, n, dt = torch.int64, S.F, S.n, S.tdt
    t = consumer_truths(S.px, spec)
    n_g = t["sum"].shape[0]
    H = n // S.width
    bh, bw = box
    frames = sorted(set(S.picks))
    boxes = [(f, (7 * i) % (H - bh + 1), (13 * i) % (S.width - bw + 1)) for i, f in enumerate(frames)] + [(F - 1, H - bh, S.width - bw), (0, 0, 0)]
    roi_truth = torch.stack([signed_view(S.px[f]).view(H, S.width)[y:y + bh, x:x + bw] for f, y, x in boxes]).view(S.tdt)
    boxes_dev = torch.tensor(boxes, dtype=torch.int32, device=S.gpu)
    n_events = int(t["rows"][-1])
    per_frame = t["rows"][1:] - t["rows"][:-1]
    for f in frames:
        assert int(per_frame[f]) > 0, (S.label, "no event in frame", f, "at threshold", spec.threshold)
    ws = codec.Workspace(S.gpu)
    events = None
    for mode in forms:
        offs, index = input_forms(S.enc, mode)
        kw = dict(index=index, workspace=ws)
        ctx = (S.label, mode)

        def run(what, shape, tdt, call, truth):
            out = DeviceGuarded(shape, tdt, S.gpu)
            st = status_block()
            call(out.view, st)
            _ok(st, ctx + (what,))
            got = out.check(what)
            assert torch.equal(wide(got), truth), ctx + (what, "differs from the torch truth")
        if "sum" in which:
            run("sum", (n_g, n), i64, lambda o, st: codec.decode_sum(S.stack, offs, n, F, dt, spec.group, out_dtype=i64, out=o, status=st, **kw), t["sum"])
        if "reduce" in which:
            run("reduce max", (n_g, n), dt, lambda o, st: codec.decode_reduce(S.stack, offs, n, F, dt, spec.group, "max", out=o, status=st, **kw), t["max"])
            run("reduce sumsq", (n_g, n), torch.uint64, lambda o, st: codec.decode_reduce(S.stack, offs, n, F, dt, spec.group, "sumsq", out=o, status=st, **kw), t["sumsq"])
        if "sum_labelled" in which:
            counts = DeviceGuarded((spec.n_out,), torch.int32, S.gpu)
            lab32 = spec.frame_labels.to(torch.int32)
            run("sum_labelled", (spec.n_out, n), i64, lambda o, st: codec.decode_sum_labelled(S.stack, offs, n, F, dt, lab32, spec.n_out, out_dtype=i64, out=o,
                                                                                               counts=counts.view, status=st, **kw), t["labelled"])
            assert torch.equal(wide(counts.check("counts")), t["counts"]), ctx + ("sum_labelled counts",)
        if "dot" in which:
            run("dot", (F, spec.weights.shape[0]), i64, lambda o, st: codec.decode_dot(S.stack, offs, n, F, dt, spec.weights, out=o, status=st, **kw), t["dot"])
        if "bins" in which:
            lab16 = spec.pixel_labels.view(torch.uint16) if spec.pixel_labels.dtype == torch.int16 else spec.pixel_labels
            run("bins", (F, spec.n_bins), i64, lambda o, st: codec.decode_bins(S.stack, offs, n, F, dt, lab16, spec.n_bins, out=o, status=st, **kw), t["bins"])
        if "binned" in which:
            run("binned", tuple(t["binned"].shape), i64, lambda o, st: codec.decode_binned(S.stack, offs, n, F, dt, S.width, spec.bin, out_dtype=i64, out=o, status=st, **kw),
                t["binned"])
        if "roi" in which:
            out = DeviceGuarded(tuple(roi_truth.shape), dt, S.gpu)
            st = status_block()
            codec.decode_roi(S.stack, offs, n, F, dt, S.width, boxes_dev, box, out=out.view, status=st, **kw)
            _ok(st, ctx + ("roi",))
            assert same_bytes(out.check("roi"), roi_truth), ctx + ("roi", boxes)
        if "sparse" in which:
            rows = DeviceGuarded((F + 1,), i64, S.gpu)
            pos = DeviceGuarded((n_events,), torch.uint32, S.gpu)
            val = DeviceGuarded((n_events,), dt, S.gpu)
            st = status_block()
            codec.decode_sparse(S.stack, offs, n, F, dt, spec.threshold, capacity=n_events, row_offsets=rows.view, positions=pos.view, values=val.view,
                                status=st, **kw)
            _ok(st, ctx + ("sparse",))
            assert torch.equal(rows.check("row_offsets"), t["rows"]), ctx + ("sparse row offsets",)
            assert torch.equal(wide(pos.check("positions")), t["positions"]), ctx + ("sparse positions",)
            assert torch.equal(wide(val.check("values")), t["values"]), ctx + ("sparse values",)
            events = (rows, pos, val)
    if "encode_sparse" in which and events is not None:
        rows, pos, val = events
        es = codec.encode_sparse(rows.view, pos.view, val.view, n, F, dt)
        es.check()

        def kept_chunk(f0, f1):
            e = encode(keep_from(S.px[f0:f1], spec.threshold), index=False)
            return e.stack(), e.frame_offsets
        assert_stream_is_chunks(es.stack(), es.frame_offsets, F, kept_chunk, 256, (S.label, "encode_sparse"))
    ws.release()


def _finish():
    import torch
    torch.cuda.empty_cache()


# ---- D1: more frames than a 16-bit grid dimension ------------------------------------------------------------------------------------
def test_d1_70001_tiny_frames(gpu, oracle):
    import torch
    need_device_memory(1 * GiB, "D1")
    F, n = 70001, 40
    S = Stack(gpu, uniform(gpu, torch.uint8, F, n, 11), 8, "D1")
    assert F > 65535
    S.cross(np.arange(F + 1), [65535, 65536])
    check_encode(S, oracle)
    check_decode(S, locator=True)
    check_convert(S, torch.uint32)
    check_select(S)
    check_consumers(S, spec_for(S, group=F // 3, bin=(5, 8), threshold=200), ("index", "offsets", "none"), box=(2, 3))
    check_two_pass(S)
    del S
    _finish()


# ---- A: stream bit 2^32 ------------------------------------------------------------------------------------------------------------------
def _case_a(gpu, oracle, px, label, threshold, wider):
    S = Stack(gpu, px, 512, label)
    assert 8 * int(S.offs[-1]) > 2 ** 32, (label, "the stream does not cross bit 2^32", int(S.offs[-1]))
    S.cross(S.offs, [2 ** 32 // 8])
    check_encode(S, oracle)
    check_decode(S, locator=True)
    check_convert(S, wider)
    check_select(S)
    check_consumers(S, spec_for(S, group=-(-S.F // 4), threshold=threshold), ("index", "offsets", "none"))
    check_two_pass(S)
    del S
    _finish()


def test_a_uint8_uniform_stream_bit_2_32(gpu, oracle):
    import torch
    need_device_memory(6 * GiB, "A (uint8)")
    _case_a(gpu, oracle, uniform(gpu, torch.uint8, 2100, N512, 21), "A u8", 255, torch.uint16)


def test_a_uint16_poisson_stream_bit_2_32(gpu, oracle):
    import torch
    from trpx_amd import workloads
    need_device_memory(12 * GiB, "A (uint16 Poisson)")
    _case_a(gpu, oracle, workloads.poisson_u16(3.0, 0, 5100, N512, device=gpu), "A u16 Poisson(3)", 64, torch.uint32)


def test_a_host_round_trip_stream_bit_2_32(gpu):
    """trpx_encode_host / trpx_decode_host on the uint8 stack of case A: the device call's bytes, the pixels back."""
    import torch
    need_device_memory(4 * GiB, "A (host round trip)")
    px = uniform(gpu, torch.uint8, 2100, N512, 21)
    enc = encode(px, index=False)
    host_px = to_np(px)
    stream, offs, pb = host_encode(host_px)
    assert 8 * int(offs[-1]) > 2 ** 32
    assert (offs.astype(np.int64) == to_np(enc.frame_offsets)).all() and pb == enc.prolix_bits()
    assert same_bytes(to_np(enc.stack()), stream), "trpx_encode_host differs from trpx_encode"
    back = host_decode(stream, offs, N512, 2100, np.uint8)
    assert same_bytes(back, host_px), "trpx_decode_host: pixels differ"
    del px, enc
    _finish()


# ---- E: frames around the frame_bits_fit_32 line ------------------------------------------------------------------------------------------
def _case_e(gpu, oracle, side, label):
    import torch
    n = side * side
    S = Stack(gpu, uniform(gpu, torch.uint32, 2, n, 31 + side), side, label)
    S.cross(np.arange(3), [1])
    return S, n


def _encode_e(S, oracle):
    """Two frames are one chunk: the oracle's bytes for the second frame, which starts behind the first, and each frame's own
    one-frame encode for the other."""
    check_encode(S, oracle, chunk=1, oracle_frames=[1])


def test_e1_just_below_the_32_bit_frame_line(gpu, oracle):
    import torch
    need_device_memory(14 * GiB, "E1")
    S, n = _case_e(gpu, oracle, 11008, "E1")
    assert 33 * n < 0xF0000000
    assert 8 * int(S.offs[1] - S.offs[0]) > 3.85e9          # in-frame positions up to about 3.9 Gbit
    _encode_e(S, oracle)
    check_decode(S)
    check_consumers(S, spec_for(S, group=2, n_out=1, n_maps=2, n_bins=1, bin=(64, 64), threshold=2 ** 32 - 2 ** 12), ("index", "offsets"),
                    which=("sum", "roi", "sparse", "dot"))
    check_two_pass(S)
    del S
    _finish()


def _refused(call, what):
    from trpx_amd import _lib
    with pytest.raises(_lib.TrpxError) as e:
        call()
    assert e.value.code == UNSUPPORTED, (what, e.value)


def _index_entry_points_refuse(S, spec):
    """Whatever works on a decode index answers TRPX_ERR_UNSUPPORTED for this geometry."""
    import torch
    from trpx_amd import codec
    F, n, dt, i64 = S.F, S.n, S.tdt, torch.int64
    tiny = torch.zeros(64, dtype=i64, device=S.gpu)
    boxes = torch.zeros((1, 3), dtype=torch.int32, device=S.gpu)
    lab = torch.zeros(F, dtype=torch.int32, device=S.gpu)
    lab16 = torch.zeros(n, dtype=torch.uint16, device=S.gpu)
    w = torch.ones((1, n), dtype=torch.int32, device=S.gpu)
    _refused(lambda: codec.build_index(S.stack, S.offs, n, F, dt), "build_index")
    _refused(lambda: codec.decode_sum(S.stack, S.offs, n, F, dt, 2, out_dtype=i64, out=tiny), "sum")
    _refused(lambda: codec.decode_reduce(S.stack, S.offs, n, F, dt, 2, "max", out=torch.zeros((1, n), dtype=dt, device=S.gpu)), "reduce")
    _refused(lambda: codec.decode_sum_labelled(S.stack, S.offs, n, F, dt, lab, 1, out_dtype=i64, out=torch.zeros((1, n), dtype=i64, device=S.gpu)), "sum_labelled")
    _refused(lambda: codec.decode_roi(S.stack, S.offs, n, F, dt, S.width, boxes, (2, 2)), "roi")
    _refused(lambda: codec.decode_sparse(S.stack, S.offs, n, F, dt, 2 ** 32 - 1, capacity=64), "sparse")
    _refused(lambda: codec.decode_dot(S.stack, S.offs, n, F, dt, w), "dot")
    _refused(lambda: codec.decode_bins(S.stack, S.offs, n, F, dt, lab16, 1), "bins")
    _refused(lambda: codec.decode_binned(S.stack, S.offs, n, F, dt, S.width, (64, 64), out_dtype=i64,
                                         out=torch.zeros((F, -(-S.width // 64), -(-S.width // 64)), dtype=i64, device=S.gpu)), "binned")


def _above_the_line(gpu, oracle, side, label, real_bits):
    import torch
    from trpx_amd import codec
    need_device_memory(10 * GiB, label)
    n = side * side
    assert 33 * n >= 0xF0000000
    px = uniform(gpu, torch.uint32, 2, n, 31 + side)
    enc = codec.encode(px)                                   # (no index: a walk of such frames is what is refused)
    enc.check()
    S = Stack.__new__(Stack)
    S.gpu, S.px, S.width, S.label, S.F, S.n, S.tdt, S.enc = gpu, px, side, label, 2, n, px.dtype, enc
    S.stack, S.offs = enc.stack(), enc.frame_offsets
    S.cross(np.arange(3), [1])
    if real_bits:
        assert 8 * int(S.offs[1] - S.offs[0]) > 2 ** 32
    _encode_e(S, oracle)
    check_decode(S, indexed=False)
    _index_entry_points_refuse(S, None)
    check_two_pass(S)
    del S, px, enc
    _finish()


def test_e2_just_above_the_32_bit_frame_line(gpu, oracle):
    _above_the_line(gpu, oracle, 11100, "E2", False)


def test_e3_frames_of_more_than_2_32_bits(gpu, oracle):
    _above_the_line(gpu, oracle, 11600, "E3", True)


# ---- B: stream bytes 2^31 and 2^32, pixel byte 2^32 ----------------------------------------------------------------------------------------
def test_b_uint32_uniform_stream_and_pixel_byte_2_32(gpu, oracle):
    import torch
    from trpx_amd import codec
    need_device_memory(20 * GiB, "B")
    S = Stack(gpu, uniform(gpu, torch.uint32, 4160, N512, 41), 512, "B")
    assert int(S.offs[-1]) > 2 ** 32 and S.px.numel() * 4 > 2 ** 32
    S.cross(S.offs, [2 ** 31, 2 ** 32])
    check_encode(S, oracle)
    located, st = codec.locate_frames(S.stack, S.n, S.F, S.tdt, status=status_block())
    _ok(st, "B locate_frames")
    assert torch.equal(located, S.offs), "B: trpx_locate_frames"
    del located
    check_decode(S)
    check_convert(S, torch.uint64)
    check_select(S)
    check_consumers(S, spec_for(S, group=-(-S.F // 4), threshold=2 ** 32 - 2 ** 21), ("index", "offsets"))
    check_two_pass(S)
    del S
    _finish()


# ---- C: value index 2^31 and 2^32 ----------------------------------------------------------------------------------------------------------
def test_c_sparse_uint8_value_index_2_32(gpu, oracle):
    import torch
    need_device_memory(20 * GiB, "C")
    F = 16500
    S = Stack(gpu, sparse_counts(gpu, F, N512, 51), 512, "C")
    assert F * S.n > 2 ** 32
    S.cross(np.arange(F + 1, dtype=np.int64) * S.n, [2 ** 31, 2 ** 32])
    check_encode(S, oracle)
    check_decode(S)
    check_convert(S, torch.uint16)
    check_select(S)
    check_consumers(S, spec_for(S, group=-(-F // 4), threshold=100), ("index", "offsets"))
    check_two_pass(S)
    del S
    _finish()


# ---- D2: the grid limit ------------------------------------------------------------------------------------------------------------------
def test_d2_beyond_the_grid_limit_every_entry_point_refuses(gpu):
    """2^24 + 3 frames of one tile (8 uint8 values): TRPX_ERR_UNSUPPORTED from every device entry point, decided before any device
    call -- a launch of 2^32 threads would answer TRPX_ERR_HIP.  The C ABI directly, every pointer into one small device buffer:
    the wrappers of trpx_amd.codec would size a workspace for the stack first, and the decode workspace of 16.7 M frames is 128 GiB
    (which is also why the largest stack that is taken, 2^24 - 1 frames, is not run here)."""
    import torch
    from trpx_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)
    P, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    F, n, TB, BIG = 2 ** 24 + 3, 8, 1 << 40, 1 << 50
    U8, I64 = _lib.U8, _lib.I64
    calls = {
        "trpx_encode": lambda: L.trpx_encode(U8, P, n, F, 12, P, BIG, P, P, P, BIG, st),
        "trpx_encode_indexed": lambda: L.trpx_encode_indexed(U8, P, n, F, 12, P, BIG, P, P, P, P, BIG, st),
        "trpx_decode": lambda: L.trpx_decode(0, U8, P, TB, P, n, F, 12, P, P, P, BIG, st),
        "trpx_decode without offsets": lambda: L.trpx_decode(0, U8, P, TB, None, n, F, 12, P, P, P, BIG, st),
        "trpx_decode_indexed": lambda: L.trpx_decode_indexed(0, U8, P, TB, P, P, n, F, 12, P, P, st),
        "trpx_decode_convert": lambda: L.trpx_decode_convert(0, _lib.U16, P, TB, P, n, F, 12, P, P, P, BIG, st),
        "trpx_build_index": lambda: L.trpx_build_index(U8, P, TB, P, n, F, 12, P, P, st),
        "trpx_locate_frames": lambda: L.trpx_locate_frames(P, TB, n, F, 12, 8, P, P, P, BIG, st),
        "trpx_select_frames": lambda: L.trpx_select_frames(U8, P, TB, P, None, n, F, 12, P, 4, P, BIG, P, None, P, P, BIG, st),
        "trpx_decode_sum": lambda: L.trpx_decode_sum(U8, I64, P, TB, P, None, n, F, 12, F, P, P, P, BIG, st),
        "trpx_decode_reduce": lambda: L.trpx_decode_reduce(U8, _lib.REDUCE_MAX, P, TB, P, None, n, F, 12, F, 0, P, P, P, BIG, st),
        "trpx_decode_sum_labelled": lambda: L.trpx_decode_sum_labelled(U8, I64, P, TB, P, None, n, F, 12, P, 4, P, None, P, P, BIG, st),
        "trpx_decode_roi": lambda: L.trpx_decode_roi(U8, P, TB, P, None, n, F, 12, 8, P, 1, 1, 2, P, P, P, BIG, st),
        "trpx_decode_sparse": lambda: L.trpx_decode_sparse(U8, P, TB, P, None, n, F, 12, 255, P, P, P, 64, P, P, BIG, st),
        "trpx_decode_dot": lambda: L.trpx_decode_dot(U8, P, TB, P, None, n, F, 12, P, 1, P, P, P, BIG, st),
        "trpx_decode_bins": lambda: L.trpx_decode_bins(U8, P, TB, P, None, n, F, 12, P, 1, P, P, P, BIG, st),
        "trpx_decode_binned": lambda: L.trpx_decode_binned(U8, I64, P, TB, P, None, n, F, 12, 8, 1, 8, P, P, P, BIG, st),
        "trpx_encode_sparse": lambda: L.trpx_encode_sparse(U8, P, None, None, 0, n, F, 12, P, BIG, P, P, P, BIG, st),
        "trpx_index_group_states": lambda: L.trpx_index_group_states(P, n, F, 12, P, st),
        "trpx_index_from_group_states": lambda: L.trpx_index_from_group_states(U8, P, TB, P, P, n, F, 12, P, P, st),
    }
    assert F * 256 >= 2 ** 32 and L.trpx_group_count(n, 12) == 1
    for path in (0, 1):                                      # (both encoders, every decode route: the refusal is in front of them all)
        with selected("trpx_set_encode_path", path):
            for name in ("trpx_encode", "trpx_encode_indexed"):
                assert calls[name]() == UNSUPPORTED, (name, path, L.trpx_last_error_string())
    for value in [0] + sorted(ROUTES.values()):
        with selected("trpx_set_decode_path", value):
            assert calls["trpx_decode"]() == UNSUPPORTED, ("trpx_decode", value, L.trpx_last_error_string())
    for name, call in calls.items():
        assert call() == UNSUPPORTED, (name, L.trpx_last_error_string())
        assert b"tiles in one call" in L.trpx_last_error_string(), (name, L.trpx_last_error_string())
    torch.cuda.synchronize()
    assert not bool(buf.any()), "a refused call wrote to the device"
    del buf
    _finish()
