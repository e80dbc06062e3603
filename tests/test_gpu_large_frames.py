"""GPU tests (-m gpu): frames of more than 32 K blocks, called through the C ABI, against the CPU oracle.  Bar: pixel-exact on
decode, whichever route a frame ends on, and a damaged frame reported or confined to its own pixels.

Reached: the index route's cuts, walks and repairs (decode_part.hip: k_chain_walk, k_part_repair, ChainVote), round 4's parts
route (decode_part_sel4.hip), both on part_walk.hpp; the walks header-dense frames are listed for (decode_seg.hip: k_seg_wg,
k_seg_fallback); trpx_decode_parts_per_frame; and the test builds weakparts, segfbgrid, alldense / segwgrounds / noclassify
and chain_timeout."""
import numpy as np
import pytest

from gpu_support import assert_round_trip, encode, run_case, run_variant, selected

pytestmark = pytest.mark.gpu


def test_large_frames_in_a_long_stack_take_the_tiled_path(gpu, oracle):
    """The per-frame decoder packs a block's bit position and width into 32 bits (units of < 2^26 bits worst case).  A
    stack whose frames' worst case is larger (1500 x 1500 int32: 74 Mbit) is cut into parts (decode_part.hip) or routed to
    the tiled kernels -- also when the per-frame path is forced -- and decodes exactly."""
    import torch
    from trpx_amd import codec
    frames, n = 130, 1500 * 1500
    px = codec.synth(np.int32, 5, frames, n, device=gpu)
    enc = encode(px, index=False)
    for f in (0, 64, 129):
        want, pb = oracle.encode(px[f].cpu().numpy())
        o = enc.frame_offsets.cpu().numpy()
        assert enc.stack()[int(o[f]): int(o[f + 1])].cpu().numpy().tobytes() == want.tobytes()
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, np.int32)
    torch.cuda.synchronize()
    assert_round_trip(back, st, px, "auto")
    run_case("frames_route_large.py", TRPX_DECODE_PATH="frames")             # the product library, the per-frame path forced


def _banded(px, rows, width, period, band, rng):
    """Header-dense bands (Poisson(1.5) counts: the block width flips with every other block) in a run-dominated frame."""
    a = px.reshape(rows, width).copy()
    for r0 in range(period // 2, rows, period):
        a[r0:r0 + band] = np.minimum(rng.poisson(1.5, a[r0:r0 + band].shape), 6).astype(px.dtype)
    return a.reshape(-1)


@pytest.mark.parametrize("dtype,rows,width,frames", [(np.uint16, 1030, 1065, 6), (np.int32, 1211, 997, 3), (np.uint8, 2048, 2048, 2),
                                                       (np.int16, 613, 1999, 33)])
def test_large_frames_are_cut_into_parts(gpu, oracle, dtype, rows, width, frames):
    """Frames of more than 32 K blocks are cut into parts (decode_part.hip, the index route; under selector 4
    decode_part_sel4.hip, round 4's parts route; both on part_walk.hpp: start states inside runs of
    equal widths, a counting walk per part, repairs of the links that did not close, the part table).  Run-dominated frames,
    frames with header-dense bands (cuts without a run to start in, parts that are too dense: the frame falls back to the
    position-parallel walk), a frame of noise; pixel counts that are no multiple of 12, frames that start anywhere in the
    stack.  Every frame must decode exactly; the stream is the oracle's (Terse.hpp:352-389 against :500-549)."""
    import torch
    from trpx_amd import codec
    rng = np.random.RandomState(rows)
    n = rows * width
    dt = np.dtype(dtype)
    base = oracle.synth(np.uint16, 3, frames, n).astype(np.int64)
    if dt.kind == "i":
        base = base - 3
    base = np.clip(base, np.iinfo(dt).min, np.iinfo(dt).max).astype(dt)
    for f in range(frames):
        if f % 3 == 1:
            base[f] = _banded(base[f], rows, width, 64, 6, rng)           # thin bands: the guess search reaches past them
        elif f % 3 == 2:
            base[f] = _banded(base[f], rows, width, 200, 60, rng)         # wide bands: plain guesses, dense parts
    if frames > 4:
        base[4] = np.minimum(rng.poisson(1.5, n), 6).astype(dt)           # all noise
    px = torch.from_numpy(base).to(gpu)
    enc = encode(px, index=False)
    o = enc.frame_offsets.cpu().numpy()
    for f in (0, 1, frames - 1):
        want, _ = oracle.encode(base[f])
        assert enc.stack()[int(o[f]): int(o[f + 1])].cpu().numpy().tobytes() == want.tobytes()
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dtype)
    torch.cuda.synchronize()
    assert_round_trip(back, st, px, "index route")
    # round 4's parts route (decode_part_sel4.hip: two walks; its header-dense frames are listed for the position-parallel walk, whose launches for a
    # list are one persistent kernel since round 5: k_seg_fallback) must give the same pixels
    with selected("trpx_set_decode_path", 4):
        back4, st4 = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dtype)
        torch.cuda.synchronize()
    assert_round_trip(back4, st4, px, "parts route")
    # a flipped bit in the middle of a large frame must not go unnoticed (every part checks the state it ends in)
    bad = enc.stack().clone()
    mid = int(o[1] + (o[2] - o[1]) // 2) if frames > 2 else int(o[0] + (o[1] - o[0]) // 2)
    bad[mid] ^= 0x10
    back2, st2 = codec.decode(bad, enc.frame_offsets, n, frames, dtype)
    torch.cuda.synchronize()
    got = back2.view(torch.uint8).reshape(frames, -1)
    assert int(st2[0].item()) == 5 or not torch.equal(got, px.view(torch.uint8).reshape(frames, -1))


def test_large_frames_every_part_link_repaired(gpu, oracle):
    """Both routes in a test build whose cuts never find a run to start in (make weakparts: -DTRPX_PART_FORCE_WEAK, decode_part.hip
    and decode_part_sel4.hip):
    every part starts on a chain that is not the frame's, every link is open, and k_part_repair has to count every part
    again from the true state up to the checkpoint where the chains have merged.  The frames change their width every 16
    blocks (a chain that is not the frame's merges at an explicit header it meets on a block start; in a frame of long runs
    it may not meet one before the part ends, and the frame then takes the other route -- which is why real cuts start
    inside runs).  The build counts its verdicts in the status block: no frame may fall back, every link must have been
    repaired, the pixels must be exact."""
    run_variant("weakparts", "weakparts_links.py")


def test_listed_large_frames_fallback_on_a_small_device(gpu, oracle):
    """k_seg_fallback (decode_seg.hip) synchronises its persistent grid with device-wide barriers, which needs every workgroup
    resident at once: the grid is sized by what the device holds (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs, halved,
    at most 1024).  Test build `segfbgrid`: a device that holds 24 (and k_seg_wg hands every header-dense frame back after one
    round, so that the listed frames ARE k_seg_fallback's).  Header-dense frames of 1030 x 1065 and 2048 x 520 pixels are listed
    by the large-frame routes and must come out exact through the 24-workgroup grid (status 0, no timeout)."""
    run_variant("segfbgrid", "segfb_small_grid.py")


def test_header_dense_large_frames_one_workgroup_each(gpu, oracle):
    """Header-dense stacks of LARGE frames (decode_part.hip: ChainVote -- more than one block in six of the voting frames' heads
    starts with an explicit header) are left alone by the serial part walkers, listed, and walked by k_seg_wg (decode_seg.hip):
    one workgroup of 2 / 4 / 8 wavefronts per frame, lane per segment, links in LDS (Terse.hpp:352-389 all the same).  Product
    build: Poisson(3) frames of the three workgroup shapes, signed and 32-bit pixels, every frame listed (status[2]), pixels
    exact, the index built from the stream and used; a stack of run-dominated frames is NOT listed; frames 0 and last against
    the oracle.  Test builds: `alldense` -- run-dominated synth-v1 frames are called header-dense, their links do not close in
    twenty rounds, k_seg_wg hands them back and k_seg_fallback walks them; `segwgrounds` -- every header-dense frame is handed
    back after one round; `noclassify` -- the serial walkers and their repairs on header-dense data (what the product does for
    stacks whose frame heads are blank)."""
    import torch
    from trpx_amd import codec, _lib, workloads
    L = _lib.lib()
    cases = [(700 * 700, 5, np.uint16), (1030 * 1065, 6, np.uint16), (1300 * 1000, 3, np.uint16), (1030 * 1065, 3, np.int16), (1200 * 900, 3, np.int32)]
    for n, frames, dt in cases:
        px = workloads.poisson_u16(3.0, 0, frames, n, device=gpu)
        if dt == np.int16: px = (px.view(torch.int16) - 3)
        if dt == np.int32: px = px.view(torch.int16).to(torch.int32) * 37 - 90
        assert L.trpx_decode_parts_per_frame(codec.dtype_code(dt), n, frames, 12) > 1
        enc = encode(px, index=False)
        offs = enc.frame_offsets.cpu().numpy()
        for f in (0, frames - 1):
            want = oracle.encode_stack(px[f:f + 1].cpu().numpy())[0]
            assert bytes(enc.data[int(offs[f]): int(offs[f + 1])].cpu().numpy()) == bytes(want), (n, f)
        back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt)
        torch.cuda.synchronize()
        s = st.cpu().numpy()
        assert s[0] == 0 and torch.equal(back, px), (n, dt, s)
        assert s[2] == frames, (n, dt, s)                     # every frame listed for k_seg_wg
        idx = codec.build_index(enc.stack(), enc.frame_offsets, n, frames, dt)
        back2, st2 = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dt, index=idx)
        torch.cuda.synchronize()
        assert_round_trip(back2, st2, px, (n, dt, "index"))
        del px, enc, back, back2, idx
    px = codec.synth(np.uint16, 3, 6, 1030 * 1065, device=gpu)
    enc = encode(px, index=False)
    back, st = codec.decode(enc.stack(), enc.frame_offsets, 1030 * 1065, 6, np.uint16)
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and int(st[2]) == 0 and torch.equal(back, px), st.tolist()
    del enc, back
    # mixed stacks: the verdict is the stack's -- a run-dominated frame in a header-dense stack goes to k_seg_wg with the others (and
    # back to k_seg_fallback if its links do not close), a header-dense frame in a run-dominated stack stays with the serial walkers
    dense = workloads.poisson_u16(3.0, 0, 6, 1030 * 1065, device=gpu)
    for majority, odd in ((dense, px), (px, dense)):
        mix = majority.clone()
        mix[3] = odd[3]
        enc = encode(mix, index=False)
        back, st = codec.decode(enc.stack(), enc.frame_offsets, 1030 * 1065, 6, np.uint16)
        torch.cuda.synchronize()
        s = st.cpu().numpy()
        assert s[0] == 0 and torch.equal(back, mix), s
        assert (s[2] >= 5) if majority is dense else (s[2] <= 1), s    # (the odd frame's walkers may be through before the verdict is in)
        del mix, enc, back
    del px, dense
    for name in ("alldense", "segwgrounds", "noclassify"):
        run_variant(name, "header_dense_variants.py", name)


def test_many_large_frames_stay_whole(gpu, oracle):
    """Stacks of 768 frames and more keep frames of more than 32 K blocks on the per-frame route (one workgroup per frame,
    header-dense frames handed to the one-wavefront position-parallel walk) instead of cutting them into parts
    (encode_kernels.hpp: single_part_blocks; Terse.hpp:352-389 either way): 768 frames of 640 x 640 pixels -- 34 134 blocks --,
    Poisson(3) counts (every frame handed over) and synth-v1 (none), index-free decode, index built from the stream, decode
    with it; two frames against the oracle."""
    import torch
    from trpx_amd import codec, _lib, workloads
    n, frames = 640 * 640, 768
    assert _lib.lib().trpx_decode_parts_per_frame(codec.dtype_code(np.uint16), n, frames, 12) == 1
    assert _lib.lib().trpx_decode_parts_per_frame(codec.dtype_code(np.uint16), n, frames - 1, 12) > 1
    for kind in ("poisson3", "synth"):
        px = workloads.poisson_u16(3.0, 0, frames, n, device=gpu) if kind == "poisson3" else codec.synth(np.uint16, 5, frames, n, device=gpu)
        enc = encode(px, index=False)
        offs = enc.frame_offsets.cpu().numpy()
        for f in (0, frames - 1):
            want = oracle.encode_stack(px[f:f + 1].cpu().numpy())[0]
            assert bytes(enc.data[int(offs[f]): int(offs[f + 1])].cpu().numpy()) == bytes(want), (kind, f)
        back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, np.uint16)
        torch.cuda.synchronize()
        assert_round_trip(back, st, px, kind)
        idx = codec.build_index(enc.stack(), enc.frame_offsets, n, frames, np.uint16)
        back2, st2 = codec.decode(enc.stack(), enc.frame_offsets, n, frames, np.uint16, index=idx)
        torch.cuda.synchronize()
        assert_round_trip(back2, st2, px, (kind, "index"))
        del px, enc, back, back2, idx


def test_index_route_waits_are_bounded(gpu):
    """The index route's walk is ONE launch in which every part's wavefront waits for words its neighbours publish: the start
    state of the part behind (its walk ends there) and that part's walk record (the link into it) -- decode_part.hip,
    k_chain_walk.  The waits are bounded; a wavefront that gives up reports a bad walk / a failed link and the frame takes the
    position-parallel route.  Test build (make chain_timeout): frame 0's part 3 never publishes its start state, frame 1's
    part 5 never its record, the bound is 2 ms.  Both frames must be handed over (status[2]), nothing may hang, the pixels
    are exact -- header-dense frames (every link open, records waited for) and frames whose cuts lie in runs."""
    run_variant("chain_timeout", "chain_timeout.py")


@pytest.mark.parametrize("dtype,lo,hi", [(np.uint16, 100, 108), (np.int32, 1000, 1024), (np.uint8, 192, 200), (np.int16, -300, -290)])
def test_large_frames_with_a_pedestal(gpu, oracle, dtype, lo, hi):
    """Raw detector counts sit on a pedestal: every pixel in [lo, hi).  Their constant payload bits pass the run test of the
    part cuts (decode_part.hip: header bits 1 at the run's stride) like header bits do, at twelve positions per constant bit
    and stride; the cuts have to tell the header among them (part_header_phase), or the frame must take another route and
    still decode exactly.  One run-dominated frame and one with a sprinkling of outliers per type."""
    import torch
    from trpx_amd import codec
    rng = np.random.RandomState(11)
    n, frames = 1030 * 1065 + 7, 5
    a = rng.randint(lo, hi, (frames, n)).astype(dtype)
    a[1::2, rng.randint(0, n, 300)] = lo + (hi - lo) * 3                   # outliers: explicit headers every few thousand blocks
    px = torch.from_numpy(a).to(gpu)
    enc = encode(px, index=False)
    want, _ = oracle.encode(a[1])
    o = enc.frame_offsets.cpu().numpy()
    assert enc.stack()[int(o[1]): int(o[2])].cpu().numpy().tobytes() == want.tobytes()
    back, st = codec.decode(enc.stack(), enc.frame_offsets, n, frames, dtype)
    torch.cuda.synchronize()
    assert_round_trip(back, st, px, (dtype, lo, hi))


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_large_frames_hostile_streams(gpu, oracle, dtype):
    """Frames of more than 32 K blocks are cut at positions whose chain state is GUESSED and walked from there by walks that
    tolerate anything (decode_part.hip) -- so what a damaged frame does to that route is tested on its own: one frame of a
    stack of six is overwritten (ones, zeroes, noise, a burst, its first / last byte, single bits, offsets that run
    backwards), everything else stays as the encoder wrote it.  The call must come back with status 0 or TRPX_ERR_CORRUPT
    -- CORRUPT whenever the damage is gross --, the frames that were not touched must decode exactly whenever it says 0
    (frames are independent: Terse.hpp:502-505), and the workspace must serve the next call (the hand-over list, the part
    tables and the stack statistics live in it)."""
    import torch
    from trpx_amd import codec, _lib
    n, frames, victim = 12 * 70000 + 5, 6, 2
    px = codec.synth(dtype, 0, frames, n, device=gpu)
    enc = encode(px, index=False)
    good = enc.stack().clone()
    offs = enc.frame_offsets.clone()
    o = offs.cpu().numpy()
    lo, hi = int(o[victim]), int(o[victim + 1])
    want, _ = oracle.encode(px[victim].cpu().numpy())
    assert good[lo:hi].cpu().numpy().tobytes() == want.tobytes()
    ws = codec.Workspace(gpu)
    view = torch.int32 if np.dtype(dtype).itemsize == 4 else torch.int16
    others = [f for f in range(frames) if f != victim]

    def run(stream, offsets=offs):
        back, st = codec.decode(stream, offsets, n, frames, dtype, workspace=ws)
        torch.cuda.synchronize()
        return back, int(st[0].item())

    def clean_call_still_works(after):
        back, s = run(good)
        assert s == 0 and torch.equal(back.view(view), px.view(view)), f"the workspace does not serve a clean call after: {after}"

    clean_call_still_works("nothing")
    g = torch.Generator().manual_seed(20260104)
    gross = {"ones": lambda b: b[lo:hi].fill_(0xFF), "zeroes": lambda b: b[lo:hi].zero_(),
             "noise": lambda b: b[lo:hi].copy_(torch.randint(0, 256, (hi - lo,), generator=g, dtype=torch.uint8).to(gpu)),
             "burst": lambda b: b[(lo + hi) // 2: (lo + hi) // 2 + 4096].copy_(torch.randint(0, 256, (4096,), generator=g, dtype=torch.uint8).to(gpu))}
    for what, spoil in gross.items():
        bad = good.clone()
        spoil(bad)
        assert torch.equal(bad[:lo], good[:lo]) and torch.equal(bad[hi:], good[hi:])          # (only the victim's bytes)
        back, s = run(bad)
        assert s == _lib.ERR_CORRUPT, (what, s)
        clean_call_still_works(what)
    # small damage: a flip in payload bits still parses (status 0, the victim's pixels differ); one in a header or a width does not
    positions = [lo, hi - 1] + [int(p) for p in torch.randint(lo, hi, (24,), generator=g)]
    seen = {0: 0, _lib.ERR_CORRUPT: 0}
    for k, p in enumerate(positions):
        bad = good.clone()
        bad[p] ^= 1 << (k % 8)
        back, s = run(bad)
        assert s in (0, _lib.ERR_CORRUPT), (p - lo, s)
        seen[s] += 1
        if s == 0:
            for f in others:
                assert torch.equal(back[f].view(view), px[f].view(view)), f"a flip in frame {victim} (byte {p - lo}) changed frame {f}"
    assert seen[_lib.ERR_CORRUPT] > 0 and seen[0] > 0, seen        # (both kinds occurred: the check on the other frames above has run)
    clean_call_still_works("single flips")
    # offsets that run backwards / past the stream: refused, not followed
    for what, k, v in (("backwards", victim + 1, lo - 5), ("past the end", frames, int(good.numel()) + 4096)):
        ob = offs.clone()
        ob[k] = v
        back, s = run(good, ob)
        assert s == _lib.ERR_CORRUPT, (what, s)
        clean_call_still_works(what)
