// Only selector 4 of trpx_set_decode_path reaches this file (A/B only): round 4's parts route.  What it shares with
// the index route (decode_part.hip) -- the window, the walker, the recount -- is part_walk.hpp.
//
// PROLIX decode of LARGE frames on the per-frame route (gfx950 / CDNA4): cutting a frame into PARTS.
//
// The per-frame decoder (decode_frame.hip) puts one serial header walker (reference include/Terse.hpp:360-372: block b+1's
// position is only known after block b's header) and three extraction waves on a frame.  For the 22 K blocks of a 512 x 512
// frame that is the right grain; a 1030 x 1065 frame (91 K blocks) is a 4 x longer chain on 4 x fewer workgroups, a 2048 x
// 2048 frame (350 K blocks) 16 x -- 200 frames of 1030 x 1065 decoded at 0.13 of the HBM peak, 128 frames of 2048 x 2048 at
// 0.07 (on the tiled route).  A frame of more than kPartMaxBlocks blocks is therefore cut into P parts, every part a unit of
// work of its own for the per-frame decoder (k_decode_parts), which needs the chain state in front of every part: the
// bit position of its first block's header, the width of the block before it, and -- for the place of its pixels -- the
// number of its first block.  This file finds them, with the serial walker's own cheap steps (one per RUN of equal widths):
//
//   k_part_guess    a start state S_p for every part p >= 1.  The parts are cut at bit positions X_p = p * L.  Behind X_p the
//                   wavefront looks for a run of blocks that repeat their width: kPartEvid header bits 1 at stride 1 + 12 w
//                   (bit-parallel: 2048 candidate positions per width and pass); a position kPartSkip blocks inside such a
//                   run is a block start with all but certainty.  No run within 16 K bits: the plain (X_p, 0), which is
//                   almost surely not a state of the chain -- but a chain started there merges with the true one at the first
//                   explicit header it meets on a block start (its state after an explicit header does not depend on the
//                   width before, Terse.hpp:362-370).
//   k_part_walk     one wavefront per part p < P - 1 walks from S_p to the position of S_(p+1), counts the blocks and leaves
//                   the state it arrives in (OUT_p) plus a checkpoint (state, blocks so far) every few thousand bits.
//                   A part whose explicit headers are too dense for the serial walker (more than 1 in 6 blocks) stops:
//                   its frame is the position-parallel walk's case.
//   k_part_repair   one wavefront per link p -> p + 1 that is OPEN (OUT_p != S_(p+1)): the blocks of part p + 1 counted again
//                   from OUT_p -- only until this chain meets the one k_part_walk walked there (a checkpoint), which in
//                   run-dominated data is the next explicit header; the count follows from the checkpoint's.
//   k_part_resolve  one wavefront per frame.  S_0 = (0, 0) is true (Terse.hpp:359, :505); a chain that starts in a true state
//                   is true to its end; a link is closed, or repaired from the true OUT_p -- by induction every part's
//                   start state, block count and end state are the true chain's, the prefix sums of the counts are the
//                   parts' first blocks, and the part table is written.  A frame where this does not work out (a dense
//                   part, a repair that ran into another repair, a part of more than kPartMaxBlocks blocks, a corrupt
//                   stream) is listed as a whole for the route large frames took before (position-parallel walk + tiled
//                   extraction, decode_seg.hip): guesses and repairs only ever steer the speed, never the result -- and
//                   every part's decoder checks again that it ends in the next part's state, the last one that
//                   S_f = 1 + bits/8 (Terse.hpp:547).
//
// HBM traffic: the stream once more (walk only: no pixels), 0.2 of the algorithmic bytes of a u16 stack.
#include "part_walk.hpp"

namespace trpx {

struct PartFix {                               // what k_part_repair leaves per (frame, part 1 <= p < P - 1)
    uint32_t state;                            // 0: link closed, nothing done; 1: merged into the part's walk; 2: walked to T_p on its own; 3: failed
    uint32_t cnt, o_pos, o_w;                  // the part's block count (and, state 2, its end state) from the true start
};

uint32_t parts_per_frame(const FrameGeom& g, size_t n_frames) {
    if (g.n_blocks <= single_part_blocks(n_frames) || n_frames == 0) return 1u;
    // enough parts to fill the GPU one and a half times over (8 workgroups per CU), of 4 K .. 16 K blocks
    constexpr uint64_t want_total = 3072u, min_blocks = 4096u;
    const uint64_t p_min = (g.n_blocks + kPartBlocks - 1u) / kPartBlocks, p_max = g.n_blocks / min_blocks;
    const uint64_t p_want = (want_total + n_frames - 1u) / n_frames;
    const uint64_t hi = p_max > p_min ? p_max : p_min;
    const uint64_t P = p_want < p_min ? p_min : (p_want > hi ? hi : p_want);
    return (uint32_t)P;
}
struct PartWs { size_t states, walks, fixes, cks, total; };
static PartWs part_ws_layout(size_t n_frames, size_t P) {
    PartWs w;
    w.states = 0;
    w.walks = align_up(w.states + n_frames * P * sizeof(PartState), 256);
    w.fixes = align_up(w.walks + n_frames * (P - 1) * sizeof(PartWalk), 256);
    w.cks = align_up(w.fixes + n_frames * (P - 1) * sizeof(PartFix), 256);
    w.total = align_up(w.cks + n_frames * (P - 1) * kPartCk * sizeof(PartCk), 256);
    return w;
}
size_t part_workspace_bytes(const FrameGeom& g, size_t n_frames) {
    const size_t P = parts_per_frame(g, n_frames);
    return P > 1 ? part_ws_layout(n_frames, P).total : 0;
}

// A block start inside a run of equal widths at or behind frame bit X, or the plain guess.  kPartEvid header bits 1 at stride
// s = 1 + 12 w from some q in [X, X + 2048 kPartSearch) on -- 32 candidate positions per lane and AND chain, the widths in
// ascending order, for each of them the range in passes of 2048 positions -- make (q + kPartSkip * s, w) the state; inside a run of EMPTY blocks (every bit a
// header bit 1) X itself is one.  (Payload bits pass the test with probability 2^-32 per candidate, and the first kPartSkip
// of the evidence may be a neighbour's bits: a guess is only a guess, k_part_resolve verifies.  Pixels with a pedestal: part_header_phase, part_walk.hpp.)
// reach: the search (and the state it returns) stays inside [X, X + reach).
__device__ __forceinline__ PartState part_guess(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t* __restrict__ s_pm, uint32_t X, uint32_t limit,
                                                uint32_t max_w, uint32_t reach = 0xFFFFFFFFu, uint32_t max_passes = kPartSearch) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t s_max = 1u + (uint32_t)kBlock * max_w;
    const PartState plain{X, kPartWeak};
#ifdef TRPX_PART_FORCE_WEAK
    return plain;                              // test build (make weakparts): every link is open and goes through k_part_repair
#endif
    // the search range and its evidence lie inside one window: [X, X + 2048 kPartSearch + kPartEvid s_max) < 64 K bits
    static_assert(2048u * kPartSearch + kPartEvid * (1u + 12u * 32u) + 256u < 32u * (uint32_t)kPartChunkDw - 128u, "one window per guess");
    uint32_t passes = max_passes < kPartSearch ? max_passes : kPartSearch;
    while (passes && (uint64_t)X + 2048ull * passes + (uint64_t)kPartEvid * s_max + 128u > (uint64_t)limit) --passes;   // too close to the frame's end
    while (passes && 2048ull * passes + (uint64_t)kPartSkip * s_max > (uint64_t)reach) --passes;
    if (passes == 0u) return plain;
    part_fill(W, s_chunk, X);
    {
        const uint32_t a = lane < 4u ? part_bits(W, s_chunk, X + 32u * lane) : 0xFFFFFFFFu;
        if (!__ballot(a != 0xFFFFFFFFu)) return PartState{X, 0u};
    }
    // widths outside, passes inside: a stream whose runs are short (a change every ten blocks) has no run of kPartEvid blocks in
    // most passes, and all max_w widths of a pass without a hit cost 30 x what the first pass with a hit does
    // (widths above 8 get two passes: a cut without a run of a small width in reach is rare, and sweeping every width of a
    // 32-bit type over the whole range for it cost eight 4096 x 4096 int32 frames 70 of 100 us here)
    bool ambiguous = false;
    for (uint32_t w = 1; w <= max_w; ++w) {
        const uint32_t s = 1u + (uint32_t)kBlock * w;
        const uint32_t passes_w = w <= 8u || passes < 2u ? passes : (max_passes < kPartSearch ? 1u : 2u);
        for (uint32_t pass = 0; pass < passes_w; ++pass) {
            const uint32_t X0 = X + 2048u * pass;
            uint32_t a = 0xFFFFFFFFu;
            for (uint32_t k = 0; k < kPartEvid; k += 4u) {                   // (a wrong width's candidates are gone after a dozen bits)
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) a &= part_bits(W, s_chunk, X0 + 32u * lane + (k + i) * s);
                if (!__ballot(a != 0u)) break;
            }
            const uint64_t hits = __ballot(a != 0u);
            if (hits) {
                const int l0 = __builtin_ctzll(hits);
                const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)a, l0);
                const uint32_t r0 = 32u * (uint32_t)l0 + (uint32_t)__builtin_ctz(a0);
                __builtin_amdgcn_wave_barrier();
                s_pm[lane] = a;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const uint32_t h = part_header_phase(s_pm, r0, s, w);
                if (h != ~0u) return PartState{X0 + h + kPartSkip * s, w};
                ambiguous = true;               // (cannot tell the header here: the range's later passes, then other widths)
            }
        }
    }
    return ambiguous ? PartState{X, kPartWeak | kPartAmbig} : plain;
}

// A frame many of whose cuts found no run to start in (run-dominated stacks: one cut in a thousand) is header-dense: 1; one
// many of whose cuts found runs but not the headers in them is run-dominated with a problem (part_header_phase): 2; else 0.
__device__ __forceinline__ uint32_t part_frame_kind(const PartState* __restrict__ sf, uint32_t P) {
#ifdef TRPX_PART_FORCE_WEAK
    return 0u;
#endif
    uint32_t n_weak = 0, n_amb = 0;
    for (uint32_t q = (uint32_t)lane_id(); q < P; q += kWave) {
        const uint32_t w = sf[q].w;
        n_weak += (w & kPartWeak) != 0u && (w & kPartAmbig) == 0u ? 1u : 0u;
        n_amb += (w & kPartAmbig) != 0u ? 1u : 0u;
    }
    n_weak = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(n_weak), 63);
    n_amb = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(n_amb), 63);
    return 4u * n_weak > P ? 1u : (4u * n_amb > P ? 2u : 0u);
}

__global__ __launch_bounds__(kWave) void k_part_guess(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                      const uint64_t* __restrict__ frame_offsets, uint32_t max_w, uint32_t P,
                                                      PartState* __restrict__ states) {
    __shared__ __attribute__((aligned(16))) uint32_t s_chunk[kPartChunkDw + 4];
    __shared__ uint32_t s_pm[kWave + 2];
    const uint32_t frame = blockIdx.x / P, p = blockIdx.x % P;
    const uint32_t lane = (uint32_t)lane_id();
    if (lane < 4u) s_chunk[kPartChunkDw + lane] = 0u;
    if (lane < 2u) s_pm[kWave + lane] = 0u;
    PartState s{0u, 0u};                                                      // a frame starts at bit 0 with width 0 (Terse.hpp:359, :505)
    if (p != 0u) {
        PartFrame f = part_frame(terse, terse_bytes, frame_offsets, frame, P);
        s = f.ok ? part_guess(f.W, s_chunk, s_pm, p * f.L, f.limit, max_w) : PartState{0u, kPartWeak};
    }
    if (lane == 0) states[blockIdx.x] = s;
}

__global__ __launch_bounds__(kWave) void k_part_walk(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                     const uint64_t* __restrict__ frame_offsets, uint32_t max_w, uint32_t P,
                                                     const PartState* __restrict__ states, PartWalk* __restrict__ walks,
                                                     PartCk* __restrict__ cks) {
    __shared__ __attribute__((aligned(16))) uint32_t s_chunk[kPartChunkDw + 4];
    const uint32_t frame = blockIdx.x / (P - 1u), p = blockIdx.x % (P - 1u);
    const uint32_t lane = (uint32_t)lane_id();
    if (lane < 4u) s_chunk[kPartChunkDw + lane] = 0u;
    PartWalk r{};
    r.flags = 1u;
    PartFrame f = part_frame(terse, terse_bytes, frame_offsets, frame, P);
    const PartState s = states[(uint64_t)frame * P + p], t = states[(uint64_t)frame * P + p + 1u];
    // a frame a quarter of whose cuts found no run to start in is header-dense: not worth a walk (it takes the other route)
    const uint32_t kind = part_frame_kind(states + (uint64_t)frame * P, P);
    if (kind) r.flags = kind == 1u ? 2u : 4u;                               // (4: not dense, but not worth a walk either)
    else if (f.ok && t.pos > s.pos && t.pos < f.limit) {
        uint32_t pos = s.pos, w = s.w & ~(kPartWeak | kPartAmbig), cnt = 0, n_ck = 0;
        bool bad = false, dense = false;
        const uint32_t span = t.pos - s.pos;
        const uint32_t every = span / (kPartCk - 8u) > 4096u ? span / (kPartCk - 8u) : 4096u;
        // (only the frame's first part is known to start on the frame's chain: a run guess can be wrong too -- one in a few
        // thousand was, with 24 bits of evidence -- and its walk then has to get to the merge like a plain guess's)
        part_walk(f.W, s_chunk, pos, w, t.pos, f.limit, max_w, cnt, bad, dense, cks + (uint64_t)blockIdx.x * kPartCk, every, n_ck,
                  p != 0u);
        r.o_pos = pos; r.o_w = w; r.cnt = cnt; r.n_ck = n_ck; r.flags = (bad ? 1u : 0u) | (dense ? 2u : 0u);
    }
    if (lane == 0) walks[blockIdx.x] = r;
}

// One wavefront per part 1 <= p <= P - 2 (the frame's last part is not walked here: its start is simply OUT_(P-2)).
__global__ __launch_bounds__(kWave) void k_part_repair(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                       const uint64_t* __restrict__ frame_offsets, uint32_t max_w, uint32_t P,
                                                       const PartState* __restrict__ states, const PartWalk* __restrict__ walks,
                                                       const PartCk* __restrict__ cks, PartFix* __restrict__ fixes) {
    __shared__ __attribute__((aligned(16))) uint32_t s_chunk[kPartChunkDw + 4];
    const uint32_t frame = blockIdx.x / (P - 1u), p = blockIdx.x % (P - 1u);
    const uint32_t lane = (uint32_t)lane_id();
    if (p == 0u) return;                                                      // (part 0 starts in the true state)
    const uint64_t wi = (uint64_t)frame * (P - 1u) + p;
    const PartWalk prev = walks[wi - 1u], mine = walks[wi];
    const PartState s = states[(uint64_t)frame * P + p], t = states[(uint64_t)frame * P + p + 1u];
    PartFix x{0u, 0u, 0u, 0u};
    // a frame a quarter of whose links are open has a systematic problem with its cuts (see k_part_resolve: pedestals): counting
    // every part again from its neighbour's end state would be a second walk of the frame for nothing
    uint32_t n_open = 0;
    for (uint32_t q = 1u + lane; q + 1u < P; q += kWave) {
        const PartWalk wq = walks[(uint64_t)frame * (P - 1u) + q - 1u];
        const PartState sq = states[(uint64_t)frame * P + q];
        n_open += wq.flags == 0u && !(wq.o_pos == sq.pos && wq.o_w == sq.w) ? 1u : 0u;
    }
    n_open = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(n_open), 63);
#ifdef TRPX_PART_FORCE_WEAK
    n_open = 0;
#endif
    if (part_frame_kind(states + (uint64_t)frame * P, P) != 0u || 4u * n_open > P) x.state = 3u;   // (the frame takes another route)
    else if (prev.flags == 0u && !(prev.o_pos == s.pos && prev.o_w == s.w)) { // an open link behind a walk that arrived somewhere
        x.state = 3u;
        if (lane < 4u) s_chunk[kPartChunkDw + lane] = 0u;
        PartFrame f = part_frame(terse, terse_bytes, frame_offsets, frame, P);
        if (f.ok && mine.flags == 0u && prev.o_pos < t.pos && t.pos < f.limit) {
            uint32_t pos = prev.o_pos, w = prev.o_w, cnt = 0;
            x.state = part_rewalk(f.W, s_chunk, pos, w, t.pos, f.limit, max_w, cks + wi * kPartCk, mine.n_ck < kPartCk ? mine.n_ck : kPartCk,
                                  mine.cnt, cnt);
            x.cnt = cnt; x.o_pos = pos; x.o_w = w;
        }
    }
    if (lane == 0) fixes[wi] = x;
}

// See the head of the file.  list[0] = count, list[1 + i] = frame | (dense: bit 31).
__global__ __launch_bounds__(kWave) void k_part_resolve(const PartState* __restrict__ states, const PartWalk* __restrict__ walks,
                                                        const PartFix* __restrict__ fixes, FrameGeom g, uint32_t P,
                                                        const uint64_t* __restrict__ frame_offsets, uint64_t terse_bytes,
                                                        PartDesc* __restrict__ parts, uint32_t* __restrict__ list,
                                                        uint32_t* __restrict__ status) {
    const uint32_t frame = blockIdx.x, lane = (uint32_t)lane_id();
    const PartState* __restrict__ sf = states + (uint64_t)frame * P;
    const PartWalk* __restrict__ wf = walks + (uint64_t)frame * (P - 1u);
    const PartFix* __restrict__ xf = fixes + (uint64_t)frame * (P - 1u);
    PartDesc* __restrict__ pf = parts + (uint64_t)frame * P;
    bool ok = true, dense = false;
    uint32_t running = 0;
    for (uint32_t base = 0; base < P - 1u; base += kWave) {
        const uint32_t p = base + lane;
        const bool valid = p < P - 1u;
        PartWalk r{};
        PartFix x{};
        PartState s{}, t{};
        bool good = true;
        uint32_t cnt = 0;
        PartState st{0u, 0u}, en{0u, 0u};                                     // the part's true start and end states
        if (valid) {
            r = wf[p]; s = sf[p]; t = sf[p + 1u];
            if (p > 0u) x = xf[p];
            good = r.flags == 0u;
            if (p == 0u || x.state == 0u) {                                   // starts in its guess: S_0, or the link in front of it is closed
                st = PartState{s.pos, s.w & ~(kPartWeak | kPartAmbig)}; en = PartState{r.o_pos, r.o_w}; cnt = r.cnt;
            } else {
                const PartWalk q = wf[p - 1u];
                st = PartState{q.o_pos, q.o_w};
                cnt = x.cnt;
                if (x.state == 1u) en = PartState{r.o_pos, r.o_w};
                else if (x.state == 2u) { en = PartState{x.o_pos, x.o_w}; good = good && x.o_pos == r.o_pos && x.o_w == r.o_w; }   // (the next link was judged by r's end state)
                else good = false;
            }
            good = good && cnt >= 1u && cnt <= kPartMaxBlocks;
        }
        ok = ok && !__ballot(valid && !good);
        dense = dense || __ballot(valid && (r.flags & 2u) != 0u) != 0ull;
#ifdef TRPX_PART_STATS
        {   // diagnostic build: status[2..7] = fallback frames, plain guesses, bad / dense walks, repaired links, failed repairs, oversized parts
            const uint32_t n3 = (uint32_t)__builtin_popcountll(__ballot(valid && p > 0u && (s.w & kPartWeak) != 0u));
            const uint32_t n4 = (uint32_t)__builtin_popcountll(__ballot(valid && r.flags != 0u));
            const uint32_t n5 = (uint32_t)__builtin_popcountll(__ballot(valid && p > 0u && (x.state == 1u || x.state == 2u)));
            const uint32_t n6 = (uint32_t)__builtin_popcountll(__ballot(valid && p > 0u && x.state == 3u));
            const uint32_t n7 = (uint32_t)__builtin_popcountll(__ballot(valid && r.flags == 0u && (cnt < 1u || cnt > kPartMaxBlocks)));
            if (lane == 0) { atomicAdd(status + 3, n3); atomicAdd(status + 4, n4); atomicAdd(status + 5, n5); atomicAdd(status + 6, n6); atomicAdd(status + 7, n7); }
        }
#endif
        const uint32_t c = valid && good ? cnt : 0u;
        const uint32_t inc = wave_inclusive_scan(c);
        if (valid && good) {
            PartDesc d;
            d.frame = frame; d.b0 = running + inc - c; d.b1 = d.b0 + c;
            d.pos0 = st.pos; d.w0 = st.w; d.pos1 = en.pos; d.w1 = en.w; d.pad = 0u;
            pf[p] = d;
            if (p == P - 2u) {                                                // the frame's last part starts where this one ends
                PartDesc e;
                e.frame = frame; e.b0 = d.b1; e.b1 = g.n_blocks; e.pos0 = en.pos; e.w0 = en.w; e.pos1 = 0u; e.w1 = 0u; e.pad = 0u;
                pf[P - 1u] = e;
            }
        }
        running += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        if (running >= g.n_blocks) ok = false;                                // (the last part holds at least the frame's last block)
    }
    if (ok && g.n_blocks - running > kPartMaxBlocks) ok = false;
    if (!ok) {
        // No part table for this frame.  Header-dense: the position-parallel walk + tiled extraction (the list).  Otherwise --
        // run-dominated, but the cuts did not work out: e.g. pixels with a pedestal, whose constant payload bits look like
        // header bits at the same stride, so that every cut starts beside the chain and stays there -- the frame is ONE unit for
        // its one workgroup's serial walker, as before there were parts (0.4 ms for 200 frames of 1030 x 1065 against 2.9 ms on
        // the list's route), provided its bits fit the decoder's 26-bit positions.
        const uint64_t fo = frame_offsets[frame], fe = frame_offsets[frame + 1];
        const bool one_unit = !dense && fe > fo && fe <= terse_bytes && 8 * (fe - fo) + (1u << 17) < (1ull << 26);
        __builtin_amdgcn_s_waitcnt(0);
        for (uint32_t p = lane; p < P; p += kWave) {
            PartDesc d{};
            d.frame = frame;
            if (one_unit && p == 0u) d.b1 = g.n_blocks;
            pf[p] = d;
        }
        if (!one_unit && lane == 0) {
            list[1u + atomicAdd(&list[0], 1u)] = frame | (dense ? 0x80000000u : 0u);
            if (dense) atomicAdd(reinterpret_cast<unsigned long long*>(list) - 2, 1ull);   // (k_seg_wg's: their number, codec_common.hpp)
        }
#ifdef TRPX_PART_STATS
        if (lane == 0) atomicAdd(status + 2, 1u);
#endif
    }
}

hipError_t launch_build_parts(const DecodeArgs& a, uint32_t max_w, hipStream_t st) {
    const uint32_t P = a.plan.parts_per_frame;
    if (P < 2u || !a.parts || !a.part_ws || !a.defer) return hipErrorInvalidValue;
    const PartWs l = part_ws_layout(a.n_frames, P);
    char* ws = static_cast<char*>(a.part_ws);
    PartState* states = reinterpret_cast<PartState*>(ws + l.states);
    PartWalk* walks = reinterpret_cast<PartWalk*>(ws + l.walks);
    PartFix* fixes = reinterpret_cast<PartFix*>(ws + l.fixes);
    PartCk* cks = reinterpret_cast<PartCk*>(ws + l.cks);
    const dim3 links(a.n_frames * (P - 1u));
    hipLaunchKernelGGL(k_part_guess, dim3(a.n_frames * P), dim3(kWave), 0, st, a.terse, (uint64_t)a.terse_bytes, a.frame_offsets, max_w, P,
                       states);
    hipLaunchKernelGGL(k_part_walk, links, dim3(kWave), 0, st, a.terse, (uint64_t)a.terse_bytes, a.frame_offsets, max_w, P,
                       static_cast<const PartState*>(states), walks, cks);
    hipLaunchKernelGGL(k_part_repair, links, dim3(kWave), 0, st, a.terse, (uint64_t)a.terse_bytes, a.frame_offsets, max_w, P,
                       static_cast<const PartState*>(states), static_cast<const PartWalk*>(walks), static_cast<const PartCk*>(cks), fixes);
    hipLaunchKernelGGL(k_part_resolve, dim3(a.n_frames), dim3(kWave), 0, st, static_cast<const PartState*>(states),
                       static_cast<const PartWalk*>(walks), static_cast<const PartFix*>(fixes), a.geom, P, a.frame_offsets, (uint64_t)a.terse_bytes,
                       a.parts, a.defer, a.status);
    return hipGetLastError();
}

}  // namespace trpx
