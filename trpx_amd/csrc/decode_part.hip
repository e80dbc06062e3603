// PROLIX decode of LARGE frames (gfx950 / CDNA4): the INDEX route, the one frames of more than single_part_blocks() blocks take by
// default.
//
// The per-frame decoder (decode_frame.hip) puts one serial header walker on a frame (reference include/Terse.hpp:360-372: block
// b + 1's position is only known after block b's header); a 2048 x 2048 frame is a 16 x longer chain than a 512 x 512 one, on 16 x
// fewer workgroups.  So a large frame is cut at bit positions X_p = p * L into as many PARTS as the GPU holds walkers at once
// (chain_parts_per_frame; the last cut lies kChainTail bits in front of the frame's end), and the route finds the chain state in
// front of every part -- and, while it is there, the frame's decode index (widths[] by block, the bit offset of every 256th block:
// launchers.hpp), from which the frames are extracted as if the caller had brought it (k_unpack_tiles / k_decode_units_indexed;
// run-dominated 8 / 16-bit frames part by part, k_decode_parts on the part table).  A serial walker is a latency chain, ~130 ns
// per run of equal widths whatever else runs on the SIMD: the walk's time is its longest part's.  Launches:
//
//   k_chain_zero     the words the route needs cleared (status, hand-over list, start states, records).
//   k_chain_walk     ONE launch, one wavefront per part, three things in a row:
//                    1. the part's START STATE -- a position inside a run of equal widths behind the cut (chain_guess; part_try,
//                       part_header_phase), else a plain guess ON the cut -- published for the wavefront of the part in front;
//                    2. the WALK to the start state of the part behind (part_walk<true>: fast steps, no position entries), which
//                       counts the blocks and leaves one byte per block (the width in front of it, part-relative) and up to
//                       kChainCk checkpoints.  A chain from a plain guess merges with the frame's at the first explicit header it
//                       meets on a block start; a width the pixel type does not have proves it false: early in the part the walk
//                       starts again behind it, later it stops.  The walk record is published;
//                    3. the LINK into the part behind (chain_link_into): closed if that part was started where this chain arrives;
//                       open: that part is counted again from here, checkpoint by checkpoint of its own walk, until the chains have
//                       merged (chain_rewalk; chain_walk_ahead where the neighbour started from a plain guess), the entries
//                       spliced in front of the walk's.  Stopped parts are counted whole, the same wavefront going on behind them.
//                    Part 0 of up to sixteen frames first votes on whether the stack is header-dense (ChainVote, part_walk.hpp):
//                    such a stack's walkers stop, its frames are listed with bit 31 for k_seg_wg (decode_seg.hip).
//   k_chain_resolve  one wavefront per frame: S_0 = (0, 0) is true (Terse.hpp:359, :505), links closed or repaired => by induction
//                    every part's start, count and end are the frame's chain's; prefix sums; the part table; the extraction mode.
//   k_chain_index    one wavefront per part: entries -> widths[b0 ..), group offsets by a prefix sum over header + payload lengths,
//                    the end checked against the next part's start.  Parts without entries and the frame's tail are walked from
//                    their true start, by count (chain_walk_abs).
//
// A frame where this does not work out is listed for the position-parallel walk (decode_seg.hip), which writes the same index.
// Guesses, restarts, stops and links only ever steer the speed: every part's end is checked against its successor's start, the
// last one against S_f = 1 + bits/8 (Terse.hpp:547).  The window, the walker and the words the wavefronts exchange are
// part_walk.hpp's, shared with round 4's parts route (decode_part_sel4.hip, selector 4 only); the rule for which frames are
// large at all (single_part_blocks) lives here.
// HBM traffic: the stream once more (walk only: no pixels), 0.2 of the algorithmic bytes of a u16 stack.
#include "part_walk.hpp"

namespace trpx {

// Which frames stay whole on the per-frame route (one workgroup per frame; header-dense ones handed to the one-wavefront
// position-parallel walk): up to kPartMaxBlocks blocks always; in a stack of kManyFrames frames and more up to kManyBlocks -- the
// workgroups of such a stack fill the GPU by themselves, and cutting its frames costs more than it levels (1280 x 640^2 Poisson(3)
// frames through the index route: 1.42 ms; 2000 x 512^2, the same bytes: 0.74).
static uint32_t g_many_frames = kManyFrames, g_many_blocks = kManyBlocks;
void set_single_part_rule(uint32_t many_frames, uint32_t many_blocks) { g_many_frames = many_frames; g_many_blocks = many_blocks; }
uint32_t single_part_blocks(size_t n_frames) {
    return n_frames >= g_many_frames && g_many_blocks > kPartMaxBlocks ? g_many_blocks : kPartMaxBlocks;
}

constexpr uint32_t kChainWaves = 4352;         // parts per stack (chain_parts_per_frame) ...
constexpr uint32_t kChainWavesNarrow = 4096;   // ... of 8 / 16-bit pixels
constexpr uint32_t kChainCk = 64;              // checkpoints per part
constexpr uint32_t kChainTail = 2048;          // bits of the frame's last part (walked by count in k_chain_index)
constexpr uint32_t kChainPatience = 8192;      // bits into a part after which a walk that reads an illegal width stops instead of starting again
constexpr uint32_t kChainEntSlack = 80;

// Parts per frame: as many walkers as the GPU holds at once (8 KB of LDS each: 19 per CU) -- a second round of a few hundred
// stragglers doubled k_chain_walk's time (eight 4096 x 4096 frames, 5464 parts: 146 us; tools/chain_stamps.py) --, of 1 K ..
// 16 K blocks each; + the tail part.
uint32_t chain_parts_per_frame(const FrameGeom& g, size_t n_frames, size_t pixel_bytes) {
    if (g.n_blocks <= single_part_blocks(n_frames) || n_frames == 0) return 1u;
    // (8 / 16-bit pixels: 4096 -- the parts are also the units k_decode_parts extracts, eight workgroups per CU: two whole rounds
    // of them instead of two and a tenth; 200 x (1030 x 1065) 0.202 -> 0.193 ms, 128 x 2048^2 0.43 -> 0.405, Poisson(3) mid-size
    // 0.559 -> 0.537; the int32 frames, extracted by tiles, lose 6 % to the longer parts: 0.3105 -> 0.331)
    const uint64_t waves = pixel_bytes < 4 ? kChainWavesNarrow : kChainWaves;
    const uint64_t lo = ((uint64_t)g.n_blocks + kPartBlocks - 1u) / kPartBlocks, hi = (uint64_t)g.n_blocks / 1024u;
    uint64_t n = waves / n_frames;
    n = n < lo ? lo : (n > hi ? hi : n);
    return (uint32_t)(n < 3u ? 4u : n + 1u);
}
__host__ __device__ inline uint32_t chain_ent_cap(uint32_t n_blocks, uint32_t P) { return 2u * ((n_blocks + P - 1u) / P) + kChainEntSlack; }
struct ChainFix {                              // what chain_link_into leaves per (frame, part 1 <= p < P - 1)
    uint32_t state;                            // 0: link closed, nothing done; 1: merged into the part's walk; 2: walked to T_p on its own; 3: failed
    uint32_t cnt, o_pos, o_w;                  // the part's block count (and, state 2, its end state) from the true start
    uint32_t b_merge, ck_cnt;                  // state 1: the repair's block b_merge is the part's own walk's block ck_cnt (a checkpoint)
    uint32_t n_fix;                            // entries the repair left for its blocks [0, b_merge] (0: they did not fit)
    uint32_t pad;
};
struct ChainWs { size_t states, walks, fixes, cks, ents, fixents, modes, total; };
static ChainWs chain_ws_layout(const FrameGeom& g, size_t n_frames, size_t P) {
    ChainWs w;
    w.states = 0;                                                             // [states, cks): start states, walk records (with their ready / published bits) and link records, cleared in front of every call (launch_chain_zero)
    w.walks = align_up(w.states + n_frames * P * sizeof(PartState), 256);
    w.fixes = align_up(w.walks + n_frames * P * sizeof(PartWalk), 256);
    w.cks = align_up(w.fixes + n_frames * P * sizeof(ChainFix), 256);
    w.ents = align_up(w.cks + n_frames * P * kChainCk * sizeof(PartCk), 256);
    w.fixents = align_up(w.ents + n_frames * P * (size_t)chain_ent_cap(g.n_blocks, (uint32_t)P) + 16, 256);
    w.modes = align_up(w.fixents + n_frames * P * (size_t)chain_ent_cap(g.n_blocks, (uint32_t)P) + 16, 256);   // (a repair's entries: as many as a walk's)
    w.total = align_up(w.modes + 4 * n_frames, 256);
    return w;
}
size_t chain_workspace_bytes(const FrameGeom& g, size_t n_frames, size_t pixel_bytes) {
    const size_t P = chain_parts_per_frame(g, n_frames, pixel_bytes);
    return P > 1 ? chain_ws_layout(g, n_frames, P).total : 0;
}

// The frame's cuts: X_p = p * L for p < P, the last one kChainTail bits (or a sixteenth of a small frame) in front of the end.
__device__ __forceinline__ PartFrame chain_frame(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                 const uint64_t* __restrict__ frame_offsets, uint32_t frame, uint32_t P) {
    PartFrame f = part_frame(terse, terse_bytes, frame_offsets, frame, P);
    if (!f.ok) return f;
    const uint32_t tail = f.limit > 16u * kChainTail ? kChainTail : f.limit / 16u;
    f.L = (f.limit - tail + (P - 2u)) / (P - 1u);
    f.ok = f.L >= 128u && tail > P;                                         // (a frame of a few bits per part: another route; an all-zero 4096 x 4096 frame has 1 Kbit parts)
    return f;
}

// The index route's search (k_chain_walk's first step), staged by what the data show: (1) widths up to 8, the first 4096 positions -- two
// thirds of the cuts of a stack with a width change every nine blocks end here, and header-dense data, where no run exists, pays
// for no more than this; (2) the width whose candidates survived longest, if they survived 20 header bits (chance: 2^-20 per
// candidate, 32 K candidates), over the rest of the range: runs of that width exist nearby; (3) wider widths, one pass each,
// only if no small width has runs here (fewer than 20 positions of a pass with 12 header bits 1: pedestals, wide data --
// header-dense narrow data shows 20 and more and mostly skips this stage).  A cut that ends without a run starts from a plain guess.
__device__ __forceinline__ PartState chain_guess(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t* __restrict__ s_pm, uint32_t X, uint32_t limit,
                                                 uint32_t max_w, uint32_t reach, ChainVote* vote = nullptr) {   // (vote: a header-dense stack needs no guesses)
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t s_max = 1u + (uint32_t)kBlock * max_w;
    const PartState plain{X, kPartWeak};
#ifdef TRPX_PART_FORCE_WEAK
    return plain;
#endif
    uint32_t passes = kPartSearch;
    while (passes && (uint64_t)X + 2048ull * passes + (uint64_t)kPartEvid * s_max + 128u > (uint64_t)limit) --passes;   // too close to the frame's end
    while (passes && 2048ull * passes + (uint64_t)kPartSkip * s_max > (uint64_t)reach) --passes;
    if (X + 256u > limit) return plain;
    part_fill(W, s_chunk, X);
    {
        const uint32_t a = lane < 4u ? part_bits(W, s_chunk, X + 32u * lane) : 0xFFFFFFFFu;
        if (!__ballot(a != 0xFFFFFFFFu)) return PartState{X, 0u};            // inside a run of empty blocks (parts of any size: an all-zero frame's are short)
    }
    if (passes == 0u) return plain;
    const uint32_t w1 = max_w < 8u ? max_w : 8u, p1 = passes < 2u ? passes : 2u;
    uint32_t best_w = 0, best_d = 0, most12 = 0;
    for (uint32_t w = 1; w <= w1; ++w)
        for (uint32_t pass = 0; pass < p1; ++pass) {
            uint32_t d, n12;
            if (vote && chain_vote_look(*vote)) return plain;
            const uint32_t q = part_try(W, s_chunk, s_pm, X + 2048u * pass, w, d, n12);
            if (q != ~0u) return PartState{q, w};
            if (d > best_d) { best_d = d; best_w = w; }
            most12 = n12 > most12 ? n12 : most12;
        }
    if (best_d >= 20u)
        for (uint32_t pass = p1; pass < passes; ++pass) {
            uint32_t d, n12;
            const uint32_t q = part_try(W, s_chunk, s_pm, X + 2048u * pass, best_w, d, n12);
            if (q != ~0u) return PartState{q, best_w};
        }
    if (most12 < 20u)                                                         // (no small width has runs here: wide data, a pedestal -- whose payload shows up to 16 by itself)
        for (uint32_t w = w1 + 1u; w <= max_w; ++w) {
            uint32_t d, n12;
            const uint32_t q = part_try(W, s_chunk, s_pm, X, w, d, n12);
            if (q != ~0u) return PartState{q, w};
            most12 = n12 > most12 ? n12 : most12;
        }
    // How run-dominated?  What tells is how MANY of a pass's ~55 block starts carry 12 header bits 1 at one stride: ~45 where one
    // block in sixty changes its width (synth-v1), ~28 at one in nine (eight 4096^2 int32 frames), ~22 in Poisson(3) counts, a
    // handful in noise -- the deepest single candidate does not tell: runs of 28 blocks occur a few times per thousand cuts in
    // Poisson(3) counts too.  Only the first kind gets the flag (a walk that stops instead of starting again, k_chain_walk):
    // there a false chain may not merge for a whole part; in the others it merges within a few K bits, and a stopped part
    // costs its repair a whole part's walk (71 of 4200 parts stopped: the repair launch 236 instead of ~20 us).
    // (32-bit pixels: from 24 on -- their parts hold half the blocks per bit, a stopped part's repair is a short walk (65 us for
    // eight 4096^2 frames' parts, where two walks that kept starting again for 100 Kbits made k_chain_walk 187 instead of ~100 us))
    return most12 >= (max_w > 16u ? 24u : 40u) ? PartState{X, kPartWeak | kPartRuns} : plain;
}

// The blocks of a part counted again from the true state (pos, w), checkpoint by checkpoint of the part's own walk: fast steps to
// the next checkpoint's position (part_walk: it stops at the first block start at or behind it), and if the chain arrives IN the
// checkpoint's state the two have merged -- the rest of that walk is this chain's.  Leaves the entries of the blocks it counted in
// fix[] (part_walk<true>) as long as they fit.  Returns the ChainFix state.
__device__ __forceinline__ uint32_t chain_rewalk(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t& pos, uint32_t& w, uint32_t T,
                                                 uint32_t limit, uint32_t max_w, const PartCk* __restrict__ ck, uint32_t n_ck,
                                                 uint32_t walk_cnt, uint8_t* __restrict__ fix, uint32_t fix_cap, ChainFix& x,
                                                 uint32_t b = 0, bool fits = true) {   // (b, fits: blocks already counted by chain_walk_ahead)
    uint32_t k = 0;
    bool bad = false, dense = false;
    for (;;) {
        PartCk c{};
        while (k < n_ck && (c = part_ck_load(ck + k)).pos <= pos) {
            if (c.pos == pos && c.w == w) {                                   // (starts in a checkpoint: nothing to count)
                x.b_merge = b; x.ck_cnt = c.cnt; x.cnt = b + (walk_cnt - c.cnt); x.n_fix = fits ? b + 1u : 0u;
                return 1u;
            }
            ++k;
        }
        const uint32_t target = k < n_ck ? c.pos : T;                         // (c: checkpoint k, the first one behind pos)
        uint32_t cnt = 0, n0 = 0;
        if (fits && b + 160u < fix_cap)
            part_walk<true>(W, s_chunk, pos, w, target, limit, max_w, cnt, bad, dense, nullptr, 0u, n0, false, 0u, false, fix + b, fix_cap - b);
        else
            part_walk<false>(W, s_chunk, pos, w, target, limit, max_w, cnt, bad, dense, nullptr, 0u, n0, false, 0u, false);
        if (bad) return 3u;
        b += cnt;
        fits = fits && b + 1u < fix_cap;
        if (k >= n_ck) break;                                                 // at T on its own
    }
    x.cnt = b; x.o_pos = pos; x.o_w = w; x.b_merge = b; x.ck_cnt = 0u; x.n_fix = fits ? b + 1u : 0u;
    return 2u;
}

// A walk record / a start state of ANOTHER wavefront of this launch, once it has been published (bounded wait: a record that does
// not come reads as a bad walk, a state as position 0 -- the link fails and the frame takes the other route).
#if defined(TRPX_CHAIN_FORCE_TIMEOUT)
constexpr uint64_t kChainWaitTicks = 200000ull;        // (test build, see k_chain_walk: 2 ms)
#elif defined(TRPX_PART_STATS)
constexpr uint64_t kChainWaitTicks = 3000000000ull;    // (diagnostic build: its printfs hold wavefronts up for milliseconds)
#else
constexpr uint64_t kChainWaitTicks = 25000000ull;      // how long a wavefront waits for another's word: 0.25 s of the 100 MHz counter
#endif
__device__ __forceinline__ PartWalk chain_walk_wait(const PartWalk* src) {
    const uint64_t* d = reinterpret_cast<const uint64_t*>(src);
    uint64_t v[4] = {0, 0, 0, 0};
    if (lane_id() == 0) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            v[1] = __hip_atomic_load(d + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // cnt | flags << 32
            if (((v[1] >> 32) & kWalkPublished) != 0u) break;
            __builtin_amdgcn_s_sleep(64);
            if (__builtin_amdgcn_s_memrealtime() - t0 > kChainWaitTicks) { v[1] = 1ull << 32; break; }   // 0.25 s: a bad walk
        }
        // (the record's other words -- and whatever the caller reads of the part's checkpoints -- only after the published bit has
        // been SEEN: the flag's value has arrived here, the statement keeps the compiler from moving the relaxed loads below
        // in front of it; the hardware returns loads in order)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        v[0] = __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[2] = __hip_atomic_load(d + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[3] = __hip_atomic_load(d + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    uint32_t u[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u[2 * i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v[i]);
        u[2 * i + 1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v[i] >> 32));
    }
    PartWalk r;
    __builtin_memcpy(&r, u, 32);
    return r;
}
__device__ __forceinline__ void chain_walk_publish(PartWalk* dst, PartWalk r) {
    static_assert(sizeof(PartWalk) == 32, "four 64-bit words");
    r.flags |= kWalkPublished;
    uint64_t v[4];
    __builtin_memcpy(v, &r, 32);
    uint64_t* d = reinterpret_cast<uint64_t*>(dst);
    if (lane_id() == 0) {
        __hip_atomic_store(d, v[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d + 2, v[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(d + 3, v[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                          // the record's other words and the checkpoints (write-through) have arrived
    if (lane_id() == 0) __hip_atomic_store(d + 1, v[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... without waiting: false if the record is not there yet
__device__ __forceinline__ bool chain_walk_poll(const PartWalk* src, PartWalk& r) {
    const uint64_t* d = reinterpret_cast<const uint64_t*>(src);
    uint64_t v[4] = {0, 0, 0, 0};
    if (lane_id() == 0) {
        v[1] = __hip_atomic_load(d + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (((v[1] >> 32) & kWalkPublished) != 0u) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // (as in chain_walk_wait)
            v[0] = __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v[2] = __hip_atomic_load(d + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v[3] = __hip_atomic_load(d + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    uint32_t u[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u[2 * i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v[i]);
        u[2 * i + 1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v[i] >> 32));
    }
    __builtin_memcpy(&r, u, 32);
    return (r.flags & kWalkPublished) != 0u;
}
// The part behind, counted from the true state while its own wavefront is still walking it: kChainAhead bits at a time, its record
// polled in between.  True: the record has come (`mine`); the chain stands at (pos, w), b blocks in, and chain_rewalk goes on from
// there with the record's checkpoints.  False: the chain is at T (or `bad`) and the record still is not there.
constexpr uint32_t kChainAhead = 8192;
__device__ __forceinline__ bool chain_walk_ahead(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t& pos, uint32_t& w, uint32_t T, uint32_t limit,
                                                 uint32_t max_w, uint8_t* __restrict__ fix, uint32_t fix_cap, uint32_t& b, bool& fits, bool& bad,
                                                 const PartWalk* rec, PartWalk& mine) {
    bool dense = false;
    for (;;) {
        if (chain_walk_poll(rec, mine)) return true;
        if (pos >= T || bad) return false;
        const uint32_t target = T - pos > kChainAhead ? pos + kChainAhead : T;
        uint32_t cnt = 0, n0 = 0;
        if (fits && b + 160u < fix_cap)
            part_walk<true>(W, s_chunk, pos, w, target, limit, max_w, cnt, bad, dense, nullptr, 0u, n0, false, 0u, false, fix + b, fix_cap - b);
        else
            part_walk<false>(W, s_chunk, pos, w, target, limit, max_w, cnt, bad, dense, nullptr, 0u, n0, false, 0u, false);
        b += cnt;
        fits = fits && b + 1u < fix_cap;
        pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);
        w = (uint32_t)__builtin_amdgcn_readfirstlane((int)w);
    }
}
__device__ __forceinline__ PartState chain_state_wait(const PartState* src) {
    const uint64_t* d = reinterpret_cast<const uint64_t*>(src);
    uint64_t v = 0;
    if (lane_id() == 0) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            v = __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (((v >> 32) & kPartReady) != 0u) break;
            __builtin_amdgcn_s_sleep(32);
            if (__builtin_amdgcn_s_memrealtime() - t0 > kChainWaitTicks) { v = 0; break; }           // 0.25 s of the 100 MHz counter
        }
    }
    return PartState{(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32))};
}

// The link INTO part p (1 <= p <= P - 2), by the wavefront that has just walked part p - 1 (`prev`: its record) and arrived in front
// of it.  Closed -- the part's walk started where this chain arrives -- nothing is counted.  Open: the part's blocks are counted again
// from here, checkpoint by checkpoint of the part's own walk, until the chains have merged (chain_rewalk).  A part whose walk stopped
// on a false chain (flag 16) is counted as a whole (state 2: nothing to merge into), and the same wavefront goes on into the parts
// behind it for as long as they are stopped parts: their own wavefronts, which cannot know the true end of a stopped part, leave the
// link behind them alone.  Every part's ChainFix is written by exactly one wavefront.
// (Until round 5 a launch of its own behind the walk: its critical path -- the longest-lived false chain of 4000, a part's restart
// far into it, a stopped part -- was 47 us for eight 4096^2 frames and 130 us for 200 x (1030 x 1065) Poisson(3) frames, with the
// GPU all but idle; here it falls into the slack every wavefront but the launch's slowest has.)
__device__ __forceinline__ void chain_link_into(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                const uint64_t* __restrict__ frame_offsets, uint32_t max_w, uint32_t P,
                                                const PartState* states, const PartWalk* walks, const PartCk* cks, ChainFix* __restrict__ fixes,
                                                uint8_t* __restrict__ fixents, uint32_t fix_cap, uint32_t frame, uint32_t p, const PartWalk& prev,
                                                PartFrame& f, uint32_t* __restrict__ s_chunk) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t slot0 = (uint64_t)frame * P;
    uint32_t pos = prev.o_pos, w = prev.o_w;                                  // the true end of the part in front (if ITS start was true: k_chain_resolve)
    // arrives in the state the part's walk was started in: closed (a walk that began again behind an illegal width, or stopped, did
    // so on a chain this one would then be too)
    const PartState g = chain_state_wait(states + slot0 + p);
    if ((prev.flags & 1u) != 0u || (g.pos == pos && (g.w & ~kPartFlags) == w)) {
        if (lane == 0) fixes[slot0 + p] = ChainFix{};
        return;
    }
    // A part that started from a plain guess (no run behind its cut: header-dense data, wide data) is not on the frame's chain until
    // it has merged with it, so this link is open: the count from here starts at once, ahead of the part's record (chain_walk_ahead)
    // -- waiting for it first left the launch's last wavefronts idle for 60 us and more, behind the slowest walks of all.
    const bool ahead = (g.w & kPartWeak) != 0u;
#ifdef TRPX_PART_STATS
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
#endif
    for (uint32_t cur = p;;) {
        ChainFix x{};
        pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);             // (wave-uniform by construction)
        w = (uint32_t)__builtin_amdgcn_readfirstlane((int)w);
        cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
        const PartState t = chain_state_wait(states + slot0 + cur + 1u);
        const bool can_walk = f.ok && pos < t.pos && t.pos < f.limit;
        const uint32_t pos_in = pos, w_in = w;
        uint8_t* const fix = fixents + (slot0 + cur) * (uint64_t)fix_cap;
        uint32_t b = 0;
        bool fits = true, bad = false, have = false;
        PartWalk mine{};
        if (ahead && cur == p && can_walk) have = chain_walk_ahead(f.W, s_chunk, pos, w, t.pos, f.limit, max_w, fix, fix_cap, b, fits, bad, walks + slot0 + cur, mine);
        if (!have) mine = chain_walk_wait(walks + slot0 + cur);
        const bool open = !(pos_in == mine.s_pos && w_in == mine.s_w) || (mine.flags & 16u) != 0u;
        if (open) {
            x.state = 3u;
            if (can_walk && !bad && (mine.flags & 1u) == 0u) {
                const uint32_t n_ck = (mine.flags & 16u) != 0u ? 0u : (mine.n_ck < kChainCk ? mine.n_ck : kChainCk);   // (a stopped walk: nothing to merge into)
                x.state = chain_rewalk(f.W, s_chunk, pos, w, t.pos, f.limit, max_w, cks + (slot0 + cur) * kChainCk, n_ck, mine.cnt, fix, fix_cap, x, b, fits);
                if (x.state == 1u && (mine.flags & 8u) != 0u) x.n_fix = 0u;  // (the part's own entries did not fit: nothing to splice onto)
#ifdef TRPX_PART_STATS
                if (x.state == 3u && lane == 0)
                    printf("repair failed in its walk: frame %u part %u of %u at %u/%u target %u limit %u, own walk %u/%u -> %u/%u cnt %u n_ck %u flags %u\n",
                           frame, cur, P, pos, w, t.pos, f.limit, mine.s_pos, mine.s_w, mine.o_pos, mine.o_w, mine.cnt, mine.n_ck, mine.flags);
#endif
            }
        } else { pos = pos_in; w = w_in; }                                    // (closed after all: what was counted ahead is dropped)
        if (lane == 0) fixes[slot0 + cur] = x;
#ifdef TRPX_PART_STATS
        {
            const uint64_t t_now = __builtin_amdgcn_s_memrealtime();
            if (lane == 0 && t_now - t_start > 30000u)
                printf("slow repair: frame %u part %u (from %u) %u us: state %u cnt %u merge at %u (own block %u), own walk cnt %u n_ck %u flags %u start %u/%u, true start %u\n", frame, cur, p,
                       (uint32_t)(t_now - t_start) / 100u, x.state, x.cnt, x.b_merge, x.ck_cnt, mine.cnt, mine.n_ck, mine.flags, mine.s_pos, mine.s_w, prev.o_pos);
        }
#endif
        // on into the next part?  only behind a stopped part that this wavefront has counted to its end
        if (x.state != 2u || (mine.flags & 16u) == 0u || cur + 1u > P - 2u) break;
        ++cur;                                                                // (pos, w: the true end of the part just counted)
    }
}

// One wavefront per part: its start state first -- a position inside a run of equal widths behind the cut, or a plain guess
// (chain_guess) --, published for the wavefront of the part in front, whose walk ends there; then the walk to the start state of the
// part behind, which that part's wavefront publishes.  (One launch instead of a guessing and a walking one: the waits are for a
// wavefront that needs nothing from anybody -- a neighbour's guess is 15 .. 30 us of work from its dispatch --, bounded, and a
// wavefront that gives up reports a bad walk: the frame takes the other route.)
__global__ __launch_bounds__(kWave) void k_chain_walk(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                      const uint64_t* __restrict__ frame_offsets, uint32_t max_w, uint32_t P,
                                                      uint32_t ent_cap, PartState* states, PartWalk* walks, PartCk* cks,
                                                      uint8_t* __restrict__ ents, ChainFix* __restrict__ fixes, uint8_t* __restrict__ fixents,
                                                      uint64_t* __restrict__ vote_words, [[maybe_unused]] uint32_t* __restrict__ stamps) {
    __shared__ __attribute__((aligned(16))) uint32_t s_chunk[kPartChunkDw + 4];
    __shared__ uint32_t s_pm[kWave + 2];
    const uint32_t item = blockIdx.x;
    const uint32_t frame = item / P, p = item % P;
    const uint32_t lane = (uint32_t)lane_id();
    // (the stack's vote, see ChainVote: part 0 of up to sixteen frames votes, every part looks at the verdict at its checkpoints)
    const uint32_t n_frames = gridDim.x / P, n_voters = chain_voters(n_frames);
    const uint32_t my_voter = (uint32_t)(((uint64_t)frame * n_voters + n_frames - 1u) / n_frames);   // the voter whose frame this would be
    const bool voter = p == 0u && my_voter < n_voters && (uint32_t)((uint64_t)my_voter * n_frames / n_voters) == frame;
    ChainVote vote{vote_words, false};
    if (chain_verdict(vote_words) == 2u) {                                    // (the test build alldense; a wavefront that starts late)
        if (p + 1u < P) { PartWalk r0{}; r0.flags = 1u; chain_walk_publish(walks + (uint64_t)frame * P + p, r0); }
        if (lane == 0) __hip_atomic_store(reinterpret_cast<uint64_t*>(states) + (uint64_t)frame * P + p, (uint64_t)(p * 128u) | ((uint64_t)(kPartWeak | kPartReady) << 32),
                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (somebody may wait for this part's start state)
        return;
    }
#ifdef TRPX_CHAIN_STAMPS
    const uint64_t st_a = __builtin_amdgcn_s_memrealtime();
    uint64_t st_b = st_a, st_c = st_a;
#endif
    if (lane < 4u) s_chunk[kPartChunkDw + lane] = 0u;
    if (lane < 2u) s_pm[kWave + lane] = 0u;
    const uint64_t slot = (uint64_t)frame * P + p;
    PartWalk r{};
    r.flags = 1u;
    PartFrame f = chain_frame(terse, terse_bytes, frame_offsets, frame, P);
    if (voter && chain_verdict(vote_words) == 0u) {                           // this wavefront's vote first: its share of ~1000 blocks from the frame's true start, 4 Kbit at a time
        const uint32_t want = 1024u / n_voters < 64u ? 64u : 1024u / n_voters;
        uint32_t vp = 0u, vw = 0u, vb = 0u, ve = 0u;
        bool vbad = !f.ok;                                                    // (every voter votes, if with nothing: the verdict waits for the last one)
        __builtin_amdgcn_s_setprio(3);                                        // (everybody else is looking for a start state that a header-dense stack will not need)
        for (uint32_t T = 4096u; !vbad && vb < want && T <= 32768u && T < f.limit / 2u; T += 4096u) {   // (the walker's fast steps need their 64 candidates in front of T)
            uint32_t c1 = 0u, e1 = 0u, n1 = 0u;
            bool dn = false;
            part_walk<false>(f.W, s_chunk, vp, vw, T, f.limit, max_w, c1, vbad, dn, nullptr, 0u, n1, false, kPartCk, false, nullptr, 1u, false, 0u, &e1);
            vb += c1; ve += e1;
        }
        chain_vote_cast(vote_words, n_voters, vbad ? 0u : vb, vbad ? 0u : ve);
        __builtin_amdgcn_s_setprio(0);
    }
    PartState s{0u, 0u};                                                      // a frame starts at bit 0 with width 0 (Terse.hpp:359, :505)
    if (p != 0u) {
        if (!f.ok) s = PartState{0u, kPartWeak};
        else {
            const uint32_t X = p * f.L;
            // the search stays inside the part's first half: a start state lies in front of the next cut
            const uint32_t reach = p + 1u < P ? f.L / 2u : (f.limit - X) / 2u;
            s = chain_guess(f.W, s_chunk, s_pm, X, f.limit, max_w, reach, &vote);
        }
    }
    s.pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.pos);
    s.w = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.w);
    uint64_t* const sw = reinterpret_cast<uint64_t*>(states);
#ifdef TRPX_CHAIN_FORCE_TIMEOUT
    // test build (make chain_timeout, tests/test_gpu_large_frames.py): frame 0's part 3 never publishes its start state, frame 1's part 5
    // never its record -- the wavefronts that wait for them give up after kChainWaitTicks, the frames take the other route
    const bool mute_start = frame == 0u && p == 3u, mute_record = frame == 1u && p == 5u;
#else
    constexpr bool mute_start = false, mute_record = false;
#endif
    if (lane == 0 && !mute_start)
        __hip_atomic_store(sw + slot, (uint64_t)s.pos | ((uint64_t)(s.w | kPartReady) << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the word is all there is to publish: no fence)
    if (p + 1u == P) return;                                                  // (the frame's last part is walked by count: k_chain_index)
#ifdef TRPX_CHAIN_STAMPS
    st_b = __builtin_amdgcn_s_memrealtime();
#endif
    const PartState t = chain_state_wait(states + slot + 1u);                 // (never came: t.pos = 0 -> a bad walk)
    if (chain_verdict(vote_words) == 2u) {                                    // (the verdict came while this part looked for its start)
        PartWalk r0{}; r0.flags = 1u;
        if (!mute_record) chain_walk_publish(walks + slot, r0);
        return;
    }
    if (f.ok && t.pos > s.pos && t.pos < f.limit) {
        uint32_t pos = s.pos, w = s.w & ~kPartFlags, cnt = 0, n_ck = 0;
        bool bad = false, dense = false, stopped = false;
        uint32_t n_exp = 0;
        const uint32_t X = pos;
        // (how long a walk that reads illegal widths keeps starting again: for ever where the cut found no runs at all -- header-dense
        // data: false chains merge within a few K bits, and a stopped part costs its repair a whole part's walk, the repair launch's
        // critical path: 233 against 15 us for 200 x (1030 x 1065) Poisson(3) counts --, kChainPatience bits where runs lie nearby or
        // the start was a run guess, which is then a wrong one: run-dominated data)
        // (... and even there not for ever: a chain that still reads illegal widths a quarter of the part in is one of the few --
        // two of eight 4096^2 frames' 4352 -- that will not merge in time: 184 against 70 us)
        const uint32_t patience = (s.w & kPartWeak) != 0u && (s.w & kPartRuns) == 0u ? (t.pos - X) / 4u : kChainPatience;
#ifdef TRPX_CHAIN_STAMPS
        st_c = __builtin_amdgcn_s_memrealtime();
#endif
        // A cut without a run to start in (header-dense data; the weakparts test build: every cut) starts ON the cut from a plain
        // guess: the chain is not the frame's until it has merged with it -- at the first explicit header it meets on a block start,
        // a median of 94 blocks in Poisson(3) counts (tools/merge_stats.py) -- and the link in front of the part is open: the
        // repair counts from the true state to the first checkpoint behind the merge, a few hundred blocks, in parallel for all
        // parts.  (A warm-up stretch in FRONT of the cut, so that the chain arrives merged -- round 5's first version, 16 K bits --
        // closed 95 % of such links and cost every wavefront 28 .. 52 us of walking on a false chain, which takes a step every
        // other block: more than the repairs of all links together.)
        // A width the pixel type does not have says the chain is not the frame's yet (2 - 6 % of a false chain's explicit headers
        // read one; a true chain's none).  Early in the part the walk RESTARTS behind it -- count, checkpoints and entries begin
        // again: what they held was not the frame's --; kChainPatience bits into the part it STOPS: in run-dominated data a
        // false chain may not merge for a whole part, at five times a true chain's time per bit, and the launch ends with its
        // slowest wavefront (one such part of 4200: 227 against 50 us); the repair then counts the part from its true start.
        for (;;) {
            pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);         // (wave-uniform by construction: the steps' state lives in scalar registers)
            w = (uint32_t)__builtin_amdgcn_readfirstlane((int)w);
            r.s_pos = pos; r.s_w = w;
            const uint32_t span = t.pos - pos;
            const uint32_t every = span / (kChainCk - 8u) > 4096u ? span / (kChainCk - 8u) : 4096u;
            dense = false;
            part_walk<true>(f.W, s_chunk, pos, w, t.pos, f.limit, max_w, cnt, bad, dense, cks + slot * kChainCk, every, n_ck, p != 0u,
                            kChainCk, false, ents + slot * ent_cap, ent_cap, p != 0u, t.pos - X, &n_exp, false, &vote);
            if (dense && chain_verdict(vote_words) == 2u) {                   // a header-dense stack: k_seg_wg's (the record says: no walk)
                PartWalk r0{}; r0.flags = 1u;
                if (!mute_record) chain_walk_publish(walks + slot, r0);
                return;
            }
            if (!dense || bad) break;
            if (pos >= t.pos || pos - X >= patience) {
                stopped = true;
#ifdef TRPX_PART_STATS
                if (lane == 0) printf("walk stopped: frame %u part %u guess flags %x start %u at %u (target %u) patience %u cnt %u\n", frame, p, s.w >> 28, X, pos, t.pos, patience, cnt);
#endif
                break;
            }
            w = 0u;                                                           // (pos: behind the illegal header)
        }
        r.o_pos = pos; r.o_w = w; r.cnt = cnt; r.n_ck = n_ck; r.pad = n_exp;
        r.flags = (bad ? 1u : 0u) | (cnt + 1u > ent_cap - 1u ? 8u : 0u) | (stopped ? 16u : 0u);   // 8: more blocks than entries; 16: stopped on a false chain
    }
    if (!mute_record) chain_walk_publish(walks + slot, r);
#ifdef TRPX_CHAIN_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    const uint64_t st_d = __builtin_amdgcn_s_memrealtime();
#endif
    // the link into the part behind (parts 1 .. P - 2; the last part's is checked by k_chain_index, which walks it by count) -- unless
    // this walk stopped on a false chain: the wavefront that counts this part from its true start goes on through that link
    if (p + 2u < P && (r.flags & 16u) == 0u)
        chain_link_into(terse, terse_bytes, frame_offsets, max_w, P, states, walks, cks, fixes, fixents, ent_cap, frame, p + 1u, r, f, s_chunk);
#ifdef TRPX_CHAIN_STAMPS
    if (lane == 0) {       // diagnostic build (tools/chain_stamps.py): a status block of 16 + 8 * parts words
        __builtin_amdgcn_s_waitcnt(0);
        const uint64_t st_e = __builtin_amdgcn_s_memrealtime();
        uint32_t* o = stamps + 16 + 8 * slot;
        o[0] = (uint32_t)st_a; o[1] = (uint32_t)(st_b - st_a); o[2] = (uint32_t)(st_c - st_b); o[3] = (uint32_t)(st_d - st_c);
        o[4] = f.W.n_fill; o[5] = (uint32_t)(st_e - st_d); o[6] = r.cnt; o[7] = r.n_ck;
    }
#endif
}

// list[0] = count, list[1 + i] = frame (bit 31 clear: the position-parallel walk may look for runs).
// mode[frame]: how the frame's pixels are extracted -- 1: through the decode index (k_chain_index, then the kernels that take the
// widths as given); 0: part by part by the per-frame decoder's walker + extraction waves (k_decode_parts on this table: a second
// walk, but one that hides under the extraction where explicit headers are rare -- 200 x (1030 x 1065) u16 synth-v1: 106 us
// against k_chain_index 24 + k_unpack_tiles 122; where they are frequent the walker is that kernel's bound: Poisson(3) counts
// 200 against 25 + 131).  `narrow` (8 / 16-bit pixels): by the frame's explicit headers per block; 32-bit pixels: always 1.
// One wavefront per frame.
__device__ __forceinline__ void chain_resolve_frame(const PartWalk* walks, const ChainFix* fixes, const FrameGeom& g, uint32_t frame,
                                                    uint32_t P, uint32_t narrow, PartDesc* __restrict__ parts, uint32_t* __restrict__ mode,
                                                    uint32_t* __restrict__ list, uint32_t* __restrict__ status) {
    const uint32_t lane = (uint32_t)lane_id();
    const bool hd = chain_verdict(reinterpret_cast<const uint64_t*>(list) - 4) == 2u;   // (the stack's verdict, ChainVote)
    const PartWalk* wf = walks + (uint64_t)frame * P;
    const ChainFix* xf = fixes + (uint64_t)frame * P;
    PartDesc* __restrict__ pf = parts + (uint64_t)frame * P;
    bool ok = true;
    uint32_t running = 0, n_explicit = 0;
    for (uint32_t base = 0; base < P - 1u; base += kWave) {
        const uint32_t p = base + lane;
        const bool valid = p < P - 1u;
        PartWalk r{};
        ChainFix x{};
        bool good = true, own = true, spliced = false;
        uint32_t cnt = 0;
        PartState st{0u, 0u}, en{0u, 0u};                                     // the part's true start and end states
        if (valid) {
            // (Everything is loaded up front, with clamped indices, and combined without branches: fixes[] of a frame's part 0 is
            // never written and never used -- every use is masked by p.  A first version with the loads inside nested divergent
            // ifs marked EVERY frame for the other route in the optimised build and none with a printf in the loop.)
            const uint32_t p1 = p > 0u ? p - 1u : 0u;
            r = wf[p];
            x = xf[p];
            const PartWalk q = wf[p1];
            const ChainFix xq = xf[p1];
            if (p == 0u) x = ChainFix{};
            // The true end of the part in front: its walk's; of a part whose walk STOPPED on a false chain (flag 16), its repair's
            // (state 2) -- and this part's ChainFix was then left by that same wavefront, from that true end (chain_link_into).
            // A part in front whose walk ran to the cut on a false chain without reading an illegal width (its repair met nothing:
            // state 2 with another end than the walk's) leaves this part's link judged from a false state: the other route.
            const bool q_stopped = p > 0u && (q.flags & 16u) != 0u;
            const bool q_lost = p > 1u && !q_stopped && xq.state == 2u && !(xq.o_pos == q.o_pos && xq.o_w == q.o_w);
            const PartState te = q_stopped ? PartState{xq.o_pos, xq.o_w} : PartState{q.o_pos, q.o_w};
            const bool closed = p == 0u || (te.pos == r.s_pos && te.w == r.s_w);
            const bool use_own = closed && (r.flags & 16u) == 0u;             // starts in the state it was walked from, on the frame's chain
            const bool use_fix = !use_own && (x.state == 1u || x.state == 2u);
            good = (r.flags & 1u) == 0u && (use_own || use_fix) && !q_lost && !(q_stopped && xq.state != 2u);
            st = use_own ? PartState{r.s_pos, r.s_w} : te;
            cnt = use_own ? r.cnt : x.cnt;
            en = use_own || x.state == 1u ? PartState{r.o_pos, r.o_w} : PartState{x.o_pos, x.o_w};
            own = use_own && (r.flags & 8u) == 0u;
            spliced = use_fix && x.n_fix != 0u;                               // (entries: the repair's up to the merge, the walk's own behind it)
            good = good && cnt >= 1u;
        }
        ok = ok && !__ballot(valid && !good);
#ifdef TRPX_PART_STATS
        {   // diagnostic build: status[4..7] = bad walks, repaired links, failed repairs, parts without entries
            const uint32_t n4 = (uint32_t)__builtin_popcountll(__ballot(valid && (r.flags & 1u) != 0u));
            const uint32_t n5 = (uint32_t)__builtin_popcountll(__ballot(valid && p > 0u && (x.state == 1u || x.state == 2u)));
            const uint32_t n6 = (uint32_t)__builtin_popcountll(__ballot(valid && p > 0u && x.state == 3u));
            const uint32_t n7 = (uint32_t)__builtin_popcountll(__ballot(valid && good && !own && !spliced));
            if (lane == 0) { atomicAdd(status + 4, n4); atomicAdd(status + 5, n5); atomicAdd(status + 6, n6); atomicAdd(status + 7, n7); }
        }
#endif
        n_explicit += (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(valid ? r.pad : 0u), 63);
        const uint32_t c = valid && good ? cnt : 0u;
        const uint32_t inc = wave_inclusive_scan(c);
        if (valid && good) {
            PartDesc d;
            d.frame = frame; d.b0 = running + inc - c; d.b1 = d.b0 + c;
            d.pos0 = st.pos; d.w0 = st.w; d.pos1 = en.pos; d.w1 = en.w; d.pad = own ? 1u : (spliced ? 2u : 0u);
            pf[p] = d;
            if (p == P - 2u) {                                                // the frame's last part starts where this one ends
                PartDesc e;
                e.frame = frame; e.b0 = d.b1; e.b1 = g.n_blocks; e.pos0 = en.pos; e.w0 = en.w; e.pos1 = 0u; e.w1 = 0u; e.pad = 0u;
                pf[P - 1u] = e;
            }
        }
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        if (tot >= g.n_blocks - running) ok = false;                          // (the last part holds at least the frame's last block)
        running += ok ? tot : 0u;
    }
    if (lane == 0) mode[frame] = !narrow || !ok || 12u * n_explicit > running ? 1u : 0u;   // (a listed frame's index comes from the other route)
    if (!ok) {
#ifdef TRPX_PART_STATS
        if (frame < 3u && lane == 0) printf("resolve: frame %u not ok, running %u of %u blocks, P %u\n", frame, running, g.n_blocks, P);
#endif
        __builtin_amdgcn_s_waitcnt(0);
        for (uint32_t p = lane; p < P; p += kWave) {
            PartDesc d{};
            d.frame = frame;
            pf[p] = d;                                                        // b1 <= b0: nothing to do for k_chain_index
        }
        if (lane == 0) {
            // bit 31: k_seg_wg's (their number: the word in front of the barrier counter, codec_common.hpp)
            list[1u + atomicAdd(&list[0], 1u)] = frame | (hd ? 0x80000000u : 0u);
            if (hd) atomicAdd(reinterpret_cast<unsigned long long*>(list) - 2, 1ull);
            atomicAdd(status + 2, 1u);                                        // status[2]: frames the index route handed to the position-parallel walk
        }
    }
}

__global__ __launch_bounds__(kWave) void k_chain_resolve(const PartWalk* __restrict__ walks, const ChainFix* __restrict__ fixes, FrameGeom g,
                                                         uint32_t P, uint32_t narrow, PartDesc* __restrict__ parts, uint32_t* __restrict__ mode,
                                                         uint32_t* __restrict__ list, uint32_t* __restrict__ status) {
    chain_resolve_frame(walks, fixes, g, blockIdx.x, P, narrow, parts, mode, list, status);
}

// Walks `nb` blocks from (pos, w_prev) -- general steps, Terse.hpp:360-372 -- and writes their widths to wf[0 .. nb) and the bit
// offset of every block whose frame number b0 + i is a multiple of 256 to tf[(b0 + i) / 256].  at_end: the last of them is the
// frame's last block (nb_last values).  Returns false on a width the pixel type does not have or a chain that leaves the frame.
__device__ __forceinline__ bool chain_walk_abs(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t& pos, uint32_t& w_prev, uint32_t nb,
                                               bool at_end, uint32_t nb_last, uint32_t limit, uint32_t max_w, uint8_t* __restrict__ wf,
                                               uint64_t* __restrict__ tf, uint32_t b0) {
    const uint32_t lane = (uint32_t)lane_id();
    uint32_t b = 0;
    while (b < nb) {
        const uint32_t stride = 1u + (uint32_t)kBlock * w_prev;
        {
            const uint32_t need_lo = (W.frame_sh + pos) >> 5;
            const uint32_t need_hi = ((W.frame_sh + pos + 63u * stride) >> 5) + 2u;
            if ((int32_t)need_lo < W.c_lo || (int32_t)need_hi > W.c_hi) part_fill(W, s_chunk, pos);
        }
        const uint32_t lpos = pos + lane * stride;
        const uint32_t bits = part_bits(W, s_chunk, lpos);
        const uint32_t left = nb - b;
        const uint64_t valid = left >= 64u ? ~0ull : ((1ull << left) - 1ull);
        const uint64_t stop = ~(__ballot((bits & 1u) != 0u) & valid);
        const uint32_t first = stop ? (uint32_t)__builtin_ctzll(stop) : 64u;
        uint32_t e_w = w_prev, new_pos, new_b;
        if (first < left && first < 64u) {                                    // explicit header at block b + first
            auto [w, hl] = parse_explicit_header((uint32_t)__builtin_amdgcn_readlane((int)bits, (int)first));
            if (w > max_w) return false;
            e_w = w;
            const uint32_t nbv = at_end && b + first + 1u == nb ? nb_last : (uint32_t)kBlock;
            new_pos = pos + first * stride + hl + nbv * w;
            new_b = b + first + 1u;
        } else {                                                              // they all repeat the width
            const uint32_t cnt = left < 64u ? left : 64u;
            new_pos = pos + cnt * stride;
            if (at_end && b + cnt == nb) new_pos = pos + (cnt - 1u) * stride + 1u + nb_last * w_prev;
            new_b = b + cnt;
        }
        const uint32_t n_done = new_b - b;
        if (lane < n_done) {
            wf[b + lane] = (uint8_t)(lane < first ? w_prev : e_w);
            if (((b0 + b + lane) & (uint32_t)(kTileBlocks - 1)) == 0u) tf[(b0 + b + lane) / (uint32_t)kTileBlocks] = lpos;
        }
        pos = new_pos; w_prev = e_w; b = new_b;
        if (pos > limit) return false;
    }
    return true;
}

// Entries j .. j + 3 of a part as one dword: its own walk's (E), or -- a repaired part -- the repair's up to the block where the
// chains merged and the walk's own, shifted, behind it.  (Unaligned dword loads; bytes behind the part's last entry are the
// neighbour's or slack and are not used.)
__device__ __forceinline__ uint32_t chain_ent4(const uint8_t* __restrict__ E, const uint8_t* __restrict__ F, uint32_t j, uint32_t b_merge,
                                               int32_t shift) {
    uint32_t q;
    if (!F || j > b_merge) { __builtin_memcpy(&q, E + (int64_t)j + (F ? shift : 0), 4); return q; }
    __builtin_memcpy(&q, F + j, 4);
    if (j + 3u > b_merge) {
        uint32_t e;
        __builtin_memcpy(&e, E + (int64_t)j + shift, 4);
        const uint32_t keep = 0xFFFFFFFFu >> (8u * (3u - (b_merge - j)));   // bytes j .. b_merge from the repair
        q = (q & keep) | (e & ~keep);
    }
    return q;
}

__global__ __launch_bounds__(kWave) void k_chain_index(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                       const uint64_t* __restrict__ frame_offsets, FrameGeom g, uint32_t max_w, uint32_t P,
                                                       uint32_t ent_cap, PartDesc* __restrict__ parts, uint8_t* __restrict__ ents,
                                                       const ChainFix* __restrict__ fixes, const uint8_t* __restrict__ fixents,
                                                       uint8_t* __restrict__ widths, uint64_t* __restrict__ tile_off,
                                                       uint32_t* __restrict__ mode, uint32_t* __restrict__ list, uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint32_t s_chunk[kPartChunkDw + 4];
    const uint32_t lane = (uint32_t)lane_id();
    const PartDesc d = parts[blockIdx.x];
    if (d.b1 <= d.b0 || mode[d.frame] == 0u) return;                          // the frame took another route / is extracted part by part
    const uint32_t frame = d.frame, cnt = d.b1 - d.b0;
    const bool at_end = d.b1 == g.n_blocks;
    const uint32_t nb_last = (uint32_t)(g.n_values - (uint64_t)(g.n_blocks - 1) * kBlock);
    uint8_t* __restrict__ wf = widths + (uint64_t)frame * g.n_blocks + d.b0;
    uint64_t* __restrict__ tf = tile_off + (uint64_t)frame * g.n_tiles;
    const uint64_t fo = frame_offsets[frame], fe = frame_offsets[frame + 1];
    bool done = false, have = (d.pad & 3u) != 0u;
    uint8_t* __restrict__ E = ents + (uint64_t)blockIdx.x * ent_cap;
    if (!have && !at_end && cnt + 2u < ent_cap) {
        // No entries of the true chain (a repair's did not fit, the walk's own overflowed into ...): the part's counting walk once
        // more, fast steps, from its true start to its true end -- into the part's own entry array.
        if (lane < 4u) s_chunk[kPartChunkDw + lane] = 0u;
        PartFrame f = chain_frame(terse, terse_bytes, frame_offsets, frame, P);
        if (f.ok && d.pos0 < d.pos1 && d.pos1 < f.limit) {
            uint32_t pos = d.pos0, w = d.w0, c2 = 0, n0 = 0;
            bool bad = false, dense = false;
            part_walk<true>(f.W, s_chunk, pos, w, d.pos1, f.limit, max_w, c2, bad, dense, nullptr, 0u, n0, false, 0u, false, E, ent_cap);
            __builtin_amdgcn_s_waitcnt(0);                                    // (the entries are read back below)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            have = !bad && c2 == cnt && pos == d.pos1 && w == d.w1;
        }
    }
    if (have && !at_end) {
        // ---- entries -> index: lengths from the widths (Terse.hpp:517-535), positions by a prefix sum; 256 blocks per step, four
        // consecutive ones per lane (one dword of entries in, one dword of widths out), the next step's entries requested first ----
        const uint8_t* __restrict__ F = nullptr;
        uint32_t b_merge = 0;
        int32_t shift = 0;
        if ((d.pad & 2u) != 0u) {
            const ChainFix x = fixes[blockIdx.x];
            F = fixents + (uint64_t)blockIdx.x * ent_cap;
            b_merge = x.b_merge; shift = (int32_t)x.ck_cnt - (int32_t)x.b_merge;
        }
        uint32_t pos = d.pos0;
        bool bad = false;
        uint32_t q = chain_ent4(E, F, 4u * lane, b_merge, shift), w_last = 0;
        const uint32_t w_first = (uint32_t)__builtin_amdgcn_readlane((int)q, 0) & 0xFFu;
        for (uint32_t c = 0; c < cnt; c += 4u * kWave) {
            const uint32_t j0 = c + 4u * lane;
            const uint32_t qn = c + 4u * kWave <= cnt ? chain_ent4(E, F, j0 + 4u * kWave, b_merge, shift) : 0u;   // (entry cnt included)
            uint32_t e4 = (uint32_t)__shfl_down((int)(q & 0xFFu), 1, 64);
            if (lane == 63u) e4 = (uint32_t)__builtin_amdgcn_readlane((int)qn, 0) & 0xFFu;
            const uint32_t e[5] = {q & 0xFFu, (q >> 8) & 0xFFu, (q >> 16) & 0xFFu, q >> 24, e4};
            uint32_t len[4], sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = j0 + (uint32_t)k < cnt;
                len[k] = in ? header_len(e[k + 1], e[k]) + (uint32_t)kBlock * e[k + 1] : 0u;
                bad = bad || (in && e[k + 1] > max_w);
                sum += len[k];
            }
            const uint32_t incl = wave_inclusive_scan(sum);
            uint32_t at = pos + incl - sum;
            const uint32_t packed = e[1] | (e[2] << 8) | (e[3] << 16) | (e[4] << 24);
            if (j0 + 4u <= cnt) __builtin_memcpy(wf + j0, &packed, 4);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (j0 + (uint32_t)k < cnt) wf[j0 + (uint32_t)k] = (uint8_t)e[k + 1];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (j0 + (uint32_t)k < cnt && ((d.b0 + j0 + (uint32_t)k) & (uint32_t)(kTileBlocks - 1)) == 0u)
                    tf[(d.b0 + j0 + (uint32_t)k) / (uint32_t)kTileBlocks] = at;
                at += len[k];
            }
            pos += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            // the width of the part's last block (entry cnt): whichever lane holds it in this step
            const uint32_t rel = cnt - c;                                    // entry cnt = e[rel - 4 * lane] of lane (rel - 1) / 4 ... or lane rel / 4's e[0]
            if (rel <= 4u * kWave) {
                const uint32_t ln = (rel - 1u) / 4u, kk = rel - 4u * ln;     // 1 .. 4
                const uint32_t v = kk == 1u ? e[1] : kk == 2u ? e[2] : kk == 3u ? e[3] : e[4];
                w_last = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)ln);
            }
            q = qn;
        }
        done = !__ballot(bad) && pos == d.pos1 && w_last == d.w1 && w_first == d.w0;
        // (not what the walk arrived at: e.g. a stream whose writer spelled out a width that repeats -- the walk below reads
        // the headers themselves)
    }
    if (!done) {
        if (lane < 4u) s_chunk[kPartChunkDw + lane] = 0u;
        PartFrame f = chain_frame(terse, terse_bytes, frame_offsets, frame, P);
        uint32_t pos = d.pos0, w = d.w0;
        bool ok = f.ok && d.pos0 < f.limit && chain_walk_abs(f.W, s_chunk, pos, w, cnt, at_end, nb_last, f.limit, max_w, wf, tf, d.b0);
        if (ok) ok = at_end ? (pos <= f.limit && 1u + (uint64_t)pos / 8u == fe - fo) : (pos == d.pos1 && w == d.w1);   // S_f (Terse.hpp:547) / the next part's start
        // Not the frame's chain after all (a table k_chain_resolve put together from walks that agreed by chance, or a damaged
        // stream): the frame is listed -- once -- for the position-parallel walk, which writes its whole index again and reports
        // what is corrupt.
        if (!ok && lane == 0 && (atomicOr(&parts[(uint64_t)frame * P].pad, 0x80000000u) & 0x80000000u) == 0u) {
            list[1u + atomicAdd(&list[0], 1u)] = frame;
            atomicAdd(status + 2, 1u);
        }
    }
}

// The words the index route needs cleared in front of every call: the status block (if asked), the deferred-frame count and the
// stack statistics in front of it, and the route's start states, walk records and link records (ChainWs: [states, cks) -- the
// link records too: a wavefront that skips a link writes none, and a record left by an earlier call must not be read as this
// call's).  One launch.
__global__ __launch_bounds__(kThreads) void k_chain_zero(uint64_t* __restrict__ p, uint64_t n, uint64_t* __restrict__ q, uint64_t m,
                                                         uint64_t* __restrict__ r, uint64_t k) {
    const uint64_t i0 = (uint64_t)blockIdx.x * kThreads + threadIdx.x, stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = i0; i < k; i += stride) r[i] = 0ull;
    for (uint64_t i = i0; i < n; i += stride) p[i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x < m) q[threadIdx.x] = 0ull;
}
hipError_t launch_chain_zero(const DecodeArgs& a, uint32_t max_w, bool clear_status, hipStream_t st) {
    (void)max_w;
    const uint32_t P = a.plan.parts_per_frame;
    if (P < 4u || !a.part_ws || !a.defer) return hipErrorInvalidValue;
    const ChainWs l = chain_ws_layout(a.geom, a.n_frames, P);
    const uint64_t k = l.cks / 8;
    hipLaunchKernelGGL(k_chain_zero, dim3((uint32_t)((k + 4 * kThreads - 1) / (4 * kThreads))), dim3(kThreads), 0, st,
                       reinterpret_cast<uint64_t*>(a.defer) - kDeferSlots * kDeferSlotWords, (uint64_t)(kDeferSlots * kDeferSlotWords + 1),
                       reinterpret_cast<uint64_t*>(a.status), (uint64_t)(clear_status ? 4 : 0), reinterpret_cast<uint64_t*>(a.part_ws), k);
    return hipGetLastError();
}

// Fills a.widths / a.tile_off for every frame that works out and lists the others in a.defer.  The caller has cleared the route's
// words (launch_chain_zero) earlier on the stream.
hipError_t launch_build_index_chain(const DecodeArgs& a, uint32_t max_w, const uint32_t** frame_mode, hipStream_t st) {
    const uint32_t P = a.plan.parts_per_frame;
    if (P < 4u || !a.parts || !a.part_ws || !a.defer) return hipErrorInvalidValue;
    const ChainWs l = chain_ws_layout(a.geom, a.n_frames, P);
    char* ws = static_cast<char*>(a.part_ws);
    PartState* states = reinterpret_cast<PartState*>(ws + l.states);
    PartWalk* walks = reinterpret_cast<PartWalk*>(ws + l.walks);
    ChainFix* fixes = reinterpret_cast<ChainFix*>(ws + l.fixes);
    PartCk* cks = reinterpret_cast<PartCk*>(ws + l.cks);
    uint8_t* ents = reinterpret_cast<uint8_t*>(ws + l.ents);
    uint8_t* fixents = reinterpret_cast<uint8_t*>(ws + l.fixents);
    uint32_t* modes = reinterpret_cast<uint32_t*>(ws + l.modes);
    uint64_t* vote_words = reinterpret_cast<uint64_t*>(a.defer) - 4;             // (ChainVote: [0] verdict, [1] votes; cleared by launch_chain_zero)
    const uint32_t cap = chain_ent_cap(a.geom.n_blocks, P);
    hipLaunchKernelGGL(k_chain_walk, dim3(a.n_frames * P), dim3(kWave), 0, st, a.terse, (uint64_t)a.terse_bytes, a.frame_offsets, max_w, P, cap,
                       states, walks, cks, ents, fixes, fixents, vote_words, a.status);
    hipLaunchKernelGGL(k_chain_resolve, dim3(a.n_frames), dim3(kWave), 0, st, static_cast<const PartWalk*>(walks),
                       static_cast<const ChainFix*>(fixes), a.geom, P, a.plan.narrow ? 1u : 0u, a.parts, modes, a.defer, a.status);
    hipLaunchKernelGGL(k_chain_index, dim3(a.n_frames * P), dim3(kWave), 0, st, a.terse, (uint64_t)a.terse_bytes, a.frame_offsets, a.geom,
                       max_w, P, cap, a.parts, ents, static_cast<const ChainFix*>(fixes), static_cast<const uint8_t*>(fixents), a.widths,
                       a.tile_off, modes, a.defer, a.status);
    *frame_mode = modes;
    return hipGetLastError();
}

}  // namespace trpx
