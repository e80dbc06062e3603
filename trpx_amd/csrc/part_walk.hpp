// What both large-frame routes share (gfx950 / CDNA4): a frame of more than kPartMaxBlocks blocks is cut into PARTS at bit
// positions, and a wavefront per part walks the header chain with the serial walker's cheap steps -- one per RUN of equal widths --
// behind an LDS window of the stream.  Here, in reading order: the words the routes leave in HBM (start state, checkpoint, walk
// record), the window (PartWin, part_fill, part_bits), the pieces of the search for a start state inside a run (part_header_phase,
// part_try), the stack's vote (ChainVote), the walker (part_walk) and the recount from a true state (part_rewalk), and a frame's
// geometry (PartFrame).  decode_part.hip builds the index route on them (the one large frames take), decode_part_sel4.hip
// round 4's parts route (selector 4 only).
#pragma once
#include "codec_common.hpp"
#include "launchers.hpp"
#include "lds_dma.hpp"

namespace trpx {

constexpr int kPartChunkDw = 2048;             // the walker's stream window: 8 KB
constexpr uint32_t kPartEvid = 32;             // header bits of evidence for a start inside a run: a stack has thousands of cuts x 10^5 candidates each, and with 24 bits one guess per stack WAS wrong -- on a chain that, in run-dominated data, does not merge before its part ends (the frame then takes the other route: +4 ms)
constexpr uint32_t kPartSkip = 12;             // the start lies this many blocks inside the evidence (the bits in front of a run are 1 half the time)
constexpr uint32_t kPartSearch = 8;            // passes of 2048 candidate positions behind X_p
constexpr uint32_t kPartCk = 256;              // checkpoints per part
constexpr uint32_t kPartWeak = 0x80000000u;    // PartState::w: a plain guess (not expected to be a state of the chain)
constexpr uint32_t kPartAmbig = 0x40000000u;   //   ... because runs were found, but not which of their passing positions is the header's
constexpr uint32_t kPartRuns = 0x20000000u;    //   ... (index route) although runs of equal widths lie nearby: run-dominated data, where a false chain is slow to merge
constexpr uint32_t kPartReady = 0x10000000u;   //   (index route) the state has been published: k_chain_walk's wavefronts wait for their neighbour's
constexpr uint32_t kPartFlags = kPartWeak | kPartAmbig | kPartRuns | kPartReady;

struct PartState { uint32_t pos, w; };
struct PartCk { uint32_t pos, w, cnt; };
struct PartWalk {                              // what k_part_walk / k_chain_walk leave per (frame, part p < P - 1)
    uint32_t o_pos, o_w;                       // OUT_p: the state at the chain's first block start >= T_p
    uint32_t cnt;                              // blocks started in [S_p, T_p)
    uint32_t flags;                            // 1: the chain left the frame / held an illegal width; 2: too dense for the serial walker
    uint32_t n_ck;                             // checkpoints left behind
    uint32_t s_pos, s_w;                       // (index route) the state the counting walk started in: the guess, or behind the last illegal width
    uint32_t pad;                              // (index route) explicit headers among the blocks counted
};

// Checkpoints and walk records are read by OTHER wavefronts of the launch that writes them (index route: k_chain_walk's links), on
// other XCDs: agent-scope atomic words -- write-through stores, loads that do not trust a cached line -- ordered by the record's
// `published` bit alone.  (Fences instead write back or invalidate the XCD's whole L2, dirty with the walk's entries: measured,
// 45 - 100 us per launch of 4000 wavefronts.)
constexpr uint32_t kWalkPublished = 0x80000000u;   // PartWalk::flags
__device__ __forceinline__ void part_ck_store(PartCk* dst, const PartCk& c) {
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    __hip_atomic_store(d, c.pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d + 1, c.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(d + 2, c.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ PartCk part_ck_load(const PartCk* src) {
    const uint32_t* d = reinterpret_cast<const uint32_t*>(src);
    PartCk c;
    c.pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));   // (wave-uniform address)
    c.w = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(d + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    c.cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(d + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return c;
}

struct PartWin {                               // the frame's stream behind an LDS window
    const uint32_t* s32;
    uint64_t n_dw, frame_dw;                   // dwords of the stream; dword of the frame's first bit
    uint32_t frame_sh;                         // bit of the frame's first bit inside that dword
    bool base16;
    int32_t c_lo, c_hi;                        // the window holds dwords [c_lo, c_hi) of the frame
#ifdef TRPX_CHAIN_STAMPS
    uint32_t n_fill = 0, t_fill = 0;           // diagnostic build: window fills and the 10 ns ticks they took
#endif
};

// Window := the kPartChunkDw dwords from the (16-byte aligned) dword that holds frame bit `pos` on.
__device__ __forceinline__ void part_fill(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t pos) {
    const uint32_t lane = (uint32_t)lane_id();
#ifdef TRPX_CHAIN_STAMPS
    const uint64_t st_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    const uint32_t need_lo = (W.frame_sh + pos) >> 5;
    W.c_lo = (int32_t)(((W.frame_dw + need_lo) & ~3ull) - W.frame_dw);
    W.c_hi = W.c_lo + kPartChunkDw;
    const uint64_t d0 = (uint64_t)((int64_t)W.frame_dw + W.c_lo);
    __builtin_amdgcn_wave_barrier();           // (every lane is through with the old window)
    if (W.base16 && (d0 & 3) == 0 && d0 + kPartChunkDw <= W.n_dw) {
#pragma unroll
        for (int it = 0; it < kPartChunkDw / (kWave * 4); ++it) {
            // (wave-uniform by construction; said again for the builds in which the compiler loses sight of it: "invalid operand")
            const uint64_t src = uniform64((uintptr_t)(W.s32 + d0 + it * kWave * 4));
            const uint32_t lds_base = uniform32((uint32_t)(uintptr_t)&s_chunk[it * kWave * 4]);
            lds_dma16(reinterpret_cast<const uint32_t*>((uintptr_t)src), lane * 16u, lds_base);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        for (uint32_t i = lane * 4; i < (uint32_t)kPartChunkDw; i += kWave * 4)
            *reinterpret_cast<uint4*>(&s_chunk[i]) = load_stream16_guarded(W.s32, d0 + i, W.n_dw);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#ifdef TRPX_CHAIN_STAMPS
    __builtin_amdgcn_s_waitcnt(0);
    ++W.n_fill; W.t_fill += (uint32_t)(__builtin_amdgcn_s_memrealtime() - st_t0);
#endif
}

// 32 stream bits from frame bit q on (inside the window)
__device__ __forceinline__ uint32_t part_bits(const PartWin& W, const uint32_t* __restrict__ s_chunk, uint32_t q) {
    const uint32_t fbit = W.frame_sh + q - 32u * (uint32_t)W.c_lo;
    const uint32_t i = fbit >> 5 < (uint32_t)kPartChunkDw ? fbit >> 5 : (uint32_t)kPartChunkDw - 1u;   // (s_chunk has 4 dwords of slack)
    return __builtin_amdgcn_alignbit(s_chunk[i + 1u], s_chunk[i], fbit);
}

// The searches for a start state (part_try here, part_guess in decode_part_sel4.hip) look for kPartEvid header bits 1 at stride
// s = 1 + 12 w behind a cut: a position kPartSkip blocks inside such a run is a block start with all but certainty.
//
// Pixels with a pedestal (raw detector counts: every value in 100 .. 107, say) have CONSTANT payload bits, and those pass the
// test at the run's own stride just like its header bits: the first passing position is then a payload bit's more often than
// not, a chain started there stays beside the frame's for as long as the run lasts, and every cut of every frame is wrong the
// same way.  But the passing positions of one stride are a header's plus, for every constant bit b of the pixels, the twelve
// positions header + 1 + b + j w of that bit in the block's twelve fields: the header is the one passing position relative to
// which all the others fall into complete classes of twelve (part_header_phase; one passing position per stride, the case
// without a pedestal, needs no such test).
__device__ __forceinline__ bool part_pm_bit(const uint32_t* __restrict__ pm, uint32_t i) { return ((pm[i >> 5] >> (i & 31u)) & 1u) != 0u; }

// pm: pass bits of 2048 consecutive positions; r0: the first passing one; s, w: the stride and its width.  Returns the index of
// the header among the passing positions in [r0, r0 + s), or ~0 if that cannot be told (fewer than s positions left, no or
// several consistent ones).
__device__ __forceinline__ uint32_t part_header_phase(const uint32_t* __restrict__ pm, uint32_t r0, uint32_t s, uint32_t w) {
    const uint32_t lane = (uint32_t)lane_id();
    if (r0 + 2u * s > 2048u) return ~0u;
    uint32_t n = 0;
    for (uint32_t i = lane; i < s; i += kWave) n += part_pm_bit(pm, r0 + i) ? 1u : 0u;
    n = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(n), 63);
    if (n == 1u) return r0;
    if (n % 12u != 1u) return ~0u;
    uint32_t found = ~0u, n_found = 0, found_any = ~0u, n_any = 0;
    for (uint32_t base = 0; base < s; base += kWave) {
        const uint32_t c = base + lane;                                        // candidate header: position r0 + c
        bool ok = c < s && part_pm_bit(pm, r0 + c);
        // (the grid of twelve fields may be shifted along a run of constant bits and still fit -- constant bits 5 and 6 of 7 read
        // as {0, 6} one position to the left, as {0, 1} two --: a pedestal's constant bits are the TOP ones, w - k .. w - 1, and
        // only the candidate whose complete classes are exactly such a run counts.  `top` = length of the run of complete classes
        // that ends at bit w - 1.)
        uint32_t classes = 0, top = 0;
        for (uint32_t b = 0; b < w && __ballot(ok); ++b) {
            uint32_t cnt = 0;
#pragma unroll
            for (uint32_t j = 0; j < (uint32_t)kBlock; ++j) {
                uint32_t o = c + 1u + b + j * w;                               // < 2 s
                o = o >= s ? o - s : o;
                cnt += ok && part_pm_bit(pm, r0 + o) ? 1u : 0u;
            }
            ok = ok && (cnt == 0u || cnt == (uint32_t)kBlock);
            classes += cnt == (uint32_t)kBlock ? 1u : 0u;
            top = cnt == (uint32_t)kBlock ? top + 1u : 0u;
        }
        ok = ok && 1u + (uint32_t)kBlock * classes == n;
        // (The grid shifted by one bit ALWAYS fits too: a pedestal's top bit w - 1 is constant, and seen from the position in
        // front of the header -- the last field's top bit -- the header bits are class 0 and every class b is class b + 1.  What
        // tells them apart: the block's width says bit w - 1 is set somewhere, in a pedestal everywhere -- the true grid HAS class
        // w - 1, the shifted one only if bit w - 2 is constant too, and then the top-run rule decides.  Pixels 40 or 41: bits 5
        // and 3 -- no top run, but only one grid with class 5.)
        const uint64_t m_any = __ballot(ok && top >= 1u);
        if (m_any) { n_any += (uint32_t)__builtin_popcountll(m_any); found_any = r0 + base + (uint32_t)__builtin_ctzll(m_any); }
        const uint64_t m = __ballot(ok && top == classes);
        if (m) { n_found += (uint32_t)__builtin_popcountll(m); found = r0 + base + (uint32_t)__builtin_ctzll(m); }
    }
    return n_any == 1u ? found_any : (n_found == 1u ? found : ~0u);
}

// One (width, pass) of that search, for the index route's staged variant (chain_guess, decode_part.hip): kPartEvid header bits 1
// at stride 1 + 12 w from the 2048 positions behind X0.  Returns the state's position or ~0; depth = evidence bits the last candidates survived.
__device__ __forceinline__ uint32_t part_try(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t* __restrict__ s_pm, uint32_t X0, uint32_t w,
                                             uint32_t& depth, uint32_t& surv12) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t s = 1u + (uint32_t)kBlock * w;
    uint32_t a = 0xFFFFFFFFu, k = 0;
    surv12 = 0;
    for (; k < kPartEvid; k += 4u) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) a &= part_bits(W, s_chunk, X0 + 32u * lane + (k + i) * s);
        if (!__ballot(a != 0u)) break;
        if (k == 8u) surv12 = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan((uint32_t)__builtin_popcount(a)), 63);   // positions with 12 header bits 1 at this stride
    }
    depth = k;
    const uint64_t hits = __ballot(a != 0u);
    if (!hits) return ~0u;
    const int l0 = __builtin_ctzll(hits);
    const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)a, l0);
    const uint32_t r0 = 32u * (uint32_t)l0 + (uint32_t)__builtin_ctz(a0);
    __builtin_amdgcn_wave_barrier();
    s_pm[lane] = a;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t h = part_header_phase(s_pm, r0, s, w);
    return h != ~0u ? X0 + h + kPartSkip * s : ~0u;
}

// ---- is the stack header-dense?  (the index route's vote, k_chain_walk) ----------------------------------------------------------------
// The serial walkers of the index route take a step per explicit header: 370 us for 200 x (1030 x 1065) Poisson(3) frames (one block
// in four starts with one), which the lane-per-segment walk of decode_seg.hip (k_seg_wg: one workgroup per frame) does in 290.  On
// run-dominated frames it is the other way round (plain guesses inside runs do not merge: 3.2 ms for 200 synth-v1 frames).  What
// tells the two apart is the share of explicit headers on a TRUE chain (Poisson(3): one block in four; the int32 test frames: one in
// nine; synth-v1: one in sixty) -- the position-parallel walk's run search does not (random bits pass its eight-header test
// somewhere in most windows) --, and part 0 of every frame starts ON the true chain.  So the wavefronts of part 0 of up to sixteen
// frames spread over the stack first walk their share of ~1000 blocks and VOTE (blocks and explicit headers into one atomic
// word; ~10 us), the last voter writes the verdict (more than one block in six: header-dense), and every part looks at it between
// the passes of its guess and at its checkpoints until it reads "run-dominated": a header-dense stack's walkers stop within
// ~20 us of the launch, k_chain_resolve lists its frames (bit 31) and k_seg_wg walks them.  The verdict is the STACK's: a frame judged alone by a hundred blocks is misjudged once in a few
// hundred, and ONE frame on the other route costs the call that route's whole latency.  Only the speed hangs on it -- either walk is
// checked the same way --; where the frames' heads mislead, blank heads keep the stack on this route (round 5's time) and k_seg_wg
// hands a frame back whose links do not close.  The two words live in front of the hand-over list (codec_common.hpp: [-3] votes,
// [-4] verdict), cleared by the call's first launch.
constexpr uint32_t kChainVoters = 16;
__host__ __device__ inline uint32_t chain_voters(uint32_t n_frames) { return n_frames < kChainVoters ? n_frames : kChainVoters; }
struct ChainVote {
    const uint64_t* words;     // words[0] = verdict (0: none yet, 1: run-dominated, 2: header-dense), words[1] = voters << 56 | blocks << 28 | explicit headers
    bool settled;              // the verdict was "run-dominated" when last looked at: it is final, no more looks
};
__device__ __forceinline__ uint32_t chain_verdict(const uint64_t* words) {
#ifdef TRPX_CHAIN_NO_CLASSIFY                                  // (test build, make noclassify: every stack through the serial walkers, as in round 5)
    return 1u;
#elif defined(TRPX_CHAIN_ALL_DENSE)                            // (test build, make alldense: every stack to k_seg_wg)
    return 2u;
#else
    return (uint32_t)__hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
// A look at the verdict (at a checkpoint of a walk, between the passes of a guess); true: the stack is header-dense, stop.
__device__ __forceinline__ bool chain_vote_look(ChainVote& v) {
    if (v.settled) return false;
    const uint32_t verdict = chain_verdict(v.words);
    v.settled = verdict == 1u;
    return verdict == 2u;
}
// A voter's vote: b blocks with n_exp explicit headers; the last of the stack's voters writes the verdict.
__device__ __forceinline__ void chain_vote_cast(uint64_t* words, uint32_t voters, uint32_t b, uint32_t n_exp) {
    if (lane_id() != 0) return;
    const uint64_t mine = (1ull << 56) | ((uint64_t)(b < 0xFFFFFu ? b : 0xFFFFFu) << 28) | (uint64_t)(n_exp < 0xFFFFFu ? n_exp : 0xFFFFFu);
    const uint64_t all = __hip_atomic_fetch_add(words + 1, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + mine;
    if ((uint32_t)(all >> 56) == voters) {
        const uint64_t blocks = (all >> 28) & 0xFFFFFFFull, expl = all & 0xFFFFFFFull;
        __hip_atomic_store(words, blocks >= 512u && 6u * expl > blocks ? 2ull : 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Walks the chain from (pos, w) and counts the blocks that start in front of frame bit T; leaves the state at the first block
// start >= T, and in ck[] the state and count at the first step end behind every `ck_every` bits (a state of the chain at a
// block boundary: another chain that has merged with this one passes through it).  dense: more than one explicit header in 6
// blocks over 2048 blocks and more -- the walk stops (two serial walks of such a part, this one and the decoder's,
// cost more than the position-parallel walk of the frame).  tolerant: the walk started from a plain guess, i.e. on a chain
// that is not the frame's until it has merged with it -- such a chain may hold anything, also widths the pixel type does not
// have: it goes on from there with width 0 (what it counts in front of the merge is never used).  The steps are decode_frame.hip's (one per run of equal widths + the explicit header that ends it, the header
// parsed on the scalar unit) without the position entries; the fast loop only takes steps whose 64 candidates all lie in
// front of T and inside the window, the general step does the rest.
//
// STORE (the index route, see k_chain_walk): every step also leaves ent[j] = width of the block BEFORE the part's block j, for the 64
// candidates of the step (one byte store per lane, no mask: what lies behind the step's last block is overwritten by the next
// step, a wavefront's stores to one address arrive in program order), indices clamped to ent_cap - 1 -- a part that counts more
// blocks than its entry array holds has no entries, which the caller sees from the count.  ent[count] = the width in front of
// the block the walk stopped at.  ck == nullptr: no checkpoints and no density stop (ck_cap: entries ck[] has room for;
// stop_dense: the serial walker's hand-over test, round 4's parts route only).
template <bool STORE = false>
__device__ __forceinline__ void part_walk(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t& pos, uint32_t& w_prev, uint32_t T,
                                          uint32_t limit, uint32_t max_w, uint32_t& count, bool& bad, bool& dense,
                                          PartCk* __restrict__ ck, uint32_t ck_every, uint32_t& n_ck, bool tolerant,
                                          uint32_t ck_cap = kPartCk, bool stop_dense = true, uint8_t* __restrict__ ent = nullptr,
                                          uint32_t ent_cap = 1u, bool abort_illegal = false, uint32_t prio_span = 0u,
                                          uint32_t* __restrict__ exp_out = nullptr, bool ratio_stop = false, ChainVote* vote = nullptr) {
    const uint32_t lane = (uint32_t)lane_id();
    uint32_t b = 0, n_exp = 0, b_ref = 0, exp_ref = 0;
    uint32_t ck_next = ck ? pos + ck_every : 0xFFFFFFFFu;
    [[maybe_unused]] const uint32_t capm1 = ent_cap - 1u;
    n_ck = 0;
    while (pos < T && !bad) {
        if (pos >= ck_next) {
            if (n_ck < ck_cap && lane == 0) part_ck_store(ck + n_ck, PartCk{pos, w_prev, b});
            n_ck = n_ck < ck_cap ? n_ck + 1u : n_ck;
            ck_next = pos + ck_every;
            if (vote && chain_vote_look(*vote)) { dense = true; break; }      // (k_chain_walk: a header-dense stack is k_seg_wg's)
            if (ratio_stop) {
                // (run-dominated locales, k_chain_walk: more than 35 % explicit headers over a checkpoint interval is a chain that is
                // not the frame's -- a false chain reads one at every other block -- even if it has not read an illegal width yet)
                if (b - b_ref >= 32u && (n_exp - exp_ref) * 20u > (b - b_ref) * 7u) { dense = true; break; }
                b_ref = b; exp_ref = n_exp;
            }
            if (prio_span) {
                // The SIMD's arbiter serves equal-priority waves oldest first: of the ~17 walkers of a CU the last to arrive finished
                // at 115 - 137 us, the median at 65 (eight 4096 x 4096 frames, tools/chain_stamps.py) -- and a walker alone on its SIMD
                // cannot use the issue slots the others left.  Priority by what is LEFT of the part keeps them level.
                const uint32_t left = T - pos;
                if (4u * left > 3u * prio_span) __builtin_amdgcn_s_setprio(3);
                else if (2u * left > prio_span) __builtin_amdgcn_s_setprio(2);
                else if (4u * left > prio_span) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
            }
            // (a chain that is not the frame's yet may look like anything until it has merged: a tolerant walk's count starts
            // at its sixteenth checkpoint)
            // (the weakparts test build never stops one: every part there has to get through k_part_repair)
            if (tolerant && n_ck == 16u) { b_ref = b; exp_ref = n_exp; }
#ifdef TRPX_PART_FORCE_WEAK
            constexpr bool stoppable = false;
#else
            const bool stoppable = stop_dense && (!tolerant || n_ck >= 16u);
#endif
            if (stoppable && b - b_ref >= 2048u && (n_exp - exp_ref) * 6u > b - b_ref) { dense = true; break; }
        }
        uint32_t stride = 1u + (uint32_t)kBlock * w_prev;
        {   // the window holds the 64 candidates of a step from here
            const uint32_t need_lo = (W.frame_sh + pos) >> 5;
            const uint32_t need_hi = ((W.frame_sh + pos + 63u * stride) >> 5) + 2u;
            if ((int32_t)need_lo < W.c_lo || (int32_t)need_hi > W.c_hi) part_fill(W, s_chunk, pos);
        }
        {
            const uint32_t base8 = 8u * (uint32_t)(uintptr_t)&s_chunk[0];               // the window's LDS address, in bits
            uint32_t pw = W.frame_sh + pos - 32u * (uint32_t)W.c_lo + base8;             // the header's bit address in LDS
            uint32_t pw_end = 32u * (uint32_t)(W.c_hi - W.c_lo - 1) + base8;
            const uint64_t t_rel = (uint64_t)W.frame_sh + T - 32ull * (uint64_t)(int64_t)W.c_lo;   // (c_lo >= -3; T >= pos: inside or behind the window)
            if (t_rel + base8 < (uint64_t)pw_end) pw_end = (uint32_t)t_rel + base8;       // candidates stay in front of T
            {   // ... and the fast steps end where the next checkpoint is due
                const uint32_t c_pw = W.frame_sh + ck_next - 32u * (uint32_t)W.c_lo + base8 + 64u * stride;
                if (ck_next - pos < 0x4000000u && c_pw < pw_end) pw_end = c_pw;
            }
            uint32_t pw_max = pw_end - 63u * stride;
            uint32_t v_ls = __umul24(lane, stride);
            uint32_t s_bad = 0, t_first, t_h, t_t, t_p, t_a, t_bits;
            // (the steps' state lives in scalar registers -- wave-uniform by construction, which the compiler cannot always see through
            // the callers' loops: "illegal VGPR to SGPR copy" in some builds, not in others)
            pw = uniform32(pw); pw_end = uniform32(pw_end); pw_max = uniform32(pw_max); stride = uniform32(stride); b = uniform32(b); n_exp = uniform32(n_exp); w_prev = uniform32(w_prev);
#define TRPX_PART_STEP_ASM(ST_STEP, ST_WIDTH)                                                                                  \
                "s_cmp_lt_i32 %[pw], %[pwmax]\n\t"                                                                             \
                "s_cbranch_scc0 9f\n"                                                                                          \
                "1:\n\t"                                                                                                       \
                "v_add_u32 %[p], %[pw], %[ls]\n\t"                 /* this lane's candidate header */                          \
                "v_lshrrev_b32 %[a], 3, %[p]\n\t"                                                                              \
                "v_and_b32 %[a], 0x1ffffffc, %[a]\n\t"                                                                         \
                "ds_read2_b32 v[62:63], %[a] offset1:1\n\t"                                                                    \
                ST_STEP                                              /* (in the LDS read's shadow) */                          \
                "s_waitcnt lgkmcnt(0)\n\t"                                                                                     \
                "v_alignbit_b32 %[bits], v63, v62, %[p]\n\t"                                                                   \
                "v_and_b32 %[a], 1, %[bits]\n\t"                                                                               \
                "v_cmp_eq_u32 vcc, 0, %[a]\n\t"                   /* lanes whose block has an explicit header (Terse.hpp:361) */ \
                "s_cbranch_vccz 5f\n\t"                                                                                        \
                "s_ff1_i32_b64 %[first], vcc\n\t"                                                                              \
                "v_readlane_b32 %[h], %[bits], %[first]\n\t"                                                                   \
                "s_bfe_u32 %[w], %[h], 0x30001\n\t"               /* Terse.hpp:362 */                                          \
                "s_cmp_lg_u32 %[w], 7\n\t"                                                                                     \
                "s_cbranch_scc0 6f\n\t"                                                                                        \
                "s_addc_u32 %[b], %[b], %[first]\n\t"             /* b += first + 1 (SCC = 1) */                               \
                "s_add_i32 %[nexp], %[nexp], 1\n\t"                                                                            \
                "s_mul_i32 %[t], %[first], %[stride]\n\t"                                                                      \
                "s_mul_i32 %[stride], %[w], 12\n\t"                                                                            \
                "s_add_i32 %[pw], %[pw], %[t]\n\t"                                                                             \
                "s_add_i32 %[stride], %[stride], 1\n\t"                                                                        \
                "s_add_i32 %[pw], %[pw], %[stride]\n\t"                                                                        \
                "s_add_i32 %[pw], %[pw], 3\n"                      /* pos += first * stride + 4 + 12 w */                       \
                "3:\n\t"                                                                                                       \
                ST_WIDTH                                                                                                       \
                "v_mul_u32_u24 %[ls], %[stride], %[lane]\n\t"                                                                  \
                "s_mul_i32 %[t], %[stride], 63\n\t"                                                                            \
                "s_sub_i32 %[pwmax], %[pwend], %[t]\n"                                                                         \
                "4:\n\t"                                                                                                       \
                "s_cmp_lt_i32 %[pw], %[pwmax]\n\t"                                                                             \
                "s_cbranch_scc1 1b\n\t"                                                                                        \
                "s_branch 9f\n"                                                                                                \
                "5:\n\t"                                           /* 64 blocks repeat the width */                            \
                "s_lshl_b32 %[t], %[stride], 6\n\t"                                                                            \
                "s_add_i32 %[pw], %[pw], %[t]\n\t"                                                                             \
                "s_add_i32 %[b], %[b], 64\n\t"                                                                                 \
                "s_branch 4b\n"                                                                                                \
                "6:\n\t"                                           /* widths >= 7: Terse.hpp:364-370 */                        \
                "s_bfe_u32 %[t], %[h], 0x20004\n\t"                                                                            \
                "s_add_i32 %[w], %[t], 7\n\t"                                                                                  \
                "s_mul_i32 %[t], %[first], %[stride]\n\t"                                                                      \
                "s_add_i32 %[pw], %[pw], %[t]\n\t"                                                                             \
                "s_add_i32 %[pw], %[pw], 6\n\t"                                                                                \
                "s_cmp_lg_u32 %[w], 10\n\t"                                                                                    \
                "s_cbranch_scc1 7f\n\t"                                                                                        \
                "s_bfe_u32 %[t], %[h], 0x60006\n\t"                                                                            \
                "s_add_i32 %[w], %[t], 10\n\t"                                                                                 \
                "s_add_i32 %[pw], %[pw], 6\n"                                                                                  \
                "7:\n\t"                                                                                                       \
                "s_cmp_gt_u32 %[w], %[maxw]\n\t"                                                                               \
                "s_cbranch_scc1 8f\n\t"                                                                                        \
                "s_add_i32 %[b], %[b], %[first]\n\t"                                                                           \
                "s_add_i32 %[b], %[b], 1\n\t"                                                                                  \
                "s_add_i32 %[nexp], %[nexp], 1\n\t"                                                                            \
                "s_mul_i32 %[stride], %[w], 12\n\t"                                                                            \
                "s_add_i32 %[pw], %[pw], %[stride]\n\t"                                                                        \
                "s_add_i32 %[stride], %[stride], 1\n\t"                                                                        \
                "s_branch 3b\n"                                                                                                \
                "8:\n\t"                                                                                                       \
                "s_mov_b32 %[bad], 1\n"                                                                                        \
                "9:\n"
            if constexpr (STORE) {
                uint32_t t_eo, v_wv = w_prev;
                const uint32_t capm1_u = uniform32(capm1), max_w_u = uniform32(max_w);
                uint8_t* const ent_u = reinterpret_cast<uint8_t*>((uintptr_t)uniform64((uintptr_t)ent));
                asm volatile(TRPX_PART_STEP_ASM("v_add_u32 %[eo], %[b], %[lane]\n\t"
                                                "v_min_u32 %[eo], %[capm1], %[eo]\n\t"
                                                "global_store_byte %[eo], %[wv], %[ebase]\n\t",
                                                "v_mov_b32 %[wv], %[w]\n\t")
                    : [pw] "+s"(pw), [b] "+s"(b), [nexp] "+s"(n_exp), [w] "+s"(w_prev), [stride] "+s"(stride), [pwmax] "+s"(pw_max),
                      [ls] "+v"(v_ls), [bad] "+s"(s_bad), [first] "=&s"(t_first), [h] "=&s"(t_h), [t] "=&s"(t_t), [p] "=&v"(t_p),
                      [a] "=&v"(t_a), [bits] "=&v"(t_bits), [eo] "=&v"(t_eo), [wv] "+v"(v_wv)
                    : [lane] "v"(lane), [pwend] "s"(pw_end), [maxw] "s"(max_w_u), [capm1] "s"(capm1_u), [ebase] "s"(ent_u)
                    : "vcc", "scc", "memory", "v62", "v63");
            } else {
                const uint32_t max_w_u = uniform32(max_w);
                asm volatile(TRPX_PART_STEP_ASM("", "")
                    : [pw] "+s"(pw), [b] "+s"(b), [nexp] "+s"(n_exp), [w] "+s"(w_prev), [stride] "+s"(stride), [pwmax] "+s"(pw_max),
                      [ls] "+v"(v_ls), [bad] "+s"(s_bad), [first] "=&s"(t_first), [h] "=&s"(t_h), [t] "=&s"(t_t), [p] "=&v"(t_p),
                      [a] "=&v"(t_a), [bits] "=&v"(t_bits)
                    : [lane] "v"(lane), [pwend] "s"(pw_end), [maxw] "s"(max_w_u)
                    : "vcc", "scc", "memory", "v62", "v63");
            }
#undef TRPX_PART_STEP_ASM
            pos = pw - base8 + 32u * (uint32_t)W.c_lo - W.frame_sh;
            if (s_bad) {
                if (!tolerant) { bad = true; break; }
                if (abort_illegal) { dense = true; break; }                               // (a chain that is not the frame's: see k_chain_walk)
                w_prev = 0u;                                                              // (pos: behind the illegal header)
            }
        }
        if (pos >= T) break;
        if (pos > limit) { bad = true; break; }
        if (pos >= ck_next) continue;                                             // (the fast steps stopped for a checkpoint: no general step)
        stride = 1u + (uint32_t)kBlock * w_prev;
        {
            const uint32_t need_lo = (W.frame_sh + pos) >> 5;
            const uint32_t need_hi = ((W.frame_sh + pos + 63u * stride) >> 5) + 2u;
            if ((int32_t)need_lo < W.c_lo || (int32_t)need_hi > W.c_hi) { part_fill(W, s_chunk, pos); continue; }   // the window's end stopped the fast steps
        }
        // ---- general step: the candidates in front of T (Terse.hpp:360-372) ----
        const uint32_t lpos = pos + lane * stride;
        const uint32_t bits = part_bits(W, s_chunk, lpos);
        const uint32_t k_raw = (T - pos + stride - 1u) / stride;              // candidates with lpos < T (>= 1)
        const uint32_t kT = k_raw < 64u ? k_raw : 64u;
        const uint64_t valid = kT >= 64u ? ~0ull : ((1ull << kT) - 1ull);
        const uint64_t stop = ~(__ballot((bits & 1u) != 0u) & valid);
        const uint32_t first = stop ? (uint32_t)__builtin_ctzll(stop) : 64u;
        if constexpr (STORE) {                                                // the width in front of this step's blocks
            const uint32_t n_done = first < kT ? first + 1u : kT;
            if (lane < n_done) ent[b + lane < capm1 ? b + lane : capm1] = (uint8_t)w_prev;
        }
        if (first < kT) {                                                     // explicit header at candidate `first`
            auto [w, hl] = parse_explicit_header((uint32_t)__builtin_amdgcn_readlane((int)bits, (int)first));
            if (w > max_w) {
                if (!tolerant) { bad = true; break; }
                if (abort_illegal) {                                          // (stops behind the illegal header, as the fast steps do)
                    pos += first * stride + hl; w_prev = 0u; b += first + 1u;
                    dense = true;
                    break;
                }
                w = 0u;
            }
            pos += first * stride + hl + (uint32_t)kBlock * w;
            w_prev = w;
            b += first + 1u;
            ++n_exp;
        } else {                                                              // they all repeat the width
            pos += kT * stride;
            b += kT;
        }
        if (pos > limit) { bad = true; break; }
    }
    count = b;
    if (exp_out) *exp_out = n_exp;                                            // explicit headers among the blocks counted
    if constexpr (STORE) {
        if (lane == 0) ent[b < capm1 ? b : capm1] = (uint8_t)w_prev;
    }
}

// Counts the blocks of a part again from the true state (pos, w) -- general steps only -- until the chain passes through a
// checkpoint of the part's first walk (the chains have merged: the rest of that walk is this chain's) or reaches T.
// Returns 1: merged, `count` = the part's blocks; 2: at T, `count` / (pos, w) are the part's count and end state; 3: failed.
__device__ __forceinline__ uint32_t part_rewalk(PartWin& W, uint32_t* __restrict__ s_chunk, uint32_t& pos, uint32_t& w_prev, uint32_t T,
                                                uint32_t limit, uint32_t max_w, const PartCk* __restrict__ ck, uint32_t n_ck,
                                                uint32_t walk_cnt, uint32_t& count) {
    const uint32_t lane = (uint32_t)lane_id();
    uint32_t b = 0, ci = 0;
    PartCk c{0xFFFFFFFFu, 0u, 0u};
    if (n_ck) c = ck[0];
    while (pos < T) {
        while (ci < n_ck && c.pos < pos) { ++ci; c = ci < n_ck ? ck[ci] : PartCk{0xFFFFFFFFu, 0u, 0u}; }
        const uint32_t stride = 1u + (uint32_t)kBlock * w_prev;
        {
            const uint32_t need_lo = (W.frame_sh + pos) >> 5;
            const uint32_t need_hi = ((W.frame_sh + pos + 63u * stride) >> 5) + 2u;
            if ((int32_t)need_lo < W.c_lo || (int32_t)need_hi > W.c_hi) part_fill(W, s_chunk, pos);
        }
        const uint32_t lpos = pos + lane * stride;
        const uint32_t bits = part_bits(W, s_chunk, lpos);
        const uint32_t k_raw = (T - pos + stride - 1u) / stride;              // candidates with lpos < T (>= 1)
        const uint32_t kT = k_raw < 64u ? k_raw : 64u;
        const uint64_t valid = kT >= 64u ? ~0ull : ((1ull << kT) - 1ull);
        const uint64_t stop = ~(__ballot((bits & 1u) != 0u) & valid);
        const uint32_t first = stop ? (uint32_t)__builtin_ctzll(stop) : 64u;
        const uint32_t n_run = first < kT ? first : kT - 1u;                  // candidates 0 .. n_run are block starts in front of T, width before them: w_prev
        // a checkpoint among them?
        while (ci < n_ck && c.pos <= pos + n_run * stride) {
            if ((c.pos - pos) % stride == 0u && c.w == w_prev) { count = b + (c.pos - pos) / stride + (walk_cnt - c.cnt); return 1u; }
            ++ci; c = ci < n_ck ? ck[ci] : PartCk{0xFFFFFFFFu, 0u, 0u};
        }
        if (first < kT) {                                                     // explicit header at candidate `first` (Terse.hpp:362-370)
            auto [w, hl] = parse_explicit_header((uint32_t)__builtin_amdgcn_readlane((int)bits, (int)first));
            if (w > max_w) return 3u;
            pos += first * stride + hl + (uint32_t)kBlock * w;
            w_prev = w;
            b += first + 1u;
        } else {
            pos += kT * stride;
            b += kT;
        }
        if (pos > limit) return 3u;
    }
    count = b;
    return 2u;
}

// The frame's cut positions: X_p = p * L.
__device__ __forceinline__ uint32_t part_len_bits(uint32_t limit, uint32_t P) {
    return (uint32_t)((((uint64_t)limit + P - 1u) / P + 127u) & ~127ull);
}

struct PartFrame { PartWin W; uint32_t limit, L; bool ok; };
__device__ __forceinline__ PartFrame part_frame(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                const uint64_t* __restrict__ frame_offsets, uint32_t frame, uint32_t P) {
    PartFrame f{};
    const uint64_t fo = frame_offsets[frame], fe = frame_offsets[frame + 1];
    f.ok = fe > fo && fe <= terse_bytes && 8 * (fe - fo) < 0xF0000000ull;
    if (!f.ok) return f;
    f.W.s32 = reinterpret_cast<const uint32_t*>(terse);
    f.W.n_dw = (terse_bytes + 3) / 4;
    f.W.frame_dw = (8 * fo) >> 5;
    f.W.frame_sh = (uint32_t)((8 * fo) & 31);
    f.W.base16 = ((uintptr_t)terse & 15) == 0;
    f.W.c_lo = f.W.c_hi = 0;
    f.limit = (uint32_t)(8 * (fe - fo));
    f.L = part_len_bits(f.limit, P);
    return f;
}

}  // namespace trpx
