// A RUN of consecutive 256-block groups of one frame on one wavefront, as the kernels that walk a whole stack through its decode
// index see it (decode_sparse.hip: trpx_decode_sparse, decode_dot.hip: trpx_decode_dot, decode_bins.hip: trpx_decode_bins,
// decode_binned.hip: trpx_decode_binned).  The group itself: group_front.hpp.  THE WALK, written here once:
//
//   run_at / run_place, run_load   where the run lies, and what is loaded once for it (the frame's bytes, the groups' offsets: one
//                                  per lane)
//   run_groups    per chosen group of the run: its widths (and, where the consumer has them, its support words) were prefetched
//                 during the group before -> header_len + 12 * w -> wave scans from the group's offset -> the group validated
//                 against its frame and the next group's offset, unconditionally (so the whole stack is) -> the caller's step.
//                 Returns "a group failed": such a group is never handed on, it adds nothing.
//   list_compact  the blocks of the group the caller wants, in block order, compacted into consecutive entries of the wavefront's
//                 list in LDS (ballot + lanes below)
//   list_rounds   per 64 entries one round: the lane's entry -> block, values, width, payload bit -> the payload dwords straight
//                 from the stream into registers and the register extraction (group_extract) -> the caller's body
//   run_walk      the three composed, with the verdict (run_verdict: CORRUPT into the status word), for the consumers that need
//                 nothing between them
// and around it: runs_per_frame / support_words (host and device), support_write (the "some pixel of this block is wanted" bits),
// for_each_run (a wavefront per run, strided), k_reduce_parts (partial sums in part order).
#pragma once
#include <type_traits>
#include "codec_common.hpp"
#include "group_front.hpp"

namespace trpx {

constexpr int kWavesPerWg = kThreads / kWave;
constexpr uint32_t kRun = 8;                                // consecutive groups of one frame per wavefront
static_assert(kRun * kGroupRows <= kWave && kRun < kWave, "a run's offsets and flag words: one per lane");

__host__ __device__ inline uint32_t runs_per_frame(const FrameGeom& g) { return (g.n_tiles + kRun - 1) / kRun; }
// one bit per block of a frame, in 32-bit words
__host__ __device__ inline size_t support_words(const FrameGeom& g) { return ((size_t)g.n_blocks + 31) / 32; }

__device__ __forceinline__ uint64_t lane_value64(uint64_t v, uint32_t src) {
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, (int)src, kWave) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, kWave) << 32);
}
// lanes below this one in a ballot
__device__ __forceinline__ uint32_t lanes_below(uint64_t ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}
// The wavefront's list of chosen blocks in LDS (kTileBlocks entries, block order): written by the lanes that own the blocks,
// read 64 at a time by consecutive lanes.  An entry: payload bit in the group (17 bits: a group has < 2^17 bits), width (6),
// block in the group (8).
__device__ __forceinline__ uint32_t list_entry(uint32_t off, uint32_t w, uint32_t block) { return off | (w << 17) | (block << 23); }
__device__ __forceinline__ uint32_t entry_off(uint32_t e) { return e & 0x1FFFFu; }
__device__ __forceinline__ uint32_t entry_width(uint32_t e) { return (e >> 17) & 63u; }
__device__ __forceinline__ uint32_t entry_block(uint32_t e) { return e >> 23; }
__device__ __forceinline__ void list_sync() {               // the wavefront's LDS writes are seen by its other lanes' reads behind this
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t* wave_list() {          // this wavefront's list (one array per workgroup, whoever asks)
    __shared__ uint32_t s_list[kWavesPerWg * kTileBlocks];
    return s_list + wave_id() * kTileBlocks;
}

// The support words (one bit per block of a frame: trpx_decode_dot's and trpx_decode_bins' "some map / some label wants this
// block") as a consumer hands them to the walk; NoSupport: the consumer has none, and the walk neither loads nor carries any.
struct SupportWords { const uint32_t* __restrict__ words; uint32_t n_words; };
struct NoSupport {};
// those of group grp's rows: the lane's block's bit is bit lane % 32 of s[r]
__device__ __forceinline__ void group_load_support(uint32_t (&s)[kGroupRows], const SupportWords& support, uint32_t grp, uint32_t lane) {
#pragma unroll
    for (int r = 0; r < kGroupRows; ++r) {
        const uint32_t word = grp * (kTileBlocks / 32) + r * (kWave / 32) + (lane >> 5);
        s[r] = word < support.n_words ? support.words[word] : 0u;
    }
}
__device__ __forceinline__ void group_load_support(uint32_t (&)[kGroupRows], const NoSupport&, uint32_t, uint32_t) {}
__device__ __forceinline__ bool support_bit(const uint32_t (&s)[kGroupRows], int r, uint32_t lane) { return (s[r] >> (lane & 31u)) & 1u; }

// Writes them: bit b = any(first pixel of block b, its values), for every block of a frame.  The whole grid calls it.
template <typename Any>
__device__ __forceinline__ void support_write(uint32_t* __restrict__ support, const FrameGeom& g, Any&& any) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t n_words = (uint32_t)support_words(g);
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t b0 = (uint64_t)blockIdx.x * kThreads + (uint32_t)wave_id() * kWave; b0 < g.n_blocks; b0 += stride) {   // (b0: uniform)
        const uint64_t b = b0 + lane;
        bool some = false;
        if (b < g.n_blocks) {
            const uint64_t first = b * kBlock;
            some = any(first, first + kBlock <= g.n_values ? (uint32_t)kBlock : (uint32_t)(g.n_values - first));
        }
        const uint64_t ballot = __ballot(some);
        const uint32_t word = (uint32_t)(b0 >> 5);
        if (lane == 0 && word < n_words) support[word] = (uint32_t)ballot;
        if (lane == 32 && word + 1 < n_words) support[word + 1] = (uint32_t)(ballot >> 32);
    }
}

// what a wavefront holds for its run: lane j the offset of group g0 + j (lane n: the group behind the run)
struct Run {
    uint64_t frame, u0, fo, fe, my_off;
    uint32_t g0, n;
    const uint8_t* __restrict__ wf;
};
// where the run lies (arithmetic only): the groups [g0, g0 + n) of `frame`, n <= kRun; run number `run` of runs_per_frame a frame ...
__device__ __forceinline__ Run run_at(const IndexedStack& a, uint64_t frame, uint32_t g0, uint32_t n) {
    Run r;
    r.frame = frame;
    r.g0 = g0;
    r.n = n;
    r.u0 = frame * a.geom.n_tiles + g0;
    r.wf = a.widths + frame * a.geom.n_blocks;
    return r;
}
__device__ __forceinline__ Run run_place(const IndexedStack& a, uint64_t run, uint32_t runs_per_frame) {
    const uint64_t frame = run / runs_per_frame;
    const uint32_t g0 = (uint32_t)(run - frame * runs_per_frame) * kRun;
    return run_at(a, frame, g0, a.geom.n_tiles - g0 < kRun ? a.geom.n_tiles - g0 : kRun);
}
// ... and what is loaded once for it
__device__ __forceinline__ void run_load(Run& r, const IndexedStack& a, uint32_t lane) {
    r.fo = a.frame_offsets[r.frame];
    r.fe = a.frame_offsets[r.frame + 1];
    r.my_off = lane <= r.n && r.g0 + lane < a.geom.n_tiles ? a.tile_off[r.u0 + lane] : 0ull;
}
// the groups of a run that a walk takes, in rising order: all n of them, or those of a mask (not empty).  (Two types, not
// the mask alone: counting costs two SGPRs less, which k_binned_bands would spill.)
struct AllGroups {
    uint32_t n, j = 0;
    __device__ bool left() const { return j < n; }
    __device__ uint32_t first() const { return j; }
    __device__ void pop() { ++j; }
};
struct MaskGroups {
    uint64_t mask;
    __device__ bool left() const { return mask != 0ull; }
    __device__ uint32_t first() const { return (uint32_t)__builtin_ctzll(mask); }
    __device__ void pop() { mask &= mask - 1; }
};

// The groups `todo` of the loaded run R: step(j, w, nb, sup, off, gs) for every group that is valid -- per row r the lane's
// block's width, values, support word (Support = SupportWords only) and first payload bit, and where the payload is read from.
// The next chosen group's loads are in flight during a group.  True: a group was not valid.
template <typename T, typename Groups, typename Support, typename Step>
__device__ __forceinline__ bool run_groups(const IndexedStack& a, const Run& R, Groups todo, const Support& support, uint32_t lane, Step&& step) {
    const FrameGeom& g = a.geom;
    uint32_t wn[kGroupRows], nbn[kGroupRows], wp0n[kGroupRows], sn[kGroupRows];
    group_load_widths(wn, nbn, wp0n, R.wf, g, R.g0 + todo.first(), lane);
    group_load_support(sn, support, R.g0 + todo.first(), lane);
    bool bad = false;
#pragma unroll 1
    while (todo.left()) {
        const uint32_t j = todo.first();
        todo.pop();
        uint32_t w[kGroupRows], nb[kGroupRows], wp0[kGroupRows], sup[kGroupRows], off[kGroupRows];
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) {
            w[r] = wn[r]; nb[r] = nbn[r]; wp0[r] = wp0n[r];
            if constexpr (std::is_same_v<Support, SupportWords>) sup[r] = sn[r];
        }
        if (todo.left()) {                                  // in flight during this group
            group_load_widths(wn, nbn, wp0n, R.wf, g, R.g0 + todo.first(), lane);
            group_load_support(sn, support, R.g0 + todo.first(), lane);
        }
        const uint64_t t_off = lane_value64(R.my_off, j), t_next = lane_value64(R.my_off, j + 1);
        if (!group_offsets<T>(off, w, nb, wp0, R.fo, R.fe, t_off, t_next, R.g0 + j + 1 == g.n_tiles, a.terse_bytes, lane)) {
            bad = true;                                     // (validated whether or not a block of it is wanted)
            continue;
        }
        step(j, w, nb, sup, off, group_stream(a.terse, a.terse_bytes, R.fo, t_off));
    }
    return bad;
}
__device__ __forceinline__ void run_verdict(bool bad, uint32_t* __restrict__ status, uint32_t lane) {
    if (bad && lane == 0) atomicMax(&status[0], kStatusCorrupt);
}

// The blocks of a group whose lanes say want(r), r = 0 .. kGroupRows - 1 in this order and once each (all 64 lanes call it: it
// may vote), in block order into consecutive entries of the list; returns their number.
template <typename Want>
__device__ __forceinline__ uint32_t list_compact(uint32_t* __restrict__ list, const uint32_t (&off)[kGroupRows], const uint32_t (&w)[kGroupRows],
                                                 uint32_t lane, Want&& want) {
    uint32_t n = 0;
#pragma unroll
    for (int r = 0; r < kGroupRows; ++r) {
        const bool mine = want(r);
        const uint64_t ballot = __ballot(mine);
        if (mine) list[n + lanes_below(ballot)] = list_entry(off[r], w[r], r * kWave + lane);
        n += (uint32_t)__builtin_popcountll(ballot);
    }
    list_sync();
    return n;
}

// The n entries of the list of group grp, 64 a round: body(c, block, nr, o, have) with entry 64 * c + lane's block (of the
// frame), its nr values extracted into o; have false (and nr 0) behind the list's end.  All 64 lanes run the body.
template <typename T, typename Body>
__device__ __forceinline__ void list_rounds(const uint32_t* __restrict__ list, uint32_t n, uint32_t grp, const FrameGeom& g, const GroupStream& gs,
                                            uint32_t lane, Body&& body) {
#pragma unroll 1
    for (uint32_t c = 0; c * kWave < n; ++c) {
        const bool have = c * kWave + lane < n;
        const uint32_t e = have ? list[c * kWave + lane] : 0u;
        const uint32_t block = grp * kTileBlocks + entry_block(e);
        const uint32_t left = (uint32_t)g.n_values - block * kBlock;   // (listed blocks lie inside the frame: < 2^29 values)
        const uint32_t nr = have ? (left < (uint32_t)kBlock ? left : (uint32_t)kBlock) : 0u;
        uint32_t o[PackedDwords<T>::n];
        group_extract<T>(o, gs, have, entry_width(e), nr, entry_off(e));
        body(c, block, nr, o, have);
    }
    list_sync();                                            // (the next group rewrites the list)
}

// The whole walk of the run R (placed, not yet loaded) for a consumer with nothing between the steps: of every valid group the
// CANDIDATE blocks -- those with values, their support bit where there is support, and want(block of the frame, width, values) --
// through body as list_rounds hands them on; a group that is not valid sets CORRUPT.
template <typename T, typename Support, typename Want, typename Body>
__device__ __forceinline__ void run_walk(const IndexedStack& a, Run R, const Support& support, uint32_t* __restrict__ status,
                                         uint32_t* __restrict__ list, Want&& want, Body&& body) {
    const uint32_t lane = (uint32_t)lane_id();
    run_load(R, a, lane);
    const bool bad = run_groups<T>(a, R, AllGroups{R.n}, support, lane,
        [&](uint32_t j, const uint32_t (&w)[kGroupRows], const uint32_t (&nb)[kGroupRows], const uint32_t (&sup)[kGroupRows],
            const uint32_t (&off)[kGroupRows], const GroupStream& gs) {
            const uint32_t grp = R.g0 + j;
            const uint32_t n = list_compact(list, off, w, lane, [&](int r) {
                if constexpr (std::is_same_v<Support, SupportWords>)
                    if (!support_bit(sup, r, lane)) return false;
                return nb[r] != 0u && want(grp * kTileBlocks + r * kWave + lane, w[r], nb[r]);
            });
            list_rounds<T>(list, n, grp, a.geom, gs, lane, body);
        });
    run_verdict(bad, status, lane);
}

// A wavefront per run, strided over the grid: f(run, the wavefront's list)
template <typename F>
__device__ __forceinline__ void for_each_run(uint64_t runs, F&& f) {
    uint32_t* const list = wave_list();
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerWg;
    for (uint64_t run = (uint64_t)blockIdx.x * kWavesPerWg + (uint32_t)wave_id(); run < runs; run += stride) f(run, list);
}

// per (frame, k): the frame's parts' partial sums [n_frames][parts][n], added in part order -> out[n_frames][n].  Every element
// is written.  (A template, as k_zero_words is: the units that launch it emit it.)
template <int kUnused = 0>
__global__ __launch_bounds__(kThreads) void k_reduce_parts(const int64_t* __restrict__ partials, uint64_t n_frames, uint32_t parts, uint32_t n,
                                                           int64_t* __restrict__ out) {
    const uint64_t total = n_frames * n;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t frame = i / n;
        const uint32_t k = (uint32_t)(i - frame * n);
        uint64_t s = 0;
        for (uint32_t p = 0; p < parts; ++p) s += (uint64_t)partials[(frame * parts + p) * n + k];
        out[i] = (int64_t)s;
    }
}

}  // namespace trpx
