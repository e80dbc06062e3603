// A RUN of consecutive 256-block groups of one frame on one wavefront, as the kernels that walk a whole stack through its decode
// index see it (decode_sparse.hip: trpx_decode_sparse, decode_dot.hip: trpx_decode_dot, decode_bins.hip: trpx_decode_bins,
// decode_binned.hip: trpx_decode_binned): what belongs to the run is loaded once
// (the frame's bytes, the groups' offsets: one per lane), and the blocks a group chooses are compacted into consecutive lanes
// through a per-wavefront list in LDS, 64 at a time.  The group itself: group_front.hpp.
#pragma once
#include "codec_common.hpp"
#include "group_front.hpp"

namespace trpx {

constexpr int kWavesPerWg = kThreads / kWave;
constexpr uint32_t kRun = 8;                                // consecutive groups of one frame per wavefront
static_assert(kRun * kGroupRows <= kWave && kRun < kWave, "a run's offsets and flag words: one per lane");

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
__device__ __forceinline__ void list_sync() {               // the wavefront's LDS writes are seen by its other lanes' reads behind this
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The support words of group grp's rows (one bit per block of a frame: trpx_decode_dot's and trpx_decode_bins' "some map / some
// label wants this block"): the lane's block's bit is bit lane % 32 of s[r]
__device__ __forceinline__ void group_load_support(uint32_t (&s)[kGroupRows], const uint32_t* __restrict__ support, uint32_t n_words,
                                                   uint32_t grp, uint32_t lane) {
#pragma unroll
    for (int r = 0; r < kGroupRows; ++r) {
        const uint32_t word = grp * (kTileBlocks / 32) + r * (kWave / 32) + (lane >> 5);
        s[r] = word < n_words ? support[word] : 0u;
    }
}

// what a wavefront holds for its run: lane j the offset of group g0 + j (lane n: the group behind the run)
struct Run {
    uint64_t frame, u0, fo, fe, my_off;
    uint32_t g0, n;
    const uint8_t* __restrict__ wf;
};
// where the run lies (arithmetic only) ...
__device__ __forceinline__ Run run_place(const IndexedStack& a, uint64_t run, uint32_t runs_per_frame) {
    const FrameGeom& g = a.geom;
    Run r;
    r.frame = run / runs_per_frame;
    r.g0 = (uint32_t)(run - r.frame * runs_per_frame) * kRun;
    r.n = g.n_tiles - r.g0 < kRun ? g.n_tiles - r.g0 : kRun;
    r.u0 = r.frame * g.n_tiles + r.g0;
    r.wf = a.widths + r.frame * g.n_blocks;
    return r;
}
// ... and what is loaded once for it
__device__ __forceinline__ void run_load(Run& r, const IndexedStack& a, uint32_t lane) {
    r.fo = a.frame_offsets[r.frame];
    r.fe = a.frame_offsets[r.frame + 1];
    r.my_off = lane <= r.n && r.g0 + lane < a.geom.n_tiles ? a.tile_off[r.u0 + lane] : 0ull;
}

}  // namespace trpx
