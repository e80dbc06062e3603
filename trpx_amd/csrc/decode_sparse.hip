// Threshold decode (trpx_decode_sparse): a stack with its decode index -> the pixels at or above a threshold as (row offsets,
// positions, values), without expanding the frames.  The order of the output is fixed (by frame, then by pixel), so the
// shape is count -> scan -> write.  The two kernels that read the stream give a wavefront a RUN of kRun consecutive 256-block
// groups of one frame and walk it with the pieces of group_runs.hpp (run_groups, list_compact, list_rounds): the run's counts,
// bases and flag words are loaded and stored coalesced, one per lane, in one access each.
//
//   k_sparse_count       every group of every frame.  The CANDIDATE blocks are those wide enough to hold an event (a block's
//                        width bounds its values); per round the compare on the extracted values -> per group the number of
//                        events and a 256-bit set, bit i = "candidate i (in block order) has events".  A group that fails
//                        validation sets CORRUPT and counts nothing.
//   k_sparse_frame_scan  per frame (one wavefront): exclusive scan of its groups' counts, the frame's total
//   k_sparse_stack_scan  one workgroup: exclusive scan of the frames' totals -> row_offsets; CAPACITY when the total exceeds it
//   k_sparse_write       groups with events only (run_groups over a mask): the candidates that have events compacted and extracted
//                        again, each event stored at row_offsets[frame] + base[group] + its rank in the group (block order,
//                        then k), under index < capacity.
// HBM traffic: the widths (and 16 bytes per group) twice at most, the payload of the candidate blocks, 40 bytes per group of
// counts / flags / bases, the events.  Nothing depends on the order in which wavefronts run: the output is bit-identical across runs.
#include "codec_common.hpp"
#include "decode_sparse.hpp"
#include "group_front.hpp"
#include "group_runs.hpp"

namespace trpx {

namespace {

// the lane's block's values (first nr of the 12 in o) at or above the threshold: the comparison is on the extracted value
template <typename T>
__device__ __forceinline__ uint32_t event_mask(const uint32_t (&o)[PackedDwords<T>::n], uint32_t nr, int64_t threshold) {
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < kBlock; ++k)
        if ((uint32_t)k < nr && (int64_t)packed_value<T>(o, k) >= threshold) mask |= 1u << k;
    return mask;
}

__device__ __forceinline__ uint64_t pick64(uint32_t k, uint64_t v0, uint64_t v1, uint64_t v2, uint64_t v3) {   // (values, not references: the choice stays in registers)
    return k == 0u ? v0 : k == 1u ? v1 : k == 2u ? v2 : v3;
}

template <typename T>
__device__ __forceinline__ void sparse_count_run(const SparseArgs& a, uint64_t run, uint32_t runs_per_frame, uint32_t* __restrict__ list) {
    const uint32_t lane = (uint32_t)lane_id();
    Run R = run_place(a, run, runs_per_frame);
    run_load(R, a, lane);
    uint32_t my_count = 0;                                  // lane j: group g0 + j's events
    uint64_t my_flags = 0;                                  // lane 4 * j + c: "has events" of its candidates 64 c .. 64 c + 63
    const bool bad = run_groups<T>(a, R, AllGroups{R.n}, NoSupport{}, lane,   // (not valid: count 0, no flags: the later passes never touch the group)
        [&](uint32_t j, const uint32_t (&w)[kGroupRows], const uint32_t (&nb)[kGroupRows], const uint32_t (&)[kGroupRows],
            const uint32_t (&off)[kGroupRows], const GroupStream& gs) {
            // (the width: an optimisation only, the verdict is the compare on the values)
            const uint32_t n_cand = list_compact(list, off, w, lane, [&](int r) { return nb[r] != 0u && w[r] >= a.min_width; });
            uint32_t count = 0;
            list_rounds<T>(list, n_cand, R.g0 + j, a.geom, gs, lane,
                [&](uint32_t c, uint32_t, uint32_t nr, const uint32_t (&o)[PackedDwords<T>::n], bool have) {
                    const uint32_t mask = have ? event_mask<T>(o, nr, a.threshold) : 0u;
                    count += (uint32_t)__builtin_popcount(mask);
                    const uint64_t has = __ballot(mask != 0u);
                    if (lane == (uint32_t)kGroupRows * j + c) my_flags = has;
                });
            const uint32_t inc = wave_inclusive_scan(count);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            if (lane == j) my_count = total;
        });
    run_verdict(bad, a.status, lane);
    if (lane < R.n) a.counts[R.u0 + lane] = my_count;
    if (lane < (uint32_t)kGroupRows * R.n) a.flags[kGroupRows * R.u0 + lane] = my_flags;
}

template <typename T>
__device__ __forceinline__ void sparse_write_run(const SparseArgs& a, uint64_t run, uint32_t runs_per_frame, uint32_t* __restrict__ list) {
    const uint32_t lane = (uint32_t)lane_id();
    Run R = run_place(a, run, runs_per_frame);
    const uint32_t my_count = lane < R.n ? a.counts[R.u0 + lane] : 0u;
    const uint64_t todo = __ballot(my_count != 0u);         // the run's groups with events
    if (todo == 0ull) return;                               // (after one load)
    run_load(R, a, lane);
    const uint32_t my_base = lane < R.n ? a.base[R.u0 + lane] : 0u;
    const uint64_t my_flags = lane < (uint32_t)kGroupRows * R.n ? a.flags[kGroupRows * R.u0 + lane] : 0ull;
    const uint64_t row = a.row_offsets[R.frame];
    T* __restrict__ values = static_cast<T*>(a.values);
    run_groups<T>(a, R, MaskGroups{todo}, NoSupport{}, lane,           // (no verdict: a group with a count was valid)
        [&](uint32_t j, const uint32_t (&w)[kGroupRows], const uint32_t (&nb)[kGroupRows], const uint32_t (&)[kGroupRows],
            const uint32_t (&off)[kGroupRows], const GroupStream& gs) {
            // ---- the candidates again, in the count pass's order; those it found events in go into the list: the predicate
            // ranks the row's candidates first (list_compact calls it row by row)
            const uint32_t l0 = (uint32_t)kGroupRows * j;
            const uint64_t has0 = uniform64(lane_value64(my_flags, l0)), has1 = uniform64(lane_value64(my_flags, l0 + 1)),
                           has2 = uniform64(lane_value64(my_flags, l0 + 2)), has3 = uniform64(lane_value64(my_flags, l0 + 3));
            uint32_t n_cand = 0;
            const uint32_t n_list = list_compact(list, off, w, lane, [&](int r) {
                const bool cand = nb[r] != 0u && w[r] >= a.min_width;
                const uint64_t ballot = __ballot(cand);
                const uint32_t i = n_cand + lanes_below(ballot);              // the block's place among the candidates
                n_cand += (uint32_t)__builtin_popcountll(ballot);
                return cand && ((pick64(i >> 6, has0, has1, has2, has3) >> (i & 63u)) & 1ull);
            });
            uint64_t at = row + (uint32_t)__shfl((int)my_base, (int)j, kWave);   // where the group's next event goes
            list_rounds<T>(list, n_list, R.g0 + j, a.geom, gs, lane,
                [&](uint32_t, uint32_t block, uint32_t nr, const uint32_t (&o)[PackedDwords<T>::n], bool have) {
                    const uint32_t mask = have ? event_mask<T>(o, nr, a.threshold) : 0u;
                    const uint32_t m = (uint32_t)__builtin_popcount(mask);
                    const uint32_t inc = wave_inclusive_scan(m);
                    uint64_t i = at + (inc - m);            // rank: the blocks in front (block order), then k ascending
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        if (mask & (1u << k)) {
                            if (i < a.capacity) {
                                a.positions[i] = block * kBlock + k;
                                values[i] = packed_value<T>(o, k);
                            }
                            ++i;
                        }
                    }
                    at += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
                });
        });
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kThreads) void k_sparse_count(SparseArgs a, uint32_t runs_per_frame) {
    for_each_run(a.n_frames * runs_per_frame, [&](uint64_t run, uint32_t* __restrict__ list) { sparse_count_run<T>(a, run, runs_per_frame, list); });
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_sparse_write(SparseArgs a, uint32_t runs_per_frame) {
    for_each_run(a.n_frames * runs_per_frame, [&](uint64_t run, uint32_t* __restrict__ list) { sparse_write_run<T>(a, run, runs_per_frame, list); });
}

// per frame, one wavefront: exclusive scan of the groups' counts (a frame has < 2^29 pixels: 32 bits), the frame's total
__global__ __launch_bounds__(kThreads) void k_sparse_frame_scan(const uint32_t* __restrict__ counts, uint64_t n_frames, uint32_t n_tiles,
                                                                 uint32_t* __restrict__ base, uint32_t* __restrict__ frame_total) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerWg;
    for (uint64_t frame = (uint64_t)blockIdx.x * kWavesPerWg + (uint32_t)wave_id(); frame < n_frames; frame += stride) {
        uint32_t carry = 0;
        for (uint32_t g0 = 0; g0 < n_tiles; g0 += kWave) {
            const uint32_t i = g0 + lane;
            const uint32_t c = i < n_tiles ? counts[frame * n_tiles + i] : 0u;
            const uint32_t inc = wave_inclusive_scan(c);
            if (i < n_tiles) base[frame * n_tiles + i] = carry + inc - c;
            carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
        if (lane == 0) frame_total[frame] = carry;
    }
}

// one workgroup: exclusive scan of the frames' totals -> row_offsets[0 .. n_frames]; the total against the capacity
__global__ __launch_bounds__(kThreads) void k_sparse_stack_scan(const uint32_t* __restrict__ frame_total, uint64_t n_frames, uint64_t capacity,
                                                                 uint64_t* __restrict__ row_offsets, uint32_t* __restrict__ status) {
    __shared__ uint64_t s_tot[kWavesPerWg];
    uint64_t carry = 0;
    for (uint64_t f0 = 0; f0 < n_frames; f0 += kThreads) {
        const uint64_t i = f0 + threadIdx.x;
        const uint64_t v = i < n_frames ? (uint64_t)frame_total[i] : 0ull;
        const uint64_t inc = wave_inclusive_scan64(v);
        if (lane_id() == 63) s_tot[wave_id()] = inc;
        __syncthreads();
        uint64_t wbase = 0;
        for (int k = 0; k < wave_id(); ++k) wbase += s_tot[k];
        if (i < n_frames) row_offsets[i] = carry + wbase + inc - v;
        for (int k = 0; k < kWavesPerWg; ++k) carry += s_tot[k];
        __syncthreads();                                    // (s_tot is reused by the next round)
    }
    if (threadIdx.x == 0) {
        row_offsets[n_frames] = carry;
        if (carry > capacity) atomicMax(&status[0], (uint32_t)TRPX_ERR_CAPACITY);   // (CORRUPT, the graver code, stays)
    }
}

uint32_t sparse_min_width(int64_t threshold, bool stream_signed) {
    if (threshold <= 0) return 0;                           // zeros are events: width-0 blocks too
    uint32_t bl = 0;
    for (uint64_t t = (uint64_t)threshold; t; t >>= 1) ++bl;
    return bl + (stream_signed ? 1u : 0u);                  // w-bit two's complement fields hold up to 2^(w - 1) - 1
}

hipError_t launch_decode_sparse(int dtype, const SparseArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    // launch shapes from the geometry alone: a wavefront per run of kRun groups up to 4096 workgroups, strided runs beyond
    const uint32_t rpf = runs_per_frame(a.geom);
    const uint32_t grid = grid_capped(a.n_frames * rpf, kWavesPerWg);
    const uint32_t fgrid = grid_capped(a.n_frames, kWavesPerWg);
    return for_pixel_type(dtype, [&]<class T>() {
        hipLaunchKernelGGL((k_sparse_count<T>), dim3(grid), dim3(kThreads), 0, st, a, rpf);
        hipLaunchKernelGGL(k_sparse_frame_scan, dim3(fgrid), dim3(kThreads), 0, st, a.counts, a.n_frames, a.geom.n_tiles, a.base, a.frame_total);
        hipLaunchKernelGGL(k_sparse_stack_scan, dim3(1), dim3(kThreads), 0, st, a.frame_total, a.n_frames, a.capacity, a.row_offsets, a.status);
        if (a.positions) hipLaunchKernelGGL((k_sparse_write<T>), dim3(grid), dim3(kThreads), 0, st, a, rpf);
        return hipGetLastError();
    });
}

}  // namespace trpx
