// Binned decode (trpx_decode_binned): a stack with its decode index -> every frame summed over bins of bin_y x bin_x neighbouring
// pixels, out[f][Y][X] = sum of px[f][y][x] over Y * bin_y <= y < min((Y + 1) * bin_y, height), X * bin_x <= x < min((X + 1) * bin_x,
// width), without writing the decoded frames: previews, binned diffraction patterns, down-sampled movies.  One kernel; the front
// end is decode_bins.hip's (group_front.hpp, group_runs.hpp), the consumer is a 2-D tile of accumulators in LDS.
//
//   k_binned_bands  a workgroup per BAND: a range of whole output rows of one frame (binned_plan(): as many rows as kBinnedAccs
//                   accumulators hold, fewer where few frames would leave the GPU idle), and so the consecutive pixels [p_lo, p_hi)
//                   of the frame.  The workgroup keeps [rows][out_w] accumulators in dynamic LDS -- uint32 for pixel types of up
//                   to 16 bits (a bin has at most 64 x 64 pixels: 4096 * 65535 < 2^32; signed: two's complement), uint64 for
//                   32-bit types --, zeroed first.  Its four wavefronts take the 256-block groups p_lo / 3072 .. (p_hi - 1) / 3072
//                   in runs of up to kRun groups (a Run filled by hand: a band starts at any group).  A wavefront walks its run as
//                   bins_run does: widths -> header_len + 12 * w -> wave scans from the group's offset -> the group validated,
//                   unconditionally -> the CANDIDATE blocks, those with a width and a pixel inside the band, compacted into
//                   consecutive lanes through the list in LDS -> per 64 candidates one round: the payload dwords into registers,
//                   the register extraction, and binned_map.hpp: the block's pixels stepped through the bins, neighbours of one
//                   bin summed in registers, one LDS atomic add (ds_add_u32 / ds_add_u64) per change of bin, none for a zero sum
//                   or a pixel outside the band.  A group that two bands share is walked (and validated) by both; each adds only
//                   its own pixels, also inside a block that straddles the edge: plain ownership, no global atomics, no clearing
//                   launch, no partial sums.  Behind a barrier the workgroup converts its accumulators (put_sum.hpp, on the
//                   run-time output type) and stores its rows -- consecutive elements of the output -- with coalesced stores.  A
//                   group that fails validation sets CORRUPT and adds nothing.
// Integer arithmetic only; addition modulo 2^32 / 2^64 is associative and commutative, so the sums do not depend on the order in
// which the atomics arrive.  Global memory sees no atomic except the status word.  The output is bit-identical across runs, input
// forms and launch shapes.
#include <algorithm>
#include <type_traits>
#include "codec_common.hpp"
#include "decode_binned.hpp"
#include "group_front.hpp"
#include "group_runs.hpp"
#include "put_sum.hpp"

namespace trpx {

static_assert(kBinnedBlock == (uint32_t)kBlock && kBinnedRunGroups == kRun && kBinnedGroupValues == (uint32_t)kTileValues,
              "binned_map.hpp restates the codec's constants");

namespace {

template <typename T> using BinnedAcc = std::conditional_t<PixelTraits<T>::bits == 32, unsigned long long, uint32_t>;

// value i of an extracted block as the accumulator type (signed types: sign-extended)
template <typename T>
__device__ __forceinline__ BinnedAcc<T> binned_value(const uint32_t (&o)[PackedDwords<T>::n], int i) {
    if constexpr (PixelTraits<T>::is_signed) return (BinnedAcc<T>)(std::make_signed_t<BinnedAcc<T>>)packed_value<T>(o, i);
    else return (BinnedAcc<T>)packed_value<T>(o, i);
}
template <typename T>
__device__ __forceinline__ int64_t binned_sum(BinnedAcc<T> s) {
    if constexpr (PixelTraits<T>::bits == 32) return (int64_t)s;
    else if constexpr (PixelTraits<T>::is_signed) return (int64_t)(int32_t)s;
    else return (int64_t)s;
}

// the groups [g0, g0 + n) of `frame` (n <= kRun) on one wavefront, the pixels of the band d into acc
template <typename T>
__device__ __forceinline__ void binned_run(const BinnedArgs& a, uint64_t frame, uint32_t g0, uint32_t n, const BinnedBand& d,
                                           uint32_t* __restrict__ list, BinnedAcc<T>* __restrict__ acc) {
    const FrameGeom& g = a.geom;
    const uint32_t lane = (uint32_t)lane_id();
    Run R;                                                  // (run_place() starts runs at multiples of kRun: a band starts anywhere)
    R.frame = frame;
    R.g0 = g0;
    R.n = n;
    R.u0 = frame * g.n_tiles + g0;
    R.wf = a.widths + frame * g.n_blocks;
    run_load(R, a, lane);
    uint32_t wn[kGroupRows], nbn[kGroupRows], wp0n[kGroupRows];
    group_load_widths(wn, nbn, wp0n, R.wf, g, R.g0, lane);
    bool bad = false;
#pragma unroll 1
    for (uint32_t j = 0; j < R.n; ++j) {
        uint32_t w[kGroupRows], nb[kGroupRows], wp0[kGroupRows], off[kGroupRows];
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) { w[r] = wn[r]; nb[r] = nbn[r]; wp0[r] = wp0n[r]; }
        if (j + 1 < R.n) group_load_widths(wn, nbn, wp0n, R.wf, g, R.g0 + j + 1, lane);   // in flight during this group
        const uint64_t t_off = lane_value64(R.my_off, j), t_next = lane_value64(R.my_off, j + 1);
        if (!group_offsets<T>(off, w, nb, wp0, R.fo, R.fe, t_off, t_next, R.g0 + j + 1 == g.n_tiles, a.terse_bytes, lane)) {
            bad = true;                                     // (validated whether or not a block of it is wanted)
            continue;
        }
        const GroupStream gs = group_stream(a.terse, a.terse_bytes, R.fo, t_off);
        // ---- the candidates, in block order, into consecutive entries: a width, and a pixel inside the band
        uint32_t n_cand = 0;
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) {
            const uint32_t first = ((R.g0 + j) * kTileBlocks + r * kWave + lane) * kBlock;
            const bool want = nb[r] != 0u && w[r] != 0u && first < d.p_hi && first + nb[r] > d.p_lo;
            const uint64_t ballot = __ballot(want);
            if (want) list[n_cand + lanes_below(ballot)] = list_entry(off[r], w[r], r * kWave + lane);
            n_cand += (uint32_t)__builtin_popcountll(ballot);
        }
        list_sync();
#pragma unroll 1
        for (uint32_t c = 0; c * kWave < n_cand; ++c) {
            const bool have = c * kWave + lane < n_cand;
            const uint32_t e = have ? list[c * kWave + lane] : 0u;
            const uint32_t block = (R.g0 + j) * kTileBlocks + (e >> 23);
            const uint32_t left = (uint32_t)g.n_values - block * kBlock;   // (listed blocks lie inside the frame: < 2^29 values)
            const uint32_t nr = have ? (left < (uint32_t)kBlock ? left : (uint32_t)kBlock) : 0u;
            uint32_t o[PackedDwords<T>::n];
            group_extract<T>(o, gs, have, (e >> 17) & 63u, nr, e & 0x1FFFFu);
            if (nr != 0u)
                binned_map<BinnedAcc<T>>(block * kBlock, nr, [&](int i) { return binned_value<T>(o, i); }, a.geo, d,
                                         [&](uint32_t idx, BinnedAcc<T> s) { atomicAdd(&acc[idx], s); });
        }
        list_sync();                                        // (the next group rewrites the list)
    }
    if (bad && lane == 0) atomicMax(&a.status[0], kStatusCorrupt);
}

}  // namespace

// a unit = (frame, band)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_binned_bands(BinnedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_binned[];   // [plan.rows][out_w] of BinnedAcc<T>
    __shared__ uint32_t s_list[kWavesPerWg * kTileBlocks];
    BinnedAcc<T>* const acc = reinterpret_cast<BinnedAcc<T>*>(s_binned);
    const uint64_t units = a.n_frames * a.plan.bands;
    const uint32_t wave = (uint32_t)wave_id();
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {        // (uniform: every barrier below is reached by all)
        const uint64_t frame = unit / a.plan.bands;
        const BinnedBand d = binned_band(a.geo, a.plan, (uint32_t)(unit - frame * a.plan.bands));
        const uint32_t n_acc = d.rows * a.geo.out_w;        // (<= plan.rows * out_w: what the launch sized the LDS for)
        for (uint32_t i = threadIdx.x; i < n_acc; i += kThreads) acc[i] = 0;
        __syncthreads();
        // the band's groups, in runs of equal length over the four wavefronts
        const uint32_t g_lo = d.p_lo / (uint32_t)kTileValues, g_hi = (d.p_hi - 1u) / (uint32_t)kTileValues;
        const uint32_t groups = g_hi - g_lo + 1u;
        const uint32_t per = std::min<uint32_t>(kRun, (groups + kWavesPerWg - 1) / kWavesPerWg);
        for (uint32_t g0 = g_lo + wave * per; g0 <= g_hi; g0 += kWavesPerWg * per)
            binned_run<T>(a, frame, g0, std::min<uint32_t>(per, g_hi - g0 + 1u), d, s_list + wave * kTileBlocks, acc);
        __syncthreads();
        const uint64_t base = (frame * a.geo.out_h + d.row0) * a.geo.out_w;
        for (uint32_t i = threadIdx.x; i < n_acc; i += kThreads) put_sum(a.out, base + i, a.out_code, binned_sum<T>(acc[i]));
        __syncthreads();                                    // (the next unit zeroes the accumulators)
    }
}

hipError_t launch_decode_binned(int dtype, const BinnedArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    // the launch shape from the geometry alone: a workgroup per (frame, band) up to 2^20 workgroups, strided units beyond;
    // plan.rows * out_w accumulators of dynamic LDS
    const uint64_t units = a.n_frames * a.plan.bands;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(units, 1u << 20);
    return for_pixel_type(dtype, [&]<class T>() {
        const size_t lds = sizeof(BinnedAcc<T>) * (size_t)a.plan.rows * a.geo.out_w;
        if (lds > 48u * 1024u) {                            // (a widest row of 64-bit sums: 64 KB beside the lists)
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_binned_bands<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((k_binned_bands<T>), dim3(grid), dim3(kThreads), lds, st, a);
        return hipGetLastError();                           // (one check behind the clear and the launch, as the siblings do: the first error stays)
    });
}

}  // namespace trpx
