// Binned decode (trpx_decode_binned): a stack with its decode index -> every frame summed over bins of bin_y x bin_x neighbouring
// pixels, out[f][Y][X] = sum of px[f][y][x] over Y * bin_y <= y < min((Y + 1) * bin_y, height), X * bin_x <= x < min((X + 1) * bin_x,
// width), without writing the decoded frames: previews, binned diffraction patterns, down-sampled movies.  One kernel; the walk
// of a run is group_runs.hpp's (run_walk), the consumer is a 2-D tile of accumulators in LDS.
//
//   k_binned_bands  a workgroup per BAND: a range of whole output rows of one frame (binned_plan(): as many rows as kBinnedAccs
//                   accumulators hold, fewer where few frames would leave the GPU idle), and so the consecutive pixels [p_lo, p_hi)
//                   of the frame.  The workgroup keeps [rows][out_w] accumulators in dynamic LDS -- uint32 for pixel types of up
//                   to 16 bits (a bin has at most 64 x 64 pixels: 4096 * 65535 < 2^32; signed: two's complement), uint64 for
//                   32-bit types --, zeroed first.  Its four wavefronts take the 256-block groups p_lo / 3072 .. (p_hi - 1) / 3072
//                   in runs of up to kRun groups (run_at: a band starts at any group).  The CANDIDATE blocks are those with a
//                   width and a pixel inside the band; per extracted block binned_map.hpp: the block's pixels stepped through
//                   the bins, neighbours of one bin summed in registers, one LDS atomic add (ds_add_u32 / ds_add_u64) per change
//                   of bin, none for a zero sum or a pixel outside the band.  A group that two bands share is walked (and
//                   validated) by both; each adds only its own pixels, also inside a block that straddles the edge: plain
//                   ownership, no global atomics, no clearing launch, no partial sums.  Behind a barrier the workgroup converts
//                   its accumulators (put_sum.hpp, on the run-time output type) and stores its rows -- consecutive elements of
//                   the output -- with coalesced stores.  A group that fails validation sets CORRUPT and adds nothing.
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
    run_walk<T>(a, run_at(a, frame, g0, n), NoSupport{}, a.status, list,
                [&](uint32_t block, uint32_t w, uint32_t nb) {
                    const uint32_t first = block * kBlock;
                    return w != 0u && first < d.p_hi && first + nb > d.p_lo;
                },
                [&](uint32_t, uint32_t block, uint32_t nr, const uint32_t (&o)[PackedDwords<T>::n], bool) {
                    if (nr != 0u)
                        binned_map<BinnedAcc<T>>(block * kBlock, nr, [&](int i) { return binned_value<T>(o, i); }, a.geo, d,
                                                 [&](uint32_t idx, BinnedAcc<T> s) { atomicAdd(&acc[idx], s); });
                });
}

}  // namespace

// a unit = (frame, band)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_binned_bands(BinnedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_binned[];   // [plan.rows][out_w] of BinnedAcc<T>
    uint32_t* const list = wave_list();
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
            binned_run<T>(a, frame, g0, std::min<uint32_t>(per, g_hi - g0 + 1u), d, list, acc);
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
    const uint32_t grid = grid_capped(a.n_frames * a.plan.bands, 1, 1u << 20);
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
