// Weighted per-frame sums (trpx_decode_dot): a stack with its decode index and K maps of int32 weights ->
// dots[f][k] = sum_p px[f][p] * weights[k][p] in int64 (mod 2^64), without expanding the frames.  The shape is
// support -> runs -> reduce; the walk of a run is group_runs.hpp's (run_walk).
//
//   k_dot_support   one bit per block of a frame: some map is non-zero on some pixel of the block.  In every call: the maps are
//                   device data that a graph replay may have changed.
//   k_dot_runs      a wavefront per run of kRun consecutive groups of one frame.  The CANDIDATE blocks are those with a width and
//                   their support bit; per extracted block and map: the block's 12 weights (byte 48 * block of the map) and 12
//                   multiply-adds into the lane's int64 accumulator of that map.  At the run's end the accumulators are summed
//                   over the wavefront and leave in one plain store: partials[run][map].  A group that fails validation sets
//                   CORRUPT and adds nothing.
//   k_reduce_parts  (group_runs.hpp) per (frame, map): the frame's runs' partial sums, added in run order -> dots_out.  Every
//                   element is written.
// Integer arithmetic only; the sums wrap mod 2^64 and no addition depends on the order in which wavefronts run: the output is
// bit-identical across runs, input forms and launch shapes.  Nothing is added into memory that another wavefront adds into.
#include "codec_common.hpp"
#include "decode_dot.hpp"
#include "group_front.hpp"
#include "group_runs.hpp"

namespace trpx {

namespace {

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {  // every lane gets the sum of the 64 lanes' values (mod 2^64)
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, kWave);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, kWave);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// value * weight, exact in int64 for every pixel type (|value| < 2^32, |weight| <= 2^31), as the bits of the sum it joins
template <typename T>
__device__ __forceinline__ uint64_t dot_product(T v, int32_t wt) { return (uint64_t)((int64_t)v * (int64_t)wt); }

// One extracted block (o: its nr values, nr == 0: none) against every map: acc[k] += sum_i value[i] * weights[k][12 * block + i].
// whole16: the maps are 16-byte aligned with n_values % 4 == 0 -- a whole block's weights are three 16-byte loads, twelve dword
// loads otherwise.  The weights behind a frame's last value are never read.
template <typename T, int KM>
__device__ __forceinline__ void dot_accumulate(uint64_t (&acc)[KM], const uint32_t (&o)[PackedDwords<T>::n], const int32_t* __restrict__ weights,
                                               uint32_t n_maps, uint64_t n_values, uint32_t block, uint32_t nr, bool whole16) {
    const int32_t* __restrict__ m0 = weights + (uint64_t)block * kBlock;
    if (nr == (uint32_t)kBlock) {                           // a whole block: its 12 weights lie inside the map
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if ((uint32_t)k < n_maps) {                     // (uniform)
                const int32_t* __restrict__ m = m0 + (uint64_t)k * n_values;
                int32_t wt[kBlock];
                if (whole16) {                              // (uniform)
                    const int4* __restrict__ q = reinterpret_cast<const int4*>(m);
                    const int4 x0 = q[0], x1 = q[1], x2 = q[2];
                    wt[0] = x0.x; wt[1] = x0.y; wt[2] = x0.z; wt[3] = x0.w; wt[4] = x1.x; wt[5] = x1.y; wt[6] = x1.z; wt[7] = x1.w;
                    wt[8] = x2.x; wt[9] = x2.y; wt[10] = x2.z; wt[11] = x2.w;
                } else {                                    // maps of another alignment (an odd frame size): twelve dword loads
#pragma unroll
                    for (int i = 0; i < kBlock; ++i) wt[i] = m[i];
                }
                uint64_t s = acc[k];
#pragma unroll
                for (int i = 0; i < kBlock; ++i) s += dot_product<T>(packed_value<T>(o, i), wt[i]);
                acc[k] = s;
            }
        }
    } else if (nr != 0u) {                                  // a frame's partial last block: value by value, nothing behind n_values read
#pragma unroll 1
        for (uint32_t k = 0; k < n_maps; ++k) {
            const int32_t* __restrict__ m = m0 + (uint64_t)k * n_values;
            uint64_t s = 0;
#pragma unroll
            for (int i = 0; i < kBlock; ++i) {
                const int32_t wt = (uint32_t)i < nr ? m[i] : 0;
                s += (uint32_t)i < nr ? dot_product<T>(packed_value<T>(o, i), wt) : 0ull;
            }
#pragma unroll
            for (int kk = 0; kk < KM; ++kk) acc[kk] += (uint32_t)kk == k ? s : 0ull;   // (the accumulators stay in registers)
        }
    }
}

template <typename T, int KM>
__device__ __forceinline__ void dot_run(const DotArgs& a, uint64_t run, uint32_t runs_per_frame, uint32_t n_words, bool whole16,
                                        uint32_t* __restrict__ list) {
    const uint32_t lane = (uint32_t)lane_id();
    uint64_t acc[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) acc[k] = 0ull;
    run_walk<T>(a, run_place(a, run, runs_per_frame), SupportWords{a.support, n_words}, a.status, list,
                [](uint32_t, uint32_t w, uint32_t) { return w != 0u; },
                [&](uint32_t, uint32_t block, uint32_t nr, const uint32_t (&o)[PackedDwords<T>::n], bool) {
                    // (a lane without a block skips, as the sibling consumers' bodies do: written without the test, the 16-map
                    // kernel of 8-bit pixels needs 131 VGPRs instead of 113 and loses its fourth wave per SIMD)
                    if (nr != 0u) dot_accumulate<T, KM>(acc, o, a.weights, a.n_maps, a.geom.n_values, block, nr, whole16);
                });
    uint64_t mine = 0;                                      // lane k: the run's sum for map k
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        if ((uint32_t)k < a.n_maps) {
            const uint64_t total = wave_sum64(acc[k]);
            if (lane == (uint32_t)k) mine = total;
        }
    }
    if (lane < a.n_maps) a.partials[run * a.n_maps + lane] = (int64_t)mine;
}

}  // namespace

// bit b of the support words: some map is non-zero on block b (pixels 12 b .. 12 b + 11 of a frame, as far as the frame goes)
__global__ __launch_bounds__(kThreads) void k_dot_support(const int32_t* __restrict__ weights, uint32_t n_maps, FrameGeom g, bool whole16,
                                                          uint32_t* __restrict__ support) {
    support_write(support, g, [&](uint64_t first, uint32_t nb) {
        uint32_t any = 0;
        for (uint32_t k = 0; k < n_maps; ++k) {
            const int32_t* __restrict__ m = weights + (uint64_t)k * g.n_values + first;
            if (whole16 && nb == (uint32_t)kBlock) {
                const int4* __restrict__ q = reinterpret_cast<const int4*>(m);
                const int4 x0 = q[0], x1 = q[1], x2 = q[2];
                any |= (uint32_t)(x0.x | x0.y | x0.z | x0.w | x1.x | x1.y | x1.z | x1.w | x2.x | x2.y | x2.z | x2.w);
            } else {
                for (uint32_t i = 0; i < nb; ++i) any |= (uint32_t)m[i];
            }
        }
        return any != 0u;
    });
}

template <typename T, int KM>
__global__ __launch_bounds__(kThreads) void k_dot_runs(DotArgs a, uint32_t runs_per_frame, bool whole16) {
    const uint32_t n_words = (uint32_t)support_words(a.geom);
    for_each_run(a.n_frames * runs_per_frame,
                 [&](uint64_t run, uint32_t* __restrict__ list) { dot_run<T, KM>(a, run, runs_per_frame, n_words, whole16, list); });
}

hipError_t launch_decode_dot(int dtype, const DotArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    // launch shapes from the geometry and the number of maps alone: a wavefront per run of kRun groups up to 4096 workgroups,
    // strided runs beyond; the accumulators of up to 4 maps or of all 16 in registers
    const uint32_t rpf = runs_per_frame(a.geom);
    const uint32_t grid = grid_capped(a.n_frames * rpf, kWavesPerWg);
    const uint32_t sgrid = grid_capped(a.geom.n_blocks, kThreads);
    const uint32_t rgrid = grid_capped(a.n_frames * a.n_maps, kThreads);
    const bool whole16 = (uintptr_t)a.weights % 16 == 0 && a.geom.n_values % 4 == 0;
    return for_pixel_type(dtype, [&]<class T>() {
        hipLaunchKernelGGL(k_dot_support, dim3(sgrid), dim3(kThreads), 0, st, a.weights, a.n_maps, a.geom, whole16, a.support);
        if (a.n_maps <= 4) hipLaunchKernelGGL((k_dot_runs<T, 4>), dim3(grid), dim3(kThreads), 0, st, a, rpf, whole16);
        else hipLaunchKernelGGL((k_dot_runs<T, (int)kDotMaxMaps>), dim3(grid), dim3(kThreads), 0, st, a, rpf, whole16);
        hipLaunchKernelGGL(k_reduce_parts<0>, dim3(rgrid), dim3(kThreads), 0, st, a.partials, a.n_frames, rpf, a.n_maps, a.dots_out);
        return hipGetLastError();                           // (one check behind the clear and the three launches, as the siblings do: the first error stays)
    });
}

}  // namespace trpx
