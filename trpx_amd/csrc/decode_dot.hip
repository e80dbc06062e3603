// Weighted per-frame sums (trpx_decode_dot): a stack with its decode index and K maps of int32 weights ->
// dots[f][k] = sum_p px[f][p] * weights[k][p] in int64 (mod 2^64), without expanding the frames.  The shape is
// support -> runs -> reduce; the front end is decode_sparse.hip's (group_front.hpp, group_runs.hpp).
//
//   k_dot_support   one bit per block of a frame: some map is non-zero on some pixel of the block.  In every call: the maps are
//                   device data that a graph replay may have changed.
//   k_dot_runs      a wavefront per run of kRun consecutive groups of one frame: widths -> header_len + 12 * w -> wave scans from
//                   the group's offset -> the group validated, unconditionally (so the whole stack is) -> the CANDIDATE blocks,
//                   those with a width and their support bit, compacted into consecutive lanes through the list in LDS -> per 64
//                   candidates one round: the payload dwords straight from the stream into registers, the register extraction,
//                   per map the block's 12 weights (byte 48 * block of the map) and 12 multiply-adds into the lane's int64
//                   accumulator of that map.  At the run's end the accumulators are summed over the wavefront and leave in one
//                   plain store: partials[run][map].  A group that fails validation sets CORRUPT and adds nothing.
//   k_dot_reduce    per (frame, map): the frame's runs' partial sums, added in run order -> dots_out.  Every element is written.
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
    const FrameGeom& g = a.geom;
    const uint32_t lane = (uint32_t)lane_id();
    Run R = run_place(a, run, runs_per_frame);
    run_load(R, a, lane);
    uint32_t wn[kGroupRows], nbn[kGroupRows], wp0n[kGroupRows], sn[kGroupRows];
    group_load_widths(wn, nbn, wp0n, R.wf, g, R.g0, lane);
    group_load_support(sn, a.support, n_words, R.g0, lane);
    uint64_t acc[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) acc[k] = 0ull;
    bool bad = false;
#pragma unroll 1
    for (uint32_t j = 0; j < R.n; ++j) {
        uint32_t w[kGroupRows], nb[kGroupRows], wp0[kGroupRows], sup[kGroupRows], off[kGroupRows];
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) { w[r] = wn[r]; nb[r] = nbn[r]; wp0[r] = wp0n[r]; sup[r] = sn[r]; }
        if (j + 1 < R.n) {                                  // in flight during this group
            group_load_widths(wn, nbn, wp0n, R.wf, g, R.g0 + j + 1, lane);
            group_load_support(sn, a.support, n_words, R.g0 + j + 1, lane);
        }
        const uint64_t t_off = lane_value64(R.my_off, j), t_next = lane_value64(R.my_off, j + 1);
        if (!group_offsets<T>(off, w, nb, wp0, R.fo, R.fe, t_off, t_next, R.g0 + j + 1 == g.n_tiles, a.terse_bytes, lane)) {
            bad = true;                                     // (validated whether or not a block of it is wanted)
            continue;
        }
        const GroupStream gs = group_stream(a.terse, a.terse_bytes, R.fo, t_off);
        // ---- the candidates, in block order, into consecutive entries
        uint32_t n_cand = 0;
#pragma unroll
        for (int r = 0; r < kGroupRows; ++r) {
            const bool want = nb[r] != 0u && w[r] != 0u && ((sup[r] >> (lane & 31u)) & 1u);
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
            dot_accumulate<T, KM>(acc, o, a.weights, a.n_maps, g.n_values, block, nr, whole16);
        }
        list_sync();                                        // (the next group rewrites the list)
    }
    if (bad && lane == 0) atomicMax(&a.status[0], kStatusCorrupt);
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
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t n_words = (uint32_t)dot_support_words(g);
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t b0 = (uint64_t)blockIdx.x * kThreads + (uint32_t)wave_id() * kWave; b0 < g.n_blocks; b0 += stride) {   // (b0: uniform)
        const uint64_t b = b0 + lane;
        uint32_t any = 0;
        if (b < g.n_blocks) {
            const uint64_t first = b * kBlock;
            const uint32_t nb = first + kBlock <= g.n_values ? (uint32_t)kBlock : (uint32_t)(g.n_values - first);
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
        }
        const uint64_t ballot = __ballot(any != 0u);
        const uint32_t word = (uint32_t)(b0 >> 5);
        if (lane == 0 && word < n_words) support[word] = (uint32_t)ballot;
        if (lane == 32 && word + 1 < n_words) support[word + 1] = (uint32_t)(ballot >> 32);
    }
}

template <typename T, int KM>
__global__ __launch_bounds__(kThreads) void k_dot_runs(DotArgs a, uint32_t runs_per_frame, bool whole16) {
    __shared__ uint32_t s_list[kWavesPerWg * kTileBlocks];
    const uint64_t runs = a.n_frames * runs_per_frame;
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerWg;
    const uint32_t n_words = (uint32_t)dot_support_words(a.geom);
    for (uint64_t run = (uint64_t)blockIdx.x * kWavesPerWg + (uint32_t)wave_id(); run < runs; run += stride)
        dot_run<T, KM>(a, run, runs_per_frame, n_words, whole16, s_list + wave_id() * kTileBlocks);
}

// per (frame, map): the runs' partial sums in run order
__global__ __launch_bounds__(kThreads) void k_dot_reduce(const int64_t* __restrict__ partials, uint64_t n_frames, uint32_t runs_per_frame,
                                                         uint32_t n_maps, int64_t* __restrict__ dots_out) {
    const uint64_t n = n_frames * n_maps;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t frame = i / n_maps;
        const uint32_t k = (uint32_t)(i - frame * n_maps);
        uint64_t s = 0;
        for (uint32_t r = 0; r < runs_per_frame; ++r) s += (uint64_t)partials[(frame * runs_per_frame + r) * n_maps + k];
        dots_out[i] = (int64_t)s;
    }
}

uint32_t dot_runs_per_frame(const FrameGeom& g) { return (g.n_tiles + kRun - 1) / kRun; }

hipError_t launch_decode_dot(int dtype, const DotArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    // launch shapes from the geometry and the number of maps alone: a wavefront per run of kRun groups up to 4096 workgroups,
    // strided runs beyond; the accumulators of up to 4 maps or of all 16 in registers
    const uint32_t rpf = dot_runs_per_frame(a.geom);
    const uint64_t wgs = (a.n_frames * rpf + kWavesPerWg - 1) / kWavesPerWg;
    const uint32_t grid = (uint32_t)(wgs < 4096 ? wgs : 4096);
    const uint64_t swgs = ((uint64_t)a.geom.n_blocks + kThreads - 1) / kThreads;
    const uint32_t sgrid = (uint32_t)(swgs < 4096 ? swgs : 4096);
    const uint64_t rwgs = (a.n_frames * a.n_maps + kThreads - 1) / kThreads;
    const uint32_t rgrid = (uint32_t)(rwgs < 4096 ? rwgs : 4096);
    const bool whole16 = (uintptr_t)a.weights % 16 == 0 && a.geom.n_values % 4 == 0;
    return for_pixel_type(dtype, [&]<class T>() {
        hipLaunchKernelGGL(k_dot_support, dim3(sgrid), dim3(kThreads), 0, st, a.weights, a.n_maps, a.geom, whole16, a.support);
        if (a.n_maps <= 4) hipLaunchKernelGGL((k_dot_runs<T, 4>), dim3(grid), dim3(kThreads), 0, st, a, rpf, whole16);
        else hipLaunchKernelGGL((k_dot_runs<T, (int)kDotMaxMaps>), dim3(grid), dim3(kThreads), 0, st, a, rpf, whole16);
        hipLaunchKernelGGL(k_dot_reduce, dim3(rgrid), dim3(kThreads), 0, st, a.partials, a.n_frames, rpf, a.n_maps, a.dots_out);
        return hipGetLastError();                           // (one check behind the clear and the three launches, as the siblings do: the first error stays)
    });
}

}  // namespace trpx
