// Reducing decode (trpx_decode_reduce): a stack with its decode index -> per pixel, the max, the min, the sum of squares or the
// count of frames at or above a threshold over `group` consecutive frames, without writing the decoded frames.  k_sum_tiles'
// structure (decode_sum.hip) with another accumulate step: the work unit is (output j, tile t, frame chunk c), one 256-thread
// workgroup walks the frames of its chunk through sum_tile.hpp's three-frame pipeline and keeps 12 * kSumSubTiles accumulators per
// lane in registers (reduce_ops.hpp: 32 bits for MAX / MIN / COUNT_GE, 64 for SUMSQ); they leave once, through LDS, as whole lines.
//   chunks      sum_plan's rule.  With more than one chunk each writes its raw accumulators to a partial slab in the workspace and
//               k_reduce_merge merges the chunks with the op's merge, in chunk order, and converts.  A chunk without frames (a
//               short last group) leaves the op's identity.  Integer arithmetic, no atomics on the output: the result does not
//               depend on the split.
// HBM traffic: stream + widths (+ group offsets) read once, n_out * n_values elements written (+ 2 x the partial slab when split).
#include "codec_common.hpp"
#include "decode_reduce.hpp"
#include "reduce_ops.hpp"
#include "sum_tile.hpp"

namespace trpx {

template <typename T, int op>
__global__ __launch_bounds__(kThreads) void k_reduce_tiles(ReduceArgs a) {
    using Op = ReduceOp<T, op>;
    using Acc = typename Op::Acc;
    using Out = typename Op::Out;
    constexpr int kSub = sum_sub_tiles<T>();
    static_assert(4 * kWave * kBlock * sizeof(Acc) <= 4 * sum_stage_dwords<T>(), "the waves' rows fit the image");
    __shared__ __attribute__((aligned(16))) uint32_t s_image[sum_stage_dwords<T>()];
    __shared__ uint32_t s_wtot[kSub * 4];
    if (a.status[0] != 0) return;                           // corrupt chain (the walk or the locator said so): produce nothing
    const FrameGeom g = a.geom;
    const int64_t threshold = a.threshold;
    const uint64_t units = (uint64_t)a.n_out * a.chunks * a.tpf;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t t = (uint32_t)(unit % a.tpf);        // adjacent workgroups: adjacent tiles of one output
        const uint64_t rest = unit / a.tpf;
        const uint32_t ch = (uint32_t)(rest % a.chunks);
        const uint64_t j = rest / a.chunks;
        const uint64_t g0 = j * a.group;
        const uint64_t g1 = g0 + a.group < a.n_frames ? g0 + a.group : a.n_frames;
        const uint64_t f0 = g0 + (uint64_t)ch * a.fpc;      // (past g1 for the empty chunks of a short last group: the identity)
        const uint64_t f1 = f0 + a.fpc < g1 ? f0 + a.fpc : g1;

        Acc acc[kSub][kBlock];
#pragma unroll
        for (int r = 0; r < kSub; ++r)
#pragma unroll
            for (int k = 0; k < kBlock; ++k) acc[r][k] = Op::identity();
        bool bad = false, ok = true;
        uint4 R[sum_prefetch_loads<T>()];
        SumPre<T> pn;
        SumCur<T> cur;
        if (f0 < f1) {
            sum_load_pre(pn, a.frame_offsets, g, f0, t, a.widths, a.tile_off);
            bad = !sum_scan(cur, pn, g, t, a.terse_bytes, s_wtot);
            if (!bad) sum_fetch<T>(R, cur, a.terse, a.terse_bytes);
            if (f0 + 1 < f1) sum_load_pre(pn, a.frame_offsets, g, f0 + 1, t, a.widths, a.tile_off);
        }
        for (uint64_t f = f0; f < f1 && !bad; ++f) {
            __syncthreads();                                // (the previous frame's extraction is done with the image)
            sum_stage<T>(s_image, R, cur.n_dw);
            __syncthreads();
            SumCur<T> nxt;
            if (f + 1 < f1) {                               // frame f + 1: scan, then its stream is in flight during f's extraction
                bad = !sum_scan(nxt, pn, g, t, a.terse_bytes, s_wtot);
                if (!bad) sum_fetch<T>(R, nxt, a.terse, a.terse_bytes);
                if (f + 2 < f1) sum_load_pre(pn, a.frame_offsets, g, f + 2, t, a.widths, a.tile_off);
            }
#pragma unroll
            for (int r = 0; r < kSub; ++r) {
                uint32_t u[kBlock];
                sum_fields<T>(u, ok, cur, r, s_image);
#pragma unroll
                for (int k = 0; k < kBlock; ++k) acc[r][k] = Op::step(acc[r][k], u[k], threshold);
            }
            cur = nxt;
        }
        if (!ok) atomicMax(&a.status[0], kStatusCorrupt);
        if (bad && threadIdx.x == 0) atomicMax(&a.status[0], kStatusCorrupt);

        // ---- the results leave once: per wavefront, its 64 blocks (768 values) as accumulators through LDS, then consecutive
        // elements per lane (every store instruction writes whole lines)
        const int lane = lane_id(), wave = wave_id();
        Acc* const row = reinterpret_cast<Acc*>(s_image) + wave * (kWave * kBlock);
        const bool part = a.partial != nullptr;
        const uint64_t base = part ? ((uint64_t)ch * a.n_out + j) * g.n_values : j * g.n_values;
#pragma unroll
        for (int r = 0; r < kSub; ++r) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kBlock; ++k) row[lane * kBlock + k] = acc[r][k];
            __syncthreads();
            const uint64_t first = ((uint64_t)t * kSub * kThreads + (uint64_t)r * kThreads + (uint64_t)wave * kWave) * kBlock;
            if (first < g.n_values) {
                const uint32_t n_valid = g.n_values - first < (uint64_t)(kWave * kBlock) ? (uint32_t)(g.n_values - first) : kWave * kBlock;
                if (part)
                    for (uint32_t e = lane; e < n_valid; e += kWave) static_cast<Acc*>(a.partial)[base + first + e] = row[e];
                else
                    for (uint32_t e = lane; e < n_valid; e += kWave) static_cast<Out*>(a.out)[base + first + e] = Op::convert(row[e]);
            }
        }
        __syncthreads();                                    // (the next unit's first frame reuses the image)
    }
}

// partial slabs [chunks][n_out * n_values] -> the results, merged in chunk order and converted
template <typename T, int op>
__global__ __launch_bounds__(kThreads) void k_reduce_merge(const void* __restrict__ partial, uint32_t chunks, uint64_t n_elems,
                                                            void* __restrict__ out) {
    using Op = ReduceOp<T, op>;
    using Acc = typename Op::Acc;
    const Acc* __restrict__ p = static_cast<const Acc*>(partial);
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_elems; i += (uint64_t)gridDim.x * kThreads) {
        Acc s = Op::identity();
        for (uint32_t c = 0; c < chunks; ++c) s = Op::merge(s, p[(uint64_t)c * n_elems + i]);
        static_cast<typename Op::Out*>(out)[i] = Op::convert(s);
    }
}

template <typename T, int op>
static hipError_t launch_reduce_t(const ReduceArgs& a, hipStream_t st) {
    const uint64_t units = (uint64_t)a.n_out * a.chunks * a.tpf;
    hipLaunchKernelGGL((k_reduce_tiles<T, op>), dim3(grid_capped(units, 1, 1u << 22)), dim3(kThreads), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.partial) return e;
    const uint64_t n = a.n_out * a.geom.n_values;
    hipLaunchKernelGGL((k_reduce_merge<T, op>), dim3(grid_capped(n, kThreads, 8192)), dim3(kThreads), 0, st, a.partial, a.chunks, n, a.out);
    return hipGetLastError();
}

hipError_t launch_decode_reduce(int dtype, int op, const ReduceArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    return for_pixel_type(dtype, [&]<class T>() {
        switch (op) {
        case kReduceMax: return launch_reduce_t<T, kReduceMax>(a, st);
        case kReduceMin: return launch_reduce_t<T, kReduceMin>(a, st);
        case kReduceSumSq: return launch_reduce_t<T, kReduceSumSq>(a, st);
        case kReduceCountGe: return launch_reduce_t<T, kReduceCountGe>(a, st);
        }
        return hipErrorInvalidValue;
    });
}

}  // namespace trpx
