// Summing decode (trpx_decode_sum): a stack with its decode index -> sums of `group` consecutive frames, without writing the
// decoded frames.  The work unit is (output j, tile t, frame chunk c): one 256-thread workgroup walks the frames of its chunk
// through the tile geometry of k_unpack_tiles (unpack_tile.hpp) and keeps the sums of its 12 * kSub values per lane in
// registers; only the sums leave the workgroup, once, through LDS as whole lines.
//
//   per frame   widths -> lengths -> wave/LDS scan -> the tile's stream dwords (registers -> LDS) -> width-specialised
//               extraction (UnpackDispatch) -> register accumulators.  Software-pipelined: while frame f is extracted from
//               LDS, the stream dwords of frame f + 1 are in flight to registers and the widths of frame f + 2 are loaded.
//   accumulate  u32 for 8/16-bit streams (two's complement: exact for up to 65 535 frames per chunk, signed included),
//               u64 for 32-bit streams.
//   chunks      few outputs (group = n_frames) leave the GPU idle: each group's frames are split over `chunks` chunks so that
//               about kSumTargetUnits workgroups run; each chunk writes its raw accumulators to a partial slab in the
//               workspace and k_sum_reduce adds the chunks in a fixed order and converts.  Integer sums: the result does not
//               depend on the split.
// HBM traffic: stream + widths (+ group offsets) read once, n_out * n_values sums written (+ 2 x the partial slab when split).
#include "codec_common.hpp"
#include "decode_sum.hpp"
#include "put_sum.hpp"
#include "sum_tile.hpp"
#include <type_traits>

namespace trpx {

namespace {

template <typename T> using SumAcc = std::conditional_t<PixelTraits<T>::bits == 32, uint64_t, uint32_t>;

template <typename T>
__device__ __forceinline__ int64_t acc_value(SumAcc<T> a) {
    if constexpr (PixelTraits<T>::bits == 32) return (int64_t)a;
    else if constexpr (PixelTraits<T>::is_signed) return (int64_t)(int32_t)a;
    else return (int64_t)a;
}

// (the walk's pieces -- load, scan, fetch, stage: sum_tile.hpp, shared with decode_reduce.hip)
// The frame's fields from the LDS image, added to the lane's accumulators.  Returns false for a width above the type's.
// (sum_tile.hpp's sum_fields is this text as a function; called here it changes how k_sum_tiles' checks are scheduled, so the
// kernel keeps the text it was measured with)
template <typename T>
__device__ __forceinline__ bool sum_extract(SumAcc<T> (&acc)[sum_sub_tiles<T>()][kBlock], const SumCur<T>& c,
                                            const uint32_t* __restrict__ s_image) {
    bool ok = true;
#pragma unroll
    for (int r = 0; r < sum_sub_tiles<T>(); ++r) {
        const uint32_t q = c.img_bit0 + c.off[r] + c.hl[r];  // first payload bit in the image
        uint32_t u[kBlock];
        if (c.nb[r] && tile_too_wide<T>(c.w[r])) ok = false;
        // (as unpack_tile: the "same width" bit stands exactly where header_len counted one bit, or the widths are not this
        // stream's layout -- a restated width, codec_common.hpp)
        if (c.nb[r] && ((s_image[(q - c.hl[r]) >> 5] >> ((q - c.hl[r]) & 31u)) & 1u) != (c.hl[r] == 1u ? 1u : 0u)) ok = false;
        tile_extract_full<T>(u, s_image, q, c.w[r], c.nb[r]);
        if (c.nb[r] && c.nb[r] < kBlock) {              // the frame's last, partial block (unrolled: u stays in registers)
            const uint32_t ww = tile_partial_width<T>(c.w[r]), mask = field_mask(ww);
            uint32_t p = q;
#pragma unroll
            for (int k = 0; k < kBlock; ++k) {
                if (k < c.nb[r] && ww) {
                    u[k] = tile_partial_field<T>(s_image, p, ww, mask);
                    p += ww;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            if constexpr (PixelTraits<T>::bits == 32)
                acc[r][k] += PixelTraits<T>::is_signed ? (uint64_t)(int64_t)(int32_t)u[k] : (uint64_t)u[k];
            else acc[r][k] += u[k];                         // (sign-extended to 32 bits: two's complement sums)
        }
    }
    return ok;
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kThreads) void k_sum_tiles(SumArgs a) {
    constexpr int kSub = sum_sub_tiles<T>();
    __shared__ __attribute__((aligned(16))) uint32_t s_image[sum_stage_dwords<T>()];
    __shared__ uint32_t s_wtot[kSub * 4];
    if (a.status[0] != 0) return;                           // corrupt chain (the walk or the locator said so): produce nothing
    const FrameGeom g = a.geom;
    const uint64_t units = (uint64_t)a.n_out * a.chunks * a.tpf;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t t = (uint32_t)(unit % a.tpf);        // adjacent workgroups: adjacent tiles of one output
        const uint64_t rest = unit / a.tpf;
        const uint32_t ch = (uint32_t)(rest % a.chunks);
        const uint64_t j = rest / a.chunks;
        const uint64_t g0 = j * a.group;
        const uint64_t g1 = g0 + a.group < a.n_frames ? g0 + a.group : a.n_frames;
        const uint64_t f0 = g0 + (uint64_t)ch * a.fpc;      // (past g1 for the empty chunks of a short last group: zeros)
        const uint64_t f1 = f0 + a.fpc < g1 ? f0 + a.fpc : g1;

        SumAcc<T> acc[kSub][kBlock];
#pragma unroll
        for (int r = 0; r < kSub; ++r)
#pragma unroll
            for (int k = 0; k < kBlock; ++k) acc[r][k] = 0;
        bool bad = false;
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
            if (!sum_extract<T>(acc, cur, s_image)) atomicMax(&a.status[0], kStatusCorrupt);
            cur = nxt;
        }
        if (bad && threadIdx.x == 0) atomicMax(&a.status[0], kStatusCorrupt);

        // ---- the sums leave once: per wavefront, its 64 blocks (768 values) as int64 through LDS, then consecutive elements
        // per lane (every store instruction writes whole lines)
        const int lane = lane_id(), wave = wave_id();
        int64_t* const row = reinterpret_cast<int64_t*>(s_image) + wave * (kWave * kBlock);
        const bool part = a.partial != nullptr;
        void* const dst = part ? a.partial : a.out;
        const int code = part ? (PixelTraits<T>::bits == 32 ? kSumPart64 : kSumPart32) : a.out_code;
        const uint64_t base = part ? ((uint64_t)ch * a.n_out + j) * g.n_values : j * g.n_values;
#pragma unroll
        for (int r = 0; r < kSub; ++r) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kBlock; ++k) row[lane * kBlock + k] = acc_value<T>(acc[r][k]);
            __syncthreads();
            const uint64_t first = ((uint64_t)t * kSub * kThreads + (uint64_t)r * kThreads + (uint64_t)wave * kWave) * kBlock;
            if (first < g.n_values) {
                const uint32_t n_valid = g.n_values - first < (uint64_t)(kWave * kBlock) ? (uint32_t)(g.n_values - first) : kWave * kBlock;
                for (uint32_t e = lane; e < n_valid; e += kWave) put_sum(dst, base + first + e, code, row[e]);
            }
        }
        __syncthreads();                                    // (the next unit's first frame reuses the image)
    }
}

// partial slabs [chunks][n_out * n_values] -> the sums, added in chunk order and converted
__global__ __launch_bounds__(kThreads) void k_sum_reduce(const void* __restrict__ partial, int acc64, int acc_signed, uint32_t chunks,
                                                          uint64_t n_elems, void* __restrict__ out, int code) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n_elems; i += (uint64_t)gridDim.x * kThreads) {
        int64_t s = 0;
        for (uint32_t c = 0; c < chunks; ++c) {
            if (acc64) s += (int64_t)static_cast<const uint64_t*>(partial)[(uint64_t)c * n_elems + i];
            else {
                const uint32_t v = static_cast<const uint32_t*>(partial)[(uint64_t)c * n_elems + i];
                s += acc_signed ? (int64_t)(int32_t)v : (int64_t)v;
            }
        }
        put_sum(out, i, code, s);
    }
}

SumPlan sum_plan(int dtype, const FrameGeom& g, uint64_t n_frames, uint64_t group) {
    SumPlan p;
    const uint32_t kSub = kSumSubTiles;
    p.tpf = (g.n_blocks + kSub * kThreads - 1) / (kSub * kThreads);
    p.n_out = (n_frames + group - 1) / group;
    const uint64_t per_group = group < n_frames ? group : n_frames;
    const uint64_t max_fpc = dtype >= TRPX_U32 ? 0xFFFFFFFFull : 65535ull;   // 32-bit accumulators: 65 535 frames of 8/16-bit values
    const uint64_t units = p.n_out * p.tpf;
    uint64_t chunks = units < kSumTargetUnits ? (kSumTargetUnits + units - 1) / units : 1;
    if (chunks > per_group) chunks = per_group;
    uint64_t fpc = (per_group + chunks - 1) / chunks;
    if (fpc > max_fpc) fpc = max_fpc;
    p.fpc = (uint32_t)fpc;
    p.chunks = (uint32_t)((per_group + fpc - 1) / fpc);
    p.partial_bytes = p.chunks > 1 ? align_up((uint64_t)p.chunks * p.n_out * g.n_values * (dtype >= TRPX_U32 ? 8 : 4), 256) : 0;
    return p;
}

template <typename T>
static hipError_t launch_sum_t(const SumArgs& a, hipStream_t st) {
    const uint64_t units = (uint64_t)a.n_out * a.chunks * a.tpf;
    const uint32_t grid = (uint32_t)(units < (1ull << 22) ? units : (1ull << 22));
    hipLaunchKernelGGL((k_sum_tiles<T>), dim3(grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_decode_sum(int dtype, const SumArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    const hipError_t e = for_pixel_type(dtype, [&]<class T>() { return launch_sum_t<T>(a, st); });
    if (e != hipSuccess || !a.partial) return e;
    const uint64_t n = a.n_out * a.geom.n_values;
    const uint64_t blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_sum_reduce, dim3((uint32_t)(blocks < 8192 ? blocks : 8192)), dim3(kThreads), 0, st, a.partial,
                       dtype >= TRPX_U32 ? 1 : 0, dtype & 1, a.chunks, n, a.out, a.out_code);
    return hipGetLastError();
}

}  // namespace trpx
