// Labelled summing decode (trpx_decode_sum_labelled): a stack with its decode index and one device label per frame -> the sum of
// the frames of every label, without writing the decoded frames.  trpx_decode_bins' transpose: a label per frame, not per pixel.
//   order     the frames with an output are put in the order of their labels, on the device: k_lab_count (histogram), k_lab_scan
//             (starts[n_out + 1], the cursors, counts_out), k_lab_scatter (order[starts[l] + k] = (f, l); a cursor per label with an
//             integer atomic: which frame stands where inside a label does not change an integer sum).  Up to 4096 frames and
//             8192 outputs one workgroup does all three in LDS (k_lab_order_small).  The scan also lists the labels the merge
//             has work for.
//   walk      that order is cut at fixed positions into chunks of fpc frames (label_runs.hpp).  The work unit is (tile t, chunk c):
//             one 256-thread workgroup walks order[c * fpc ..) through sum_tile.hpp's three-frame pipeline, the frame numbers from
//             the list (entries i + 2 and i + 3 in flight), k_sum_tiles' accumulators in registers.  Whenever the label changes and
//             at the chunk's end they leave through LDS as whole lines: converted into sums_out for a label that lies inside the
//             chunk, raw into slot 0 / 1 of the chunk's partial slab for one that crosses a cut.
//   merge     k_lab_merge, over the listed labels: 0 for a label without frames, the partials in chunk order (int64) and one
//             conversion for one that crosses a cut.  A label the walk wrote is not listed.
// The launch shapes depend on n_frames, n_values, n_out and the pixel type alone; what the labels hold decides only which units
// find work.  A MASKED FRAME IS NOT IN THE ORDER: no byte of it is read.
// HBM traffic: labels 2 x, 16 B per ordered frame, the labelled frames' stream + widths once, n_out * n_values sums written
// (+ 2 x the runs that cross a cut).
#include "codec_common.hpp"
#include "decode_sum_labelled.hpp"
#include "label_runs.hpp"
#include "put_sum.hpp"
#include "sum_tile.hpp"
#include <type_traits>

namespace trpx {

namespace {

template <typename T> using LabAcc = std::conditional_t<PixelTraits<T>::bits == 32, uint64_t, uint32_t>;

template <typename T>
__device__ __forceinline__ int64_t lab_acc_value(LabAcc<T> a) {
    if constexpr (PixelTraits<T>::bits == 32) return (int64_t)a;
    else if constexpr (PixelTraits<T>::is_signed) return (int64_t)(int32_t)a;
    else return (int64_t)a;
}

// entry i of the order, by a vector load (sum_load_pre's reason: a scalar load in flight shares lgkmcnt with LDS)
__device__ __forceinline__ uint2 lab_entry(const uint2* __restrict__ order, uint32_t i) {
    asm volatile("" : "+v"(i));
    return order[i];
}

// ---- the order ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_lab_count(const uint32_t* __restrict__ labels, uint64_t n_frames, uint32_t n_out,
                                                         uint32_t* __restrict__ counts) {
    for (uint64_t f = (uint64_t)blockIdx.x * kThreads + threadIdx.x; f < n_frames; f += (uint64_t)gridDim.x * kThreads) {
        const uint32_t l = labels[f];
        if (l < n_out) atomicAdd(&counts[l], 1u);
    }
}

// exclusive scan of the counts (single workgroup): starts[0 .. n_out], the cursors, the caller's counts, and the merge's list
// (*n_todo: cleared with the counts)
__global__ __launch_bounds__(kThreads) void k_lab_scan(const uint32_t* __restrict__ counts, uint32_t n_out, uint32_t fpc,
                                                        uint32_t* __restrict__ starts, uint32_t* __restrict__ cursor,
                                                        uint32_t* __restrict__ counts_out, uint32_t* __restrict__ todo,
                                                        uint32_t* __restrict__ n_todo) {
    __shared__ uint32_t s_tot[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_out; base += kThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_out ? counts[i] : 0u;
        uint32_t total;
        const uint32_t excl = block_exclusive_scan(v, s_tot, &total);
        if (i < n_out) {
            starts[i] = carry + excl;
            cursor[i] = carry + excl;
            if (counts_out) counts_out[i] = v;
            uint32_t cf, cl;
            if (label_merge_plan(carry + excl, carry + excl + v, fpc, &cf, &cl) != kLabelDirect) todo[atomicAdd(n_todo, 1u)] = i;
        }
        carry += total;
        __syncthreads();                                    // s_tot is reused next iteration
    }
    if (threadIdx.x == 0) starts[n_out] = carry;
}

__global__ __launch_bounds__(kThreads) void k_lab_scatter(const uint32_t* __restrict__ labels, uint64_t n_frames, uint32_t n_out,
                                                           uint32_t* __restrict__ cursor, uint2* __restrict__ order) {
    for (uint64_t f = (uint64_t)blockIdx.x * kThreads + threadIdx.x; f < n_frames; f += (uint64_t)gridDim.x * kThreads) {
        const uint32_t l = labels[f];
        if (l >= n_out) continue;
        const uint32_t pos = atomicAdd(&cursor[l], 1u);
        if (pos < n_frames) order[pos] = make_uint2((uint32_t)f, l);   // (always, unless the labels changed under the call)
    }
}

// The three steps above in one workgroup, histogram and cursors in LDS: short stacks with few outputs (the usual scan), where the
// four launches would cost more than the walk.  Also the call's status clear.
constexpr uint32_t kLabSmallThreads = 1024;
__global__ __launch_bounds__(kLabSmallThreads) void k_lab_order_small(const uint32_t* __restrict__ labels, uint32_t n_frames, uint32_t n_out,
                                                                      uint32_t fpc, uint32_t* __restrict__ starts, uint2* __restrict__ order,
                                                                      uint32_t* __restrict__ counts_out, uint32_t* __restrict__ todo,
                                                                      uint32_t* __restrict__ n_todo, uint32_t* __restrict__ status_to_clear) {
    __shared__ uint32_t s_cnt[kLabelledSmallOut];
    __shared__ uint32_t s_tot[kLabSmallThreads / kWave];
    __shared__ uint32_t s_todo;
    const uint32_t tid = threadIdx.x;
    if (status_to_clear && tid < 8) status_to_clear[tid] = 0u;
    if (tid == 0) s_todo = 0u;
    for (uint32_t i = tid; i < n_out; i += kLabSmallThreads) s_cnt[i] = 0u;
    __syncthreads();
    for (uint32_t f = tid; f < n_frames; f += kLabSmallThreads) {
        const uint32_t l = labels[f];
        if (l < n_out) atomicAdd(&s_cnt[l], 1u);
    }
    __syncthreads();
    // exclusive scan: `per` consecutive counts a thread, the threads' totals through the waves
    const uint32_t per = (n_out + kLabSmallThreads - 1) / kLabSmallThreads, b = tid * per;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < per; ++k)
        if (b + k < n_out) sum += s_cnt[b + k];
    const uint32_t inc = wave_inclusive_scan(sum);
    if (lane_id() == 63) s_tot[wave_id()] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (int k = 0; k < wave_id(); ++k) run += s_tot[k];
    for (uint32_t k = 0; k < per; ++k)
        if (b + k < n_out) {
            const uint32_t c = s_cnt[b + k];
            if (counts_out) counts_out[b + k] = c;
            starts[b + k] = run;
            s_cnt[b + k] = run;                             // (from here on: the label's cursor)
            uint32_t cf, cl;
            if (label_merge_plan(run, run + c, fpc, &cf, &cl) != kLabelDirect) todo[atomicAdd(&s_todo, 1u)] = b + k;
            run += c;
        }
    if (tid == kLabSmallThreads - 1) starts[n_out] = run;   // (the last thread ends at the total)
    __syncthreads();
    if (tid == 0) *n_todo = s_todo;
    for (uint32_t f = tid; f < n_frames; f += kLabSmallThreads) {
        const uint32_t l = labels[f];
        if (l >= n_out) continue;
        const uint32_t pos = atomicAdd(&s_cnt[l], 1u);
        if (pos < n_frames) order[pos] = make_uint2(f, l);
    }
}

}  // namespace

// ---- the walk ----------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void k_sum_labelled(LabelledArgs a) {
    constexpr int kSub = sum_sub_tiles<T>();
    __shared__ __attribute__((aligned(16))) uint32_t s_image[sum_stage_dwords<T>()];
    __shared__ uint32_t s_wtot[kSub * 4];
    if (a.status[0] != 0) return;                           // corrupt chain (the walk or the locator said so): produce nothing
    const FrameGeom g = a.geom;
    const uint32_t kept = a.starts[a.n_out];
    const uint32_t n_kept = kept < a.n_frames ? kept : (uint32_t)a.n_frames;
    const uint32_t f_last = (uint32_t)a.n_frames - 1;
    const uint64_t units = (uint64_t)a.n_chunks * a.tpf;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t t = (uint32_t)(unit % a.tpf);        // adjacent workgroups: adjacent tiles of one chunk
        const uint32_t ch = (uint32_t)(unit / a.tpf);
        uint32_t p0, p1;
        label_chunk_span(ch, a.fpc, n_kept, &p0, &p1);
        if (p0 >= p1) continue;                             // behind the last labelled frame: nothing to do

        LabAcc<T> acc[kSub][kBlock];
#pragma unroll
        for (int r = 0; r < kSub; ++r)
#pragma unroll
            for (int k = 0; k < kBlock; ++k) acc[r][k] = 0;
        bool bad = false, ok = true;
        uint4 R[sum_prefetch_loads<T>()];
        SumPre<T> pn;
        SumCur<T> cur;
        // the list runs two entries ahead of the widths' loads (sum_load_pre of position i + 2 finds its frame number loaded)
        const uint2 e0 = lab_entry(a.order, p0);
        uint2 e1 = p0 + 1 < p1 ? lab_entry(a.order, p0 + 1) : e0;
        uint2 e2 = p0 + 2 < p1 ? lab_entry(a.order, p0 + 2) : e0;
        uint32_t lab_cur = e0.y, lab_n1 = e1.y;
        sum_load_pre(pn, a.frame_offsets, g, (uint64_t)(e0.x < f_last ? e0.x : f_last), t, a.widths, a.tile_off);
        bad = !sum_scan(cur, pn, g, t, a.terse_bytes, s_wtot);
        if (!bad) sum_fetch<T>(R, cur, a.terse, a.terse_bytes);
        if (p0 + 1 < p1) sum_load_pre(pn, a.frame_offsets, g, (uint64_t)(e1.x < f_last ? e1.x : f_last), t, a.widths, a.tile_off);

        for (uint32_t i = p0; i < p1 && !bad; ++i) {
            __syncthreads();                                // (the previous frame's extraction, or its run's flush, is done with the image)
            sum_stage<T>(s_image, R, cur.n_dw);
            __syncthreads();
            SumCur<T> nxt;
            uint2 e3 = e2;
            if (i + 1 < p1) {                               // position i + 1: scan, then its stream is in flight during i's extraction
                bad = !sum_scan(nxt, pn, g, t, a.terse_bytes, s_wtot);
                if (!bad) sum_fetch<T>(R, nxt, a.terse, a.terse_bytes);
                if (i + 2 < p1) sum_load_pre(pn, a.frame_offsets, g, (uint64_t)(e2.x < f_last ? e2.x : f_last), t, a.widths, a.tile_off);
                if (i + 3 < p1) e3 = lab_entry(a.order, i + 3);
            }
#pragma unroll
            for (int r = 0; r < kSub; ++r) {
                uint32_t u[kBlock];
                sum_fields<T>(u, ok, cur, r, s_image);
#pragma unroll
                for (int k = 0; k < kBlock; ++k) {
                    if constexpr (PixelTraits<T>::bits == 32)
                        acc[r][k] += PixelTraits<T>::is_signed ? (uint64_t)(int64_t)(int32_t)u[k] : (uint64_t)u[k];
                    else acc[r][k] += u[k];                 // (sign-extended to 32 bits: two's complement sums)
                }
            }
            const uint32_t l = uniform32(lab_cur);
            if (i + 1 == p1 || uniform32(lab_n1) != l) {
                // ---- the run is over: its sums leave, per wavefront its 64 blocks (768 values) as int64 through LDS, then
                // consecutive elements per lane (every store instruction writes whole lines)
                uint32_t s = 0, e = 0;
                if (l < a.n_out) { s = a.starts[l]; e = a.starts[l + 1]; }
                const bool live = e > s && !bad;            // (always, unless the labels changed under the call)
                const bool direct = live && label_run_direct(s, e, a.fpc);
                void* const dst = direct ? a.out : a.partial;
                const int code = direct ? a.out_code : (PixelTraits<T>::bits == 32 ? kSumPart64 : kSumPart32);
                const uint64_t base = direct ? (uint64_t)l * g.n_values : label_slab_at(ch, label_run_slot(s, ch * a.fpc), a.stride);
                const int lane = lane_id(), wave = wave_id();
                int64_t* const row = reinterpret_cast<int64_t*>(s_image) + wave * (kWave * kBlock);
#pragma unroll
                for (int r = 0; r < kSub; ++r) {
                    __syncthreads();
#pragma unroll
                    for (int k = 0; k < kBlock; ++k) {
                        row[lane * kBlock + k] = lab_acc_value<T>(acc[r][k]);
                        acc[r][k] = 0;
                    }
                    __syncthreads();
                    const uint64_t first = ((uint64_t)t * kSub * kThreads + (uint64_t)r * kThreads + (uint64_t)wave * kWave) * kBlock;
                    if (live && first < g.n_values) {
                        const uint32_t n_valid = g.n_values - first < (uint64_t)(kWave * kBlock) ? (uint32_t)(g.n_values - first) : kWave * kBlock;
                        for (uint32_t x = lane; x < n_valid; x += kWave) put_sum(dst, base + first + x, code, row[x]);
                    }
                }
            }
            cur = nxt;
            lab_cur = lab_n1;
            lab_n1 = e2.y;
            e2 = e3;
        }
        if (!ok) atomicMax(&a.status[0], kStatusCorrupt);
        if (bad && threadIdx.x == 0) atomicMax(&a.status[0], kStatusCorrupt);
        __syncthreads();                                    // (the next unit's first frame reuses the image)
    }
}

namespace {

// ---- the merge: a workgroup per (listed label, 256 values); the labels the walk wrote are not on the list, and a call without
// any (every label inside a chunk) ends after one load a workgroup -------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_lab_merge(LabelledArgs a, int acc64, int acc_signed) {
    if (a.status[0] != 0) return;                           // (the outputs are unspecified; the slab may hold nothing)
    const uint64_t n_values = a.geom.n_values;
    const uint32_t listed = a.counts[a.n_out];
    const uint64_t spans = (n_values + kThreads - 1) / kThreads, units = (uint64_t)(listed < a.n_out ? listed : a.n_out) * spans;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t l = a.todo[unit / spans];
        const uint64_t p = (unit % spans) * kThreads + threadIdx.x;
        if (l >= a.n_out) continue;                         // (never)
        uint32_t cf = 0, cl = 0;
        const int plan = label_merge_plan(a.starts[l], a.starts[l + 1], a.fpc, &cf, &cl);
        if (plan == kLabelDirect || p >= n_values) continue;
        int64_t sum = 0;
        if (plan == kLabelMerged) {
            if (cl >= a.n_chunks) continue;                 // (never, unless the labels changed under the call)
            const uint32_t s = a.starts[l];
            for (uint32_t c = cf; c <= cl; ++c) {
                const uint64_t at = label_slab_at(c, label_run_slot(s, c * a.fpc), a.stride) + p;
                if (acc64) sum += (int64_t)static_cast<const uint64_t*>(a.partial)[at];
                else {
                    const uint32_t v = static_cast<const uint32_t*>(a.partial)[at];
                    sum += acc_signed ? (int64_t)(int32_t)v : (int64_t)v;
                }
            }
        }
        put_sum(a.out, (uint64_t)l * n_values + p, a.out_code, sum);
    }
}

template <typename T>
hipError_t launch_walk_t(const LabelledArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_sum_labelled<T>), dim3(grid_capped((uint64_t)a.n_chunks * a.tpf, 1, 1u << 22)), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_decode_sum_labelled(int dtype, const LabelledArgs& a, bool clear_status, hipStream_t st) {
    if (labelled_order_small(a.n_frames, a.n_out)) {
        hipLaunchKernelGGL(k_lab_order_small, dim3(1), dim3(kLabSmallThreads), 0, st, a.labels, (uint32_t)a.n_frames, a.n_out, a.fpc, a.starts,
                           a.order, a.counts_out, a.todo, a.counts + a.n_out, clear_status ? a.status : nullptr);
    } else {
        // the histogram's zeros, the list's count and the status block in one launch (whole 8-byte words up to the cursors)
        const uint64_t words = align_up(4 * ((uint64_t)a.n_out + 1), 8) / 8;
        hipLaunchKernelGGL(k_zero_words<0>, dim3(grid_capped(words, kThreads)), dim3(kThreads), 0, st, reinterpret_cast<uint64_t*>(a.counts), words,
                           reinterpret_cast<uint64_t*>(a.status), (uint64_t)(clear_status ? 4 : 0));
        hipLaunchKernelGGL(k_lab_count, dim3(grid_capped(a.n_frames, kThreads)), dim3(kThreads), 0, st, a.labels, a.n_frames, a.n_out, a.counts);
        hipLaunchKernelGGL(k_lab_scan, dim3(1), dim3(kThreads), 0, st, a.counts, a.n_out, a.fpc, a.starts, a.cursor, a.counts_out, a.todo,
                           a.counts + a.n_out);
        hipLaunchKernelGGL(k_lab_scatter, dim3(grid_capped(a.n_frames, kThreads)), dim3(kThreads), 0, st, a.labels, a.n_frames, a.n_out, a.cursor,
                           a.order);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = for_pixel_type(dtype, [&]<class T>() { return launch_walk_t<T>(a, st); });
    if (e != hipSuccess) return e;
    const uint64_t units = (uint64_t)a.n_out * ((a.geom.n_values + kThreads - 1) / kThreads);
    // (how many labels are listed is the labels' business: the grid is sized for all of them, capped where a stride costs nothing)
    hipLaunchKernelGGL(k_lab_merge, dim3(grid_capped(units, 1, 2048)), dim3(kThreads), 0, st, a, dtype >= TRPX_U32 ? 1 : 0, dtype & 1);
    return hipGetLastError();
}

}  // namespace trpx
