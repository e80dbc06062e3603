// Value histograms straight from the stream (trpx_decode_hist): a stack with its decode index -> hist[g][b] = the number of pixels
// of the frames of group g (`group` consecutive frames) whose bin is b, bin(v) = clamp((v - lo) >> shift, 0, n_bins - 1)
// (hist_bin.hpp), without expanding the frames.  The shape is spans -> (reduce); the walk of a run is group_runs.hpp's (run_walk),
// the consumer is a histogram in LDS.
//
//   k_hist_spans    a workgroup per SPAN: consecutive runs (kRun groups of 256 blocks each) out of a group's frames x runs per
//                   frame (decode_hist.hpp: the rule), its four wavefronts taking the runs in turn; a span may cross frames.  The
//                   workgroup keeps uint32 counts[n_bins] in dynamic LDS (sized by n_bins: few bins do not cost occupancy), zeroed
//                   first; a span holds fewer than 2^32 values, so they cannot wrap.  The walk's `want` vote does the skipping: a
//                   block's width bounds its values, and a width whose whole value range lies in ONE bin (hist_block_one_bin;
//                   per width, so a table of 33 entries in LDS, written once per workgroup) is counted there and then -- its value
//                   count into that bin, one non-returning LDS add (ds_add_u32) -- and is no candidate: its payload is never
//                   fetched.  Width-0 blocks are the first case of it: their twelve zeros are pixels and are counted in bin(0).
//                   Only blocks that straddle a bin edge are compacted into the list and extracted; per extracted block
//                   hist_count_block: neighbours of equal bin counted in registers, one LDS add per change of bin.  No support
//                   words, no support kernel: the vote needs the width alone.  Behind a barrier the workgroup widens its counts
//                   and stores them with plain coalesced stores: to hist_out where a group is one span, to
//                   partials[group][span][bin] otherwise.  A group of 256 blocks that fails validation sets CORRUPT and adds nothing.
//   k_reduce_parts  (group_runs.hpp) only with more than one span per group: per (group, bin) the spans' counts, added in span
//                   order.
// Integer counting only.  The LDS adds are the one place where wavefronts add into shared memory; addition is associative and
// commutative, so the counts do not depend on the order in which they arrive.  Global memory sees no atomic except the status
// word.  The output is bit-identical across runs, input forms, sub-stacks and launch shapes.
#include <algorithm>
#include "codec_common.hpp"
#include "decode_hist.hpp"
#include "group_front.hpp"
#include "group_runs.hpp"

namespace trpx {

namespace {

template <typename T, bool kNarrow>
__device__ __forceinline__ void hist_run(const HistArgs& a, uint64_t run, uint32_t runs_per_frame, const uint32_t* __restrict__ width_bin,
                                         uint32_t* __restrict__ list, uint32_t* __restrict__ counts) {
    run_walk<T>(a, run_place(a, run, runs_per_frame), NoSupport{}, a.status, list,
                [&](uint32_t, uint32_t w, uint32_t nb) {    // (a group that reaches the vote is valid: w <= the type's bits)
                    const uint32_t bin = width_bin[w < kHistMaxWidth ? w : kHistMaxWidth];
                    if (bin == kHistNoBin) return true;
                    atomicAdd(&counts[bin], nb);            // the whole block from its width: 12 values, or the frame's partial last block
                    return false;
                },
                [&](uint32_t, uint32_t, uint32_t nr, const uint32_t (&o)[PackedDwords<T>::n], bool) {
                    if (nr == 0u) return;
                    const auto add = [&](uint32_t bin, uint32_t n) { atomicAdd(&counts[bin], n); };
                    if constexpr (kNarrow)                  // (v - lo fits 32 bits: three instructions a value, not a dozen)
                        hist_count_bins(nr, [&](int i) { return hist_bin32((int32_t)packed_value<T>(o, i), (int32_t)a.lo, a.shift, a.n_bins); }, a.n_bins, add);
                    else
                        hist_count_bins(nr, [&](int i) { return hist_bin((int64_t)packed_value<T>(o, i), a.lo, a.shift, a.n_bins); }, a.n_bins, add);
                });
}

}  // namespace

// dst: hist_out (spans == 1) or the partial counts; a unit = (group, span), the runs [span * R / spans, (span + 1) * R / spans)
// of the group's R = frames * runs_per_frame runs.  kNarrow: hist_narrow_ok(lo, the type's bits) -- the 32-bit bin arithmetic
template <typename T, bool kNarrow>
__global__ __launch_bounds__(kThreads) void k_hist_spans(HistArgs a, uint32_t runs_per_frame, uint64_t* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_counts[];         // [n_bins]
    __shared__ uint32_t s_width_bin[kHistMaxWidth + 1];                          // per width: its one bin, or kHistNoBin
    uint32_t* const list = wave_list();
    const uint64_t units = a.n_groups * a.spans;
    const uint32_t wave = (uint32_t)wave_id();
    if (threadIdx.x <= kHistMaxWidth) {
        uint32_t bin;
        const bool one = hist_block_one_bin(threadIdx.x, PixelTraits<T>::is_signed, a.lo, a.shift, a.n_bins, &bin);
        s_width_bin[threadIdx.x] = one ? bin : kHistNoBin;
    }
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {         // (uniform: every barrier below is reached by all)
        for (uint32_t i = threadIdx.x; i < a.n_bins; i += kThreads) s_counts[i] = 0u;
        __syncthreads();                                    // (the table too, in the first round)
        const uint64_t grp = unit / a.spans;
        const uint64_t span = unit - grp * a.spans;
        const uint64_t f0 = grp * a.group;
        const uint64_t frames = a.n_frames - f0 < a.group ? a.n_frames - f0 : a.group;
        const uint64_t R = frames * runs_per_frame;          // (a call has fewer than 2^24 groups of 256 blocks: R < 2^24, spans <= R, the products below stay in 64 bits)
        const uint64_t r_lo = span * R / a.spans, r_hi = (span + 1) * R / a.spans;
        for (uint64_t r = r_lo + wave; r < r_hi; r += kWavesPerWg)
            hist_run<T, kNarrow>(a, f0 * runs_per_frame + r, runs_per_frame, s_width_bin, list, s_counts);
        __syncthreads();
        uint64_t* __restrict__ out = dst + unit * a.n_bins;
        for (uint32_t i = threadIdx.x; i < a.n_bins; i += kThreads) out[i] = (uint64_t)s_counts[i];
        __syncthreads();                                    // (the next unit zeroes the counts)
    }
}

uint32_t hist_spans_per_group(const FrameGeom& g, uint64_t n_frames, uint64_t group) {
    if (!n_frames || !group) return 0;
    const uint64_t frames = std::min(group, n_frames), n_groups = (n_frames + frames - 1) / frames;
    const uint64_t R = frames * runs_per_frame(g);
    const uint64_t by_runs = (R + kWavesPerWg - 1) / kWavesPerWg;
    const uint64_t by_groups = (kHistTargetWgs + n_groups - 1) / n_groups;
    const uint64_t by_counter = (R + kHistMaxSpanRuns - 1) / kHistMaxSpanRuns;
    return (uint32_t)std::max<uint64_t>(by_counter, std::min<uint64_t>(by_runs, std::max<uint64_t>(1, by_groups)));
}

hipError_t launch_decode_hist(int dtype, const HistArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    // launch shapes from the geometry, the group and the number of bins alone: a workgroup per (group, span) up to 2^20
    // workgroups, strided units beyond; 4 * n_bins bytes of dynamic LDS
    const uint32_t rpf = runs_per_frame(a.geom);
    const uint32_t grid = grid_capped(a.n_groups * a.spans, 1, 1u << 20);
    const uint32_t rgrid = grid_capped(a.n_groups * a.n_bins, kThreads);
    uint64_t* dst = a.spans > 1 ? a.partials : a.hist_out;
    return for_pixel_type(dtype, [&]<class T>() {
        bool narrow = false;
        if constexpr (sizeof(T) <= 2) narrow = hist_narrow_ok(a.lo, 8 * sizeof(T));
        if constexpr (sizeof(T) <= 2)
            if (narrow) hipLaunchKernelGGL((k_hist_spans<T, true>), dim3(grid), dim3(kThreads), 4 * (size_t)a.n_bins, st, a, rpf, dst);
        if (!narrow) hipLaunchKernelGGL((k_hist_spans<T, false>), dim3(grid), dim3(kThreads), 4 * (size_t)a.n_bins, st, a, rpf, dst);
        if (a.spans > 1)                                    // (counts are sums modulo 2^64 like any other: the reduce's int64 is their bits)
            hipLaunchKernelGGL(k_reduce_parts<0>, dim3(rgrid), dim3(kThreads), 0, st, reinterpret_cast<const int64_t*>(a.partials), a.n_groups,
                               a.spans, a.n_bins, reinterpret_cast<int64_t*>(a.hist_out));
        return hipGetLastError();                           // (one check behind the clear and the launches, as the siblings do: the first error stays)
    });
}

}  // namespace trpx
