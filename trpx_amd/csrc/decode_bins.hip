// Per-frame sums over labelled pixel bins (trpx_decode_bins): a stack with its decode index and ONE map of uint16 labels ->
// bins[f][b] = sum over the pixels p of frame f with labels[p] == b of px[f][p] in int64, without expanding the frames: the radial
// profile / azimuthal integration of every frame, whatever the number of bins.  The shape is support -> spans -> (reduce); the
// walk of a run is group_runs.hpp's (run_walk), the consumer is a histogram-by-label in LDS.
//
//   k_bins_support  one bit per block of a frame: some label of the block's <= 12 pixels is a bin (< n_bins).  In every call: the
//                   map is device data that a graph replay may have changed.
//   k_bins_spans    a workgroup per SPAN: consecutive runs (kRun groups each) of one frame, its four wavefronts taking the runs in
//                   turn.  The workgroup keeps uint64 sums[n_bins] in dynamic LDS (sized by n_bins: few bins do not cost
//                   occupancy), zeroed first.  The CANDIDATE blocks are those with a width and their support bit; per extracted
//                   block: its 12 labels (bytes 24 * block of the map: three 8-byte loads), and bins_merge.hpp: neighbouring
//                   values of equal label summed in registers, one 64-bit LDS atomic add (ds_add_u64) per label change, none for
//                   a zero sum or a label that is no bin.  Behind a barrier the workgroup stores its n_bins sums with plain
//                   coalesced stores: to bins_out where a frame is one span, to partials[frame][span][bin] otherwise.  A group
//                   that fails validation sets CORRUPT and adds nothing.
//   k_reduce_parts  (group_runs.hpp) only with more than one span per frame: per (frame, bin) the spans' partial sums, added in
//                   span order.
// Integer arithmetic only.  The LDS atomics are the one place where wavefronts add into shared memory; addition modulo 2^64 is
// associative and commutative, so the sums do not depend on the order in which they arrive (and cannot leave int64: a frame has
// fewer than 2^29 values of magnitude at most 2^32).  Global memory sees no atomic except the status word.  The output is
// bit-identical across runs, input forms and launch shapes.
#include <algorithm>
#include "codec_common.hpp"
#include "decode_bins.hpp"
#include "group_front.hpp"
#include "group_runs.hpp"

namespace trpx {

namespace {

// the bits of value i of an extracted block as int64 (signed types: sign-extended)
template <typename T>
__device__ __forceinline__ uint64_t bins_value(const uint32_t (&o)[PackedDwords<T>::n], int i) {
    return (uint64_t)(int64_t)packed_value<T>(o, i);
}

template <typename T>
__device__ __forceinline__ void bins_run(const BinsArgs& a, uint64_t run, uint32_t runs_per_frame, uint32_t n_words, bool aligned8,
                                         uint32_t* __restrict__ list, unsigned long long* __restrict__ sums) {
    run_walk<T>(a, run_place(a, run, runs_per_frame), SupportWords{a.support, n_words}, a.status, list,
                [](uint32_t, uint32_t w, uint32_t) { return w != 0u; },
                [&](uint32_t, uint32_t block, uint32_t nr, const uint32_t (&o)[PackedDwords<T>::n], bool) {
                    if (nr != 0u) {                         // (nr values from pixel 12 * block on: nothing behind labels[n_values) is read)
                        const BinsLabels l = bins_load_labels(a.labels, (uint64_t)block * kBlock, nr, aligned8);
                        bins_merge(nr, [&](int i) { return bins_value<T>(o, i); }, l, a.n_bins,
                                   [&](uint32_t bin, uint64_t s) { atomicAdd(&sums[bin], (unsigned long long)s); });
                    }
                });
}

}  // namespace

// bit b of the support words: some label of block b (pixels 12 b .. 12 b + 11 of a frame, as far as the frame goes) is a bin
__global__ __launch_bounds__(kThreads) void k_bins_support(const uint16_t* __restrict__ labels, uint32_t n_bins, FrameGeom g, bool aligned8,
                                                           uint32_t* __restrict__ support) {
    support_write(support, g, [&](uint64_t first, uint32_t nr) { return bins_any_label(bins_load_labels(labels, first, nr, aligned8), n_bins); });
}

// dst: bins_out (spans == 1) or the partial sums; a unit = (frame, span), the runs [span * rpf / spans, (span + 1) * rpf / spans)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_bins_spans(BinsArgs a, uint32_t runs_per_frame, bool aligned8, int64_t* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_sums[];   // [n_bins]
    uint32_t* const list = wave_list();
    const uint64_t units = a.n_frames * a.spans;
    const uint32_t n_words = (uint32_t)support_words(a.geom);
    const uint32_t wave = (uint32_t)wave_id();
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {        // (uniform: every barrier below is reached by all)
        for (uint32_t i = threadIdx.x; i < a.n_bins; i += kThreads) s_sums[i] = 0ull;
        __syncthreads();
        const uint64_t frame = unit / a.spans;
        const uint32_t span = (uint32_t)(unit - frame * a.spans);
        const uint32_t r_lo = (uint32_t)((uint64_t)span * runs_per_frame / a.spans);
        const uint32_t r_hi = (uint32_t)((uint64_t)(span + 1) * runs_per_frame / a.spans);
        for (uint32_t r = r_lo + wave; r < r_hi; r += kWavesPerWg)
            bins_run<T>(a, frame * runs_per_frame + r, runs_per_frame, n_words, aligned8, list, s_sums);
        __syncthreads();
        int64_t* __restrict__ out = dst + unit * a.n_bins;
        for (uint32_t i = threadIdx.x; i < a.n_bins; i += kThreads) out[i] = (int64_t)s_sums[i];
        __syncthreads();                                    // (the next unit zeroes the sums)
    }
}

uint32_t bins_spans_per_frame(const FrameGeom& g, uint64_t n_frames) {
    const uint64_t by_runs = ((uint64_t)runs_per_frame(g) + kWavesPerWg - 1) / kWavesPerWg;
    const uint64_t by_frames = n_frames ? (kBinsTargetWgs + n_frames - 1) / n_frames : 1;
    return (uint32_t)std::min<uint64_t>(by_runs, std::max<uint64_t>(1, by_frames));
}

hipError_t launch_decode_bins(int dtype, const BinsArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    // launch shapes from the geometry and the number of bins alone: a workgroup per (frame, span) up to 2^20 workgroups, strided
    // units beyond; 8 * n_bins bytes of dynamic LDS
    const uint32_t rpf = runs_per_frame(a.geom);
    const uint32_t grid = grid_capped(a.n_frames * a.spans, 1, 1u << 20);
    const uint32_t sgrid = grid_capped(a.geom.n_blocks, kThreads);
    const uint32_t rgrid = grid_capped(a.n_frames * a.n_bins, kThreads);
    const bool aligned8 = (uintptr_t)a.labels % 8 == 0;
    int64_t* dst = a.spans > 1 ? a.partials : a.bins_out;
    return for_pixel_type(dtype, [&]<class T>() {
        hipLaunchKernelGGL(k_bins_support, dim3(sgrid), dim3(kThreads), 0, st, a.labels, a.n_bins, a.geom, aligned8, a.support);
        hipLaunchKernelGGL((k_bins_spans<T>), dim3(grid), dim3(kThreads), 8 * (size_t)a.n_bins, st, a, rpf, aligned8, dst);
        if (a.spans > 1)
            hipLaunchKernelGGL(k_reduce_parts<0>, dim3(rgrid), dim3(kThreads), 0, st, a.partials, a.n_frames, a.spans, a.n_bins, a.bins_out);
        return hipGetLastError();                           // (one check behind the clear and the launches, as the siblings do: the first error stays)
    });
}

}  // namespace trpx
