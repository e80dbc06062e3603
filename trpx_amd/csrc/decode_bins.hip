// Per-frame sums over labelled pixel bins (trpx_decode_bins): a stack with its decode index and ONE map of uint16 labels ->
// bins[f][b] = sum over the pixels p of frame f with labels[p] == b of px[f][p] in int64, without expanding the frames: the radial
// profile / azimuthal integration of every frame, whatever the number of bins.  The shape is support -> spans -> (reduce); the
// front end is decode_dot.hip's (group_front.hpp, group_runs.hpp), the consumer is a histogram-by-label in LDS.
//
//   k_bins_support  one bit per block of a frame: some label of the block's <= 12 pixels is a bin (< n_bins).  In every call: the
//                   map is device data that a graph replay may have changed.
//   k_bins_spans    a workgroup per SPAN: consecutive runs (kRun groups each) of one frame, its four wavefronts taking the runs in
//                   turn.  The workgroup keeps uint64 sums[n_bins] in dynamic LDS (sized by n_bins: few bins do not cost
//                   occupancy), zeroed first.  A wavefront walks its run as k_dot_runs does: widths -> header_len + 12 * w ->
//                   wave scans from the group's offset -> the group validated, unconditionally (so the whole stack is) -> the
//                   CANDIDATE blocks, those with a width and their support bit, compacted into consecutive lanes through the list
//                   in LDS -> per 64 candidates one round: the payload dwords into registers, the register extraction, the
//                   block's 12 labels (bytes 24 * block of the map: three 8-byte loads), and bins_merge.hpp: neighbouring values
//                   of equal label summed in registers, one 64-bit LDS atomic add (ds_add_u64) per label change, none for a zero
//                   sum or a label that is no bin.  Behind a barrier the workgroup stores its n_bins sums with plain coalesced
//                   stores: to bins_out where a frame is one span, to partials[frame][span][bin] otherwise.  A group that fails
//                   validation sets CORRUPT and adds nothing.
//   k_bins_reduce   only with more than one span per frame: per (frame, bin) the spans' partial sums, added in span order.
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
    const FrameGeom& g = a.geom;
    const uint32_t lane = (uint32_t)lane_id();
    Run R = run_place(a, run, runs_per_frame);
    run_load(R, a, lane);
    uint32_t wn[kGroupRows], nbn[kGroupRows], wp0n[kGroupRows], sn[kGroupRows];
    group_load_widths(wn, nbn, wp0n, R.wf, g, R.g0, lane);
    group_load_support(sn, a.support, n_words, R.g0, lane);
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
            if (nr != 0u) {                                 // (nr values from pixel 12 * block on: nothing behind labels[n_values) is read)
                const BinsLabels l = bins_load_labels(a.labels, (uint64_t)block * kBlock, nr, aligned8);
                bins_merge(nr, [&](int i) { return bins_value<T>(o, i); }, l, a.n_bins,
                           [&](uint32_t bin, uint64_t s) { atomicAdd(&sums[bin], (unsigned long long)s); });
            }
        }
        list_sync();                                        // (the next group rewrites the list)
    }
    if (bad && lane == 0) atomicMax(&a.status[0], kStatusCorrupt);
}

}  // namespace

// bit b of the support words: some label of block b (pixels 12 b .. 12 b + 11 of a frame, as far as the frame goes) is a bin
__global__ __launch_bounds__(kThreads) void k_bins_support(const uint16_t* __restrict__ labels, uint32_t n_bins, FrameGeom g, bool aligned8,
                                                           uint32_t* __restrict__ support) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t n_words = (uint32_t)bins_support_words(g);
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t b0 = (uint64_t)blockIdx.x * kThreads + (uint32_t)wave_id() * kWave; b0 < g.n_blocks; b0 += stride) {   // (b0: uniform)
        const uint64_t b = b0 + lane;
        bool any = false;
        if (b < g.n_blocks) {
            const uint64_t first = b * kBlock;
            const uint32_t nr = first + kBlock <= g.n_values ? (uint32_t)kBlock : (uint32_t)(g.n_values - first);
            any = bins_any_label(bins_load_labels(labels, first, nr, aligned8), n_bins);
        }
        const uint64_t ballot = __ballot(any);
        const uint32_t word = (uint32_t)(b0 >> 5);
        if (lane == 0 && word < n_words) support[word] = (uint32_t)ballot;
        if (lane == 32 && word + 1 < n_words) support[word + 1] = (uint32_t)(ballot >> 32);
    }
}

// dst: bins_out (spans == 1) or the partial sums; a unit = (frame, span), the runs [span * rpf / spans, (span + 1) * rpf / spans)
template <typename T>
__global__ __launch_bounds__(kThreads) void k_bins_spans(BinsArgs a, uint32_t runs_per_frame, bool aligned8, int64_t* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_sums[];   // [n_bins]
    __shared__ uint32_t s_list[kWavesPerWg * kTileBlocks];
    const uint64_t units = a.n_frames * a.spans;
    const uint32_t n_words = (uint32_t)bins_support_words(a.geom);
    const uint32_t wave = (uint32_t)wave_id();
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {        // (uniform: every barrier below is reached by all)
        for (uint32_t i = threadIdx.x; i < a.n_bins; i += kThreads) s_sums[i] = 0ull;
        __syncthreads();
        const uint64_t frame = unit / a.spans;
        const uint32_t span = (uint32_t)(unit - frame * a.spans);
        const uint32_t r_lo = (uint32_t)((uint64_t)span * runs_per_frame / a.spans);
        const uint32_t r_hi = (uint32_t)((uint64_t)(span + 1) * runs_per_frame / a.spans);
        for (uint32_t r = r_lo + wave; r < r_hi; r += kWavesPerWg)
            bins_run<T>(a, frame * runs_per_frame + r, runs_per_frame, n_words, aligned8, s_list + wave * kTileBlocks, s_sums);
        __syncthreads();
        int64_t* __restrict__ out = dst + unit * a.n_bins;
        for (uint32_t i = threadIdx.x; i < a.n_bins; i += kThreads) out[i] = (int64_t)s_sums[i];
        __syncthreads();                                    // (the next unit zeroes the sums)
    }
}

// per (frame, bin): the spans' partial sums in span order
__global__ __launch_bounds__(kThreads) void k_bins_reduce(const int64_t* __restrict__ partials, uint64_t n_frames, uint32_t spans,
                                                          uint32_t n_bins, int64_t* __restrict__ bins_out) {
    const uint64_t n = n_frames * n_bins;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t frame = i / n_bins;
        const uint32_t b = (uint32_t)(i - frame * n_bins);
        uint64_t s = 0;
        for (uint32_t k = 0; k < spans; ++k) s += (uint64_t)partials[(frame * spans + k) * n_bins + b];
        bins_out[i] = (int64_t)s;
    }
}

uint32_t bins_runs_per_frame(const FrameGeom& g) { return (g.n_tiles + kRun - 1) / kRun; }

uint32_t bins_spans_per_frame(const FrameGeom& g, uint64_t n_frames) {
    const uint64_t by_runs = ((uint64_t)bins_runs_per_frame(g) + kWavesPerWg - 1) / kWavesPerWg;
    const uint64_t by_frames = n_frames ? (kBinsTargetWgs + n_frames - 1) / n_frames : 1;
    return (uint32_t)std::min<uint64_t>(by_runs, std::max<uint64_t>(1, by_frames));
}

hipError_t launch_decode_bins(int dtype, const BinsArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    // launch shapes from the geometry and the number of bins alone: a workgroup per (frame, span) up to 2^20 workgroups, strided
    // units beyond; 8 * n_bins bytes of dynamic LDS
    const uint32_t rpf = bins_runs_per_frame(a.geom);
    const uint64_t units = a.n_frames * a.spans;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(units, 1u << 20);
    const uint64_t swgs = ((uint64_t)a.geom.n_blocks + kThreads - 1) / kThreads;
    const uint32_t sgrid = (uint32_t)std::min<uint64_t>(swgs, 4096);
    const uint64_t rwgs = (a.n_frames * a.n_bins + kThreads - 1) / kThreads;
    const uint32_t rgrid = (uint32_t)std::min<uint64_t>(rwgs, 4096);
    const bool aligned8 = (uintptr_t)a.labels % 8 == 0;
    int64_t* dst = a.spans > 1 ? a.partials : a.bins_out;
    return for_pixel_type(dtype, [&]<class T>() {
        hipLaunchKernelGGL(k_bins_support, dim3(sgrid), dim3(kThreads), 0, st, a.labels, a.n_bins, a.geom, aligned8, a.support);
        hipLaunchKernelGGL((k_bins_spans<T>), dim3(grid), dim3(kThreads), 8 * (size_t)a.n_bins, st, a, rpf, aligned8, dst);
        if (a.spans > 1)
            hipLaunchKernelGGL(k_bins_reduce, dim3(rgrid), dim3(kThreads), 0, st, a.partials, a.n_frames, a.spans, a.n_bins, a.bins_out);
        return hipGetLastError();                           // (one check behind the clear and the launches, as the siblings do: the first error stays)
    });
}

}  // namespace trpx
