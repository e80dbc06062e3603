// Host-visible interface of decode_hist.hip (trpx_decode_hist): per group of consecutive frames the histogram of its pixel
// values, straight from the stream and its decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"
#include "hist_bin.hpp"

namespace trpx {

// SPANS PER GROUP.  A group of `group` consecutive frames is R = frames * runs_per_frame runs (a run: 8 groups of 256 blocks, one
// wavefront's piece of work); a workgroup owns a SPAN of it, span s of S the runs [s * R / S, (s + 1) * R / S) -- a span may cross
// frames.  The rule, on the geometry alone, with G = ceil(n_frames / group) groups and R that of a full group:
//
//     S = max(ceil(R / kHistMaxSpanRuns), min(ceil(R / 4), max(1, ceil(kHistTargetWgs / G))))
//
//   - kHistTargetWgs workgroups are aimed at where the groups alone give fewer: six on each of the 256 CUs, trpx_decode_bins'
//     reasoning (kBinsTargetWgs).  2000 frames of 512^2 with group = 1: G = 2000 >= 1536, S = 1 -- every workgroup stores its
//     histogram itself and nothing passes through the workspace.  The same stack with group = 2000: G = 1, R = 22000, S = 1536 -- not
//     one workgroup.
//   - no span is shorter than the four runs its four wavefronts take at once (ceil(R / 4));
//   - no span is longer than kHistMaxSpanRuns runs = 2^17 * 24576 < 2^32 values, so the 32-bit counters in LDS cannot wrap.  (Below
//     the 2^24 - 1 groups of 256 blocks one call takes the other two terms already keep a span shorter: the term states the
//     guarantee, it does not bind.)
// With S > 1 the spans' counts go to partials[G][S][n_bins] and k_reduce_parts adds them in span order.  The ragged last group
// has fewer runs and the SAME S: its spans are shorter, those without a run store zeros (padded with zero partials rather than
// a span count per group: one launch shape, one reduce).
constexpr uint32_t kHistTargetWgs = 1536;
constexpr uint64_t kHistMaxSpanRuns = 1ull << 17;

struct HistArgs : IndexedStack {
    uint64_t        group;          // frames per group (the last group: what is left)
    uint64_t        n_groups;       // ceil(n_frames / group)
    int64_t         lo;
    uint32_t        shift;
    uint32_t        n_bins;
    uint32_t        spans;          // hist_spans_per_group(): workgroups per group
    uint64_t*       partials;       // workspace, [n_groups][spans][n_bins] (spans > 1 only)
    uint64_t*       hist_out;       // [n_groups][n_bins]
    uint32_t*       status;
};
// the rule above: arithmetic on the geometry (group: clamped to n_frames)
uint32_t hist_spans_per_group(const FrameGeom& g, uint64_t n_frames, uint64_t group);
// k_hist_spans, k_reduce_parts (spans > 1); clear_status: zero the status block first
hipError_t launch_decode_hist(int dtype, const HistArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
