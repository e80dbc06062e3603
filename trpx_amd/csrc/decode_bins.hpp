// Host-visible interface of decode_bins.hip (trpx_decode_bins): per frame the sums of its pixels over the bins of a label map,
// straight from the stream and its decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"
#include "bins_merge.hpp"

namespace trpx {

// Workgroups a launch of k_bins_spans aims at where the frames alone give fewer: six on each of the 256 CUs.  (2000 x 512^2 has
// its 2000 frames and stays at one span per frame; eight 4096^2 frames are cut into 171 spans each.)
constexpr uint32_t kBinsTargetWgs = 1536;

struct BinsArgs : IndexedStack {
    const uint16_t* labels;         // [n_values]
    uint32_t        n_bins;
    uint32_t        spans;          // bins_spans_per_frame(): workgroups per frame
    uint32_t*       support;        // workspace, support_words() (group_runs.hpp): bit b = some label of block b of a frame is a bin
    int64_t*        partials;       // workspace, [n_frames][spans][n_bins] (spans > 1 only)
    int64_t*        bins_out;       // [n_frames][n_bins]
    uint32_t*       status;
};
// min(ceil(runs per frame / 4), max(1, ceil(kBinsTargetWgs / n_frames))): arithmetic on the geometry
uint32_t bins_spans_per_frame(const FrameGeom& g, uint64_t n_frames);
// k_bins_support, k_bins_spans, k_reduce_parts (spans > 1); clear_status: zero the status block first
hipError_t launch_decode_bins(int dtype, const BinsArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
