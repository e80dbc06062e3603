// Host-visible interface of decode_dot.hip (trpx_decode_dot): per frame the sums of its pixels weighted by K integer maps,
// straight from the stream and its decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"

namespace trpx {

constexpr uint32_t kDotMaxMaps = 16;

struct DotArgs : IndexedStack {
    const int32_t*  weights;        // [n_maps][n_values]
    uint32_t        n_maps;
    uint32_t*       support;        // workspace, support_words() (group_runs.hpp): bit b = some map is non-zero on block b of a frame
    int64_t*        partials;       // workspace, [n_frames][runs_per_frame()][n_maps]
    int64_t*        dots_out;       // [n_frames][n_maps]
    uint32_t*       status;
};
// k_dot_support, k_dot_runs, k_reduce_parts; clear_status: zero the status block first
hipError_t launch_decode_dot(int dtype, const DotArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
