// Host-visible interface of decode_sparse.hip (trpx_decode_sparse): the pixels at or above a threshold, in CSR form, straight
// from the stream and its decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"

namespace trpx {

struct SparseArgs : IndexedStack {
    int64_t         threshold;
    uint32_t        min_width;      // blocks narrower than this cannot hold an event (0: any block can)
    uint32_t*       counts;         // workspace, per (frame, group): events
    uint64_t*       flags;          // workspace, per (frame, group): 4 words, bit i of word c = candidate 64 c + i (in block order) has events
    uint32_t*       base;           // workspace, per (frame, group): events of the frame in front of the group (a frame has < 2^29 pixels)
    uint32_t*       frame_total;    // workspace, per frame: events
    uint64_t*       row_offsets;    // n_frames + 1
    uint32_t*       positions;      // capacity, or NULL (with values): sizes only
    void*           values;         // capacity elements of the stream's type
    uint64_t        capacity;
    uint32_t*       status;
};
// The narrowest block that can hold a value >= threshold in a stream of signed / unsigned fields (above the type's width: none can).
uint32_t sparse_min_width(int64_t threshold, bool stream_signed);
// k_sparse_count, k_sparse_frame_scan, k_sparse_stack_scan, k_sparse_write; clear_status: zero the status block first
hipError_t launch_decode_sparse(int dtype, const SparseArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
