// Host-visible interface of decode_reduce.hip (trpx_decode_reduce): per-pixel max, min, sum of squares or count of frames at or
// above a threshold over groups of consecutive frames, straight from the stream and its decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"
#include "decode_sum.hpp"
#include "reduce_ops.hpp"

namespace trpx {

// The launch geometry is trpx_decode_sum's (sum_plan: tiles per frame, outputs, frame chunks per output, frames per chunk); only
// the chunks' slab differs: raw accumulators of the op (reduce_acc_size), 0 for one chunk.
inline size_t reduce_partial_bytes(const SumPlan& p, int op, const FrameGeom& g) {
    return p.chunks > 1 ? align_up((uint64_t)p.chunks * p.n_out * g.n_values * reduce_acc_size(op), 256) : 0;
}

// (SumArgs' order of the stack's fields, filled by set_stack)
struct ReduceArgs {
    const uint8_t*  terse;
    uint64_t        terse_bytes;
    const uint64_t* frame_offsets;  // n_frames + 1
    FrameGeom       geom;
    uint64_t        n_frames, group, n_out;
    uint32_t        tpf, chunks, fpc;
    const uint8_t*  widths;         // decode index: width of every block
    const uint64_t* tile_off;       // decode index: frame-relative bit offset of every 256-block group
    void*           out;            // [n_out][n_values] of the op's element (ReduceOp<T, op>::Out)
    int64_t         threshold;      // COUNT_GE
    void*           partial;        // chunks > 1: [chunks][n_out][n_values] raw accumulators (ReduceOp<T, op>::Acc), else null
    uint32_t*       status;
};
// k_reduce_tiles (+ k_reduce_merge when split); clear_status: zero the status block first
hipError_t launch_decode_reduce(int dtype, int op, const ReduceArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
