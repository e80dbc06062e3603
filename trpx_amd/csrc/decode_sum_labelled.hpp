// Host-visible interface of decode_sum_labelled.hip (trpx_decode_sum_labelled): sums of the frames that carry the same label,
// one device label per frame, straight from the stream and its decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"
#include "decode_sum.hpp"
#include "label_runs.hpp"

namespace trpx {

// Launch geometry, decided on the host from the sizes alone: tiles per frame (sum_plan's), the chunks the ordered frames are cut
// into and the frames per chunk (label_runs.hpp), and the call's scratch behind the consumers' front:
//   [counts u32 x n_out, n_todo u32] [cursor u32 x n_out] [starts u32 x (n_out + 1)] [todo u32 x n_out]
//   [order (frame, label) x n_frames] [slab n_chunks x 2 x stride]
// 16 bytes per output, 8 per frame, and the partial slab: two runs of raw accumulators (u32 / u64) per chunk.  todo: the labels
// the merge has work for (no frames, or frames in more than one chunk), n_todo of them, in no particular order.
struct LabelledPlan {
    uint32_t tpf, n_chunks, fpc;
    uint64_t stride;                 // elements per slab slot: n_values up to whole 256-byte lines
    size_t counts, cursor, starts, todo, order, slab, total;
};
inline LabelledPlan labelled_plan(int dtype, const FrameGeom& g, uint64_t n_frames, uint64_t n_out) {
    LabelledPlan p;
    p.tpf = (g.n_blocks + kSumSubTiles * kThreads - 1) / (kSumSubTiles * kThreads);
    p.fpc = label_frames_per_chunk(n_frames, p.tpf, dtype < TRPX_U32, &p.n_chunks);
    p.stride = align_up(g.n_values, 64);
    p.counts = 0;
    p.cursor = align_up(p.counts + 4 * (n_out + 1), 8);
    p.starts = align_up(p.cursor + 4 * n_out, 8);
    p.todo = align_up(p.starts + 4 * (n_out + 1), 8);
    p.order = align_up(p.todo + 4 * n_out, 8);
    p.slab = align_up(p.order + 8 * n_frames, 256);
    p.total = p.slab + (size_t)p.n_chunks * 2 * p.stride * (dtype >= TRPX_U32 ? 8 : 4);
    return p;
}

// (SumArgs' order of the stack's fields, filled by set_stack)
struct LabelledArgs {
    const uint8_t*  terse;
    uint64_t        terse_bytes;
    const uint64_t* frame_offsets;  // n_frames + 1
    FrameGeom       geom;
    uint64_t        n_frames;
    uint32_t        n_out, tpf, n_chunks, fpc;
    const uint8_t*  widths;         // decode index: width of every block
    const uint64_t* tile_off;       // decode index: frame-relative bit offset of every 256-block group
    const uint32_t* labels;         // n_frames; >= n_out: the frame takes part in nothing
    void*           out;            // [n_out][n_values] of out_code
    int             out_code;
    uint32_t*       counts_out;     // n_out, or null
    uint32_t*       counts;         // scratch, see LabelledPlan (counts[n_out] = n_todo)
    uint32_t*       cursor;
    uint32_t*       starts;
    uint32_t*       todo;
    uint2*          order;
    void*           partial;
    uint64_t        stride;
    uint32_t*       status;
};
// the ordering (k_lab_order_small, or k_zero_words, k_lab_count, k_lab_scan, k_lab_scatter), k_sum_labelled, k_lab_merge;
// clear_status: zero the status block first
hipError_t launch_decode_sum_labelled(int dtype, const LabelledArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
