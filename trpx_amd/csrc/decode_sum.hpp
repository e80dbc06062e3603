// Host-visible interface of decode_sum.hip (trpx_decode_sum): sums of consecutive frames straight from the stream and its
// decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"
#include "put_sum.hpp"

namespace trpx {

// (the output element codes kSumU32 .. kSumPart64 and the conversion: put_sum.hpp)
// Few outputs: each group's frames are split into chunks until about this many workgroups run (about four per CU).
constexpr uint64_t kSumTargetUnits = 1024;
constexpr uint32_t kSumSubTiles = 2;                 // 256-block groups per tile

// Launch geometry, decided on the host from the geometry alone: tiles per frame (k_unpack_tiles' tiles), outputs, frame chunks
// per output and frames per chunk; partial_bytes = the chunks' slab in the workspace (0: one chunk, the sums are written directly).
struct SumPlan {
    uint32_t tpf, chunks, fpc;
    uint64_t n_out;
    size_t partial_bytes;
};
SumPlan sum_plan(int dtype, const FrameGeom& g, uint64_t n_frames, uint64_t group);

// (the fields of IndexedStack in an order of its own, filled by set_stack: with the view as a base class k_sum_tiles' argument
// loads moved and every call took 1 % longer, LABNOTES.md 15)
struct SumArgs {
    const uint8_t*  terse;
    uint64_t        terse_bytes;
    const uint64_t* frame_offsets;  // n_frames + 1
    FrameGeom       geom;
    uint64_t        n_frames, group, n_out;
    uint32_t        tpf, chunks, fpc;
    const uint8_t*  widths;         // decode index: width of every block
    const uint64_t* tile_off;       // decode index: frame-relative bit offset of every 256-block group
    void*           out;            // [n_out][n_values] of out_code
    int             out_code;
    void*           partial;        // chunks > 1: [chunks][n_out][n_values] raw accumulators (u32 / u64), else null
    uint32_t*       status;
};
// k_sum_tiles (+ k_sum_reduce when split); clear_status: zero the status block first
hipError_t launch_decode_sum(int dtype, const SumArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
