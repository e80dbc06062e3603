// Host-visible interface of decode_roi.hip (trpx_decode_roi): boxes of pixels straight from the stream and its decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"

namespace trpx {

// Work units (wavefronts) launched per box: the 256-block groups between a box's first and last pixel, at most -- from the
// geometry alone, never from the boxes' contents; the surplus units of a box exit.
uint32_t roi_units_per_box(const FrameGeom& g, uint32_t width, uint32_t box_h, uint32_t box_w);

// (the fields of IndexedStack in an order of its own, filled by set_stack: the layout k_decode_roi was measured with, LABNOTES.md 15)
struct RoiArgs {
    const uint8_t*  terse;
    uint64_t        terse_bytes;
    const uint64_t* frame_offsets;  // n_frames + 1
    FrameGeom       geom;
    uint64_t        n_frames;
    uint32_t        width, height;  // of a frame: width * height = geom.n_values (< 2^29: frames of < 2^32 bits)
    const uint32_t* boxes;          // [n_boxes][3] = {frame, y0, x0}
    uint64_t        n_boxes;
    uint32_t        box_h, box_w, units_per_box;
    const uint8_t*  widths;         // decode index: width of every block
    const uint64_t* tile_off;       // decode index: frame-relative bit offset of every 256-block group
    void*           out;            // [n_boxes][box_h][box_w] of the stream's type
    uint32_t*       status;
};
// k_decode_roi; clear_status: zero the status block first
hipError_t launch_decode_roi(int dtype, const RoiArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
