// Host-visible interface of decode_binned.hip (trpx_decode_binned): every frame of a stack summed over bins of bin_y x bin_x
// neighbouring pixels, straight from the stream and its decode index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"
#include "binned_map.hpp"

namespace trpx {

struct BinnedArgs : IndexedStack {
    BinnedGeom geo;                 // binned_geom(): the frame as rows of pixels, the bin, the output's sides
    BinnedPlan plan;                // binned_plan(): output rows per band, bands per frame
    void*      out;                 // [n_frames][out_h][out_w] of out_code
    int        out_code;            // put_sum.hpp
    uint32_t*  status;
};
// k_binned_bands; clear_status: zero the status block first
hipError_t launch_decode_binned(int dtype, const BinnedArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
