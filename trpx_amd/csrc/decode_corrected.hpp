// Host-visible interface of decode_corrected.hip (trpx_decode_corrected): a stack with its decode index -> every frame as float32
// with the dark reference subtracted and the gain reference multiplied in (correct_px.hpp: the rule).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "codec_common.hpp"
#include "correct_px.hpp"

namespace trpx {

struct CorrectedArgs : IndexedStack {
    const float*    dark;           // [n_values] or null: no subtraction
    const float*    gain;           // [n_values] or null: no multiplication
    float*          out;            // [n_frames][n_values]
    uint32_t*       status;
};
// k_decode_corrected, a workgroup per tile of k_unpack_tiles' geometry; clear_status: zero the status block first
hipError_t launch_decode_corrected(int dtype, const CorrectedArgs& a, bool clear_status, hipStream_t st);

}  // namespace trpx
