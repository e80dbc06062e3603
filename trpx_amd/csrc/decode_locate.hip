// Frame locator for stacks without an index (a .trpx file stores none, Terse.hpp:454-474): frame_offsets[0 .. n_frames] of
// the stack, stream-ordered on the caller's device copy (trpx_locate_frames).  The frames are walked one after another by one
// wavefront (walk_serial.hpp: the run-skipping header walk of Terse.hpp:360-372, count only -- no per-block width stores, so
// nothing in the workspace scales with n_frames x blocks); the next frame starts at 1 + bits/8 (Terse.hpp:547).
// It reports TRPX_ERR_CORRUPT where k_walk_serial does: a chain past terse_bytes, a width above max_w, fewer frames than asked.
#include "codec_common.hpp"
#include "encode_kernels.hpp"
#include "walk_serial.hpp"

namespace trpx {

namespace {

__global__ __launch_bounds__(kWave) void k_locate_serial(const uint8_t* __restrict__ terse, uint64_t terse_bytes, uint32_t n_frames,
                                                         FrameGeom g, uint32_t max_w, uint64_t* __restrict__ offsets,
                                                         uint32_t* __restrict__ status) {
    uint64_t fo = 0;
    bool ok = true;
    if (lane_id() == 0) offsets[0] = 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
        uint64_t bits = ~0ull;
        if (ok && fo < terse_bytes)
            bits = walk_frame<false>(reinterpret_cast<const uint32_t*>(terse), (terse_bytes + 3) / 4, 8 * fo,
                                     8 * (terse_bytes - fo), g, max_w, nullptr, nullptr);
        if (bits == ~0ull) { ok = false; bits = 0; }
        fo += ok ? 1 + bits / 8 : 0;
        if (lane_id() == 0) offsets[f + 1] = fo;
    }
    if (lane_id() == 0 && !ok) atomicMax(&status[0], 5u);                  // TRPX_ERR_CORRUPT
}

}  // namespace

size_t locate_workspace_bytes(const FrameGeom&, uint64_t) { return 256; }

hipError_t launch_locate(const uint8_t* terse, uint64_t terse_bytes, const FrameGeom& g, uint32_t n_frames, uint32_t max_w,
                         uint64_t* offsets, uint32_t* status, void*, hipStream_t st) {
    zero_status(status, st);
    hipLaunchKernelGGL(k_locate_serial, dim3(1), dim3(kWave), 0, st, terse, terse_bytes, n_frames, g, max_w, offsets, status);
    return hipGetLastError();
}

}  // namespace trpx
