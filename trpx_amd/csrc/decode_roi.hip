// Box decode (trpx_decode_roi): a stack with its decode index -> boxes of pixels, without expanding the frames.  The work unit
// is (box, 256-block group) on ONE wavefront; a box gets roi_units_per_box() units, the groups between its first and its last
// pixel at most, and the units behind its last group exit.
//
//   per unit   the box (wave-uniform) -> does any row segment of the box meet the group? (frames wider than a group: most
//              units of a box do not, and exit before loading anything) -> the group's 256 widths and the width in front of
//              it, four blocks per lane (block = group * 256 + r * 64 + lane) -> header_len + 12 * w -> wave scans from the
//              group's offset -> the group is validated: it ends where the next group's offset, or the frame's size, says, no
//              block is wider than the type, nothing lies outside the frame -> for the blocks that hold box pixels ONLY: the
//              payload dwords straight from the stream into registers, the width-specialised register extraction of
//              unpack_common.hpp, and the values inside the box stored to their place (rows of a box are short: no line images).
// Only the groups the boxes touch are read and validated.  HBM traffic: 256 widths + 2 offsets per unit, the payload of the
// box's blocks, the boxes' pixels.
#include "codec_common.hpp"
#include "decode_roi.hpp"
#include "group_front.hpp"

namespace trpx {

namespace {

template <typename T>
__device__ __forceinline__ void roi_unit(const RoiArgs& a, uint64_t unit) {
    const FrameGeom& g = a.geom;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t box = unit / a.units_per_box;
    const uint32_t k_unit = (uint32_t)(unit - box * a.units_per_box);
    const uint32_t frame = uniform32(a.boxes[3 * box]), y0 = uniform32(a.boxes[3 * box + 1]), x0 = uniform32(a.boxes[3 * box + 2]);
    const uint32_t width = a.width;
    if (frame >= a.n_frames || (uint64_t)y0 + a.box_h > a.height || (uint64_t)x0 + a.box_w > width) {
        if (k_unit == 0 && lane == 0) atomicMax(&a.status[0], kStatusInvalid);
        return;
    }
    const uint32_t y1 = y0 + a.box_h, x1 = x0 + a.box_w;
    // ---- the unit's group, and whether a row segment of the box meets it (pixel indices < n_values < 2^29)
    const uint32_t grp = (y0 * width + x0) / kTileValues + k_unit;
    if (grp > ((y1 - 1) * width + x1 - 1) / kTileValues) return;
    const uint32_t p_lo = grp * kTileValues;
    const uint32_t p_hi = (uint64_t)p_lo + kTileValues < g.n_values ? p_lo + kTileValues : (uint32_t)g.n_values;
    uint32_t ya = y0;                                       // the first row whose segment ends behind p_lo
    if (p_lo >= x1) {
        const uint32_t q = (p_lo - x1) / width + 1;
        ya = q > ya ? q : ya;
    }
    if (ya >= y1 || ya * width + x0 >= p_hi) return;

    // ---- widths -> bit offsets inside the group -> the group against the frame and the next group (group_front.hpp)
    uint32_t w[kGroupRows], off[kGroupRows], nb[kGroupRows];   // off: the block's first PAYLOAD bit, group-relative
    uint64_t fo, t_off;
    const IndexedStack stack{a.terse, a.terse_bytes, a.frame_offsets, g, a.n_frames, a.widths, a.tile_off};
    if (!group_front<T>(w, off, nb, fo, t_off, stack, frame, grp, lane)) {
        if (lane == 0) atomicMax(&a.status[0], kStatusCorrupt);
        return;
    }

    // ---- the blocks that hold box pixels: payload dwords -> registers -> fields -> the box
    const GroupStream gs = group_stream(a.terse, a.terse_bytes, fo, t_off);
    T* __restrict__ out = static_cast<T*>(a.out) + box * a.box_h * a.box_w;
#pragma unroll 1
    for (int r = 0; r < kGroupRows; ++r) {
        const uint32_t wr = group_pick(w, r), nr = group_pick(nb, r);
        const uint32_t p0 = (grp * kTileBlocks + r * kWave + lane) * kBlock;
        const uint32_t by = p0 / width, bx = p0 - by * width;
        uint32_t mask = 0;                                  // the block's values inside the box
        {
            uint32_t x = bx, y = by;
#pragma unroll
            for (int k = 0; k < kBlock; ++k) {
                if ((uint32_t)k < nr && y >= y0 && y < y1 && x >= x0 && x < x1) mask |= 1u << k;
                if (++x == width) { x = 0; ++y; }
            }
        }
        if (__ballot(mask != 0u) == 0ull) continue;
        uint32_t o[PackedDwords<T>::n];
        group_extract<T>(o, gs, mask != 0u, wr, nr, group_pick(off, r));
        {
            uint32_t x = bx, y = by;
#pragma unroll
            for (int k = 0; k < kBlock; ++k) {
                if (mask & (1u << k)) out[(uint64_t)(y - y0) * a.box_w + (x - x0)] = packed_value<T>(o, k);
                if (++x == width) { x = 0; ++y; }
            }
        }
    }
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kThreads) void k_decode_roi(RoiArgs a) {
    const uint64_t units = a.n_boxes * a.units_per_box;
    const uint64_t stride = (uint64_t)gridDim.x * (kThreads / kWave);
    for (uint64_t unit = (uint64_t)blockIdx.x * (kThreads / kWave) + (uint32_t)wave_id(); unit < units; unit += stride)
        roi_unit<T>(a, unit);
}

uint32_t roi_units_per_box(const FrameGeom& g, uint32_t width, uint32_t box_h, uint32_t box_w) {
    const uint64_t span = (uint64_t)(box_h - 1) * width + box_w;             // first to last pixel of a box
    const uint64_t units = (span + 2 * kTileValues - 2) / kTileValues + 1;   // ceil((span + 3071) / 3072) + 1
    return (uint32_t)(units < g.n_tiles ? units : g.n_tiles);
}

hipError_t launch_decode_roi(int dtype, const RoiArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    const uint64_t groups = (a.n_boxes * a.units_per_box + kThreads / kWave - 1) / (kThreads / kWave);
    const uint32_t grid = (uint32_t)(groups < (1ull << 22) ? groups : (1ull << 22));
    return for_pixel_type(dtype, [&]<class T>() {
        hipLaunchKernelGGL((k_decode_roi<T>), dim3(grid), dim3(kThreads), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace trpx
