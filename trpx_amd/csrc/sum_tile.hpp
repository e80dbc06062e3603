// The walk the per-pixel consumers share (decode_sum.hip: trpx_decode_sum, decode_reduce.hip: trpx_decode_reduce): one tile of one
// frame after another through unpack_tile.hpp's pieces, its steps spread over three frames -- while frame f is extracted from LDS,
// the stream dwords of frame f + 1 are in flight to registers and the widths of frame f + 2 are loaded.  What a kernel does with
// the extracted values (add, max, count, ...) is its own; the geometry is one: kSumSubTiles groups of 256 blocks per tile for
// every pixel type, 12 * kSumSubTiles values per lane.
#pragma once
#include "codec_common.hpp"
#include "decode_sum.hpp"
#include "unpack_common.hpp"
#include "unpack_tile.hpp"

namespace trpx {

// 512 blocks per tile for every pixel type (k_unpack_tiles: 1024 for 8/16-bit pixels): the accumulators stay at 24 per lane
template <typename T> constexpr int sum_sub_tiles() { return kSumSubTiles; }
template <typename T> constexpr int sum_image_dwords() { return kSumSubTiles * ((kThreads * max_block_bits<T>() + 31) / 32) + 12; }
template <typename T> constexpr int sum_stage_dwords() {   // LDS: the tile's stream image, reused for the results (4 waves x 768 x 8 B)
    return sum_image_dwords<T>() > 2 * kThreads * kBlock ? sum_image_dwords<T>() : 2 * kThreads * kBlock;
}
// stream dwords held in registers per lane while the previous frame is extracted (4 per load, all 256 lanes)
template <typename T> constexpr int sum_prefetch_loads() { return (sum_image_dwords<T>() + 4 * kThreads - 1) / (4 * kThreads); }

// The tile rule is unpack_tile.hpp's pieces; here: its steps spread over three frames.
// what a frame's tile needs before its scan: the lanes' widths and the frame / tile positions
template <typename T> struct SumPre {
    uint32_t w[sum_sub_tiles<T>()], wp[sum_sub_tiles<T>()];
    uint64_t fo, fe, t_off;
};
// ... and after it
template <typename T> struct SumCur {
    uint32_t w[sum_sub_tiles<T>()], hl[sum_sub_tiles<T>()], off[sum_sub_tiles<T>()];
    int nb[sum_sub_tiles<T>()];
    uint32_t tile_bits, n_dw, img_bit0;
    uint64_t d_lo;
};

template <typename T>
__device__ __forceinline__ void sum_load_pre(SumPre<T>& p, const uint64_t* __restrict__ frame_offsets, const FrameGeom& g,
                                             uint64_t frame, uint32_t t, const uint8_t* __restrict__ widths,
                                             const uint64_t* __restrict__ tile_off) {
    constexpr int kSub = sum_sub_tiles<T>();
    tile_load_widths<kSub>(p.w, p.wp, widths + frame * g.n_blocks, g, t);
    // vector loads (the index in a VGPR): a scalar load in flight shares lgkmcnt with LDS, and every LDS access of the frame
    // being extracted would wait for it
    uint64_t fi = frame, ti = frame * g.n_tiles + (uint64_t)t * kSub;   // (walk records every 256 blocks)
    asm volatile("" : "+v"(fi));
    asm volatile("" : "+v"(ti));
    p.fo = frame_offsets[fi];
    p.fe = frame_offsets[fi + 1];
    p.t_off = tile_off[ti];
}

// widths -> bit offsets inside the tile -> the window.  Returns false when the index does not fit the frame or the LDS image
// (uniform over the workgroup: every lane sees the same positions and totals).
template <typename T>
__device__ __forceinline__ bool sum_scan(SumCur<T>& c, const SumPre<T>& p, const FrameGeom& g, uint32_t t, uint64_t terse_bytes,
                                         uint32_t* __restrict__ s_wtot) {
    tile_scan<sum_sub_tiles<T>()>(c.w, c.hl, c.off, c.nb, c.tile_bits,
                                  [&](int r, uint32_t, uint32_t& w, uint32_t& w_prev) { w = p.w[r]; w_prev = p.wp[r]; }, g, t, s_wtot, lane_id(), wave_id());
    uint64_t a0;
    if (!tile_window(uniform64(p.fo), uniform64(p.fe), uniform64(p.t_off), c.tile_bits, terse_bytes, a0, c.d_lo, c.n_dw)) return false;
    c.img_bit0 = tile_img_bit0(a0, c.d_lo);
    return c.n_dw <= (uint32_t)(sum_image_dwords<T>() - 8);   // (widths above the type's: more bits than the image holds)
}

template <typename T>
__device__ __forceinline__ void sum_fetch(uint4 (&R)[sum_prefetch_loads<T>()], const SumCur<T>& c, const uint8_t* __restrict__ terse,
                                          uint64_t terse_bytes) {
#pragma unroll
    for (int k = 0; k < sum_prefetch_loads<T>(); ++k) {
        const uint32_t i = threadIdx.x * 4 + k * kThreads * 4;
        if (i < c.n_dw) R[k] = tile_fetch16(c.d_lo, i, terse, terse_bytes);
    }
}

template <typename T>
__device__ __forceinline__ void sum_stage(uint32_t* __restrict__ s_image, const uint4 (&R)[sum_prefetch_loads<T>()], uint32_t n_dw) {
#pragma unroll
    for (int k = 0; k < sum_prefetch_loads<T>(); ++k) {
        const uint32_t i = threadIdx.x * 4 + k * kThreads * 4;
        if (i < n_dw) *reinterpret_cast<uint4*>(&s_image[i]) = R[k];
    }
}

// The fields of the lane's block of round r from the LDS image, as the pixel type's values in 32 bits (zeros behind the
// frame's last value).  ok becomes false for a width above the type's or a header that is not where the widths put it.
// (k_sum_tiles has this text written out in its sum_extract: called from there the two checks are scheduled differently, and
// that kernel's code is to stay what it was measured as)
template <typename T>
__device__ __forceinline__ void sum_fields(uint32_t (&u)[kBlock], bool& ok, const SumCur<T>& c, int r, const uint32_t* __restrict__ s_image) {
    const uint32_t q = c.img_bit0 + c.off[r] + c.hl[r];  // first payload bit in the image
    if (c.nb[r] && tile_too_wide<T>(c.w[r])) ok = false;
    // (as unpack_tile: the "same width" bit stands exactly where header_len counted one bit, or the widths are not this
    // stream's layout -- a restated width, codec_common.hpp)
    if (c.nb[r] && ((s_image[(q - c.hl[r]) >> 5] >> ((q - c.hl[r]) & 31u)) & 1u) != (c.hl[r] == 1u ? 1u : 0u)) ok = false;
    tile_extract_full<T>(u, s_image, q, c.w[r], c.nb[r]);
    if (c.nb[r] && c.nb[r] < kBlock) {              // the frame's last, partial block (unrolled: u stays in registers)
        const uint32_t ww = tile_partial_width<T>(c.w[r]), mask = field_mask(ww);
        uint32_t p = q;
#pragma unroll
        for (int k = 0; k < kBlock; ++k) {
            if (k < c.nb[r] && ww) {
                u[k] = tile_partial_field<T>(s_image, p, ww, mask);
                p += ww;
            }
        }
    }
}

}  // namespace trpx
