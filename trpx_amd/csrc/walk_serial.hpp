// The serial header walk of one frame (Terse.hpp:360-372) with one wavefront, shared by decode.hip (k_walk, k_walk_serial)
// and decode_locate.hip (k_locate_serial, the count-only form).
#pragma once
#include "codec_common.hpp"

namespace trpx {

// 32 bits of the stream starting at absolute bit `abit` of the (4-byte aligned) buffer (ld_stream_dw: codec_common.hpp).
__device__ __forceinline__ uint32_t peek32(const uint32_t* __restrict__ s32, uint64_t n_dw, uint64_t abit) {
    return (uint32_t)stream_bits([&](uint64_t i) { return ld_stream_dw(s32, i, n_dw); }, abit);
}

// Walk one frame with one wavefront (kStore = false: count only, widths_f / tile_off_f are not touched).  A restated width (an
// explicit header of the width before, codec_common.hpp) is stored with kWidthRestated set: header_len_flagged.  Returns the frame's total bit count, or ~0ull if the
// chain runs past `limit_bits` or a width exceeds `max_w` (corrupt stream).
template <bool kStore = true>
__device__ uint64_t walk_frame(const uint32_t* __restrict__ s32, uint64_t n_dw, uint64_t frame_abit,
                               uint64_t limit_bits, const FrameGeom g, uint32_t max_w,
                               uint8_t* __restrict__ widths_f, uint64_t* __restrict__ tile_off_f) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t nb_last = (uint32_t)(g.n_values - (uint64_t)(g.n_blocks - 1) * g.block);
    uint32_t b = 0, w_prev = 0;
    uint64_t pos = 0;
    uint64_t final_pos = 0;
    bool bad = false;
    while (b < g.n_blocks) {
        const uint32_t stride = 1u + g.block * w_prev;
        const uint32_t cb = b + lane;
        const uint64_t cpos = pos + (uint64_t)lane * stride;
        const bool in_range = cb < g.n_blocks;
        const bool readable = in_range && cpos < limit_bits;
        const uint32_t bits = readable ? peek32(s32, n_dw, frame_abit + cpos) : 0u;
        const bool same = readable && (bits & 1u);                       // Terse.hpp:361
        const uint64_t not_same = __ballot(!same);
        const uint32_t first = not_same ? (uint32_t)__builtin_ctzll(not_same) : 64u;

        if constexpr (kStore) {
            if (lane < first) widths_f[cb] = (uint8_t)w_prev;
            if (lane <= first && in_range && (cb & (kTileBlocks - 1)) == 0) tile_off_f[cb / kTileBlocks] = cpos;
        }

        uint64_t npos = cpos;
        uint32_t nw = w_prev;
        bool lane_bad = false;
        if (lane == first && in_range) {                                 // explicit header
            if (!readable) lane_bad = true;
            auto [w, hl] = parse_explicit_header(bits);
            if (w > max_w) { lane_bad = true; w = 0; }
            const uint32_t nbv = cb + 1 == g.n_blocks ? nb_last : g.block;
            npos = cpos + hl + (uint64_t)nbv * w;
            nw = w;
            if constexpr (kStore) widths_f[cb] = (uint8_t)(w | (w == w_prev && !lane_bad ? kWidthRestated : 0u));
        }
        // position after the frame's last block (a "same" last block may be partial)
        uint64_t fin = 0;
        if (in_range && cb + 1 == g.n_blocks) {
            if (lane < first) fin = cpos + 1 + (uint64_t)nb_last * w_prev;
            else if (lane == first) fin = npos;
        }
        const uint64_t fin_mask = __ballot(fin != 0 && lane <= first);
        if (fin_mask) {
            const int src = __builtin_ctzll(fin_mask);
            final_pos = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(fin >> 32), src, 64) << 32) |
                        (uint32_t)__shfl((int)(uint32_t)fin, src, 64);
        }
        if (__ballot(lane_bad)) { bad = true; break; }
        if (first < 64u) {
            const int src = (int)first;
            pos = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(npos >> 32), src, 64) << 32) |
                  (uint32_t)__shfl((int)(uint32_t)npos, src, 64);
            w_prev = (uint32_t)__shfl((int)nw, src, 64);
            b += first + 1;
        } else {
            pos += 64ull * stride;
            b += 64;
        }
    }
    if (bad || final_pos > limit_bits || final_pos / 8 + 1 > limit_bits / 8) return ~0ull;
    return final_pos;
}

}  // namespace trpx
