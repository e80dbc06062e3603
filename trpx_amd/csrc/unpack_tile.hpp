// k_unpack_tiles' tile body as a device function (decode_fast.hip: one tile per workgroup; decode_seg.hip: the
// workgroup of a deferred frame loops over the frame's tiles).  Replaces Bit_range::get_range / operator T()
// (reference include/Bit_pointer.hpp:742-792, :597-617) for blocks whose widths are known.
#pragma once
#include "codec_common.hpp"
#include "unpack_common.hpp"

namespace trpx {

template <typename T> constexpr int unpack_sub_tiles() { return sizeof(T) <= 2 ? 4 : 2; }
// Pixels leave through a per-wavefront LDS row as whole 128-byte lines (store_group) for every pixel type: lane-owned 8..24-byte
// runs leave each line to be merged from several store instructions in L2, and under load the lines are written back half
// merged (decode_frame.hip).  2000 x 512 x 512 u16 with the decode index: 0.327 ms direct, 0.291 ms staged (five instead of six
// workgroups per CU for the rows); eight 4096 x 4096 int32 frames: 0.29 -> 0.12 ms.
// (rows at a stride of one group behind one head room: store_group_lines reads up to 127 bytes in front of a row and uses only
// what lies inside the row when no group continues another, as here -- the bytes in front may be the neighbour's)
template <typename T> constexpr int unpack_stage_row_dwords() { return kWave * kBlock * (int)sizeof(T) / 4; }
template <typename T> constexpr int unpack_stage_dwords() { return 4 * unpack_stage_row_dwords<T>() + kStageCarryDw; }
template <typename T>
constexpr int unpack_image_dwords() { return unpack_sub_tiles<T>() * ((kThreads * max_block_bits<T>() + 31) / 32) + 12; }

// ---- the tile rule, once: how the blocks of a tile (kSub groups of 256 blocks, block = group * 256 + thread) of one frame
// become pixels.  k_unpack_tiles / the deferred frames (unpack_tile below) and the summing decode (decode_sum.hip, which
// pipelines the same steps across frames) are assembled from these pieces; all 256 threads of a workgroup call each.
// (Plain arrays and references, no struct of them: the callers keep the registers they had with the rule written out.)

// the lanes' widths and the widths in front of them, for a caller that loads them ahead of the scan
template <int kSub>
__device__ __forceinline__ void tile_load_widths(uint32_t (&w)[kSub], uint32_t (&wp)[kSub], const uint8_t* __restrict__ wf,
                                                 const FrameGeom& g, uint32_t t) {
#pragma unroll
    for (int r = 0; r < kSub; ++r) {
        const uint32_t b = t * kSub * kThreads + r * kThreads + threadIdx.x;
        w[r] = 0; wp[r] = 0;
        if (b < g.n_blocks) {
            w[r] = wf[b];
            wp[r] = b ? wf[b - 1] : 0u;                     // significant_bits = 0 at frame start (Terse.hpp:359)
        }
    }
}
// ... and for one that loads them in the scan: tile_scan's `widths`
struct TileWidthsOf {
    const uint8_t* __restrict__ wf;                         // the frame's widths
    __device__ __forceinline__ void operator()(int, uint32_t b, uint32_t& w, uint32_t& w_prev) const {
        w = wf[b];
        w_prev = b ? wf[b - 1] : 0u;                        // significant_bits = 0 at frame start (Terse.hpp:359)
    }
};

// widths -> lengths -> bit offsets inside the tile.  Per round r: the lane's block's width w, header length hl, values nb
// (0: behind the frame's last) and tile-relative bit off; tile_bits: the tile's bits.  widths(r, b, w, w_prev) gives the
// width of block b (the lane's of round r) and the one in front.  s_wtot: 4 * kSub dwords of LDS (one __syncthreads).
template <int kSub, class Widths>
__device__ __forceinline__ void tile_scan(uint32_t (&w)[kSub], uint32_t (&hl)[kSub], uint32_t (&off)[kSub], int (&nb)[kSub], uint32_t& tile_bits,
                                          Widths&& widths, const FrameGeom& g, uint32_t t, uint32_t* __restrict__ s_wtot, int lane, int wave) {
    const uint32_t b0 = t * kSub * kThreads;
    const uint32_t tid = threadIdx.x;
    uint32_t len[kSub], inc[kSub];
#pragma unroll
    for (int r = 0; r < kSub; ++r) {
        const uint32_t b = b0 + r * kThreads + tid;
        nb[r] = 0; w[r] = 0; hl[r] = 0;
        if (b < g.n_blocks) {
            uint32_t w_prev;
            widths(r, b, w[r], w_prev);
            const uint64_t first = (uint64_t)b * kBlock;
            nb[r] = first + kBlock <= g.n_values ? kBlock : (int)(g.n_values - first);
            hl[r] = header_len(w[r], w_prev);
        }
        len[r] = nb[r] ? hl[r] + (uint32_t)nb[r] * w[r] : 0u;
        inc[r] = wave_inclusive_scan(len[r]);
        if (lane == 63) s_wtot[r * 4 + wave] = inc[r];
    }
    __syncthreads();
    // every wave: exclusive scan of the 4 * kSub (round, wave) piece sizes
    const uint32_t tot = lane < kSub * 4 ? s_wtot[lane] : 0u;
    const uint32_t incl = wave_inclusive_scan(tot);
    const uint32_t excl = incl - tot;
#pragma unroll
    for (int r = 0; r < kSub; ++r) off[r] = (uint32_t)__shfl((int)excl, r * 4 + wave, 64) + inc[r] - len[r];
    tile_bits = (uint32_t)__builtin_amdgcn_readlane((int)incl, kSub * 4 - 1);
}

// The tile against its frame: frame bytes [fo, fe) of the stream, the tile tile_bits bits from frame bit t_off on (the index
// records every 256 blocks).  False: chain / index inconsistent with the frame (the caller sets the status).  Else the tile's
// window, its stream bits in a 16-byte aligned LDS image: a0 the stream bit of the tile's first, d_lo the stream dword of the
// image's first, n_dw the image's dwords.
__device__ __forceinline__ bool tile_window(uint64_t fo, uint64_t fe, uint64_t t_off, uint32_t tile_bits, uint64_t terse_bytes,
                                            uint64_t& a0, uint64_t& d_lo, uint32_t& n_dw) {
    if (fe > terse_bytes || fe <= fo || t_off > 8 * (fe - fo) || tile_bits > 8 * (fe - fo) - t_off) return false;
    a0 = 8 * fo + t_off;
    d_lo = (a0 >> 5) & ~3ull;                               // 16-byte aligned start (terse is 4-byte aligned: use dwords)
    n_dw = (uint32_t)(((a0 + tile_bits + 31) >> 5) - d_lo) + 1;   // + 1: alignbit peeks one dword further
    return true;
}
// image bit of the tile's first bit (< 128)
__device__ __forceinline__ uint32_t tile_img_bit0(uint64_t a0, uint64_t d_lo) { return (uint32_t)(a0 - 32 * d_lo); }
// lane-owned piece i (dwords i .. i + 3, i < n_dw) of the window, from the stream
__device__ __forceinline__ uint4 tile_fetch16(uint64_t d_lo, uint32_t i, const uint8_t* __restrict__ terse, uint64_t terse_bytes) {
    return load_stream16(reinterpret_cast<const uint32_t*>(terse), d_lo + i, (terse_bytes + 3) / 4, ((uintptr_t)terse & 15) == 0);
}

// One round, full blocks: a lane's block (width w, nb values, payload from image bit q on) from the LDS image into u, with
// code specialised on the width, one width of the wavefront at a time; u stays zero for every other lane (width 0, the
// frame's last, partial block, no block).  A width above the type's (tile_too_wide) is read as the type's: the values are then
// not the stream's, and the caller gives the verdict.
template <typename T> __device__ __forceinline__ bool tile_too_wide(uint32_t w) { return w > (uint32_t)PixelTraits<T>::bits; }
template <typename T>
__device__ __forceinline__ void tile_extract_full(uint32_t (&u)[kBlock], const uint32_t* __restrict__ s_image, uint32_t q, uint32_t w, int nb) {
    constexpr uint32_t bits = (uint32_t)PixelTraits<T>::bits;
#pragma unroll
    for (int k = 0; k < kBlock; ++k) u[k] = 0u;             // w == 0 -> zeros (Terse.hpp:373-374)
    uint64_t todo = __ballot(nb == kBlock && w != 0u);
    while (todo) {
        const int l0 = __builtin_ctzll(todo);
        const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)w, l0);
        const bool mine = nb == kBlock && w == w0;
        uint32_t wd = w0 > bits ? bits : w0;
        asm volatile("" : "+s"(wd));                        // (a copy the compiler cannot equate with the lanes' own width: the dispatch stays scalar)
        uint32_t qq = q;
        asm volatile("" : "+v"(qq));                        // keep the specialised bodies out of LICM's reach
        if (mine) UnpackDispatch<T, 1, PixelTraits<T>::bits>::run(s_image, qq, wd, u);
        todo &= ~__ballot(mine);
    }
}
// The frame's last, partial block is read field by field, a width above the type's as width 0 (zeros): the width to read
// with, and the field of ww (1 .. bits) bits at image bit p as the pixel type's value in 32 bits (mask = field_mask(ww)).
// (stream_field of codec_common.hpp over a loader of the image reads the same field; in k_sum_tiles' unrolled loop that form
// cost the 32-bit kernels about 10 VGPRs, so the LDS image, the one hot site, has this reader of its own.)
template <typename T> __device__ __forceinline__ uint32_t tile_partial_width(uint32_t w) { return tile_too_wide<T>(w) ? 0u : w; }
template <typename T>
__device__ __forceinline__ uint32_t tile_partial_field(const uint32_t* __restrict__ s_image, uint32_t p, uint32_t ww, uint32_t mask) {
    const uint64_t two = (uint64_t)s_image[p >> 5] | ((uint64_t)s_image[(p >> 5) + 1] << 32);
    uint32_t f = (uint32_t)(two >> (p & 31u)) & mask;
    if (PixelTraits<T>::is_signed) f = (uint32_t)((int32_t)(f << (32u - ww)) >> (32u - ww));
    return f;
}

// One tile of one frame through the pieces, and its pixels stored.  s_image / s_wtot / s_stage are the workgroup's LDS
// (unpack_image_dwords<T>(), 4 * unpack_sub_tiles<T>() and unpack_stage_dwords<T>() dwords; s_stage: one row of 64 blocks per
// wavefront, through which a wavefront's pixels leave as whole 16-byte-per-lane stores).  Returns false when the index does not
// fit the frame (status set).
template <typename T>
__device__ __forceinline__ bool unpack_tile(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                            const uint64_t* __restrict__ frame_offsets, const FrameGeom& g, uint32_t frame,
                                            uint32_t t, const uint8_t* __restrict__ widths,
                                            const uint64_t* __restrict__ tile_off, T* __restrict__ pixels_out,
                                            uint32_t* __restrict__ status, uint32_t* __restrict__ s_image,
                                            uint32_t* __restrict__ s_wtot, uint32_t* __restrict__ s_stage) {
    constexpr int kSub = unpack_sub_tiles<T>();
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id(), wave = wave_id();
    const uint32_t b0 = t * kSub * kThreads;
    uint32_t w[kSub], hl[kSub], off[kSub], tile_bits;
    int nb[kSub];
    tile_scan<kSub>(w, hl, off, nb, tile_bits, TileWidthsOf{widths + (uint64_t)frame * g.n_blocks}, g, t, s_wtot, lane, wave);
    // (tile_window's rule, written out: through the piece the deferred frames' kernel, whose loop this body sits in, holds 4 more SGPRs)
    const uint64_t fo = frame_offsets[frame], fe = frame_offsets[frame + 1];
    const uint64_t t_off = tile_off[(uint64_t)frame * g.n_tiles + (uint64_t)t * kSub];   // walk records every 256 blocks
    if (fe > terse_bytes || fe <= fo || t_off > 8 * (fe - fo) || tile_bits > 8 * (fe - fo) - t_off) {
        if (tid == 0) atomicMax(&status[0], kStatusCorrupt);
        return false;
    }
    const uint64_t a0 = 8 * fo + t_off;
    const uint64_t d_lo = (a0 >> 5) & ~3ull;
    const uint32_t n_dw = (uint32_t)(((a0 + tile_bits + 31) >> 5) - d_lo) + 1;
    // ---- stage the tile's stream bits [a0, a0 + tile_bits) in LDS, 16 bytes per lane, coalesced ----------
    for (uint32_t i = tid * 4; i < n_dw; i += kThreads * 4) *reinterpret_cast<uint4*>(&s_image[i]) = tile_fetch16(d_lo, i, terse, terse_bytes);
    __syncthreads();
    const uint32_t img_bit0 = tile_img_bit0(a0, d_lo);

    // ---- extract + store ----------------------------------------------------------------------------------
    T* __restrict__ fout = pixels_out + (uint64_t)frame * g.n_values;
#pragma unroll
    for (int r = 0; r < kSub; ++r) {
        const uint32_t b = b0 + r * kThreads + tid;
        const uint32_t q = img_bit0 + off[r] + hl[r];       // first payload bit in the image
        // The layout comes from the widths alone: the "same width" bit must stand exactly where header_len counted one bit.  A
        // restated width (an explicit header of the width before: valid, codec_common.hpp) shows here -- up to the tile's first
        // one the positions are the true ones -- and the tile's pixels would be another stream's.
        if (nb[r] && ((s_image[(q - hl[r]) >> 5] >> ((q - hl[r]) & 31u)) & 1u) != (hl[r] == 1u ? 1u : 0u)) atomicMax(&status[0], kStatusCorrupt);
        uint32_t u[kBlock];
        tile_extract_full<T>(u, s_image, q, w[r], nb[r]);
        if (__ballot(nb[r] == kBlock) == ~0ull) {   // the wavefront's 64 blocks are all full: staged, coalesced stores
            if (tile_too_wide<T>(w[r])) atomicMax(&status[0], kStatusCorrupt);
            uint32_t* const st = s_stage + kStageCarryDw + wave * unpack_stage_row_dwords<T>();
            T* const gdst = fout + (uint64_t)(b - (uint32_t)lane) * kBlock;
            stage_block<T>(st + lane * (kBlock * (int)sizeof(T) / 4), u);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            store_group<T, false>(st, gdst);                                  // (from the group's first pixel, wherever in a line it lies: store_group_lines)
            __builtin_amdgcn_wave_barrier();                // (the row is rewritten in the next round)
        } else if (nb[r] == kBlock) {
            if (tile_too_wide<T>(w[r])) atomicMax(&status[0], kStatusCorrupt);
            store_block<T>(fout + (uint64_t)b * kBlock, u);
        } else if (nb[r]) {                               // the frame's last, partial block
            const uint32_t ww = tile_partial_width<T>(w[r]), mask = field_mask(ww);
            uint32_t p = q;
            for (int k = 0; k < nb[r]; ++k) {
                fout[(uint64_t)b * kBlock + k] = (T)(ww ? tile_partial_field<T>(s_image, p, ww, mask) : 0u);
                p += ww;
            }
        }
    }
    return true;
}

}  // namespace trpx
