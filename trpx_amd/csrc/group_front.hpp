// The 256-block group on ONE wavefront, as the kernels that read the stream through the decode index without expanding frames
// see it (decode_roi.hip: trpx_decode_roi, decode_sparse.hip: trpx_decode_sparse): four blocks per lane (block = group * 256 +
// r * 64 + lane), the widths and the width in front -> header_len + 12 * w -> wave scans from the group's offset -> the group
// validated against its frame and the next group's offset -> the payload of chosen blocks straight from the stream into registers
// and through the width-specialised register extraction of unpack_common.hpp.
#pragma once
#include "codec_common.hpp"
#include "unpack_common.hpp"

namespace trpx {

constexpr int kGroupRows = kTileBlocks / kWave;             // blocks per lane

__device__ __forceinline__ uint32_t group_pick(const uint32_t (&v)[kGroupRows], int r) {   // (for loops that stay rolled: one copy of the width dispatch)
    return r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3];
}

// value k of a block's packed pixels (unpack_regs_w's layout)
template <typename T>
__device__ __forceinline__ T packed_value(const uint32_t (&o)[PackedDwords<T>::n], int k) {
    if constexpr (sizeof(T) == 4) return (T)o[k];
    else if constexpr (sizeof(T) == 2) return (T)(o[k >> 1] >> (16 * (k & 1)));
    else return (T)(o[k >> 2] >> (8 * (k & 3)));
}

// The widths of group grp of a frame (wf: the frame's widths): per row r the lane's block's width w and its values nb (0: behind
// the frame's last block); wp0: for lane 0 the width in front of its block (the other lanes take their neighbour's).  Loads
// only: a caller may have the next group's in flight while it works on this one.
__device__ __forceinline__ void group_load_widths(uint32_t (&w)[kGroupRows], uint32_t (&nb)[kGroupRows], uint32_t (&wp0)[kGroupRows],
                                                  const uint8_t* __restrict__ wf, const FrameGeom& g, uint32_t grp, uint32_t lane) {
#pragma unroll
    for (int r = 0; r < kGroupRows; ++r) {
        const uint32_t b = grp * kTileBlocks + r * kWave + lane;
        w[r] = 0; nb[r] = 0; wp0[r] = 0;
        if (b < g.n_blocks) {
            w[r] = wf[b];
            if (lane == 0) wp0[r] = b ? wf[b - 1] : 0u;     // significant_bits = 0 at frame start (Terse.hpp:359)
            const uint64_t first = (uint64_t)b * kBlock;
            nb[r] = first + kBlock <= g.n_values ? kBlock : (uint32_t)(g.n_values - first);
        }
    }
}

// widths -> header_len + 12 * w -> wave scans: off, the block's first PAYLOAD bit relative to the group's first bit.  Then the
// group against its frame (bytes [fo, fe) of the stream), its offset t_off and the next group's t_next (last: the frame's last
// group, which ends with the frame instead).  False: the group does not end where it should, a block is wider than the type, or
// something lies outside the frame or the stream.  All 64 lanes call it.
template <typename T>
__device__ __forceinline__ bool group_offsets(uint32_t (&off)[kGroupRows], const uint32_t (&w)[kGroupRows], const uint32_t (&nb)[kGroupRows],
                                              const uint32_t (&wp0)[kGroupRows], uint64_t fo, uint64_t fe, uint64_t t_off, uint64_t t_next,
                                              bool last, uint64_t terse_bytes, uint32_t lane) {
    constexpr uint32_t bits = (uint32_t)PixelTraits<T>::bits;
    uint32_t total = 0;
    bool wide = false;
#pragma unroll
    for (int r = 0; r < kGroupRows; ++r) {
        const uint32_t left = (uint32_t)__shfl_up((int)w[r], 1, kWave);   // the width in front: the neighbour lane's, one more byte for lane 0
        const uint32_t wp = lane != 0 ? left : wp0[r];
        const uint32_t hl = header_len(w[r], wp);
        const uint32_t len = nb[r] ? hl + nb[r] * w[r] : 0u;
        const uint32_t inc = wave_inclusive_scan(len);
        off[r] = total + inc - len + hl;
        total += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        wide = wide || (nb[r] && w[r] > bits);
    }
    // ---- the group against the frame and the next group
    const uint64_t frame_bits = 8 * (fe - fo);
    bool bad = __ballot(wide) != 0ull || fe > terse_bytes || fe <= fo || frame_bits >= 0xFFFF0000ull ||
               t_off > frame_bits || total > frame_bits - t_off;
    const uint64_t end = t_off + total;
    bad = bad || (last ? 1 + end / 8 != fe - fo : end != t_next);   // S_f = 1 + bits / 8 (Terse.hpp:547)
    return !bad;
}

// Group grp of frame `frame` of the stack a, both steps: w, nb, off as above; fo = the frame's first byte, t_off = the
// group's first bit in the frame.  False: the caller gives the verdict.  All 64 lanes call it.
template <typename T>
__device__ __forceinline__ bool group_front(uint32_t (&w)[kGroupRows], uint32_t (&off)[kGroupRows], uint32_t (&nb)[kGroupRows],
                                            uint64_t& fo, uint64_t& t_off, const IndexedStack& a, uint64_t frame, uint32_t grp,
                                            uint32_t lane) {
    const FrameGeom& g = a.geom;
    const uint64_t ti = frame * g.n_tiles + grp;
    const bool last = grp + 1 == g.n_tiles;
    fo = a.frame_offsets[frame];
    const uint64_t fe = a.frame_offsets[frame + 1];
    t_off = a.tile_off[ti];
    const uint64_t t_next = last ? 0 : a.tile_off[ti + 1];
    uint32_t wp0[kGroupRows];
    group_load_widths(w, nb, wp0, a.widths + frame * g.n_blocks, g, grp, lane);
    return group_offsets<T>(off, w, nb, wp0, fo, fe, t_off, t_next, last, a.terse_bytes, lane);
}

// Where a validated group's payload is read from: the dwords of the stream from the frame's first on (terse is 4-byte aligned).
struct GroupStream {
    const uint32_t* __restrict__ s32;                       // the dword that holds the frame's first byte
    uint64_t avail_dw;                                      // dwords of the stream from there on: what lies behind reads as zero
    uint32_t bit0;                                          // the group's first bit, counted from s32
};
__device__ __forceinline__ GroupStream group_stream(const uint8_t* __restrict__ terse, uint64_t terse_bytes, uint64_t fo, uint64_t t_off) {
    const uint64_t d_frame = fo >> 2;
    return {reinterpret_cast<const uint32_t*>(terse) + d_frame, (terse_bytes + 3) / 4 - d_frame, 8u * (uint32_t)(fo & 3u) + (uint32_t)t_off};
}

// The blocks of one row whose lanes say `want`: the payload dwords straight from the stream into registers, then the register
// extraction once per distinct width among them.  o: the block's 12 pixels packed to the pixel type (zeros for width 0 and for
// the lanes that did not want theirs); wr / nr / offr: the lane's width, values and payload bit of that row.  All 64 lanes call it.
template <typename T>
__device__ __forceinline__ void group_extract(uint32_t (&o)[PackedDwords<T>::n], const GroupStream& gs, bool want, uint32_t wr, uint32_t nr,
                                              uint32_t offr) {
    constexpr int kRaw = 4 * RawQuads<T>::n;
    const uint32_t q = gs.bit0 + offr, d = q >> 5, s = q & 31u;
    const uint32_t nd = (s + nr * wr + 31u) >> 5;           // dwords that hold the block's fields
    uint32_t raw[kRaw];
#pragma unroll
    for (int j = 0; j < kRaw; ++j) raw[j] = want && (uint32_t)j < nd && (uint64_t)d + j < gs.avail_dw ? gs.s32[d + j] : 0u;
#pragma unroll
    for (int j = 0; j < PackedDwords<T>::n; ++j) o[j] = 0u; // w == 0 -> zeros (Terse.hpp:373-374)
    uint64_t todo = __ballot(want && wr != 0u);
    while (todo) {
        const int l0 = __builtin_ctzll(todo);
        uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)wr, l0);
        const bool mine = want && wr == w0;
        asm volatile("" : "+s"(w0));                        // (the dispatch stays scalar)
        if (mine) UnpackRegsDispatch<T, 1, PixelTraits<T>::bits>::run(raw, s, w0, o);
        todo &= ~__ballot(mine);
    }
}

}  // namespace trpx
