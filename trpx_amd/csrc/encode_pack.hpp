// What the two-pass encoders share (encode.hip: pixels from a dense stack; encode_sparse.hip: pixels from event lists): a
// block's width, the scans over tiles and frames, a tile's output span, and the serialisation of one block into the
// workgroup's LDS staging image.  Where a block's twelve values come from is each encoder's own.
#pragma once
#include <type_traits>

#include "codec_common.hpp"

namespace trpx {

// A block's twelve values in registers.  8-bit pixels are held in 32-bit registers, zero- or sign-extended: with `T v[12]` the
// compiler keeps twelve bytes in three VGPRs and merges every value into them (v_and_b32_sdwa ... dst_sel:BYTE_n, v_bitop3_b16),
// and k_pack<uint8_t> built that way wrote bytes that differed from run to run on stacks of a few hundred tiles and more
// (tests/test_gpu_large_stacks.py) -- the sequence that once made the basic 8-bit unpack kernel do the same (LABNOTES.md).
template <typename T>
using BlockReg = std::conditional_t<sizeof(T) == 1, std::conditional_t<PixelTraits<T>::is_signed, int32_t, uint32_t>, T>;

template <typename T>
__device__ __forceinline__ uint32_t block_width(const BlockReg<T> (&v)[kBlock]) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < kBlock; ++k) m |= magnitude<T>((T)v[k]);   // OR-scan (Terse.hpp:508-514)
    return width_from_or<T>(m);
}

// ---------------------------------------------------------------------------------------------
// K2a: per-frame exclusive scan of tile bits; frame size S_f = 1 + bits/8 (Terse.hpp:547).
// (static, like the two kernels below: every translation unit that launches it holds its own copy)
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(kThreads) void k_frame_scan(const uint32_t* __restrict__ tile_bits, FrameGeom g,
                                                         uint64_t* __restrict__ tile_off,
                                                         uint64_t* __restrict__ frame_size) {
    __shared__ uint32_t s_tot[4];
    const uint64_t frame = blockIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < g.n_tiles; base += kThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t vlen = i < g.n_tiles ? tile_bits[frame * g.n_tiles + i] : 0u;
        uint32_t total;
        const uint32_t excl = block_exclusive_scan(vlen, s_tot, &total);
        if (i < g.n_tiles) tile_off[frame * g.n_tiles + i] = carry + excl;
        carry += total;
        __syncthreads();                                    // s_tot is reused next iteration
    }
    if (threadIdx.x == 0) frame_size[frame] = 1 + carry / 8;
}

// ---------------------------------------------------------------------------------------------
// K2b: exclusive scan of frame sizes over the stack (single workgroup; F is small).
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(kThreads) void k_stack_scan(const uint64_t* __restrict__ frame_size,
                                                         uint32_t n_frames, uint64_t out_capacity,
                                                         uint64_t* __restrict__ frame_offsets,
                                                         uint32_t* __restrict__ status) {
    __shared__ uint64_t s_tot[4];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_frames; base += kThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < n_frames ? frame_size[i] : 0ull;
        const uint64_t inc = wave_inclusive_scan64(v);
        if (lane_id() == 63) s_tot[wave_id()] = inc;
        __syncthreads();
        uint64_t wbase = 0;
        for (int k = 0; k < wave_id(); ++k) wbase += s_tot[k];
        if (i < n_frames) frame_offsets[i] = carry + wbase + inc - v;
        carry += s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        frame_offsets[n_frames] = carry;
        // dword-granular stores may touch up to 3 zero bytes past the stack's end
        if (align_up(carry, 4) > out_capacity) status[0] = 3u;   // TRPX_ERR_CAPACITY
    }
}

// ---------------------------------------------------------------------------------------------
// Output span of a tile in units of output dwords.
// ---------------------------------------------------------------------------------------------
struct Span {
    uint64_t d0;       // first output dword touched
    uint32_t s0;       // bit position of the tile's first bit inside dword d0
    uint32_t nbits;    // bits covered (the frame's last tile also covers the pad byte, Terse.hpp:547)
    uint32_t ndw;      // dwords touched
    bool first_partial, last_partial;
};

__device__ __forceinline__ Span tile_span(uint64_t frame_off, uint64_t frame_end, uint64_t t_off,
                                          uint32_t t_bits, bool last_tile) {
    Span s;
    const uint64_t p = 8 * frame_off + t_off;
    const uint64_t e = last_tile ? 8 * frame_end : p + t_bits;
    s.d0 = p >> 5;
    s.s0 = (uint32_t)(p & 31);
    s.nbits = (uint32_t)(e - p);
    const uint32_t span = s.s0 + s.nbits;
    s.ndw = (span + 31) >> 5;
    s.first_partial = s.s0 != 0 || span < 32;
    s.last_partial = (span & 31) != 0;
    return s;
}

// K2c: zero the dwords that the pack kernel will OR into (tile edges not aligned to a dword).
static __global__ __launch_bounds__(kThreads) void k_zero_edges(FrameGeom g, uint32_t n_frames,
                                                         const uint64_t* __restrict__ tile_off,
                                                         const uint32_t* __restrict__ tile_bits,
                                                         const uint64_t* __restrict__ frame_offsets,
                                                         uint32_t* __restrict__ out32,
                                                         const uint32_t* __restrict__ status) {
    if (status[0] != 0) return;
    const uint64_t tile = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (tile >= (uint64_t)n_frames * g.n_tiles) return;
    const uint32_t frame = (uint32_t)(tile / g.n_tiles);
    const uint32_t t = (uint32_t)(tile % g.n_tiles);
    const Span s = tile_span(frame_offsets[frame], frame_offsets[frame + 1], tile_off[tile], tile_bits[tile],
                             t + 1 == g.n_tiles);
    if (s.first_partial) out32[s.d0] = 0u;
    if (s.last_partial) out32[s.d0 + s.ndw - 1] = 0u;
}

// ---------------------------------------------------------------------------------------------
// Packing.  Each lane serialises its block (header + 12 fields of w bits, LSB first) into the
// workgroup's LDS staging image at its scanned bit offset; the image is then copied to the
// output with one coalesced dword store per lane (edge dwords shared with a neighbour tile are
// OR-ed into the pre-zeroed output instead).
// ---------------------------------------------------------------------------------------------
struct BitSink {
    uint32_t* stage;
    uint64_t acc;
    uint32_t fill;     // valid bits in acc, < 32 between puts
    uint32_t d;        // current staging dword
    bool first;        // the next flushed dword is this lane's first (may be shared)

    __device__ __forceinline__ void put(uint32_t val, uint32_t len) {   // len <= 32, val < 2^len
        acc |= (uint64_t)val << fill;
        fill += len;
        if (fill >= 32) {
            if (first) atomicOr(&stage[d], (uint32_t)acc);
            else stage[d] = (uint32_t)acc;                  // interior dword: owned by this lane alone
            first = false;
            ++d;
            acc >>= 32;
            fill -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (fill) atomicOr(&stage[d], (uint32_t)acc);
    }
};

template <typename T>
constexpr int stage_dwords() { return (31 + kTileBlocks * max_block_bits<T>() + 8 + 31) / 32 + 1; }

// One block -- header of hl bits, nb values of w bits -- into the staging image at bit o.
template <typename T>
__device__ __forceinline__ void pack_block(uint32_t* stage, uint32_t o, const BlockReg<T> (&v)[kBlock], int nb, uint32_t w,
                                           uint32_t w_prev, uint32_t hl) {
    BitSink sink{stage, 0ull, o & 31u, o >> 5, true};
    sink.put(header_val(w, w_prev), hl);
    if (w) {
        const uint32_t mask = w >= 32u ? 0xFFFFFFFFu : ((1u << w) - 1u);
        uint32_t u[kBlock];
#pragma unroll
        for (int k = 0; k < kBlock; ++k) u[k] = (uint32_t)v[k] & mask;   // Bit_pointer.hpp:707-710
        if (nb == kBlock) {
            if (w <= 8u) {                              // 4 values per <=32-bit field
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    sink.put(u[4 * q] | (u[4 * q + 1] << w) | (u[4 * q + 2] << (2 * w)) | (u[4 * q + 3] << (3 * w)), 4 * w);
            } else if (w <= 16u) {                      // 2 values per field
#pragma unroll
                for (int p = 0; p < 6; ++p) sink.put(u[2 * p] | (u[2 * p + 1] << w), 2 * w);
            } else {
#pragma unroll
                for (int k = 0; k < kBlock; ++k) sink.put(u[k], w);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kBlock; ++k)
                if (k < nb) sink.put(u[k], w);
        }
    }
    sink.finish();
}

// A tile's image -- dword j of it is ld(j) -- to its span of the output (all threads of the workgroup).
template <class Ld>
__device__ __forceinline__ void store_span_from(Ld&& ld, const Span& s, uint32_t* __restrict__ out32) {
    uint32_t* dst = out32 + s.d0;
    for (uint32_t j = threadIdx.x; j < s.ndw; j += kThreads) {
        const uint32_t x = ld(j);
        const bool shared = (j == 0 && s.first_partial) || (j + 1 == s.ndw && s.last_partial);
        if (shared) { if (x) atomicOr(&dst[j], x); }
        else dst[j] = x;
    }
}
// ... from the LDS staging image, after the barrier behind the packing
__device__ __forceinline__ void store_span(const uint32_t* stage, const Span& s, uint32_t* __restrict__ out32) {
    store_span_from([&](uint32_t j) { return stage[j]; }, s, out32);
}

}  // namespace trpx
