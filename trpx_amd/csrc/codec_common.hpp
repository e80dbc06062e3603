// Shared device-side definitions of the TERSE/PROLIX kernels (gfx950 / CDNA4 only).
//
// Geometry: the codec block is 12 values (Terse.hpp:264,:478).  One lane owns one block, one
// 64-lane wavefront owns 64 consecutive blocks, one 256-thread workgroup owns a TILE of 256
// consecutive blocks (3072 values) of ONE frame.  Frames never share a tile: the header state
// resets per frame (Terse.hpp:505,:359) and frames start byte aligned (Terse.hpp:502-504).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "trpx_hip.h"

namespace trpx {

constexpr int kBlock = 12;          // values per codec block on the tuned path
constexpr int kWave = 64;
constexpr int kThreads = 256;       // threads per workgroup = blocks per tile
constexpr int kTileBlocks = kThreads;
constexpr int kTileValues = kTileBlocks * kBlock;

struct FrameGeom {
    uint64_t n_values;   // per frame
    uint32_t n_blocks;   // ceil(n_values / 12)
    uint32_t n_tiles;    // ceil(n_blocks / 256)
    uint32_t block;      // values per codec block: 12 on every tuned path; the generic kernels take any value
};

// A stack with its decode index, read only: what every consumer of the index takes (trpx_decode_sum / _roi / _sparse / _dot).
// api.hip's consumer_front fills it; SparseArgs and DotArgs derive from it, SumArgs and RoiArgs hold its fields in their own order.
struct IndexedStack {
    const uint8_t*  terse;
    uint64_t        terse_bytes;
    const uint64_t* frame_offsets;  // n_frames + 1
    FrameGeom       geom;
    uint64_t        n_frames;
    const uint8_t*  widths;         // decode index: width of every block
    const uint64_t* tile_off;       // decode index: frame-relative bit offset of every 256-block group
};
template <class Args> inline void set_stack(Args& a, const IndexedStack& s) {
    a.terse = s.terse; a.terse_bytes = s.terse_bytes; a.frame_offsets = s.frame_offsets; a.geom = s.geom; a.n_frames = s.n_frames;
    a.widths = s.widths; a.tile_off = s.tile_off;
}

template <typename T> struct PixelTraits;
template <> struct PixelTraits<uint8_t>  { using U = uint8_t;  static constexpr int bits = 8;  static constexpr bool is_signed = false; static constexpr int dtype = TRPX_U8; };
template <> struct PixelTraits<int8_t>   { using U = uint8_t;  static constexpr int bits = 8;  static constexpr bool is_signed = true;  static constexpr int dtype = TRPX_I8; };
template <> struct PixelTraits<uint16_t> { using U = uint16_t; static constexpr int bits = 16; static constexpr bool is_signed = false; static constexpr int dtype = TRPX_U16; };
template <> struct PixelTraits<int16_t>  { using U = uint16_t; static constexpr int bits = 16; static constexpr bool is_signed = true;  static constexpr int dtype = TRPX_I16; };
template <> struct PixelTraits<uint32_t> { using U = uint32_t; static constexpr int bits = 32; static constexpr bool is_signed = false; static constexpr int dtype = TRPX_U32; };
template <> struct PixelTraits<int32_t>  { using U = uint32_t; static constexpr int bits = 32; static constexpr bool is_signed = true;  static constexpr int dtype = TRPX_I32; };
// 64-bit containers (what src/terse.cpp:120-123 makes of float / double images): generic correct-first kernels only
template <> struct PixelTraits<uint64_t> { using U = uint64_t; static constexpr int bits = 64; static constexpr bool is_signed = false; static constexpr int dtype = TRPX_U64; };
template <> struct PixelTraits<int64_t>  { using U = uint64_t; static constexpr int bits = 64; static constexpr bool is_signed = true;  static constexpr int dtype = TRPX_I64; };

// Host side: calls f.template operator()<T>() with the pixel type `dtype` (include/trpx_hip.h) names -- the six 8/16/32-bit types
// every tuned kernel is instantiated for; anything else is hipErrorInvalidValue.  (Launchers that also take the 64-bit containers
// or the converting decode's output types handle those by name and leave the six to this.)
template <class F> inline hipError_t for_pixel_type(int dtype, F&& f) {
    switch (dtype) {
    case TRPX_U8:  return f.template operator()<uint8_t>();
    case TRPX_I8:  return f.template operator()<int8_t>();
    case TRPX_U16: return f.template operator()<uint16_t>();
    case TRPX_I16: return f.template operator()<int16_t>();
    case TRPX_U32: return f.template operator()<uint32_t>();
    case TRPX_I32: return f.template operator()<int32_t>();
    }
    return hipErrorInvalidValue;
}

// What the kernels leave in word 0 of a call's status block (atomicMax: the gravest verdict stays).
constexpr uint32_t kStatusInvalid = 1;               // a box that leaves its stack (trpx_decode_roi)
constexpr uint32_t kStatusCorrupt = 5;               // chain, index or widths that do not fit the frame / the stream / the type
static_assert(kStatusInvalid == TRPX_ERR_INVALID_ARG && kStatusCorrupt == TRPX_ERR_CORRUPT, "status words are trpx_status codes");

// Worst-case bits of one block: 12-bit header + 12 full-width values.
template <typename T> constexpr int max_block_bits() { return 12 + kBlock * PixelTraits<T>::bits; }

// ---- header code (Terse.hpp:517-535 encode, :361-372 decode) --------------------------------
// Returns the header length in bits for width w following a block of width w_prev.
__device__ __forceinline__ uint32_t header_len(uint32_t w, uint32_t w_prev) {
    return w == w_prev ? 1u : (w < 7u ? 4u : (w < 10u ? 6u : 12u));
}
// A RESTATED width: an explicit header although the width repeats (flag 0 + the width code, 4 / 6 / 12 bits where header_len
// says 1).  Valid (Terse.hpp:360-372 reads it), written by no encoder here.  header_len cannot know of it, so whatever rebuilds
// a layout from widths alone must be told.  The serial walker of the basic and the converting decode (walk_serial.hpp) tells
// its own extraction kernels (decode.hip) in bit 7 of the width byte of ITS workspace -- widths are at most 64 --; the decode
// index (include/trpx_hip.h) has no such bit: the walkers that write it report a restated width as kStatusCorrupt.
constexpr uint32_t kWidthMask = 0x7Fu, kWidthRestated = 0x80u;
__device__ __forceinline__ uint32_t explicit_header_len(uint32_t w) { return w < 7u ? 4u : (w < 10u ? 6u : 12u); }
// (raw, raw_prev: width bytes as walk_frame leaves them)
__device__ __forceinline__ uint32_t header_len_flagged(uint32_t raw, uint32_t raw_prev) {
    return raw & kWidthRestated ? explicit_header_len(raw & kWidthMask) : header_len(raw & kWidthMask, raw_prev & kWidthMask);
}
// Header value (LSB first, bit 0 = the "same" flag).
__device__ __forceinline__ uint32_t header_val(uint32_t w, uint32_t w_prev) {
    if (w == w_prev) return 1u;                              // Terse.hpp:518
    if (w < 7u) return w << 1;                               // 0, then 3 bits     (:523)
    if (w < 10u) return (7u + ((w - 7u) << 3)) << 1;         // 0, 111, 2 bits     (:527)
    return (31u + ((w - 10u) << 5)) << 1;                    // 0, 111, 11, 6 bits (:531)
}
// The decoders' side of it: an explicit header (Terse.hpp:362-370) from the stream bits that start at it, bit 0 = the "same
// width" flag (:361, clear here).  Every walker parses with one of these two; what follows the parse (w against max_w, the
// last block's value count, bad) is the walker's own.
struct ExplicitHeader { uint32_t w, len; };                  // width, header length in bits (flag included)
__device__ __forceinline__ ExplicitHeader parse_explicit_header(uint32_t bits) {
    uint32_t w = (bits >> 1) & 7u, len = 4;                  // 3 bits                       (:362)
    if (w == 7u) {
        w += (bits >> 4) & 3u; len = 6;                      // they read 7: 2 more          (:365)
        if (w == 10u) { w += (bits >> 6) & 63u; len = 12; }  // the sum reads 10: 6 more     (:368)
    }
    return {w, len};
}
// The same as selects, for steps in which every lane parses the header at its own candidate and nothing may branch (walk_lds.hpp,
// seg_common.hpp).  ext_mask < 63 drops high bits of the 6-bit extension (seg_common.hpp's counting passes).
__device__ __forceinline__ ExplicitHeader parse_explicit_header_select(uint32_t bits, uint32_t ext_mask = 63u) {
    const uint32_t w3 = (bits >> 1) & 7u, wa = 7u + ((bits >> 4) & 3u), wb = 10u + ((bits >> 6) & ext_mask);
    return {w3 != 7u ? w3 : (wa != 10u ? wa : wb), w3 != 7u ? 4u : (wa != 10u ? 6u : 12u)};
}

// Significant-bit width from the OR-reduction of a block (Terse.hpp:508-515, :551-560).
// `m` is OR(v) for unsigned T and OR(|v|) for signed T, as an unsigned 32-bit magnitude.
template <typename T>
__device__ __forceinline__ uint32_t width_from_or(uint32_t m) {
    uint32_t bl = 32u - (uint32_t)__builtin_clz(m | 0u) ;
    bl = m ? bl : 0u;
    if (PixelTraits<T>::is_signed) {
        uint32_t w = m ? bl + 1u : 0u;
        return w > (uint32_t)PixelTraits<T>::bits ? (uint32_t)PixelTraits<T>::bits : w;  // outside D3's domain
    }
    return bl;
}

// The same for 64-bit containers (generic kernels): OR-magnitude as 64 bits.
template <typename T>
__device__ __forceinline__ uint32_t width_from_or64(uint64_t m) {
    const uint32_t bl = m ? 64u - (uint32_t)__builtin_clzll(m) : 0u;
    if (PixelTraits<T>::is_signed) {
        const uint32_t w = m ? bl + 1u : 0u;
        return w > (uint32_t)PixelTraits<T>::bits ? (uint32_t)PixelTraits<T>::bits : w;  // outside D3's domain
    }
    return bl;
}
template <typename T>
__device__ __forceinline__ uint64_t magnitude64(T v) {
    if (PixelTraits<T>::is_signed) {
        const int64_t s = (int64_t)v;
        return s < 0 ? (uint64_t)0 - (uint64_t)s : (uint64_t)s;       // |v| (Terse.hpp:514)
    }
    return (uint64_t)(typename PixelTraits<T>::U)v;
}

template <typename T>
__device__ __forceinline__ uint32_t magnitude(T v) {
    if (PixelTraits<T>::is_signed) {
        int32_t s = (int32_t)v;
        return s < 0 ? 0u - (uint32_t)s : (uint32_t)s;       // |v| (Terse.hpp:514)
    }
    return (uint32_t)(typename PixelTraits<T>::U)v;
}

// ---- wavefront (64-lane) primitives ----------------------------------------------------------
// Inclusive +scan across the 64 lanes with DPP row shifts / broadcasts (no LDS traffic).
// Must be called with all 64 lanes active.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return v;
}

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }
// The same for 64-bit values (shuffles: the scans over frames and groups, off the hot paths).
__device__ __forceinline__ uint64_t wave_inclusive_scan64(uint64_t v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, off, 64);
        uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), off, 64);
        if (lane_id() >= off) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// Maximum over the 64 lanes (same DPP ladder as the scan; every lane gets the result).
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    auto step = [](uint32_t x, uint32_t y) { return x > y ? x : y; };
    v = step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));  // row_shr:8
    v = step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    v = step(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// wave index as a SCALAR (readfirstlane): branches on it are uniform, so whatever a single wave computes from
// wave-uniform values stays in SGPRs / on the scalar unit instead of being treated as divergent per-lane data
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// A wave-uniform value said to be one (readfirstlane): it lives in SGPRs, whatever the compiler can prove about it.
__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return (uint64_t)uniform32((uint32_t)v) | ((uint64_t)uniform32((uint32_t)(v >> 32)) << 32);
}

// ---- reading the stream (a 4-byte aligned buffer of n_dw dwords; dwords past its end read as zero) -------------
// An aligned dword that holds >= 1 valid byte never crosses into an unmapped page.
__device__ __forceinline__ uint32_t ld_stream_dw(const uint32_t* __restrict__ s32, uint64_t idx, uint64_t n_dw) {
    return idx < n_dw ? s32[idx] : 0u;
}
// 16 bytes at dword index d, dword by dword (V: uint4 or a site's own vector of four dwords)
template <class V = uint4>
__device__ __forceinline__ V load_stream16_guarded(const uint32_t* __restrict__ s32, uint64_t d, uint64_t n_dw) {
    V x;
    x.x = d < n_dw ? s32[d] : 0u; x.y = d + 1 < n_dw ? s32[d + 1] : 0u;
    x.z = d + 2 < n_dw ? s32[d + 2] : 0u; x.w = d + 3 < n_dw ? s32[d + 3] : 0u;
    return x;
}
// ... and in one load where the buffer is 16-byte aligned (base16), d % 4 == 0 and all four dwords exist (the tile kernels)
__device__ __forceinline__ uint4 load_stream16(const uint32_t* __restrict__ s32, uint64_t d, uint64_t n_dw, bool base16) {
    if (base16 && d + 4 <= n_dw) return *reinterpret_cast<const uint4*>(s32 + d);
    return load_stream16_guarded(s32, d, n_dw);
}
// The bits from bit p on of the dwords ld(i) reads -- an LDS image, a guarded global load: 64 - p % 32 of them are valid.
template <class Ld, class P>
__device__ __forceinline__ uint64_t stream_bits(Ld&& ld, P p) {
    return ((uint64_t)ld(p >> 5) | ((uint64_t)ld((p >> 5) + 1) << 32)) >> (p & 31u);
}
// One field of w bits (1 .. 32) at bit p as the pixel type's value in 32 bits: the generic read of a partial block's fields
// (Bit_pointer.hpp:597-617; sign extension :784-789).
__device__ __forceinline__ uint32_t field_mask(uint32_t w) { return w >= 32u ? 0xFFFFFFFFu : ((1u << w) - 1u); }
template <typename T, class Ld, class P>
__device__ __forceinline__ uint32_t stream_field(Ld&& ld, P p, uint32_t w, uint32_t mask) {
    uint32_t f = (uint32_t)stream_bits(ld, p) & mask;
    if (PixelTraits<T>::is_signed) f = (uint32_t)((int32_t)(f << (32u - w)) >> (32u - w));
    return f;
}

// Workgroup-wide exclusive scan of one u32 per thread (256 threads = 4 waves).
// `wave_tot` is a 4-entry LDS array.  Returns the exclusive prefix; *total gets the tile sum.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wave_tot, uint32_t* total) {
    uint32_t inc = wave_inclusive_scan(v);
    if (lane_id() == 63) wave_tot[wave_id()] = inc;
    __syncthreads();
    uint32_t t0 = wave_tot[0], t1 = wave_tot[1], t2 = wave_tot[2], t3 = wave_tot[3];
    int w = wave_id();
    uint32_t base = (w > 0 ? t0 : 0u) + (w > 1 ? t1 : 0u) + (w > 2 ? t2 : 0u);
    *total = t0 + t1 + t2 + t3;
    return base + inc - v;
}

// ---- clearing device words on the launch stream ------------------------------------------------
// Every call clears its status block (and the encoder its descriptor words) with this kernel instead of
// hipMemsetAsync: kernel nodes replay reliably when the call is captured into a hipGraph, memset nodes did
// not (ROCm 7.2 / torch 2.10: from the second replay on the words stayed uncleared; tests/test_gpu_graph.py).
template <int kUnused = 0>
__global__ __launch_bounds__(kThreads) void k_zero_words(uint64_t* __restrict__ p, uint64_t n, uint64_t* __restrict__ q,
                                                         uint64_t m) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) p[i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x < m) q[threadIdx.x] = 0ull;
}
inline void zero_status(uint32_t* status, hipStream_t st) {           // 8 x u32, 8-byte aligned
    hipLaunchKernelGGL(k_zero_words<0>, dim3(1), dim3(kThreads), 0, st, static_cast<uint64_t*>(nullptr), (uint64_t)0,
                       reinterpret_cast<uint64_t*>(status), (uint64_t)4);
}
// workgroups for `units` pieces of work at per_wg a workgroup, at most cap: a kernel launched with it strides over what is left
inline uint32_t grid_capped(uint64_t units, uint32_t per_wg, uint32_t cap = 4096) {
    const uint64_t wgs = (units + per_wg - 1) / per_wg;
    return (uint32_t)(wgs < cap ? wgs : cap);
}

// ---- workspace layouts (device memory, carved by the host API) -------------------------------
// encode: [status-shadow 64 B][frame_size u64 x F][tile_off u64 x F*T][tile_bits u32 x F*T]
// decode: [tile_off u64 x F*T][widths u8 x F*nblocks (padded to 16)]
__host__ __device__ inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
// The list of the frames the per-frame decoder hands over (DecodeArgs::defer): word 0 = count, words 1 .. n_frames = entries.
// In FRONT of it (DecodeArgs::defer points at the count): kDeferSlots accumulators of the stack's statistics, one 128-byte line
// each -- width changes << 32 | blocks, summed over the frames' first super-steps -- by which frames near the hand-over line
// decide (decode_frame.hip); cleared with the count.  The accumulators are word 0 of every line; the last line's last four words
// are the large-frame routes': [-1] k_seg_fallback's barrier counter, [-2] the number of listed frames with bit 31 set
// (header-dense large frames: k_seg_wg's, decode_seg.hip), [-3] / [-4] the index route's vote and verdict (ChainVote, decode_part.hip).
constexpr uint32_t kDeferSlots = 64, kDeferSlotWords = 16;                 // (u64 words per slot: a cache line)
constexpr size_t kDeferFront = 8u * kDeferSlots * kDeferSlotWords;         // bytes in front of the list
inline size_t defer_bytes(size_t n_frames) { return kDeferFront + align_up(4 * (n_frames + 2), 256); }

}  // namespace trpx
