// Corrected decode (trpx_decode_corrected): a stack with its decode index -> out[f][p] = ((float) px[f][p] - dark[p]) * gain[p], the
// frames a float pipeline starts from, without the integer stack and the float temporaries of decode + convert + subtract + multiply.
// Stands in for the loop of Terse.hpp:352-389 / src/prolix.cpp:69-92 with the correction in its store.
//
//   k_decode_corrected  a workgroup per TILE of k_unpack_tiles' geometry (1024 blocks, 512 for 32-bit pixels; 4 / 2 blocks per
//                       lane), assembled from unpack_tile.hpp's pieces as they are: tile_scan (widths -> bit offsets), the window
//                       check, tile_fetch16 (the tile's stream bytes, once, coalesced, into LDS), the restated-width check,
//                       tile_extract_full (code specialised on the width) and tile_partial_width / _field for the frame's last
//                       block.  The store step is its own (correct_px.hpp: the rule and the index arithmetic).  A wavefront whose
//                       64 blocks are full writes its 768 values as 32-bit words into its LDS row (64 x 12 dwords whatever the
//                       pixel type) and every lane then takes four consecutive pixels at a time, three times: 16 bytes of dark, 16
//                       bytes of gain -- 1 MB each for a 512 x 512 frame, read by every frame: they stay in cache --, the three
//                       operations, one 16-byte non-temporal store.  Each instruction of the wavefront covers 1024 consecutive
//                       bytes.  The frame's last wavefront stores lane-owned quads, the last block's cut at n_values: no map entry
//                       behind n_values is read.  Frames that start off a 16-byte boundary (n_values % 4 != 0) or maps that do
//                       take the same code with accesses that assume 4-byte alignment.
//                       Instantiated per pixel type and per presence of each map: with both absent there is no map load and no
//                       arithmetic behind the conversion.
// Every tile of every frame is validated: the window against the frame and the LDS image, the tile's end against the next tile's
// recorded offset (behind the last tile: against the frame's size, S_f = 1 + bits / 8), every width against the type, every header
// bit against the widths.  A tile that does not fit sets CORRUPT and writes nothing; a bad width or header bit sets CORRUPT.
// HBM traffic: stream + index read once, 4 * n_frames * n_values bytes written once.
#include "codec_common.hpp"
#include "decode_corrected.hpp"
#include "unpack_common.hpp"
#include "unpack_tile.hpp"

namespace trpx {

namespace {

typedef float f4_t __attribute__((ext_vector_type(4)));
typedef f4_t f4_a4 __attribute__((aligned(4)));             // a quad of a frame or a map that is only 4-byte aligned

// One quad: v its four pixels (32-bit, extended), q where it lies in the frame and how much of it exists.
template <typename T, bool kDark, bool kGain, class V4>
__device__ __forceinline__ void corr_whole_quad(const uint32_t (&v)[4], uint64_t px, const float* __restrict__ dark,
                                                const float* __restrict__ gain, float* __restrict__ fout) {
    constexpr bool sg = PixelTraits<T>::is_signed;
    f4_t d = {0.f, 0.f, 0.f, 0.f}, g = {1.f, 1.f, 1.f, 1.f};
    if constexpr (kDark) d = *reinterpret_cast<const V4*>(dark + px);
    if constexpr (kGain) g = *reinterpret_cast<const V4*>(gain + px);
    const f4_t o = {correct_px<sg, kDark, kGain>(v[0], d.x, g.x), correct_px<sg, kDark, kGain>(v[1], d.y, g.y),
                    correct_px<sg, kDark, kGain>(v[2], d.z, g.z), correct_px<sg, kDark, kGain>(v[3], d.w, g.w)};
    __builtin_nontemporal_store(o, reinterpret_cast<V4*>(fout + px));
}
template <typename T, bool kDark, bool kGain>
__device__ __forceinline__ void corr_store_quad(const uint32_t (&v)[4], const CorrQuad& q, bool frame16, const float* __restrict__ dark,
                                                const float* __restrict__ gain, float* __restrict__ fout) {
    if (corr_vec16(frame16, q)) corr_whole_quad<T, kDark, kGain, f4_t>(v, q.px, dark, gain, fout);
    else if (q.n == kCorrQuad) corr_whole_quad<T, kDark, kGain, f4_a4>(v, q.px, dark, gain, fout);
    else {
#pragma unroll
        for (uint32_t i = 0; i < kCorrQuad; ++i)
            if (i < q.n)                                    // (the cut quad of a frame's last block: nothing behind n_values)
                fout[q.px + i] = correct_px<PixelTraits<T>::is_signed, kDark, kGain>(v[i], kDark ? dark[q.px + i] : 0.f, kGain ? gain[q.px + i] : 1.f);
    }
}

}  // namespace

template <typename T, bool kDark, bool kGain>
__global__ __launch_bounds__(kThreads, 4) void k_decode_corrected(CorrectedArgs a, uint32_t tiles_per_frame) {
    constexpr int kSub = unpack_sub_tiles<T>();
    static_assert(kCorrBlock == (uint32_t)kBlock && kCorrWave == (uint32_t)kWave, "correct_px.hpp restates the block and the wavefront");
    __shared__ __attribute__((aligned(16))) uint32_t s_image[unpack_image_dwords<T>()];
    __shared__ uint32_t s_wtot[kSub * 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[(kThreads / kWave) * kCorrRowDwords];
    if (a.status[0] != 0) return;                           // corrupt chain (the walk or the locator said so): produce nothing
    const FrameGeom g = a.geom;
    const uint32_t tid = threadIdx.x;
    const int lane = lane_id(), wave = wave_id();
    const uint64_t frame = blockIdx.x / tiles_per_frame;
    const uint32_t t = (uint32_t)(blockIdx.x % tiles_per_frame);
    const uint32_t b0 = t * kSub * kThreads;
    uint32_t w[kSub], hl[kSub], off[kSub], tile_bits;
    int nb[kSub];
    tile_scan<kSub>(w, hl, off, nb, tile_bits, TileWidthsOf{a.widths + frame * g.n_blocks}, g, t, s_wtot, lane, wave);
    const uint64_t fo = a.frame_offsets[frame], fe = a.frame_offsets[frame + 1];
    const uint64_t t_off = a.tile_off[frame * g.n_tiles + (uint64_t)t * kSub];   // (the index records every 256 blocks)
    uint64_t a0, d_lo;
    uint32_t n_dw;
    // the index against the frame, and against the LDS image (widths above the type's: more bits than the image holds)
    // ... and the tile's end against what follows it: the next tile's recorded offset, or the frame's size S_f = 1 + bits / 8
    // (Terse.hpp:547) behind the frame's last tile
    bool fits = tile_window(fo, fe, t_off, tile_bits, a.terse_bytes, a0, d_lo, n_dw) && n_dw <= (uint32_t)(unpack_image_dwords<T>() - 8);
    if (fits) {
        const uint64_t end = t_off + tile_bits;
        fits = t + 1 < tiles_per_frame ? a.tile_off[frame * g.n_tiles + (uint64_t)(t + 1) * kSub] == end : 1 + end / 8 == fe - fo;
    }
    if (!fits) {
        if (tid == 0) atomicMax(&a.status[0], kStatusCorrupt);
        return;
    }
    for (uint32_t i = tid * 4; i < n_dw; i += kThreads * 4) *reinterpret_cast<uint4*>(&s_image[i]) = tile_fetch16(d_lo, i, a.terse, a.terse_bytes);
    __syncthreads();
    const uint32_t img_bit0 = tile_img_bit0(a0, d_lo);

    float* __restrict__ fout = a.out + frame * g.n_values;
    const bool frame16 = corr_frame_vec16((uintptr_t)a.out, frame, g.n_values, (uintptr_t)a.dark, (uintptr_t)a.gain);
    uint32_t* const row = s_stage + wave * kCorrRowDwords;
#pragma unroll
    for (int r = 0; r < kSub; ++r) {
        const uint32_t b = b0 + r * kThreads + tid;
        const uint32_t q = img_bit0 + off[r] + hl[r];       // first payload bit in the image
        // (as unpack_tile: the "same width" bit stands exactly where header_len counted one bit, or the widths are not this stream's
        // layout -- a restated width, codec_common.hpp)
        if (nb[r] && ((s_image[(q - hl[r]) >> 5] >> ((q - hl[r]) & 31u)) & 1u) != (hl[r] == 1u ? 1u : 0u)) atomicMax(&a.status[0], kStatusCorrupt);
        if (nb[r] && tile_too_wide<T>(w[r])) atomicMax(&a.status[0], kStatusCorrupt);
        uint32_t u[kBlock];
        tile_extract_full<T>(u, s_image, q, w[r], nb[r]);
        const uint32_t g0 = b - (uint32_t)lane;             // the wavefront's first block
        if (corr_wave_staged(g0, g.n_values)) {             // (uniform: the wavefront's 64 blocks are all full)
#pragma unroll
            for (int k = 0; k < (int)kCorrRounds; ++k)
                *reinterpret_cast<u4_t*>(row + lane * kBlock + 4 * k) = u4_t{u[4 * k], u[4 * k + 1], u[4 * k + 2], u[4 * k + 3]};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (uint32_t j = 0; j < kCorrRounds; ++j) {
                const u4_t x = *reinterpret_cast<const u4_t*>(row + corr_staged_slot((uint32_t)lane, j));
                const uint32_t v[4] = {x.x, x.y, x.z, x.w};
                corr_store_quad<T, kDark, kGain>(v, corr_staged_quad(g0, (uint32_t)lane, j, g.n_values), frame16, a.dark, a.gain, fout);
            }
            __builtin_amdgcn_wave_barrier();                // (the row is rewritten in the next round)
        } else if (nb[r]) {
            if (nb[r] < kBlock) {                           // the frame's last, partial block: field by field
                const uint32_t ww = tile_partial_width<T>(w[r]), mask = field_mask(ww);
                uint32_t p = q;
#pragma unroll
                for (int k = 0; k < kBlock; ++k) {
                    if (k < nb[r] && ww) {
                        u[k] = tile_partial_field<T>(s_image, p, ww, mask);
                        p += ww;
                    }
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < kCorrRounds; ++i) {
                const uint32_t v[4] = {u[4 * i], u[4 * i + 1], u[4 * i + 2], u[4 * i + 3]};
                corr_store_quad<T, kDark, kGain>(v, corr_block_quad(b, i, g.n_values), frame16, a.dark, a.gain, fout);
            }
        }
    }
}

hipError_t launch_decode_corrected(int dtype, const CorrectedArgs& a, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    // the launch shape from the geometry alone: a workgroup per tile (the call takes at most 2^24 - 1 groups of 256 blocks)
    return for_pixel_type(dtype, [&]<class T>() {
        constexpr uint32_t tb = unpack_sub_tiles<T>() * kThreads;
        const uint32_t tpf = (a.geom.n_blocks + tb - 1) / tb;
        const dim3 grid((uint32_t)(a.n_frames * tpf));
        if (a.dark && a.gain) hipLaunchKernelGGL((k_decode_corrected<T, true, true>), grid, dim3(kThreads), 0, st, a, tpf);
        else if (a.dark) hipLaunchKernelGGL((k_decode_corrected<T, true, false>), grid, dim3(kThreads), 0, st, a, tpf);
        else if (a.gain) hipLaunchKernelGGL((k_decode_corrected<T, false, true>), grid, dim3(kThreads), 0, st, a, tpf);
        else hipLaunchKernelGGL((k_decode_corrected<T, false, false>), grid, dim3(kThreads), 0, st, a, tpf);
        return hipGetLastError();
    });
}

}  // namespace trpx
