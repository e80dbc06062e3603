// trpx_decode_corrected (decode_corrected.hip): the correction of one pixel and the index arithmetic of the
// kernel's store step, written once.  Free of HIP: the kernel and tests/cpp/corrected_sanitize.cpp (ASan + UBSan on a CPU) run
// this text.
//
//   out[f][p] = ((float) px[f][p] - dark[p]) * gain[p]
//
// three IEEE binary32 operations in this order, each rounded once to nearest even: the conversion (exact for pixels of at most 16
// bits, rounds 32-bit pixels of magnitude above 2^24), the subtraction, the multiplication.  Nothing is fused or re-associated:
// contraction is switched off inside the rule, so the host and the device compile the same three operations.  A map that is
// absent leaves its operation out, which gives what an all +0.0f dark / an all 1.0f gain gives: x - (+0) = x for every x a
// conversion can yield (never -0), x * 1 = x.  Subnormal results are unspecified (a device may flush them).
//
// The store step.  A frame's pixels leave in QUADS of four consecutive pixels whose first is a multiple of 4 from the frame's
// first pixel (a block is 12 values: three quads).  A wavefront whose 64 blocks are all full passes its 768 values through its LDS
// row (64 x 12 dwords, block after block) and lane l takes, in round j of 3, the quad at row dword 4 * (64 j + l): one
// instruction covers 1024 consecutive bytes of the maps and of the output.  Any other wavefront -- the last of a frame -- stores
// lane-owned: lane l the three quads of its own block, the quads of the frame's last, partial block cut at n_values.  Both forms
// give (first pixel, pixels that exist); of a quad that is cut only the pixels in front of n_values are read from the maps and
// written.  A whole quad moves as one 16-byte access where the output address and both map addresses are 16-byte aligned --
// decided once per frame, since every quad starts a multiple of 16 bytes behind the frame's first pixel -- and as accesses that
// assume 4-byte alignment otherwise.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef TRPX_HD
#if defined(__HIPCC__)
#define TRPX_HD __host__ __device__
#else
#define TRPX_HD
#endif
#endif

namespace trpx {

constexpr uint32_t kCorrBlock = 12;                         // values per block (codec_common.hpp: kBlock)
constexpr uint32_t kCorrWave = 64;                          // blocks per wavefront
constexpr uint32_t kCorrQuad = 4;                           // pixels per quad: 16 bytes of float32
constexpr uint32_t kCorrRounds = kCorrBlock / kCorrQuad;    // quads per block = rounds per staged wavefront
constexpr uint32_t kCorrRowDwords = kCorrWave * kCorrBlock; // a wavefront's LDS row, whatever the pixel type

// ---- the rule for one pixel: u is the pixel as the decoders hold it, sign- or zero-extended to 32 bits ----------------------------
// (contraction off for this function alone: clang by a pragma at the head of its body, GCC by a function attribute)
#if !defined(__clang__) && defined(__GNUC__)
#define TRPX_CORR_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define TRPX_CORR_NO_CONTRACT
#endif
template <bool kSigned, bool kDark, bool kGain>
TRPX_HD TRPX_CORR_NO_CONTRACT inline float correct_px(uint32_t u, float dark, float gain) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float x = kSigned ? (float)(int32_t)u : (float)u;       // 1: the conversion
    if (kDark) x = x - dark;                                // 2: the subtraction
    if (kGain) x = x * gain;                                // 3: the multiplication
    return x;
}

// ---- the store step -------------------------------------------------------------------------------------------------------------
struct CorrQuad {
    uint64_t px;                                            // the quad's first pixel, from the frame's first
    uint32_t n;                                             // how many of its four pixels exist (0: none, nothing is read or written)
};
TRPX_HD inline CorrQuad corr_quad_at(uint64_t px, uint64_t n_values) {
    return {px, px >= n_values ? 0u : n_values - px >= kCorrQuad ? kCorrQuad : (uint32_t)(n_values - px)};
}
// the wavefront whose first block is block g0 of the frame stores staged: its 64 blocks are all full
TRPX_HD inline bool corr_wave_staged(uint32_t g0, uint64_t n_values) { return ((uint64_t)g0 + kCorrWave) * kCorrBlock <= n_values; }
// staged: the row dword at which lane `lane` reads its quad of round j < kCorrRounds, and the quad
TRPX_HD inline uint32_t corr_staged_slot(uint32_t lane, uint32_t j) { return kCorrQuad * (j * kCorrWave + lane); }
TRPX_HD inline CorrQuad corr_staged_quad(uint32_t g0, uint32_t lane, uint32_t j, uint64_t n_values) {
    return corr_quad_at((uint64_t)g0 * kCorrBlock + corr_staged_slot(lane, j), n_values);
}
// lane-owned: quad i < kCorrRounds of block b (values 4 i .. 4 i + 3 of the block)
TRPX_HD inline CorrQuad corr_block_quad(uint32_t b, uint32_t i, uint64_t n_values) {
    return corr_quad_at((uint64_t)b * kCorrBlock + kCorrQuad * i, n_values);
}
// the 16-byte path: allowed for the whole quads of a frame whose first output pixel and both maps (absent: 0) are 16-byte aligned
TRPX_HD inline bool corr_frame_vec16(uintptr_t out, uint64_t frame, uint64_t n_values, uintptr_t dark, uintptr_t gain) {
    return ((out + 4u * (uintptr_t)(frame * n_values)) & 15u) == 0 && (dark & 15u) == 0 && (gain & 15u) == 0;
}
TRPX_HD inline bool corr_vec16(bool frame16, const CorrQuad& q) { return frame16 && q.n == kCorrQuad && (q.px & (kCorrQuad - 1)) == 0; }

}  // namespace trpx
