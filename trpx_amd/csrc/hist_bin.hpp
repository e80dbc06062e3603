// trpx_decode_hist (decode_hist.hip): the bin rule, written once -- the bin of a value, the values a block
// of a given width can hold, "the whole block lies in one bin", and what one lane does with an extracted block.  Free of HIP: the
// kernel and tests/cpp/hist_sanitize.cpp (ASan + UBSan on a CPU) run this text.
//
//   bin(v) = clamp(floor((v - lo) / 2^shift), 0, n_bins - 1) in int64: the first and the last bin take everything below and above,
//   so every pixel has exactly one bin.  With |lo| <= 2^32, shift <= 32 and a pixel type of at most 32 bits v - lo cannot leave
//   int64 (|v - lo| < 2^33).
//
// A block's width bounds its values (the convention is sparse_min_width's, decode_sparse.hip): w-bit fields of an unsigned
// stream hold [0, 2^w - 1], w-bit two's-complement fields of a signed one [-2^(w-1), 2^(w-1) - 1], width 0 holds {0}.  bin() is
// monotone, so all values of that range have one bin exactly when its two ends do: such a block is counted from its width alone
// (its value count into that bin), and its payload is never fetched.  A padded width (wider than the values need) only widens
// the range: the rule may then extract a block it could have skipped, never the reverse.
//
// The extracted block: its <= 12 bin numbers as bins_merge.hpp's labels with the value 1 -- neighbours of equal bin are counted
// in registers, one add per change of bin.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "bins_merge.hpp"

namespace trpx {

constexpr uint32_t kHistMaxBins = kBinsMax;                 // 16 KB of uint32 counters in LDS per workgroup
constexpr uint32_t kHistMaxShift = 32;
constexpr int64_t kHistMaxLo = (int64_t)1 << 32;            // -2^32 <= lo <= 2^32
constexpr uint32_t kHistMaxWidth = 32;                      // the widest field of a stream with a decode index
constexpr uint32_t kHistNoBin = 0xFFFFFFFFu;                // "this width straddles a bin edge" in the per-width table

TRPX_HD inline bool hist_args_ok(int64_t lo, uint32_t shift, uint32_t n_bins) {
    return n_bins >= 1 && n_bins <= kHistMaxBins && shift <= kHistMaxShift && lo >= -kHistMaxLo && lo <= kHistMaxLo;
}

// the bin of value v (arguments within hist_args_ok, v a pixel of at most 32 bits)
TRPX_HD inline uint32_t hist_bin(int64_t v, int64_t lo, uint32_t shift, uint32_t n_bins) {
    const int64_t q = (v - lo) >> shift;                    // (arithmetic shift: floors below lo)
    return q < 0 ? 0u : q >= (int64_t)n_bins ? n_bins - 1 : (uint32_t)q;
}

// The same bin in 32-bit arithmetic, where v - lo cannot leave int32: pixels of at most 16 bits and |lo| <= 2^30
// (hist_narrow_ok).  A shift of 32 is a shift of 31 there: |v - lo| < 2^31, so both give 0 or -1.
TRPX_HD inline bool hist_narrow_ok(int64_t lo, uint32_t pixel_bits) {
    return pixel_bits <= 16 && lo >= -((int64_t)1 << 30) && lo <= ((int64_t)1 << 30);
}
TRPX_HD inline uint32_t hist_bin32(int32_t v, int32_t lo, uint32_t shift, uint32_t n_bins) {
    const int32_t q = (v - lo) >> (shift < 31u ? shift : 31u);
    return q < 0 ? 0u : q >= (int32_t)n_bins ? n_bins - 1 : (uint32_t)q;
}

// the values a block of width w <= 32 can hold
TRPX_HD inline int64_t hist_width_min(uint32_t w, bool stream_signed) { return stream_signed && w ? -((int64_t)1 << (w - 1)) : 0; }
TRPX_HD inline int64_t hist_width_max(uint32_t w, bool stream_signed) {
    return !w ? 0 : stream_signed ? ((int64_t)1 << (w - 1)) - 1 : ((int64_t)1 << w) - 1;
}

// true, and *bin: every value a block of width w can hold has this one bin
TRPX_HD inline bool hist_block_one_bin(uint32_t w, bool stream_signed, int64_t lo, uint32_t shift, uint32_t n_bins, uint32_t* bin) {
    if (w > kHistMaxWidth) w = kHistMaxWidth;               // (no such block reaches a consumer: the walk refuses its group)
    const uint32_t b = hist_bin(hist_width_min(w, stream_signed), lo, shift, n_bins);
    *bin = b;
#if defined(TRPX_HIST_NO_SKIP)                              // measurement / test build (make histnoskip): only width-0 blocks are counted unread
    if (w != 0) return false;
#endif
    return hist_bin(hist_width_max(w, stream_signed), lo, shift, n_bins) == b;
}

// The nr values of an extracted block (bin(i): the bin of value i < nr) into the counters: add(bin, count) once per stretch of
// neighbours of equal bin.  bins_merge with the value 1 and the bins as labels (a bin < 4096 fits a label; behind nr: no label).
template <class Bin, class Add>
TRPX_HD inline void hist_count_bins(uint32_t nr, Bin&& bin, uint32_t n_bins, Add&& add) {
    BinsLabels l;
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < (int)kBinsBlock / 2; ++j) {
        const uint32_t b0 = (uint32_t)(2 * j) < nr ? bin(2 * j) : kBinsNoLabel;
        const uint32_t b1 = (uint32_t)(2 * j + 1) < nr ? bin(2 * j + 1) : kBinsNoLabel;
        l.d[j] = b0 | (b1 << 16);
    }
    bins_merge(nr, [](int) { return (uint64_t)1; }, l, n_bins, [&](uint32_t b, uint64_t n) { add(b, (uint32_t)n); });
}
// ... with value(i): value i < nr as int64, and the bin rule in int64
template <class Value, class Add>
TRPX_HD inline void hist_count_block(uint32_t nr, Value&& value, int64_t lo, uint32_t shift, uint32_t n_bins, Add&& add) {
    hist_count_bins(nr, [&](int i) { return hist_bin(value(i), lo, shift, n_bins); }, n_bins, add);
}

}  // namespace trpx
