// trpx_decode_bins (decode_bins.hip): what one lane does with one block of a frame -- the block's labels
// out of the label map, and the block's <= 12 (value, label) pairs reduced to one "add" per stretch of equal labels.  Free of HIP:
// the kernels and tests/cpp/bins_sanitize.cpp (ASan + UBSan on a CPU, over exact-size heap arrays) run this text.
//
// A label >= n_bins belongs to no bin (n_bins <= kBinsMax < 0xFFFF, so 0xFFFF never does).  In a radial or ring map the
// neighbouring pixels of a row mostly share a label: the values of a stretch of equal labels are summed first and leave in ONE add
// when the label changes; a stretch whose sum is zero, or whose label is no bin, leaves in none.  Sums are the bits of int64 sums
// (signed values as their two's-complement 64-bit pattern): addition modulo 2^64, so the order of the adds does not matter.
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

constexpr uint32_t kBinsMax = 4096;                         // 32 KB of uint64 sums in LDS per workgroup
constexpr uint32_t kBinsBlock = 12;                         // values per codec block (kBlock)
constexpr uint32_t kBinsNoLabel = 0xFFFFu;                  // what stands for the pixels behind a frame's last: no bin

// a block's 12 labels, two per dword
struct BinsLabels { uint32_t d[kBinsBlock / 2]; };
TRPX_HD inline uint32_t bins_label(const BinsLabels& l, int i) { return (l.d[i >> 1] >> (16 * (i & 1))) & 0xFFFFu; }

// The labels of the block that starts at pixel `first` and holds nr values (1 .. 12; fewer than 12: a frame's partial last
// block, padded with kBinsNoLabel).  aligned8: the map is 8-byte aligned -- a whole block's labels are bytes 24 * block .., three
// 8-byte loads; label by label otherwise.  Nothing behind labels[first + nr) is read.
TRPX_HD inline BinsLabels bins_load_labels(const uint16_t* labels, uint64_t first, uint32_t nr, bool aligned8) {
    BinsLabels l;
    if (aligned8 && nr == kBinsBlock) {
        const uint64_t* q = reinterpret_cast<const uint64_t*>(labels + first);
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < 3; ++j) {
            const uint64_t x = q[j];
            l.d[2 * j] = (uint32_t)x;
            l.d[2 * j + 1] = (uint32_t)(x >> 32);
        }
    } else {
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < (int)kBinsBlock / 2; ++j) {
            const uint32_t lo = (uint32_t)(2 * j) < nr ? labels[first + 2 * j] : kBinsNoLabel;
            const uint32_t hi = (uint32_t)(2 * j + 1) < nr ? labels[first + 2 * j + 1] : kBinsNoLabel;
            l.d[j] = lo | (hi << 16);
        }
    }
    return l;
}

// some label of the block is a bin (the block's support bit)
TRPX_HD inline bool bins_any_label(const BinsLabels& l, uint32_t n_bins) {
    bool any = false;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < (int)kBinsBlock; ++i) any = any || bins_label(l, i) < n_bins;
    return any;
}

// The block's nr pairs (value(i): the bits of value i < nr as int64, l: its labels, padded with kBinsNoLabel behind nr) into the
// bins: add(bin, sum) once per stretch of equal labels whose label is a bin and whose sum is not zero.  One running sum and one
// guarded add per position (the stretch ends there: the next label differs), so that lanes whose labels change at different
// positions share the same twelve add sites.
template <class Value, class Add>
TRPX_HD inline void bins_merge(uint32_t nr, Value&& value, const BinsLabels& l, uint32_t n_bins, Add&& add) {
    uint64_t sum = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < (int)kBinsBlock; ++i) {
        const uint32_t lab = bins_label(l, i);
        sum += (uint32_t)i < nr ? value(i) : 0ull;
#if defined(TRPX_BINS_NO_MERGE)                             // measurement build (make binsnomerge, tools/bins_time.py): one add per value
        const bool ends = true;
#else
        const bool ends = i + 1 == (int)kBinsBlock || bins_label(l, i + 1 < (int)kBinsBlock ? i + 1 : i) != lab;
#endif
        if (ends) {
            if (lab < n_bins && sum != 0) add(lab, sum);
            sum = 0;
        }
    }
}

}  // namespace trpx
