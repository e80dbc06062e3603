// trpx_decode_binned (decode_binned.hip): what one lane does with one block of a frame -- the block's
// <= 12 consecutive pixels mapped onto the bins of bin_y x bin_x pixels they fall into, neighbours of one bin summed in registers,
// one "add" per change of bin.  Also the launch arithmetic (how a frame is cut into bands of whole output rows).  Free of HIP: the
// kernel and tests/cpp/binned_sanitize.cpp (ASan + UBSan on a CPU, over exact-size accumulator arrays) run this text.
//
// A band is a range of whole output rows of one frame, and so the consecutive pixels [p_lo, p_hi) of it; its accumulators are
// [rows][out_w], index (Y - row0) * out_w + X.  A block may straddle a band's edge (and a 256-block group two bands): only the
// pixels inside [p_lo, p_hi) are added, and only they can produce an index, so every emitted index lies inside the band's array.
// The two divisions by width and the two by the bin sides are done once per block; from there the position is stepped.
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

constexpr uint32_t kBinnedBlock = 12;                       // values per codec block (kBlock)
constexpr uint32_t kBinnedMaxBin = 64;                      // a bin's side: 64 * 64 * 65535 < 2^32, so types of <= 16 bits sum in 32 bits
constexpr uint32_t kBinnedAccs = 8192;                      // accumulators of a band (32 KB of uint32, 64 KB of uint64) -- and the widest output row
constexpr uint32_t kBinnedTargetWgs = 1536;                 // workgroups a launch aims at where the frames alone give fewer
constexpr uint32_t kBinnedRunGroups = 8;                    // 256-block groups per run (kRun): a band is not made shorter than that for the frames' sake
constexpr uint32_t kBinnedGroupValues = 256 * kBinnedBlock; // values of a 256-block group

struct BinnedGeom { uint32_t width, height, bin_y, bin_x, out_w, out_h; };
TRPX_HD inline BinnedGeom binned_geom(uint32_t n_values, uint32_t width, uint32_t bin_y, uint32_t bin_x) {
    const uint32_t height = n_values / width;
    return {width, height, bin_y, bin_x, (width + bin_x - 1) / bin_x, (height + bin_y - 1) / bin_y};
}

// How a frame is cut: `bands` bands of `rows` output rows (the last: what is left).  As many bands as the accumulators force
// (rows * out_w <= kBinnedAccs); more where few frames would leave the GPU idle, down to about one run of groups per band.
struct BinnedPlan { uint32_t rows, bands; };
TRPX_HD inline BinnedPlan binned_plan(const BinnedGeom& g, uint64_t n_frames) {
    const uint32_t rows_lds = kBinnedAccs / g.out_w ? kBinnedAccs / g.out_w : 1u;      // (out_w <= kBinnedAccs)
    const uint64_t by_lds = (g.out_h + rows_lds - 1) / rows_lds;
    const uint64_t by_frames = n_frames ? (kBinnedTargetWgs + n_frames - 1) / n_frames : 1;
    const uint64_t groups = ((uint64_t)g.width * g.height + kBinnedGroupValues - 1) / kBinnedGroupValues;
    const uint64_t by_runs = (groups + kBinnedRunGroups - 1) / kBinnedRunGroups;
    uint64_t want = by_frames < by_runs ? by_frames : by_runs;
    if (want < by_lds) want = by_lds;
    if (want > g.out_h) want = g.out_h;
    const uint32_t rows = (uint32_t)((g.out_h + want - 1) / want);
    return {rows, (g.out_h + rows - 1) / rows};
}

// band b of a frame: its first output row, its rows, its pixels
struct BinnedBand { uint32_t row0, rows, p_lo, p_hi; };
TRPX_HD inline BinnedBand binned_band(const BinnedGeom& g, const BinnedPlan& p, uint32_t b) {
    BinnedBand d;
    d.row0 = b * p.rows;
    d.rows = g.out_h - d.row0 < p.rows ? g.out_h - d.row0 : p.rows;
    const uint32_t y_hi = (d.row0 + d.rows) * g.bin_y < g.height ? (d.row0 + d.rows) * g.bin_y : g.height;
    d.p_lo = d.row0 * g.bin_y * g.width;
    d.p_hi = y_hi * g.width;
    return d;
}

// The block that starts at pixel `first` of its frame and holds nr values (value(i): value i < nr as the accumulator type Acc,
// signed values sign-extended: sums are two's complement) into the band d: add(index, sum) once per stretch of pixels of one bin
// whose pixels lie inside the band and whose sum is not zero.  One running sum and one guarded add per position, so that lanes
// whose bins change at different positions share the same twelve add sites.  Indices are computed modulo 2^32: a pixel in front of
// the band has a "negative" row, and the first pixel of the band comes out at 0.
template <class Acc, class Value, class Add>
TRPX_HD inline void binned_map(uint32_t first, uint32_t nr, Value&& value, const BinnedGeom& g, const BinnedBand& d, Add&& add) {
    const uint32_t y = first / g.width;
    uint32_t x = first - y * g.width;
    const uint32_t row = y / g.bin_y;
    uint32_t ry = y - row * g.bin_y;
    uint32_t col = x / g.bin_x;
    uint32_t rx = x - col * g.bin_x;
    uint32_t idx = (row - d.row0) * g.out_w + col;
    // the values of the block that lie inside the band: [lo, hi)
    const uint32_t lo = d.p_lo > first ? d.p_lo - first : 0u;
    const uint32_t behind = d.p_hi > first ? d.p_hi - first : 0u;
    const uint32_t hi = behind < nr ? behind : nr;
    Acc sum = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < (int)kBinnedBlock; ++i) {
        if ((uint32_t)i >= lo && (uint32_t)i < hi) sum += value(i);
        uint32_t next = idx;                                // the bin of the pixel behind this one
        ++x;
        ++rx;
        if (x == g.width) {                                 // a new row of pixels
            x = 0;
            rx = 0;
            next -= col;
            col = 0;
            if (++ry == g.bin_y) {
                ry = 0;
                next += g.out_w;
            }
        } else if (rx == g.bin_x) {
            rx = 0;
            ++col;
            ++next;
        }
        if (i + 1 == (int)kBinnedBlock || next != idx) {
            if (sum != 0) add(idx, sum);
            sum = 0;
        }
        idx = next;
    }
}

}  // namespace trpx
