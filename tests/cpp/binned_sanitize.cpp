// Sanitizer tier of trpx_decode_binned (CPU build only: g++ -fsanitize=address,undefined; no HIP, no GPU): what a lane does with a
// block and how a frame is cut into bands -- trpx_amd/csrc/binned_map.hpp, the text the kernel runs.  This program walks frames
// block by block and band by band as the lanes would, every band into a heap array of EXACTLY its rows x out_w accumulators, so an
// index one past a band is an ASan report; a wrong sum, an add of zero or an add from a block that has no pixel in the band is a
// FAILED line.  The truth is a plain double loop over the pixels.  Exit status 0 only when neither happens.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <type_traits>
#include <utility>
#include <vector>

#include "binned_map.hpp"

static int failures = 0;
static long cases = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// One frame of h x w values of T under one bin, cut into bands of `rows` output rows: block by block through binned_map() against
// the plain loop.  Acc: uint32_t for types of up to 16 bits, uint64_t for 32-bit types, as in the kernel.
template <class T>
static void run(std::vector<T> const& px, uint32_t h, uint32_t w, uint32_t bin_y, uint32_t bin_x, uint32_t rows) {
    using Acc = std::conditional_t<sizeof(T) == 4, uint64_t, uint32_t>;
    using SAcc = std::make_signed_t<Acc>;
    const uint32_t n = h * w;
    const trpx::BinnedGeom g = trpx::binned_geom(n, w, bin_y, bin_x);
    EXPECT(g.height == h && g.out_h == (h + bin_y - 1) / bin_y && g.out_w == (w + bin_x - 1) / bin_x);
    std::vector<Acc> want((size_t)g.out_h * g.out_w, 0);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) want[(size_t)(y / bin_y) * g.out_w + x / bin_x] += (Acc)(SAcc)px[(size_t)y * w + x];
    const trpx::BinnedPlan plan{rows, (g.out_h + rows - 1) / rows};
    const uint32_t n_blocks = (n + trpx::kBinnedBlock - 1) / trpx::kBinnedBlock;
    uint32_t covered = 0;
    for (uint32_t b = 0; b < plan.bands; ++b) {
        const trpx::BinnedBand d = trpx::binned_band(g, plan, b);
        EXPECT(d.rows >= 1 && d.rows <= rows && d.p_lo == covered && d.p_hi > d.p_lo && d.p_hi <= n && d.p_lo % w == 0 && d.p_hi % w == 0);
        covered = d.p_hi;
        const size_t n_acc = (size_t)d.rows * g.out_w;
        Acc* acc = new Acc[n_acc]();                        // exactly the band's accumulators
        // the blocks around the band (one to either side: they add nothing); the first split of a frame walks every block
        const uint32_t b_lo = rows == 1 || d.p_lo < trpx::kBinnedBlock ? 0 : d.p_lo / trpx::kBinnedBlock - 1;
        const uint32_t b_hi = rows == 1 ? n_blocks : (d.p_hi / trpx::kBinnedBlock + 2 < n_blocks ? d.p_hi / trpx::kBinnedBlock + 2 : n_blocks);
        for (uint32_t blk = b_lo; blk < b_hi; ++blk) {
            const uint32_t first = blk * trpx::kBinnedBlock;
            const uint32_t nr = n - first < trpx::kBinnedBlock ? n - first : trpx::kBinnedBlock;
            const bool touches = first < d.p_hi && first + nr > d.p_lo;
            uint32_t adds = 0;
            trpx::binned_map<Acc>(first, nr, [&](int i) { return (Acc)(SAcc)px[first + (uint32_t)i]; }, g, d, [&](uint32_t idx, Acc s) {
                EXPECT(s != 0 && touches);
                acc[idx] += s;                               // (an index outside the band: ASan)
                ++adds;
            });
            EXPECT(adds <= nr);
        }
        for (uint32_t r = 0; r < d.rows; ++r)
            for (uint32_t x = 0; x < g.out_w; ++x) EXPECT(acc[(size_t)r * g.out_w + x] == want[(size_t)(d.row0 + r) * g.out_w + x]);
        delete[] acc;
        ++cases;
    }
    EXPECT(covered == n);
}

template <class T>
static void geometry(uint32_t h, uint32_t w) {
    const T lo = std::numeric_limits<T>::min(), hi = std::numeric_limits<T>::max();
    const uint32_t n = h * w;
    std::vector<std::vector<T>> data;
    data.emplace_back(n, hi);
    data.emplace_back(n, lo);
    std::vector<T> mix(n);
    for (uint32_t p = 0; p < n; ++p) mix[p] = p % 5 == 0 ? lo : p % 5 == 1 ? hi : p % 5 == 2 ? (T)0 : (T)(p * 37 + 1);
    data.push_back(mix);
    for (uint32_t p = 0; p < n; ++p) mix[p] = (p / 7) % 3 == 0 ? (T)0 : p % 2 ? (T)5 : (T)(0 - (T)5);   // zero stretches; signed: stretches that sum to zero
    data.push_back(mix);
    const std::pair<uint32_t, uint32_t> bins[] = {{1, 1}, {2, 2}, {3, 5}, {1, 7}, {7, 1}, {13, 13}, {64, 64}, {h, w}, {h, 1}, {1, w}};
    for (auto [by, bx] : bins) {
        if (by > h || bx > w || by > trpx::kBinnedMaxBin || bx > trpx::kBinnedMaxBin) continue;
        const uint32_t out_h = (h + by - 1) / by;
        for (uint32_t rows = 1; rows <= out_h; ++rows)       // every band split of the frame
            for (auto const& px : data) run<T>(px, h, w, by, bx, rows);
    }
}

// binned_plan(): the bands cover the frame, none is empty, and a band's accumulators fit
static void plans() {
    for (uint32_t h : {1u, 2u, 7u, 64u, 331u, 512u, 1030u, 4096u, 16384u})
        for (uint32_t w : {1u, 12u, 37u, 371u, 512u, 1065u, 4096u, 8192u})
            for (uint32_t by : {1u, 2u, 3u, 13u, 64u})
                for (uint32_t bx : {1u, 2u, 5u, 64u})
                    for (uint64_t frames : {1ull, 3ull, 5ull, 200ull, 2000ull, 1ull << 20}) {
                        if (by > h || bx > w || (uint64_t)h * w >= (1ull << 29)) continue;
                        const trpx::BinnedGeom g = trpx::binned_geom(h * w, w, by, bx);
                        const trpx::BinnedPlan p = trpx::binned_plan(g, frames);
                        EXPECT(p.rows >= 1 && p.bands >= 1 && (uint64_t)p.rows * p.bands >= g.out_h && (uint64_t)p.rows * (p.bands - 1) < g.out_h);
                        EXPECT((uint64_t)p.rows * g.out_w <= trpx::kBinnedAccs);
                        const trpx::BinnedBand last = trpx::binned_band(g, p, p.bands - 1);
                        EXPECT(last.p_hi == h * w && last.rows >= 1);
                        ++cases;
                    }
}

template <class T>
static void type_cases() {
    for (uint32_t w : {1u, 11u, 12u, 13u, 24u, 25u, 37u})   // width 1, widths around 12 (a block is a row, less, more), no multiple
        for (uint32_t h : {1u, 2u, 5u, 13u, 29u}) geometry<T>(h, w);
    geometry<T>(70, 66);                                    // a 64 x 64 bin and its partial neighbours
}

int main() {
    plans();
    type_cases<uint8_t>();
    type_cases<int8_t>();
    type_cases<uint16_t>();
    type_cases<int16_t>();
    type_cases<uint32_t>();
    type_cases<int32_t>();
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("OK binned_sanitize (%ld cases)\n", cases);
    return 0;
}
