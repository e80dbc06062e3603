// Sanitizer tier of trpx_decode_hist (CPU build only: g++ -fsanitize=address,undefined; no HIP, no GPU): the bin rule --
// trpx_amd/csrc/hist_bin.hpp, the text the kernel runs.  Four checks:
//   1. for both signednesses, every width 0 .. 32 and a fixed list of (lo, shift, n_bins): hist_block_one_bin is true exactly when
//      the two ends of the width's value range have the same bin (and names that bin);
//   2. for the widths <= 8: EVERY value of the range lands in the promised bin (and where the rule says no, two values differ);
//   3. where the 32-bit form of the rule applies (hist_narrow_ok: pixels of at most 16 bits, |lo| <= 2^30), hist_bin32 is hist_bin
//      for EVERY value an 8- or 16-bit pixel can take;
//   4. the merged lane count of random blocks of 1 .. 12 values (hist_count_block) equals a plain loop, into exact-size heap
//      arrays of counters, with at most one add per change of bin.
// A signed overflow or an oversized shift is a UBSan report, a counter outside [0, n_bins) an ASan report, a wrong answer a FAILED
// line.  Exit status 0 only when none happens.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "hist_bin.hpp"

static int failures = 0;
static long cases = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Rule { int64_t lo; uint32_t shift, n_bins; };

static std::vector<Rule> rules() {
    std::vector<Rule> r;
    const int64_t los[] = {0, 1, -1, -37, 100, 255, -128, 127, 65535, -32768, 32767, (int64_t)1 << 30, -((int64_t)1 << 30), 4294967295ll,
                           -2147483648ll, 2147483647ll, (int64_t)1 << 32, -((int64_t)1 << 32)};   // each type's min and max, and the limits of lo
    for (int64_t lo : los)
        for (uint32_t shift : {0u, 1u, 3u, 4u, 8u, 16u, 31u, 32u})
            for (uint32_t n_bins : {1u, 2u, 3u, 16u, 256u, 4096u}) r.push_back({lo, shift, n_bins});
    return r;
}

// the plain definition: floor division by 2^shift in wide arithmetic, then the clamp
static uint32_t plain_bin(int64_t v, Rule const& k) {
    const __int128 d = (__int128)v - k.lo, p = (__int128)1 << k.shift;
    __int128 q = d / p;
    if (d % p != 0 && d < 0) --q;
    return q < 0 ? 0u : q >= (__int128)k.n_bins ? k.n_bins - 1 : (uint32_t)q;
}

static void widths() {
    for (Rule const& k : rules()) {
        EXPECT(trpx::hist_args_ok(k.lo, k.shift, k.n_bins));
        for (int sg = 0; sg < 2; ++sg)
            for (uint32_t w = 0; w <= 32; ++w) {
                const int64_t lo_v = trpx::hist_width_min(w, sg != 0), hi_v = trpx::hist_width_max(w, sg != 0);
                // the convention: unsigned [0, 2^w - 1], signed [-2^(w-1), 2^(w-1) - 1], width 0 {0}
                EXPECT(lo_v == (w == 0 || !sg ? 0 : -((int64_t)1 << (w - 1))));
                EXPECT(hi_v == (w == 0 ? 0 : sg ? ((int64_t)1 << (w - 1)) - 1 : ((int64_t)1 << w) - 1));
                EXPECT(trpx::hist_bin(lo_v, k.lo, k.shift, k.n_bins) == plain_bin(lo_v, k));
                EXPECT(trpx::hist_bin(hi_v, k.lo, k.shift, k.n_bins) == plain_bin(hi_v, k));
                uint32_t bin = 0xDEADu;
                const bool one = trpx::hist_block_one_bin(w, sg != 0, k.lo, k.shift, k.n_bins, &bin);
                EXPECT(one == (plain_bin(lo_v, k) == plain_bin(hi_v, k)));
                if (one) EXPECT(bin == plain_bin(lo_v, k) && bin < k.n_bins);
                if (w == 0) EXPECT(one && bin == plain_bin(0, k));
                if (k.n_bins == 1) EXPECT(one && bin == 0);
                if (w <= 8) {                               // every value of the range
                    bool all_same = true;
                    for (int64_t v = lo_v; v <= hi_v; ++v) {
                        const uint32_t b = trpx::hist_bin(v, k.lo, k.shift, k.n_bins);
                        EXPECT(b == plain_bin(v, k) && b < k.n_bins);
                        if (one) EXPECT(b == bin);
                        all_same = all_same && b == plain_bin(lo_v, k);
                    }
                    EXPECT(all_same == one);
                }
                ++cases;
            }
    }
    // outside the limits
    EXPECT(!trpx::hist_args_ok(0, 0, 0) && !trpx::hist_args_ok(0, 0, 4097) && !trpx::hist_args_ok(0, 33, 16));
    EXPECT(!trpx::hist_args_ok(((int64_t)1 << 32) + 1, 0, 16) && !trpx::hist_args_ok(-((int64_t)1 << 32) - 1, 0, 16));
    EXPECT(!trpx::hist_args_ok(std::numeric_limits<int64_t>::min(), 0, 16) && !trpx::hist_args_ok(std::numeric_limits<int64_t>::max(), 0, 16));
}

static void narrow() {
    long applies = 0;
    for (Rule const& k : rules()) {
        EXPECT(!trpx::hist_narrow_ok(k.lo, 32));
        EXPECT(trpx::hist_narrow_ok(k.lo, 8) == trpx::hist_narrow_ok(k.lo, 16));
        if (!trpx::hist_narrow_ok(k.lo, 16)) {
            EXPECT(k.lo > ((int64_t)1 << 30) || k.lo < -((int64_t)1 << 30));
            continue;
        }
        ++applies;
        bool same = true;
        for (int64_t v = -32768; v <= 65535; ++v)           // every int8 / uint8 / int16 / uint16 value
            same = same && trpx::hist_bin32((int32_t)v, (int32_t)k.lo, k.shift, k.n_bins) == trpx::hist_bin(v, k.lo, k.shift, k.n_bins);
        EXPECT(same);
        ++cases;
    }
    EXPECT(applies > 0);
    EXPECT(trpx::hist_narrow_ok((int64_t)1 << 30, 16) && !trpx::hist_narrow_ok(((int64_t)1 << 30) + 1, 16));
    EXPECT(trpx::hist_narrow_ok(-((int64_t)1 << 30), 16) && !trpx::hist_narrow_ok(-((int64_t)1 << 30) - 1, 16));
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

template <class T>
static void blocks() {
    const T lo_t = std::numeric_limits<T>::min(), hi_t = std::numeric_limits<T>::max();
    for (Rule const& k : rules()) {
        for (int rep = 0; rep < 6; ++rep) {
            const uint32_t nr = 1 + (uint32_t)(rng() % trpx::kBinsBlock);
            T* v = static_cast<T*>(std::malloc(nr * sizeof(T)));                 // exact size: a read behind nr is an ASan report
            uint64_t* got = static_cast<uint64_t*>(std::calloc(k.n_bins, 8));    // exact size: a bin >= n_bins is one too
            std::vector<uint64_t> want(k.n_bins, 0);
            const int kind = rep % 3;                       // small values around lo's bin edges, the type's extremes, anything
            for (uint32_t i = 0; i < nr; ++i) {
                const uint64_t r = rng();
                v[i] = kind == 0 ? (T)(r % 5) : kind == 1 ? (r & 1 ? lo_t : hi_t) : (T)r;
                if (r % 7 == 0 && i) v[i] = v[i - 1];       // stretches of equal values
            }
            uint32_t changes = 0, adds = 0;
            for (uint32_t i = 0; i < nr; ++i) {
                ++want[plain_bin((int64_t)v[i], k)];
                changes += i == 0 || plain_bin((int64_t)v[i], k) != plain_bin((int64_t)v[i - 1], k);
            }
            trpx::hist_count_block(nr, [&](int i) { return (int64_t)v[i]; }, k.lo, k.shift, k.n_bins, [&](uint32_t bin, uint32_t n) {
                EXPECT(bin < k.n_bins && n >= 1 && n <= nr);
                got[bin] += n;
                ++adds;
            });
            EXPECT(adds == changes);                         // one add per stretch of equal bins
            bool same = true;
            for (uint32_t b = 0; b < k.n_bins; ++b) same = same && got[b] == want[b];
            EXPECT(same);
            if (sizeof(T) <= 2 && trpx::hist_narrow_ok(k.lo, 8 * sizeof(T))) {   // the 32-bit form, as the kernel calls it
                std::vector<uint64_t> got32(k.n_bins, 0);
                trpx::hist_count_bins(nr, [&](int i) { return trpx::hist_bin32((int32_t)v[i], (int32_t)k.lo, k.shift, k.n_bins); }, k.n_bins,
                                      [&](uint32_t bin, uint32_t n) { got32.at(bin) += n; });
                EXPECT(got32 == want);
            }
            std::free(v);
            std::free(got);
            ++cases;
        }
    }
}

int main() {
    widths();
    narrow();
    blocks<uint8_t>();
    blocks<int8_t>();
    blocks<uint16_t>();
    blocks<int16_t>();
    blocks<uint32_t>();
    blocks<int32_t>();
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("OK hist_sanitize (%ld cases)\n", cases);
    return 0;
}
