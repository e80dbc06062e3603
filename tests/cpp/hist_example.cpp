// trpx::Terse::prolix_hist (include/trpx/Terse.hpp) from C++: the per-frame histograms, the histograms of pairs of frames (a ragged
// last group) and the stack's histogram of a 5-frame 35 x 20 i16 stack, in 16 bins of 8 counts from -37 on, against a plain loop
// over the original pixels; plus the error convention.  Needs a GPU: every encode / decode goes through libtrpx_hip.so.
#include <cstdio>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t n = 35 * 20, frames = 5, n_bins = 16;
    const std::int64_t lo = -37;
    const unsigned shift = 3;
    std::vector<std::int16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i)
        stack[i] = (std::int16_t)((int)((i * 2654435761u >> 20) & (i % 97 < 30 ? 0x3FF : 7)) - (i % 5 == 0 ? 60 : 2));
    trpx::Terse t;
    t.push_back(stack.data(), n, frames);

    auto bin = [&](std::int64_t v) {
        const std::int64_t q = (v - lo) >> shift;
        return (std::size_t)(q < 0 ? 0 : q >= (std::int64_t)n_bins ? (std::int64_t)n_bins - 1 : q);
    };
    for (std::size_t group : {(std::size_t)1, (std::size_t)2, frames, (std::size_t)100}) {
        const std::size_t per = group < frames ? group : frames, n_groups = (frames + per - 1) / per;
        const std::vector<std::uint64_t> hist = t.prolix_hist(group, lo, shift, n_bins);
        REQUIRE(hist.size() == n_groups * n_bins);
        std::vector<std::uint64_t> want(n_groups * n_bins, 0);
        for (std::size_t f = 0; f < frames; ++f)
            for (std::size_t p = 0; p < n; ++p) ++want[f / per * n_bins + bin(stack[f * n + p])];
        REQUIRE(hist == want);
        REQUIRE(want[0] > 0 && want[n_bins - 1] > 0);      // both clamped ends hold pixels
    }

    bool threw = false;
    try { t.prolix_hist(1, 0, 0, 4097); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // more than 4096 bins
    threw = false;
    try { t.prolix_hist(1, 0, 0, 0); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try { t.prolix_hist(0, 0, 0, 16); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // no group
    threw = false;
    try { t.prolix_hist(1, 0, 33, 16); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);
    std::printf("OK hist example\n");
    return 0;
}
