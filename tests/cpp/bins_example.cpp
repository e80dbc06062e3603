// trpx::Terse::prolix_bins (include/trpx/Terse.hpp) from C++: the radial profile of a 4-frame 35 x 20 u16 stack about (17, 10) in
// 8 rings with the corners masked, against a plain loop over the original pixels; plus the error convention.  Needs a GPU: every
// encode / decode goes through libtrpx_hip.so.
#include <cstdio>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t width = 35, height = 20, n = width * height, frames = 4, n_bins = 8;
    std::vector<std::uint16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i) stack[i] = (std::uint16_t)((i * 2654435761u >> 20) & (i % 97 < 30 ? 0xFFFF : 7));
    trpx::Terse t;
    t.push_back(stack.data(), n, frames);

    // rings of width 2 about (17, 10); what lies further out than 8 rings is masked
    std::vector<std::uint16_t> labels(n);
    std::size_t masked = 0;
    for (std::size_t y = 0; y < height; ++y)
        for (std::size_t x = 0; x < width; ++x) {
            const long dx = (long)x - 17, dy = (long)y - 10;
            long r = 0;
            while ((r + 1) * (r + 1) <= dx * dx + dy * dy) ++r;
            labels[y * width + x] = r / 2 < (long)n_bins ? (std::uint16_t)(r / 2) : (std::uint16_t)0xFFFF;
            masked += r / 2 >= (long)n_bins;
        }
    REQUIRE(masked > 0 && masked < n);
    const std::vector<std::int64_t> prof = t.prolix_bins(labels, n_bins);
    REQUIRE(prof.size() == frames * n_bins);
    for (std::size_t f = 0; f < frames; ++f) {
        std::vector<std::int64_t> want(n_bins, 0);
        for (std::size_t p = 0; p < n; ++p)
            if (labels[p] < n_bins) want[labels[p]] += stack[f * n + p];
        for (std::size_t b = 0; b < n_bins; ++b) REQUIRE(prof[f * n_bins + b] == want[b]);
        REQUIRE(want[0] > 0);
    }

    bool threw = false;
    try { std::vector<std::uint16_t> few(n - 1); t.prolix_bins(few, n_bins); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // a map of another size
    threw = false;
    try { t.prolix_bins(labels, 4097); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // more than 4096 bins
    threw = false;
    try { t.prolix_bins(labels, 0); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);
    std::printf("OK bins example\n");
    return 0;
}
