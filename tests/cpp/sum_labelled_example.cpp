// trpx::Terse::prolix_sum_labelled (include/trpx/Terse.hpp) from C++: the 2 x 2 real-space binning of a 4 x 6 scan of 35 x 20
// frames of int16 -- 24 frames into 6 sums of 4 frames that do not lie next to each other --, one position masked, against plain
// loops over the original pixels; plus the error conventions.  Needs a GPU: every encode / decode goes through libtrpx_hip.so.
#include <cstdio>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t n = 35 * 20, ny = 4, nx = 6, frames = ny * nx, n_out = (ny / 2) * (nx / 2) + 1;   // (the last output stays empty)
    std::vector<std::int16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i)
        stack[i] = (std::int16_t)(((i * 2654435761u >> 16) & (i % 97 < 30 ? 0xFFFF : 7)) - (i % 5 == 0 ? 3 : 0));
    trpx::Terse t;
    t.push_back(stack.data(), n, frames);

    std::vector<std::uint32_t> labels(frames);
    for (std::size_t y = 0; y < ny; ++y)
        for (std::size_t x = 0; x < nx; ++x) labels[y * nx + x] = (std::uint32_t)((y / 2) * (nx / 2) + x / 2);
    labels[7] = 0xFFFFFFFFu;                               // a blank position: in no sum
    std::vector<std::int64_t> want(n_out * n, 0), got(n_out * n, 77);
    std::vector<std::uint32_t> want_counts(n_out, 0), counts(n_out, 77);
    for (std::size_t f = 0; f < frames; ++f) {
        if (labels[f] >= n_out) continue;
        ++want_counts[labels[f]];
        for (std::size_t p = 0; p < n; ++p) want[labels[f] * n + p] += stack[f * n + p];
    }
    t.prolix_sum_labelled(got.data(), labels.data(), n_out, counts.data());
    REQUIRE(got == want);
    REQUIRE(counts == want_counts);
    REQUIRE(counts[n_out - 1] == 0 && counts[0] == 3);

    std::vector<float> got_f(n_out * n, 77.0f);            // the exact sum, rounded once; no counts
    t.prolix_sum_labelled(got_f.data(), labels.data(), n_out);
    for (std::size_t i = 0; i < got_f.size(); ++i) REQUIRE(got_f[i] == (float)want[i]);

    bool threw = false;
    try { t.prolix_sum_labelled(got.data(), labels.data(), 0); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // no outputs
    threw = false;
    std::vector<std::uint64_t> u(n_out * n);
    try { t.prolix_sum_labelled(u.data(), labels.data(), n_out); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // signed data into unsigned sums
    threw = false;
    try { t.prolix_sum_labelled(got.data(), labels.data(), ((std::size_t)1 << 20) + 1); } catch (std::exception const&) { threw = true; }
    REQUIRE(threw);                                        // more than 2^20 outputs: refused before anything is written
    std::printf("OK sum_labelled example\n");
    return 0;
}
