// trpx::Terse::prolix_reduce (include/trpx/Terse.hpp) from C++: a 7-frame 35 x 20 stack of int16 (a short last group) reduced in
// groups of 3 with every op, against plain loops over the original pixels; plus the error conventions.  Needs a GPU: every
// encode / decode goes through libtrpx_hip.so.
#include <algorithm>
#include <cstdio>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t n = 35 * 20, frames = 7, group = 3, n_out = (frames + group - 1) / group;
    std::vector<std::int16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i)
        stack[i] = (std::int16_t)(((i * 2654435761u >> 16) & (i % 97 < 30 ? 0xFFFF : 7)) - (i % 5 == 0 ? 3 : 0));
    trpx::Terse t;
    t.push_back(stack.data(), n, frames);

    const std::int64_t threshold = 2;
    std::vector<std::int16_t> want_max(n_out * n), want_min(n_out * n), got_max(n_out * n, 77), got_min(n_out * n, 77);
    std::vector<std::uint64_t> want_sq(n_out * n, 0), got_sq(n_out * n, 77);
    std::vector<std::uint32_t> want_ge(n_out * n, 0), got_ge(n_out * n, 77);
    for (std::size_t j = 0; j < n_out; ++j)
        for (std::size_t p = 0; p < n; ++p) {
            std::int16_t hi = stack[j * group * n + p], lo = hi;
            for (std::size_t f = j * group; f < std::min((j + 1) * group, frames); ++f) {
                const std::int16_t v = stack[f * n + p];
                hi = std::max(hi, v);
                lo = std::min(lo, v);
                want_sq[j * n + p] += (std::uint64_t)((std::int64_t)v * v);
                want_ge[j * n + p] += v >= threshold;
            }
            want_max[j * n + p] = hi;
            want_min[j * n + p] = lo;
        }
    t.prolix_reduce(got_max.data(), TRPX_REDUCE_MAX, group);
    t.prolix_reduce(got_min.data(), TRPX_REDUCE_MIN, group);
    t.prolix_reduce(got_sq.data(), TRPX_REDUCE_SUMSQ, group);
    t.prolix_reduce(got_ge.data(), TRPX_REDUCE_COUNT_GE, group, threshold);
    REQUIRE(got_max == want_max);
    REQUIRE(got_min == want_min);
    REQUIRE(got_sq == want_sq);
    REQUIRE(got_ge == want_ge);

    // a group beyond the stack: one output over all frames
    std::vector<std::int16_t> all(n, 77);
    t.prolix_reduce(all.data(), TRPX_REDUCE_MAX, 100);
    for (std::size_t p = 0; p < n; ++p) {
        std::int16_t hi = stack[p];
        for (std::size_t f = 1; f < frames; ++f) hi = std::max(hi, stack[f * n + p]);
        REQUIRE(all[p] == hi);
    }

    bool threw = false;
    try { t.prolix_reduce(got_max.data(), TRPX_REDUCE_MAX, 0); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // group 0
    threw = false;
    try { t.prolix_reduce(got_max.data(), 4, group); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // an unknown op
    threw = false;
    try { t.prolix_reduce(got_ge.data(), TRPX_REDUCE_MAX, group); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // uint32_t is not what MAX writes for int16 values
    threw = false;
    try { t.prolix_reduce(got_max.data(), TRPX_REDUCE_SUMSQ, group); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // ... nor int16_t what SUMSQ writes
    std::printf("OK reduce example\n");
    return 0;
}
