// trpx::Terse::prolix_binned (include/trpx/Terse.hpp) from C++: a 4-frame 35 x 20 u16 stack binned 3 x 4 (partial edge bins on
// both sides) into int32 and 1 x 1 into double, against a plain loop over the original pixels; plus the error conventions.  Needs
// a GPU: every encode / decode goes through libtrpx_hip.so.
#include <cstdio>
#include <utility>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t width = 35, height = 20, n = width * height, frames = 4;
    std::vector<std::uint16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i) stack[i] = (std::uint16_t)((i * 2654435761u >> 20) & (i % 97 < 30 ? 0xFFFF : 7));
    trpx::Terse t;
    t.push_back(stack.data(), n, frames);
    bool threw = false;
    try { t.prolix_binned(3, 4); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // no dim() yet
    t.dim({width, height});

    const std::size_t bin_y = 3, bin_x = 4, out_h = (height + bin_y - 1) / bin_y, out_w = (width + bin_x - 1) / bin_x;
    REQUIRE(height % bin_y != 0 && width % bin_x != 0);
    const std::vector<std::int32_t> got = t.prolix_binned(bin_y, bin_x);
    REQUIRE(got.size() == frames * out_h * out_w);
    std::vector<std::int32_t> want(got.size(), 0);
    for (std::size_t f = 0; f < frames; ++f)
        for (std::size_t y = 0; y < height; ++y)
            for (std::size_t x = 0; x < width; ++x) want[(f * out_h + y / bin_y) * out_w + x / bin_x] += stack[f * n + y * width + x];
    REQUIRE(got == want);

    const std::vector<double> wide = t.prolix_binned<double>(1, 1);              // a widening decode
    REQUIRE(wide.size() == stack.size());
    for (std::size_t i = 0; i < stack.size(); ++i) REQUIRE(wide[i] == (double)stack[i]);

    for (auto [by, bx] : {std::pair<std::size_t, std::size_t>{0, 1}, {1, 0}, {65, 1}, {21, 1}, {1, 36}}) {
        threw = false;
        try { t.prolix_binned(by, bx); } catch (std::invalid_argument const&) { threw = true; }
        REQUIRE(threw);                                    // a bin side of 0, above 64, above the frame's
    }
    std::printf("OK binned example\n");
    return 0;
}
