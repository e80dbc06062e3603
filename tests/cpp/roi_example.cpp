// trpx::Terse::prolix_roi (include/trpx/Terse.hpp) from C++: the same rectangle of some frames of a 3-frame 35 x 20 u16 stack
// against the crop of the original pixels, into a pointer and into a container iterator, plus the error conventions.
// Needs a GPU: every encode / decode goes through libtrpx_hip.so.
#include <cstdio>
#include <list>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t width = 35, height = 20, n = width * height;
    std::vector<std::uint16_t> stack(3 * n);
    for (std::size_t i = 0; i < stack.size(); ++i) stack[i] = (std::uint16_t)((i * 2654435761u >> 20) & (i % 97 < 30 ? 0xFFFF : 7));
    trpx::Terse t;
    t.push_back(stack.data(), n, 3);
    bool threw = false;
    std::vector<std::uint16_t> got(3 * 6 * 9);
    try { t.prolix_roi(got.data(), 3, 5, 6, 9); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // no dim() yet
    t.dim({width, height});
    auto crop = [&](std::size_t f0, std::size_t nf, std::size_t y0, std::size_t x0, std::size_t h, std::size_t w) {
        std::vector<std::uint16_t> c;
        for (std::size_t f = f0; f < f0 + nf; ++f)
            for (std::size_t y = y0; y < y0 + h; ++y)
                for (std::size_t x = x0; x < x0 + w; ++x) c.push_back(stack[f * n + y * width + x]);
        return c;
    };
    t.prolix_roi(got.data(), 3, 5, 6, 9);
    REQUIRE(got == crop(0, 3, 3, 5, 6, 9));
    std::list<std::uint16_t> tail(2 * 4 * 35);             // frames 1 and 2, four whole rows that end in the last pixel
    t.prolix_roi(tail.begin(), 16, 0, 4, 35, 1);
    const std::vector<std::uint16_t> want = crop(1, 2, 16, 0, 4, 35);
    REQUIRE(std::equal(tail.begin(), tail.end(), want.begin()));
    threw = false;
    try { t.prolix_roi(got.data(), 15, 5, 6, 9); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // y0 + h > height
    threw = false;
    try { std::vector<std::int16_t> wrong(3 * 6 * 9); t.prolix_roi(wrong.data(), 3, 5, 6, 9); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // not the stream's type
    std::printf("OK roi example\n");
    return 0;
}
