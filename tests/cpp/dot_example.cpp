// trpx::Terse::prolix_dot (include/trpx/Terse.hpp) from C++: a virtual bright-field image (a disc mask) and the three
// centre-of-mass sums (the maps x, y and 1) of a 4-frame 35 x 20 u16 stack, against plain loops over the original pixels; plus
// the error convention.  Needs a GPU: every encode / decode goes through libtrpx_hip.so.
#include <cstdio>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t width = 35, height = 20, n = width * height, frames = 4;
    std::vector<std::uint16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i) stack[i] = (std::uint16_t)((i * 2654435761u >> 20) & (i % 97 < 30 ? 0xFFFF : 7));
    trpx::Terse t;
    t.push_back(stack.data(), n, frames);

    // bright field: the pixels within 6 of (17, 10)
    std::vector<std::int32_t> disc(n);
    for (std::size_t y = 0; y < height; ++y)
        for (std::size_t x = 0; x < width; ++x) {
            const long dx = (long)x - 17, dy = (long)y - 10;
            disc[y * width + x] = dx * dx + dy * dy <= 36 ? 1 : 0;
        }
    const std::vector<std::int64_t> bf = t.prolix_dot(disc, 1);
    REQUIRE(bf.size() == frames);
    for (std::size_t f = 0; f < frames; ++f) {
        std::int64_t want = 0;
        for (std::size_t p = 0; p < n; ++p) want += (std::int64_t)stack[f * n + p] * disc[p];
        REQUIRE(bf[f] == want);
    }

    // centre of mass: sum x * px, sum y * px, sum px
    std::vector<std::int32_t> com(3 * n);
    for (std::size_t p = 0; p < n; ++p) { com[p] = (std::int32_t)(p % width); com[n + p] = (std::int32_t)(p / width); com[2 * n + p] = 1; }
    std::vector<std::int64_t> sums(frames * 3);
    t.prolix_dot(com.data(), 3, sums.data());
    for (std::size_t f = 0; f < frames; ++f) {
        std::int64_t sx = 0, sy = 0, s1 = 0;
        for (std::size_t p = 0; p < n; ++p) {
            const std::int64_t v = stack[f * n + p];
            sx += v * (std::int64_t)(p % width); sy += v * (std::int64_t)(p / width); s1 += v;
        }
        REQUIRE(sums[3 * f] == sx && sums[3 * f + 1] == sy && sums[3 * f + 2] == s1);
        REQUIRE(s1 > 0);
    }

    bool threw = false;
    try { t.prolix_dot(disc, 2); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // one map given, two asked for
    threw = false;
    try { std::vector<std::int64_t> o(frames * 17); std::vector<std::int32_t> w(17 * n, 1); t.prolix_dot(w.data(), 17, o.data()); }
    catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // more than 16 maps
    std::printf("OK dot example\n");
    return 0;
}
