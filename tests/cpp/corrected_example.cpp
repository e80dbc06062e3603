// trpx::Terse::prolix_corrected (include/trpx/Terse.hpp) from C++: a 5-frame 35 x 20 i16 stack as float frames with a dark and a
// gain reference applied, the frames [1, 4) alone, and the forms without one or both maps, against a plain loop over the original
// pixels (three float operations, each rounded once); plus the error convention.  Needs a GPU: every encode / decode goes through
// libtrpx_hip.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, 4) == 0; }

int main() {
    const std::size_t n = 35 * 20, frames = 5;
    std::vector<std::int16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i)
        stack[i] = (std::int16_t)((int)((i * 2654435761u >> 20) & (i % 97 < 30 ? 0x3FF : 7)) - (i % 5 == 0 ? 60 : 2));
    trpx::Terse t;
    t.push_back(stack.data(), n, frames);

    std::vector<float> dark(n), gain(n);
    for (std::size_t p = 0; p < n; ++p) {
        dark[p] = (float)(p % 17) + 0.5f;
        gain[p] = p % 13 == 0 ? 0.0f : p % 7 == 0 ? -1.25f : 1.0f + (float)(p % 5) / 64.0f;
    }
    gain[3] = std::numeric_limits<float>::infinity();
    dark[5] = std::numeric_limits<float>::quiet_NaN();

    auto want = [&](std::size_t f, std::size_t p, bool d, bool g) {
        volatile float x = (float)stack[f * n + p];
        if (d) x = x - dark[p];
        if (g) x = x * gain[p];
        return (float)x;
    };
    for (int form = 0; form < 4; ++form) {
        const bool d = form & 1, g = form & 2;
        const std::vector<float> out = t.prolix_corrected(d ? dark.data() : nullptr, g ? gain.data() : nullptr);
        REQUIRE(out.size() == frames * n);
        for (std::size_t f = 0; f < frames; ++f)
            for (std::size_t p = 0; p < n; ++p) REQUIRE(same(out[f * n + p], want(f, p, d, g)));
    }
    const std::vector<float> part = t.prolix_corrected(dark, gain, 1, 3);
    REQUIRE(part.size() == 3 * n);
    for (std::size_t f = 0; f < 3; ++f)
        for (std::size_t p = 0; p < n; ++p) REQUIRE(same(part[f * n + p], want(f + 1, p, true, true)));
    REQUIRE(t.prolix_corrected(dark, gain, 4, 100).size() == n);       // clipped to the stack
    REQUIRE(t.prolix_corrected(dark, gain, 5).empty());

    bool threw = false;
    try { t.prolix_corrected(dark, gain, 6); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // behind the stack
    threw = false;
    try { t.prolix_corrected(std::vector<float>(n - 1), gain); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // a map of another size
    std::printf("OK corrected example\n");
    return 0;
}
