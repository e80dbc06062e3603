// trpx::Terse::select (include/trpx/Terse.hpp) from C++: the hit / blank step behind prolix_dot -- keep the frames whose summed
// intensity passes a line, reorder and repeat a few -- on a 6-frame 35 x 20 u16 stack, against the original pixels and against
// an object built from those pixels directly; plus the error convention.  Needs a GPU: every call goes through libtrpx_hip.so.
#include <cstdio>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t width = 35, height = 20, n = width * height, frames = 6;
    std::vector<std::uint16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i)          // odd frames are "hits": a few bright pixels
        stack[i] = (std::uint16_t)((i * 2654435761u >> 20) & ((i / n) % 2 && i % 97 < 30 ? 0xFFFF : 7));
    trpx::Terse t;
    t.dim({width, height});
    t.push_back(stack.data(), n, frames);

    // the picker: per-frame dose from the stream, then the list of hits
    const std::vector<std::int64_t> dose = t.prolix_dot(std::vector<std::int32_t>(n, 1), 1);
    std::vector<std::uint32_t> hits;
    for (std::uint32_t f = 0; f < frames; ++f)
        if (dose[f] > (std::int64_t)(8 * n)) hits.push_back(f);
    REQUIRE(hits.size() == 3 && hits[0] == 1 && hits[1] == 3 && hits[2] == 5);

    trpx::Terse kept = t.select(hits);
    REQUIRE(kept.number_of_frames() == hits.size() && kept.size() == n && kept.dim() == t.dim());
    REQUIRE(!kept.is_signed() && kept.bits_per_val() == t.bits_per_val());
    std::vector<std::uint16_t> back(hits.size() * n), want(hits.size() * n);
    for (std::size_t i = 0; i < hits.size(); ++i) std::copy_n(stack.data() + hits[i] * n, n, want.data() + i * n);
    kept.prolix_all(back.data());
    REQUIRE(back == want);
    trpx::Terse direct;                                    // the same frames encoded from their pixels: the same bytes
    direct.push_back(want.data(), n, hits.size());
    REQUIRE(kept.data() == direct.data() && kept.frame_sizes() == direct.frame_sizes());

    // any order, repeats, more entries than frames
    const std::vector<std::uint32_t> list = {5, 0, 0, 2, 5, 4, 1, 3, 0};
    trpx::Terse longer = t.select(list);
    REQUIRE(longer.number_of_frames() == list.size());
    std::vector<std::uint16_t> one(n);
    for (std::size_t i = 0; i < list.size(); ++i) {
        longer.prolix(one.begin(), i);
        REQUIRE(std::equal(one.begin(), one.end(), stack.begin() + list[i] * n));
    }

    REQUIRE(t.select(std::vector<std::uint32_t>{}).number_of_frames() == 0);
    bool threw = false;
    try { t.select(std::vector<std::uint32_t>{1, 6}); } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // entry 6 of a 6-frame stack
    std::printf("OK select example\n");
    return 0;
}
