// trpx::Terse::prolix_sparse (include/trpx/Terse.hpp) from C++: the pixels at or above a threshold of a 3-frame 35 x 20 u16
// stack, in CSR form, against a scan of the original pixels; thresholds with every pixel, some pixels and no pixel as events,
// plus the error convention.  Needs a GPU: every encode / decode goes through libtrpx_hip.so.
#include <cstdio>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const std::size_t n = 35 * 20, frames = 3;
    std::vector<std::uint16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i) stack[i] = (std::uint16_t)((i * 2654435761u >> 20) & (i % 97 < 30 ? 0xFFFF : 7));
    trpx::Terse t;
    t.push_back(stack.data(), n, frames);
    for (std::int64_t threshold : {std::int64_t(-5), std::int64_t(0), std::int64_t(6), std::int64_t(4096), std::int64_t(65535), std::int64_t(65536)}) {
        std::vector<std::uint64_t> rows, want_rows(1, 0);
        std::vector<std::uint32_t> pos, want_pos;
        std::vector<std::uint16_t> val, want_val;
        for (std::size_t f = 0; f < frames; ++f) {
            for (std::size_t p = 0; p < n; ++p)
                if ((std::int64_t)stack[f * n + p] >= threshold) { want_pos.push_back((std::uint32_t)p); want_val.push_back(stack[f * n + p]); }
            want_rows.push_back(want_pos.size());
        }
        t.prolix_sparse(threshold, rows, pos, val);
        REQUIRE(rows == want_rows);
        REQUIRE(pos == want_pos);
        REQUIRE(val == want_val);
        if (threshold <= 0) REQUIRE(pos.size() == frames * n);         // every pixel
        if (threshold > 65535) REQUIRE(pos.empty());                   // above the type's range: none
    }
    bool threw = false;
    try {
        std::vector<std::uint64_t> rows;
        std::vector<std::uint32_t> pos;
        std::vector<std::int16_t> wrong;
        t.prolix_sparse(6, rows, pos, wrong);
    } catch (std::invalid_argument const&) { threw = true; }
    REQUIRE(threw);                                        // not the stream's type
    std::printf("OK sparse example\n");
    return 0;
}
