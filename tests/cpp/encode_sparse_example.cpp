// trpx::Terse::push_back_sparse (include/trpx/Terse.hpp) from C++: the events prolix_sparse gives of a 3-frame 35 x 20 u16
// stack -- threshold 1: the non-zero pixels -- pushed into a new Terse, whose write() output must be the original's byte for
// byte; the same in two pushes, plus the error convention.  Needs a GPU: every encode / decode goes through libtrpx_hip.so.
#include <cstdio>
#include <sstream>
#include <vector>
#include "trpx/Terse.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <typename F> static bool throws_invalid(F&& f) {
    try { f(); } catch (std::invalid_argument const&) { return true; }
    return false;
}

int main() {
    const std::size_t n = 35 * 20, frames = 3;
    std::vector<std::uint16_t> stack(frames * n);
    for (std::size_t i = 0; i < stack.size(); ++i)
        stack[i] = i % 5 == 0 ? (std::uint16_t)((i * 2654435761u >> 20) & (i % 97 < 30 ? 0xFFFF : 7)) : 0;   // four pixels in five are zero
    trpx::Terse dense;
    dense.dim({35, 20});
    dense.push_back(stack.data(), n, frames);
    std::vector<std::uint64_t> rows;
    std::vector<std::uint32_t> pos;
    std::vector<std::uint16_t> val;
    dense.prolix_sparse(1, rows, pos, val);
    REQUIRE(rows.size() == frames + 1 && !pos.empty() && pos.size() < stack.size() / 4);

    trpx::Terse sparse;
    sparse.dim({35, 20});                                  // (the frame size of the first push: the product of dim())
    sparse.push_back_sparse(rows, pos, val);
    REQUIRE(sparse.size() == n && sparse.number_of_frames() == frames && !sparse.is_signed());
    REQUIRE(sparse.bits_per_val() == dense.bits_per_val());
    std::ostringstream a, b;
    dense.write(a);
    sparse.write(b);
    REQUIRE(a.str() == b.str());

    // frame by frame, the size given: rows of a larger CSR keep their absolute indices
    trpx::Terse steps;
    for (std::size_t f = 0; f < frames; ++f) steps.push_back_sparse(std::vector<std::uint64_t>{rows[f], rows[f + 1]}, pos, val, n);
    steps.dim({35, 20});
    std::ostringstream c;
    steps.write(c);
    REQUIRE(a.str() == c.str());
    std::vector<std::uint16_t> back(n);
    steps.prolix(back.begin(), 2);
    REQUIRE(std::equal(back.begin(), back.end(), stack.begin() + 2 * n));

    // an empty frame: no lists at all
    trpx::Terse blank;
    blank.push_back_sparse(std::vector<std::uint64_t>{0, 0}, std::vector<std::uint32_t>{}, std::vector<std::uint16_t>{}, n);
    trpx::Terse zeros;
    std::vector<std::uint16_t> z(n, 0);
    zeros.push_back(z.data(), n);
    std::ostringstream d, e;
    blank.write(d);
    zeros.write(e);
    REQUIRE(d.str() == e.str());

    const std::size_t before = sparse.terse_size();
    REQUIRE(throws_invalid([&] { sparse.push_back_sparse(std::vector<std::uint64_t>{0, 2}, std::vector<std::uint32_t>{7, 7}, std::vector<std::uint16_t>{1, 1}); }));   // a duplicate
    REQUIRE(throws_invalid([&] { sparse.push_back_sparse(std::vector<std::uint64_t>{0, 1}, std::vector<std::uint32_t>{(std::uint32_t)n}, std::vector<std::uint16_t>{1}); }));   // out of range
    REQUIRE(throws_invalid([&] { sparse.push_back_sparse(std::vector<std::uint64_t>{0, 1}, std::vector<std::uint32_t>{1}, std::vector<std::int16_t>{1}); }));   // signedness
    REQUIRE(throws_invalid([&] { trpx::Terse t; t.push_back_sparse(rows, pos, val); }));                   // no frame size
    REQUIRE(sparse.terse_size() == before && sparse.number_of_frames() == frames);
    std::printf("OK encode sparse example\n");
    return 0;
}
