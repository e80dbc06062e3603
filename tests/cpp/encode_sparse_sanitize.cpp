// Host-code sanitizer tier of trpx_encode_sparse_host (CPU build only: g++ -fsanitize=address,undefined; no HIP, no GPU): the
// event validation, the size bound and the staging layout of trpx_amd/csrc/sparse_events.hpp, which api.hip runs on the caller's lists before a
// device is looked for.  Every list sits in a heap allocation of its exact size, so a read outside row_offsets[0 .. n_frames] or
// positions[0 .. n_events) is an ASan report; a wrong verdict is a FAILED line.  Exit status 0 only when neither happens.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse_events.hpp"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// verdict on exact-size copies of the lists
static const char* verdict(std::vector<uint64_t> const& rows, std::vector<uint32_t> const& pos, uint64_t n_events, uint64_t n_values) {
    uint64_t* r = new uint64_t[rows.size()];
    uint32_t* p = pos.empty() ? nullptr : new uint32_t[pos.size()];
    std::memcpy(r, rows.data(), 8 * rows.size());
    if (p) std::memcpy(p, pos.data(), 4 * pos.size());
    uint64_t frame = 0, event = 0;
    const char* why = trpx::bad_events(r, p, n_events, n_values, rows.size() - 1, &frame, &event);
    if (why) EXPECT(frame <= rows.size() - 1 && event <= n_events);
    delete[] r;
    delete[] p;
    return why;
}

int main() {
    const uint64_t n_values = 6149;
    // three good rows: 4, 0 and 3 events; the lists start with two events of no frame
    const std::vector<uint64_t> rows{2, 6, 6, 9};
    const std::vector<uint32_t> pos{0xFFFFFFFFu, 0xFFFFFFFFu, 0, 11, 3072, 6148, 5, 6, 7};
    EXPECT(verdict(rows, pos, 9, n_values) == nullptr);
    EXPECT(verdict(rows, pos, 12, n_values + 1) == nullptr);               // (n_events beyond the last row is legal; never read)
    EXPECT(verdict({0, 0, 0}, {}, 0, n_values) == nullptr);                // empty frames, no lists
    // each condition alone
    { auto p = pos; p[5] = (uint32_t)n_values; EXPECT(verdict(rows, p, 9, n_values)); }
    { auto p = pos; p[8] = 0xFFFFFFFFu; EXPECT(verdict(rows, p, 9, n_values)); }
    { auto p = pos; std::swap(p[3], p[4]); EXPECT(verdict(rows, p, 9, n_values)); }
    { auto p = pos; p[7] = p[6]; EXPECT(verdict(rows, p, 9, n_values)); }
    { auto r = rows; r[2] = 5; EXPECT(verdict(r, pos, 9, n_values)); }    // a decreasing row
    { auto r = rows; r[3] = 10; EXPECT(verdict(r, pos, 9, n_values)); }   // ends beyond the events
    EXPECT(verdict({0, 100, 5}, {1, 2, 3, 4, 5}, 5, n_values));            // a row that leaves the lists although the end fits: nothing read there
    EXPECT(verdict({~0ull, ~0ull}, {}, 0, n_values));                      // offsets near 2^64
    EXPECT(verdict({7, 3}, {1, 2, 3}, 3, n_values));
    // random lists, bent at random: the verdict is that of a plain scan of the same lists
    for (int round = 0; round < 2000; ++round) {
        const uint64_t n_frames = 1 + rnd() % 5, nv = 1 + rnd() % 40;
        std::vector<uint64_t> r(n_frames + 1);
        std::vector<uint32_t> p;
        r[0] = rnd() % 3;
        for (uint64_t i = 0; i < r[0]; ++i) p.push_back(rnd());
        for (uint64_t f = 0; f < n_frames; ++f) {
            for (uint32_t x = 0; x < nv; ++x)
                if (rnd() % 3 == 0) p.push_back(x);
            r[f + 1] = p.size();
        }
        uint64_t n_events = p.size();
        bool want_bad = false;
        switch (rnd() % 6) {
        case 0: if (!p.empty()) { p[rnd() % p.size()] = rnd() % (2 * nv); } break;
        case 1: r[rnd() % r.size()] = rnd() % (n_events + 3); break;
        case 2: if (n_events) --n_events; break;
        default: break;
        }
        if (r[n_frames] > n_events) want_bad = true;
        for (uint64_t f = 0; f < n_frames && !want_bad; ++f) want_bad = r[f] > r[f + 1];
        for (uint64_t f = 0; f < n_frames && !want_bad; ++f)
            for (uint64_t i = r[f]; i < r[f + 1] && !want_bad; ++i) want_bad = p[i] >= nv || (i > r[f] && p[i - 1] >= p[i]);
        p.resize(n_events);                                                 // exactly the lists the call may read
        EXPECT((verdict(r, p, n_events, nv) != nullptr) == want_bad);
    }
    // the bound: arithmetic at the edges of its range
    EXPECT(trpx::sparse_bound_bytes(2, 21846, 1, 0, 1 << 30) == (1 + 21846 / 8 + 15) / 16 * 16);
    EXPECT(trpx::sparse_bound_bytes(4, 1, 1, 0, 7) == 16);
    EXPECT(trpx::sparse_bound_bytes(4, 0xFFFFFFFFull, 0x7FFFFFFFull, ~0ull, (1ull << 62) + 3) == (1ull << 62) + 16);   // clamped, no wrap
    EXPECT(trpx::sparse_bound_bytes(1, 3, 2, 5, 1000) == (2 + (2 * 3 + 5 * (14 + 96)) / 8 + 15) / 16 * 16);
    // the host form's staging layout: parts in order, aligned, non-overlapping, exactly as long as the lists; too-long lists refused
    for (int round = 0; round < 2000; ++round) {
        const uint64_t f = 1 + rnd() % 5000, e = rnd() % 100000;
        const size_t es = (size_t)1 << (rnd() % 3);
        trpx::SparseStaging l{};
        EXPECT(trpx::sparse_staging(f, e, es, &l));
        EXPECT(l.pos_at % 16 == 0 && l.val_at % 16 == 0 && l.pos_at >= 8 * (f + 1) && l.pos_at < 8 * (f + 1) + 16);
        EXPECT(l.val_at >= l.pos_at + 4 * e && l.val_at < l.pos_at + 4 * e + 16 && l.total == l.val_at + es * e);
        std::vector<unsigned char> block(l.total ? l.total : 1);             // what the wrapper allocates: fill each part to its end
        std::memset(block.data(), 1, 8 * (f + 1));
        std::memset(block.data() + l.pos_at, 2, 4 * e);
        std::memset(block.data() + l.val_at, 3, es * e);
    }
    { trpx::SparseStaging l{};
      EXPECT(!trpx::sparse_staging(1, (1ull << 62) / 5 + 1, 1, &l));           // 5 bytes per event reach 2^62
      EXPECT(!trpx::sparse_staging(1, ~0ull, 4, &l));
      EXPECT(!trpx::sparse_staging(~0ull, 0, 2, &l));
      EXPECT(trpx::sparse_staging(0x7FFFFFFFull, (1ull << 40), 4, &l) && l.total == l.val_at + (4ull << 40)); }
    if (failures) { std::printf("%d check(s) FAILED\n", failures); return 1; }
    std::printf("OK encode sparse host checks\n");
    return 0;
}
