// Sanitizer tier of trpx_select_frames (CPU build only: g++ -fsanitize=address,undefined; no HIP, no GPU): the map from an output
// byte to (list slot, source byte) of trpx_amd/csrc/select_map.hpp, the text the copy kernel runs.  This program does what the
// call does -- sizes and verdicts, the scan, then `out` chunk by chunk and line by line exactly as a wavefront's lanes would --
// on heap arrays of their exact sizes (the stream: align4(terse_bytes), what the ABI lets the call read), so a read or a write
// outside them is an ASan report; a wrong byte is a FAILED line.  Exit status 0 only when neither happens.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "select_map.hpp"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

template <class T>
static T* exact(size_t n, size_t align = alignof(T)) {       // n elements and not a byte more, at `align`
    void* p = nullptr;
    if (posix_memalign(&p, align < sizeof(void*) ? sizeof(void*) : align, n ? n * sizeof(T) : 1)) std::abort();
    return static_cast<T*>(p);
}
static uint8_t pattern(uint64_t i) { return (uint8_t)(0xA5u ^ (i * 37u) ^ (i >> 8)); }

enum { kOk = 0, kCapacity = 3 };

struct Stack {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offs;                              // n_frames + 1
    uint64_t terse_bytes;                                    // what the call is told (bad-input cases lie about it)
};
static Stack make_stack(std::vector<uint32_t> const& sizes) {
    Stack s;
    s.offs.push_back(0);
    for (uint32_t z : sizes) {
        for (uint32_t k = 0; k < z; ++k) s.bytes.push_back((uint8_t)rnd());
        s.offs.push_back(s.bytes.size());
    }
    s.terse_bytes = s.bytes.size();
    return s;
}

// One call on exact-size arrays; returns the status.  want_status: what the call has to answer.
static uint32_t run(Stack const& s, std::vector<uint32_t> const& list, uint64_t capacity, uint32_t want_status) {
    const uint64_t n_frames = s.offs.size() - 1, n_select = list.size();
    const uint64_t held = trpx::sel_align4(s.bytes.size());
    uint8_t* terse = exact<uint8_t>(held, 4);
    std::memset(terse, 0, held);
    std::memcpy(terse, s.bytes.data(), s.bytes.size());
    uint64_t* offs = exact<uint64_t>(n_frames + 1);
    std::memcpy(offs, s.offs.data(), 8 * (n_frames + 1));
    uint32_t* frames = exact<uint32_t>(n_select);
    std::memcpy(frames, list.data(), 4 * n_select);
    uint64_t* out_offs = exact<uint64_t>(n_select + 1);
    uint8_t* out = exact<uint8_t>(capacity, 16);
    for (uint64_t i = 0; i < capacity; ++i) out[i] = pattern(i);

    // k_sel_sizes + k_stack_scan + k_sel_verdict
    uint32_t status = 0;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_select; ++i) {
        uint32_t code;
        out_offs[i] = total;
        total += trpx::select_size(frames[i], offs, n_frames, s.terse_bytes, &code);
        if (code > status) status = code;
    }
    out_offs[n_select] = total;
    if (!status && !trpx::select_fits(total, capacity)) status = kCapacity;

    // the truth: the concatenation of the listed frames, bad entries empty
    std::vector<uint8_t> want;
    std::vector<uint64_t> want_offs{0};
    for (uint32_t f : list) {
        if (f < n_frames && s.offs[f] <= s.offs[f + 1] && s.offs[f + 1] <= s.terse_bytes)
            want.insert(want.end(), s.bytes.begin() + s.offs[f], s.bytes.begin() + s.offs[f + 1]);
        want_offs.push_back(want.size());
    }
    EXPECT(status == want_status);
    EXPECT(total == want.size());
    for (uint64_t i = 0; i <= n_select; ++i) EXPECT(out_offs[i] == want_offs[i]);

    // the host form's check of the same list
    uint64_t slot = 0, sum = 0;
    const uint32_t host = trpx::select_check_list(frames, n_select, offs, n_frames, s.terse_bytes, &slot, &sum);
    EXPECT((host != 0) == (status == trpx::kSelInvalid || status == trpx::kSelCorrupt));
    if (!host) EXPECT(sum == total);
    else EXPECT(slot < n_select);

    // k_sel_copy: every chunk, every lane's lines
    if (!status) {
        const uint64_t n_chunks = (trpx::sel_align4(total) + trpx::kSelChunk - 1) / trpx::kSelChunk;
        for (uint64_t c = 0; c < n_chunks; ++c) {
            const uint64_t c0 = c * trpx::kSelChunk;
            const trpx::SelChunkSlots ch = trpx::select_chunk(out_offs, (uint32_t)n_select, c0);
            for (uint32_t line = 0; line < trpx::kSelChunk / trpx::kSelLine; ++line) {
                const uint64_t L = c0 + (uint64_t)line * trpx::kSelLine;
                if (ch.lo == ch.hi) {
                    const trpx::SelSlot s = trpx::select_slot_at(out_offs, frames, offs, ch.lo);
                    if (trpx::select_chunk_whole(s, c0)) trpx::select_store16(out, L, trpx::select_line_whole(terse, s, L));
                    else trpx::select_line_in(terse, out_offs, frames, offs, ch.lo, s, L, total, out);
                } else
                    trpx::select_line(terse, out_offs, frames, offs, ch, L, total, out);
            }
        }
    }
    const uint64_t written = status ? 0 : trpx::sel_align4(total);
    uint64_t wrong = 0;
    for (uint64_t i = 0; i < capacity; ++i) {
        const uint8_t w = i < written ? (i < total ? want[i] : 0) : pattern(i);
        wrong += out[i] != w;
    }
    EXPECT(wrong == 0);
    free(terse); free(offs); free(frames); free(out_offs); free(out);
    return status;
}

// a list at the capacity edges: align4(total) fits, four bytes less and nothing do not
static void edges(Stack const& s, std::vector<uint32_t> const& list) {
    uint64_t total = 0;
    for (uint32_t f : list) total += s.offs[f + 1] - s.offs[f];
    const uint64_t fit = trpx::sel_align4(total);
    run(s, list, fit, kOk);
    run(s, list, fit + 64, kOk);                             // the pattern behind the pad stays
    if (fit >= 4) run(s, list, fit - 4, kCapacity);
    run(s, list, 0, total ? kCapacity : kOk);
}

static std::vector<uint32_t> iota(uint32_t n, uint32_t step = 1) {
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < n; i += step) v.push_back(i);
    return v;
}

int main() {
    // misalignment: 48 frames of about 100 bytes; identity, reverse, every third, a list with repeats longer than the stack
    {
        std::vector<uint32_t> sizes;
        for (int i = 0; i < 48; ++i) sizes.push_back(60 + rnd() % 50);
        const Stack s = make_stack(sizes);
        std::vector<uint32_t> rev = iota(48), rep;
        for (uint32_t i = 0; i < 48; ++i) rev[i] = 47 - i;
        for (int i = 0; i < 77; ++i) rep.push_back(rnd() % 48);
        bool pair[4][4] = {};
        for (auto const& list : {iota(48), rev, iota(48, 3), rep}) {
            uint64_t o = 0;
            for (uint32_t f : list) { pair[s.offs[f] % 4][o % 4] = true; o += s.offs[f + 1] - s.offs[f]; }
            edges(s, list);
        }
        for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) EXPECT(pair[a][b]);   // every (source, destination) residue pair
    }
    // tiny frames: 300 of 1..3 bytes, many boundaries per line; all of one byte
    {
        std::vector<uint32_t> sizes;
        for (int i = 0; i < 300; ++i) sizes.push_back(1 + rnd() % 3);
        const Stack s = make_stack(sizes);
        std::vector<uint32_t> rep;
        for (int i = 0; i < 3000; ++i) rep.push_back(rnd() % 300);                    // more than a chunk of tiny frames
        edges(s, iota(300));
        edges(s, iota(300, 3));
        edges(s, rep);
        const Stack ones = make_stack(std::vector<uint32_t>(300, 1));
        edges(ones, iota(300));
        edges(ones, rep);
    }
    // large frames: each longer than two chunks, [2, 0, 2]
    {
        const Stack s = make_stack({2 * trpx::kSelChunk + 803, 3 * trpx::kSelChunk + 1, 2 * trpx::kSelChunk + 4094});
        edges(s, {2, 0, 2});
        edges(s, {1});
    }
    // the containers' case: 7 frames of about 1000 bytes, and frames that end exactly on line and chunk ends
    {
        std::vector<uint32_t> sizes;
        for (int i = 0; i < 7; ++i) sizes.push_back(900 + rnd() % 300);
        edges(make_stack(sizes), {6, 1, 1, 4, 0});
        const Stack s = make_stack({16, 32, trpx::kSelChunk - 48, trpx::kSelChunk, 5, 11});
        edges(s, iota(6));
        edges(s, {3, 3});
        edges(s, {4, 5, 3, 0});
    }
    // empty frames (legal for the call: offsets that do not move) between others
    {
        Stack s = make_stack({7, 0, 0, 30, 0});
        edges(s, {1, 0, 2, 1, 3, 4, 4});
        edges(s, {1, 2, 4});
    }
    // bad entries: n_frames itself and 0xFFFFFFFF; bad offsets: a decreasing pair, an end beyond the stream
    {
        std::vector<uint32_t> sizes;
        for (int i = 0; i < 12; ++i) sizes.push_back(20 + rnd() % 20);
        const Stack s = make_stack(sizes);
        run(s, {3, 12, 5}, 4096, trpx::kSelInvalid);
        run(s, {3, 0xFFFFFFFFu, 5}, 4096, trpx::kSelInvalid);
        run(s, {12}, 0, trpx::kSelInvalid);                                           // wins over CAPACITY
        Stack dec = s;
        std::swap(dec.offs[4], dec.offs[5]);                                          // frame 4 runs backwards, 3 and 5 changed their sizes
        run(dec, {4}, 4096, trpx::kSelCorrupt);
        run(dec, iota(12), 4096, trpx::kSelCorrupt);
        run(dec, {0, 1, 2, 7}, 4096, kOk);                                            // (only selected frames are judged)
        Stack beyond = s;
        beyond.offs[12] = beyond.terse_bytes + 1;
        run(beyond, {11}, 4096, trpx::kSelCorrupt);
        run(beyond, {11, 12}, 0, trpx::kSelCorrupt);                                  // CORRUPT where both occur
        run(beyond, iota(11), 4096, kOk);
    }
    if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
    std::printf("OK select map checks\n");
    return 0;
}
