// Sanitizer tier of trpx_decode_sum_labelled (CPU build only: g++ -fsanitize=address,undefined; no HIP, no GPU): what the call
// decides about runs -- where a chunk's runs begin and end, which flush is direct, which slot a partial takes, which partials the
// merge adds: trpx_amd/csrc/label_runs.hpp, the text the kernels run.  This program runs a model of the call over small integer
// "frames": the frames with an output in the order of their labels (any order inside a label), that order cut into chunks of fpc
// positions, every chunk walked as k_sum_labelled walks it -- a flush whenever the label changes and at the chunk's end, direct
// into an output of EXACTLY n_out x values elements or into a slab of EXACTLY chunks x 2 x values on the heap --, then the merge.
// An index one past either is an ASan report, a wrong sum, an output written twice or never, a slot used twice or a partial
// that nobody adds a FAILED line.  Exit status 0 only when none of that happens.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <random>
#include <vector>

#include "label_runs.hpp"

static int failures = 0;
static long cases = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const uint32_t kMask = 0xFFFFFFFFu;
static const size_t kValues = 3;
static int64_t pixel(size_t f, size_t p) { return (int64_t)((f * 7 + p * 3 + 1) % 23) - 5; }

static void run(std::vector<uint32_t> const& labels, uint32_t n_out, uint32_t fpc, uint32_t seed) {
    const size_t n_frames = labels.size();
    ++cases;
    // the truth: the direct sums
    std::vector<int64_t> want((size_t)n_out * kValues, 0);
    std::vector<uint32_t> want_counts(n_out, 0);
    for (size_t f = 0; f < n_frames; ++f)
        if (labels[f] < n_out) {
            ++want_counts[labels[f]];
            for (size_t p = 0; p < kValues; ++p) want[labels[f] * kValues + p] += pixel(f, p);
        }
    // the order: histogram, exclusive scan, scatter -- the frames of a label in an arbitrary order, as the cursors leave them
    std::vector<uint32_t> starts(n_out + 1, 0);
    for (uint32_t l = 0; l < n_out; ++l) starts[l + 1] = starts[l] + want_counts[l];
    const uint32_t n_kept = starts[n_out];
    std::vector<uint32_t> frames_shuffled(n_frames);
    for (size_t f = 0; f < n_frames; ++f) frames_shuffled[f] = (uint32_t)f;
    std::mt19937 rng(seed);
    std::shuffle(frames_shuffled.begin(), frames_shuffled.end(), rng);
    uint32_t* order = new uint32_t[n_kept ? n_kept : 1];   // exactly the ordered frames
    uint32_t* order_label = new uint32_t[n_kept ? n_kept : 1];
    {
        std::vector<uint32_t> cursor(starts.begin(), starts.end() - 1);
        for (uint32_t f : frames_shuffled)
            if (labels[f] < n_out) { order[cursor[labels[f]]] = f; order_label[cursor[labels[f]]++] = labels[f]; }
    }
    // the plan's chunks come from n_frames, not from how many frames have an output
    const uint32_t n_chunks = (uint32_t)((n_frames + fpc - 1) / fpc);
    int64_t* slab = new int64_t[(size_t)n_chunks * 2 * kValues];          // exactly the partial slab
    int64_t* out = new int64_t[(size_t)n_out * kValues];                  // exactly the output
    std::vector<int> slot_used((size_t)n_chunks * 2, 0), slot_added((size_t)n_chunks * 2, 0), written(n_out, 0);

    // the walk
    for (uint32_t c = 0; c < n_chunks; ++c) {
        uint32_t p0, p1;
        trpx::label_chunk_span(c, fpc, n_kept, &p0, &p1);
        EXPECT(p0 <= p1 && p1 <= n_kept);
        if (p0 >= p1) continue;                                          // behind the last labelled frame
        EXPECT(p0 == (uint64_t)c * fpc);
        int64_t acc[kValues] = {0, 0, 0};
        int partials = 0;
        for (uint32_t i = p0; i < p1; ++i) {
            for (size_t p = 0; p < kValues; ++p) acc[p] += pixel(order[i], p);
            const uint32_t l = order_label[i];
            if (i + 1 != p1 && order_label[i + 1] == l) continue;
            const uint32_t s = starts[l], e = starts[l + 1];
            EXPECT(e > s);
            if (trpx::label_run_direct(s, e, fpc)) {
                EXPECT(s >= p0 && e <= p1);                              // all its frames were in this run
                for (size_t p = 0; p < kValues; ++p) out[(size_t)l * kValues + p] = acc[p];
                ++written[l];
            } else {
                const uint32_t slot = trpx::label_run_slot(s, c * fpc);
                EXPECT(slot < 2);
                EXPECT(!slot_used[(size_t)c * 2 + slot]);
                slot_used[(size_t)c * 2 + slot] = 1;
                ++partials;
                for (size_t p = 0; p < kValues; ++p) slab[trpx::label_slab_at(c, slot, kValues) + p] = acc[p];
            }
            for (size_t p = 0; p < kValues; ++p) acc[p] = 0;
        }
        EXPECT(partials <= 2);
    }
    // the merge
    for (uint32_t l = 0; l < n_out; ++l) {
        uint32_t cf = 0, cl = 0;
        const int plan = trpx::label_merge_plan(starts[l], starts[l + 1], fpc, &cf, &cl);
        if (plan == trpx::kLabelDirect) continue;
        int64_t sum[kValues] = {0, 0, 0};
        if (plan == trpx::kLabelMerged) {
            EXPECT(cf < cl && cl < n_chunks);
            for (uint32_t c = cf; c <= cl; ++c) {
                const uint32_t slot = trpx::label_run_slot(starts[l], c * fpc);
                EXPECT(slot_used[(size_t)c * 2 + slot]);
                ++slot_added[(size_t)c * 2 + slot];
                for (size_t p = 0; p < kValues; ++p) sum[p] += slab[trpx::label_slab_at(c, slot, kValues) + p];
            }
        } else EXPECT(plan == trpx::kLabelEmpty && want_counts[l] == 0);
        for (size_t p = 0; p < kValues; ++p) out[(size_t)l * kValues + p] = sum[p];
        ++written[l];
    }
    bool once = true, same = true, slots = true;
    for (uint32_t l = 0; l < n_out; ++l) once = once && written[l] == 1;                     // direct xor merged
    for (size_t i = 0; i < (size_t)n_out * kValues; ++i) same = same && (written[i / kValues] != 1 || out[i] == want[i]);
    for (size_t i = 0; i < slot_used.size(); ++i) slots = slots && slot_used[i] == slot_added[i];   // every partial is added, once
    EXPECT(once);
    EXPECT(same);
    EXPECT(slots);
    delete[] order;
    delete[] order_label;
    delete[] slab;
    delete[] out;
}

static void all_cuts(std::vector<uint32_t> const& labels, uint32_t n_out) {
    uint32_t seed = 1;
    for (uint32_t fpc : {1u, 2u, 5u, 65535u}) run(labels, n_out, fpc, seed++);
}

int main() {
    const size_t n = 37;
    std::vector<uint32_t> lab(n);
    all_cuts(std::vector<uint32_t>(n, 0), 1);                            // all one label
    all_cuts(std::vector<uint32_t>(n, 0), 4);
    all_cuts(std::vector<uint32_t>(n, kMask), 3);                        // all masked
    for (size_t f = 0; f < n; ++f) lab[f] = (uint32_t)(n - 1 - f);
    all_cuts(lab, (uint32_t)n);                                          // every frame its own label
    for (size_t f = 0; f < n; ++f) lab[f] = (uint32_t)(f % 3);
    all_cuts(lab, 3);
    all_cuts(lab, 2);                                                    // ... and label 2 masked by n_out
    for (size_t f = 0; f < n; ++f) lab[f] = (uint32_t)(f / 5);          // boundaries exactly on the cuts of fpc = 5 (and 1)
    all_cuts(lab, 8);
    for (size_t f = 0; f < n; ++f) lab[f] = (uint32_t)(f / 10 * 2);     // ... on every second cut, odd labels empty
    all_cuts(lab, 9);
    // one label over >= 3 chunks with short labels on both sides: 2 + 1 | 17 | 1 + 2 frames, the rest masked
    for (size_t f = 0; f < n; ++f) lab[f] = f < 2 ? 0 : f < 3 ? 1 : f < 20 ? 2 : f < 21 ? 3 : f < 23 ? 4 : kMask;
    all_cuts(lab, 5);
    std::reverse(lab.begin(), lab.end());
    all_cuts(lab, 5);
    for (size_t f = 0; f < n; ++f) lab[f] = (uint32_t)(f % 4 * 25);     // n_out > n_frames, most outputs empty
    all_cuts(lab, 100);
    std::mt19937 rng(20240807);
    for (int round = 0; round < 200; ++round) {
        const size_t frames = 1 + rng() % 60;
        const uint32_t n_out = 1 + rng() % 9;
        std::vector<uint32_t> r(frames);
        for (auto& l : r) l = rng() % 3 == 0 ? kMask : rng() % (n_out + 2);   // (n_out, n_out + 1: masked by the count)
        for (uint32_t fpc : {1u, 2u, 3u, 5u, 7u, 65535u}) run(r, n_out, fpc, (uint32_t)rng());
    }
    // the cut itself: the chunks cover the frames, the 65 535 cap binds for narrow types only
    for (uint64_t frames : {1ull, 3ull, 1024ull, 1025ull, 5000ull, 70000000ull})
        for (uint64_t tpf : {1ull, 2ull, 43ull, 1024ull, 5000ull})
            for (bool narrow : {false, true}) {
                uint32_t chunks = 0;
                const uint32_t fpc = trpx::label_frames_per_chunk(frames, tpf, narrow, &chunks);
                EXPECT(fpc >= 1 && (uint64_t)fpc * chunks >= frames && (uint64_t)fpc * (chunks - 1) < frames);
                EXPECT(!narrow || fpc <= 65535);
            }
    uint32_t chunks = 0;
    EXPECT(trpx::label_frames_per_chunk(70000000, 1, true, &chunks) == 65535 && chunks == 1069);
    EXPECT(trpx::label_frames_per_chunk(70000000, 1, false, &chunks) == 68360 && chunks == 1024);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("OK sum_labelled_sanitize (%ld cases)\n", cases);
    return 0;
}
