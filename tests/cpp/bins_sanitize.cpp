// Sanitizer tier of trpx_decode_bins (CPU build only: g++ -fsanitize=address,undefined; no HIP, no GPU): what a lane does with a
// block -- trpx_amd/csrc/bins_merge.hpp, the text the kernels run: the block's labels out of the map, its support bit, and the
// merge of neighbouring values of equal label into one add.  This program walks frames block by block as the lanes would, over
// heap arrays that END where the frame ends (labels: n_values elements at every 2-byte alignment; values: n_values), so a read
// behind labels[n_values) is an ASan report and a misaligned 8-byte load a UBSan report; a wrong sum is a FAILED line.  Exit status
// 0 only when neither happens.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "bins_merge.hpp"

static int failures = 0;
static long cases = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// n elements whose last one is the last of the allocation, `shift` elements behind an 8-byte boundary
template <class T>
struct Exact {
    void* base = nullptr;
    T* p = nullptr;
    Exact(size_t n, size_t shift) {
        const size_t bytes = (n + shift) * sizeof(T);
        if (posix_memalign(&base, 8, bytes ? bytes : 1)) std::abort();
        p = static_cast<T*>(base) + shift;
    }
    ~Exact() { std::free(base); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

// One frame of n values under one map: block by block through bins_merge.hpp against the plain per-pixel loop.
template <class T>
static void run(std::vector<T> const& values, std::vector<uint16_t> const& map, uint32_t n_bins, size_t shift) {
    const size_t n = values.size();
    Exact<uint16_t> labels(n, shift);
    Exact<T> px(n, 0);
    std::memcpy(labels.p, map.data(), 2 * n);
    std::memcpy(px.p, values.data(), sizeof(T) * n);
    const bool aligned8 = reinterpret_cast<uintptr_t>(labels.p) % 8 == 0;
    EXPECT(aligned8 == (shift % 4 == 0));
    std::vector<uint64_t> got(n_bins, 0), want(n_bins, 0);
    for (size_t p = 0; p < n; ++p)
        if (map[p] < n_bins) want[map[p]] += (uint64_t)(int64_t)values[p];
    for (size_t first = 0; first < n; first += trpx::kBinsBlock) {
        const uint32_t nr = n - first < trpx::kBinsBlock ? (uint32_t)(n - first) : trpx::kBinsBlock;
        const trpx::BinsLabels l = trpx::bins_load_labels(labels.p, first, nr, aligned8);
        bool any = false;
        uint32_t changes = 0;
        for (uint32_t i = 0; i < nr; ++i) {
            EXPECT(trpx::bins_label(l, (int)i) == map[first + i]);
            any = any || map[first + i] < n_bins;
            changes += i == 0 || map[first + i] != map[first + i - 1];
        }
        for (uint32_t i = nr; i < trpx::kBinsBlock; ++i) EXPECT(trpx::bins_label(l, (int)i) == trpx::kBinsNoLabel);
        EXPECT(trpx::bins_any_label(l, n_bins) == any);
        uint32_t adds = 0;
        trpx::bins_merge(nr, [&](int i) { return (uint64_t)(int64_t)px.p[first + i]; }, l, n_bins, [&](uint32_t bin, uint64_t s) {
            EXPECT(bin < n_bins && s != 0);
            if (bin < n_bins) got[bin] += s;
            ++adds;
        });
        EXPECT(adds <= changes);                             // one add per stretch of equal labels at the most
        if (!any) EXPECT(adds == 0);
    }
    EXPECT(got == want);
    ++cases;
}

template <class T>
static void maps_for(std::vector<T> const& values) {
    const size_t n = values.size();
    for (uint32_t n_bins : {1u, 2u, 37u, 4096u}) {
        std::vector<std::vector<uint16_t>> maps;
        maps.emplace_back(n, (uint16_t)0);                                       // all equal
        maps.emplace_back(n, (uint16_t)(n_bins - 1));
        maps.emplace_back(n, (uint16_t)0xFFFF);                                  // all masked
        std::vector<uint16_t> m(n);
        for (size_t p = 0; p < n; ++p) m[p] = (uint16_t)(p % (n_bins + 1));      // all different (n_bins itself: masked)
        maps.push_back(m);
        for (size_t at = 1; at < trpx::kBinsBlock; ++at) {                       // the label changes at position `at` of every block
            for (size_t p = 0; p < n; ++p) m[p] = (uint16_t)(p % trpx::kBinsBlock < at ? 0 : n_bins > 1 ? 1 : 0xFFFF);
            maps.push_back(m);
        }
        for (uint16_t edge : {(uint16_t)(n_bins - 1), (uint16_t)n_bins, (uint16_t)0xFFFF}) {   // the edge labels first and last
            for (size_t p = 0; p < n; ++p) m[p] = 0;
            m[0] = edge;
            maps.push_back(m);
            m[0] = 0;
            m[n - 1] = edge;
            maps.push_back(m);
            m[0] = edge;
            maps.push_back(m);
        }
        for (auto const& map : maps)
            for (size_t shift = 0; shift < 4; ++shift) run<T>(values, map, n_bins, shift);
    }
}

template <class T>
static void type_cases() {
    const T lo = std::numeric_limits<T>::min(), hi = std::numeric_limits<T>::max();
    for (size_t n = 1; n <= 2 * trpx::kBinsBlock; ++n) {       // every block length 1 .. 12, alone and behind a whole block
        maps_for<T>(std::vector<T>(n, (T)0));
        maps_for<T>(std::vector<T>(n, lo));
        maps_for<T>(std::vector<T>(n, hi));
        std::vector<T> mix(n);
        for (size_t p = 0; p < n; ++p) mix[p] = p % 3 == 0 ? lo : p % 3 == 1 ? hi : (T)(p * 37 + 1);
        maps_for<T>(mix);
        for (size_t p = 0; p < n; ++p) mix[p] = p % 2 ? (T)5 : (T)(0 - (T)5);    // (signed: stretches that sum to zero)
        maps_for<T>(mix);
    }
}

int main() {
    type_cases<uint8_t>();
    type_cases<int8_t>();
    type_cases<uint16_t>();
    type_cases<int16_t>();
    type_cases<uint32_t>();
    type_cases<int32_t>();
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("OK bins_sanitize (%ld cases)\n", cases);
    return 0;
}
