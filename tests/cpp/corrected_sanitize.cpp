// Sanitizer tier of trpx_decode_corrected (CPU build only: g++ -fsanitize=address,undefined; no HIP, no GPU): the pixel rule and
// the index arithmetic of the kernel's store step -- trpx_amd/csrc/correct_px.hpp, the text the kernel runs.  Whole frames are
// stored on the host exactly as k_decode_corrected stores them: tile by tile (4 and 2 groups of 256 blocks per tile), round by
// round, wavefront by wavefront, every (lane, round) of the staged form where corr_wave_staged says so and every lane-owned quad
// elsewhere, into exact-size heap arrays whose first element lies 0, 4, 8 or 12 bytes behind a 16-byte boundary (output and both
// maps independently).  Checks:
//   1. every pixel of every frame is owned exactly once, by a quad that starts a multiple of 4 from the frame's first pixel;
//   2. no map or output index falls outside its array (an explicit check, and an ASan report behind the arrays' ends);
//   3. the 16-byte path is taken exactly where a quad is whole and all three addresses are 16-byte aligned;
//   4. what is stored equals a plain float loop, bit for bit (NaN: by isnan), for pixel values at the edges of every type --
//      2^24 + 1 and 2^24 + 3, the types' minima and maxima -- and maps with fractions, negative and zero gains, +-inf, NaN, 1e30;
//      an absent map gives what an all +0.0f dark / an all 1.0f gain gives.
// A wrong answer is a FAILED line.  Exit status 0 only when none happens.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "correct_px.hpp"

static int failures = 0;
static long cases = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static uint32_t bits_of(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static bool same_float(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits_of(a) == bits_of(b); }

// the plain definition: three separately rounded operations (volatile: nothing is contracted or reordered)
template <class T> static float plain(T v, float d, float g) {
    volatile float x = (float)v;
    volatile float y = x - d;
    volatile float z = y * g;
    return z;
}

// n floats whose first lies `residue` bytes behind a 16-byte boundary and whose last ends the allocation
struct Carved {
    void* base = nullptr;
    float* p = nullptr;
    Carved(size_t n, unsigned residue) {
        if (posix_memalign(&base, 16, residue + 4 * n)) std::abort();
        p = reinterpret_cast<float*>(static_cast<char*>(base) + residue);
    }
    ~Carved() { std::free(base); }
    Carved(Carved const&) = delete;
};

static const float kDarks[] = {0.5f, 1.5f, 100.5f, -3.25f, 0.0f, -0.0f, 1e30f, std::numeric_limits<float>::infinity(),
                               -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(), 16777216.0f};
static const float kGains[] = {1.0f, -1.0f, 0.0f, 0.5f, 1.0009765625f, -2.75f, std::numeric_limits<float>::infinity(),
                               std::numeric_limits<float>::quiet_NaN(), 3.0e-3f, -0.0f};

template <class T> static std::vector<T> edge_values() {
    std::vector<T> v = {0, 1, 2, 3, 7, 100, std::numeric_limits<T>::max(), std::numeric_limits<T>::min(), (T)(std::numeric_limits<T>::max() - 1)};
    if (sizeof(T) == 4) {
        v.push_back((T)((1 << 24) + 1));                    // rounds down to 2^24
        v.push_back((T)((1 << 24) + 3));                    // rounds up to 2^24 + 4
        v.push_back((T)((1 << 24) - 1));
        v.push_back((T)(1u << 31 >> (std::numeric_limits<T>::is_signed ? 1 : 0)));
    }
    if (std::numeric_limits<T>::is_signed) { v.push_back((T)-1); v.push_back((T)-100); v.push_back((T)(std::numeric_limits<T>::min() + 1)); }
    if (sizeof(T) == 4 && std::numeric_limits<T>::is_signed) { v.push_back((T)(-(1 << 24) - 1)); v.push_back((T)(-(1 << 24) - 3)); }
    return v;
}

// One stack of `frames` frames stored as the kernel stores it.  kSub: groups of 256 blocks per tile.
template <class T, bool kDark, bool kGain>
static void store_stack(size_t n_values, unsigned r_out, unsigned r_dark, unsigned r_gain, int kSub) {
    constexpr bool sg = std::numeric_limits<T>::is_signed;
    const size_t frames = 3;
    const uint32_t n_blocks = (uint32_t)((n_values + trpx::kCorrBlock - 1) / trpx::kCorrBlock);
    const std::vector<T> edges = edge_values<T>();
    std::vector<T> px(frames * n_values);
    for (size_t i = 0; i < px.size(); ++i) px[i] = edges[(i * 7 + i / 5) % edges.size()];
    Carved dark(n_values, r_dark), gain(n_values, r_gain), out(frames * n_values, r_out);
    for (size_t p = 0; p < n_values; ++p) {
        dark.p[p] = kDarks[(p * 3 + p / 11) % (sizeof kDarks / sizeof *kDarks)];
        gain.p[p] = kGains[(p * 5 + p / 13) % (sizeof kGains / sizeof *kGains)];
    }
    const float unwritten = -12345.0f;
    for (size_t i = 0; i < frames * n_values; ++i) out.p[i] = unwritten;
    std::vector<uint8_t> owned(frames * n_values, 0);
    long vec16 = 0, narrow = 0;

    auto quad = [&](size_t frame, bool frame16, trpx::CorrQuad q) {
        EXPECT(q.n <= trpx::kCorrQuad && q.px % trpx::kCorrQuad == 0);
        if (q.n == 0) return;
        EXPECT(q.px + q.n <= n_values);                     // map and output indices inside their arrays
        if (q.px + q.n > n_values) return;
        const float* d = dark.p + q.px;
        const float* g = gain.p + q.px;
        float* o = out.p + frame * n_values + q.px;
        const bool all_aligned = (uintptr_t)o % 16 == 0 && (!kDark || (uintptr_t)d % 16 == 0) && (!kGain || (uintptr_t)g % 16 == 0);
        const bool v16 = trpx::corr_vec16(frame16, q);
        EXPECT(v16 == (all_aligned && q.n == trpx::kCorrQuad));     // the 16-byte path exactly where all three addresses allow it
        (v16 ? vec16 : narrow) += 1;
        for (uint32_t i = 0; i < q.n; ++i) {
            const T v = px[frame * n_values + q.px + i];
            const uint32_t u = sg ? (uint32_t)(int32_t)v : (uint32_t)v;           // as the decoders hold a pixel: extended to 32 bits
            o[i] = trpx::correct_px<sg, kDark, kGain>(u, kDark ? d[i] : 0.f, kGain ? g[i] : 1.f);
            ++owned[frame * n_values + q.px + i];
        }
    };

    const uint32_t tile_blocks = (uint32_t)kSub * 256u;
    const uint32_t tiles = (n_blocks + tile_blocks - 1) / tile_blocks;
    for (size_t frame = 0; frame < frames; ++frame) {
        // (a map that is absent counts as address 0, as the kernel passes it)
        const bool frame16 = trpx::corr_frame_vec16((uintptr_t)out.p, frame, n_values, kDark ? (uintptr_t)dark.p : 0, kGain ? (uintptr_t)gain.p : 0);
        for (uint32_t t = 0; t < tiles; ++t)
            for (int r = 0; r < kSub; ++r)
                for (uint32_t wave = 0; wave < 4; ++wave) {
                    const uint32_t g0 = t * tile_blocks + (uint32_t)r * 256u + wave * trpx::kCorrWave;
                    if (trpx::corr_wave_staged(g0, n_values)) {
                        EXPECT(g0 + trpx::kCorrWave <= n_blocks && (uint64_t)(g0 + trpx::kCorrWave) * trpx::kCorrBlock <= n_values);
                        std::vector<uint8_t> slot(trpx::kCorrRowDwords, 0);
                        for (uint32_t j = 0; j < trpx::kCorrRounds; ++j)
                            for (uint32_t lane = 0; lane < trpx::kCorrWave; ++lane) {
                                const uint32_t s = trpx::corr_staged_slot(lane, j);
                                EXPECT(s + trpx::kCorrQuad <= trpx::kCorrRowDwords);      // inside the wavefront's LDS row
                                for (uint32_t i = 0; i < trpx::kCorrQuad && s + i < trpx::kCorrRowDwords; ++i) ++slot[s + i];
                                const trpx::CorrQuad q = trpx::corr_staged_quad(g0, lane, j, n_values);
                                EXPECT(q.n == trpx::kCorrQuad && q.px == (uint64_t)g0 * trpx::kCorrBlock + s);   // row dword s = pixel s of the group
                                quad(frame, frame16, q);
                            }
                        for (uint8_t c : slot) EXPECT(c == 1);
                    } else {
                        for (uint32_t lane = 0; lane < trpx::kCorrWave; ++lane) {
                            const uint32_t b = g0 + lane;
                            if (b >= n_blocks) continue;            // (nb = 0: the lane has no block)
                            for (uint32_t i = 0; i < trpx::kCorrRounds; ++i) quad(frame, frame16, trpx::corr_block_quad(b, i, n_values));
                        }
                    }
                }
    }
    bool once = true, equal = true;
    for (size_t f = 0; f < frames; ++f)
        for (size_t p = 0; p < n_values; ++p) {
            once = once && owned[f * n_values + p] == 1;
            // absent maps against an all +0.0f dark / an all 1.0f gain
            equal = equal && same_float(out.p[f * n_values + p], plain<T>(px[f * n_values + p], kDark ? dark.p[p] : 0.0f, kGain ? gain.p[p] : 1.0f));
        }
    EXPECT(once);
    EXPECT(equal);
    if (n_values >= 768 && n_values % 4 == 0 && r_out == 0 && r_dark == 0 && r_gain == 0) EXPECT(vec16 > 0);
    if (r_out || r_dark || r_gain) EXPECT(vec16 == 0 || (n_values % 4 != 0 && r_dark == 0 && r_gain == 0));
    ++cases;
}

template <class T> static void rule() {
    constexpr bool sg = std::numeric_limits<T>::is_signed;
    for (T v : edge_values<T>())
        for (float d : kDarks)
            for (float g : kGains) {
                const uint32_t u = sg ? (uint32_t)(int32_t)v : (uint32_t)v;
                EXPECT(same_float(trpx::correct_px<sg, true, true>(u, d, g), plain<T>(v, d, g)));
                EXPECT(same_float(trpx::correct_px<sg, false, true>(u, d, g), plain<T>(v, 0.0f, g)));
                EXPECT(same_float(trpx::correct_px<sg, true, false>(u, d, g), plain<T>(v, d, 1.0f)));
                EXPECT(same_float(trpx::correct_px<sg, false, false>(u, d, g), plain<T>(v, 0.0f, 1.0f)));
                ++cases;
            }
}

template <class T> static void frames_of() {
    const size_t sizes[] = {1, 11, 12, 13, 767, 769, 12288 + 67};
    const int kSub = sizeof(T) == 4 ? 2 : 4;                // unpack_sub_tiles
    for (size_t n : sizes)
        for (unsigned ro : {0u, 4u, 8u, 12u})
            for (unsigned rd : {0u, 4u, 8u, 12u})
                for (unsigned rg : {0u, 4u, 8u, 12u}) {
                    if (n > 1000 && (ro + rd + rg) % 8 != 0 && !(ro == rd && rd == rg)) continue;   // (the large size: a third of the residue triples)
                    store_stack<T, true, true>(n, ro, rd, rg, kSub);
                    if (rd == 0) store_stack<T, false, true>(n, ro, rd, rg, kSub);
                    if (rg == 0) store_stack<T, true, false>(n, ro, rd, rg, kSub);
                    if (rd == 0 && rg == 0) store_stack<T, false, false>(n, ro, rd, rg, kSub);
                }
}

int main() {
    rule<uint8_t>(); rule<int8_t>(); rule<uint16_t>(); rule<int16_t>(); rule<uint32_t>(); rule<int32_t>();
    frames_of<uint8_t>(); frames_of<int8_t>(); frames_of<uint16_t>(); frames_of<int16_t>(); frames_of<uint32_t>(); frames_of<int32_t>();
    // the 2^24 neighbours round in opposite directions
    EXPECT((trpx::correct_px<false, false, false>((1u << 24) + 1, 0.f, 1.f) == 16777216.0f));
    EXPECT((trpx::correct_px<false, false, false>((1u << 24) + 3, 0.f, 1.f) == 16777220.0f));
    EXPECT((trpx::correct_px<true, false, false>((uint32_t)INT32_MIN, 0.f, 1.f) == -2147483648.0f));
    EXPECT((trpx::correct_px<false, false, false>(UINT32_MAX, 0.f, 1.f) == 4294967296.0f));
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("OK corrected_sanitize (%ld cases)\n", cases);
    return 0;
}
