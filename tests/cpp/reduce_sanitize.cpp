// Sanitizer tier of trpx_decode_reduce (CPU build only: g++ -fsanitize=address,undefined; no HIP, no GPU): what the op decides --
// identity, step, merge of two partials, conversion: trpx_amd/csrc/reduce_ops.hpp, the text the kernels run.  This program runs a
// model of the call for every (pixel type, op): the frames of every group cut into chunks as the launch plan cuts them (chunks
// without frames included), every chunk's accumulators into a partial slab of EXACTLY chunks x outputs x values elements on the
// heap, the chunks merged in order and converted into an output of exactly outputs x values elements -- an index one past either
// is an ASan report, a signed overflow or a bad shift a UBSan report, a wrong element a FAILED line.  The truth is a direct loop
// over the pixels in 128-bit arithmetic.  Exit status 0 only when none of that happens.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include <type_traits>
#include <vector>

#include "reduce_ops.hpp"

static int failures = 0;
static long cases = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// a pixel as the extraction hands it to the step: the type's value in 32 bits, sign-extended
template <class T> static uint32_t widened(T v) { return (uint32_t)(int32_t)v; }

template <class T, int op>
static void run(std::vector<T> const& px, size_t frames, size_t n, size_t group, size_t fpc, int64_t threshold) {
    using Op = trpx::ReduceOp<T, op>;
    using Acc = typename Op::Acc;
    using Out = typename Op::Out;
    static_assert(sizeof(Acc) == trpx::reduce_acc_size(op) && sizeof(Out) == trpx::reduce_out_size(op, sizeof(T)));
    const size_t n_out = (frames + group - 1) / group, per_group = group < frames ? group : frames, chunks = (per_group + fpc - 1) / fpc;
    // the truth: a direct loop, 128-bit arithmetic
    std::vector<Out> want(n_out * n);
    for (size_t j = 0; j < n_out; ++j)
        for (size_t p = 0; p < n; ++p) {
            const size_t g0 = j * group, g1 = g0 + group < frames ? g0 + group : frames;
            T hi = px[g0 * n + p], lo = hi;
            unsigned __int128 sq = 0;
            uint32_t ge = 0;
            for (size_t f = g0; f < g1; ++f) {
                const T v = px[f * n + p];
                if (v > hi) hi = v;
                if (v < lo) lo = v;
                sq += (unsigned __int128)((__int128)v * (__int128)v);
                ge += (__int128)v >= (__int128)threshold ? 1u : 0u;
            }
            want[j * n + p] = op == trpx::kReduceMax ? (Out)hi : op == trpx::kReduceMin ? (Out)lo : op == trpx::kReduceSumSq ? (Out)(uint64_t)sq : (Out)ge;
        }
    // the model: chunk by chunk into the slab, then the merge
    Acc* slab = new Acc[chunks * n_out * n];                // exactly the partial slab
    Out* out = new Out[n_out * n];                          // exactly the output
    size_t empty = 0;
    for (size_t j = 0; j < n_out; ++j)
        for (size_t c = 0; c < chunks; ++c) {
            const size_t g0 = j * group, g1 = g0 + group < frames ? g0 + group : frames;
            const size_t f0 = g0 + c * fpc, f1 = f0 + fpc < g1 ? f0 + fpc : g1;   // (f0 past g1: a chunk without frames)
            empty += f0 >= f1;
            for (size_t p = 0; p < n; ++p) {
                Acc a = Op::identity();
                for (size_t f = f0; f < f1; ++f) a = Op::step(a, widened<T>(px[f * n + p]), threshold);
                slab[(c * n_out + j) * n + p] = a;
            }
        }
    for (size_t i = 0; i < n_out * n; ++i) {
        Acc s = Op::identity();
        for (size_t c = 0; c < chunks; ++c) s = Op::merge(s, slab[c * n_out * n + i]);
        out[i] = Op::convert(s);
    }
    bool same = true;
    for (size_t i = 0; i < n_out * n; ++i) same = same && out[i] == want[i];
    EXPECT(same);
    if (frames % group && (frames % group + fpc - 1) / fpc < chunks) EXPECT(empty > 0);   // a short last group leaves empty chunks
    delete[] slab;
    delete[] out;
    ++cases;
}

template <class T, int op>
static void splits(std::vector<T> const& px, size_t frames, size_t n, int64_t threshold) {
    for (size_t group : {(size_t)1, (size_t)2, (size_t)3, frames - 1, frames, frames + 5})
        for (size_t fpc : {(size_t)1, (size_t)2, (size_t)3, group})
            if (group >= 1 && fpc >= 1) run<T, op>(px, frames, n, group, fpc, threshold);
}

template <class T>
static void type_cases() {
    const T lo = std::numeric_limits<T>::min(), hi = std::numeric_limits<T>::max();
    const size_t frames = 11, n = 13;
    std::vector<std::vector<T>> data;
    data.emplace_back(frames * n, hi);                      // 32-bit types: eleven squares of the maximum wrap 2^64
    data.emplace_back(frames * n, lo);                      // int32: INT32_MIN squared, 2^62, eleven times
    std::vector<T> mix(frames * n);
    for (size_t i = 0; i < mix.size(); ++i) mix[i] = i % 5 == 0 ? lo : i % 5 == 1 ? hi : i % 5 == 2 ? (T)0 : (T)(i * 37 + 1);
    data.push_back(mix);
    for (size_t i = 0; i < mix.size(); ++i) mix[i] = std::is_signed_v<T> ? (T)(0 - (T)(1 + i % 7)) : (T)(1 + i % 7);   // strictly negative / positive ...
    data.push_back(mix);
    for (size_t p = 0; p < n; ++p) mix[4 * n + p] = 0;      // ... and one blank frame: the zeros take part
    data.push_back(mix);
    if constexpr (sizeof(T) == 4) {
        std::vector<T> wrap(frames * n);
        for (size_t i = 0; i < wrap.size(); ++i) wrap[i] = i % 2 ? hi : lo;
        data.push_back(wrap);
        uint64_t s = 0;                                     // the fixture does what it is for: the true sum of squares passes 2^64
        unsigned __int128 t = 0;
        const uint64_t m = std::is_signed_v<T> ? (uint64_t)(-(int64_t)lo) : (uint64_t)hi;   // the magnitude of data[1] / data[0]
        for (size_t f = 0; f < frames; ++f) { s += m * m; t += (unsigned __int128)m * m; }
        EXPECT((unsigned __int128)s != t);
    }
    const int64_t l = (int64_t)lo, h = (int64_t)hi;
    for (auto const& px : data) {
        splits<T, trpx::kReduceMax>(px, frames, n, 0);
        splits<T, trpx::kReduceMin>(px, frames, n, 0);
        splits<T, trpx::kReduceSumSq>(px, frames, n, 0);
        for (int64_t thr : {(int64_t)0, (int64_t)1, (int64_t)-1, h / 2, l, l - 1, h, h + 1, std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max()})
            splits<T, trpx::kReduceCountGe>(px, frames, n, thr);
    }
    // the identities: what a chunk without frames leaves does not move any merge
    EXPECT((trpx::ReduceOp<T, trpx::kReduceMax>::merge(trpx::ReduceOp<T, trpx::kReduceMax>::identity(), lo) == lo));
    EXPECT((trpx::ReduceOp<T, trpx::kReduceMin>::merge(trpx::ReduceOp<T, trpx::kReduceMin>::identity(), hi) == hi));
    EXPECT((trpx::ReduceOp<T, trpx::kReduceSumSq>::identity() == 0 && trpx::ReduceOp<T, trpx::kReduceCountGe>::identity() == 0));
}

int main() {
    type_cases<uint8_t>();
    type_cases<int8_t>();
    type_cases<uint16_t>();
    type_cases<int16_t>();
    type_cases<uint32_t>();
    type_cases<int32_t>();
    // INT32_MIN squared is 2^62, exactly
    EXPECT((trpx::ReduceOp<int32_t, trpx::kReduceSumSq>::step(0, 0x80000000u, 0) == (1ull << 62)));
    EXPECT((trpx::ReduceOp<uint32_t, trpx::kReduceSumSq>::step(0, 0xFFFFFFFFu, 0) == 0xFFFFFFFE00000001ull));
    EXPECT((trpx::ReduceOp<int16_t, trpx::kReduceSumSq>::step(0, 0xFFFF8000u, 0) == (1ull << 30)));
    EXPECT((trpx::ReduceOp<uint16_t, trpx::kReduceSumSq>::step(0, 0xFFFFu, 0) == 0xFFFE0001ull));
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("OK reduce_sanitize (%ld cases)\n", cases);
    return 0;
}
