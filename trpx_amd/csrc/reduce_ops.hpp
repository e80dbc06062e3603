// What the op of trpx_decode_reduce decides, once: the accumulator and the output element, the identity, the step that takes one
// pixel, the merge of two partial accumulators and the conversion to the output element.  __host__ __device__: the kernels
// (decode_reduce.hip) and the CPU sanitizer program (tests/cpp/reduce_sanitize.cpp) compile this text.
//   MAX / MIN   the pixel type widened to 32 bits, with its signedness; identity = the type's minimum / maximum, so that a chunk
//               without frames (a short last group) leaves the merge alone; the element is T
//   SUMSQ       sum of (int64)v * (int64)v modulo 2^64, in unsigned arithmetic (no signed overflow anywhere); the element is uint64_t
//   COUNT_GE    frames with (int64)v >= threshold (trpx_decode_sparse's comparison); the element is uint32_t
// A pixel arrives as the extraction leaves it: the type's value in 32 bits, sign-extended for signed types.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <limits>
#include <type_traits>

#ifndef TRPX_HD
#if defined(__HIPCC__)
#define TRPX_HD __host__ __device__
#else
#define TRPX_HD
#endif
#endif

namespace trpx {

// (the values of trpx_reduce_op, include/trpx_hip.h)
enum : int { kReduceMax = 0, kReduceMin = 1, kReduceSumSq = 2, kReduceCountGe = 3, kReduceOps = 4 };

template <typename T, int op> struct ReduceOp {
    static_assert(std::is_integral_v<T> && sizeof(T) <= 4 && op >= 0 && op < kReduceOps);
    using Wide = std::conditional_t<std::is_signed_v<T>, int32_t, uint32_t>;    // the pixel type widened to 32 bits
    using Acc = std::conditional_t<op == kReduceSumSq, uint64_t, std::conditional_t<op == kReduceCountGe, uint32_t, Wide>>;
    using Out = std::conditional_t<op == kReduceSumSq, uint64_t, std::conditional_t<op == kReduceCountGe, uint32_t, T>>;

    TRPX_HD static constexpr Acc identity() {
        if constexpr (op == kReduceMax) return (Acc)std::numeric_limits<T>::min();
        else if constexpr (op == kReduceMin) return (Acc)std::numeric_limits<T>::max();
        else return 0;
    }
    // one pixel: u = the type's value in 32 bits (sign-extended)
    TRPX_HD static inline Acc step(Acc a, uint32_t u, int64_t threshold) {
        const Wide v = (Wide)u;
        if constexpr (op == kReduceMax) return v > a ? v : a;
        else if constexpr (op == kReduceMin) return v < a ? v : a;
        else if constexpr (op == kReduceCountGe) return a + ((int64_t)v >= threshold ? 1u : 0u);
        else if constexpr (sizeof(T) < 4) return a + (uint64_t)(u * u);         // |v| <= 65535: v * v < 2^32, also from the sign-extended bits
        else {
            const uint64_t m = (uint64_t)(int64_t)v;                             // (int64)v as bits: the product modulo 2^64 is the square's
            return a + m * m;
        }
    }
    TRPX_HD static inline Acc merge(Acc a, Acc b) {
        if constexpr (op == kReduceMax) return b > a ? b : a;
        else if constexpr (op == kReduceMin) return b < a ? b : a;
        else return a + b;
    }
    TRPX_HD static inline Out convert(Acc a) { return (Out)a; }
};

// bytes of an output element / of a raw accumulator in a partial slab, for the host's sizes (elem: the pixel type's bytes)
constexpr size_t reduce_out_size(int op, size_t elem) { return op == kReduceSumSq ? 8 : op == kReduceCountGe ? 4 : elem; }
constexpr size_t reduce_acc_size(int op) { return op == kReduceSumSq ? 8 : 4; }

}  // namespace trpx
