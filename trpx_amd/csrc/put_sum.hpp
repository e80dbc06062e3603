// The one conversion of an exact integer sum to an output element, shared by the calls that leave sums (decode_sum.hip:
// trpx_decode_sum, decode_binned.hip: trpx_decode_binned): 32-bit integers clamp (Bit_pointer.hpp:747-763), 64-bit integers keep
// the value, float / double round it once to nearest even.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace trpx {

// output element codes (the trpx_dtype values of include/trpx_hip.h) and the partial slabs' raw accumulators
enum : int { kSumU32 = 4, kSumI32 = 5, kSumF32 = 6, kSumF64 = 7, kSumU64 = 8, kSumI64 = 9, kSumPart32 = 100, kSumPart64 = 101 };

// The exact sum s -> element i of `out`, of the type `code` names.  kSumPart32 / kSumPart64: a chunk's raw accumulator (partial slab).
__device__ __forceinline__ void put_sum(void* __restrict__ out, uint64_t i, int code, int64_t s) {
    switch (code) {
    case kSumI32: static_cast<int32_t*>(out)[i] = (int32_t)(s > INT_MAX ? (int64_t)INT_MAX : s < INT_MIN ? (int64_t)INT_MIN : s); break;
    case kSumU32: static_cast<uint32_t*>(out)[i] = (uint32_t)(s > (int64_t)UINT_MAX ? (int64_t)UINT_MAX : s < 0 ? 0 : s); break;
    case kSumI64: static_cast<int64_t*>(out)[i] = s; break;
    case kSumU64: static_cast<uint64_t*>(out)[i] = (uint64_t)s; break;
    case kSumF32: static_cast<float*>(out)[i] = (float)s; break;
    case kSumF64: static_cast<double*>(out)[i] = (double)s; break;
    case kSumPart32: static_cast<uint32_t*>(out)[i] = (uint32_t)s; break;
    case kSumPart64: static_cast<uint64_t*>(out)[i] = (uint64_t)s; break;
    }
}

}  // namespace trpx
