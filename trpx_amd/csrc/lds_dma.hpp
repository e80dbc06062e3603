// LDS-DMA: stream bytes straight into an LDS window, no staging registers (the walkers' refills in decode_frame.hip and decode_part.hip).
#pragma once
#include "codec_common.hpp"

namespace trpx {

// One piece: lane l's 16 bytes at `src` land at LDS byte address lds_base + 16 * l.  src_uniform and lds_base are wave-uniform
// (where the compiler loses sight of that -- "invalid operand" --, the caller says so: uniform64 / uniform32).  The caller waits
// with s_waitcnt vmcnt(0) before it reads the bytes.  (An asm statement: with the builtin in the kernel's body the host pass of
// hipcc 7.2 silently dropped the kernel's launch stubs.)
__device__ __forceinline__ void lds_dma16(const uint32_t* src_uniform, uint32_t lane_byte_offset, uint32_t lds_base) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_byte_offset), "s"(src_uniform), "s"(lds_base) : "memory");
}

}  // namespace trpx
