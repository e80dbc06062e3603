// Frames of a stack into a new stack, without decoding them (trpx_select_frames): the stack of any list
// of frames is the concatenation of those frames' bytes (Terse.hpp:502-505), so the call is a gather of variable-length byte
// segments at byte alignment -- memory bound, no pixel is touched.  All stream ordered, no host sync, every launch shape from
// n_select / n_frames / terse_bytes / out_capacity alone:
//   k_sel_sizes     size[i] = off[frames[i] + 1] - off[frames[i]] with the verdict of every entry (select_map.hpp), the worst
//                   verdict of each workgroup beside it; also the call's status clear
//   k_stack_scan    (encode_pack.hpp: the encoders' scan of frame sizes serves as it is) -> out_offsets, CAPACITY
//   k_sel_verdict   the workgroups' verdicts -> status[0], a plain store behind the stack scan's: INVALID_ARG / CORRUPT win over
//                   CAPACITY; in front of the first store to `out`
//   k_sel_copy      output centric: a wavefront owns kSelChunk aligned bytes of `out` at a time, grid-stride up to the total it
//                   reads from out_offsets[n_select]; one binary search per chunk, per-line searches only in a chunk that holds a
//                   frame boundary; a line inside one frame is aligned source dwords funnel-shifted into one 16-byte store, a
//                   line with a boundary, the stack's end or its pad goes byte by byte (select_map.hpp).  No two lanes ever
//                   write the same dword: no stitch pass, no atomics, bit-identical from run to run
//   k_sel_index     (with out_index) the widths row and the group-offset row of every listed frame
#include <algorithm>

#include "codec_common.hpp"
#include "encode_pack.hpp"
#include "launchers.hpp"
#include "select_map.hpp"

namespace trpx {

static_assert(kSelInvalid == kStatusInvalid && kSelCorrupt == kStatusCorrupt, "select_map.hpp's verdicts are status codes");
constexpr uint32_t kSelMaxGroups = 256 * 8;                 // workgroups of the copy: eight per CU, grid-stride beyond

// ---------------------------------------------------------------------------------------------
// Sizes and verdicts of the list's entries.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sel_sizes(const uint32_t* __restrict__ frames, uint32_t n_select,
                                                        const uint64_t* __restrict__ frame_offsets, uint64_t n_frames,
                                                        uint64_t terse_bytes, uint64_t* __restrict__ sizes,
                                                        uint32_t* __restrict__ wg_code, uint32_t* __restrict__ status) {
    __shared__ uint32_t s_code[4];
    if (blockIdx.x == 0 && threadIdx.x < 4) reinterpret_cast<uint64_t*>(status)[threadIdx.x] = 0ull;   // the call's status clear (8 x u32; nothing else of this launch writes there)
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t code = 0;
    if (i < n_select) sizes[i] = select_size(frames[i], frame_offsets, n_frames, terse_bytes, &code);
    const uint32_t worst = wave_max(code);
    if (lane_id() == 0) s_code[wave_id()] = worst;
    __syncthreads();
    if (threadIdx.x == 0) wg_code[blockIdx.x] = max(max(s_code[0], s_code[1]), max(s_code[2], s_code[3]));
}

// One workgroup: the worst verdict of all (CORRUPT over INVALID_ARG, by their codes) into status[0].
__global__ __launch_bounds__(kThreads) void k_sel_verdict(const uint32_t* __restrict__ wg_code, uint32_t n_groups,
                                                          uint32_t* __restrict__ status) {
    __shared__ uint32_t s_code[4];
    uint32_t code = 0;
    for (uint32_t i = threadIdx.x; i < n_groups; i += kThreads) code = max(code, wg_code[i]);
    const uint32_t worst = wave_max(code);
    if (lane_id() == 0) s_code[wave_id()] = worst;
    __syncthreads();
    const uint32_t all = max(max(s_code[0], s_code[1]), max(s_code[2], s_code[3]));
    if (threadIdx.x == 0 && all) status[0] = all;           // (plain store behind k_stack_scan's: it wins over CAPACITY)
}

// ---------------------------------------------------------------------------------------------
// The copy.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sel_copy(const uint8_t* __restrict__ terse, const uint64_t* __restrict__ frame_offsets,
                                                       const uint32_t* __restrict__ frames, uint32_t n_select,
                                                       const uint64_t* __restrict__ out_offsets, uint8_t* __restrict__ out,
                                                       uint64_t out_capacity, const uint32_t* __restrict__ status) {
    if (status[0] != 0) return;                             // a bad entry, bad offsets, capacity: write nothing
    const uint64_t total = out_offsets[n_select];
    if (!select_fits(total, out_capacity)) return;          // (the scan's own verdict, once more in front of the stores)
    const uint64_t n_chunks = (sel_align4(total) + kSelChunk - 1) / kSelChunk;
    const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + wave_id(), n_waves = (uint64_t)gridDim.x * (kThreads / 64);
    const uint32_t lane = lane_id();
    for (uint64_t c = wave; c < n_chunks; c += n_waves) {
        const uint64_t c0 = c * kSelChunk;                  // (< total: c0 is a multiple of 4 below align4(total))
        SelChunkSlots ch = select_chunk(out_offsets, n_select, c0);
        ch.lo = uniform32(ch.lo);
        ch.hi = uniform32(ch.hi);
        if (ch.lo == ch.hi) {                               // the chunk starts in the frame it ends in: its slot once, no search per line
            const SelSlot s = select_slot_at(out_offsets, frames, frame_offsets, ch.lo);
            if (select_chunk_whole(s, c0)) {                // nothing but interior lines: every load in flight before the first store
                SelLine16 v[kSelLinesPerLane];
#pragma unroll
                for (uint32_t j = 0; j < kSelLinesPerLane; ++j) v[j] = select_line_whole(terse, s, c0 + (uint64_t)(j * 64 + lane) * kSelLine);
#pragma unroll
                for (uint32_t j = 0; j < kSelLinesPerLane; ++j) select_store16(out, c0 + (uint64_t)(j * 64 + lane) * kSelLine, v[j]);
                continue;
            }
            for (uint32_t j = 0; j < kSelLinesPerLane; ++j)  // (the list's last frame: the stack ends inside the chunk)
                select_line_in(terse, out_offsets, frames, frame_offsets, ch.lo, s, c0 + (uint64_t)(j * 64 + lane) * kSelLine, total, out);
        } else {
            for (uint32_t j = 0; j < kSelLinesPerLane; ++j)
                select_line(terse, out_offsets, frames, frame_offsets, ch, c0 + (uint64_t)(j * 64 + lane) * kSelLine, total, out);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The decode index of the selected stack: row frames[i] of widths (n_blocks bytes) and of the group offsets (n_tiles u64, relative
// to the frame) into row i.  The widths rows are a gather of fixed-length byte segments: the same lines as the copy, a line inside
// one row funnel-shifted from aligned source dwords, a line with a row boundary byte by byte; the lines end at
// align16(n_select * n_blocks), inside the index's padding.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sel_index(const uint32_t* __restrict__ frames, uint32_t n_select, uint32_t n_frames,
                                                        uint32_t n_blocks, uint32_t n_tiles, const uint8_t* __restrict__ widths,
                                                        const uint64_t* __restrict__ tile_off, uint8_t* __restrict__ out_widths,
                                                        uint64_t* __restrict__ out_tile_off, const uint32_t* __restrict__ status) {
    if (status[0] == kStatusInvalid || status[0] == kStatusCorrupt) return;   // (a stack that does not fit still has its index)
    const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x, n_thr = (uint64_t)gridDim.x * kThreads;
    const uint64_t n_off = (uint64_t)n_select * n_tiles;
    for (uint64_t j = tid; j < n_off; j += n_thr) {
        const uint32_t f = frames[j / n_tiles];
        if (f < n_frames) out_tile_off[j] = tile_off[(uint64_t)f * n_tiles + j % n_tiles];
    }
    const uint64_t n_w = (uint64_t)n_select * n_blocks, n_lines = (n_w + kSelLine - 1) / kSelLine;
    for (uint64_t line = tid; line < n_lines; line += n_thr) {
        const uint64_t L = line * kSelLine;
        const uint64_t slot = L / n_blocks, in_row = L % n_blocks;
        const uint32_t f = frames[slot];
        if (in_row + kSelLine <= n_blocks) {
            if (f < n_frames)
                *reinterpret_cast<SelLine16*>(out_widths + L) = select_funnel16(reinterpret_cast<const uint32_t*>(widths), (uint64_t)f * n_blocks + in_row);
            continue;
        }
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < kSelLine; ++k) {
            const uint64_t b = L + k;
            if (b >= n_w) break;
            const uint32_t fb = frames[b / n_blocks];
            if (fb < n_frames) w[k / 4] |= (uint32_t)widths[(uint64_t)fb * n_blocks + b % n_blocks] << (8u * (k % 4));
        }
        *reinterpret_cast<SelLine16*>(out_widths + L) = SelLine16{w[0], w[1], w[2], w[3]};
    }
}

// ---------------------------------------------------------------------------------------------
// Host-side launcher (called by the C ABI in api.hip).
// ---------------------------------------------------------------------------------------------
size_t select_workspace_bytes(size_t n_select) {
    return align_up(8 * n_select, 8) + align_up(4 * ((n_select + kThreads - 1) / kThreads), 8);
}

hipError_t launch_select_frames(const SelectArgs& a, hipStream_t st) {
    const uint32_t n_groups = (a.n_select + kThreads - 1) / kThreads;
    uint64_t* sizes = static_cast<uint64_t*>(a.workspace);
    uint32_t* wg_code = reinterpret_cast<uint32_t*>(sizes + a.n_select);
    const dim3 blk(kThreads);

    hipLaunchKernelGGL(k_sel_sizes, dim3(n_groups), blk, 0, st, a.frames, a.n_select, a.frame_offsets, (uint64_t)a.n_frames,
                       (uint64_t)a.terse_bytes, sizes, wg_code, a.status);
    hipLaunchKernelGGL(k_stack_scan, dim3(1), blk, 0, st, sizes, a.n_select, (uint64_t)a.out_capacity, a.out_offsets, a.status);
    hipLaunchKernelGGL(k_sel_verdict, dim3(1), blk, 0, st, wg_code, n_groups, a.status);
    if (a.out_capacity) {
        // the most the call can write: out_capacity, and no more than n_select copies of the whole stream
        const unsigned __int128 most = (unsigned __int128)a.n_select * a.terse_bytes + 3;
        const uint64_t bytes = most < a.out_capacity ? (uint64_t)most : (uint64_t)a.out_capacity;
        const uint64_t chunks = (bytes + kSelChunk - 1) / kSelChunk, groups = (chunks + kThreads / 64 - 1) / (kThreads / 64);
        hipLaunchKernelGGL(k_sel_copy, dim3((uint32_t)std::min<uint64_t>(groups, kSelMaxGroups)), blk, 0, st, a.terse, a.frame_offsets,
                           a.frames, a.n_select, a.out_offsets, a.out, (uint64_t)a.out_capacity, a.status);
    }
    if (a.out_widths) {
        const uint64_t lines = ((uint64_t)a.n_select * a.n_blocks + kSelLine - 1) / kSelLine;
        const uint64_t groups = (std::max<uint64_t>(lines, (uint64_t)a.n_select * a.n_tiles) + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(k_sel_index, dim3((uint32_t)std::min<uint64_t>(groups, kSelMaxGroups)), blk, 0, st, a.frames, a.n_select,
                           a.n_frames, a.n_blocks, a.n_tiles, a.widths, a.tile_off, a.out_widths, a.out_tile_off, a.status);
    }
    return hipGetLastError();
}

}  // namespace trpx
