// PROLIX decode, tuned kernels for gfx950 (CDNA4).  Replaces jpa::Terse::prolix(Iterator, frame)
// (reference include/Terse.hpp:352-389) and Bit_range::get_range / operator T()
// (Bit_pointer.hpp:742-792, :597-617).  Same two stages as decode.hip, restructured:
//
//   k_walk_lds      one wavefront per frame walks the header chain (Terse.hpp:360-372) with the
//                   frame's stream staged through LDS in 16 KB chunks: a step costs an LDS round
//                   trip instead of an L2/HBM one.  64 candidate blocks are tested per step, so a run
//                   of equal-width blocks is one step.  Emits width[b] (u8) and the bit offset of
//                   every 256-block group.
//   k_unpack_tiles  tile = 1024 blocks (512 for 32-bit pixels), 4 (2) blocks per lane.  widths ->
//                   lengths -> wave/LDS scan -> the tile's stream bytes are fetched once, coalesced,
//                   into LDS -> every lane extracts its 12 fields with code specialised on the block
//                   width (static shifts, v_bfe) -> 24/48-byte streaming stores.
//
// HBM traffic per frame: S (stream, read twice: walk + unpack) + n_blocks (widths, written+read)
// + N*sizeof(T) (pixels, written once).  Algorithmic bytes: S + N*sizeof(T).
#include "codec_common.hpp"
#include "launchers.hpp"
#include "profile.hpp"
#include "unpack_common.hpp"
#include "unpack_tile.hpp"
#include "walk_lds.hpp"
#include <stdlib.h>
#include <string.h>

namespace trpx {

// ---------------------------------------------------------------------------------------------
// k_walk_lds (body: walk_lds.hpp)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void k_walk_lds(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                    const uint64_t* __restrict__ frame_offsets, FrameGeom g,
                                                    uint32_t max_w, uint8_t* __restrict__ widths,
                                                    uint64_t* __restrict__ tile_off, const uint32_t* __restrict__ only,
                                                    const uint32_t* __restrict__ list, uint32_t* __restrict__ status) {
    __shared__ uint32_t s_chunk[kWalkChunkDw + 4];
    uint64_t frame = blockIdx.x;
    if (list) {                                       // (the frames k_decode_frames listed, see decode_seg.hip)
        if (blockIdx.x >= list[0]) return;
        frame = list[1u + blockIdx.x] & 0x7FFFFFFFu;
    }
    if (only && !only[frame]) return;                 // (frames the position-parallel walk has done)
    walk_lds_frame(terse, terse_bytes, frame_offsets, g, max_w, widths, tile_off, frame, s_chunk, status);
}

// ---------------------------------------------------------------------------------------------
// k_unpack_tiles
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads, sizeof(T) == 4 ? 4 : 5) void k_unpack_tiles(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                              const uint64_t* __restrict__ frame_offsets, FrameGeom g,
                                                              uint32_t tiles_per_frame,
                                                              const uint8_t* __restrict__ widths,
                                                              const uint64_t* __restrict__ tile_off,
                                                              T* __restrict__ pixels_out, uint32_t* __restrict__ status,
                                                              const uint32_t* __restrict__ frame_mode) {
    __shared__ uint32_t s_image[unpack_image_dwords<T>()];
    __shared__ uint32_t s_wtot[unpack_sub_tiles<T>() * 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[unpack_stage_dwords<T>()];
    if (status[0] != 0) return;                             // corrupt chain: produce nothing
    const uint64_t tile = blockIdx.x;
    if (frame_mode && frame_mode[tile / tiles_per_frame] == 0u) return;   // (large frames: this one is extracted part by part, decode_part.hip)
    unpack_tile<T>(terse, terse_bytes, frame_offsets, g, (uint32_t)(tile / tiles_per_frame), (uint32_t)(tile % tiles_per_frame),
                   widths, tile_off, pixels_out, status, s_image, s_wtot, s_stage);
}

// ---------------------------------------------------------------------------------------------
// Group states (row f1 for files): the chain state (bit offset, width of the block before) at every 256th block is
// all a decoder needs to walk a frame's groups independently.  k_index_group_states reads the states off a decode
// index; k_walk_groups rebuilds the index from them -- one lane per group, 256 dependent steps, every group checked
// against its successor's state (the last one against S_f = 1 + bits/8, Terse.hpp:547).
// ---------------------------------------------------------------------------------------------
constexpr uint64_t kStateOffMask = (1ull << 40) - 1;

__global__ __launch_bounds__(kThreads) void k_index_group_states(const uint8_t* __restrict__ widths, const uint64_t* __restrict__ tile_off,
                                                                 FrameGeom g, uint64_t n_groups_total, uint64_t* __restrict__ states) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_groups_total) return;
    const uint64_t frame = i / g.n_tiles, k = i % g.n_tiles;
    const uint32_t w_prev = k ? widths[frame * g.n_blocks + k * kTileBlocks - 1] : 0u;
    states[i] = (tile_off[i] & kStateOffMask) | ((uint64_t)w_prev << 40);
}

__global__ __launch_bounds__(kThreads) void k_walk_groups(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                          const uint64_t* __restrict__ frame_offsets, FrameGeom g, uint32_t max_w,
                                                          const uint64_t* __restrict__ states, uint64_t n_groups_total,
                                                          uint8_t* __restrict__ widths, uint64_t* __restrict__ tile_off,
                                                          uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_groups_total) return;
    const uint64_t frame = i / g.n_tiles;
    const uint32_t k = (uint32_t)(i % g.n_tiles);
    const uint64_t fo = frame_offsets[frame], fe = frame_offsets[frame + 1];
    bool bad = !(fe > fo && fe <= terse_bytes);
    const uint64_t limit = bad ? 0 : 8 * (fe - fo);
    const uint32_t* __restrict__ s32 = reinterpret_cast<const uint32_t*>(terse);
    const uint64_t n_dw = (terse_bytes + 3) / 4;
    const uint64_t st = states[i];
    uint64_t pos = st & kStateOffMask;
    uint32_t w = (uint32_t)(st >> 40);
    if (k == 0 && st != 0) bad = true;                       // a frame starts at bit 0 with width 0 (Terse.hpp:359, :505)
    if (pos > limit || w > max_w) bad = true;
    const uint32_t b0 = k * kTileBlocks;
    const uint32_t b1 = b0 + kTileBlocks < g.n_blocks ? b0 + kTileBlocks : g.n_blocks;
    const uint32_t nb_last = (uint32_t)(g.n_values - (uint64_t)(g.n_blocks - 1) * kBlock);
    if (!bad) tile_off[i] = pos;
    for (uint32_t b = b0; b < b1 && !bad; ++b) {
        const uint32_t bits = (uint32_t)stream_bits([&](uint64_t i) { return ld_stream_dw(s32, i, n_dw); }, 8 * fo + pos);
        uint32_t hl = 1;
        if (!(bits & 1u)) {                                  // Terse.hpp:361
            const ExplicitHeader h = parse_explicit_header(bits);
            w = h.w; hl = h.len;
        }
        if (w > max_w) { bad = true; break; }
        widths[frame * g.n_blocks + b] = (uint8_t)w;
        pos += hl + (uint64_t)(b + 1 == g.n_blocks ? nb_last : (uint32_t)kBlock) * w;
        if (pos > limit) bad = true;
    }
    if (!bad) {
        if (b1 < g.n_blocks) bad = ((pos & kStateOffMask) | ((uint64_t)w << 40)) != states[i + 1];   // lands in the next group's state
        else bad = 1 + pos / 8 != fe - fo;                                                           // S_f (Terse.hpp:547)
    }
    if (bad) atomicMax(&status[0], kStatusCorrupt);
}

// ---------------------------------------------------------------------------------------------
// A freshly written decode index against its stream, block by block.  Whatever consumes an index rebuilds the layout from the
// widths alone (header_len: one bit where a width repeats), so an index must not describe a stream with a RESTATED width (an
// explicit header of the width before: valid, codec_common.hpp) -- and the walkers that write indices do not look for one.
// One lane per block, a workgroup per group of 256: positions by the consumers' own rule from the group's recorded offset,
// and at each the stream's header must be what the widths say: the "same width" bit exactly where the width repeats, else the
// width's code.  Up to a group's first restated width the rule's positions are the true ones, so that header is seen: CORRUPT.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_check_index(const uint8_t* __restrict__ terse, uint64_t terse_bytes,
                                                          const uint64_t* __restrict__ frame_offsets, FrameGeom g,
                                                          const uint8_t* __restrict__ widths, const uint64_t* __restrict__ tile_off,
                                                          uint32_t* __restrict__ status) {
    __shared__ uint32_t s_tot[4];
    if (status[0] != 0) return;                             // (uniform: the walk has given its verdict)
    const uint64_t tile = blockIdx.x;
    const uint64_t frame = tile / g.n_tiles;
    const uint32_t b = (uint32_t)(tile % g.n_tiles) * kTileBlocks + threadIdx.x;
    const bool valid = b < g.n_blocks;
    uint32_t w = 0, w_prev = 0, nb = 0;
    if (valid) {
        const uint8_t* wf = widths + frame * g.n_blocks;
        w = wf[b];
        w_prev = b ? wf[b - 1] : 0u;
        const uint64_t first = (uint64_t)b * kBlock;
        nb = (uint32_t)(first + kBlock <= g.n_values ? kBlock : g.n_values - first);
    }
    const uint32_t hl = header_len(w, w_prev);
    uint32_t total;
    const uint32_t excl = block_exclusive_scan(valid ? hl + nb * w : 0u, s_tot, &total);
    if (!valid) return;
    const uint64_t fo = frame_offsets[frame], fe = frame_offsets[frame + 1];
    const uint64_t pos = tile_off[tile] + excl;             // the block's header, relative to the frame
    bool ok = fe > fo && fe <= terse_bytes && pos + hl <= 8 * (fe - fo);
    if (ok) {
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(terse);
        const uint64_t n_dw = (terse_bytes + 3) / 4;
        const uint32_t bits = (uint32_t)stream_bits([&](uint64_t i) { return ld_stream_dw(s32, i, n_dw); }, 8 * fo + pos);
        ok = bits & 1u ? hl == 1u : (hl != 1u && parse_explicit_header(bits).w == w);   // Terse.hpp:361-370
    }
    if (!ok) atomicMax(&status[0], kStatusCorrupt);
}

hipError_t launch_check_index(const DecodeArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_check_index, dim3((uint32_t)((uint64_t)a.n_frames * a.geom.n_tiles)), dim3(kThreads), 0, st, a.terse,
                       (uint64_t)a.terse_bytes, a.frame_offsets, a.geom, a.widths, a.tile_off, a.status);
    return hipGetLastError();
}

hipError_t launch_index_group_states(const DecodeArgs& a, uint64_t* states, hipStream_t st) {
    const uint64_t n = (uint64_t)a.n_frames * a.geom.n_tiles;
    hipLaunchKernelGGL(k_index_group_states, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a.widths, a.tile_off,
                       a.geom, n, states);
    return hipGetLastError();
}

hipError_t launch_walk_groups(const DecodeArgs& a, uint32_t max_w, const uint64_t* states, bool clear_status, hipStream_t st) {
    if (clear_status) zero_status(a.status, st);
    const uint64_t n = (uint64_t)a.n_frames * a.geom.n_tiles;
    // frames of less than 2^32 bits: the write pass of the position-parallel walk, one lane per group (k_seg_groups)
    const uint64_t worst_bits = (uint64_t)a.geom.n_blocks * (12u + (uint64_t)kBlock * max_w) + 8u;
    if (worst_bits < 0xF0000000ull) return launch_seg_groups(a, max_w, states, st);
    hipLaunchKernelGGL(k_walk_groups, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a.terse,
                       (uint64_t)a.terse_bytes, a.frame_offsets, a.geom, max_w, states, n, a.widths, a.tile_off, a.status);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_decode_fast_t(const DecodeArgs& a, hipStream_t st) {
    const FrameGeom g = a.geom;
    constexpr uint32_t tb = unpack_sub_tiles<T>() * kThreads;
    const uint32_t tpf = (g.n_blocks + tb - 1) / tb;
    zero_status(a.status, st);
    Profiler& prof = profiler();
    prof.begin();
    prof.mark(st);
    if (a.plan.walk != Walk::kCallers) {
        const hipError_t e = launch_walk_only(a, PixelTraits<T>::bits, false, st);
        if (e != hipSuccess) return e;
    }
    prof.mark(st);
    hipError_t e = hipErrorInvalidValue;
    if (a.plan.extract == Extract::kFramesIndexed)              // many small frames: the per-frame decoder with the widths given
        e = launch_decode_frames_indexed(PixelTraits<T>::dtype, a, nullptr, st);
    else if (a.plan.extract == Extract::kUnitsIndexed)          // large frames of 8/16-bit pixels with their index: as the index route extracts them (decode_frame.hip)
        e = launch_decode_units_indexed(PixelTraits<T>::dtype, a, st, nullptr);
    else if (a.plan.extract == Extract::kTiled)
        hipLaunchKernelGGL((k_unpack_tiles<T>), dim3((uint32_t)((uint64_t)a.n_frames * tpf)), dim3(kThreads), 0, st, a.terse,
                           (uint64_t)a.terse_bytes, a.frame_offsets, g, tpf, a.widths, a.tile_off,
                           static_cast<T*>(a.pixels_out), a.status, static_cast<const uint32_t*>(nullptr));
    prof.mark(st);
    return a.plan.extract == Extract::kTiled ? hipGetLastError() : e;
}

template <typename T>
static hipError_t launch_unpack_tiles_t(const DecodeArgs& a, hipStream_t st, const uint32_t* frame_mode) {
    constexpr uint32_t tb = unpack_sub_tiles<T>() * kThreads;
    const uint32_t tpf = (a.geom.n_blocks + tb - 1) / tb;
    hipLaunchKernelGGL((k_unpack_tiles<T>), dim3((uint32_t)((uint64_t)a.n_frames * tpf)), dim3(kThreads), 0, st, a.terse,
                       (uint64_t)a.terse_bytes, a.frame_offsets, a.geom, tpf, a.widths, a.tile_off, static_cast<T*>(a.pixels_out), a.status, frame_mode);
    return hipGetLastError();
}
hipError_t launch_unpack_tiles(int dtype, const DecodeArgs& a, hipStream_t st, const uint32_t* frame_mode) {
    return for_pixel_type(dtype, [&]<class T>() { return launch_unpack_tiles_t<T>(a, st, frame_mode); });
}

hipError_t launch_walk_lds_only(const DecodeArgs& a, uint32_t max_w, const uint32_t* only, hipStream_t st, const uint32_t* list = nullptr);

// Fast path preconditions (checked by the caller): block = 12, frame offsets known, frames of < 2^32 bits (T-aligned pointers, any pixel count).
hipError_t launch_walk_only(const DecodeArgs& a, uint32_t max_w, bool clear_status, hipStream_t st) {
    if (a.plan.walk == Walk::kChain) {
        // large frames: one walk of many short parts writes the index (every frame through k_chain_index: not narrow); the
        // frames where that does not work out are listed and get theirs from the position-parallel walk
        hipError_t e = launch_chain_zero(a, max_w, clear_status, st);
        if (e != hipSuccess) return e;
        const uint32_t* mode = nullptr;
        e = launch_build_index_chain(a, max_w, &mode, st);
        if (e != hipSuccess) return e;
        return launch_seg_listed(a, max_w, st);
    }
    if (clear_status) zero_status(a.status, st);
    switch (a.plan.walk) {
    case Walk::kFrames: return launch_index_frames(max_w, a, false, st);        // (status cleared above if asked)
    case Walk::kSeg: return launch_seg_walk(a, max_w, st);
    case Walk::kLds: return launch_walk_lds_only(a, max_w, nullptr, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_walk_lds_only(const DecodeArgs& a, uint32_t max_w, const uint32_t* only, hipStream_t st, const uint32_t* list) {
    hipLaunchKernelGGL(k_walk_lds, dim3(a.n_frames), dim3(kWave), 0, st, a.terse, (uint64_t)a.terse_bytes,
                       a.frame_offsets, a.geom, max_w, a.widths, a.tile_off, only, list, a.status);
    return hipGetLastError();
}

hipError_t launch_decode_fast(int dtype, const DecodeArgs& a, hipStream_t st) {
    return for_pixel_type(dtype, [&]<class T>() { return launch_decode_fast_t<T>(a, st); });
}

}  // namespace trpx
