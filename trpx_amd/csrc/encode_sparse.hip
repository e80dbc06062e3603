// TERSE encode of a stack given as its events (trpx_encode_sparse): frame f is n_values zeros with
// px[f][positions[i]] = values[i] for i in [row_offsets[f], row_offsets[f + 1]) -- the CSR form trpx_decode_sparse writes.  The
// stream is byte for byte what trpx_encode writes for the dense frames; no dense frame ever exists in HBM.
//
// The two-pass pipeline of encode.hip with another source of pixels (the scans, the span logic and the packing are shared:
// encode_pack.hpp), all stream ordered, no host sync, every launch shape from n_frames / n_values / n_events alone:
//   k_se_bounds     per tile: the first event of its frame at or behind the tile's first pixel (binary search in the row)
//   k_se_tile_bits  events -> per-block OR of magnitudes in LDS -> widths -> bit length of every tile, prolix_bits
//   k_frame_scan, k_stack_scan                    (encode_pack.hpp)
//   k_se_validate   every row and every adjacent pair of events -> status[0] = TRPX_ERR_INVALID_ARG (behind the stack scan: it wins
//                   over CAPACITY; in front of the first store to `out`)
//   k_zero_edges                                  (encode_pack.hpp)
//   k_se_pack       events -> zeroed LDS pixel tile (a dword per pixel) -> LDS bit staging -> coalesced dword stores
// A tile without events is one explicit or repeated width-0 header and then one-bits: both passes leave it after reading its
// bounds, without touching LDS.
//
// Bad event lists are the caller's data, not a trusted structure: every row is clamped to [0, n_events] before it is used, every
// search runs inside the clamped row, and every LDS scatter is guarded by its own range check, whatever the searches found.
#include <algorithm>

#include "codec_common.hpp"
#include "encode_pack.hpp"
#include "launchers.hpp"

namespace trpx {

constexpr uint32_t kRunTiles = 8;   // consecutive tiles per workgroup of the two passes over the events

// Row f of the CSR, clamped: r0 <= r1 <= n_events whatever row_offsets holds.
__device__ __forceinline__ void row_range(const uint64_t* __restrict__ row_offsets, uint64_t f, uint64_t n_events, uint64_t& r0,
                                          uint64_t& r1) {
    const uint64_t a = row_offsets[f], b = row_offsets[f + 1];
    r0 = a < n_events ? a : n_events;
    r1 = b < n_events ? b : n_events;
    if (r1 < r0) r1 = r0;
}

// The events [e0, e1) of tile t of a frame (row [r0, r1)): inside the row whatever tile_lo holds.
__device__ __forceinline__ void tile_events(const uint32_t* __restrict__ tile_lo, uint64_t tile, uint32_t t, uint32_t n_tiles,
                                            uint64_t r0, uint64_t r1, uint64_t& e0, uint64_t& e1) {
    e0 = r0 + tile_lo[tile];
    if (e0 > r1) e0 = r1;
    e1 = t + 1 < n_tiles ? r0 + tile_lo[tile + 1] : r1;
    if (e1 > r1) e1 = r1;
    if (e1 < e0) e1 = e0;
}

// ---------------------------------------------------------------------------------------------
// K0: per tile, the number of events of its frame in front of the tile's first pixel.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_se_bounds(const uint64_t* __restrict__ row_offsets,
                                                        const uint32_t* __restrict__ positions, uint64_t n_events, FrameGeom g,
                                                        uint32_t n_frames, uint32_t* __restrict__ tile_lo) {
    const uint64_t tile = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (tile >= (uint64_t)n_frames * g.n_tiles) return;
    const uint64_t frame = tile / g.n_tiles;
    const uint64_t p0 = (tile % g.n_tiles) * (uint64_t)kTileValues;
    uint64_t r0, r1;
    row_range(row_offsets, frame, n_events, r0, r1);
    uint64_t lo = r0, hi = r1;
    while (lo < hi) {                                       // lower bound of p0 (sorted rows; any row: lo stays in [r0, r1])
        const uint64_t mid = lo + (hi - lo) / 2;
        if (positions[mid] < p0) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t n = lo - r0;
    tile_lo[tile] = n < 0xFFFFFFFFull ? (uint32_t)n : 0xFFFFFFFFu;   // (a valid row has < 2^32 events: positions are 32-bit and ascend)
}

// Width of the block in front of tile t (0 at a frame's start): the events of the twelve pixels below p0 lie just below e0.
template <typename T>
__device__ __forceinline__ uint32_t halo_width(const uint32_t* __restrict__ positions, const T* __restrict__ values, uint64_t r0,
                                               uint64_t e0, uint64_t p0) {
    uint32_t m = 0;
    for (uint64_t i = e0; i > r0 && e0 - i < (uint64_t)kBlock; --i) {
        const uint64_t p = positions[i - 1];
        if (p >= p0 || p + kBlock < p0) break;
        m |= magnitude<T>(values[i - 1]);
    }
    return width_from_or<T>(m);
}

// The tile's events into the zeroed LDS pixel tile, then this thread's block from there, its width and -- through s_w -- the width
// of the block before it.  Contains three __syncthreads().
template <typename T>
__device__ __forceinline__ void blocks_from_events(const uint32_t* __restrict__ positions, const T* __restrict__ values,
                                                   uint64_t e0, uint64_t e1, uint64_t p0, const FrameGeom& g, uint32_t t,
                                                   uint32_t w_halo, uint32_t* s_px, uint32_t* s_w, BlockReg<T> (&v)[kBlock], int& nb, uint32_t& w,
                                                   uint32_t& w_prev, bool& valid) {
    const uint32_t tid = threadIdx.x;
    uint4* z = reinterpret_cast<uint4*>(s_px);            // (dwords through a vector of dwords: 3 stores per thread)
    for (uint32_t i = tid; i < (uint32_t)kTileValues / 4; i += kThreads) z[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (uint64_t i = e0 + tid; i < e1; i += kThreads) {
        const uint64_t p = positions[i], rel = p - p0;       // (p < p0 wraps to a huge rel)
        if (rel < (uint64_t)kTileValues && p < g.n_values) s_px[rel] = (uint32_t)values[i];   // the scatter's own range check
    }
    __syncthreads();
    const uint32_t b = t * kTileBlocks + tid;
    valid = b < g.n_blocks;
    nb = 0;
    w = 0;
    if (valid) {
        const uint64_t first = (uint64_t)b * kBlock;
        nb = first + kBlock <= g.n_values ? kBlock : (int)(g.n_values - first);   // (pixels past n_values were never scattered: zero)
#pragma unroll
        for (int k = 0; k < kBlock; ++k) v[k] = (T)s_px[tid * kBlock + k];
        w = block_width<T>(v);
    }
    s_w[tid + 1] = w;
    if (tid == 0) s_w[0] = w_halo;
    __syncthreads();
    w_prev = s_w[tid];
}

// A tile without events: one header for width 0 behind width w_halo, then a repeat bit per block.
__device__ __forceinline__ uint32_t empty_tile_bits(uint32_t n_blk, uint32_t w_halo) { return header_len(0u, w_halo) + n_blk - 1u; }

// ---------------------------------------------------------------------------------------------
// K1: bit length of every tile + prolix_bits.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void k_se_tile_bits(const uint64_t* __restrict__ row_offsets,
                                                           const uint32_t* __restrict__ positions, const T* __restrict__ values,
                                                           uint64_t n_events, FrameGeom g, uint32_t n_frames,
                                                           const uint32_t* __restrict__ tile_lo,
                                                           uint32_t* __restrict__ tile_bits, uint32_t* __restrict__ status) {
    __shared__ uint32_t s_w[kThreads + 1];                  // OR of the magnitudes of every block's events; [0]: the block before
    __shared__ uint32_t s_tot[4];
    __shared__ uint32_t s_max[4];
  // a workgroup takes a run of kRunTiles consecutive tiles (they may cross a frame's end): most tiles of a sparse stack are a few
  // loads' work, and 172 000 workgroups of that cost more to launch than to run
  const uint64_t tile_end = min((uint64_t)n_frames * g.n_tiles, ((uint64_t)blockIdx.x + 1) * kRunTiles);
  for (uint64_t tile = (uint64_t)blockIdx.x * kRunTiles; tile < tile_end; ++tile) {
    const uint64_t frame = tile / g.n_tiles;
    const uint32_t t = (uint32_t)(tile % g.n_tiles);
    const uint64_t p0 = (uint64_t)t * kTileValues;
    uint64_t r0, r1, e0, e1;
    row_range(row_offsets, frame, n_events, r0, r1);
    tile_events(tile_lo, tile, t, g.n_tiles, r0, r1, e0, e1);
    const uint32_t w_halo = t ? halo_width<T>(positions, values, r0, e0, p0) : 0u;
    if (e0 == e1) {                                         // (uniform: nothing below depends on the lane)
        const uint32_t n_blk = min((uint32_t)kTileBlocks, g.n_blocks - t * kTileBlocks);
        if (threadIdx.x == 0) tile_bits[tile] = empty_tile_bits(n_blk, w_halo);
        continue;
    }

    // a block's width needs only the OR of its values' magnitudes (zeros add nothing): one LDS word per block, no pixel tile
    const uint32_t tid = threadIdx.x;
    s_w[tid + 1] = 0u;
    __syncthreads();
    for (uint64_t i = e0 + tid; i < e1; i += kThreads) {
        const uint64_t p = positions[i], rel = p - p0;       // (p < p0 wraps to a huge rel)
        if (rel < (uint64_t)kTileValues && p < g.n_values) {  // the scatter's own range check
            const uint32_t m = magnitude<T>(values[i]);
            if (m) atomicOr(&s_w[1 + (uint32_t)rel / kBlock], m);
        }
    }
    __syncthreads();
    const uint32_t b = t * kTileBlocks + tid;
    const bool valid = b < g.n_blocks;
    const uint32_t w = width_from_or<T>(s_w[tid + 1]);
    const uint32_t w_left = tid ? width_from_or<T>(s_w[tid]) : w_halo;
    const uint64_t left = valid ? g.n_values - (uint64_t)b * kBlock : 0u;      // values of the block (the frame's last may be partial)
    const uint32_t nb = left < (uint64_t)kBlock ? (uint32_t)left : (uint32_t)kBlock;
    const uint32_t len = valid ? header_len(w, w_left) + nb * w : 0u;
    uint32_t total;
    block_exclusive_scan(len, s_tot, &total);
    const uint32_t mx = wave_max(w);
    if (lane_id() == 0) s_max[wave_id()] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_bits[tile] = total;
        const uint32_t m = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        // d_prolix_bits (Terse.hpp:516): read first, as k_tile_bits does
        if (m > __hip_atomic_load(&status[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&status[1], m);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Validation: row_offsets non-decreasing and ending inside the lists; every position < n_values and above its left neighbour
// in the row.  Grid (n_frames, chunks): workgroup (f, c) takes the events r0 + c * 256 + tid, + chunks * 256, ... of row f.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_se_validate(const uint64_t* __restrict__ row_offsets,
                                                          const uint32_t* __restrict__ positions, uint64_t n_events,
                                                          uint64_t n_values, uint32_t n_frames, uint32_t* __restrict__ status) {
    const uint64_t frame = blockIdx.x;
    bool bad = false;
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        const uint64_t a = row_offsets[frame], b = row_offsets[frame + 1];
        bad = a > b || (frame + 1 == n_frames && b > n_events);
    }
    uint64_t r0, r1;
    row_range(row_offsets, frame, n_events, r0, r1);
    for (uint64_t i = r0 + (uint64_t)blockIdx.y * kThreads + threadIdx.x; i < r1; i += (uint64_t)gridDim.y * kThreads) {
        const uint32_t p = positions[i];
        bad |= p >= n_values || (i > r0 && positions[i - 1] >= p);
    }
    if (bad) status[0] = kStatusInvalid;                     // (plain store behind k_stack_scan's: INVALID_ARG wins over CAPACITY)
}

// ---------------------------------------------------------------------------------------------
// K3: pack.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void k_se_pack(const uint64_t* __restrict__ row_offsets,
                                                      const uint32_t* __restrict__ positions, const T* __restrict__ values,
                                                      uint64_t n_events, FrameGeom g, uint32_t n_frames,
                                                      const uint32_t* __restrict__ tile_lo,
                                                      const uint64_t* __restrict__ tile_off,
                                                      const uint64_t* __restrict__ frame_offsets, uint32_t* __restrict__ out32,
                                                      const uint32_t* __restrict__ status) {
    constexpr int kStage = stage_dwords<T>();
    __shared__ __attribute__((aligned(16))) uint32_t s_px[kTileValues];   // one dword per pixel, whatever the type: whole-dword LDS stores only
    __shared__ uint32_t s_stage[kStage];
    __shared__ uint32_t s_w[kThreads + 1];
    __shared__ uint32_t s_tot[4];
    if (status[0] != 0) return;                             // bad events, capacity: write nothing
    const uint32_t tid = threadIdx.x;
  const uint64_t tile_end = min((uint64_t)n_frames * g.n_tiles, ((uint64_t)blockIdx.x + 1) * kRunTiles);
  for (uint64_t tile = (uint64_t)blockIdx.x * kRunTiles; tile < tile_end; ++tile) {   // (a run of tiles, as k_se_tile_bits)
    const uint64_t frame = tile / g.n_tiles;
    const uint32_t t = (uint32_t)(tile % g.n_tiles);
    const uint64_t p0 = (uint64_t)t * kTileValues;
    const bool last_tile = t + 1 == g.n_tiles;
    uint64_t r0, r1, e0, e1;
    row_range(row_offsets, frame, n_events, r0, r1);
    tile_events(tile_lo, tile, t, g.n_tiles, r0, r1, e0, e1);
    const uint32_t w_halo = t ? halo_width<T>(positions, values, r0, e0, p0) : 0u;
    if (e0 == e1) {
        // the image is constant: (w_halo != 0: four zero bits, the explicit width-0 header) one-bits up to the tile's length
        const uint32_t n_blk = min((uint32_t)kTileBlocks, g.n_blocks - t * kTileBlocks);
        const uint32_t total = empty_tile_bits(n_blk, w_halo);
        const Span s = tile_span(frame_offsets[frame], frame_offsets[frame + 1], tile_off[tile], total, last_tile);
        const uint32_t one0 = s.s0 + (w_halo ? 4u : 0u), one1 = s.s0 + total;   // the one-bits, in bits from dword d0
        store_span_from([&](uint32_t j) {
            const uint32_t lo = max(one0, 32u * j), hi = min(one1, 32u * j + 32u);
            return hi > lo ? field_mask(hi - lo) << (lo - 32u * j) : 0u;
        }, s, out32);
        continue;
    }

    BlockReg<T> v[kBlock];
    int nb; uint32_t w, w_prev; bool valid;
    blocks_from_events<T>(positions, values, e0, e1, p0, g, t, w_halo, s_px, s_w, v, nb, w, w_prev, valid);
    const uint32_t hl = header_len(w, w_prev);
    const uint32_t len = valid ? hl + (uint32_t)nb * w : 0u;
    uint32_t total;
    const uint32_t excl = block_exclusive_scan(len, s_tot, &total);

    // only the part of the staging image this tile reaches is cleared (a sparse tile is a few hundred bits of kStage dwords)
    const uint32_t need = min((uint32_t)kStage, (31u + total + 8u + 31u) / 32u + 1u);
    for (uint32_t i = tid; i < need; i += kThreads) s_stage[i] = 0u;
    __syncthreads();

    const Span s = tile_span(frame_offsets[frame], frame_offsets[frame + 1], tile_off[tile], total, last_tile);
    if (valid) pack_block<T>(s_stage, s.s0 + excl, v, nb, w, w_prev, hl);
    __syncthreads();
    store_span(s_stage, s, out32);                          // (the next tile's first store to s_stage lies behind four barriers)
  }
}

// ---------------------------------------------------------------------------------------------
// Host-side launcher (called by the C ABI in api.hip).
// ---------------------------------------------------------------------------------------------
template <typename T>
static hipError_t launch_encode_sparse_t(const SparseEncodeArgs& a, hipStream_t st) {
    const FrameGeom g = a.geom;
    const uint64_t n_tiles_total = (uint64_t)a.n_frames * g.n_tiles;
    const T* val = static_cast<const T*>(a.values);
    uint32_t* out32 = reinterpret_cast<uint32_t*>(a.out);
    const dim3 grid((uint32_t)((n_tiles_total + kRunTiles - 1) / kRunTiles)), per_tile((uint32_t)((n_tiles_total + kThreads - 1) / kThreads)), blk(kThreads);
    // validation: about four rounds of an average row per workgroup, at most 64 workgroups per row
    const uint64_t per_frame = a.n_events / a.n_frames;
    const uint32_t chunks = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, (per_frame + 4 * kThreads - 1) / (4 * kThreads)));

    zero_status(a.status, st);
    hipLaunchKernelGGL(k_se_bounds, per_tile, blk, 0, st, a.row_offsets, a.positions, a.n_events, g, a.n_frames, a.tile_lo);
    hipLaunchKernelGGL((k_se_tile_bits<T>), grid, blk, 0, st, a.row_offsets, a.positions, val, a.n_events, g, a.n_frames, a.tile_lo,
                       a.tile_bits, a.status);
    hipLaunchKernelGGL(k_frame_scan, dim3(a.n_frames), blk, 0, st, a.tile_bits, g, a.tile_off, a.frame_size);
    hipLaunchKernelGGL(k_stack_scan, dim3(1), blk, 0, st, a.frame_size, a.n_frames, (uint64_t)a.out_capacity,
                       a.frame_offsets, a.status);
    hipLaunchKernelGGL(k_se_validate, dim3(a.n_frames, chunks), blk, 0, st, a.row_offsets, a.positions, a.n_events,
                       g.n_values, a.n_frames, a.status);
    hipLaunchKernelGGL(k_zero_edges, per_tile, blk, 0, st, g, a.n_frames, a.tile_off, a.tile_bits, a.frame_offsets, out32,
                       a.status);
    hipLaunchKernelGGL((k_se_pack<T>), grid, blk, 0, st, a.row_offsets, a.positions, val, a.n_events, g, a.n_frames, a.tile_lo, a.tile_off,
                       a.frame_offsets, out32, a.status);
    return hipGetLastError();
}

hipError_t launch_encode_sparse(int dtype, const SparseEncodeArgs& a, hipStream_t st) {
    return for_pixel_type(dtype, [&]<class T>() { return launch_encode_sparse_t<T>(a, st); });
}

}  // namespace trpx
