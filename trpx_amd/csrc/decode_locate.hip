// Frame locator for stacks without an index (a .trpx file stores none, Terse.hpp:454-474): frame_offsets[0 .. n_frames] of
// the stack, stream-ordered on the caller's device copy (trpx_locate_frames).  The next frame starts at 1 + bits/8
// (Terse.hpp:547).  Two routes, both reporting TRPX_ERR_CORRUPT where k_walk_serial does (a chain past terse_bytes, a width
// above max_w, fewer frames than asked):
//
// * serial (k_locate_serial): the frames walked one after another by one wavefront (walk_serial.hpp: the run-skipping header
//   walk of Terse.hpp:360-372, count only).  Every block size and max_w; small stacks; TRPX_LOCATE_PATH=serial.
// * position-parallel (block 12, max_w <= 32), five launches:
//   1. k_loc_chunks -- the stream cut into chunks of kLocChunkBits; one wavefront per chunk walks the frame-oblivious header
//      chain (every block 12 values) from a guessed state (its first bit, previous width 0) to the chunk's end and leaves a
//      checkpoint in every window of kLocWinBits bits: the first block start of its chain there (bit, previous width, blocks
//      from the chunk's start).
//   2. k_loc_links -- each chain goes on past its chunk until it lands on a checkpoint of a later chunk's chain (the first one
//      met, not only the next): from there the two are one chain, so block counts carry over.  Chains that meet nothing within
//      kLocLinkBits / kLocLinkBlocks stay open.  The walk past the chunk leaves a checkpoint in each of its first 64 windows
//      too (ext), so that a frame whose last block lies on it before the link need not walk there from the chunk's end.
//   3. k_loc_chase -- one wavefront, frame by frame: the frame's chain from (its first bit, width 0) until it lands on any
//      checkpoint, then its last block by block counts along the links, the nearest checkpoint and a walk of less than one
//      window; next start = 1 + bits/8.  On a valid stream every step is exact: landing means equal state, and equal states
//      have equal futures.
//   4. k_loc_verify -- one wavefront per frame walks it from its proposed offset (walk_serial.hpp, with every check the serial
//      route makes) and compares the end with the next offset; a mismatch records the first such frame.
//   5. k_loc_repair -- exits at once unless a frame failed; else the serial walk from the first failed frame on, skipping
//      frames whose proposed start turned out true and whose verification passed.  So the serial walk decides every status.
// Workspace: locate_workspace_bytes() -- 256 bytes + a flag byte per frame + 8 bytes per window (terse_bytes / 64) + as many
// for the checkpoints of the chains' walks past their chunks + 32 bytes per chunk.  Nothing waits on another workgroup; the host reads nothing.
#include <cstdlib>
#include <cstring>

#include "codec_common.hpp"
#include "launchers.hpp"
#include "walk_serial.hpp"

namespace trpx {

namespace {

constexpr uint32_t kLocWinLog = 12;                                       // checkpoint window: 4096 bits
constexpr uint64_t kLocWinBits = 1ull << kLocWinLog;
constexpr uint32_t kLocWinPerChunk = 64;                                  // chunk: 64 windows = 256 Kbit
constexpr uint64_t kLocChunkBits = kLocWinBits * kLocWinPerChunk;
constexpr uint64_t kLocLinkBits = 4 * kLocChunkBits;                      // how far a chain looks for a later chunk's chain,
constexpr uint64_t kLocLinkBlocks = 8192;                                  // in bits and in blocks (a false chain can crawl
                                                                           // through 1-bit blocks of width 0)
constexpr uint32_t kLocExtWins = 64;                                      // checkpoints of a chain's walk past its chunk
constexpr uint64_t kCpValid = 1ull << 63;
constexpr uint32_t kCpExplicit = 0xFFu;                                    // checkpoint tag: the block has an explicit header
// parallel route only for stacks of at least this many frames and bytes (below, the serial walk is as fast as five launches)
constexpr uint32_t kLocMinFrames = 4;
constexpr uint64_t kLocMinBytes = 8192;

struct LocLayout { size_t flags, cp, ext, chunks, total; uint64_t n_win, n_chunks; };
LocLayout loc_layout(uint64_t terse_bytes, uint64_t n_frames) {
    LocLayout l;
    l.n_win = (8 * terse_bytes + kLocWinBits - 1) >> kLocWinLog;
    l.n_chunks = (l.n_win + kLocWinPerChunk - 1) / kLocWinPerChunk;
    l.flags = 256;                                                        // [0, 256): word 0 = first failed frame
    l.cp = align_up(l.flags + n_frames, 256);
    l.ext = l.cp + 8 * l.n_chunks * kLocWinPerChunk;
    l.chunks = l.ext + 8 * l.n_chunks * kLocExtWins;
    l.total = l.chunks + 32 * l.n_chunks;
    return l;
}

// Chunk record (4 x u64): [0] state at its chain's first block start at or past the chunk's end: blocks << 24 | width << 16 |
// (bit - chunk end); [1] link: kCpValid | window of the checkpoint it landed on (0: open); [2] blocks from the chunk's start to
// that checkpoint; [3] the checkpoint's own block count (in its chunk's chain).
struct ChainHit { uint64_t blocks; uint64_t cp; };          // blocks advanced; the checkpoint landed on (0: none)

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, 64);
}
// the same from a wave-uniform lane (a ballot's): v_readlane instead of a trip through the LDS crossbar
__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t src) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)src) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)src);
}

// The frame-oblivious header chain (Terse.hpp:360-372, every block 12 values), one wavefront, 64 candidate block starts per
// step as in walk_serial.hpp.  State in front of a block: (pos, w) = its first bit, the width of the block before.  A width
// above max_w reads as 0: any fixed rule does, since the true chain of a valid stream never meets one.  Advances from (pos, w)
// until nblk blocks are done, or the next block start is at or past stop_bit, or (kMode 1) it lands on a checkpoint of a window
// in [win_lo, win_hi); kMode 2 stores a checkpoint in every window of [st_lo, st_hi) the chain enters (cp_out[window - st_lo];
// blocks counted from blk0); kMode 3 does both.  pos / w are left at the state where it stopped.
// Readers of the stream and the checkpoints: straight from global memory (the chunk launches: every wavefront reads its own
// chunk once), or through a window in LDS (the chase: its walks are short and land on lines nobody has touched, so a step
// that waits for memory costs an HBM round trip; one cooperative load of 16 KB + the checkpoints of its windows instead).
struct GlobalRd {
    const uint32_t* __restrict__ s32;
    uint64_t n_dw;
    const uint64_t* __restrict__ cp;
    __device__ void ensure(uint64_t, uint32_t) {}
    __device__ uint32_t peek(uint64_t abit) const { return peek32(s32, n_dw, abit); }
    __device__ uint64_t cpat(uint64_t win) const { return cp[win]; }
};
constexpr uint32_t kLdsDw = 4096;                                          // stream window of the chase: 16 KB
constexpr uint32_t kLdsWins = kLdsDw * 32 / kLocWinBits;                   // = its 32 checkpoint windows
struct LdsRd {
    const uint32_t* __restrict__ s32;
    uint64_t n_dw;
    const uint64_t* __restrict__ cp;
    uint64_t n_win;
    uint32_t* dw;                                                          // LDS: kLdsDw stream dwords from base
    uint64_t* lcp;                                                         // LDS: checkpoints of windows base / 128 ..
    uint64_t base;
    __device__ void load(uint64_t dw0) {                                   // (wave-uniform; one wavefront per workgroup)
        base = dw0 & ~(uint64_t)(kLocWinBits / 32 - 1);                    // on a checkpoint window
        const uint32_t lane = (uint32_t)lane_id();
        __syncthreads();
        constexpr uint32_t kBatch = 8;                                     // 16-byte loads in flight per lane
#pragma unroll
        for (uint32_t r = 0; r < kLdsDw / (4 * kWave); r += kBatch) {
            uint4 v[kBatch];
#pragma unroll
            for (uint32_t k = 0; k < kBatch; ++k) {
                const uint64_t i = base + 4ull * ((r + k) * kWave + lane);      // (base: a multiple of 128 dwords)
                if (i + 3 < n_dw) v[k] = *reinterpret_cast<const uint4*>(s32 + i);
                else v[k] = make_uint4(ld_stream_dw(s32, i, n_dw), ld_stream_dw(s32, i + 1, n_dw), ld_stream_dw(s32, i + 2, n_dw),
                                       ld_stream_dw(s32, i + 3, n_dw));
            }
#pragma unroll
            for (uint32_t k = 0; k < kBatch; ++k) reinterpret_cast<uint4*>(dw)[(r + k) * kWave + lane] = v[k];
        }
        const uint64_t w0 = base * 32 / kLocWinBits;
        if (lane < kLdsWins) lcp[lane] = w0 + lane < n_win ? cp[w0 + lane] : 0ull;
        __syncthreads();
    }
    __device__ void ensure(uint64_t pos, uint32_t span_bits) {            // the step's candidates [pos, pos + span) inside
        if ((pos >> 5) < base || ((pos + span_bits) >> 5) + 2 > base + kLdsDw) load(pos >> 5);
    }
    __device__ uint32_t peek(uint64_t abit) const {
        const uint64_t di = (abit >> 5) - base;
        if (di + 1 >= kLdsDw) return peek32(s32, n_dw, abit);              // (abit < base wraps: also global)
        const uint64_t x = (uint64_t)dw[di] | ((uint64_t)dw[di + 1] << 32);
        return (uint32_t)(x >> (abit & 31));
    }
    __device__ uint64_t cpat(uint64_t win) const {
        const uint64_t wi = win - base * 32 / kLocWinBits;
        return wi < kLdsWins ? lcp[wi] : cp[win];
    }
};

template <int kMode, class Rd>
__device__ ChainHit chain_walk(Rd& rd, uint64_t& pos, uint32_t& w, uint64_t nblk, uint64_t stop_bit, uint32_t max_w,
                               uint64_t* __restrict__ cp_out, uint64_t win_lo, uint64_t win_hi, uint64_t st_lo, uint64_t st_hi,
                               uint64_t blk0) {
    const uint32_t lane = (uint32_t)lane_id();
    uint64_t b = 0, last_win = ~0ull;
    while (true) {
        const uint32_t stride = 1u + 12u * w;
        rd.ensure(pos, 64u * stride + 32u);
        const uint64_t cb = b + lane;
        const uint64_t cpos = pos + (uint64_t)lane * stride;
        const uint32_t bits = rd.peek(cpos);
        const uint64_t not_same = __ballot(!(bits & 1u));
        const uint32_t first = not_same ? (uint32_t)__builtin_ctzll(not_same) : 64u;
        const uint64_t win = cpos >> kLocWinLog;
        bool stop = lane <= first && (cb >= nblk || cpos >= stop_bit);
        uint64_t cpv = 0;
        if constexpr (kMode == 1 || kMode == 3) {
            if (lane <= first && !stop && win >= win_lo && win < win_hi) {
                cpv = rd.cpat(win);
                const uint32_t tag = (uint32_t)(cpv >> 16) & 0xFFu;
                if (!(cpv & kCpValid) || (cpv & (kLocWinBits - 1)) != (cpos & (kLocWinBits - 1)) || (tag != kCpExplicit && tag != w))
                    cpv = 0;
            }
            stop = stop || cpv != 0;
        }
        const uint64_t stop_mask = __ballot(stop);
        const uint32_t end = stop_mask ? (uint32_t)__builtin_ctzll(stop_mask) : 65u;   // lanes < end are walked blocks
        if constexpr (kMode == 2 || kMode == 3) {
            const uint64_t prev_win = shfl64(win, lane ? (int)lane - 1 : 0);
            const bool opens = win != (lane ? prev_win : last_win);     // the chain's first block start in this window
            if (lane < end && lane <= first && opens && win >= st_lo && win < st_hi)
                cp_out[win - st_lo] = kCpValid | (blk0 + cb) << 24 | (uint64_t)(first == lane ? kCpExplicit : w) << 16 |
                              (cpos & (kLocWinBits - 1));
            last_win = readlane64(win, first < 63u ? first : 63u);
        }
        if (stop_mask) {
            pos = readlane64(cpos, end);
            return {b + end, kMode == 1 || kMode == 3 ? readlane64(cpv, end) : 0ull};
        }
        if (first < 64u) {                                                 // explicit header
            auto [nw, hl] = parse_explicit_header(bits);
            if (nw > max_w) nw = 0;
            const uint64_t npos = cpos + hl + 12ull * nw;
            pos = readlane64(npos, first);
            w = (uint32_t)__builtin_amdgcn_readlane((int)nw, (int)first);
            b += first + 1;
        } else {
            pos += 64ull * stride;
            b += 64;
        }
    }
}

__global__ __launch_bounds__(kWave) void k_locate_serial(const uint8_t* __restrict__ terse, uint64_t terse_bytes, uint32_t n_frames,
                                                         FrameGeom g, uint32_t max_w, uint64_t* __restrict__ offsets,
                                                         uint32_t* __restrict__ status) {
    uint64_t fo = 0;
    bool ok = true;
    if (lane_id() == 0) offsets[0] = 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
        uint64_t bits = ~0ull;
        if (ok && fo < terse_bytes)
            bits = walk_frame<false>(reinterpret_cast<const uint32_t*>(terse), (terse_bytes + 3) / 4, 8 * fo,
                                     8 * (terse_bytes - fo), g, max_w, nullptr, nullptr);
        if (bits == ~0ull) { ok = false; bits = 0; }
        fo += ok ? 1 + bits / 8 : 0;
        if (lane_id() == 0) offsets[f + 1] = fo;
    }
    if (lane_id() == 0 && !ok) atomicMax(&status[0], kStatusCorrupt);
}

// 1. one wavefront per chunk: its chain from (first bit, 0) to the chunk's end, a checkpoint per window
__global__ __launch_bounds__(kWave) void k_loc_chunks(const uint32_t* __restrict__ s32, uint64_t n_dw, uint64_t n_win, uint32_t max_w,
                                                      uint64_t* __restrict__ cp, uint64_t* __restrict__ chunks,
                                                      uint32_t* __restrict__ first_bad) {
    const uint64_t c = blockIdx.x;
    if (c == 0 && lane_id() == 0) *first_bad = ~0u;
    const uint64_t w_lo = c * kLocWinPerChunk, w_hi = w_lo + kLocWinPerChunk < n_win ? w_lo + kLocWinPerChunk : n_win;
    uint64_t pos = w_lo << kLocWinLog;
    uint32_t w = 0;
    const uint64_t end_bit = w_hi << kLocWinLog;
    GlobalRd rd{s32, n_dw, nullptr};
    const ChainHit h = chain_walk<2>(rd, pos, w, ~0ull, end_bit, max_w, cp + w_lo, 0, 0, w_lo, w_hi, 0);
    if (lane_id() == 0) chunks[4 * c] = h.blocks << 24 | (uint64_t)w << 16 | (pos - end_bit);
}

// 2. one wavefront per chunk: its chain on past the chunk until it lands on a checkpoint of a later chunk's chain
__global__ __launch_bounds__(kWave) void k_loc_links(const uint32_t* __restrict__ s32, uint64_t n_dw, uint64_t n_win, uint32_t max_w,
                                                     const uint64_t* __restrict__ cp, uint64_t* __restrict__ ext,
                                                     uint64_t* __restrict__ chunks) {
    const uint64_t c = blockIdx.x;
    ext[c * kLocExtWins + lane_id()] = 0ull;                               // (entries this walk does not reach stay empty)
    __syncthreads();
    const uint64_t w_hi = (c + 1) * kLocWinPerChunk < n_win ? (c + 1) * kLocWinPerChunk : n_win;
    const uint64_t rec = chunks[4 * c];
    uint64_t pos = (w_hi << kLocWinLog) + (rec & 0xFFFFu);
    uint32_t w = (uint32_t)(rec >> 16) & 0xFFu;
    const uint64_t blk = rec >> 24;
    const uint64_t stop = (w_hi << kLocWinLog) + kLocLinkBits;
    ChainHit h{0, 0};
    __shared__ __attribute__((aligned(16))) uint32_t win_dw[kLdsDw];
    __shared__ uint64_t win_cp[kLdsWins];
    LdsRd rd{s32, n_dw, cp, n_win, win_dw, win_cp, 0};
    if (w_hi < n_win) {
        rd.load(pos >> 5);
        h = chain_walk<3>(rd, pos, w, kLocLinkBlocks, stop, max_w, ext + c * kLocExtWins, w_hi, n_win, w_hi, w_hi + kLocExtWins,
                          blk);
    }
    if (lane_id() == 0) {
        chunks[4 * c + 1] = h.cp ? kCpValid | (pos >> kLocWinLog) : 0ull;
        chunks[4 * c + 2] = blk + h.blocks;
        chunks[4 * c + 3] = h.cp >> 24 & ((1ull << 39) - 1);
    }
}

// 3. one wavefront: the frames one after another, each by a landing walk, block counts along the links and a short walk
__global__ __launch_bounds__(kWave) void k_loc_chase(const uint32_t* __restrict__ s32, uint64_t n_dw, uint64_t terse_bytes,
                                                     uint64_t n_win, uint32_t n_frames, FrameGeom g, uint32_t max_w,
                                                     const uint64_t* __restrict__ cp, const uint64_t* __restrict__ ext,
                                                     const uint64_t* __restrict__ chunks, uint64_t* __restrict__ offsets) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t n_chunks = (n_win + kLocWinPerChunk - 1) / kLocWinPerChunk;
    const uint32_t nb_last = (uint32_t)(g.n_values - (uint64_t)(g.n_blocks - 1) * 12u);
    __shared__ __attribute__((aligned(16))) uint32_t win_dw[kLdsDw];
    __shared__ uint64_t win_cp[kLdsWins];
    LdsRd rd{s32, n_dw, cp, n_win, win_dw, win_cp, 0};
    rd.load(0);
    uint64_t s = 0;
    if (lane == 0) offsets[0] = 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
        if (s < terse_bytes) {
            uint64_t pos = 8 * s;
            uint32_t w = 0;
            uint64_t rem = g.n_blocks - 1;                                 // blocks in front of the frame's last block
            const ChainHit h = chain_walk<1>(rd, pos, w, rem, ~0ull, max_w, nullptr, 0, n_win, 0, 0, 0);
            rem -= h.blocks;
            if (h.cp) {                                                    // landed: the frame's chain is a chunk chain from here
                uint64_t c = (pos >> kLocWinLog) / kLocWinPerChunk;
                uint64_t blk = h.cp >> 24 & ((1ull << 39) - 1);
                for (uint64_t hop = 0; hop < n_chunks; ++hop) {            // along the links while the last block lies beyond
                    const uint64_t link = chunks[4 * c + 1], at = chunks[4 * c + 2];
                    if (!(link & kCpValid) || blk + rem < at) break;
                    rem -= at - blk;
                    blk = chunks[4 * c + 3];
                    c = (link & ~kCpValid) / kLocWinPerChunk;
                }
                const uint64_t target = blk + rem;
                const uint64_t rec = chunks[4 * c];
                const uint64_t w_hi = (c + 1) * kLocWinPerChunk < n_win ? (c + 1) * kLocWinPerChunk : n_win;
                uint64_t from_blk;
                if (target >= (rec >> 24)) {                               // past the chunk: the checkpoints of its walk on
                    const uint64_t v = ext[c * kLocExtWins + lane];
                    const uint64_t ok = __ballot((v & kCpValid) && (v >> 24 & ((1ull << 39) - 1)) <= target);
                    if (ok) {
                        const uint32_t src = 63u - (uint32_t)__builtin_clzll(ok);
                        const uint64_t vs = readlane64(v, src);
                        pos = ((w_hi + src) << kLocWinLog) + (vs & (kLocWinBits - 1));
                        const uint32_t tag = (uint32_t)(vs >> 16) & 0xFFu;
                        w = tag == kCpExplicit ? 0u : tag;
                        from_blk = vs >> 24 & ((1ull << 39) - 1);
                    } else {                                               // (none: from the chain's state at the chunk's end)
                        pos = (w_hi << kLocWinLog) + (rec & 0xFFFFu);
                        w = (uint32_t)(rec >> 16) & 0xFFu;
                        from_blk = rec >> 24;
                    }
                } else {                                                   // the nearest checkpoint at or before the last block
                    const uint64_t wi = c * kLocWinPerChunk + lane;
                    const uint64_t v = wi < w_hi ? cp[wi] : 0ull;
                    const uint64_t ok = __ballot((v & kCpValid) && (v >> 24 & ((1ull << 39) - 1)) <= target);
                    const int src = ok ? 63 - __builtin_clzll(ok) : 0;     // (a checkpoint at or before `blk` exists: ok != 0)
                    const uint64_t vs = readlane64(v, (uint32_t)src);
                    pos = ((c * kLocWinPerChunk + (uint64_t)src) << kLocWinLog) + (vs & (kLocWinBits - 1));
                    const uint32_t tag = (uint32_t)(vs >> 16) & 0xFFu;
                    w = tag == kCpExplicit ? 0u : tag;                     // (an explicit header does not read the width before)
                    from_blk = vs >> 24 & ((1ull << 39) - 1);
                }
                chain_walk<0>(rd, pos, w, target >= from_blk ? target - from_blk : 0, ~0ull, max_w, nullptr, 0, 0, 0, 0, 0);
            }
            // the last block (nb_last values): its header at pos, width before it w
            const uint32_t bits = rd.peek(pos);
            uint64_t fin;
            if (bits & 1u) fin = pos + 1 + (uint64_t)nb_last * w;
            else {
                const auto [nw, hl] = parse_explicit_header(bits);
                fin = pos + hl + (uint64_t)nb_last * nw;
            }
            s += 1 + (fin - 8 * s) / 8;
        }
        if (lane == 0) offsets[f + 1] = s;
    }
}

// 4. one wavefront per frame: the serial walk of frame f from its proposed start must end where frame f + 1 is proposed to start
__global__ __launch_bounds__(kWave) void k_loc_verify(const uint8_t* __restrict__ terse, uint64_t terse_bytes, FrameGeom g, uint32_t max_w,
                                                      const uint64_t* __restrict__ offsets, uint8_t* __restrict__ flags,
                                                      uint32_t* __restrict__ first_bad) {
    const uint32_t f = blockIdx.x;
    const uint64_t fo = offsets[f], next = offsets[f + 1];
    bool ok = fo < terse_bytes;
    if (ok) {
        const uint64_t bits = walk_frame<false>(reinterpret_cast<const uint32_t*>(terse), (terse_bytes + 3) / 4, 8 * fo,
                                                8 * (terse_bytes - fo), g, max_w, nullptr, nullptr);
        ok = bits != ~0ull && fo + 1 + bits / 8 == next;
    }
    if (lane_id() == 0) {
        flags[f] = ok ? 1 : 0;
        if (!ok) atomicMin(first_bad, f);
    }
}

// 5. the serial walk from the first failed frame on (k_locate_serial's steps); exits at once when every frame verified
__global__ __launch_bounds__(kWave) void k_loc_repair(const uint8_t* __restrict__ terse, uint64_t terse_bytes, uint32_t n_frames,
                                                      FrameGeom g, uint32_t max_w, uint64_t* __restrict__ offsets,
                                                      const uint8_t* __restrict__ flags, const uint32_t* __restrict__ first_bad,
                                                      uint32_t* __restrict__ status) {
    const uint32_t j = *first_bad;
    if (j >= n_frames) return;
    uint64_t fo = offsets[j], prop = fo;                                   // frames < j verified: offsets[j] is the serial walk's
    bool ok = true;
    for (uint32_t f = j; f < n_frames; ++f) {
        const uint64_t prop_next = offsets[f + 1];
        uint64_t next;
        if (ok && fo == prop && flags[f]) next = prop_next;                // true start, verified frame: its end is the walk's
        else {
            uint64_t bits = ~0ull;
            if (ok && fo < terse_bytes)
                bits = walk_frame<false>(reinterpret_cast<const uint32_t*>(terse), (terse_bytes + 3) / 4, 8 * fo,
                                         8 * (terse_bytes - fo), g, max_w, nullptr, nullptr);
            if (bits == ~0ull) { ok = false; bits = 0; }
            next = ok ? fo + 1 + bits / 8 : fo;
        }
        if (lane_id() == 0) offsets[f + 1] = next;
        prop = prop_next;
        fo = next;
    }
    if (lane_id() == 0 && !ok) atomicMax(&status[0], kStatusCorrupt);
}

// trpx_decode(frame_offsets = NULL) on located offsets: the decode clears the status block, so the locate's verdict is re-read
// from the offsets behind it -- every frame the serial walk accepts is at least one byte, and after a failure it adds none
__global__ __launch_bounds__(kWave) void k_loc_status(const uint64_t* __restrict__ offsets, uint32_t n_frames,
                                                      uint32_t* __restrict__ status) {
    if (threadIdx.x == 0 && offsets[n_frames] == offsets[n_frames - 1]) atomicMax(&status[0], kStatusCorrupt);
}

bool parallel_ok(const FrameGeom& g, uint64_t terse_bytes, uint64_t n_frames, uint32_t max_w) {
    return g.block == 12u && max_w <= 32u && n_frames >= kLocMinFrames && terse_bytes >= kLocMinBytes &&
           8 * terse_bytes < (1ull << 50);
}

}  // namespace

// 0 = auto, 1 = serial.  Initialised from $TRPX_LOCATE_PATH ("serial"), changed by trpx_set_locate_path().
int g_locate_path = [] {
    const char* e = getenv("TRPX_LOCATE_PATH");
    return e && strcmp(e, "serial") == 0 ? 1 : 0;
}();

size_t locate_workspace_bytes(const FrameGeom& g, uint64_t terse_bytes, uint64_t n_frames) {
    return g.block == 12u ? loc_layout(terse_bytes, n_frames).total : 256;
}

bool locate_parallel(const FrameGeom& g, uint64_t terse_bytes, uint64_t n_frames, uint32_t max_w) {
    return g_locate_path == 0 && parallel_ok(g, terse_bytes, n_frames, max_w);
}

hipError_t launch_locate(const uint8_t* terse, uint64_t terse_bytes, const FrameGeom& g, uint32_t n_frames, uint32_t max_w,
                         uint64_t* offsets, uint32_t* status, void* workspace, hipStream_t st, bool clear_status) {
    if (clear_status) zero_status(status, st);
    if (!locate_parallel(g, terse_bytes, n_frames, max_w)) {
        hipLaunchKernelGGL(k_locate_serial, dim3(1), dim3(kWave), 0, st, terse, terse_bytes, n_frames, g, max_w, offsets, status);
        return hipGetLastError();
    }
    const LocLayout l = loc_layout(terse_bytes, n_frames);
    char* ws = static_cast<char*>(workspace);
    uint32_t* first_bad = reinterpret_cast<uint32_t*>(ws);
    uint8_t* flags = reinterpret_cast<uint8_t*>(ws + l.flags);
    uint64_t* cp = reinterpret_cast<uint64_t*>(ws + l.cp);
    uint64_t* ext = reinterpret_cast<uint64_t*>(ws + l.ext);
    uint64_t* chunks = reinterpret_cast<uint64_t*>(ws + l.chunks);
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(terse);
    const uint64_t n_dw = (terse_bytes + 3) / 4;
    hipLaunchKernelGGL(k_loc_chunks, dim3((uint32_t)l.n_chunks), dim3(kWave), 0, st, s32, n_dw, l.n_win, max_w, cp, chunks, first_bad);
    hipLaunchKernelGGL(k_loc_links, dim3((uint32_t)l.n_chunks), dim3(kWave), 0, st, s32, n_dw, l.n_win, max_w,
                       static_cast<const uint64_t*>(cp), ext, chunks);
    hipLaunchKernelGGL(k_loc_chase, dim3(1), dim3(kWave), 0, st, s32, n_dw, terse_bytes, l.n_win, n_frames, g, max_w,
                       static_cast<const uint64_t*>(cp), static_cast<const uint64_t*>(ext), static_cast<const uint64_t*>(chunks), offsets);
    hipLaunchKernelGGL(k_loc_verify, dim3(n_frames), dim3(kWave), 0, st, terse, terse_bytes, g, max_w,
                       static_cast<const uint64_t*>(offsets), flags, first_bad);
    hipLaunchKernelGGL(k_loc_repair, dim3(1), dim3(kWave), 0, st, terse, terse_bytes, n_frames, g, max_w, offsets,
                       static_cast<const uint8_t*>(flags), static_cast<const uint32_t*>(first_bad), status);
    return hipGetLastError();
}

hipError_t launch_locate_status(const uint64_t* offsets, uint32_t n_frames, uint32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(k_loc_status, dim3(1), dim3(kWave), 0, st, offsets, n_frames, status);
    return hipGetLastError();
}

}  // namespace trpx
