// trpx_select_frames (select_frames.hip): the map from a byte of the selected stack to (list slot, byte of
// the source stack), and the copy of one 16-byte output line built on it.  Free of HIP: the kernel and
// tests/cpp/select_sanitize.cpp (ASan + UBSan on a CPU, over exact-size heap arrays) run this text.
//
// The selected stack is the concatenation of the listed frames' bytes (Terse.hpp:502-505: every frame starts byte aligned and
// does not depend on its neighbours).  out_offsets[0 .. n_select] are the cumulative sizes; slot i owns the output bytes
// [out_offsets[i], out_offsets[i + 1]), which are terse[frame_offsets[frames[i]] ...].  An output line is 16 aligned bytes:
//   interior   all 16 bytes belong to one slot: aligned dwords of the source, funnel-shifted by the source's byte residue, one
//              16-byte store
//   exact      the line holds a frame boundary, the end of the stack or its zero pad: byte by byte, stored dword by dword up to
//              align4(total) and no further
//   nothing    the line starts at or behind align4(total)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRPX_HD __host__ __device__
#else
#define TRPX_HD
#endif

namespace trpx {

constexpr uint32_t kSelLine = 16;                          // bytes of an output line
constexpr uint32_t kSelLinesPerLane = 4;                   // lines a lane takes per chunk
constexpr uint32_t kSelChunk = 64 * kSelLinesPerLane * kSelLine;   // bytes of `out` a wavefront owns at a time (4096)
constexpr uint32_t kSelInvalid = 1, kSelCorrupt = 5;       // TRPX_ERR_INVALID_ARG, TRPX_ERR_CORRUPT

TRPX_HD inline uint64_t sel_align4(uint64_t x) { return (x + 3) & ~(uint64_t)3; }

// The bytes of list entry f and its verdict: an entry outside the stack is kSelInvalid, offsets that decrease or end beyond the
// stream are kSelCorrupt; either counts as an empty frame, so that no byte of the output maps to it.
TRPX_HD inline uint64_t select_size(uint32_t f, const uint64_t* frame_offsets, uint64_t n_frames, uint64_t terse_bytes, uint32_t* code) {
    *code = 0;
    if (f >= n_frames) { *code = kSelInvalid; return 0; }
    const uint64_t a = frame_offsets[f], b = frame_offsets[f + 1];
    if (a > b || b > terse_bytes) { *code = kSelCorrupt; return 0; }
    return b - a;
}

// The whole list, as trpx_select_frames_host checks it before a device is looked for: 0 with *total = the selected bytes, or the
// verdict of the first bad entry (*slot: which).  Reads frames[0 .. n_select) and the two offsets of entries inside the stack.
TRPX_HD inline uint32_t select_check_list(const uint32_t* frames, uint64_t n_select, const uint64_t* frame_offsets, uint64_t n_frames,
                                          uint64_t terse_bytes, uint64_t* slot, uint64_t* total) {
    *total = 0;
    for (uint64_t i = 0; i < n_select; ++i) {
        uint32_t code;
        *total += select_size(frames[i], frame_offsets, n_frames, terse_bytes, &code);
        if (code) { *slot = i; return code; }
    }
    return 0;
}

// the capacity edge (trpx_encode's rule): stores are dword granular, so align4(total) has to fit
TRPX_HD inline bool select_fits(uint64_t total, uint64_t out_capacity) { return sel_align4(total) <= out_capacity; }

// The slot that owns output byte pos, searched in [lo, hi]: the LAST i with out_offsets[i] <= pos (empty frames share an
// offset with their successor and own nothing).  Needs out_offsets[lo] <= pos < out_offsets[hi + 1].
TRPX_HD inline uint32_t select_slot(const uint64_t* out_offsets, uint32_t lo, uint32_t hi, uint64_t pos) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (out_offsets[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A chunk's slots: lo owns its first byte c0 (< total); hi == lo where the whole chunk lies inside that frame, else the last
// slot of the list (the lines of such a chunk search for themselves, inside [lo, hi]).
struct SelChunkSlots { uint32_t lo, hi; };
TRPX_HD inline SelChunkSlots select_chunk(const uint64_t* out_offsets, uint32_t n_select, uint64_t c0) {
    SelChunkSlots c;
    c.lo = select_slot(out_offsets, 0, n_select - 1, c0);
    c.hi = c0 + kSelChunk <= out_offsets[c.lo + 1] ? c.lo : n_select - 1;
    return c;
}

// A slot as the copy needs it: its output bytes [begin, end) and the source byte of `begin`.
struct SelSlot { uint64_t begin, end, src; };
TRPX_HD inline SelSlot select_slot_at(const uint64_t* out_offsets, const uint32_t* frames, const uint64_t* frame_offsets, uint32_t slot) {
    SelSlot s;
    s.begin = out_offsets[slot];
    s.end = out_offsets[slot + 1];
    s.src = s.end > s.begin ? frame_offsets[frames[slot]] : 0;   // (an empty slot -- a bad entry among them -- has no source)
    return s;
}

struct alignas(16) SelLine16 { uint32_t x, y, z, w; };

// 16 bytes from source byte src on, read as the aligned dwords that hold them (five where src % 4 != 0: the fifth holds byte
// src + 15, so nothing behind the dword of the last byte copied is read) and funnel-shifted by the residue.  Little endian.
TRPX_HD inline uint32_t sel_funnel(uint32_t lo, uint32_t hi, uint32_t r) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> r); }   // r < 32
TRPX_HD inline SelLine16 select_funnel16(const uint32_t* src32, uint64_t src) {
    const uint32_t* p = src32 + (src >> 2);
    const uint32_t r = 8u * (uint32_t)(src & 3u);
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = r ? p[4] : 0u;
    return SelLine16{sel_funnel(w0, w1, r), sel_funnel(w1, w2, r), sel_funnel(w2, w3, r), sel_funnel(w3, w4, r)};
}
TRPX_HD inline void select_store16(uint8_t* out, uint64_t L, const SelLine16& v) { *reinterpret_cast<SelLine16*>(out + L) = v; }

// A chunk that lies inside slot s as a whole (its first byte does): every line of it is interior, and the kernel takes them
// together -- all loads, then all stores.
TRPX_HD inline bool select_chunk_whole(const SelSlot& s, uint64_t c0) { return c0 + kSelChunk <= s.end; }
TRPX_HD inline SelLine16 select_line_whole(const uint8_t* terse, const SelSlot& s, uint64_t L) {
    return select_funnel16(reinterpret_cast<const uint32_t*>(terse), s.src + (L - s.begin));
}

// Output byte b (>= the begin of `slot`, which moves forward to b's owner): the source byte, 0 in the pad behind `total`.
TRPX_HD inline uint8_t select_byte(const uint8_t* terse, const uint64_t* out_offsets, const uint32_t* frames, const uint64_t* frame_offsets,
                                   uint32_t* slot, uint64_t b, uint64_t total) {
    if (b >= total) return 0;
    while (out_offsets[*slot + 1] <= b) ++*slot;            // (b < total = out_offsets[n_select]: the walk ends inside the list)
    return terse[frame_offsets[frames[*slot]] + (b - out_offsets[*slot])];
}

// The exact path of the line at L (< align4(total)), whose first byte -- if it has one below total -- belongs to `slot` or a
// later one: every dword that starts below align4(total) is stored whole, the others are not touched.
TRPX_HD inline void select_line_exact(const uint8_t* terse, const uint64_t* out_offsets, const uint32_t* frames, const uint64_t* frame_offsets,
                                      uint32_t slot, uint64_t L, uint64_t total, uint8_t* out) {
    const uint64_t end = sel_align4(total);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < kSelLine; ++k)
        w[k / 4] |= (uint32_t)select_byte(terse, out_offsets, frames, frame_offsets, &slot, L + k, total) << (8u * (k % 4));
    if (L + kSelLine <= end) {
        select_store16(out, L, SelLine16{w[0], w[1], w[2], w[3]});
        return;
    }
    for (uint32_t k = 0; k < 4; ++k)
        if (L + 4 * k < end) *reinterpret_cast<uint32_t*>(out + L + 4 * k) = w[k];
}

// The line at L (16-aligned) with its slot known (s: the owner of byte L; only read where L < total).
TRPX_HD inline void select_line_in(const uint8_t* terse, const uint64_t* out_offsets, const uint32_t* frames, const uint64_t* frame_offsets,
                                   uint32_t slot, const SelSlot& s, uint64_t L, uint64_t total, uint8_t* out) {
    if (L >= sel_align4(total)) return;
    if (L < total && L + kSelLine <= s.end)
        select_store16(out, L, select_line_whole(terse, s, L));
    else
        select_line_exact(terse, out_offsets, frames, frame_offsets, slot, L, total, out);
}

// The line at L of a chunk whose slots are c: what the kernel runs per lane and line, and the CPU model per line.
TRPX_HD inline void select_line(const uint8_t* terse, const uint64_t* out_offsets, const uint32_t* frames, const uint64_t* frame_offsets,
                                const SelChunkSlots& c, uint64_t L, uint64_t total, uint8_t* out) {
    if (L >= sel_align4(total)) return;
    const uint32_t slot = L < total ? select_slot(out_offsets, c.lo, c.hi, L) : c.hi;
    select_line_in(terse, out_offsets, frames, frame_offsets, slot, select_slot_at(out_offsets, frames, frame_offsets, slot), L, total, out);
}

}  // namespace trpx
