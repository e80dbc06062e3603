// Host-only arithmetic and checks of trpx_encode_sparse / trpx_encode_sparse_host (api.hip), free of HIP so that
// tests/cpp/encode_sparse_sanitize.cpp can drive them under ASan + UBSan on a CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace trpx {

// An upper bound on the stack from the event count alone.  Per frame: every block costs at least its 1-bit "same width" header,
// n_blocks bits.  On top of that only blocks with events and their right neighbours cost more: a block with events at most a
// 12-bit header and 12 values of bits(T) bits (11 + 12 bits(T) more than its 1 bit), and a block without events behind it an
// explicit width-0 header of 4 bits (3 more).  There are at most n_events blocks with events, so the stack's frames hold at most
// n_frames x n_blocks + n_events x (14 + 12 bits(T)) bits; a frame of b bits is 1 + b / 8 bytes (the pad byte, Terse.hpp:547),
// and the sum of the rounded-down quotients is at most the quotient of the sum.  Clamped to `worst` (n_frames x
// trpx_worst_case_bytes, < 2^63), rounded up to 16.
inline size_t sparse_bound_bytes(size_t elem_bytes, uint64_t n_blocks, uint64_t n_frames, uint64_t n_events, uint64_t worst) {
    const unsigned __int128 bits = (unsigned __int128)n_frames * n_blocks + (unsigned __int128)n_events * (14 + 12 * 8 * elem_bytes);
    const unsigned __int128 bytes = (unsigned __int128)n_frames + bits / 8;
    const uint64_t bound = bytes < worst ? (uint64_t)bytes : worst;
    return (size_t)((bound + 15) / 16 * 16);
}

// trpx_encode_sparse_host's device block of inputs, [row_offsets u64 x (n_frames + 1)] [positions u32 x n_events] [values x
// n_events], each part 16-byte aligned.  false: the lists are too long to stage (their bytes reach 2^62; no product wraps).
struct SparseStaging { size_t pos_at, val_at, total; };
inline bool sparse_staging(uint64_t n_frames, uint64_t n_events, size_t elem_bytes, SparseStaging* l) {
    const unsigned __int128 lim = (unsigned __int128)1 << 62;
    if ((unsigned __int128)n_events * (4 + elem_bytes) >= lim || (unsigned __int128)8 * ((unsigned __int128)n_frames + 1) >= lim) return false;
    l->pos_at = (size_t)((8 * (n_frames + 1) + 15) / 16 * 16);
    l->val_at = (size_t)((l->pos_at + 4 * n_events + 15) / 16 * 16);
    l->total = l->val_at + elem_bytes * (size_t)n_events;
    return true;
}

// The event lists of n_frames frames: nullptr when they are good, else what is wrong with them (*frame, *event: where).  Reads
// row_offsets[0 .. n_frames] and, only once every row is known to lie inside the lists, positions[0 .. n_events).
inline const char* bad_events(const uint64_t* row_offsets, const uint32_t* positions, uint64_t n_events, uint64_t n_values,
                              uint64_t n_frames, uint64_t* frame, uint64_t* event) {
    *frame = n_frames;
    *event = 0;
    if (row_offsets[n_frames] > n_events) return "row_offsets ends beyond the events";
    for (uint64_t f = 0; f < n_frames; ++f)
        if (row_offsets[f] > row_offsets[f + 1]) { *frame = f; return "row_offsets decreases"; }
    for (uint64_t f = 0; f < n_frames; ++f)                  // (every row now lies inside [0, n_events))
        for (uint64_t i = row_offsets[f]; i < row_offsets[f + 1]; ++i) {
            *frame = f;
            *event = i;
            if (positions[i] >= n_values) return "a position is not below n_values";
            if (i > row_offsets[f] && positions[i - 1] >= positions[i]) return "positions do not ascend strictly";
        }
    return nullptr;
}

}  // namespace trpx
