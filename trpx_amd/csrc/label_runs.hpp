// What trpx_decode_sum_labelled decides about runs, once.  The frames with an output stand in the order of their labels
// (starts[l] .. starts[l + 1] are the positions of label l, starts[n_out] = n_kept), and that order is cut at fixed positions into
// chunks of fpc positions: chunk c is [c * fpc, min((c + 1) * fpc, n_kept)).  A RUN is what a chunk holds of one label.
//   direct   a label whose positions all lie inside one chunk: its run is the whole sum, converted and stored by the walk
//   partial  a label that crosses a cut leaves its runs' raw accumulators in the slab [n_chunks][2][stride]: slot 0 for the run
//            that contains the chunk's first position, slot 1 for the other one (a chunk has at most one of each: a run that
//            neither begins the chunk nor ends it is a whole label)
//   merge    a label without positions is 0; one inside a single chunk is already written; one over chunks cf .. cl adds its
//            partials in chunk order -- slot 1 in cf where it does not begin the chunk, slot 0 everywhere else
// Everything follows from starts and fpc alone.  __host__ __device__: the kernels (decode_sum_labelled.hip) and the CPU sanitizer
// program (tests/cpp/sum_labelled_sanitize.cpp) compile this text.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef TRPX_HD
#if defined(__HIPCC__)
#define TRPX_HD __host__ __device__
#else
#define TRPX_HD
#endif
#endif

namespace trpx {

constexpr uint64_t kLabelledMaxOut = 1ull << 20;           // outputs per call (include/trpx_hip.h)
constexpr uint64_t kLabelledTargetChunks = 1024;           // = kSumTargetUnits (decode_sum.hpp): about four workgroups per CU

// Short stacks with few outputs are ordered by one workgroup in LDS (k_lab_order_small), the others by four launches.
constexpr uint32_t kLabelledSmallFrames = 4096, kLabelledSmallOut = 8192;
TRPX_HD inline bool labelled_order_small(uint64_t n_frames, uint64_t n_out) {
    return n_frames <= kLabelledSmallFrames && n_out <= kLabelledSmallOut;
}

// The cut, from the sizes alone (tpf: tiles per frame, sum_plan's; narrow: 8/16-bit pixels, whose accumulators are 32 bits wide
// and exact for 65 535 frames).  Returns the frames per chunk, *n_chunks the chunks.  About kLabelledTargetChunks units (tile,
// chunk); for frames of more than one tile as many more chunks as still fit the last round of resident workgroups -- the units
// are long (a chunk of frames each), and 1032 of them on 768 places take two rounds of 20 frames where 1505 take two of 14
// (DESIGN.md 4.20).  Frames of one tile are too short for rounds to matter.
constexpr uint64_t kLabelledCUs = 256;                     // MI355X; k_sum_labelled: 3 workgroups a CU (8/16-bit pixels), 2 (32-bit)
TRPX_HD inline uint32_t label_frames_per_chunk(uint64_t n_frames, uint64_t tpf, bool narrow, uint32_t* n_chunks) {
    uint64_t chunks = (kLabelledTargetChunks + tpf - 1) / tpf;
    if (chunks < 1) chunks = 1;
    if (tpf > 1) {
        const uint64_t places = kLabelledCUs * (narrow ? 3 : 2), rounds = (chunks * tpf + places - 1) / places;
        chunks = rounds * places / tpf;                     // (>= the chunks it had: rounds * places >= chunks * tpf)
    }
    if (chunks > n_frames) chunks = n_frames;
    uint64_t fpc = (n_frames + chunks - 1) / chunks;
    if (narrow && fpc > 65535) fpc = 65535;
    if (n_chunks) *n_chunks = (uint32_t)((n_frames + fpc - 1) / fpc);
    return (uint32_t)fpc;
}

// chunk c's positions [*p0, *p1) of the n_kept ordered ones (empty behind n_kept)
TRPX_HD inline void label_chunk_span(uint32_t c, uint32_t fpc, uint32_t n_kept, uint32_t* p0, uint32_t* p1) {
    const uint64_t a = (uint64_t)c * fpc, b = a + fpc;
    *p0 = a < n_kept ? (uint32_t)a : n_kept;
    *p1 = b < n_kept ? (uint32_t)b : n_kept;
}

// the label's positions [s, e), e > s: do they lie inside one chunk?  (then its one run is flushed directly)
TRPX_HD inline bool label_run_direct(uint32_t s, uint32_t e, uint32_t fpc) { return s / fpc == (e - 1) / fpc; }

// the slab slot of the run that a label beginning at position s leaves in the chunk that begins at p0 (the run is not direct)
TRPX_HD inline uint32_t label_run_slot(uint32_t s, uint32_t p0) { return s > p0 ? 1u : 0u; }

// element 0 of a run's accumulators in the slab (stride: elements per slot)
TRPX_HD inline uint64_t label_slab_at(uint32_t c, uint32_t slot, uint64_t stride) { return ((uint64_t)c * 2 + slot) * stride; }

// What the merge does with the label at [s, e): kLabelEmpty -- write 0; kLabelDirect -- nothing, the walk wrote it;
// kLabelMerged -- add the partials of chunks *cf .. *cl, each from label_run_slot(s, c * fpc).
enum : int { kLabelEmpty = 0, kLabelDirect = 1, kLabelMerged = 2 };
TRPX_HD inline int label_merge_plan(uint32_t s, uint32_t e, uint32_t fpc, uint32_t* cf, uint32_t* cl) {
    if (e <= s) return kLabelEmpty;
    *cf = s / fpc;
    *cl = (e - 1) / fpc;
    return *cf == *cl ? kLabelDirect : kLabelMerged;
}

}  // namespace trpx
