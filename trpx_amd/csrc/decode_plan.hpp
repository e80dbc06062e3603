// The decode side's routing.  Which launch sequence a call takes is decided here, once, from a PlanInput, and carried as a
// value (DecodeArgs::plan) that the launchers follow: none of them infers a route from the pointers it was given.  Pure
// functions of their argument -- no HIP call, no allocation, no getenv --, free of HIP so that tests/cpp/decode_plan_test.cpp
// can drive them on a CPU.  DESIGN.md 4.6 has the table: entry point and condition -> plan -> kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace trpx {

// The forced route, with the values trpx_set_decode_path documents.  A forced route is still subject to its preconditions
// (alignment, block = 12, frame size).  Selector 5 / "dense" is no route: it is kRouteAuto plus PlanInput::dense.
enum DecodeRoute {
    kRouteAuto = 0,
    kRouteBasic = 1,     // decode.hip
    kRouteTiled = 2,     // position-parallel walk + k_unpack_tiles
    kRouteFrames = 3,    // per-frame decoder for any number of frames
    kRouteParts = 4,     // large frames by round 4's parts route (two walks) instead of the index route
};
enum class Entry : uint8_t { kDecode, kConvert, kBuildIndex, kIndexed };   // trpx_decode / _decode_convert / build_index_impl / _decode_indexed

// Everything a routing decision depends on.  The counts in the last group come from the kernel files' host functions.
struct PlanInput {
    Entry    entry = Entry::kDecode;
    int      route = kRouteAuto;
    bool     dense = false;            // the frames a walker lists: the dense walk (decode_dense.hip) instead of the fix-point rounds
    size_t   elem_size = 2;            // of the output type; 8: the converting decoder's
    unsigned block = 12;
    uint64_t n_blocks = 0, n_frames = 0;
    uint64_t frame_bits = 0;           // of a worst-case frame: 8 * trpx_worst_case_bytes
    bool     have_offsets = true;
    bool     keep_status = false;      // kBuildIndex: an earlier step of the call left its verdict in the status block
    bool     check_index = true;       // kBuildIndex: the stream is not the encoder's own and the consumer does not compare
    bool     frames_misaligned = false;   // frame bytes % 128 != 0
    bool     out_misaligned = false;      // pixels_out % 128 != 0
    bool     indexed_scratch = true;   // kIndexed: the hand-over list's scratch can be had (the caller asks lazily, and plans again without)
    uint32_t parts_per_frame = 1, chain_parts_per_frame = 1;   // parts_per_frame() / chain_parts_per_frame()
    bool     seg_single_wave = true;   // seg_single_wave(): the listed frames are extracted per frame, not by tiles
    bool     locate_parallel = false;  // locate_parallel(): the position-parallel locator applies ...
    bool     locate_fits = false;      // ... and its scratch fits behind tile_off
    // compile-time switches of api.hip (A/B and diagnostic builds)
    int      chain_extract = -1;       // TRPX_CHAIN_EXTRACT_TILES: 1 = tiles, 0 = units, -1 = by type and size
    bool     indexed_large_tiles = false;   // (no build sets it; tests/cpp/decode_plan_test.cpp pins what it would route)
    bool     no_defer = false;         // TRPX_DIAGNOSTICS, $TRPX_NO_DEFER: the per-frame decoder keeps every frame
    bool     lds_walk = false;         // TRPX_DIAGNOSTICS, $TRPX_WALK = lds: every index by the one-wavefront-per-frame walk
};

enum class Walk : uint8_t {            // what writes a.widths / a.tile_off
    kNone,                             // nothing: the extraction walks itself
    kCallers,                          // nothing: the index is the caller's
    kSerial,                           // k_walk_serial, which finds the frames as well (no offsets)
    kHeaders,                          // k_walk, a wavefront per frame (decode.hip)
    kSeg,                              // the position-parallel walk (decode_seg.hip)
    kLds,                              // k_walk_lds (diagnostic builds)
    kFrames,                           // the per-frame decoder's walker, k_index_frames; listed frames: launch_seg_listed
    kChain,                            // large frames: one walk of many short parts (decode_part.hip); listed frames likewise
};
enum class Extract : uint8_t {
    kNone,                             // an index is all that is asked for
    kBasic,                            // k_unpack / k_unpack_g
    kConvert,                          // k_unpack_conv
    kTiled,                            // k_unpack_tiles
    kFrames,                           // k_decode_frames, walking: one workgroup per frame
    kParts,                            // round 4: launch_build_parts, k_decode_parts
    kChainTiles, kChainUnits,          // behind Walk::kChain: k_unpack_tiles / k_decode_units_indexed (narrow: then k_decode_parts)
    kFramesIndexed,                    // k_decode_frames_indexed, or units of the frames where launch_decode_frames_indexed finds them cheaper
    kUnitsIndexed,                     // k_decode_units_indexed
};
struct DecodePlan {
    bool     locate = false;           // launch_locate in front (offsets into walk_offsets), launch_locate_status behind
    Walk     walk = Walk::kNone;
    Extract  extract = Extract::kNone;
    uint32_t parts_per_frame = 1;      // > 1: parts / part_ws are pointed
    bool     narrow = false;           // Walk::kChain: frames with few explicit headers get no index, k_decode_parts extracts them
    bool     misaligned = false;       // Extract::kFrames: some frame starts inside a cache line
    bool     defer = false;            // Extract::kFrames / kParts: the frames the walker lists are decoded behind it (launch_decode_deferred)
    bool     listed_tiles = false;     // ... by k_unpack_listed, not per frame
    bool     dense = false;            // launch_seg_listed: launch_dense_listed for frames of one part
    bool     check_index = false;      // k_check_index follows
    bool     clear_status = true;      // the route's first launch clears the status block (false: an earlier verdict stays)
};
// the scratch regions of a workspace or index block that a plan's launches use (Walk::kCallers: the block is the caller's index,
// read only -- the one list that route needs lies elsewhere)
enum : unsigned { kSeg = 1, kDefer = 2, kParts = 4 };
inline unsigned plan_scratch(const DecodePlan& p) {
    if (p.walk == Walk::kCallers) return 0u;
    const bool walker = p.walk == Walk::kFrames || p.walk == Walk::kChain;
    return (p.walk == Walk::kSeg || walker || p.defer ? kSeg : 0u) | (walker || p.defer ? kDefer : 0u) | (p.parts_per_frame > 1u ? kParts : 0u);
}

// frame-relative bit positions are kept in 32 bits (with head room for one step's overshoot)
inline bool frame_bits_fit_32(uint64_t frame_bits) { return frame_bits < 0xF0000000ull; }
// the per-frame decoder packs a block's bit position with its width into 32 bits: frames of < 2^26 bits less the walker's ring
// offset and one step's overshoot
inline bool fits_per_frame_decoder(uint64_t frame_bits) { return frame_bits + (1u << 17) < (1ull << 26); }

// Large frames (more than single_part_blocks(): 32 K blocks) are cut into parts.  They take the index route -- one walk of many
// short parts, decode_part.hip; a part's positions are relative to its own first bit, the frame's must fit 32 bits -- unless the
// tiled route is forced (it walks them position-parallel) or round 4's parts route is; the two routes cut differently.
// trpx_decode and trpx_build_index choose alike for the same stack: both ask here.
struct LargeFrames { bool by_index; uint32_t parts; bool split; };   // split: there are parts, and few enough for a grid
inline LargeFrames large_frames(const PlanInput& in, int route) {
    LargeFrames l;
    l.by_index = route != kRouteTiled && route != kRouteParts && frame_bits_fit_32(in.frame_bits);
    l.parts = l.by_index ? in.chain_parts_per_frame : in.parts_per_frame;
    l.split = l.parts > 1u && in.n_frames * (uint64_t)l.parts < 0x7FFFFFFFull;
    return l;
}
// trpx_decode_parts_per_frame's answer is the rule's part count, with two differences from what trpx_decode then uses: under
// kRouteTiled it reports the index route's parts although that route walks position-parallel, and a count too large for a grid
// is reported although the frames then stay whole.
inline uint32_t plan_parts_query(const PlanInput& in) { return large_frames(in, in.route == kRouteTiled ? kRouteAuto : in.route).parts; }

// trpx_decode and trpx_decode_convert
inline DecodePlan plan_stack(const PlanInput& in) {
    DecodePlan p;
    p.dense = in.dense;
    if (in.entry == Entry::kConvert || in.elem_size == 8) {                   // any output type, fields of up to 64 bits
        p.walk = in.have_offsets ? Walk::kHeaders : Walk::kSerial;
        p.extract = Extract::kConvert;
        return p;
    }
    const bool tuned = in.route != kRouteBasic && in.block == 12u && frame_bits_fit_32(in.frame_bits);
    // no offsets: the frames located by the position-parallel locator, then the routes a caller with offsets takes.  Elsewhere
    // (the basic or serial route asked for, other sizes, scratch too small): the decode's own serial walk.
    p.locate = !in.have_offsets && tuned && in.locate_parallel && in.locate_fits;
    if (!tuned || !(in.have_offsets || p.locate)) {
        p.walk = in.have_offsets ? Walk::kHeaders : Walk::kSerial;
        p.extract = Extract::kBasic;
        return p;
    }
    const LargeFrames l = large_frames(in, in.route);
    const bool parts = l.split && !in.no_defer;                               // (every route over parts lists frames)
    p.parts_per_frame = parts ? l.parts : 1u;
    // Frames that fit the per-frame decoder: one workgroup per frame, the walk and the extraction overlap inside it -- whatever
    // the number of frames (since the round-3 walker a single 512^2 frame takes 0.10 ms this way against 0.24 ms through the
    // position-parallel walk + tiled extraction, eight 1024^2 frames 0.37 against 0.73 ms).  Larger frames in parts; what is
    // neither, or the tiled route forced: the tiled kernels.
    const bool whole = fits_per_frame_decoder(in.frame_bits) && in.parts_per_frame == 1u;
    if (in.route == kRouteTiled || !(parts || whole)) {
        p.walk = in.lds_walk ? Walk::kLds : Walk::kSeg;
        p.extract = Extract::kTiled;
        return p;
    }
    p.defer = !in.no_defer;
    p.listed_tiles = !in.seg_single_wave;
    if (parts && l.by_index) {
        // (the tiled kernel, or units of the per-frame decoder with the widths given: eight 4096^2 int32 frames 0.406 / 0.444 ms,
        // 200 x (1030 x 1065) u16 0.246 / 0.268, 128 x 2048^2 u16 0.594 / 0.554 -- make chainextract)
        const bool tiles = in.chain_extract >= 0 ? in.chain_extract != 0 : in.elem_size == 4 || in.n_blocks < (1u << 18);
        p.walk = Walk::kChain;
        p.extract = tiles ? Extract::kChainTiles : Extract::kChainUnits;
        p.narrow = in.elem_size < 4;
    } else if (parts)
        p.extract = Extract::kParts;
    else {
        p.extract = Extract::kFrames;
        p.misaligned = in.frames_misaligned || in.out_misaligned;
    }
    return p;
}

// build_index_impl: trpx_build_index, the two-pass encoder's index, and the index consumers without one (sum / roi / sparse)
inline DecodePlan plan_index(const PlanInput& in) {
    DecodePlan p;
    p.dense = in.dense;
    p.check_index = in.check_index;
    p.clear_status = !in.keep_status;
    const LargeFrames l = large_frames(in, in.route);
    if (in.lds_walk) p.walk = Walk::kLds;
    else if (l.by_index && l.split) {                                        // every frame through k_chain_index: not narrow
        p.walk = Walk::kChain;
        p.parts_per_frame = l.parts;
    } else if (fits_per_frame_decoder(in.frame_bits) && in.route != kRouteTiled)   // (the conditions of trpx_decode's per-frame route)
        p.walk = Walk::kFrames;
    else
        p.walk = Walk::kSeg;
    return p;
}

// trpx_decode_indexed
inline DecodePlan plan_indexed(const PlanInput& in) {
    DecodePlan p;
    p.dense = in.dense;
    p.walk = Walk::kCallers;
    // a thousand frames and more: one workgroup per frame; fewer: the tiled kernel spreads a frame's tiles over the whole GPU
    // (512^2 u16 frames, tiled / per-frame: 128 frames 0.023 / 0.121 ms, 600 frames 0.092 / 0.137, 1000 frames 0.148 / 0.142, 2000
    // frames 0.30 / 0.21 -- both scale with the blocks per frame, so the frame count alone decides)
    const bool per_frame = fits_per_frame_decoder(in.frame_bits) && in.route != kRouteTiled && (in.route == kRouteFrames || in.n_frames >= 1024);
    // Frames that start inside a cache line (513 x 511 u16: most detectors): the indexed extraction's 16-byte stores are then
    // misaligned and it LOSES to the walking decoder, whose extraction waves write line images (2000 frames: 0.33 against 0.27 ms).
    // Such stacks take the walking decoder, and the frames it hands over -- header-dense ones, where the walk is what costs --
    // are extracted with the caller's index instead of being walked position-parallel: never slower than trpx_decode.
    const bool misaligned = in.frames_misaligned || in.out_misaligned;
    const uint32_t max_w = 8u * (uint32_t)in.elem_size;
    if (per_frame && misaligned && in.route == kRouteAuto && in.parts_per_frame == 1u && in.indexed_scratch) {
        p.extract = Extract::kFrames;
        p.misaligned = true;
        p.defer = true;
        p.listed_tiles = !in.seg_single_wave;
    } else if (per_frame)
        p.extract = Extract::kFramesIndexed;
    else if (!in.indexed_large_tiles && in.elem_size < 4 && in.n_blocks >= (1u << 18) && 8 * in.n_blocks * (12u + 12u * max_w) < (1ull << 31))
        p.extract = Extract::kUnitsIndexed;      // large frames of 8/16-bit pixels: units of the per-frame decoder, as the index route extracts them
    else
        p.extract = Extract::kTiled;
    return p;
}

inline DecodePlan plan_decode(const PlanInput& in) {
    return in.entry == Entry::kBuildIndex ? plan_index(in) : in.entry == Entry::kIndexed ? plan_indexed(in) : plan_stack(in);
}

}  // namespace trpx
