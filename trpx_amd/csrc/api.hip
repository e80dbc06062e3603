// C ABI of libtrpx_hip.so (declared in include/trpx_hip.h).  Thin: argument checks, workspace
// carving, kernel launches on the caller's stream.  No CPU codec lives here: without a gfx950
// device every compute entry point fails with TRPX_ERR_NO_DEVICE / TRPX_ERR_HIP.
// Layout: predicates and routes, the one argument prologue, workspace layouts, the device-pointer ABI, the consumers of a decode
// index behind their shared front (consumer_front), then the host staging helpers (Arena, enter, stage, finish, ...) and the
// host-pointer wrappers built from them; those of the index consumers all go through one staged call (consumer_host), which lays
// their inputs and outputs out as pieces of one device block.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "../../include/trpx_hip.h"
#include "decode_roi.hpp"
#include "decode_sparse.hpp"
#include "decode_dot.hpp"
#include "decode_bins.hpp"
#include "decode_hist.hpp"
#include "decode_corrected.hpp"
#include "decode_binned.hpp"
#include "decode_sum.hpp"
#include "decode_reduce.hpp"
#include "decode_sum_labelled.hpp"
#include "group_runs.hpp"
#include "launchers.hpp"
#include "profile.hpp"
#include "select_map.hpp"
#include "sparse_events.hpp"

namespace trpx {
Profiler& profiler() {
    static thread_local Profiler p;
    return p;
}
}  // namespace trpx

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(TRPX_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr unsigned kMaxBlock = 4096;           // generic kernels: tile bit counts stay well inside 32 bits
constexpr unsigned kBlock = trpx::kBlock;      // the tuned kernels' block size (Terse.hpp:264), the only one with a decode index

bool is64(int dtype) { return dtype == TRPX_U64 || dtype == TRPX_I64; }
// element size of a converting decode's output: the integer containers and float / double
size_t convert_elem_size(int out_dtype) { return out_dtype == TRPX_F32 ? 4 : out_dtype == TRPX_F64 ? 8 : trpx_dtype_size(out_dtype); }
// the tuned decoders' types: an integer container of <= 32 bits with the stream's signedness (Terse.hpp:356-357)
bool tuned_type(int stream_signed, int out_dtype) {
    return trpx_dtype_size(out_dtype) && out_dtype <= TRPX_I32 && (stream_signed != 0) == (trpx_dtype_is_signed(out_dtype) != 0);
}
uint64_t worst_frame_bits(int dtype, size_t n_values, unsigned block) { return 8 * (uint64_t)trpx_worst_case_bytes(dtype, n_values, block); }
// what the index entry points refuse (the routes' own use of the limit: decode_plan.hpp)
bool frame_bits_fit_32(int dtype, size_t n_values, unsigned block) { return trpx::frame_bits_fit_32(worst_frame_bits(dtype, n_values, block)); }

bool geom_of(size_t n_values, unsigned block, trpx::FrameGeom* g) {
    if (n_values == 0 || block == 0 || block > kMaxBlock) return false;
    const uint64_t nb = (n_values + block - 1) / block;
    if (nb > 0xFFFFFFFFull) return false;
    g->n_values = n_values;
    g->n_blocks = (uint32_t)nb;
    g->n_tiles = (uint32_t)((nb + trpx::kTileBlocks - 1) / trpx::kTileBlocks);
    g->block = block;
    return true;
}

// One size check for every entry point (sizes may come straight from an untrusted .trpx header): frame count and
// tiles must fit the 31-bit grids, and n_values * n_frames * 8 (the widest element) must not wrap.
bool sizes_ok(const trpx::FrameGeom& g, size_t n_frames) {
    if (n_frames == 0 || n_frames > 0x7FFFFFFFull / g.n_tiles) return false;
    const unsigned __int128 bytes = (unsigned __int128)g.n_values * n_frames * 8;
    return bytes < ((unsigned __int128)1 << 62);
}
// What the device can be asked to launch: HIP refuses a grid of 2^32 threads or more (gridDim.x * blockDim.x), and the hot
// kernels start one workgroup of 256 threads per tile (encode.hip, decode.hip, decode_fast.hip) or one wavefront per frame
// (decode.hip, decode_seg.hip, decode_locate.hip) with no cap.  So a call takes at most 2^24 - 1 tiles in all
// (TRPX_MAX_TILES_PER_CALL, include/trpx_hip.h) -- 51 G values of frames of 512 x 512, but only 16.7 M frames of one tile
// each; beyond it every device entry point answers UNSUPPORTED before its first device call.  (n_frames <= the tiles.)
bool grid_ok(const trpx::FrameGeom& g, size_t n_frames) { return n_frames <= (size_t)TRPX_MAX_TILES_PER_CALL / g.n_tiles; }
int grid_refused(const char* fn, const trpx::FrameGeom& g, size_t n_frames) {
    return fail(TRPX_ERR_UNSUPPORTED, "%s: %zu frames of %u tiles: more than %u tiles in one call (split the stack)", fn, n_frames, g.n_tiles,
                (unsigned)TRPX_MAX_TILES_PER_CALL);
}
// the locator and the host wrappers: a geometry that cannot be had is laid to the block size unless that is the tuned one
int bad_geom(const char* fn, unsigned block) {
    return fail(block != kBlock ? TRPX_ERR_UNSUPPORTED : TRPX_ERR_INVALID_ARG, "%s: unsupported sizes/block (block=%u)", fn, block);
}

// ---- the argument prologue of the device-pointer entry points ---------------------------------------------------------------
// Every error is decided here, before the first device call, in one order: [unknown dtype] -> block size -> 64-bit container ->
// signedness (all UNSUPPORTED) -> dtype / sizes (INVALID_ARG) -> more tiles than one call takes (grid_ok, UNSUPPORTED; a stream of
// fewer bytes than frames stays INVALID_ARG) -> null ->
// misaligned pointers (both INVALID_ARG).  tests/test_abi_args.py pins
// the code and the prefix of each; trpx_locate_frames and trpx_decode_sum keep their own, different orders.
struct PtrReq { const void* p; size_t align; bool required = true; };
enum : unsigned {
    kDtypeFirst = 1,     // an unknown dtype is reported in front of the block size (otherwise with the sizes, behind it)
    kIndexOnly = 2,      // works on a decode index: block = kBlock, containers of <= 32 bits
    kSameSign = 4,       // the stream's signedness must be the container's
    kHasStream = 8,      // takes a stream: terse_bytes != 0
};
int check_args(const char* fn, unsigned rules, int dtype, size_t elem, int stream_signed, size_t terse_bytes, size_t n_values,
               size_t n_frames, unsigned block, std::initializer_list<PtrReq> ptrs, trpx::FrameGeom* g) {
    if ((rules & kDtypeFirst) && !elem) return fail(TRPX_ERR_INVALID_ARG, "%s: unknown dtype %d", fn, dtype);
    if (rules & kIndexOnly ? block != kBlock : block == 0 || block > kMaxBlock)
        return fail(TRPX_ERR_UNSUPPORTED, rules & kIndexOnly ? "%s: block=%u (the decode index needs %u)" : "%s: block=%u (supported: 1..%u; 12 is the tuned default, Terse.hpp:264)",
                    fn, block, rules & kIndexOnly ? kBlock : kMaxBlock);
    if ((rules & kIndexOnly) && is64(dtype)) return fail(TRPX_ERR_UNSUPPORTED, "%s: no decode index for 64-bit containers (generic kernels)", fn);
    if ((rules & kSameSign) && (stream_signed != 0) != (trpx_dtype_is_signed(dtype) != 0))
        return fail(TRPX_ERR_UNSUPPORTED, "%s: stream signed=%d into dtype %d: only same-signedness decode is defined by the reference (Terse.hpp:356-357)",
                    fn, stream_signed, dtype);
    if (!elem) return fail(TRPX_ERR_INVALID_ARG, "%s: unknown dtype %d", fn, dtype);
    if (!geom_of(n_values, block, g) || !sizes_ok(*g, n_frames) || ((rules & kHasStream) && !terse_bytes))
        return fail(TRPX_ERR_INVALID_ARG, "%s: bad sizes n_values=%zu n_frames=%zu", fn, n_values, n_frames);
    if (!grid_ok(*g, n_frames)) {
        if ((rules & kHasStream) && n_frames > terse_bytes)                     // no such stack: every frame is at least one byte (Terse.hpp:547)
            return fail(TRPX_ERR_INVALID_ARG, "%s: bad sizes n_values=%zu n_frames=%zu", fn, n_values, n_frames);
        return grid_refused(fn, *g, n_frames);
    }
    for (const PtrReq& q : ptrs)
        if (q.required && !q.p) return fail(TRPX_ERR_INVALID_ARG, "%s: null pointer", fn);
    for (const PtrReq& q : ptrs)
        if ((uintptr_t)q.p % q.align) return fail(TRPX_ERR_INVALID_ARG, "%s: misaligned pointer (%p needs %zu B)", fn, q.p, q.align);
    return TRPX_OK;
}

// ---- workspace layouts ------------------------------------------------------------------------------------------------------
struct EncWs { size_t frame_size, tile_off, tile_bits, fused, total; };
EncWs enc_ws(const trpx::FrameGeom& g, size_t n_frames) {
    EncWs w;
    const size_t tiles = n_frames * (size_t)g.n_tiles;
    w.frame_size = 0;
    w.tile_off = trpx::align_up(w.frame_size + 8 * n_frames, 16);
    w.tile_bits = trpx::align_up(w.tile_off + 8 * tiles, 16);
    w.fused = trpx::align_up(w.tile_bits + 4 * tiles, 256);          // descriptors of the single-pass encoder
    w.total = w.fused + trpx::fused_workspace_bytes(g, n_frames);
    return w;
}

// The decode index and the decode workspace are one carve: [front] [tile_off] [widths] | [seg] [defer] [parts] [part_ws].
// An index has no front and its tile_off is its group offsets; what lies behind the bar is scratch of the walk that
// writes it.  A workspace starts with the serial walk's frame offsets (walk_offsets, at 0) and leaves room for round 4's
// parts route as well, which shares `parts` / `part_ws` with the index route (many short parts).  The index a caller
// builds and the one trpx_decode builds in its workspace agree on everything behind tile_off.
struct DecLayout { size_t tile_off, widths, seg, defer, parts, part_ws, total; };
DecLayout dec_layout(const trpx::FrameGeom& g, size_t n_frames, size_t pixel_bytes, size_t front, bool parts_route) {
    DecLayout l;
    l.tile_off = trpx::align_up(front, 16);
    l.widths = trpx::align_up(l.tile_off + 8 * n_frames * (size_t)g.n_tiles, 16);
    l.seg = trpx::align_up(l.widths + n_frames * (size_t)g.n_blocks, 256);    // scratch of the position-parallel walk
    l.defer = l.seg + trpx::seg_workspace_bytes(g, n_frames);                  // list of the frames the per-frame walker hands over
    l.parts = l.defer + trpx::defer_bytes(n_frames);                           // large frames: the part table and its scratch (decode_part.hip)
    size_t P = trpx::chain_parts_per_frame(g, n_frames, pixel_bytes), scratch = trpx::chain_workspace_bytes(g, n_frames, pixel_bytes);
    if (parts_route) {
        P = std::max<size_t>(P, trpx::parts_per_frame(g, n_frames));
        scratch = std::max(scratch, trpx::part_workspace_bytes(g, n_frames));
    }
    l.part_ws = l.parts + (P > 1 ? trpx::align_up(sizeof(trpx::PartDesc) * n_frames * P, 256) : 0);
    l.total = l.part_ws + scratch;
    return l;
}
// (pixel_bytes: only the scratch behind the index proper depends on it)
DecLayout idx_layout(const trpx::FrameGeom& g, size_t n_frames, size_t pixel_bytes = 4) { return dec_layout(g, n_frames, pixel_bytes, 0, false); }
DecLayout dec_ws(const trpx::FrameGeom& g, size_t n_frames, size_t pixel_bytes) { return dec_layout(g, n_frames, pixel_bytes, 8 * (n_frames + 1), true); }

trpx::DecodeArgs decode_args(const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const trpx::FrameGeom& g,
                             size_t n_frames, void* pixels_out, uint32_t* status) {
    trpx::DecodeArgs a{};
    a.terse = terse;
    a.terse_bytes = terse_bytes;
    a.frame_offsets = frame_offsets;
    a.geom = g;
    a.n_frames = (uint32_t)n_frames;
    a.pixels_out = pixels_out;
    a.status = status;
    return a;
}
// points a's index (always) and the scratch a.plan's launches use into an index or workspace block laid out as l: the one
// place that matches pointers to a plan
void point_into(trpx::DecodeArgs& a, const void* block, const DecLayout& l) {
    char* b = const_cast<char*>(static_cast<const char*>(block));
    const unsigned scratch = trpx::plan_scratch(a.plan);
    a.tile_off = reinterpret_cast<uint64_t*>(b + l.tile_off);
    a.widths = reinterpret_cast<uint8_t*>(b + l.widths);
    if (scratch & trpx::kSeg) a.seg_ws = b + l.seg;
    if (scratch & trpx::kDefer) a.defer = reinterpret_cast<uint32_t*>(b + l.defer + trpx::kDeferFront);
    if (scratch & trpx::kParts) {
        a.parts = reinterpret_cast<trpx::PartDesc*>(b + l.parts);
        a.part_ws = b + l.part_ws;
    }
}

// ---- routes -----------------------------------------------------------------------------------------------------------------
// 0 = auto (single-pass encoder), 1 = force the two-pass pipeline.
// Initialised from $TRPX_ENCODE_PATH ("twopass" / "fused"), changed by trpx_set_encode_path().
int g_encode_path = [] {
    const char* e = getenv("TRPX_ENCODE_PATH");
    return e && strcmp(e, "twopass") == 0 ? 1 : 0;
}();
// The decode route (trpx::DecodeRoute, decode_plan.hpp).  Initialised from $TRPX_DECODE_PATH ("basic" / "tiles" / "frames" /
// "parts" / "dense"), changed by trpx_set_decode_path().  Selector 5 / "dense" is kRouteAuto plus g_dense_listed.
using trpx::kRouteAuto;
constexpr int kSelectDense = 5;
bool g_dense_listed = false;
trpx::DecodeRoute g_decode_path = [] {
    using namespace trpx;
    const char* e = getenv("TRPX_DECODE_PATH");
    if (!e) return kRouteAuto;
    g_dense_listed = strcmp(e, "dense") == 0;
    return strcmp(e, "basic") == 0 ? kRouteBasic : (strcmp(e, "tiles") == 0 || strcmp(e, "seg") == 0) ? kRouteTiled
           : strcmp(e, "frames") == 0 ? kRouteFrames : strcmp(e, "parts") == 0 ? kRouteParts : kRouteAuto;
}();
// $TRPX_SINGLE_PART = "frames,blocks": stacks of that many frames and more keep frames of up to that many blocks on the per-frame
// route (launchers.hpp: single_part_blocks; tuning runs -- the built-in rule otherwise)
[[maybe_unused]] const int g_single_part_env = [] {
    const char* e = getenv("TRPX_SINGLE_PART");
    unsigned f = 0, b = 0;
    if (e && sscanf(e, "%u,%u", &f, &b) == 2) trpx::set_single_part_rule(f, b);
    return 0;
}();
// What a routing decision depends on (decode_plan.hpp), gathered from the call, the selectors above and the kernel files' host
// functions; the entry points add what only they know.  dtype: the one the worst-case frame is reckoned in.
trpx::PlanInput plan_input(trpx::Entry entry, int dtype, size_t es, const trpx::FrameGeom& g, size_t n_frames, bool have_offsets = true) {
    trpx::PlanInput in;
    in.entry = entry;
    in.route = g_decode_path;                                                  // trpx_set_decode_path / $TRPX_DECODE_PATH
    in.dense = g_dense_listed;
    in.elem_size = es;
    in.block = g.block;
    in.n_blocks = g.n_blocks;
    in.n_frames = n_frames;
    in.frame_bits = worst_frame_bits(dtype, g.n_values, g.block);
    in.have_offsets = have_offsets;
    in.parts_per_frame = trpx::parts_per_frame(g, n_frames);
    in.chain_parts_per_frame = trpx::chain_parts_per_frame(g, n_frames, es);
    in.seg_single_wave = trpx::seg_single_wave(g, n_frames);
#ifdef TRPX_CHAIN_EXTRACT_TILES
    in.chain_extract = TRPX_CHAIN_EXTRACT_TILES;                               // (make chainextract)
#endif
#ifdef TRPX_DIAGNOSTICS
    static const bool no_defer = getenv("TRPX_NO_DEFER") != nullptr;
    static const bool lds_walk = getenv("TRPX_WALK") && strcmp(getenv("TRPX_WALK"), "lds") == 0;
    in.no_defer = no_defer;
    in.lds_walk = lds_walk;
#endif
    return in;
}
void misalignment(trpx::PlanInput& in, const trpx::FrameGeom& g, const void* pixels_out) {
    in.frames_misaligned = (g.n_values * in.elem_size) % 128u != 0u;
    in.out_misaligned = (uintptr_t)pixels_out % 128u != 0u;
}
// the launcher of a plan with an extraction (the converting decoder's apart: it takes the stream's signedness)
hipError_t launch_planned(int dtype, const trpx::DecodeArgs& a, hipStream_t hs) {
    using trpx::Extract;
    switch (a.plan.extract) {
    case Extract::kBasic: return trpx::launch_decode(dtype, a, hs);
    case Extract::kTiled: case Extract::kFramesIndexed: case Extract::kUnitsIndexed: return trpx::launch_decode_fast(dtype, a, hs);
    case Extract::kFrames: case Extract::kParts: case Extract::kChainTiles: case Extract::kChainUnits: return trpx::launch_decode_frames(dtype, a, hs);
    default: return hipErrorInvalidValue;
    }
}

// trpx_decode_indexed's hand-over list (see there): per calling thread, one buffer per (device, stream), grow-only, freed with the thread.
struct IdxScratch {
    struct Slot { int dev; hipStream_t st; void* p; size_t bytes; };
    std::vector<Slot> slots;
    ~IdxScratch() { for (auto& s : slots) if (s.p) (void)hipFree(s.p); }
};
void* indexed_scratch(size_t bytes, hipStream_t st) {
    static thread_local IdxScratch t;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    // never under stream capture: a graph would keep the buffer's address, and a later, larger call frees it
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (cs != hipStreamCaptureStatusNone) return nullptr;
    for (auto& s : t.slots)
        if (s.dev == dev && s.st == st) {
            if (s.bytes >= bytes) return s.p;
            if (hipStreamSynchronize(st) != hipSuccess) return nullptr;        // (calls that still use the smaller buffer)
            (void)hipFree(s.p);
            s.p = nullptr; s.bytes = 0;
            if (hipMalloc(&s.p, bytes) != hipSuccess) { s.p = nullptr; (void)hipGetLastError(); return nullptr; }
            s.bytes = bytes;
            return s.p;
        }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    t.slots.push_back({dev, st, p, bytes});
    return p;
}

// check: compare the index with the stream's headers (k_check_index); false where the stream is the encoder's own, or the
// consumer makes the comparison itself
int build_index_impl(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                     size_t n_frames, unsigned block, void* index, uint32_t* status, bool clear_status, void* stream, bool check = true) {
    trpx::FrameGeom g;
    if (const int rc = check_args("trpx_build_index", kIndexOnly | kHasStream, dtype, trpx_dtype_size(dtype), 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {frame_offsets, 8}, {index, 16}, {status, 8}}, &g))
        return rc;
    if (!frame_bits_fit_32(dtype, n_values, block)) return fail(TRPX_ERR_UNSUPPORTED, "trpx_build_index: frames of >= 2^32 bits");
    trpx::PlanInput in = plan_input(trpx::Entry::kBuildIndex, dtype, trpx_dtype_size(dtype), g, n_frames);
    in.keep_status = !clear_status;
    in.check_index = check;
    trpx::DecodeArgs a = decode_args(terse, terse_bytes, frame_offsets, g, n_frames, nullptr, status);
    a.plan = trpx::plan_decode(in);
    point_into(a, index, idx_layout(g, n_frames, trpx_dtype_size(dtype)));
    HIP_TRY(trpx::launch_walk_only(a, (uint32_t)(8 * trpx_dtype_size(dtype)), a.plan.clear_status, static_cast<hipStream_t>(stream)));
    // an index is only good for a stream whose layout follows from its widths: a restated width (valid, written by no encoder
    // here) makes the index CORRUPT here, not pixels wrong in whatever consumes it
    if (a.plan.check_index) HIP_TRY(trpx::launch_check_index(a, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

// trpx_encode / trpx_encode_indexed; two_pass: the retry of the checked entry points after a look-back timeout
int encode_impl(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block, uint8_t* out, size_t out_capacity,
                uint64_t* frame_offsets, uint32_t* status, void* index, void* workspace, size_t workspace_bytes, void* stream,
                bool two_pass) {
    trpx::FrameGeom g;
    if (const int rc = check_args("trpx_encode", kDtypeFirst, dtype, trpx_dtype_size(dtype), 0, 0, n_values, n_frames, block,
                                  {{pixels, trpx_dtype_size(dtype)}, {frame_offsets, 8}, {status, 8}, {workspace, 8},
                                   {out, 16, out_capacity != 0}}, &g))   // (out: the kernels' 16-byte stores)
        return rc;
    const EncWs w = enc_ws(g, n_frames);
    if (workspace_bytes < w.total)
        return fail(TRPX_ERR_CAPACITY, "trpx_encode: workspace %zu < %zu", workspace_bytes, w.total);

    trpx::EncodeArgs a;
    a.pixels = pixels;
    a.geom = g;
    a.n_frames = (uint32_t)n_frames;
    a.out = out;
    a.out_capacity = out_capacity;
    a.frame_offsets = frame_offsets;
    a.status = status;
    char* ws = static_cast<char*>(workspace);
    a.frame_size = reinterpret_cast<uint64_t*>(ws + w.frame_size);
    a.tile_off = reinterpret_cast<uint64_t*>(ws + w.tile_off);
    a.tile_bits = reinterpret_cast<uint32_t*>(ws + w.tile_bits);
    if ((uintptr_t)index % 16) return fail(TRPX_ERR_INVALID_ARG, "trpx_encode_indexed: index must be 16-byte aligned");
    const DecLayout il = idx_layout(g, n_frames, trpx_dtype_size(dtype));
    a.idx_group_off = index ? reinterpret_cast<uint64_t*>(static_cast<char*>(index) + il.tile_off) : nullptr;
    a.idx_widths = index ? reinterpret_cast<uint8_t*>(static_cast<char*>(index) + il.widths) : nullptr;
    if (block != kBlock || is64(dtype)) {  // any other block size, 64-bit containers: generic (correct-first) kernels
        if (index) return fail(TRPX_ERR_UNSUPPORTED, "trpx_encode_indexed: the decode index needs block=12 and pixels of <= 32 bits");
        trpx::fused_ws_forget(workspace, workspace_bytes);
        HIP_TRY(trpx::launch_encode_generic(dtype, a, static_cast<hipStream_t>(stream)));
        return TRPX_OK;
    }
    // (frames need not be vector aligned -- most detectors' pixel counts are not multiples of 4: 1030 x 1065, 2463 x 2527 --: the
    // kernels' 16-byte accesses only need what the hardware needs, which in HSA's unaligned access mode is nothing)
    const bool vec_ok = (uint64_t)g.n_blocks * 396 < (1ull << 40);       // frame bits fit the fused encoder's 40-bit accumulator
    if (g_encode_path == 0 && !two_pass && vec_ok) {
        trpx::fused_ws_forget(workspace, workspace_bytes, ws + w.fused);   // (a clean descriptor block of another geometry in this memory is no longer)
        HIP_TRY(trpx::launch_encode_fused(dtype, a, ws + w.fused, static_cast<hipStream_t>(stream)));
    } else {
        trpx::fused_ws_forget(workspace, workspace_bytes);
        HIP_TRY(trpx::launch_encode(dtype, a, static_cast<hipStream_t>(stream)));
        if (index && out)   // the two-pass pipeline does not emit the index: build it from the stream it just wrote
            return build_index_impl(dtype, out, out_capacity, frame_offsets, n_values, n_frames, block, index, status, false, stream, false);
    }
    return TRPX_OK;
}

// copy on the caller's private stream and wait for that stream (never for the device)
hipError_t copy_sync(hipStream_t hs, void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    const hipError_t e = hipMemcpyAsync(dst, src, n, kind, hs);
    return e != hipSuccess ? e : hipStreamSynchronize(hs);
}
// the status block of the work queued on hs so far, on the host (waits for hs alone) ...
int read_status(hipStream_t hs, const uint32_t* d_status, uint32_t st[TRPX_STATUS_WORDS]) {
    HIP_TRY(copy_sync(hs, st, d_status, 4 * TRPX_STATUS_WORDS, hipMemcpyDeviceToHost));
    return TRPX_OK;
}
// ... and its verdict as a return code
int status_result(const char* fn, const uint32_t* st) {
    return st[0] ? fail((int)st[0], "%s: device status %u (5: corrupt or truncated stream)", fn, st[0]) : TRPX_OK;
}

// Encode and read the status back; after a look-back wait that gave up (TRPX_ERR_TIMEOUT: never seen in practice, keeps the API
// total) once more through the two-pass pipeline, which has no waits.  (With the two-pass pipeline forced by
// trpx_set_encode_path the first attempt has no waits either: its status is never TIMEOUT and there is no second one.)
int encode_retrying(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block, uint8_t* out, size_t out_capacity,
                    uint64_t* frame_offsets, uint32_t* status, void* index, void* workspace, size_t workspace_bytes, void* stream,
                    uint32_t st[TRPX_STATUS_WORDS]) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        int rc = encode_impl(dtype, pixels, n_values, n_frames, block, out, out_capacity, frame_offsets, status, index, workspace,
                             workspace_bytes, stream, attempt == 1);
        if (rc || (rc = read_status(static_cast<hipStream_t>(stream), status, st))) return rc;   // the caller's stream alone, not the device
        if (st[0] != TRPX_ERR_TIMEOUT) break;
    }
    return TRPX_OK;
}

}  // namespace

extern "C" {

int trpx_abi_version(void) { return TRPX_ABI_VERSION; }
const char* trpx_last_error_string(void) { return g_err; }

size_t trpx_dtype_size(int dtype) {
    switch (dtype) {
    case TRPX_U8: case TRPX_I8: return 1;
    case TRPX_U16: case TRPX_I16: return 2;
    case TRPX_U32: case TRPX_I32: return 4;
    case TRPX_U64: case TRPX_I64: return 8;
    }
    return 0;
}
int trpx_dtype_is_signed(int dtype) { return dtype >= 0 && dtype <= TRPX_I32 ? (dtype & 1) : (dtype == TRPX_I64 ? 1 : 0); }

int trpx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

size_t trpx_worst_case_bytes(int dtype, size_t n_values, unsigned block) {
    const size_t es = trpx_dtype_size(dtype);
    if (!es || !block) return 0;
    const size_t nblocks = (n_values + block - 1) / block;
    return n_values * es + (12 * nblocks + 7) / 8 + 1;
}

size_t trpx_encode_workspace_bytes(int dtype, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    if (!trpx_dtype_size(dtype) || !geom_of(n_values, block, &g)) return 0;
    return enc_ws(g, n_frames).total;
}
size_t trpx_decode_workspace_bytes(int dtype, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    if (!trpx_dtype_size(dtype) || !geom_of(n_values, block, &g)) return 0;
    return dec_ws(g, n_frames, trpx_dtype_size(dtype)).total;
}
size_t trpx_index_bytes(int dtype, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    if (!trpx_dtype_size(dtype) || !geom_of(n_values, block, &g)) return 0;
    return idx_layout(g, n_frames, trpx_dtype_size(dtype)).total;
}

unsigned trpx_decode_parts_per_frame(int dtype, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    if (!trpx_dtype_size(dtype) || is64(dtype) || block != kBlock || !geom_of(n_values, block, &g)) return 1;
    // (not always the count trpx_decode then uses: see plan_parts_query)
    return trpx::plan_parts_query(plan_input(trpx::Entry::kDecode, dtype, trpx_dtype_size(dtype), g, n_frames));
}

int trpx_encode(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block, uint8_t* out,
                size_t out_capacity, uint64_t* frame_offsets, uint32_t* status, void* workspace,
                size_t workspace_bytes, void* stream) {
    return encode_impl(dtype, pixels, n_values, n_frames, block, out, out_capacity, frame_offsets, status, nullptr, workspace,
                       workspace_bytes, stream, false);
}

int trpx_encode_indexed(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block, uint8_t* out,
                        size_t out_capacity, uint64_t* frame_offsets, uint32_t* status, void* index,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return encode_impl(dtype, pixels, n_values, n_frames, block, out, out_capacity, frame_offsets, status, index, workspace,
                       workspace_bytes, stream, false);
}

int trpx_encode_checked(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block, uint8_t* out,
                        size_t out_capacity, uint64_t* frame_offsets, uint32_t* status, void* index, void* workspace,
                        size_t workspace_bytes, void* stream, uint32_t* host_status) {
    uint32_t st[TRPX_STATUS_WORDS] = {0};
    if (const int rc = encode_retrying(dtype, pixels, n_values, n_frames, block, out, out_capacity, frame_offsets, status, index,
                                       workspace, workspace_bytes, stream, st))
        return rc;
    if (host_status) memcpy(host_status, st, sizeof st);
    return status_result("trpx_encode_checked", st);
}

int trpx_decode(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                const uint64_t* frame_offsets, size_t n_values, size_t n_frames, unsigned block, void* pixels_out,
                uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(out_dtype);
    if (!es) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode: unknown dtype %d", out_dtype);
    if (is64(out_dtype))                                   // 64-bit containers: the converting decoder (fields of up to 64 bits)
        return trpx_decode_convert(stream_signed, out_dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block, pixels_out,
                                   status, workspace, workspace_bytes, stream);
    if (const int rc = check_args("trpx_decode", kDtypeFirst | kSameSign | kHasStream, out_dtype, es, stream_signed, terse_bytes, n_values, n_frames,
                                  block, {{terse, 4}, {pixels_out, es}, {status, 8}, {workspace, 8}, {frame_offsets, 8, false}}, &g))
        return rc;
    const DecLayout w = dec_ws(g, n_frames, es);
    if (workspace_bytes < w.total)
        return fail(TRPX_ERR_CAPACITY, "trpx_decode: workspace %zu < %zu", workspace_bytes, w.total);

    hipStream_t hs = static_cast<hipStream_t>(stream);
    trpx::fused_ws_forget(workspace, workspace_bytes);      // (an encoder's clean descriptor words in this memory are about to be overwritten)
    trpx::PlanInput in = plan_input(trpx::Entry::kDecode, out_dtype, es, g, n_frames, frame_offsets != nullptr);
    misalignment(in, g, pixels_out);
    char* ws = static_cast<char*>(workspace);
    const uint32_t max_w = 8u * (uint32_t)es;
    if (!frame_offsets) {
        // the locator writes into walk_offsets, its scratch laid over the regions behind them (nothing the decode writes exists yet)
        in.locate_parallel = trpx::locate_parallel(g, terse_bytes, n_frames, max_w);
        in.locate_fits = w.total - w.tile_off >= trpx::locate_workspace_bytes(g, terse_bytes, n_frames);
    }
    trpx::DecodeArgs a = decode_args(terse, terse_bytes, frame_offsets, g, n_frames, pixels_out, status);
    a.plan = trpx::plan_decode(in);
    a.walk_offsets = reinterpret_cast<uint64_t*>(ws);
    point_into(a, ws, w);
    if (a.plan.locate) {
        HIP_TRY(trpx::launch_locate(terse, terse_bytes, g, (uint32_t)n_frames, max_w, a.walk_offsets, status, ws + w.tile_off, hs));
        a.frame_offsets = a.walk_offsets;
    }
    HIP_TRY(launch_planned(out_dtype, a, hs));
    if (a.plan.locate)                                                         // (the decode cleared the status: the locate's verdict again)
        HIP_TRY(trpx::launch_locate_status(a.walk_offsets, (uint32_t)n_frames, status, hs));
    return TRPX_OK;
}

int trpx_build_index(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                     size_t n_values, size_t n_frames, unsigned block, void* index, uint32_t* status, void* stream) {
    return build_index_impl(dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block, index, status, true, stream);
}

int trpx_decode_indexed(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                        const uint64_t* frame_offsets, const void* index, size_t n_values, size_t n_frames,
                        unsigned block, void* pixels_out, uint32_t* status, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(out_dtype);
    if (const int rc = check_args("trpx_decode_indexed", kDtypeFirst | kIndexOnly | kSameSign | kHasStream, out_dtype, es, stream_signed, terse_bytes,
                                  n_values, n_frames, block, {{terse, 4}, {index, 16}, {frame_offsets, 8}, {pixels_out, es}, {status, 8}}, &g))
        return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    trpx::PlanInput in = plan_input(trpx::Entry::kIndexed, out_dtype, es, g, n_frames);
    misalignment(in, g, pixels_out);
    trpx::DecodeArgs a = decode_args(terse, terse_bytes, frame_offsets, g, n_frames, pixels_out, status);
    a.plan = trpx::plan_decode(in);
    point_into(a, index, idx_layout(g, n_frames, es));
    if (a.plan.extract == trpx::Extract::kFrames) {
        // The walking decoder's hand-over list needs a few KB of scratch, which this entry point has no argument for: one grow-only
        // buffer per calling thread, device and stream (calls on one stream are ordered; a call that is being captured into a graph
        // takes the plain indexed route: a graph would keep the buffer's address, and a later, larger call frees it).
        void* scratch = indexed_scratch(trpx::defer_bytes(n_frames), hs);
        if (scratch) a.defer = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + trpx::kDeferFront);
        else {
            in.indexed_scratch = false;
            a.plan = trpx::plan_decode(in);
        }
    }
    HIP_TRY(launch_planned(out_dtype, a, hs));
    return TRPX_OK;
}

size_t trpx_group_count(size_t n_values, unsigned block) {
    trpx::FrameGeom g;
    if (block != kBlock || !geom_of(n_values, block, &g)) return 0;
    return g.n_tiles;
}

int trpx_index_group_states(const void* index, size_t n_values, size_t n_frames, unsigned block, uint64_t* states, void* stream) {
    trpx::FrameGeom g;
    if (const int rc = check_args("trpx_index_group_states", kIndexOnly, TRPX_U8, 1, 0, 0, n_values, n_frames, block, {{index, 16}, {states, 8}}, &g))
        return rc;
    trpx::DecodeArgs a = decode_args(nullptr, 0, nullptr, g, n_frames, nullptr, nullptr);
    point_into(a, index, idx_layout(g, n_frames));
    HIP_TRY(trpx::launch_index_group_states(a, states, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

int trpx_index_from_group_states(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                                 const uint64_t* states, size_t n_values, size_t n_frames, unsigned block, void* index,
                                 uint32_t* status, void* stream) {
    trpx::FrameGeom g;
    if (const int rc = check_args("trpx_index_from_group_states", kIndexOnly | kHasStream, dtype, trpx_dtype_size(dtype), 0, terse_bytes, n_values,
                                  n_frames, block, {{terse, 4}, {frame_offsets, 8}, {states, 8}, {index, 16}, {status, 8}}, &g))
        return rc;
    if (worst_frame_bits(dtype, n_values, block) >= (1ull << 40))              // (a group state keeps a bit offset in 40 bits)
        return fail(TRPX_ERR_UNSUPPORTED, "trpx_index_from_group_states: frames of >= 2^40 bits");
    trpx::DecodeArgs a = decode_args(terse, terse_bytes, frame_offsets, g, n_frames, nullptr, status);
    point_into(a, index, idx_layout(g, n_frames));
    HIP_TRY(trpx::launch_walk_groups(a, (uint32_t)(8 * trpx_dtype_size(dtype)), states, true, static_cast<hipStream_t>(stream)));
    HIP_TRY(trpx::launch_check_index(a, static_cast<hipStream_t>(stream)));         // (as trpx_build_index)
    return TRPX_OK;
}

int trpx_decode_convert(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                        const uint64_t* frame_offsets, size_t n_values, size_t n_frames, unsigned block, void* pixels_out,
                        uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = convert_elem_size(out_dtype);
    if (const int rc = check_args("trpx_decode_convert", kDtypeFirst | kHasStream, out_dtype, es, stream_signed, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {pixels_out, es}, {status, 8}, {workspace, 8}, {frame_offsets, 8, false}}, &g))
        return rc;
    const DecLayout w = dec_ws(g, n_frames, es);
    if (workspace_bytes < w.total) return fail(TRPX_ERR_CAPACITY, "trpx_decode_convert: workspace %zu < %zu", workspace_bytes, w.total);
    trpx::fused_ws_forget(workspace, workspace_bytes);
    trpx::DecodeArgs a = decode_args(terse, terse_bytes, frame_offsets, g, n_frames, pixels_out, status);
    a.plan = trpx::plan_decode(plan_input(trpx::Entry::kConvert, out_dtype, es, g, n_frames, frame_offsets != nullptr));
    a.walk_offsets = static_cast<uint64_t*>(workspace);
    point_into(a, workspace, w);
    HIP_TRY(trpx::launch_decode_convert(out_dtype, a, stream_signed != 0, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

int trpx_workspace_invalidate(const void* workspace, size_t workspace_bytes) {
    trpx::fused_ws_forget(workspace, workspace_bytes);
    return TRPX_OK;
}

int trpx_set_encode_path(int path) {
    if (path != 0 && path != 1) return fail(TRPX_ERR_INVALID_ARG, "trpx_set_encode_path: 0 = auto, 1 = two-pass");
    g_encode_path = path;
    return TRPX_OK;
}

int trpx_set_decode_path(int path) {
    if (path < kRouteAuto || path > kSelectDense) return fail(TRPX_ERR_INVALID_ARG, "trpx_set_decode_path: 0 = auto, 1 = basic, 2 = tiled, 3 = per-frame, 4 = parts route for large frames, 5 = auto with the dense walk for listed frames");
    g_dense_listed = path == kSelectDense;
    g_decode_path = path == kSelectDense ? kRouteAuto : static_cast<trpx::DecodeRoute>(path);
    return TRPX_OK;
}

int trpx_set_locate_path(int path) {
    if (path != 0 && path != 1) return fail(TRPX_ERR_INVALID_ARG, "trpx_set_locate_path: 0 = auto, 1 = serial");
    trpx::g_locate_path = path;
    return TRPX_OK;
}

int trpx_profile_enable(int on) {
    trpx::profiler().enabled = on != 0;
    return TRPX_OK;
}
int trpx_profile_read(float* stage_ms, int capacity) {
    if (!stage_ms || capacity <= 0) return 0;
    return trpx::profiler().read(stage_ms, capacity);
}

int trpx_synth_fill(int dtype, uint64_t seed, uint64_t frame0, size_t n_frames, size_t n_values, void* pixels_dev,
                    void* stream) {
    if (dtype != TRPX_U16 && dtype != TRPX_I32)
        return fail(TRPX_ERR_UNSUPPORTED, "trpx_synth_fill: synth-v1 is defined for U16 and I32");
    if (!pixels_dev) return fail(TRPX_ERR_INVALID_ARG, "trpx_synth_fill: null pointer");
    HIP_TRY(trpx::launch_synth(dtype, seed, frame0, n_frames, n_values, pixels_dev, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

size_t trpx_locate_workspace_bytes(size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    if (!terse_bytes || !geom_of(n_values, block, &g) || !sizes_ok(g, n_frames)) return 0;
    return trpx::locate_workspace_bytes(g, terse_bytes, n_frames);
}

// (its own order of checks: the pointers and max_bits first, and any block size the geometry can be had for)
int trpx_locate_frames(const uint8_t* terse, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block, unsigned max_bits,
                       uint64_t* frame_offsets, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    if (!terse || !terse_bytes || !frame_offsets || !status || !workspace || max_bits == 0 || max_bits > 64)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_locate_frames: bad argument");
    if (!geom_of(n_values, block, &g)) return bad_geom("trpx_locate_frames", block);
    if (!sizes_ok(g, n_frames) || n_frames > terse_bytes)                      // every frame is at least one byte (Terse.hpp:547)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_locate_frames: bad sizes n_values=%zu n_frames=%zu", n_values, n_frames);
    if (!grid_ok(g, n_frames)) return grid_refused("trpx_locate_frames", g, n_frames);
    if ((uintptr_t)terse % 4 || (uintptr_t)workspace % 8 || (uintptr_t)frame_offsets % 8 || (uintptr_t)status % 8)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_locate_frames: misaligned pointer (terse needs 4 B, workspace 8 B)");
    const size_t need = trpx::locate_workspace_bytes(g, terse_bytes, n_frames);
    if (workspace_bytes < need) return fail(TRPX_ERR_CAPACITY, "trpx_locate_frames: workspace %zu < %zu", workspace_bytes, need);
    trpx::fused_ws_forget(workspace, workspace_bytes);
    HIP_TRY(trpx::launch_locate(terse, terse_bytes, g, (uint32_t)n_frames, max_bits, frame_offsets, status, workspace,
                                static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

}  // extern "C"
// ---- the consumers of a decode index: trpx_decode_sum, trpx_decode_roi, trpx_decode_sparse, trpx_decode_dot, trpx_decode_bins, trpx_decode_binned, trpx_decode_reduce, trpx_decode_sum_labelled, trpx_decode_hist ----
// Each reads: its own checks, the shared checks (stack_limits, consumer_ws), the front (consumer_front), its own few fields, launch.
namespace {
// The consumers take three input forms: index given; offsets only -- the index is built by trpx_build_index's walk; neither --
// the frames are located first.  Their workspace starts with what the missing inputs need:
// [frame offsets (no offsets given)] [the locator's scratch, then the decode index (no index given)]; the consumer's own scratch
// follows at `total`, and `need` is the whole of it (consumer_ws).
struct IndexWs { size_t offsets, region, total, need; };
IndexWs index_ws(int dtype, const trpx::FrameGeom& g, size_t terse_bytes, size_t n_frames, bool have_offsets, bool have_index) {
    IndexWs w;
    w.offsets = 0;
    w.region = have_offsets ? 0 : trpx::align_up(8 * (n_frames + 1), 256);
    const size_t idx = have_index ? 0 : idx_layout(g, n_frames, trpx_dtype_size(dtype)).total;
    const size_t loc = have_offsets ? 0 : trpx::locate_workspace_bytes(g, terse_bytes, n_frames);
    w.need = w.total = w.region + trpx::align_up(std::max(idx, loc), 256);
    return w;
}
// what the *_workspace_bytes queries answer for: the front of the form without offsets and index, 0 for what no consumer takes
size_t consumer_front_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block, trpx::FrameGeom* g) {
    if (dtype < TRPX_U8 || dtype > TRPX_I32 || block != kBlock || !terse_bytes || !geom_of(n_values, block, g) || !sizes_ok(*g, n_frames))
        return 0;
    return index_ws(dtype, *g, terse_bytes, n_frames, false, false).total;
}
// a consumer's call, as the shared steps see it (g: from the entry point's own argument checks)
struct Consumer {
    const char* fn;
    int dtype;
    const uint8_t* terse;
    size_t terse_bytes;
    const uint64_t* frame_offsets;
    const void* index;
    size_t n_values, n_frames;
    unsigned block;
    trpx::FrameGeom g;
    uint32_t* status;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
};
int stack_limits(const Consumer& c) {
    if (!frame_bits_fit_32(c.dtype, c.n_values, c.block)) return fail(TRPX_ERR_UNSUPPORTED, "%s: frames of >= 2^32 bits", c.fn);
    if (c.n_frames > c.terse_bytes)                                             // every frame is at least one byte (Terse.hpp:547)
        return fail(TRPX_ERR_INVALID_ARG, "%s: bad sizes n_values=%zu n_frames=%zu", c.fn, c.n_values, c.n_frames);
    if (!grid_ok(c.g, c.n_frames)) return grid_refused(c.fn, c.g, c.n_frames);    // (trpx_decode_sum / _sum_labelled: not through check_args)
    return TRPX_OK;
}
// The workspace against what this form of the call needs: *w, then own_bytes of the consumer's.  always: why the consumer needs
// a workspace in every form (asked before the capacity), or null: only a form that needs one has to bring one.
int consumer_ws(const Consumer& c, size_t own_bytes, const char* always, IndexWs* w) {
    if (c.index && !c.frame_offsets) return fail(TRPX_ERR_INVALID_ARG, "%s: an index needs its frame offsets", c.fn);
    if (always && !c.workspace) return fail(TRPX_ERR_INVALID_ARG, "%s: null workspace (%s)", c.fn, always);
    *w = index_ws(c.dtype, c.g, c.terse_bytes, c.n_frames, c.frame_offsets != nullptr, c.index != nullptr);
    w->need = w->total + own_bytes;
    if (c.workspace_bytes < w->need) return fail(TRPX_ERR_CAPACITY, "%s: workspace %zu < %zu", c.fn, c.workspace_bytes, w->need);
    if (w->need && !c.workspace) return fail(TRPX_ERR_INVALID_ARG, "%s: null workspace", c.fn);
    return TRPX_OK;
}
// The front itself: a workspace that is used is forgotten as an encoder's, the offsets and the index are made valid, in the
// workspace where the caller gave none, and the stack is viewed through them.  clear: the consumer still has to clear the status block (false once the locator or the walk has written
// its verdict there); own: the consumer's scratch.  check_index: compare a walked index with the stream's headers
// (k_check_index; false where the consumer makes the comparison itself).
struct Front { trpx::IndexedStack stack; bool clear; char* own; };
int consumer_front(const Consumer& c, const IndexWs& w, bool check_index, Front* f) {
    char* ws = static_cast<char*>(c.workspace);
    const uint64_t* frame_offsets = c.frame_offsets;
    const char* index = static_cast<const char*>(c.index);
    if (w.need) trpx::fused_ws_forget(c.workspace, c.workspace_bytes);
    f->clear = true;
    f->own = ws + w.total;
    if (!frame_offsets) {                                                       // index-free: locate the frames first (its scratch: the index region)
        uint64_t* offs = reinterpret_cast<uint64_t*>(ws + w.offsets);
        HIP_TRY(trpx::launch_locate(c.terse, c.terse_bytes, c.g, (uint32_t)c.n_frames, 8u * (uint32_t)trpx_dtype_size(c.dtype), offs, c.status,
                                    ws + w.region, static_cast<hipStream_t>(c.stream)));
        frame_offsets = offs;
        f->clear = false;                                                       // (the locator's verdict stays)
    }
    if (!index) {                                                               // the walk of trpx_build_index, into the workspace
        if (const int rc = build_index_impl(c.dtype, c.terse, c.terse_bytes, frame_offsets, c.n_values, c.n_frames, c.block, ws + w.region,
                                            c.status, f->clear, c.stream, check_index))
            return rc;
        index = ws + w.region;
        f->clear = false;
    }
    const DecLayout il = idx_layout(c.g, c.n_frames, trpx_dtype_size(c.dtype));
    f->stack = {c.terse, c.terse_bytes, frame_offsets, c.g, c.n_frames, reinterpret_cast<const uint8_t*>(index + il.widths),
                reinterpret_cast<const uint64_t*>(index + il.tile_off)};
    return TRPX_OK;
}

// ---- summing decode (decode_sum.hip): its scratch is [partial slab] --------------------------------------------------------------
bool sum_out_ok(int out_dtype) {
    return out_dtype == TRPX_I32 || out_dtype == TRPX_U32 || out_dtype == TRPX_I64 || out_dtype == TRPX_U64 ||
           out_dtype == TRPX_F32 || out_dtype == TRPX_F64;
}
size_t sum_out_size(int out_dtype) { return out_dtype == TRPX_I32 || out_dtype == TRPX_U32 || out_dtype == TRPX_F32 ? 4 : 8; }
// What trpx_decode_sum and trpx_decode_sum_labelled check, in an order of their own, not check_args': a 64-bit dtype is UNSUPPORTED
// before an unknown one is INVALID_ARG (tests/test_decode_sum_args.py; tests/test_consumer_args_order.py pins every pair).  own:
// the refusal of the consumer's own count (group / n_out), asked where it stands in that order; more: its pointers besides
// terse, status and the sums, and words4 how the message names those of 4-byte alignment.  Fills c.g.
template <class Own>
int sum_checks(Consumer& c, int out_dtype, const void* sums_out, Own&& own, std::initializer_list<PtrReq> more, const char* words4) {
    if (is64(c.dtype)) return fail(TRPX_ERR_UNSUPPORTED, "%s: no decode index for 64-bit containers", c.fn);
    if (c.dtype < TRPX_U8 || c.dtype > TRPX_I32) return fail(TRPX_ERR_INVALID_ARG, "%s: unknown stream dtype %d", c.fn, c.dtype);
    if (!sum_out_ok(out_dtype)) return fail(TRPX_ERR_INVALID_ARG, "%s: out_dtype %d (I32, U32, I64, U64, F32, F64)", c.fn, out_dtype);
    if (c.block != kBlock) return fail(TRPX_ERR_UNSUPPORTED, "%s: block=%u (the decode index needs 12)", c.fn, c.block);
    if (trpx_dtype_is_signed(c.dtype) && (out_dtype == TRPX_U32 || out_dtype == TRPX_U64))
        return fail(TRPX_ERR_UNSUPPORTED, "%s: signed stream into an unsigned output (Terse.hpp:356-357)", c.fn);
    if (const int rc = own()) return rc;
    if (!geom_of(c.n_values, c.block, &c.g) || !sizes_ok(c.g, c.n_frames) || c.terse_bytes == 0 || c.n_frames > c.terse_bytes)
        return fail(TRPX_ERR_INVALID_ARG, "%s: bad sizes n_values=%zu n_frames=%zu", c.fn, c.n_values, c.n_frames);
    bool null = !c.terse || !sums_out || !c.status;
    bool askew = (uintptr_t)c.terse % 4 || (uintptr_t)c.frame_offsets % 8 || (uintptr_t)c.index % 16 || (uintptr_t)c.status % 8 ||
                 (uintptr_t)c.workspace % 8 || (uintptr_t)sums_out % sum_out_size(out_dtype);
    for (const PtrReq& q : more) {
        null = null || (q.required && !q.p);
        askew = askew || (uintptr_t)q.p % q.align;
    }
    if (null) return fail(TRPX_ERR_INVALID_ARG, "%s: null pointer", c.fn);
    if (c.index && !c.frame_offsets) return fail(TRPX_ERR_INVALID_ARG, "%s: an index needs its frame offsets", c.fn);
    if (askew)
        return fail(TRPX_ERR_INVALID_ARG, "%s: misaligned pointer (%s 4 B, offsets / workspace 8 B, index 16 B, sums their type)", c.fn, words4);
    return stack_limits(c);
}

// ---- box decode (decode_roi.hip): no scratch of its own ------------------------------------------------------------------------------
// the geometry checks the device-pointer and the host-pointer entry point share (sizes from the frame: < 2^29 values, see
// frame_bits_fit_32); 0 = fine
int roi_geometry(const char* fn, size_t n_values, size_t width, size_t n_boxes, unsigned box_h, unsigned box_w) {
    if (width == 0 || n_values % width) return fail(TRPX_ERR_INVALID_ARG, "%s: width %zu does not divide n_values %zu", fn, width, n_values);
    if (box_h == 0 || box_w == 0 || box_h > n_values / width || box_w > width)
        return fail(TRPX_ERR_INVALID_ARG, "%s: box %u x %u in frames of %zu x %zu", fn, box_h, box_w, n_values / width, width);
    if (n_boxes == 0) return fail(TRPX_ERR_INVALID_ARG, "%s: no boxes", fn);
    return TRPX_OK;
}

// ---- threshold decode (decode_sparse.hip): its scratch is per (frame, group) [counts u32] [flags 4 x u64] [base u32] and per
// frame [total u32] -----------------------------------------------------------------------------------------------------------------
struct SparseWs { size_t counts, flags, base, frame_total, total; };
SparseWs sparse_ws(const trpx::FrameGeom& g, size_t n_frames) {
    SparseWs w;
    const size_t groups = n_frames * (size_t)g.n_tiles;
    w.counts = 0;
    w.flags = trpx::align_up(w.counts + 4 * groups, 8);
    w.base = w.flags + 32 * groups;
    w.frame_total = w.base + 4 * groups;
    w.total = trpx::align_up(w.frame_total + 4 * n_frames, 8);
    return w;
}
// the rule the device-pointer and the host-pointer entry point share: both outputs, or neither and no capacity (sizes only)
int sparse_outputs(const char* fn, const void* positions, const void* values, size_t capacity) {
    if ((positions == nullptr) != (values == nullptr)) return fail(TRPX_ERR_INVALID_ARG, "%s: positions and values go together", fn);
    if (!positions && capacity) return fail(TRPX_ERR_INVALID_ARG, "%s: capacity %zu without outputs", fn, capacity);
    return TRPX_OK;
}

// ---- weighted per-frame sums (decode_dot.hip): its scratch is [support: one bit per block of a frame] and per (frame, run of 8
// groups, map) [partial sum i64] ------------------------------------------------------------------------------------------------------
struct DotWs { size_t support, partials, total; };
DotWs dot_ws(const trpx::FrameGeom& g, size_t n_frames, unsigned n_maps) {
    DotWs w;
    w.support = 0;
    w.partials = trpx::align_up(w.support + 4 * trpx::support_words(g), 8);
    w.total = w.partials + 8 * n_frames * (size_t)trpx::runs_per_frame(g) * n_maps;
    return w;
}
bool dot_maps_ok(unsigned n_maps) { return n_maps >= 1 && n_maps <= trpx::kDotMaxMaps; }

// ---- sums over labelled bins (decode_bins.hip): its scratch is [support: one bit per block of a frame] and, with more than one
// span per frame, per (frame, span, bin) [partial sum i64] ---------------------------------------------------------------------------
struct BinsWs { size_t support, partials, total; };
BinsWs bins_ws(const trpx::FrameGeom& g, size_t n_frames, unsigned n_bins) {
    BinsWs w;
    const size_t spans = trpx::bins_spans_per_frame(g, n_frames);
    w.support = 0;
    w.partials = trpx::align_up(w.support + 4 * trpx::support_words(g), 8);
    w.total = w.partials + (spans > 1 ? 8 * (size_t)n_bins * n_frames * spans : 0);
    return w;
}
bool bins_count_ok(unsigned n_bins) { return n_bins >= 1 && n_bins <= trpx::kBinsMax; }

// ---- value histograms (decode_hist.hip): its scratch is, with more than one span per group, per (group, span, bin) [partial
// count u64] -- nothing otherwise ------------------------------------------------------------------------------------------------
size_t hist_ws(const trpx::FrameGeom& g, size_t n_frames, size_t group, unsigned n_bins) {
    const size_t spans = trpx::hist_spans_per_group(g, n_frames, group), frames = std::min(group, n_frames);
    return spans > 1 ? 8 * (size_t)n_bins * ((n_frames + frames - 1) / frames) * spans : 0;
}

// ---- binned decode (decode_binned.hip): no scratch of its own ------------------------------------------------------------------------
// the checks the device-pointer and the host-pointer entry point share, behind the stack's own (a frame has < 2^29 values, see
// frame_bits_fit_32); 0 = fine
int binned_geometry(const char* fn, int dtype, int out_dtype, size_t n_values, size_t width, unsigned bin_y, unsigned bin_x) {
    if (!sum_out_ok(out_dtype)) return fail(TRPX_ERR_INVALID_ARG, "%s: out_dtype %d (I32, U32, I64, U64, F32, F64)", fn, out_dtype);
    if (trpx_dtype_is_signed(dtype) && (out_dtype == TRPX_U32 || out_dtype == TRPX_U64))
        return fail(TRPX_ERR_UNSUPPORTED, "%s: signed stream into an unsigned output (Terse.hpp:356-357)", fn);
    if (width == 0 || n_values % width) return fail(TRPX_ERR_INVALID_ARG, "%s: width %zu does not divide n_values %zu", fn, width, n_values);
    const size_t height = n_values / width;
    if (bin_y == 0 || bin_x == 0 || bin_y > trpx::kBinnedMaxBin || bin_x > trpx::kBinnedMaxBin || bin_y > height || bin_x > width)
        return fail(TRPX_ERR_INVALID_ARG, "%s: bin %u x %u in frames of %zu x %zu (1..%u, within the frame)", fn, bin_y, bin_x, height, width,
                    trpx::kBinnedMaxBin);
    if ((width + bin_x - 1) / bin_x > trpx::kBinnedAccs)
        return fail(TRPX_ERR_UNSUPPORTED, "%s: %zu bins in a row (at most %u)", fn, (width + bin_x - 1) / bin_x, trpx::kBinnedAccs);
    return TRPX_OK;
}

// ---- reducing decode (decode_reduce.hip): the ops of trpx_reduce_op ---------------------------------------------------------------
static_assert((int)TRPX_REDUCE_MAX == (int)trpx::kReduceMax && (int)TRPX_REDUCE_MIN == (int)trpx::kReduceMin &&
              (int)TRPX_REDUCE_SUMSQ == (int)trpx::kReduceSumSq && (int)TRPX_REDUCE_COUNT_GE == (int)trpx::kReduceCountGe,
              "reduce_ops.hpp names the values of trpx_reduce_op");
bool reduce_op_ok(int op) { return op >= 0 && op < trpx::kReduceOps; }

// ---- labelled summing decode (decode_sum_labelled.hip) -----------------------------------------------------------------------------
bool labelled_out_ok(size_t n_out) { return n_out >= 1 && n_out <= trpx::kLabelledMaxOut; }
}  // namespace

extern "C" {

size_t trpx_decode_sum_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                                       unsigned group) {
    trpx::FrameGeom g;
    const size_t front = consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
    return front && group ? front + trpx::sum_plan(dtype, g, n_frames, group).partial_bytes : 0;
}

// (its own order of checks: sum_checks)
int trpx_decode_sum(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                    const void* index, size_t n_values, size_t n_frames, unsigned block, unsigned group, void* sums_out,
                    uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    Consumer c{"trpx_decode_sum", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, {}, status, workspace,
               workspace_bytes, stream};
    const auto own = [&] { return group ? TRPX_OK : fail(TRPX_ERR_INVALID_ARG, "trpx_decode_sum: group = 0"); };
    if (const int rc = sum_checks(c, out_dtype, sums_out, own, {}, "terse")) return rc;
    const trpx::FrameGeom& g = c.g;
    const trpx::SumPlan p = trpx::sum_plan(dtype, g, n_frames, group);
    IndexWs w;
    if (const int rc = consumer_ws(c, p.partial_bytes, nullptr, &w)) return rc;
    if (p.n_out * p.chunks * (uint64_t)p.tpf >= (1ull << 40)) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_sum: bad sizes");
    if (workspace) trpx::fused_ws_forget(workspace, workspace_bytes);            // (also in the form that needs none)
    Front f;
    // (no k_check_index behind the walk: k_sum_tiles compares every block's header bit with its widths on the way)
    if (const int rc = consumer_front(c, w, false, &f)) return rc;
    trpx::SumArgs a{};
    trpx::set_stack(a, f.stack);
    a.group = group;
    a.n_out = p.n_out;
    a.tpf = p.tpf;
    a.chunks = p.chunks;
    a.fpc = p.fpc;
    a.out = sums_out;
    a.out_code = out_dtype;
    a.partial = p.chunks > 1 ? f.own : nullptr;
    a.status = status;
    HIP_TRY(trpx::launch_decode_sum(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

size_t trpx_decode_roi_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    return consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
}

int trpx_decode_roi(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                    size_t n_values, size_t n_frames, unsigned block, size_t width, const uint32_t* boxes, size_t n_boxes,
                    unsigned box_h, unsigned box_w, void* pixels_out, uint32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (const int rc = check_args("trpx_decode_roi", kDtypeFirst | kIndexOnly | kHasStream, dtype, es, 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {boxes, 4}, {pixels_out, es}, {status, 8}, {frame_offsets, 8, false}, {index, 16, false},
                                   {workspace, 8, false}}, &g))
        return rc;
    const Consumer c{"trpx_decode_roi", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, g, status, workspace,
                     workspace_bytes, stream};
    if (const int rc = stack_limits(c)) return rc;
    if (const int rc = roi_geometry("trpx_decode_roi", n_values, width, n_boxes, box_h, box_w)) return rc;
    const uint32_t units = trpx::roi_units_per_box(g, (uint32_t)width, box_h, box_w);
    if ((unsigned __int128)n_boxes * units >= ((unsigned __int128)1 << 40) || (unsigned __int128)n_boxes * box_h * box_w * es >= ((unsigned __int128)1 << 62))
        return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_roi: bad sizes n_boxes=%zu", n_boxes);
    IndexWs w;
    Front f;
    if (const int rc = consumer_ws(c, 0, nullptr, &w)) return rc;             // (offsets and index given: no workspace at all)
    if (const int rc = consumer_front(c, w, true, &f)) return rc;
    trpx::RoiArgs a{};
    trpx::set_stack(a, f.stack);
    a.width = (uint32_t)width;
    a.height = (uint32_t)(n_values / width);
    a.boxes = boxes;
    a.n_boxes = n_boxes;
    a.box_h = box_h;
    a.box_w = box_w;
    a.units_per_box = units;
    a.out = pixels_out;
    a.status = status;
    HIP_TRY(trpx::launch_decode_roi(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

size_t trpx_decode_sparse_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    const size_t front = consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
    return front ? front + sparse_ws(g, n_frames).total : 0;
}

int trpx_decode_sparse(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                       size_t n_values, size_t n_frames, unsigned block, int64_t threshold, uint64_t* row_offsets,
                       uint32_t* positions, void* values, size_t capacity, uint32_t* status, void* workspace, size_t workspace_bytes,
                       void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (const int rc = check_args("trpx_decode_sparse", kDtypeFirst | kIndexOnly | kHasStream, dtype, es, 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {row_offsets, 8}, {status, 8}, {frame_offsets, 8, false}, {index, 16, false},
                                   {workspace, 8, false}, {positions, 4, false}, {values, es, false}}, &g))
        return rc;
    const Consumer c{"trpx_decode_sparse", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, g, status, workspace,
                     workspace_bytes, stream};
    if (const int rc = stack_limits(c)) return rc;
    if (const int rc = sparse_outputs("trpx_decode_sparse", positions, values, capacity)) return rc;
    const SparseWs own = sparse_ws(g, n_frames);
    IndexWs w;
    Front f;
    if (const int rc = consumer_ws(c, own.total, "the counts live there", &w)) return rc;
    if (const int rc = consumer_front(c, w, true, &f)) return rc;
    trpx::SparseArgs a{};
    static_cast<trpx::IndexedStack&>(a) = f.stack;
    a.threshold = threshold;
    a.min_width = trpx::sparse_min_width(threshold, trpx_dtype_is_signed(dtype) != 0);
    a.counts = reinterpret_cast<uint32_t*>(f.own + own.counts);
    a.flags = reinterpret_cast<uint64_t*>(f.own + own.flags);
    a.base = reinterpret_cast<uint32_t*>(f.own + own.base);
    a.frame_total = reinterpret_cast<uint32_t*>(f.own + own.frame_total);
    a.row_offsets = row_offsets;
    a.positions = positions;
    a.values = values;
    a.capacity = capacity;
    a.status = status;
    HIP_TRY(trpx::launch_decode_sparse(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

size_t trpx_decode_dot_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block, unsigned n_maps) {
    trpx::FrameGeom g;
    const size_t front = consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
    return front && dot_maps_ok(n_maps) ? front + dot_ws(g, n_frames, n_maps).total : 0;
}

int trpx_decode_dot(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                    size_t n_values, size_t n_frames, unsigned block, const int32_t* weights, unsigned n_maps, int64_t* dots_out,
                    uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (const int rc = check_args("trpx_decode_dot", kDtypeFirst | kIndexOnly | kHasStream, dtype, es, 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {weights, 4}, {dots_out, 8}, {status, 8}, {frame_offsets, 8, false}, {index, 16, false},
                                   {workspace, 8, false}}, &g))
        return rc;
    const Consumer c{"trpx_decode_dot", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, g, status, workspace,
                     workspace_bytes, stream};
    if (const int rc = stack_limits(c)) return rc;
    if (!dot_maps_ok(n_maps)) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_dot: n_maps=%u (1..%u)", n_maps, trpx::kDotMaxMaps);
    const DotWs own = dot_ws(g, n_frames, n_maps);
    IndexWs w;
    Front f;
    if (const int rc = consumer_ws(c, own.total, "the support bits and the partial sums live there", &w)) return rc;
    if (const int rc = consumer_front(c, w, true, &f)) return rc;
    trpx::DotArgs a{};
    static_cast<trpx::IndexedStack&>(a) = f.stack;
    a.weights = weights;
    a.n_maps = n_maps;
    a.support = reinterpret_cast<uint32_t*>(f.own + own.support);
    a.partials = reinterpret_cast<int64_t*>(f.own + own.partials);
    a.dots_out = dots_out;
    a.status = status;
    HIP_TRY(trpx::launch_decode_dot(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

size_t trpx_decode_bins_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block, unsigned n_bins) {
    trpx::FrameGeom g;
    const size_t front = consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
    return front && bins_count_ok(n_bins) ? front + bins_ws(g, n_frames, n_bins).total : 0;
}

unsigned trpx_decode_bins_spans_per_frame(size_t n_values, size_t n_frames) {
    trpx::FrameGeom g;
    return geom_of(n_values, kBlock, &g) && sizes_ok(g, n_frames) ? trpx::bins_spans_per_frame(g, n_frames) : 0;
}

int trpx_decode_bins(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                     size_t n_values, size_t n_frames, unsigned block, const uint16_t* labels, unsigned n_bins, int64_t* bins_out,
                     uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (const int rc = check_args("trpx_decode_bins", kDtypeFirst | kIndexOnly | kHasStream, dtype, es, 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {labels, 2}, {bins_out, 8}, {status, 8}, {frame_offsets, 8, false}, {index, 16, false},
                                   {workspace, 8, false}}, &g))
        return rc;
    const Consumer c{"trpx_decode_bins", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, g, status, workspace,
                     workspace_bytes, stream};
    if (const int rc = stack_limits(c)) return rc;
    if (!bins_count_ok(n_bins)) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_bins: n_bins=%u (1..%u)", n_bins, trpx::kBinsMax);
    const BinsWs own = bins_ws(g, n_frames, n_bins);
    IndexWs w;
    Front f;
    if (const int rc = consumer_ws(c, own.total, "the support bits live there", &w)) return rc;
    if (const int rc = consumer_front(c, w, true, &f)) return rc;
    trpx::BinsArgs a{};
    static_cast<trpx::IndexedStack&>(a) = f.stack;
    a.labels = labels;
    a.n_bins = n_bins;
    a.spans = trpx::bins_spans_per_frame(g, n_frames);
    a.support = reinterpret_cast<uint32_t*>(f.own + own.support);
    a.partials = reinterpret_cast<int64_t*>(f.own + own.partials);
    a.bins_out = bins_out;
    a.status = status;
    HIP_TRY(trpx::launch_decode_bins(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

size_t trpx_decode_hist_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block, size_t group,
                                        unsigned n_bins) {
    trpx::FrameGeom g;
    const size_t front = consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
    return front && group && bins_count_ok(n_bins) && grid_ok(g, n_frames) ? front + hist_ws(g, n_frames, group, n_bins) : 0;
}

unsigned trpx_decode_hist_spans_per_group(size_t n_values, size_t n_frames, size_t group) {
    trpx::FrameGeom g;
    // (0 for what the call refuses: also for more groups of 256 blocks than one call takes)
    return group && geom_of(n_values, kBlock, &g) && sizes_ok(g, n_frames) && grid_ok(g, n_frames) ? trpx::hist_spans_per_group(g, n_frames, group) : 0;
}

int trpx_decode_hist(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                     size_t n_values, size_t n_frames, unsigned block, size_t group, int64_t lo, unsigned shift, unsigned n_bins,
                     uint64_t* hist_out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (const int rc = check_args("trpx_decode_hist", kDtypeFirst | kIndexOnly | kHasStream, dtype, es, 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {hist_out, 8}, {status, 8}, {frame_offsets, 8, false}, {index, 16, false},
                                   {workspace, 8, false}}, &g))
        return rc;
    const Consumer c{"trpx_decode_hist", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, g, status, workspace,
                     workspace_bytes, stream};
    if (const int rc = stack_limits(c)) return rc;
    if (group == 0) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_hist: group = 0");
    if (!trpx::hist_args_ok(lo, shift, n_bins))
        return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_hist: lo=%lld shift=%u n_bins=%u (|lo| <= 2^32, shift <= %u, 1..%u bins)", (long long)lo, shift,
                    n_bins, trpx::kHistMaxShift, trpx::kHistMaxBins);
    IndexWs w;
    Front f;
    if (const int rc = consumer_ws(c, hist_ws(g, n_frames, group, n_bins), nullptr, &w)) return rc;   // (index given, one span a group: no workspace at all)
    if (const int rc = consumer_front(c, w, true, &f)) return rc;
    trpx::HistArgs a{};
    static_cast<trpx::IndexedStack&>(a) = f.stack;
    a.group = std::min(group, n_frames);
    a.n_groups = (n_frames + a.group - 1) / a.group;
    a.lo = lo;
    a.shift = shift;
    a.n_bins = n_bins;
    a.spans = trpx::hist_spans_per_group(g, n_frames, group);
    a.partials = reinterpret_cast<uint64_t*>(f.own);
    a.hist_out = hist_out;
    a.status = status;
    HIP_TRY(trpx::launch_decode_hist(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

// ---- corrected decode (decode_corrected.hip): no scratch of its own ------------------------------------------------------------------

size_t trpx_decode_corrected_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    const size_t front = consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
    return front && grid_ok(g, n_frames) && n_frames <= terse_bytes && frame_bits_fit_32(dtype, n_values, block) ? front : 0;
}

int trpx_decode_corrected(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                          const void* index, size_t n_values, size_t n_frames, unsigned block, const float* dark, const float* gain,
                          void* out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (const int rc = check_args("trpx_decode_corrected", kDtypeFirst | kIndexOnly | kHasStream, dtype, es, 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {out, out_dtype == TRPX_F32 ? 4u : 1u}, {status, 8}, {frame_offsets, 8, false}, {index, 16, false},
                                   {workspace, 8, false}, {dark, 4, false}, {gain, 4, false}}, &g))
        return rc;
    if (out_dtype != TRPX_F32) return fail(TRPX_ERR_UNSUPPORTED, "trpx_decode_corrected: out_dtype %d (F32)", out_dtype);
    const Consumer c{"trpx_decode_corrected", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, g, status, workspace,
                     workspace_bytes, stream};
    if (const int rc = stack_limits(c)) return rc;
    IndexWs w;
    Front f;
    if (const int rc = consumer_ws(c, 0, nullptr, &w)) return rc;             // (offsets and index given: no workspace at all)
    // (no k_check_index behind the walk: k_decode_corrected compares every block's header bit with its widths on the way)
    if (const int rc = consumer_front(c, w, false, &f)) return rc;
    trpx::CorrectedArgs a{};
    static_cast<trpx::IndexedStack&>(a) = f.stack;
    a.dark = dark;
    a.gain = gain;
    a.out = static_cast<float*>(out);
    a.status = status;
    HIP_TRY(trpx::launch_decode_corrected(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

size_t trpx_decode_binned_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    return consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
}

unsigned trpx_decode_binned_bands_per_frame(size_t n_values, size_t width, unsigned bin_y, unsigned bin_x, size_t n_frames) {
    trpx::FrameGeom g;
    if (!geom_of(n_values, kBlock, &g) || !sizes_ok(g, n_frames) || n_values >= ((size_t)1 << 29) || width == 0 || n_values % width) return 0;
    if (bin_y == 0 || bin_x == 0 || bin_y > trpx::kBinnedMaxBin || bin_x > trpx::kBinnedMaxBin || bin_y > n_values / width || bin_x > width) return 0;
    const trpx::BinnedGeom geo = trpx::binned_geom((uint32_t)n_values, (uint32_t)width, bin_y, bin_x);
    return geo.out_w > trpx::kBinnedAccs ? 0 : trpx::binned_plan(geo, n_frames).bands;
}

int trpx_decode_binned(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                       const void* index, size_t n_values, size_t n_frames, unsigned block, size_t width, unsigned bin_y,
                       unsigned bin_x, void* binned_out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (const int rc = check_args("trpx_decode_binned", kDtypeFirst | kIndexOnly | kHasStream, dtype, es, 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {binned_out, sum_out_ok(out_dtype) ? sum_out_size(out_dtype) : 1}, {status, 8},
                                   {frame_offsets, 8, false}, {index, 16, false}, {workspace, 8, false}}, &g))
        return rc;
    const Consumer c{"trpx_decode_binned", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, g, status, workspace,
                     workspace_bytes, stream};
    if (const int rc = stack_limits(c)) return rc;
    if (const int rc = binned_geometry("trpx_decode_binned", dtype, out_dtype, n_values, width, bin_y, bin_x)) return rc;
    IndexWs w;
    Front f;
    if (const int rc = consumer_ws(c, 0, nullptr, &w)) return rc;             // (offsets and index given: no workspace at all)
    if (const int rc = consumer_front(c, w, true, &f)) return rc;
    trpx::BinnedArgs a{};
    static_cast<trpx::IndexedStack&>(a) = f.stack;
    a.geo = trpx::binned_geom((uint32_t)n_values, (uint32_t)width, bin_y, bin_x);
    a.plan = trpx::binned_plan(a.geo, n_frames);
    a.out = binned_out;
    a.out_code = out_dtype;
    a.status = status;
    HIP_TRY(trpx::launch_decode_binned(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

// ---- reducing decode (decode_reduce.hip): trpx_decode_sum's launch plan; its scratch is [partial slab of the op's accumulators] ----

size_t trpx_decode_reduce_workspace_bytes(int dtype, int op, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                                          unsigned group) {
    trpx::FrameGeom g;
    const size_t front = consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
    return front && group && reduce_op_ok(op) ? front + trpx::reduce_partial_bytes(trpx::sum_plan(dtype, g, n_frames, group), op, g) : 0;
}

unsigned trpx_decode_reduce_chunks(int dtype, size_t n_values, size_t n_frames, unsigned group) {
    trpx::FrameGeom g;
    if (dtype < TRPX_U8 || dtype > TRPX_I32 || !group || !geom_of(n_values, kBlock, &g) || !sizes_ok(g, n_frames) ||
        !frame_bits_fit_32(dtype, n_values, kBlock))
        return 0;
    return trpx::sum_plan(dtype, g, n_frames, group).chunks;
}

int trpx_decode_reduce(int dtype, int op, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                       size_t n_values, size_t n_frames, unsigned block, unsigned group, int64_t threshold, void* out,
                       uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (const int rc = check_args("trpx_decode_reduce", kDtypeFirst | kIndexOnly | kHasStream, dtype, es, 0, terse_bytes, n_values, n_frames, block,
                                  {{terse, 4}, {out, reduce_op_ok(op) ? trpx::reduce_out_size(op, es) : 1}, {status, 8},
                                   {frame_offsets, 8, false}, {index, 16, false}, {workspace, 8, false}}, &g))
        return rc;
    if (!reduce_op_ok(op)) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_reduce: unknown op %d (MAX, MIN, SUMSQ, COUNT_GE)", op);
    if (group == 0) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_reduce: group = 0");
    const Consumer c{"trpx_decode_reduce", dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, g, status, workspace,
                     workspace_bytes, stream};
    if (const int rc = stack_limits(c)) return rc;
    const trpx::SumPlan p = trpx::sum_plan(dtype, g, n_frames, group);
    IndexWs w;
    Front f;
    if (const int rc = consumer_ws(c, trpx::reduce_partial_bytes(p, op, g), nullptr, &w)) return rc;   // (index given, one chunk: no workspace at all)
    if (p.n_out * p.chunks * (uint64_t)p.tpf >= (1ull << 40)) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_reduce: bad sizes");
    // (no k_check_index behind the walk: k_reduce_tiles compares every block's header bit with its widths on the way)
    if (const int rc = consumer_front(c, w, false, &f)) return rc;
    trpx::ReduceArgs a{};
    trpx::set_stack(a, f.stack);
    a.group = group;
    a.n_out = p.n_out;
    a.tpf = p.tpf;
    a.chunks = p.chunks;
    a.fpc = p.fpc;
    a.out = out;
    a.threshold = threshold;
    a.partial = p.chunks > 1 ? f.own : nullptr;
    a.status = status;
    HIP_TRY(trpx::launch_decode_reduce(dtype, op, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

// ---- labelled summing decode (decode_sum_labelled.hip): its scratch is LabelledPlan's -- the frames' order and the partial slab ----

size_t trpx_decode_sum_labelled_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                                                size_t n_out) {
    trpx::FrameGeom g;
    const size_t front = consumer_front_bytes(dtype, terse_bytes, n_values, n_frames, block, &g);
    return front && labelled_out_ok(n_out) ? front + trpx::labelled_plan(dtype, g, n_frames, n_out).total : 0;
}

unsigned trpx_decode_sum_labelled_frames_per_chunk(int dtype, size_t n_values, size_t n_frames) {
    trpx::FrameGeom g;
    if (dtype < TRPX_U8 || dtype > TRPX_I32 || !geom_of(n_values, kBlock, &g) || !sizes_ok(g, n_frames) ||
        !frame_bits_fit_32(dtype, n_values, kBlock))
        return 0;
    return trpx::labelled_plan(dtype, g, n_frames, 1).fpc;
}

// (trpx_decode_sum's order of checks, sum_checks, the outputs' count where its group stands)
int trpx_decode_sum_labelled(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                             const void* index, size_t n_values, size_t n_frames, unsigned block, const uint32_t* labels, size_t n_out,
                             void* sums_out, uint32_t* counts_out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const char* const fn = "trpx_decode_sum_labelled";
    Consumer c{fn, dtype, terse, terse_bytes, frame_offsets, index, n_values, n_frames, block, {}, status, workspace, workspace_bytes, stream};
    const auto own = [&] {
        if (n_out == 0) return fail(TRPX_ERR_INVALID_ARG, "%s: n_out = 0", fn);
        return labelled_out_ok(n_out) ? TRPX_OK : fail(TRPX_ERR_UNSUPPORTED, "%s: n_out=%zu (at most 2^20)", fn, n_out);
    };
    if (const int rc = sum_checks(c, out_dtype, sums_out, own, {{labels, 4}, {counts_out, 4, false}}, "terse / labels / counts")) return rc;
    const trpx::FrameGeom& g = c.g;
    const trpx::LabelledPlan p = trpx::labelled_plan(dtype, g, n_frames, n_out);
    IndexWs w;
    if (const int rc = consumer_ws(c, p.total, "the order of the frames lives there", &w)) return rc;
    Front f;
    // (no k_check_index behind the walk: k_sum_labelled compares every block's header bit with its widths on the way)
    if (const int rc = consumer_front(c, w, false, &f)) return rc;
    trpx::LabelledArgs a{};
    trpx::set_stack(a, f.stack);
    a.n_out = (uint32_t)n_out;
    a.tpf = p.tpf;
    a.n_chunks = p.n_chunks;
    a.fpc = p.fpc;
    a.labels = labels;
    a.out = sums_out;
    a.out_code = out_dtype;
    a.counts_out = counts_out;
    a.counts = reinterpret_cast<uint32_t*>(f.own + p.counts);
    a.cursor = reinterpret_cast<uint32_t*>(f.own + p.cursor);
    a.starts = reinterpret_cast<uint32_t*>(f.own + p.starts);
    a.todo = reinterpret_cast<uint32_t*>(f.own + p.todo);
    a.order = reinterpret_cast<uint2*>(f.own + p.order);
    a.partial = f.own + p.slab;
    a.stride = p.stride;
    a.status = status;
    HIP_TRY(trpx::launch_decode_sum_labelled(dtype, a, f.clear, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

// ---- encode from events (encode_sparse.hip) ----------------------------------------------------------------------------------
}  // extern "C"
namespace {
// trpx_encode_sparse's workspace: the two-pass encoder's [frame_size u64 x F] [tile_off u64 x F*T] [tile_bits u32 x F*T] and
// [tile_lo u32 x F*T], the events of the frame in front of every tile: 16 bytes per tile + 8 per frame, nothing per pixel.
struct SparseEncWs { size_t frame_size, tile_off, tile_bits, tile_lo, total; };
SparseEncWs sparse_enc_ws(const trpx::FrameGeom& g, size_t n_frames) {
    SparseEncWs w;
    const size_t tiles = n_frames * (size_t)g.n_tiles;
    w.frame_size = 0;
    w.tile_off = 8 * n_frames;
    w.tile_bits = w.tile_off + 8 * tiles;
    w.tile_lo = w.tile_bits + 4 * tiles;
    w.total = trpx::align_up(w.tile_lo + 4 * tiles, 8);
    return w;
}
// what the call supports at all (the rest is UNSUPPORTED or INVALID_ARG there, 0 in the size queries)
bool sparse_enc_supported(int dtype, size_t n_values, size_t n_frames, unsigned block, trpx::FrameGeom* g) {
    return dtype >= TRPX_U8 && dtype <= TRPX_I32 && block == kBlock && n_values < (1ull << 32) && geom_of(n_values, block, g) &&
           sizes_ok(*g, n_frames);
}
// the rule the device-pointer and the host-pointer entry point share: both lists, or neither and no events
int sparse_enc_inputs(const char* fn, const void* positions, const void* values, size_t n_events) {
    if ((positions == nullptr) != (values == nullptr)) return fail(TRPX_ERR_INVALID_ARG, "%s: positions and values go together", fn);
    if (!positions && n_events) return fail(TRPX_ERR_INVALID_ARG, "%s: %zu events without lists", fn, n_events);
    return TRPX_OK;
}
}  // namespace
extern "C" {

size_t trpx_encode_sparse_workspace_bytes(int dtype, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    if (!sparse_enc_supported(dtype, n_values, n_frames, block, &g)) return 0;
    return sparse_enc_ws(g, n_frames).total;
}

size_t trpx_encode_sparse_bound_bytes(int dtype, size_t n_values, size_t n_frames, size_t n_events, unsigned block) {
    trpx::FrameGeom g;
    if (!sparse_enc_supported(dtype, n_values, n_frames, block, &g)) return 0;
    return trpx::sparse_bound_bytes(trpx_dtype_size(dtype), g.n_blocks, n_frames, n_events,               // (derived there)
                                    (uint64_t)n_frames * trpx_worst_case_bytes(dtype, n_values, block));
}

int trpx_encode_sparse(int dtype, const uint64_t* row_offsets, const uint32_t* positions, const void* values, size_t n_events,
                       size_t n_values, size_t n_frames, unsigned block, uint8_t* out, size_t out_capacity, uint64_t* frame_offsets,
                       uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (!es) return fail(TRPX_ERR_INVALID_ARG, "trpx_encode_sparse: unknown dtype %d", dtype);
    if (block != kBlock || is64(dtype)) return fail(TRPX_ERR_UNSUPPORTED, "trpx_encode_sparse: block=%u dtype=%d (block 12, containers of <= 32 bits)", block, dtype);
    if (const int rc = check_args("trpx_encode_sparse", kDtypeFirst, dtype, es, 0, 0, n_values, n_frames, block,
                                  {{row_offsets, 8}, {frame_offsets, 8}, {status, 8}, {workspace, 8}, {positions, 4, false},
                                   {values, es, false}, {out, 16, out_capacity != 0}}, &g))
        return rc;
    if (n_values >= (1ull << 32)) return fail(TRPX_ERR_UNSUPPORTED, "trpx_encode_sparse: n_values=%zu (positions are 32-bit)", n_values);
    if (const int rc = sparse_enc_inputs("trpx_encode_sparse", positions, values, n_events)) return rc;
    const SparseEncWs w = sparse_enc_ws(g, n_frames);
    if (workspace_bytes < w.total) return fail(TRPX_ERR_CAPACITY, "trpx_encode_sparse: workspace %zu < %zu", workspace_bytes, w.total);

    trpx::fused_ws_forget(workspace, workspace_bytes);
    char* ws = static_cast<char*>(workspace);
    trpx::SparseEncodeArgs a{};
    a.row_offsets = row_offsets;
    a.positions = positions;
    a.values = values;
    a.n_events = n_events;
    a.geom = g;
    a.n_frames = (uint32_t)n_frames;
    a.out = out;
    a.out_capacity = out_capacity;
    a.frame_offsets = frame_offsets;
    a.status = status;
    a.frame_size = reinterpret_cast<uint64_t*>(ws + w.frame_size);
    a.tile_off = reinterpret_cast<uint64_t*>(ws + w.tile_off);
    a.tile_bits = reinterpret_cast<uint32_t*>(ws + w.tile_bits);
    a.tile_lo = reinterpret_cast<uint32_t*>(ws + w.tile_lo);
    HIP_TRY(trpx::launch_encode_sparse(dtype, a, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

// ---- frames of a stack into a new stack (select_frames.hip): bytes move, no pixel is touched -------------------------------------
}  // extern "C"
namespace {
// what the device-pointer and the host-pointer entry point refuse alike, behind their dtype / block / geometry checks
int select_sizes(const char* fn, size_t terse_bytes, size_t n_frames, size_t n_select) {
    if (!terse_bytes || !n_select || n_select > 0x7FFFFFFFull || n_frames > terse_bytes)   // every frame is at least one byte (Terse.hpp:547)
        return fail(TRPX_ERR_INVALID_ARG, "%s: bad sizes terse_bytes=%zu n_frames=%zu n_select=%zu", fn, terse_bytes, n_frames, n_select);
    return TRPX_OK;
}
}  // namespace
extern "C" {

size_t trpx_select_frames_workspace_bytes(size_t n_frames, size_t n_select) {
    if (!n_frames || !n_select || n_select > 0x7FFFFFFFull) return 0;
    return trpx::select_workspace_bytes(n_select);
}

int trpx_select_frames(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                       size_t n_values, size_t n_frames, unsigned block, const uint32_t* frames, size_t n_select, uint8_t* out,
                       size_t out_capacity, uint64_t* out_offsets, void* out_index, uint32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream) {
    trpx::FrameGeom g;
    if (const int rc = check_args("trpx_select_frames", kDtypeFirst | kHasStream, dtype, trpx_dtype_size(dtype), 0, terse_bytes, n_values, n_frames,
                                  block, {{terse, 4}, {frame_offsets, 8}, {frames, 4}, {out_offsets, 8}, {status, 8}, {workspace, 8},
                                          {out, 16, out_capacity != 0}, {index, 16, false}, {out_index, 16, false}}, &g))
        return rc;
    if (const int rc = select_sizes("trpx_select_frames", terse_bytes, n_frames, n_select)) return rc;
    if ((index == nullptr) != (out_index == nullptr)) return fail(TRPX_ERR_INVALID_ARG, "trpx_select_frames: index and out_index go together");
    if (index && (block != kBlock || is64(dtype)))
        return fail(TRPX_ERR_UNSUPPORTED, "trpx_select_frames: the decode index needs block=12 and pixels of <= 32 bits");
    if (index && !sizes_ok(g, n_select)) return fail(TRPX_ERR_INVALID_ARG, "trpx_select_frames: no index for n_select=%zu frames", n_select);
    const size_t need = trpx::select_workspace_bytes(n_select);
    if (workspace_bytes < need) return fail(TRPX_ERR_CAPACITY, "trpx_select_frames: workspace %zu < %zu", workspace_bytes, need);

    trpx::fused_ws_forget(workspace, workspace_bytes);
    trpx::SelectArgs a{};
    a.terse = terse;
    a.terse_bytes = terse_bytes;
    a.frame_offsets = frame_offsets;
    a.n_frames = (uint32_t)n_frames;
    a.frames = frames;
    a.n_select = (uint32_t)n_select;
    a.out = out;
    a.out_capacity = out_capacity;
    a.out_offsets = out_offsets;
    a.status = status;
    a.workspace = workspace;
    if (index) {                                                                // rows of the source's index into the result's
        const DecLayout in = idx_layout(g, n_frames, trpx_dtype_size(dtype)), ol = idx_layout(g, n_select, trpx_dtype_size(dtype));
        a.n_blocks = g.n_blocks;
        a.n_tiles = g.n_tiles;
        a.widths = static_cast<const uint8_t*>(index) + in.widths;
        a.tile_off = reinterpret_cast<const uint64_t*>(static_cast<const char*>(index) + in.tile_off);
        a.out_widths = static_cast<uint8_t*>(out_index) + ol.widths;
        a.out_tile_off = reinterpret_cast<uint64_t*>(static_cast<char*>(out_index) + ol.tile_off);
    }
    HIP_TRY(trpx::launch_select_frames(a, static_cast<hipStream_t>(stream)));
    return TRPX_OK;
}

// ---- host-pointer convenience wrappers ---------------------------------------------------
// The callers of the reference's API work frame by frame from host memory (src/terse.cpp:63-69 pushes one image at a
// time, src/prolix.cpp:69-92 expands one frame at a time): a device allocation per call would cost more than the
// codec.  Every thread keeps ONE grow-only set of device buffers per role (freed by trpx_host_release or at exit of the
// process); the host wrappers carve their pixels / stream / offsets / status / workspace from it.  Each wrapper reads:
// enter, validate, stage, call the device-pointer entry point, read the status, copy back; the ten of the index consumers
// validate and leave the rest to consumer_host.
}  // extern "C"
namespace {
struct Arena {
    enum { kPixels, kStream, kOffsets, kStatus, kWorkspace, kSlots };
    void* p[kSlots] = {};
    size_t cap[kSlots] = {};
    int device = -1;
    hipStream_t stream = nullptr;                            // this thread's private, non-blocking stream: the host wrappers
                                                             // order their copies and kernels on it and wait for IT alone
    hipError_t on_device() {
        int dev = 0;
        const hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev != device) { release(); device = dev; }
        return hipSuccess;
    }
    // (the workspace slot is the one piece of memory trpx_encode registers as a clean descriptor block: every OTHER user of
    // it -- an index, a walk's scratch -- makes the library forget that first; `encoder` = trpx_encode_host itself)
    hipError_t get(int slot, size_t n, void** out, bool encoder = false) {
        hipError_t e = on_device();
        if (e != hipSuccess) return e;
        if (slot == kWorkspace && !encoder && p[slot]) trpx::fused_ws_forget(p[slot], cap[slot]);
        if (cap[slot] < n) {
            if (p[slot] && slot == kWorkspace) trpx::fused_ws_forget(p[slot], cap[slot]);
            if (p[slot]) (void)hipFree(p[slot]);
            p[slot] = nullptr; cap[slot] = 0;
            const size_t want = n + n / 8 + 256;             // a little head room: stacks of slightly different sizes reuse it
            e = hipMalloc(&p[slot], want);
            if (e != hipSuccess) return e;
            cap[slot] = want;
        }
        *out = p[slot];
        return hipSuccess;
    }
    hipError_t get_stream(hipStream_t* out) {
        hipError_t e = on_device();
        if (e != hipSuccess) return e;
        if (!stream && (e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) != hipSuccess) return e;
        *out = stream;
        return hipSuccess;
    }
    void release() {
        if (p[kWorkspace]) trpx::fused_ws_forget(p[kWorkspace], cap[kWorkspace]);
        for (int i = 0; i < kSlots; ++i) { if (p[i]) (void)hipFree(p[i]); p[i] = nullptr; cap[i] = 0; }
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
    ~Arena() { release(); }                                  // thread exit: the buffers go back (errors of a runtime that is already down are ignored)
};
Arena& arena() {
    static thread_local Arena a;
    return a;
}

// every host wrapper starts here: a device at all, the device asked for, this thread's private stream
int enter(const char* fn, int device, hipStream_t* hs) {
    if (trpx_device_count() == 0) return fail(TRPX_ERR_NO_DEVICE, "%s: no HIP device", fn);
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    HIP_TRY(arena().get_stream(hs));
    return TRPX_OK;
}
// The kernels read the stream in aligned 32-bit words and a little past its end, and rely on the bytes behind it reading as zero:
// a device copy of a stream is padded_stream_bytes() long, and this is the one place that writes its zero tail.
size_t padded_stream_bytes(size_t terse_bytes) { return trpx::align_up(terse_bytes, 4) + 8; }
hipError_t copy_stream_zero_tail(hipStream_t hs, void* d_terse, const uint8_t* terse, size_t terse_bytes) {
    const size_t whole = terse_bytes & ~size_t(3);
    const hipError_t e = hipMemsetAsync(static_cast<char*>(d_terse) + whole, 0, padded_stream_bytes(terse_bytes) - whole, hs);
    return e != hipSuccess ? e : copy_sync(hs, d_terse, terse, terse_bytes, hipMemcpyHostToDevice);
}
int upload_stream(hipStream_t hs, const uint8_t* terse, size_t terse_bytes, const uint8_t** d_terse) {
    void* p = nullptr;
    HIP_TRY(arena().get(Arena::kStream, padded_stream_bytes(terse_bytes), &p));
    HIP_TRY(copy_stream_zero_tail(hs, p, terse, terse_bytes));
    *d_terse = static_cast<const uint8_t*>(p);
    return TRPX_OK;
}
// the offsets slot: n_frames + 1 offsets (uploaded where the caller has them) and `extra` bytes behind them
int upload_offsets(hipStream_t hs, const uint64_t* frame_offsets, size_t n_frames, size_t extra, uint64_t** d_offs) {
    void* p = nullptr;
    HIP_TRY(arena().get(Arena::kOffsets, 8 * (n_frames + 1) + extra, &p));
    if (frame_offsets) HIP_TRY(copy_sync(hs, p, frame_offsets, 8 * (n_frames + 1), hipMemcpyHostToDevice));
    *d_offs = static_cast<uint64_t*>(p);
    return TRPX_OK;
}
int status_slot(uint32_t** d_st) {
    void* p = nullptr;
    HIP_TRY(arena().get(Arena::kStatus, 4 * TRPX_STATUS_WORDS, &p));
    *d_st = static_cast<uint32_t*>(p);
    return TRPX_OK;
}
// What every decoding host wrapper stages: the padded stream, the status slot, the offsets slot (offs_slot: wanted at all;
// uploaded where the caller has them, offs_extra bytes behind them), the output block and the workspace.
struct Staged { const uint8_t* terse; uint32_t* status; uint64_t* offs; void* out; void* ws; };
int stage(hipStream_t hs, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_frames, bool offs_slot,
          size_t offs_extra, size_t out_bytes, size_t ws_bytes, Staged* s) {
    *s = {};
    int rc = upload_stream(hs, terse, terse_bytes, &s->terse);
    if (rc || (rc = status_slot(&s->status)) || (offs_slot && (rc = upload_offsets(hs, frame_offsets, n_frames, offs_extra, &s->offs)))) return rc;
    if (out_bytes) HIP_TRY(arena().get(Arena::kPixels, out_bytes, &s->out));
    HIP_TRY(arena().get(Arena::kWorkspace, ws_bytes, &s->ws));
    return TRPX_OK;
}
// what a host wrapper answers for the work it queued on hs: the status block read back (into st), as a return code
int finish(const char* fn, hipStream_t hs, const uint32_t* d_status, uint32_t st[TRPX_STATUS_WORDS]) {
    const int rc = read_status(hs, d_status, st);
    return rc ? rc : status_result(fn, st);
}
// what the host wrappers of the index consumers refuse first (own_ok: the wrapper's own pointers and counts)
int consumer_host_refusals(const char* fn, bool own_ok, int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block) {
    trpx::FrameGeom g;
    if (!own_ok || !terse_bytes) return fail(TRPX_ERR_INVALID_ARG, "%s: bad argument", fn);
    if (block != kBlock || is64(dtype)) return fail(TRPX_ERR_UNSUPPORTED, "%s: block=%u dtype=%d", fn, block, dtype);
    if (!geom_of(n_values, block, &g) || !sizes_ok(g, n_frames)) return fail(TRPX_ERR_INVALID_ARG, "%s: bad sizes", fn);
    return TRPX_OK;
}
// the end of the encoding host wrappers: the offsets back, their total against the caller's room, the stream back
int download_stream(const char* fn, hipStream_t hs, const uint64_t* d_off, const void* d_out, size_t n_frames, const uint32_t* st, uint8_t* out,
                    size_t out_capacity, size_t* total_bytes, uint64_t* frame_offsets, uint32_t* prolix_bits) {
    std::vector<uint64_t> offs(n_frames + 1);
    HIP_TRY(copy_sync(hs, offs.data(), d_off, 8 * (n_frames + 1), hipMemcpyDeviceToHost));
    const size_t total = (size_t)offs[n_frames];
    if (total > out_capacity) return fail(TRPX_ERR_CAPACITY, "%s: need %zu bytes, have %zu", fn, total, out_capacity);
    HIP_TRY(copy_sync(hs, out, d_out, total, hipMemcpyDeviceToHost));
    *total_bytes = total;
    if (frame_offsets) memcpy(frame_offsets, offs.data(), 8 * (n_frames + 1));
    if (prolix_bits) *prolix_bits = st[1];
    return TRPX_OK;
}

// Decode into any output type, everything on the device, the last status block in st.  Same signedness into <= 32 bits: the
// tuned decoders.  They report CORRUPT for a block wider than the output type, which is also what a legitimately wider stream
// looks like (e.g. u16 data into a u8 container, Bit_pointer.hpp:747-763; a stream of 64-bit pixels): those -- and every
// cross-kind / float / double / 64-bit request -- take the converting decoder, whose verdict is final.
int decode_any(int stream_signed, int out_dtype, const uint8_t* d_terse, size_t terse_bytes, const uint64_t* d_offs, size_t n_values,
               size_t n_frames, unsigned block, void* d_out, uint32_t* d_st, void* d_ws, size_t ws_bytes, hipStream_t hs,
               uint32_t st[TRPX_STATUS_WORDS]) {
    for (bool convert = !tuned_type(stream_signed, out_dtype);; convert = true) {
        int rc = convert ? trpx_decode_convert(stream_signed, out_dtype, d_terse, terse_bytes, d_offs, n_values, n_frames, block, d_out, d_st, d_ws, ws_bytes, hs)
                         : trpx_decode(stream_signed, out_dtype, d_terse, terse_bytes, d_offs, n_values, n_frames, block, d_out, d_st, d_ws, ws_bytes, hs);
        if (rc || (rc = read_status(hs, d_st, st))) return rc;
        if (st[0] != TRPX_ERR_CORRUPT || convert) return TRPX_OK;
    }
}
// Walk-free decode of frames whose group states came with the file: the decode index from the states, then the indexed decode.
// The last status block in st; *decoded: the indexed decode ran.  It does not run when the index step reports CORRUPT (the
// states do not describe this stream, or the data are wider than the output type) or, with stop_on_any, anything at all.
int decode_walk_free(int stream_signed, int out_dtype, const uint8_t* d_terse, size_t terse_bytes, const uint64_t* d_offs,
                     const uint64_t* d_states, size_t n_values, size_t n_frames, unsigned block, void* d_index, void* d_out,
                     uint32_t* d_st, hipStream_t hs, bool stop_on_any, uint32_t st[TRPX_STATUS_WORDS], bool* decoded) {
    *decoded = false;
    int rc = trpx_index_from_group_states(out_dtype, d_terse, terse_bytes, d_offs, d_states, n_values, n_frames, block, d_index, d_st, hs);
    if (rc || (rc = read_status(hs, d_st, st))) return rc;
    if (st[0] == TRPX_ERR_CORRUPT || (stop_on_any && st[0])) return TRPX_OK;
    rc = trpx_decode_indexed(stream_signed, out_dtype, d_terse, terse_bytes, d_offs, d_index, n_values, n_frames, block, d_out, d_st, hs);
    if (rc || (rc = read_status(hs, d_st, st))) return rc;
    *decoded = true;
    return TRPX_OK;
}
}  // namespace
extern "C" {

void trpx_host_release(void) { arena().release(); }

int trpx_encode_host(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block, uint8_t* out,
                     size_t out_capacity, size_t* total_bytes, uint64_t* frame_offsets, uint32_t* prolix_bits,
                     int device) {
    hipStream_t hs = nullptr;
    if (const int rc = enter("trpx_encode_host", device, &hs)) return rc;
    const size_t es = trpx_dtype_size(dtype);
    if (!es || !pixels || !out || !total_bytes) return fail(TRPX_ERR_INVALID_ARG, "trpx_encode_host: bad argument");
    trpx::FrameGeom g;
    if (!geom_of(n_values, block, &g)) return fail(block == 0 || block > kMaxBlock ? TRPX_ERR_UNSUPPORTED : TRPX_ERR_INVALID_ARG, "trpx_encode_host: unsupported sizes/block (block=%u)", block);
    if (!sizes_ok(g, n_frames)) return fail(TRPX_ERR_INVALID_ARG, "trpx_encode_host: bad sizes n_values=%zu n_frames=%zu", n_values, n_frames);
    const size_t in_bytes = n_values * n_frames * es;
    const size_t cap = trpx::align_up(n_frames * trpx_worst_case_bytes(dtype, n_values, block), 16);
    const size_t ws_bytes = enc_ws(g, n_frames).total;
    void *d_px = nullptr, *d_out = nullptr, *d_ws = nullptr;
    uint64_t* d_off = nullptr;
    uint32_t* d_st = nullptr;
    Arena& A = arena();
    HIP_TRY(A.get(Arena::kPixels, in_bytes, &d_px));
    HIP_TRY(A.get(Arena::kStream, cap, &d_out));
    HIP_TRY(A.get(Arena::kWorkspace, ws_bytes, &d_ws, true));
    int rc = upload_offsets(hs, nullptr, n_frames, 0, &d_off);
    if (rc || (rc = status_slot(&d_st))) return rc;
    HIP_TRY(copy_sync(hs, d_px, pixels, in_bytes, hipMemcpyHostToDevice));
    uint32_t st[TRPX_STATUS_WORDS];
    rc = encode_retrying(dtype, d_px, n_values, n_frames, block, static_cast<uint8_t*>(d_out), cap, d_off, d_st, nullptr, d_ws, ws_bytes, hs, st);
    if (rc || (rc = status_result("trpx_encode_host", st))) return rc;
    return download_stream("trpx_encode_host", hs, d_off, d_out, n_frames, st, out, out_capacity, total_bytes, frame_offsets, prolix_bits);
}

int trpx_decode_host(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                     const uint64_t* frame_offsets, size_t n_values, size_t n_frames, unsigned block,
                     void* pixels_out, int device) {
    hipStream_t hs = nullptr;
    if (const int rc = enter("trpx_decode_host", device, &hs)) return rc;
    const size_t es = convert_elem_size(out_dtype);
    if (!es || !terse || !pixels_out || !terse_bytes) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_host: bad argument");
    trpx::FrameGeom g;
    if (!geom_of(n_values, block, &g)) return bad_geom("trpx_decode_host", block);
    if (!sizes_ok(g, n_frames)) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_host: bad sizes");
    const size_t out_bytes = n_values * n_frames * es;
    const size_t ws_bytes = trpx_decode_workspace_bytes(TRPX_U8, n_values, n_frames, block);
    Staged d;
    int rc = stage(hs, terse, terse_bytes, frame_offsets, n_frames, frame_offsets != nullptr, 0, out_bytes, ws_bytes, &d);
    if (rc) return rc;
    uint32_t st[TRPX_STATUS_WORDS];
    rc = decode_any(stream_signed, out_dtype, d.terse, terse_bytes, d.offs, n_values, n_frames, block, d.out, d.status, d.ws, ws_bytes, hs, st);
    if (rc || (rc = status_result("trpx_decode_host", st))) return rc;
    HIP_TRY(copy_sync(hs, pixels_out, d.out, out_bytes, hipMemcpyDeviceToHost));
    return TRPX_OK;
}

int trpx_frame_offsets_host(const uint8_t* terse, size_t terse_bytes, size_t n_values, size_t n_frames,
                            unsigned block, unsigned max_bits, uint64_t* frame_offsets, int device) {
    hipStream_t hs = nullptr;
    if (const int rc = enter("trpx_frame_offsets_host", device, &hs)) return rc;
    trpx::FrameGeom g;
    if (!terse || !terse_bytes || !frame_offsets || !n_frames || max_bits == 0 || max_bits > 64)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_frame_offsets_host: bad argument");
    if (!geom_of(n_values, block, &g)) return bad_geom("trpx_frame_offsets_host", block);
    if (!sizes_ok(g, n_frames) || n_frames > terse_bytes)                     // every frame is at least one byte (Terse.hpp:547)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_frame_offsets_host: bad sizes n_values=%zu n_frames=%zu", n_values, n_frames);
    const size_t ws_bytes = trpx::locate_workspace_bytes(g, terse_bytes, n_frames);
    Staged d;                                                                  // (the offsets slot is the output)
    int rc = stage(hs, terse, terse_bytes, nullptr, n_frames, true, 0, 0, ws_bytes, &d);
    if (rc) return rc;
    uint32_t st[TRPX_STATUS_WORDS];
    rc = trpx_locate_frames(d.terse, terse_bytes, n_values, n_frames, block, max_bits, d.offs, d.status, d.ws, ws_bytes, hs);
    if (rc || (rc = finish("trpx_frame_offsets_host", hs, d.status, st))) return rc;
    HIP_TRY(copy_sync(hs, frame_offsets, d.offs, 8 * (n_frames + 1), hipMemcpyDeviceToHost));
    return TRPX_OK;
}

}  // extern "C"
namespace {
// ---- the host forms of the index consumers: one staged call -----------------------------------------------------------------------
// A wrapper refuses what is its own (consumer_host_refusals, then its own shapes and counts), asks its workspace query and hands
// the rest to consumer_host: the stack's limits, the device, the staging, the device-pointer call, its status, the copies back.
// The argument checks need no device, so they come first: the same answers with and without one.
struct HostStack { int dtype; const uint8_t* terse; size_t terse_bytes; const uint64_t* frame_offsets; size_t n_values, n_frames; unsigned block; };
// one piece of a call's device block: uploaded from `in` (null: not), downloaded to `out` (null: not)
struct HostPiece { const void* in; void* out; size_t bytes; };
constexpr size_t kHostPieces = 4;
struct HostCall { hipStream_t hs; Staged d; void* at[kHostPieces]; };
// Everything in front of the device-pointer call.  ws_bytes: the consumer's workspace query (0: it takes no such stack).  The
// pieces lie 16-byte aligned in the pixels slot, in the order given, c->at[i] the i-th; those with an `in` are uploaded.
// entered: the stream of a wrapper that looked for the device first, null: the device is looked for here, behind the refusals.
// frames_late: more frames than bytes are left to the device-pointer call, behind the device.
int consumer_host_stage(const char* fn, int device, hipStream_t entered, const HostStack& s, size_t ws_bytes, bool frames_late,
                        std::initializer_list<HostPiece> pieces, HostCall* c) {
    if (!ws_bytes || (!frames_late && s.n_frames > s.terse_bytes)) return fail(TRPX_ERR_INVALID_ARG, "%s: bad dtype/sizes", fn);
    if (!frame_bits_fit_32(s.dtype, s.n_values, s.block)) return fail(TRPX_ERR_UNSUPPORTED, "%s: frames of >= 2^32 bits", fn);
    if (pieces.size() > kHostPieces) return fail(TRPX_ERR_INVALID_ARG, "%s: more than %zu pieces", fn, kHostPieces);
    c->hs = entered;
    if (!entered)
        if (const int rc = enter(fn, device, &c->hs)) return rc;
    size_t at[kHostPieces + 1] = {0}, n = 0;
    for (const HostPiece& p : pieces) {
        at[n + 1] = trpx::align_up(at[n] + p.bytes, 16);
        ++n;
    }
    if (const int rc = stage(c->hs, s.terse, s.terse_bytes, s.frame_offsets, s.n_frames, s.frame_offsets != nullptr, 0, at[n], ws_bytes, &c->d)) return rc;
    n = 0;
    for (const HostPiece& p : pieces) {
        c->at[n] = static_cast<char*>(c->d.out) + at[n];
        if (p.in) HIP_TRY(copy_sync(c->hs, c->at[n], p.in, p.bytes, hipMemcpyHostToDevice));
        ++n;
    }
    return TRPX_OK;
}
// The whole call: staged as above, call(c) -- the device-pointer entry point on c.d, c.at and c.hs --, the status read back as
// the return code, the pieces with an `out` downloaded.
template <class Call>
int consumer_host(const char* fn, int device, hipStream_t entered, const HostStack& s, size_t ws_bytes, bool frames_late,
                  std::initializer_list<HostPiece> pieces, Call&& call) {
    HostCall c;
    int rc = consumer_host_stage(fn, device, entered, s, ws_bytes, frames_late, pieces, &c);
    if (rc) return rc;
    uint32_t st[TRPX_STATUS_WORDS];
    rc = call(c);
    if (rc || (rc = finish(fn, c.hs, c.d.status, st))) return rc;
    size_t n = 0;
    for (const HostPiece& p : pieces) {
        if (p.out) HIP_TRY(copy_sync(c.hs, p.out, c.at[n], p.bytes, hipMemcpyDeviceToHost));
        ++n;
    }
    return TRPX_OK;
}
}  // namespace
extern "C" {

int trpx_decode_sum_host(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                         size_t n_values, size_t n_frames, unsigned block, unsigned group, void* sums_out, int device) {
    const char* const fn = "trpx_decode_sum_host";
    hipStream_t hs = nullptr;
    if (const int rc = enter(fn, device, &hs)) return rc;                     // (recorded: NO_DEVICE before every other refusal)
    if (const int rc = consumer_host_refusals(fn, terse && sums_out && sum_out_ok(out_dtype) && group, dtype, terse_bytes, n_values, n_frames, block))
        return rc;
    const size_t ws_bytes = trpx_decode_sum_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block, group);
    const size_t out_bytes = (n_frames + group - 1) / group * n_values * sum_out_size(out_dtype);
    return consumer_host(fn, device, hs, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                         {{nullptr, sums_out, out_bytes}}, [&](const HostCall& c) {
        return trpx_decode_sum(dtype, out_dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block, group, c.at[0], c.d.status,
                               c.d.ws, ws_bytes, c.hs);
    });
}

int trpx_decode_roi_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                         size_t n_frames, unsigned block, size_t width, const uint32_t* boxes, size_t n_boxes, unsigned box_h,
                         unsigned box_w, void* pixels_out, int device) {
    const char* const fn = "trpx_decode_roi_host";
    if (const int rc = consumer_host_refusals(fn, terse && boxes && pixels_out, dtype, terse_bytes, n_values, n_frames, block)) return rc;
    if (const int rc = roi_geometry(fn, n_values, width, n_boxes, box_h, box_w)) return rc;
    if ((unsigned __int128)n_boxes * box_h * box_w * trpx_dtype_size(dtype) >= ((unsigned __int128)1 << 62) || n_boxes >= ((size_t)1 << 40))
        return fail(TRPX_ERR_INVALID_ARG, "%s: bad sizes n_boxes=%zu", fn, n_boxes);
    for (size_t i = 0; i < n_boxes; ++i)
        if (boxes[3 * i] >= n_frames || (uint64_t)boxes[3 * i + 1] + box_h > n_values / width || (uint64_t)boxes[3 * i + 2] + box_w > width)
            return fail(TRPX_ERR_INVALID_ARG, "%s: box %zu (frame %u, y0 %u, x0 %u) leaves the stack", fn, i, boxes[3 * i], boxes[3 * i + 1],
                        boxes[3 * i + 2]);
    const size_t ws_bytes = trpx_decode_roi_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block);
    // (recorded: more frames than bytes get as far as the device, and are trpx_decode_roi's to refuse)
    return consumer_host(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, true,
                         {{boxes, nullptr, 12 * n_boxes}, {nullptr, pixels_out, n_boxes * box_h * box_w * trpx_dtype_size(dtype)}},
                         [&](const HostCall& c) {
        return trpx_decode_roi(dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block, width, static_cast<const uint32_t*>(c.at[0]),
                               n_boxes, box_h, box_w, c.at[1], c.d.status, c.d.ws, ws_bytes, c.hs);
    });
}

// (its tail is its own: a capacity too small is an answer, not a failure, and what comes back depends on the total)
int trpx_decode_sparse_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                            size_t n_frames, unsigned block, int64_t threshold, uint64_t* row_offsets, uint32_t* positions,
                            void* values, size_t capacity, size_t* n_found, int device) {
    const char* const fn = "trpx_decode_sparse_host";
    if (const int rc = consumer_host_refusals(fn, terse && row_offsets && n_found, dtype, terse_bytes, n_values, n_frames, block)) return rc;
    const size_t ws_bytes = trpx_decode_sparse_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block);
    if (const int rc = sparse_outputs(fn, positions, values, capacity)) return rc;
    const size_t es = trpx_dtype_size(dtype);
    if ((unsigned __int128)capacity * (4 + es) >= ((unsigned __int128)1 << 62)) return fail(TRPX_ERR_INVALID_ARG, "%s: bad capacity %zu", fn, capacity);
    HostCall c;                                                                // (the stage step downloads nothing: the copies back are below)
    int rc = consumer_host_stage(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                                 {{nullptr, row_offsets, 8 * (n_frames + 1)}, {nullptr, positions, 4 * capacity}, {nullptr, values, es * capacity}}, &c);
    if (rc) return rc;
    uint32_t st[TRPX_STATUS_WORDS];
    rc = trpx_decode_sparse(dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block, threshold, static_cast<uint64_t*>(c.at[0]),
                            positions ? static_cast<uint32_t*>(c.at[1]) : nullptr, positions ? c.at[2] : nullptr, capacity, c.d.status, c.d.ws,
                            ws_bytes, c.hs);
    if (rc || (rc = read_status(c.hs, c.d.status, st))) return rc;
    if (st[0] && st[0] != TRPX_ERR_CAPACITY) return status_result(fn, st);
    HIP_TRY(copy_sync(c.hs, row_offsets, c.at[0], 8 * (n_frames + 1), hipMemcpyDeviceToHost));   // (valid when the capacity is too small, too)
    const size_t total = (size_t)row_offsets[n_frames];
    *n_found = total;
    if (st[0]) return fail(TRPX_ERR_CAPACITY, "%s: %zu events, capacity %zu", fn, total, capacity);
    if (total) {
        HIP_TRY(copy_sync(c.hs, positions, c.at[1], 4 * total, hipMemcpyDeviceToHost));
        HIP_TRY(copy_sync(c.hs, values, c.at[2], es * total, hipMemcpyDeviceToHost));
    }
    return TRPX_OK;
}

int trpx_decode_dot_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                         size_t n_frames, unsigned block, const int32_t* weights, unsigned n_maps, int64_t* dots_out, int device) {
    const char* const fn = "trpx_decode_dot_host";
    if (const int rc = consumer_host_refusals(fn, terse && weights && dots_out && dot_maps_ok(n_maps), dtype, terse_bytes, n_values, n_frames, block))
        return rc;
    const size_t ws_bytes = trpx_decode_dot_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block, n_maps);
    return consumer_host(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                         {{weights, nullptr, 4 * (size_t)n_maps * n_values}, {nullptr, dots_out, 8 * n_frames * (size_t)n_maps}},
                         [&](const HostCall& c) {
        return trpx_decode_dot(dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block, static_cast<const int32_t*>(c.at[0]), n_maps,
                               static_cast<int64_t*>(c.at[1]), c.d.status, c.d.ws, ws_bytes, c.hs);
    });
}

int trpx_decode_bins_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                          size_t n_frames, unsigned block, const uint16_t* labels, unsigned n_bins, int64_t* bins_out, int device) {
    const char* const fn = "trpx_decode_bins_host";
    if (const int rc = consumer_host_refusals(fn, terse && labels && bins_out && bins_count_ok(n_bins), dtype, terse_bytes, n_values, n_frames, block))
        return rc;
    const size_t ws_bytes = trpx_decode_bins_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block, n_bins);
    return consumer_host(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                         {{labels, nullptr, 2 * n_values}, {nullptr, bins_out, 8 * n_frames * (size_t)n_bins}}, [&](const HostCall& c) {
        return trpx_decode_bins(dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block, static_cast<const uint16_t*>(c.at[0]), n_bins,
                                static_cast<int64_t*>(c.at[1]), c.d.status, c.d.ws, ws_bytes, c.hs);
    });
}

int trpx_decode_hist_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                          size_t n_frames, unsigned block, size_t group, int64_t lo, unsigned shift, unsigned n_bins, uint64_t* hist_out,
                          int device) {
    const char* const fn = "trpx_decode_hist_host";
    if (const int rc = consumer_host_refusals(fn, terse && hist_out && group && trpx::hist_args_ok(lo, shift, n_bins), dtype, terse_bytes, n_values,
                                              n_frames, block))
        return rc;
    const size_t ws_bytes = trpx_decode_hist_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block, group, n_bins);
    const size_t frames = std::min(group, n_frames), out_bytes = 8 * ((n_frames + frames - 1) / frames) * (size_t)n_bins;
    return consumer_host(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                         {{nullptr, hist_out, out_bytes}}, [&](const HostCall& c) {
        return trpx_decode_hist(dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block, group, lo, shift, n_bins,
                                static_cast<uint64_t*>(c.at[0]), c.d.status, c.d.ws, ws_bytes, c.hs);
    });
}

int trpx_decode_corrected_host(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                               size_t n_values, size_t n_frames, unsigned block, const float* dark, const float* gain, void* out, int device) {
    const char* const fn = "trpx_decode_corrected_host";
    if (const int rc = consumer_host_refusals(fn, terse && out, dtype, terse_bytes, n_values, n_frames, block)) return rc;
    if (out_dtype != TRPX_F32) return fail(TRPX_ERR_UNSUPPORTED, "%s: out_dtype %d (F32)", fn, out_dtype);
    // (its workspace query answers 0 for such frames as well: asked first, they stay UNSUPPORTED)
    if (!frame_bits_fit_32(dtype, n_values, block)) return fail(TRPX_ERR_UNSUPPORTED, "%s: frames of >= 2^32 bits", fn);
    const size_t ws_bytes = trpx_decode_corrected_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block);
    return consumer_host(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                         {{dark, nullptr, 4 * n_values}, {gain, nullptr, 4 * n_values}, {nullptr, out, 4 * n_frames * n_values}},
                         [&](const HostCall& c) {
        return trpx_decode_corrected(dtype, out_dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block,
                                     dark ? static_cast<const float*>(c.at[0]) : nullptr, gain ? static_cast<const float*>(c.at[1]) : nullptr, c.at[2],
                                     c.d.status, c.d.ws, ws_bytes, c.hs);
    });
}

int trpx_decode_binned_host(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                            size_t n_values, size_t n_frames, unsigned block, size_t width, unsigned bin_y, unsigned bin_x,
                            void* binned_out, int device) {
    const char* const fn = "trpx_decode_binned_host";
    if (const int rc = consumer_host_refusals(fn, terse && binned_out, dtype, terse_bytes, n_values, n_frames, block)) return rc;
    if (const int rc = binned_geometry(fn, dtype, out_dtype, n_values, width, bin_y, bin_x)) return rc;
    const size_t ws_bytes = trpx_decode_binned_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block);
    const size_t out_h = (n_values / width + bin_y - 1) / bin_y, out_w = (width + bin_x - 1) / bin_x;
    return consumer_host(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                         {{nullptr, binned_out, n_frames * out_h * out_w * sum_out_size(out_dtype)}}, [&](const HostCall& c) {
        return trpx_decode_binned(dtype, out_dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block, width, bin_y, bin_x, c.at[0],
                                  c.d.status, c.d.ws, ws_bytes, c.hs);
    });
}

int trpx_decode_reduce_host(int dtype, int op, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                            size_t n_frames, unsigned block, unsigned group, int64_t threshold, void* out, int device) {
    const char* const fn = "trpx_decode_reduce_host";
    if (const int rc = consumer_host_refusals(fn, terse && out && reduce_op_ok(op) && group, dtype, terse_bytes, n_values, n_frames, block)) return rc;
    const size_t ws_bytes = trpx_decode_reduce_workspace_bytes(dtype, op, terse_bytes, n_values, n_frames, block, group);
    const size_t out_bytes = (n_frames + group - 1) / group * n_values * trpx::reduce_out_size(op, trpx_dtype_size(dtype));
    return consumer_host(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                         {{nullptr, out, out_bytes}}, [&](const HostCall& c) {
        return trpx_decode_reduce(dtype, op, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block, group, threshold, c.at[0], c.d.status,
                                  c.d.ws, ws_bytes, c.hs);
    });
}

int trpx_decode_sum_labelled_host(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                                  size_t n_values, size_t n_frames, unsigned block, const uint32_t* labels, size_t n_out, void* sums_out,
                                  uint32_t* counts_out, int device) {
    const char* const fn = "trpx_decode_sum_labelled_host";
    if (const int rc = consumer_host_refusals(fn, terse && labels && sums_out && sum_out_ok(out_dtype) && n_out, dtype, terse_bytes, n_values, n_frames,
                                              block))
        return rc;
    if (!labelled_out_ok(n_out)) return fail(TRPX_ERR_UNSUPPORTED, "%s: n_out=%zu (at most 2^20)", fn, n_out);
    if (trpx_dtype_is_signed(dtype) && (out_dtype == TRPX_U32 || out_dtype == TRPX_U64))
        return fail(TRPX_ERR_UNSUPPORTED, "%s: signed stream into an unsigned output (Terse.hpp:356-357)", fn);
    const size_t ws_bytes = trpx_decode_sum_labelled_workspace_bytes(dtype, terse_bytes, n_values, n_frames, block, n_out);
    // (the counts are made on the device whether the caller wants them or not)
    return consumer_host(fn, device, nullptr, {dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block}, ws_bytes, false,
                         {{labels, nullptr, 4 * n_frames}, {nullptr, sums_out, n_out * n_values * sum_out_size(out_dtype)}, {nullptr, counts_out, 4 * n_out}},
                         [&](const HostCall& c) {
        return trpx_decode_sum_labelled(dtype, out_dtype, c.d.terse, terse_bytes, c.d.offs, nullptr, n_values, n_frames, block,
                                        static_cast<const uint32_t*>(c.at[0]), n_out, c.at[1], static_cast<uint32_t*>(c.at[2]), c.d.status, c.d.ws, ws_bytes,
                                        c.hs);
    });
}

int trpx_encode_sparse_host(int dtype, const uint64_t* row_offsets, const uint32_t* positions, const void* values, size_t n_events,
                            size_t n_values, size_t n_frames, unsigned block, uint8_t* out, size_t out_capacity, size_t* total_bytes,
                            uint64_t* frame_offsets, uint32_t* prolix_bits, int device) {
    // (the argument and event checks need no device: they come first)
    trpx::FrameGeom g;
    const size_t es = trpx_dtype_size(dtype);
    if (!es || !row_offsets || !out || !total_bytes) return fail(TRPX_ERR_INVALID_ARG, "trpx_encode_sparse_host: bad argument");
    if (block != kBlock || is64(dtype)) return fail(TRPX_ERR_UNSUPPORTED, "trpx_encode_sparse_host: block=%u dtype=%d", block, dtype);
    if (n_values >= (1ull << 32)) return fail(TRPX_ERR_UNSUPPORTED, "trpx_encode_sparse_host: n_values=%zu (positions are 32-bit)", n_values);
    if (!geom_of(n_values, block, &g) || !sizes_ok(g, n_frames)) return fail(TRPX_ERR_INVALID_ARG, "trpx_encode_sparse_host: bad sizes");
    if (const int rc = sparse_enc_inputs("trpx_encode_sparse_host", positions, values, n_events)) return rc;
    trpx::SparseStaging in_at;
    if (!trpx::sparse_staging(n_frames, n_events, es, &in_at)) return fail(TRPX_ERR_INVALID_ARG, "trpx_encode_sparse_host: bad n_events %zu", n_events);
    uint64_t bad_frame = 0, bad_event = 0;
    if (const char* why = trpx::bad_events(row_offsets, positions, n_events, n_values, n_frames, &bad_frame, &bad_event))
        return fail(TRPX_ERR_INVALID_ARG, "trpx_encode_sparse_host: %s (frame %llu, event %llu)", why, (unsigned long long)bad_frame,
                    (unsigned long long)bad_event);
    hipStream_t hs = nullptr;
    if (const int rc = enter("trpx_encode_sparse_host", device, &hs)) return rc;
    // the inputs in one device block: [row_offsets] [positions] [values]
    const size_t pos_at = in_at.pos_at, val_at = in_at.val_at;            // (sparse_events.hpp)
    const size_t cap = trpx_encode_sparse_bound_bytes(dtype, n_values, n_frames, n_events, block);
    const size_t ws_bytes = sparse_enc_ws(g, n_frames).total;
    void *d_in = nullptr, *d_out = nullptr, *d_ws = nullptr;
    uint64_t* d_off = nullptr;
    uint32_t* d_st = nullptr;
    Arena& A = arena();
    HIP_TRY(A.get(Arena::kPixels, in_at.total, &d_in));
    HIP_TRY(A.get(Arena::kStream, cap, &d_out));
    HIP_TRY(A.get(Arena::kWorkspace, ws_bytes, &d_ws));
    int rc = upload_offsets(hs, nullptr, n_frames, 0, &d_off);
    if (rc || (rc = status_slot(&d_st))) return rc;
    char* in = static_cast<char*>(d_in);
    HIP_TRY(copy_sync(hs, in, row_offsets, 8 * (n_frames + 1), hipMemcpyHostToDevice));
    if (n_events) {
        HIP_TRY(copy_sync(hs, in + pos_at, positions, 4 * n_events, hipMemcpyHostToDevice));
        HIP_TRY(copy_sync(hs, in + val_at, values, es * n_events, hipMemcpyHostToDevice));
    }
    uint32_t st[TRPX_STATUS_WORDS];
    rc = trpx_encode_sparse(dtype, reinterpret_cast<const uint64_t*>(in), n_events ? reinterpret_cast<const uint32_t*>(in + pos_at) : nullptr,
                            n_events ? in + val_at : nullptr, n_events, n_values, n_frames, block, static_cast<uint8_t*>(d_out), cap, d_off,
                            d_st, d_ws, ws_bytes, hs);
    if (rc || (rc = finish("trpx_encode_sparse_host", hs, d_st, st))) return rc;
    return download_stream("trpx_encode_sparse_host", hs, d_off, d_out, n_frames, st, out, out_capacity, total_bytes, frame_offsets, prolix_bits);
}

int trpx_select_frames_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                            size_t n_frames, unsigned block, const uint32_t* frames, size_t n_select, uint8_t* out, size_t out_capacity,
                            uint64_t* out_offsets, size_t* total_bytes, int device) {
    // (the argument checks and the list's need no device: they come first)
    trpx::FrameGeom g;
    if (!trpx_dtype_size(dtype) || !terse || !frame_offsets || !frames || !out || !total_bytes)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_select_frames_host: bad argument");
    if (!geom_of(n_values, block, &g)) return fail(block == 0 || block > kMaxBlock ? TRPX_ERR_UNSUPPORTED : TRPX_ERR_INVALID_ARG, "trpx_select_frames_host: unsupported sizes/block (block=%u)", block);
    if (!sizes_ok(g, n_frames)) return fail(TRPX_ERR_INVALID_ARG, "trpx_select_frames_host: bad sizes n_values=%zu n_frames=%zu", n_values, n_frames);
    if (const int rc = select_sizes("trpx_select_frames_host", terse_bytes, n_frames, n_select)) return rc;
    uint64_t bad_slot = 0, total = 0;
    if (const uint32_t code = trpx::select_check_list(frames, n_select, frame_offsets, n_frames, terse_bytes, &bad_slot, &total))
        return fail((int)code, code == TRPX_ERR_INVALID_ARG ? "trpx_select_frames_host: entry %llu of the list is not a frame of the stack"
                                                            : "trpx_select_frames_host: the frame of entry %llu has decreasing offsets or leaves the stream",
                    (unsigned long long)bad_slot);
    if (total > out_capacity) return fail(TRPX_ERR_CAPACITY, "trpx_select_frames_host: need %llu bytes, have %zu", (unsigned long long)total, out_capacity);
    hipStream_t hs = nullptr;
    if (const int rc = enter("trpx_select_frames_host", device, &hs)) return rc;
    // the result and the list in one device block: [out] [out_offsets] [frames]
    const size_t cap = trpx::align_up(total, 16), off_at = cap, list_at = off_at + 8 * (n_select + 1);
    const size_t ws_bytes = trpx::select_workspace_bytes(n_select);
    Staged d;
    int rc = stage(hs, terse, terse_bytes, frame_offsets, n_frames, true, 0, list_at + 4 * n_select, ws_bytes, &d);
    if (rc) return rc;
    char* o = static_cast<char*>(d.out);
    HIP_TRY(copy_sync(hs, o + list_at, frames, 4 * n_select, hipMemcpyHostToDevice));
    uint32_t st[TRPX_STATUS_WORDS];
    rc = trpx_select_frames(dtype, d.terse, terse_bytes, d.offs, nullptr, n_values, n_frames, block, reinterpret_cast<const uint32_t*>(o + list_at),
                            n_select, reinterpret_cast<uint8_t*>(o), cap, reinterpret_cast<uint64_t*>(o + off_at), nullptr, d.status, d.ws, ws_bytes, hs);
    if (rc || (rc = finish("trpx_select_frames_host", hs, d.status, st))) return rc;
    if (total) HIP_TRY(copy_sync(hs, out, o, total, hipMemcpyDeviceToHost));
    if (out_offsets) HIP_TRY(copy_sync(hs, out_offsets, o + off_at, 8 * (n_select + 1), hipMemcpyDeviceToHost));
    *total_bytes = total;
    return TRPX_OK;
}

int trpx_group_states_host(const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                           size_t n_frames, unsigned block, unsigned max_bits, uint64_t* group_states, int device) {
    hipStream_t hs = nullptr;
    if (const int rc = enter("trpx_group_states_host", device, &hs)) return rc;
    trpx::FrameGeom g;
    if (!terse || !terse_bytes || !frame_offsets || !group_states || max_bits == 0 || max_bits > 32)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_group_states_host: bad argument");
    if (block != kBlock) return fail(TRPX_ERR_UNSUPPORTED, "trpx_group_states_host: block=%u", block);
    if (!geom_of(n_values, block, &g) || !sizes_ok(g, n_frames) || n_frames > terse_bytes)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_group_states_host: bad sizes");
    const int dtype = max_bits <= 8 ? TRPX_U8 : max_bits <= 16 ? TRPX_U16 : TRPX_U32;
    const size_t ib = trpx_index_bytes(dtype, n_values, n_frames, block), ng = n_frames * (size_t)g.n_tiles;
    Staged d;                                                                  // (the offsets slot: the offsets, then the states; the workspace: the index)
    int rc = stage(hs, terse, terse_bytes, frame_offsets, n_frames, true, 8 * ng, 0, ib, &d);
    if (rc) return rc;
    uint64_t* d_states = d.offs + (n_frames + 1);
    uint32_t st[TRPX_STATUS_WORDS];
    rc = trpx_build_index(dtype, d.terse, terse_bytes, d.offs, n_values, n_frames, block, d.ws, d.status, hs);
    if (rc || (rc = trpx_index_group_states(d.ws, n_values, n_frames, block, d_states, hs)) || (rc = finish("trpx_group_states_host", hs, d.status, st)))
        return rc;
    HIP_TRY(copy_sync(hs, group_states, d_states, 8 * ng, hipMemcpyDeviceToHost));
    return TRPX_OK;
}

int trpx_decode_host_grouped(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                             const uint64_t* group_states, size_t n_values, size_t n_frames, unsigned block, void* pixels_out,
                             int device) {
    // the tuned, walk-free route needs a same-signedness integer type; everything else (and a
    // state table that does not fit the stream) goes the general way
    trpx::FrameGeom g;
    const bool tuned = group_states && frame_offsets && tuned_type(stream_signed, out_dtype) && block == kBlock &&
                       geom_of(n_values, block, &g) && sizes_ok(g, n_frames);
    if (!tuned) return trpx_decode_host(stream_signed, out_dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block, pixels_out, device);
    hipStream_t hs = nullptr;
    if (const int rc = enter("trpx_decode_host_grouped", device, &hs)) return rc;
    if (!terse || !terse_bytes || !pixels_out) return fail(TRPX_ERR_INVALID_ARG, "trpx_decode_host_grouped: bad argument");
    const size_t out_bytes = n_values * n_frames * trpx_dtype_size(out_dtype), ng = n_frames * (size_t)g.n_tiles;
    const size_t ib = trpx_index_bytes(out_dtype, n_values, n_frames, block);
    Staged d;                                                                  // (the offsets slot: the offsets, then the states; the workspace: the index)
    int rc = stage(hs, terse, terse_bytes, frame_offsets, n_frames, true, 8 * ng, out_bytes, ib, &d);
    if (rc) return rc;
    uint64_t* d_states = d.offs + (n_frames + 1);
    HIP_TRY(copy_sync(hs, d_states, group_states, 8 * ng, hipMemcpyHostToDevice));
    uint32_t st[TRPX_STATUS_WORDS];
    bool decoded = false;
    rc = decode_walk_free(stream_signed, out_dtype, d.terse, terse_bytes, d.offs, d_states, n_values, n_frames, block, d.ws, d.out, d.status, hs,
                          false, st, &decoded);
    if (rc) return rc;
    if (!decoded)                      // the states do not describe this stream (or the data are wider than the output type): general route
        return trpx_decode_host(stream_signed, out_dtype, terse, terse_bytes, frame_offsets, n_values, n_frames, block, pixels_out, device);
    if ((rc = status_result("trpx_decode_host_grouped", st))) return rc;
    HIP_TRY(copy_sync(hs, pixels_out, d.out, out_bytes, hipMemcpyDeviceToHost));
    return TRPX_OK;
}

// ---- a compressed stack kept on the device, read frame by frame (src/prolix.cpp:69-92's loop shape) --------------------
struct trpx_stack {
    int device = 0;
    int stream_signed = 0;
    size_t n_values = 0, n_frames = 0, terse_bytes = 0;
    unsigned block = kBlock;
    void* d_terse = nullptr;       // the stack (+ zero tail)
    void* d_offs = nullptr;        // u64[n_frames + 1]
    void* d_status = nullptr;
    void* d_ws = nullptr;
    size_t ws_bytes = 0;
    void* d_states = nullptr;      // u64[n_frames * groups]: chain state at every 256th block (may be absent)
    void* d_index = nullptr;       // decode index of the window's frames, rebuilt from the states (walk-free expansion)
    size_t groups = 0;
    void* d_window = nullptr;      // decoded frames [win_first, win_first + win_count) as win_dtype
    size_t window_cap = 0, win_first = 0, win_count = 0, window_frames = 0;
    int win_dtype = -1;
    std::vector<uint64_t> offs;    // host copy of the frame offsets
};

static void stack_free(trpx_stack* s) {
    if (!s) return;
    for (void* q : {s->d_terse, s->d_offs, s->d_status, s->d_ws, s->d_window, s->d_states, s->d_index}) if (q) (void)hipFree(q);
    delete s;
}

int trpx_stack_open(trpx_stack** handle, int stream_signed, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                    const uint64_t* group_states, size_t n_values, size_t n_frames, unsigned block, unsigned max_bits, int device) {
    if (!handle) return fail(TRPX_ERR_INVALID_ARG, "trpx_stack_open: null handle");
    *handle = nullptr;
    hipStream_t hs = nullptr;                                                  // the calling thread's private stream (see Arena)
    if (const int rc = enter("trpx_stack_open", device, &hs)) return rc;
    trpx::FrameGeom g;
    if (!terse || !terse_bytes || !geom_of(n_values, block, &g) || !sizes_ok(g, n_frames) || n_frames > terse_bytes)
        return fail(TRPX_ERR_INVALID_ARG, "trpx_stack_open: bad argument / sizes");
    std::vector<uint64_t> offs(n_frames + 1);
    if (frame_offsets) {
        memcpy(offs.data(), frame_offsets, 8 * (n_frames + 1));
        if (offs[0] != 0 || offs[n_frames] > terse_bytes) return fail(TRPX_ERR_CORRUPT, "trpx_stack_open: frame offsets do not fit the stack");
        for (size_t f = 0; f < n_frames; ++f)
            if (offs[f + 1] <= offs[f]) return fail(TRPX_ERR_CORRUPT, "trpx_stack_open: frame offsets are not increasing");
    } else if (max_bits > 64) {
        return fail(TRPX_ERR_INVALID_ARG, "trpx_stack_open: max_bits=%u", max_bits);
    }
    trpx_stack* s = new trpx_stack;
    auto bail = [&](hipError_t e, const char* what) { stack_free(s); return fail(TRPX_ERR_HIP, "trpx_stack_open: %s: %s", what, hipGetErrorString(e)); };
    hipError_t e;
    if ((e = hipGetDevice(&s->device)) != hipSuccess) return bail(e, "hipGetDevice");
    s->stream_signed = stream_signed != 0;
    s->n_values = n_values; s->n_frames = n_frames; s->terse_bytes = terse_bytes; s->block = block;
    s->offs.swap(offs);
    const size_t frame_bytes = n_values * 8;                                   // widest output (double)
    s->window_frames = std::max<size_t>(1, std::min<size_t>(n_frames, (size_t(64) << 20) / frame_bytes));   // <= 64 MB of decoded frames
    s->ws_bytes = trpx_decode_workspace_bytes(TRPX_U8, n_values, s->window_frames, block);
    if ((e = hipMalloc(&s->d_terse, padded_stream_bytes(terse_bytes))) != hipSuccess) return bail(e, "hipMalloc(stack)");
    if ((e = hipMalloc(&s->d_offs, 8 * (n_frames + 1))) != hipSuccess) return bail(e, "hipMalloc(offsets)");
    if ((e = hipMalloc(&s->d_status, 4 * TRPX_STATUS_WORDS)) != hipSuccess) return bail(e, "hipMalloc(status)");
    if ((e = hipMalloc(&s->d_ws, s->ws_bytes ? s->ws_bytes : 256)) != hipSuccess) return bail(e, "hipMalloc(workspace)");
    if ((e = copy_stream_zero_tail(hs, s->d_terse, terse, terse_bytes)) != hipSuccess) return bail(e, "upload of the stack");
    if (frame_offsets) {
        if ((e = copy_sync(hs, s->d_offs, s->offs.data(), 8 * (n_frames + 1), hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(offsets)");
    } else {                                                                   // no index: the frames are located on the stack just uploaded
        const size_t lb = trpx::locate_workspace_bytes(g, terse_bytes, n_frames);
        void* d_lws = nullptr;
        if ((e = arena().get(Arena::kWorkspace, lb, &d_lws)) != hipSuccess) return bail(e, "locate workspace");
        uint32_t st[TRPX_STATUS_WORDS];
        int rc = trpx_locate_frames(static_cast<const uint8_t*>(s->d_terse), terse_bytes, n_values, n_frames, block,
                                    max_bits ? max_bits : 32, static_cast<uint64_t*>(s->d_offs),
                                    static_cast<uint32_t*>(s->d_status), d_lws, lb, hs);
        if (rc || (rc = finish("trpx_stack_open", hs, static_cast<uint32_t*>(s->d_status), st))) { stack_free(s); return rc; }
        if ((e = copy_sync(hs, s->offs.data(), s->d_offs, 8 * (n_frames + 1), hipMemcpyDeviceToHost)) != hipSuccess) return bail(e, "hipMemcpy(offsets)");
    }
    if (group_states && block == kBlock) {   // row f1: the file carried its group states
        s->groups = g.n_tiles;
        if ((e = hipMalloc(&s->d_states, 8 * n_frames * s->groups)) != hipSuccess) return bail(e, "hipMalloc(states)");
        if ((e = copy_sync(hs, s->d_states, group_states, 8 * n_frames * s->groups, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(states)");
        if ((e = hipMalloc(&s->d_index, trpx_index_bytes(TRPX_U8, n_values, s->window_frames, block))) != hipSuccess) return bail(e, "hipMalloc(index)");
    }
    *handle = s;
    return TRPX_OK;
}

int trpx_stack_read(trpx_stack* s, size_t frame, int out_dtype, void* pixels_out) {
    if (!s || !pixels_out || frame >= s->n_frames) return fail(TRPX_ERR_INVALID_ARG, "trpx_stack_read: bad argument");
    const size_t es = convert_elem_size(out_dtype);
    if (!es) return fail(TRPX_ERR_INVALID_ARG, "trpx_stack_read: unknown dtype %d", out_dtype);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t hs = nullptr;                                                  // the calling thread's private stream
    HIP_TRY(arena().get_stream(&hs));
    if (out_dtype != s->win_dtype || frame < s->win_first || frame >= s->win_first + s->win_count) {
        // a miss: expand the window of frames that starts here (the callers of the reference walk the stack in order)
        const size_t count = std::min(s->window_frames, s->n_frames - frame);
        const size_t need = count * s->n_values * es;
        if (s->window_cap < need) {
            if (s->d_window) (void)hipFree(s->d_window);
            s->d_window = nullptr; s->window_cap = 0;
            HIP_TRY(hipMalloc(&s->d_window, need));
            s->window_cap = need;
        }
        s->win_count = 0;
        const uint64_t first_byte = s->offs[frame] & ~uint64_t(3);            // trpx_decode wants a 4-byte aligned stream
        const uint8_t* base = static_cast<const uint8_t*>(s->d_terse) + first_byte;
        uint64_t* d_offs = static_cast<uint64_t*>(s->d_offs);
        uint32_t* d_st = static_cast<uint32_t*>(s->d_status);
        std::vector<uint64_t> rel(count + 1);
        for (size_t i = 0; i <= count; ++i) rel[i] = s->offs[frame + i] - first_byte;
        HIP_TRY(copy_sync(hs, d_offs, rel.data(), 8 * (count + 1), hipMemcpyHostToDevice));
        const size_t bytes = (size_t)rel[count];
        uint32_t st[TRPX_STATUS_WORDS];
        bool done = false;
        if (s->d_states && tuned_type(s->stream_signed, out_dtype)) {          // walk-free: index from the file's group states
            if (const int rc = decode_walk_free(s->stream_signed, out_dtype, base, bytes, d_offs, static_cast<const uint64_t*>(s->d_states) + frame * s->groups,
                                                s->n_values, count, s->block, s->d_index, s->d_window, d_st, hs, true, st, &done))
                return rc;
            done = done && st[0] == 0;                                         // (states that do not fit the stream: the general route decides)
        }
        if (!done)
            if (const int rc = decode_any(s->stream_signed, out_dtype, base, bytes, d_offs, s->n_values, count, s->block, s->d_window, d_st,
                                          s->d_ws, s->ws_bytes, hs, st))
                return rc;
        if (const int rc = status_result("trpx_stack_read", st)) return rc;
        s->win_first = frame; s->win_count = count; s->win_dtype = out_dtype;
    }
    const size_t fb = s->n_values * es;
    HIP_TRY(copy_sync(hs, pixels_out, static_cast<const char*>(s->d_window) + (frame - s->win_first) * fb, fb, hipMemcpyDeviceToHost));
    return TRPX_OK;
}

void trpx_stack_close(trpx_stack* s) {
    if (s) { (void)hipSetDevice(s->device); stack_free(s); }
}

}  // extern "C"
