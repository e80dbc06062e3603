// The decode routes as decode_plan.hpp names them, on a CPU under ASan + UBSan: every row is a stack, an entry
// point and a selector, and the plan it must get.  The part counts stand in for what the kernel files' host functions answer:
// frames of more than 32 K blocks have kRound4 / kChain parts unless the many-frames rule keeps them whole.
#include <stdio.h>

#include "decode_plan.hpp"

using namespace trpx;

namespace {
constexpr uint32_t kRound4 = 22, kChain = 31;
int g_failed = 0;

PlanInput stack(Entry entry, size_t es, uint64_t n_values, uint64_t n_frames, int route = kRouteAuto, bool whole_frames = false) {
    PlanInput in;
    in.entry = entry;
    in.route = route;
    in.elem_size = es;
    in.n_blocks = (n_values + 11) / 12;
    in.n_frames = n_frames;
    in.frame_bits = 8 * (n_values * es + (12 * in.n_blocks + 7) / 8 + 1);
    in.frames_misaligned = (n_values * es) % 128 != 0;
    const bool large = in.n_blocks > 32768 && !whole_frames;
    in.parts_per_frame = large ? kRound4 : 1;
    in.chain_parts_per_frame = large ? kChain : 1;
    in.seg_single_wave = !large;
    return in;
}
struct Want {
    Walk walk; Extract extract; uint32_t parts = 1;
    bool narrow = false, misaligned = false, defer = false, listed_tiles = false, locate = false;
};
void expect(const char* what, const PlanInput& in, const Want& w, unsigned scratch) {
    const DecodePlan p = plan_decode(in);
    const bool ok = p.walk == w.walk && p.extract == w.extract && p.parts_per_frame == w.parts && p.narrow == w.narrow &&
                    p.misaligned == w.misaligned && p.defer == w.defer && p.listed_tiles == w.listed_tiles && p.locate == w.locate &&
                    plan_scratch(p) == scratch;
    if (!ok) {
        ++g_failed;
        printf("FAIL %s: walk %d extract %d parts %u narrow %d misaligned %d defer %d listed_tiles %d locate %d scratch %u\n", what, (int)p.walk,
               (int)p.extract, p.parts_per_frame, p.narrow, p.misaligned, p.defer, p.listed_tiles, p.locate, plan_scratch(p));
    }
}
void expect_true(const char* what, bool ok) {
    if (!ok) { ++g_failed; printf("FAIL %s\n", what); }
}
}  // namespace

int main() {
    constexpr uint64_t small = 64 * 64, odd = 65 * 63, mid = 1030 * 1065, big = 2048 * 2048;
    const Want per_frame{Walk::kNone, Extract::kFrames, 1, false, false, true};
    const Want chain_u16{Walk::kChain, Extract::kChainTiles, kChain, true, false, true, true};
    const Want basic{Walk::kHeaders, Extract::kBasic}, serial{Walk::kSerial, Extract::kBasic};

    // ---- trpx_decode ----
    expect("decode 4 x 64^2", stack(Entry::kDecode, 2, small, 4), per_frame, kSeg | kDefer);
    expect("decode 4 x 65.63", stack(Entry::kDecode, 2, odd, 4), {Walk::kNone, Extract::kFrames, 1, false, true, true}, kSeg | kDefer);
    {
        PlanInput in = stack(Entry::kDecode, 2, small, 4);
        in.out_misaligned = true;
        expect("decode 4 x 64^2 into a misaligned buffer", in, {Walk::kNone, Extract::kFrames, 1, false, true, true}, kSeg | kDefer);
        in.out_misaligned = false;
        in.no_defer = true;
        expect("decode 4 x 64^2, no hand-over", in, {Walk::kNone, Extract::kFrames}, 0);
    }
    expect("decode 3 x mid u16", stack(Entry::kDecode, 2, mid, 3), chain_u16, kSeg | kDefer | kParts);
    expect("decode 3 x mid i32", stack(Entry::kDecode, 4, mid, 3), {Walk::kChain, Extract::kChainTiles, kChain, false, false, true, true}, kSeg | kDefer | kParts);
    expect("decode 1 x 2048^2 u16", stack(Entry::kDecode, 2, big, 1), {Walk::kChain, Extract::kChainUnits, kChain, true, false, true, true}, kSeg | kDefer | kParts);
    expect("decode 1 x 2048^2 i32", stack(Entry::kDecode, 4, big, 1), {Walk::kChain, Extract::kChainTiles, kChain, false, false, true, true}, kSeg | kDefer | kParts);
    expect("decode 3 x mid u16, parts", stack(Entry::kDecode, 2, mid, 3, kRouteParts), {Walk::kNone, Extract::kParts, kRound4, false, false, true, true}, kSeg | kDefer | kParts);
    expect("decode 3 x mid u16, tiled", stack(Entry::kDecode, 2, mid, 3, kRouteTiled), {Walk::kSeg, Extract::kTiled, kRound4}, kSeg | kParts);
    expect("decode 4 x 64^2, tiled", stack(Entry::kDecode, 2, small, 4, kRouteTiled), {Walk::kSeg, Extract::kTiled}, kSeg);
    expect("decode 3 x mid u16, frames", stack(Entry::kDecode, 2, mid, 3, kRouteFrames), chain_u16, kSeg | kDefer | kParts);
    expect("decode 4 x 64^2, frames", stack(Entry::kDecode, 2, small, 4, kRouteFrames), per_frame, kSeg | kDefer);
    {
        PlanInput in = stack(Entry::kDecode, 2, mid, 3);
        in.n_frames = 0x7FFFFFFFull / kChain + 1;                             // (more parts than a grid holds: the frames stay whole)
        expect("decode, too many parts", in, {Walk::kSeg, Extract::kTiled}, kSeg);
        in = stack(Entry::kDecode, 2, mid, 3);
        in.chain_extract = 0;
        Want w = chain_u16;
        w.extract = Extract::kChainUnits;
        expect("decode 3 x mid u16, units build", in, w, kSeg | kDefer | kParts);
        in = stack(Entry::kDecode, 4, mid, 3);
        in.chain_extract = 0;
        expect("decode 3 x mid i32, units build", in, {Walk::kChain, Extract::kChainUnits, kChain, false, false, true, true}, kSeg | kDefer | kParts);
        in = stack(Entry::kDecode, 2, big, 1);
        in.chain_extract = 1;
        expect("decode 1 x 2048^2 u16, tiles build", in, chain_u16, kSeg | kDefer | kParts);
    }
    // basic: asked for, or another block size, or no offsets and no locator
    expect("decode basic", stack(Entry::kDecode, 2, small, 4, kRouteBasic), basic, 0);
    {
        PlanInput in = stack(Entry::kDecode, 2, small, 4);
        in.block = 13;
        expect("decode block 13", in, basic, 0);
        in.have_offsets = false;
        in.locate_parallel = in.locate_fits = true;
        expect("decode block 13, no offsets", in, serial, 0);
        in = stack(Entry::kDecode, 2, small, 3);
        in.have_offsets = false;
        expect("decode 3 frames, no offsets, no locator", in, serial, 0);
        in.locate_parallel = true;
        expect("decode, no offsets, the locator's scratch does not fit", in, serial, 0);
        in.route = kRouteBasic;
        in.locate_fits = true;
        expect("decode basic, no offsets", in, serial, 0);
        in = stack(Entry::kDecode, 2, 512 * 512, 8);
        in.have_offsets = false;
        in.locate_parallel = in.locate_fits = true;
        Want w = per_frame;
        w.locate = true;
        expect("decode 8 x 512^2, located", in, w, kSeg | kDefer);
        in = stack(Entry::kDecode, 4, uint64_t(1) << 28, 1);                  // frames of >= 2^32 bits
        expect("decode, frame bits beyond 32", in, basic, 0);
    }
    expect("decode into u64", stack(Entry::kDecode, 8, small, 4), {Walk::kHeaders, Extract::kConvert}, 0);
    {
        PlanInput in = stack(Entry::kConvert, 4, mid, 3);
        expect("convert", in, {Walk::kHeaders, Extract::kConvert}, 0);
        in.have_offsets = false;
        expect("convert, no offsets", in, {Walk::kSerial, Extract::kConvert}, 0);
    }
    // the many-frames rule keeps frames of up to 2^20 blocks whole: per frame below 2^26 bits, tiled above
    expect("decode 768 x 640^2, whole", stack(Entry::kDecode, 2, 640 * 640, 768, kRouteAuto, true), per_frame, kSeg | kDefer);
    expect("decode 768 x 2048^2, whole", stack(Entry::kDecode, 2, big, 768, kRouteAuto, true), {Walk::kSeg, Extract::kTiled}, kSeg);

    // ---- build_index_impl ----
    const Want idx_frames{Walk::kFrames, Extract::kNone}, idx_seg{Walk::kSeg, Extract::kNone};
    expect("index small", stack(Entry::kBuildIndex, 2, small, 4), idx_frames, kSeg | kDefer);
    expect("index small, tiled", stack(Entry::kBuildIndex, 2, small, 4, kRouteTiled), idx_seg, kSeg);
    expect("index large", stack(Entry::kBuildIndex, 2, mid, 3), {Walk::kChain, Extract::kNone, kChain}, kSeg | kDefer | kParts);
    expect("index large i32", stack(Entry::kBuildIndex, 4, mid, 3), {Walk::kChain, Extract::kNone, kChain}, kSeg | kDefer | kParts);
    expect("index large, tiled", stack(Entry::kBuildIndex, 2, mid, 3, kRouteTiled), idx_seg, kSeg);
    // (round 4's parts route forced: no chain, and frames of < 2^26 bits go to the per-frame walker whatever their block count)
    expect("index large, parts", stack(Entry::kBuildIndex, 2, mid, 3, kRouteParts), idx_frames, kSeg | kDefer);
    expect("index 2048^2 i32, parts", stack(Entry::kBuildIndex, 4, big, 1, kRouteParts), idx_seg, kSeg);
    {
        PlanInput in = stack(Entry::kBuildIndex, 2, mid, 3);
        in.lds_walk = true;
        expect("index large, lds walk", in, {Walk::kLds, Extract::kNone}, 0);
        in = stack(Entry::kBuildIndex, 2, small, 4);
        DecodePlan p = plan_decode(in);                                       // trpx_build_index, roi, sparse
        expect_true("index: check on, status cleared", p.check_index && p.clear_status && !p.dense);
        in.check_index = false;                                               // sum; the two-pass encoder's own stream
        in.keep_status = true;
        in.dense = true;
        p = plan_decode(in);
        expect_true("index: check off, status kept", !p.check_index && !p.clear_status && p.dense);
    }

    // ---- trpx_decode_indexed ----
    const Want idx_per_frame{Walk::kCallers, Extract::kFramesIndexed}, idx_tiled{Walk::kCallers, Extract::kTiled};
    const Want walker{Walk::kCallers, Extract::kFrames, 1, false, true, true};
    expect("indexed 1024 x 64^2", stack(Entry::kIndexed, 2, small, 1024), idx_per_frame, 0);
    expect("indexed 1023 x 64^2", stack(Entry::kIndexed, 2, small, 1023), idx_tiled, 0);
    expect("indexed 1023 x 64^2, frames", stack(Entry::kIndexed, 2, small, 1023, kRouteFrames), idx_per_frame, 0);
    expect("indexed 1024 x 64^2, tiled", stack(Entry::kIndexed, 2, small, 1024, kRouteTiled), idx_tiled, 0);
    expect("indexed 1024 x 65.63", stack(Entry::kIndexed, 2, odd, 1024), walker, 0);
    for (int route = kRouteBasic; route <= kRouteParts; ++route)
        expect("indexed 1024 x 65.63, forced", stack(Entry::kIndexed, 2, odd, 1024, route), route == kRouteTiled ? idx_tiled : idx_per_frame, 0);
    {
        PlanInput in = stack(Entry::kIndexed, 2, odd, 1024);
        in.indexed_scratch = false;
        expect("indexed 1024 x 65.63, no scratch", in, idx_per_frame, 0);
        in = stack(Entry::kIndexed, 2, small, 1024);
        in.out_misaligned = true;
        expect("indexed 1024 x 64^2 into a misaligned buffer", in, walker, 0);
        in = stack(Entry::kIndexed, 2, big, 1);
        in.indexed_large_tiles = true;
        expect("indexed 1 x 2048^2 u16, tiles build", in, idx_tiled, 0);
    }
    expect("indexed 1 x 2048^2 u16", stack(Entry::kIndexed, 2, big, 1), {Walk::kCallers, Extract::kUnitsIndexed}, 0);
    expect("indexed 1 x 2048^2 i32", stack(Entry::kIndexed, 4, big, 1), idx_tiled, 0);

    // ---- trpx_decode_parts_per_frame: the rule's count, with the forced tiled route read as auto and no grid limit ----
    expect_true("parts query auto", plan_parts_query(stack(Entry::kDecode, 2, mid, 3)) == kChain);
    expect_true("parts query tiled", plan_parts_query(stack(Entry::kDecode, 2, mid, 3, kRouteTiled)) == kChain);
    expect_true("parts query parts", plan_parts_query(stack(Entry::kDecode, 2, mid, 3, kRouteParts)) == kRound4);
    expect_true("parts query small", plan_parts_query(stack(Entry::kDecode, 2, small, 4)) == 1);
    expect_true("parts query beyond 32 bits", plan_parts_query(stack(Entry::kDecode, 4, uint64_t(1) << 28, 1)) == kRound4);

    if (g_failed) return 1;
    puts("OK decode plan");
    return 0;
}
