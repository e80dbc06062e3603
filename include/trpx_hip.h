/*
 * trpx_hip.h -- C ABI of libtrpx_hip.so: the MI355X (gfx950) implementation of the
 * TERSE encode / PROLIX decode hot path of senikm/trpx.
 *
 * The reference has no FFI/plugin boundary: the hot path is the two inline bodies
 * jpa::Terse::f_compress (include/Terse.hpp:500-549) and jpa::Terse::prolix(Iterator, frame)
 * (include/Terse.hpp:352-389) plus the Bit_pointer.hpp primitives they use.  This header is
 * the boundary a maintainer would bind instead (INTEGRATION.md shows the binding).  Plain
 * pointers and sizes only, no C++/torch types, no exceptions across the boundary.
 *
 * Conventions
 *   - every function returning int returns TRPX_OK (0) or a trpx_status error code;
 *     trpx_last_error_string() gives the thread's last error text.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - functions taking DEVICE pointers only enqueue work on `stream`: no allocation, no
 *     host synchronisation (they can be captured into a hipGraph); the caller supplies the
 *     workspace.  The *_host convenience entry points own their staging and synchronise.
 *   - the bitstream is bit-identical to the reference's: a stack is the
 *     plain concatenation of its frames, frame k starting at byte frame_offsets[k]
 *     (Terse.hpp:502-504; the intended semantics of Terse.hpp:562-585).
 */
#ifndef TRPX_HIP_H
#define TRPX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: the opaque decode index / workspace layouts grew (hand-over list with its statistics, part table); trpx_bench_stream.
 * A caller compiled against one version must not run against a library of another: size its buffers with THIS library's
 * trpx_index_bytes / trpx_*_workspace_bytes and compare trpx_abi_version() with TRPX_ABI_VERSION first (the Terse classes do). */
#define TRPX_ABI_VERSION 3

typedef enum trpx_status {
    TRPX_OK = 0,
    TRPX_ERR_INVALID_ARG = 1,   /* null/misaligned pointer, zero sizes, unknown dtype        */
    TRPX_ERR_UNSUPPORTED = 2,   /* block outside 1..4096, decode index with block != 12, ...   */
    TRPX_ERR_CAPACITY = 3,      /* output or workspace too small                              */
    TRPX_ERR_HIP = 4,           /* a HIP runtime call failed (text has the HIP error)         */
    TRPX_ERR_CORRUPT = 5,       /* bitstream runs past its frame / buffer; also a VALID stream with
                                   RESTATED widths on the device entry points named below      */
    TRPX_ERR_NO_DEVICE = 6,     /* no gfx950 device visible                                   */
    TRPX_ERR_TIMEOUT = 7        /* single-pass encoder: a bounded inter-workgroup wait expired;
                                   re-issue through the two-pass pipeline (trpx_set_encode_path) */
} trpx_status;

/* Restated widths.  The decoder grammar (Terse.hpp:360-372) also accepts an explicit header -- flag 0 + the width code -- for a
 * block whose width equals the one before ("restated"), and widths larger than the values need ("padded").  No encoder here
 * writes either; files of another TERSE writer may hold them.  Padded widths decode everywhere.  A decode index describes a
 * stream by its widths alone (one header bit where a width repeats), so it cannot describe a restated width:
 *   - trpx_build_index and trpx_index_from_group_states report such a stream as TRPX_ERR_CORRUPT (every index they leave has
 *     been compared with the stream's headers block by block), and so do trpx_decode_sum, trpx_decode_roi,
 *     trpx_decode_sparse, trpx_decode_dot, trpx_decode_bins, trpx_decode_binned, trpx_decode_reduce,
 *     trpx_decode_sum_labelled, trpx_decode_hist and trpx_decode_corrected where they build the index themselves (no index
 *     given) -- and their _host forms;
 *   - trpx_decode: the basic route (trpx_set_decode_path(1)) decodes it, and so does every route for 64-bit containers; on
 *     the other routes a frame the per-frame decoder extracts from its own walk is decoded, a frame that goes through a
 *     decode index (header-dense frames, frames of more than 32 K blocks, the tiled route) is TRPX_ERR_CORRUPT;
 *   - trpx_decode_convert and trpx_locate_frames handle it like any other stream;
 *   - the host entry points that stand in for the reference class -- trpx_decode_host, trpx_decode_host_grouped,
 *     trpx_stack_read, the Terse classes' prolix -- decode it: where the tuned route reports CORRUPT they go on to the
 *     converting decoder.
 * Status 0 with pixels that are not the stream's is never an outcome (tests/test_gpu_noncanonical.py). */

/* Pixel types = the reference CLI's dispatch set (src/terse.cpp:113-118). Odd = signed. */
typedef enum trpx_dtype {
    TRPX_U8 = 0, TRPX_I8 = 1, TRPX_U16 = 2, TRPX_I16 = 3, TRPX_U32 = 4, TRPX_I32 = 5,
    TRPX_F32 = 6, TRPX_F64 = 7,     /* output types of trpx_decode_convert / trpx_decode_host only */
    TRPX_U64 = 8, TRPX_I64 = 9      /* 64-bit containers (what src/terse.cpp:120-123 makes of float / double images; Terse.hpp:249
                                     * takes any integral type): correct-first generic kernels, fields of up to 64 bits, no decode
                                     * index; as an output type: values of narrower streams widened, wider ones clamped */
} trpx_dtype;

/* Device status block written by the kernels (u32 words); zeroed by each call's first node. */
enum { TRPX_STATUS_WORDS = 8 };
/*   word 0: 0 = ok, else a trpx_status (CAPACITY / CORRUPT) detected on the device
 *   word 1: prolix_bits of this call (max significant bits over all blocks, Terse.hpp:516)   */

/* Size limits of one call.  A frame is cut into tiles of 256 blocks (3072 values at block 12): tiles = ceil(ceil(n_values /
 * block) / 256).  Every device entry point takes
 *   - n_frames * tiles <= TRPX_MAX_TILES_PER_CALL = 2^24 - 1: the hot kernels start one workgroup of 256 threads per tile, or one
 *     wavefront per frame, and the device launches no grid of 2^32 threads or more.  That is 195 083 frames of 512 x 512
 *     (51 G values), but only 16 777 215 frames of a single tile.  A larger stack is TRPX_ERR_UNSUPPORTED, decided before the
 *     first device call, never a TRPX_ERR_HIP of a launch: split the stack (frames are independent; trpx_select_frames moves
 *     bytes only and is under the same limit for its source);
 *   - n_values * n_frames * 8 < 2^62 bytes and at most 2^32 - 1 blocks a frame (otherwise TRPX_ERR_INVALID_ARG);
 *   - a frame whose worst case is 0xF0000000 bits or more (about 122 M values of 32 bits) decodes and encodes, on the routes
 *     that need no 32-bit position inside the frame; trpx_build_index and the consumers of a decode index (trpx_decode_sum ..
 *     trpx_decode_sum_labelled) answer TRPX_ERR_UNSUPPORTED.
 * The host entry points (_host) pass a stack to the device entry points and answer what those answer. */
#define TRPX_MAX_TILES_PER_CALL 0xFFFFFFu

int         trpx_abi_version(void);
const char* trpx_last_error_string(void);
size_t      trpx_dtype_size(int dtype);          /* 0 for an unknown dtype */
int         trpx_dtype_is_signed(int dtype);
int         trpx_device_count(void);             /* gfx950 devices visible to HIP; 0 = none   */

/*
 * Bytes that can hold ANY encoding of one frame: N*sizeof(T) + ceil(12*nblocks/8) + 1.
 * Replaces the (slightly short) bound of Terse.hpp:503.  Pure arithmetic.
 */
size_t trpx_worst_case_bytes(int dtype, size_t n_values, unsigned block);

/* Workspace sizes (bytes) for the device entry points below.  Pure arithmetic. */
size_t trpx_encode_workspace_bytes(int dtype, size_t n_values, size_t n_frames, unsigned block);
size_t trpx_decode_workspace_bytes(int dtype, size_t n_values, size_t n_frames, unsigned block);
/* How many parts trpx_decode cuts a frame of this geometry into on the current route (1: frames are not cut; large frames --
 * more than 32 K blocks -- are: Terse.hpp:360-372's serial chain is walked as many short chains, decode_part.hip).  For tests
 * and diagnostics; pure arithmetic. */
unsigned trpx_decode_parts_per_frame(int dtype, size_t n_values, size_t n_frames, unsigned block);

/*
 * Encode n_frames frames of n_values pixels each (contiguous, frame-major, DEVICE memory) into
 * one compact stack.  Replaces jpa::Terse::f_compress called once per frame from the ctor /
 * push_back (Terse.hpp:263-270, :290-302, :500-549) and the Bit_range::append_range /
 * operator|= / Bit::set primitives under it (Bit_pointer.hpp:700-730, :628-649, :490).
 *
 *   pixels        DEVICE  const T[n_frames * n_values], aligned to T (16-byte aligned with n_values % 4 == 0 is the fastest case:
 *                           every vector access then stays inside aligned lines; any n_values runs on the same kernels)
 *   out           DEVICE  uint8_t[out_capacity], 16-byte aligned; receives sum(S_f) bytes
 *   frame_offsets DEVICE  uint64_t[n_frames + 1]; [k] = first byte of frame k, [n_frames] = total
 *   status        DEVICE  uint32_t[TRPX_STATUS_WORDS], 8-byte aligned (see above); word 1 = prolix_bits
 *   workspace     DEVICE  >= trpx_encode_workspace_bytes(...), 16-byte aligned
 *
 * If the stack does not fit out_capacity, frame_offsets is still valid, status[0] =
 * TRPX_ERR_CAPACITY and the contents of out[0 .. out_capacity) are unspecified (nothing beyond
 * out_capacity is ever touched; sizes-only query: pass out = NULL, out_capacity = 0).
 * Bytes [total, align_up(total, 4)) of `out` are zeroed (stores are dword granular).
 */
int trpx_encode(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block,
                uint8_t* out, size_t out_capacity, uint64_t* frame_offsets, uint32_t* status,
                void* workspace, size_t workspace_bytes, void* stream);

/*
 * Decode n_frames frames.  Replaces jpa::Terse::prolix(Iterator, frame) (Terse.hpp:352-389),
 * f_find_terse_frame (Terse.hpp:562-585, intended semantics: offset_k = sum of S_j, j < k) and
 * Bit_range::get_range / operator T() (Bit_pointer.hpp:742-792, :597-617).
 *
 *   stream_signed  the header's `signed` attribute; must equal trpx_dtype_is_signed(out_dtype)
 *                  (same-type decode is the reference's contract)
 *   terse          DEVICE const uint8_t[terse_bytes], 4-byte aligned
 *   frame_offsets  DEVICE const uint64_t[n_frames + 1], or NULL: the frames are then located on the device
 *                  (the .trpx format stores no index), see below
 *   pixels_out     DEVICE T[n_frames * n_values], aligned to T (16-byte aligned with n_values % 4 == 0: the fastest case)
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS]; word 0 = TRPX_ERR_CORRUPT if a frame's
 *                  bits run past its end (the reference does not check; we do), and for a valid stream with restated widths
 *                  in a frame that is decoded through block widths ("Restated widths" above; the basic route decodes it)
 * frame_offsets = NULL (an index-free stack, a .trpx file): where trpx_locate_frames takes its position-parallel route (block
 * 12, pixels of up to 32 bits, 4 frames and 8 KB and more, not TRPX_LOCATE_PATH=serial / TRPX_DECODE_PATH=basic) and its
 * workspace fits behind the offsets in this call's workspace, the frames are located that way and then decoded by the same
 * routes as with offsets given (trpx_decode_workspace_bytes does not change); otherwise by one serial walk over the whole
 * stack and the basic kernels.  Offsets, status and pixels are the same either way.  Callers that keep the offsets call
 * trpx_locate_frames and decode with what it wrote.
 */
int trpx_decode(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                const uint64_t* frame_offsets, size_t n_values, size_t n_frames, unsigned block,
                void* pixels_out, uint32_t* status, void* workspace, size_t workspace_bytes,
                void* stream);

/*
 * Converting decode: the output type is free and the stream's signedness is given separately.  Replaces the
 * cross-type branches of jpa::Terse::prolix / Bit_range::get_range: narrower integral output clamps to
 * numeric_limits (Bit_pointer.hpp:747-763), float / double output is exact (Terse.hpp:379-383,
 * Bit_range::next :580-587), wider integral output keeps the value -- also for an unsigned stream into a
 * signed type, where the reference sign-extends wrongly.  out_dtype: TRPX_U8 .. TRPX_F64;
 * workspace: trpx_decode_workspace_bytes().  Correct-first kernels (one lane per block).
 * trpx_decode_host picks this path by itself when out_dtype does not match the stream's signedness or is a
 * floating-point type.
 */
int trpx_decode_convert(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                        const uint64_t* frame_offsets, size_t n_values, size_t n_frames, unsigned block,
                        void* pixels_out, uint32_t* status, void* workspace, size_t workspace_bytes,
                        void* stream);

/*
 * Decode index.  The .trpx stream stores no index, so a plain trpx_decode first walks
 * every frame's header chain (serial per frame, Terse.hpp:360-372).  An encoder that is about to decode its
 * own stack again -- or a reader that decodes a stack more than once -- can keep what that walk produces:
 * width[b] (1 byte per block) and the bit offset of every 256-block group.  The index is an opaque DEVICE
 * buffer of trpx_index_bytes(); it is NOT part of the bitstream (files stay byte-identical).
 *   trpx_encode_indexed   = trpx_encode that also fills `index` (index == NULL: plain trpx_encode)
 *   trpx_build_index      fills `index` from an existing stack (the walk alone), and compares it with the stream's headers
 *                           block by block: a valid stream with restated widths ("Restated widths" above) has no index,
 *                           status[0] = TRPX_ERR_CORRUPT (trpx_index_from_group_states: the same)
 *   trpx_decode_indexed   = trpx_decode without the walk; the index is validated against the frame sizes
 *                           (inconsistent -> status[0] = TRPX_ERR_CORRUPT), frame_offsets is mandatory.
 *                           Stacks of >= 1024 small frames that start inside a 128-byte line (pixel bytes per frame no
 *                           multiple of 128) take the walking decoder, whose stores are line images, and only the
 *                           header-dense frames it hands over are extracted through the index -- never slower than
 *                           trpx_decode.  That needs a few KB for the hand-over list: one grow-only device buffer per
 *                           calling thread, device and stream, allocated at the first such call (a call that is being
 *                           captured into a graph takes the plain indexed route and allocates nothing).
 */
size_t trpx_index_bytes(int dtype, size_t n_values, size_t n_frames, unsigned block);
int trpx_encode_indexed(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block,
                        uint8_t* out, size_t out_capacity, uint64_t* frame_offsets, uint32_t* status,
                        void* index, void* workspace, size_t workspace_bytes, void* stream);
int trpx_build_index(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                     size_t n_values, size_t n_frames, unsigned block, void* index, uint32_t* status,
                     void* stream);
int trpx_decode_indexed(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                        const uint64_t* frame_offsets, const void* index, size_t n_values, size_t n_frames,
                        unsigned block, void* pixels_out, uint32_t* status, void* stream);

/*
 * Host-pointer convenience wrappers (what the C++ trpx::Terse class calls): allocate device
 * staging, copy in, run the device entry point, copy out, synchronise.  `out` must hold
 * n_frames * trpx_worst_case_bytes(); *total_bytes receives sum(S_f); frame_offsets (host,
 * n_frames + 1) and prolix_bits may be NULL.  device < 0 keeps the current HIP device.
 */
int trpx_encode_host(int dtype, const void* pixels, size_t n_values, size_t n_frames,
                     unsigned block, uint8_t* out, size_t out_capacity, size_t* total_bytes,
                     uint64_t* frame_offsets, uint32_t* prolix_bits, int device);
int trpx_decode_host(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                     const uint64_t* frame_offsets, size_t n_values, size_t n_frames,
                     unsigned block, void* pixels_out, int device);

/*
 * Locate the frames of a stack that comes without an index (a .trpx file): trpx_locate_frames on a device copy of the
 * stack, the intended semantics of jpa::Terse::f_find_terse_frame (Terse.hpp:562-585).
 * frame_offsets: HOST uint64_t[n_frames + 1].  max_bits = widest legal block (8, 16 or 32).
 */
int trpx_frame_offsets_host(const uint8_t* terse, size_t terse_bytes, size_t n_values, size_t n_frames,
                            unsigned block, unsigned max_bits, uint64_t* frame_offsets, int device);

/*
 * Locate the frames of an index-free stack on the device: frame_offsets[k] = first byte of frame k, [n_frames] = end of the
 * last frame asked for -- the intended semantics of Terse.hpp:562-585, the offsets trpx_decode's own walk finds.  For callers
 * whose stack is already in device memory (a torch pipeline, trpx_decode_sharded's global table, a graph capture).  Block 12
 * with max_bits <= 32, from 4 frames and 8 KB on: position-parallel (decode_locate.hip: header chains of fixed chunks of the
 * stack with checkpoints and links, one wavefront that resolves each frame's end by block counts along them, a parallel
 * verification of every frame by the serial walk, and that serial walk from the first frame that fails verification on,
 * decided on the device) -- the offsets and the status are the serial walk's in every case.  Otherwise, or after
 * trpx_set_locate_path(1) / TRPX_LOCATE_PATH=serial: the frames are walked one after another by one wavefront (the
 * run-skipping header walk of trpx_decode's own serial walk, count only).  Any block size, max_bits up to 64.
 *   terse          DEVICE const uint8_t[terse_bytes], 4-byte aligned
 *   max_bits       widest legal block: 8, 16, 32 or 64 by the pixel type
 *   frame_offsets  DEVICE uint64_t[n_frames + 1], 8-byte aligned; unspecified when status[0] = TRPX_ERR_CORRUPT
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS]; word 0 = TRPX_ERR_CORRUPT for a chain past terse_bytes, a width above
 *                  max_bits or fewer frames present than n_frames (n_frames smaller than the frames present is no error)
 *   workspace      DEVICE >= trpx_locate_workspace_bytes(), 8-byte aligned: a function of terse_bytes and n_frames, never
 *                  of n_frames x blocks -- for block 12 in this version 256 bytes + one byte per frame + 16 bytes per 4096
 *                  bits of the stack (about terse_bytes / 32) + 32 bytes per 256 Kbit, rounded up to 256; 256 bytes otherwise.
 *                  The size does not depend on max_bits, so a block-12 stack that takes the serial route (max_bits 64,
 *                  fewer than 4 frames, under 8 KB) is asked for the same scratch and leaves it unused
 * Stream-ordered, no allocation, no host synchronisation: capturable into a HIP graph.  Argument errors are return codes.
 */
size_t trpx_locate_workspace_bytes(size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block);
int trpx_locate_frames(const uint8_t* terse, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                       unsigned max_bits, uint64_t* frame_offsets, uint32_t* status, void* workspace, size_t workspace_bytes,
                       void* stream);
/*
 * Frame locator selection (trpx_locate_frames and the entry points built on it): 0 = auto (position-parallel where its
 * preconditions hold), 1 = always the serial walk.  Both yield the same offsets and status; the setter exists for tests and
 * A/B measurements.  Process-wide; also settable with the environment variable TRPX_LOCATE_PATH=serial.
 */
int trpx_set_locate_path(int path);

/*
 * Summing decode: sums of consecutive frames straight from the stream, without writing the decoded frames.
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32: its signedness and the widest legal block (as trpx_build_index)
 *   out_dtype      TRPX_I32, U32, I64, U64, F32 or F64
 *   terse          DEVICE const uint8_t[terse_bytes], 4-byte aligned
 *   frame_offsets  DEVICE const uint64_t[n_frames + 1], 8-byte aligned, or NULL (an index-free stack): the frames are then
 *                  located in the workspace first, as trpx_decode(frame_offsets = NULL) does (position-parallel where
 *                  trpx_locate_frames takes that route, the serial walk otherwise)
 *   index          DEVICE decode index of exactly these frames (trpx_encode_indexed / trpx_build_index), 16-byte aligned, or
 *                  NULL: the index is built in the workspace by trpx_build_index's walk.  Given, it is validated against the
 *                  frame sizes as in trpx_decode_indexed (a mismatch: status[0] = TRPX_ERR_CORRUPT).  Needs frame_offsets.
 *   group          frames per output, >= 1
 *   sums_out       DEVICE [n_out][n_values] of out_dtype, n_out = ceil(n_frames / group), aligned to its type (16 B: the
 *                  fast case).  Output j = the sum of frames [j * group, min((j + 1) * group, n_frames)): a group that does
 *                  not divide n_frames leaves a shorter last group.
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS]; word 0 = TRPX_ERR_CORRUPT in the cases of trpx_decode, for an index
 *                  that does not fit the frames and for a block wider than dtype's; with index == NULL also for a valid stream
 *                  with restated widths (trpx_build_index's verdict; the host form returns it); the sums are then unspecified
 *   workspace      DEVICE, 8-byte aligned, >= trpx_decode_sum_workspace_bytes() (the need with frame_offsets and index both
 *                  NULL; with them given less is used: a call with offsets, index and no frame chunks needs none)
 * The sum is exact in integers and converted once: I32 / U32 clamp to their limits (the narrowing of Bit_pointer.hpp:747-763),
 * I64 / U64 are exact, F32 / F64 are the exact sum rounded once to nearest even.  A signed stream into U32 / U64 is
 * TRPX_ERR_UNSUPPORTED (Terse.hpp:356-357); an unsigned stream into a signed output keeps the value, up to the clamp.  The
 * sums are bit-identical across runs, input forms and launch splits (integer accumulation, no float atomics).
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL (offsets are absolute into terse).
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, a signed stream into an
 * unsigned output; TRPX_ERR_INVALID_ARG for group 0, null or misaligned pointers, an unknown dtype / out_dtype, an index
 * without offsets; TRPX_ERR_CAPACITY for a workspace that is too small.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape and split is
 * decided on the host from the geometry alone.
 * trpx_decode_sum_host: host terse / frame_offsets (or NULL) / sums_out; stages, calls trpx_decode_sum and synchronises.
 */
size_t trpx_decode_sum_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames,
                                       unsigned block, unsigned group);
int trpx_decode_sum(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                    const uint64_t* frame_offsets, const void* index, size_t n_values, size_t n_frames,
                    unsigned block, unsigned group, void* sums_out, uint32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream);
int trpx_decode_sum_host(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes,
                         const uint64_t* frame_offsets, size_t n_values, size_t n_frames, unsigned block,
                         unsigned group, void* sums_out, int device);

/*
 * Box decode: boxes of pixels straight from the stream and its decode index, without expanding the frames.
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32; the output has the same type
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_sum: index given -- the kernel runs alone, no workspace is used;
 *                  offsets only -- the index is built in the workspace by trpx_build_index's walk; offsets NULL -- the frames
 *                  are located in the workspace first.  workspace: DEVICE, 8-byte aligned, >=
 *                  trpx_decode_roi_workspace_bytes() (the need with offsets and index both NULL), may be NULL with an index
 *   width          row length of a frame: n_values % width == 0, height = n_values / width
 *   boxes          DEVICE const uint32_t[n_boxes][3] = {frame, y0, x0}, 4-byte aligned (a device list: a picker on the GPU can
 *                  feed it, a captured graph is replayed with new boxes).  All boxes are box_h x box_w, 1 <= box_h <= height,
 *                  1 <= box_w <= width; they may overlap, repeat and come in any order
 *   pixels_out     DEVICE T[n_boxes][box_h][box_w], compact, aligned to T: [i][r][c] = pixel (y0 + r) * width + x0 + c of
 *                  frame boxes[i].frame
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  Word 0 = TRPX_ERR_CORRUPT when a 256-block group the kernel walks does
 *                  not end where the next group's offset (the last group: the frame's size) says, a block is wider than dtype
 *                  allows, or a read would leave the frame; with index == NULL also for a valid stream with restated widths
 *                  (trpx_build_index's verdict on the whole stack); TRPX_ERR_INVALID_ARG when a box has frame >= n_frames, y0 + box_h
 *                  > height or x0 + box_w > width -- that box's output is unspecified, the other boxes are still correct.  With
 *                  errors of both kinds either is reported.  ONLY THE GROUPS THE BOXES TOUCH ARE READ AND VALIDATED: status 0
 *                  says nothing about the rest of the stack (with offsets or index NULL the locator's / the walk's verdict on
 *                  the whole stack is reported as by trpx_decode_sum).
 * The stream is read in aligned 32-bit words, as by every decoder here: nothing outside terse[0 .. align4(terse_bytes)) is read,
 * nothing outside pixels_out is written.
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL; box frame numbers are relative to a.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, frames of >= 2^32 bits;
 * TRPX_ERR_INVALID_ARG for an unknown dtype, width 0 or not dividing n_values, box_h / box_w 0 or larger than the frame,
 * n_boxes 0, null or misaligned pointers, an index without offsets; TRPX_ERR_CAPACITY for a workspace that is too small.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape is decided on the
 * host from n_boxes, box_h, box_w, width and n_values alone, never from the boxes' contents.
 * trpx_decode_roi_host: host terse / frame_offsets (or NULL) / boxes / pixels_out; checks the boxes on the host
 * (TRPX_ERR_INVALID_ARG for one that leaves the stack), stages, calls trpx_decode_roi and synchronises.
 */
size_t trpx_decode_roi_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block);
int trpx_decode_roi(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                    size_t n_values, size_t n_frames, unsigned block, size_t width, const uint32_t* boxes, size_t n_boxes,
                    unsigned box_h, unsigned box_w, void* pixels_out, uint32_t* status, void* workspace,
                    size_t workspace_bytes, void* stream);
int trpx_decode_roi_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                         size_t n_frames, unsigned block, size_t width, const uint32_t* boxes, size_t n_boxes,
                         unsigned box_h, unsigned box_w, void* pixels_out, int device);

/*
 * Threshold decode: the pixels at or above a threshold, in CSR form, straight from the stream and its decode index, without
 * expanding the frames.  A block's width bounds its values: the payload of a block too narrow to hold the threshold is never read.
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32; `values` has the same type
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_sum: index given; offsets only -- the index is built in the workspace by
 *                  trpx_build_index's walk; offsets NULL -- the frames are located in the workspace first.  workspace: DEVICE,
 *                  8-byte aligned, ALWAYS needed (the counts live there): trpx_decode_sparse_workspace_bytes() is the need with
 *                  offsets and index both NULL; with offsets or index given less is used, and the call checks against what its
 *                  own form needs.  The size is arithmetic on terse_bytes, n_frames and the number of 256-block groups
 *   threshold      pixel p of frame f is an event iff (int64) value >= threshold, a mathematical comparison whatever the type.
 *                  At or below the type's minimum every pixel is an event, above its maximum none is; both are legal.  The
 *                  twelve zeros of a width-0 block are events, with value 0, when threshold <= 0
 *   row_offsets    DEVICE uint64_t[n_frames + 1], 8-byte aligned: [f] = events in the frames < f, [n_frames] = the total
 *   positions      DEVICE uint32_t[capacity]: the pixel index of event i inside its frame
 *   values         DEVICE T[capacity], aligned to T: its value.  Events come by frame and, inside a frame, by ascending pixel
 *                  index -- frame by frame what np.flatnonzero(px[f] >= threshold) and px[f][...] give -- bit-identical across
 *                  runs, input forms and launch shapes
 *   capacity       elements of positions / values.  A total above it: status word 0 = TRPX_ERR_CAPACITY, row_offsets is still
 *                  complete and valid, positions / values [0 .. capacity) are unspecified and nothing at or behind capacity is
 *                  touched (trpx_encode's convention); capacity == total is success.  A sizes-only query passes positions =
 *                  values = NULL with capacity 0 (one NULL without the other, or NULL with capacity > 0: TRPX_ERR_INVALID_ARG)
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  Word 0 = TRPX_ERR_CORRUPT when a 256-block group does not end where the
 *                  next group's offset (the last group: the frame's size) says, a block is wider than dtype allows, a frame lies
 *                  outside the stream or the index does not fit the offsets, with index == NULL also for a valid stream with
 *                  restated widths (trpx_build_index's verdict): EVERY group of EVERY frame is walked, so the whole
 *                  stack is validated (unlike trpx_decode_roi).  The outputs are then unspecified.  TRPX_ERR_CORRUPT wins over
 *                  TRPX_ERR_CAPACITY when both apply
 * The stream is read in aligned 32-bit words: nothing outside terse[0 .. align4(terse_bytes)) is read, nothing outside
 * row_offsets[0 .. n_frames], positions[0 .. capacity) and values[0 .. capacity) is written, whatever the status.
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, frames of >= 2^32 bits (which
 * is also what makes positions fit 32 bits); TRPX_ERR_INVALID_ARG for an unknown dtype, bad sizes, null or misaligned pointers,
 * the NULL / capacity rule above, an index without offsets, a NULL workspace; TRPX_ERR_CAPACITY for a workspace that is too small.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape is decided on the
 * host from n_frames and n_values alone, never from the data or the threshold.
 * trpx_decode_sparse_host: host terse / frame_offsets (or NULL) / outputs; checks its arguments before a device is looked for,
 * stages, calls trpx_decode_sparse, synchronises and sets *n_found to the total.  With a capacity that is too small *n_found
 * and row_offsets are still valid and it returns TRPX_ERR_CAPACITY: a caller sizes a second call from them.
 */
size_t trpx_decode_sparse_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block);
int trpx_decode_sparse(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                       size_t n_values, size_t n_frames, unsigned block, int64_t threshold, uint64_t* row_offsets,
                       uint32_t* positions, void* values, size_t capacity, uint32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream);
int trpx_decode_sparse_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                            size_t n_frames, unsigned block, int64_t threshold, uint64_t* row_offsets, uint32_t* positions,
                            void* values, size_t capacity, size_t* n_found, int device);

/*
 * Weighted per-frame sums: dots_out[f][k] = sum over the pixels p of frame f of px[f][p] * weights[k][p], straight from the stream
 * and its decode index, without expanding the frames -- a virtual detector image (a mask per detector region), the centre of mass
 * (the maps x, y and 1), the per-frame dose.  A width-0 block adds nothing and has no payload; the payload of a block on which
 * every map is zero is never read.
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_sum: index given -- validated against the frame sizes as in
 *                  trpx_decode_indexed; offsets only -- the index is built in the workspace by trpx_build_index's walk; offsets
 *                  NULL -- the frames are located in the workspace first.  workspace: DEVICE, 8-byte aligned, ALWAYS needed (one
 *                  support bit per block of a frame and the partial sums live there): trpx_decode_dot_workspace_bytes() is the
 *                  need with offsets and index both NULL; with offsets or index given less is used, and the call checks against
 *                  what its own form needs.  The size is arithmetic on terse_bytes, n_frames, the number of 256-block groups and
 *                  n_maps: beyond what the index needs, 8 * n_maps bytes per run of 8 groups and n_values / 96 bytes
 *   weights        DEVICE const int32_t[n_maps][n_values], map after map, compact, 4-byte aligned; 16-byte aligned with
 *                  n_values % 4 == 0 is the fast case.  Any int32 is legal, INT32_MIN included.  A device array on purpose: a
 *                  captured graph is replayed with new maps in the same buffer, and nothing derived from its contents is decided
 *                  on the host.  1 <= n_maps <= 16
 *   dots_out       DEVICE int64_t[n_frames][n_maps], 8-byte aligned: [f][k] = sum_p (int64) px[f][p] * (int64) weights[k][p] modulo
 *                  2^64 (two's-complement wrap; every single product fits int64 for every pixel type, so only the sum can wrap) --
 *                  what numpy's int64 arithmetic gives.  Integer arithmetic throughout: bit-identical across runs, input forms
 *                  and launch shapes
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  Word 0 = TRPX_ERR_CORRUPT in exactly the cases of trpx_decode_sparse: a
 *                  256-block group does not end where the next group's offset (the last group: the frame's size) says, a block is
 *                  wider than dtype allows, a frame lies outside the stream or the index does not fit the offsets, with index ==
 *                  NULL also for a valid stream with restated widths (trpx_build_index's verdict).  EVERY group of EVERY frame is
 *                  walked and validated, also where no block of it is fetched.  The outputs are then unspecified
 * The stream is read in aligned 32-bit words: nothing outside terse[0 .. align4(terse_bytes)) and weights[0 .. n_maps * n_values)
 * is read (the weights behind a map's n_values are never read for a frame's partial last block), nothing outside dots_out, status
 * and the workspace is written, whatever the status.
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, frames of >= 2^32 bits;
 * TRPX_ERR_INVALID_ARG for an unknown or float dtype, zero sizes, n_maps 0 or above 16, null or misaligned pointers, an index
 * without offsets, a NULL workspace; TRPX_ERR_CAPACITY for a workspace that is too small.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape is decided on the
 * host from n_frames, n_values and n_maps alone, never from the data or the maps.
 * trpx_decode_dot_host: host terse / frame_offsets (or NULL) / weights / dots_out; checks its arguments before a device is looked
 * for, stages, calls trpx_decode_dot and synchronises.
 */
size_t trpx_decode_dot_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                                       unsigned n_maps);
int trpx_decode_dot(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                    size_t n_values, size_t n_frames, unsigned block, const int32_t* weights, unsigned n_maps,
                    int64_t* dots_out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int trpx_decode_dot_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                         size_t n_values, size_t n_frames, unsigned block, const int32_t* weights, unsigned n_maps,
                         int64_t* dots_out, int device);

/*
 * Per-frame sums over labelled pixel bins: bins_out[f][b] = sum over the pixels p of frame f with labels[p] == b of px[f][p],
 * straight from the stream and its decode index, without expanding the frames -- the radial profile (azimuthal integration) of
 * every frame, ring detectors, any partition of the detector into up to 4096 regions.  One label per pixel whatever the number
 * of bins: the stream is walked once.  A width-0 block adds nothing and has no payload; the payload of a block none of whose
 * labels is a bin is never read.
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_dot: index given -- validated against the frame sizes as in
 *                  trpx_decode_indexed; offsets only -- the index is built in the workspace by trpx_build_index's walk; offsets
 *                  NULL -- the frames are located in the workspace first.  workspace: DEVICE, 8-byte aligned, ALWAYS needed (one
 *                  support bit per block of a frame lives there): trpx_decode_bins_workspace_bytes() is the need with offsets
 *                  and index both NULL; with offsets or index given less is used, and the call checks against what its own form
 *                  needs.  The size is arithmetic: beyond what the index needs (trpx_decode_roi_workspace_bytes()), the support
 *                  words, 4 * ceil(ceil(n_values / 12) / 32) bytes rounded up to 8, and, where spans =
 *                  trpx_decode_bins_spans_per_frame(n_values, n_frames) is more than 1, 8 * n_bins * n_frames * spans bytes of
 *                  partial sums -- nothing otherwise
 *   labels         DEVICE const uint16_t[n_values], 2-byte aligned; 8-byte aligned is the fast case (a block's 12 labels are
 *                  three 8-byte loads).  A label >= n_bins belongs to NO bin: this is how a beam stop, dead pixels and detector
 *                  gaps are masked (0xFFFF); it is legal, not an error.  A device array on purpose: a captured graph is replayed
 *                  with a new map in the same buffer, and nothing derived from its contents is decided on the host.
 *                  1 <= n_bins <= 4096
 *   bins_out       DEVICE int64_t[n_frames][n_bins], 8-byte aligned.  EVERY element is written by every successful call (a bin
 *                  without pixels is 0): the caller clears nothing.  The sums are exact: a frame has fewer than 2^29 values of
 *                  magnitude at most 2^32, so no sum leaves int64.  Integer arithmetic throughout: bit-identical across runs,
 *                  input forms and launch shapes
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  Word 0 = TRPX_ERR_CORRUPT in exactly the cases of trpx_decode_dot: a
 *                  256-block group does not end where the next group's offset (the last group: the frame's size) says, a block is
 *                  wider than dtype allows, a frame lies outside the stream or the index does not fit the offsets, with index ==
 *                  NULL also for a valid stream with restated widths (trpx_build_index's verdict).  EVERY group of EVERY frame is
 *                  walked and validated, also where every label of it is masked or every block has width 0.  The outputs are
 *                  then unspecified
 * The stream is read in aligned 32-bit words: nothing outside terse[0 .. align4(terse_bytes)) and labels[0 .. n_values) is read
 * (the labels behind n_values are never read for a frame's partial last block), nothing outside bins_out, status and the
 * workspace is written, whatever the status.
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, frames of >= 2^32 bits;
 * TRPX_ERR_INVALID_ARG for an unknown or float dtype, zero sizes, n_bins 0 or above 4096, null or misaligned pointers, an index
 * without offsets, a NULL workspace; TRPX_ERR_CAPACITY for a workspace that is too small for the call's own form.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape is decided on the
 * host from n_frames, n_values and n_bins alone, never from the data or the map.
 * trpx_decode_bins_spans_per_frame: the workgroups a frame is cut into, min(ceil(runs / 4), max(1, ceil(1536 / n_frames))) with
 * runs = ceil(groups / 8) -- pure arithmetic, for tests and diagnostics (0 for sizes no call takes); above 1 the partial sums of
 * the spans pass through the workspace.
 * trpx_decode_bins_host: host terse / frame_offsets (or NULL) / labels / bins_out; checks its arguments before a device is looked
 * for, stages, calls trpx_decode_bins and synchronises.
 */
size_t trpx_decode_bins_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                                        unsigned n_bins);
unsigned trpx_decode_bins_spans_per_frame(size_t n_values, size_t n_frames);
int trpx_decode_bins(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                     size_t n_values, size_t n_frames, unsigned block, const uint16_t* labels, unsigned n_bins,
                     int64_t* bins_out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int trpx_decode_bins_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                          size_t n_values, size_t n_frames, unsigned block, const uint16_t* labels, unsigned n_bins,
                          int64_t* bins_out, int device);

/*
 * Value histograms: hist_out[g][b] = the number of pixels of the frames of group g whose bin is b, straight from the stream and
 * its decode index, without expanding the frames -- the threshold of trpx_decode_sparse, the percentiles a preview is scaled by,
 * detector QC (saturation pile-up in the last bin, a negative tail after dark subtraction), "how many pixels >= t" for many t at
 * once.  It stands in for the loop of src/prolix.cpp:69-92 (one `trpx_data.prolix(image, i)` per frame, Terse.hpp:387-388) with a
 * histogram of every expanded image behind it.
 *     bin(v) = clamp(floor((v - lo) / 2^shift), 0, n_bins - 1), computed in int64
 * -- in numpy np.bincount(np.clip((px.astype(np.int64) - lo) >> shift, 0, n_bins - 1).ravel(), minlength=n_bins) per group (>> is
 * arithmetic: values below lo floor).  The first and the last bin take everything below and above: every pixel is counted
 * exactly once, and each row sums to n_values * (frames in the group).  The twelve zeros of a width-0 block are pixels and are
 * counted, in bin(0).  A block's width bounds its values: a block whose whole value range lies inside one bin is counted from
 * its width alone, and its payload is never fetched.
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_bins: index given -- validated against the frame sizes as in
 *                  trpx_decode_indexed; offsets only -- the index is built in the workspace by trpx_build_index's walk; offsets
 *                  NULL -- the frames are located in the workspace first.  workspace: DEVICE, 8-byte aligned;
 *                  trpx_decode_hist_workspace_bytes() is the need with offsets and index both NULL; with offsets or index given
 *                  less is used, and the call checks against what its own form needs (index given and one span per group:
 *                  nothing, NULL is legal).  The size is arithmetic: beyond what the index needs
 *                  (trpx_decode_roi_workspace_bytes()), where spans = trpx_decode_hist_spans_per_group(n_values, n_frames, group)
 *                  is more than 1, 8 * n_bins * ceil(n_frames / group) * spans bytes of partial counts -- nothing otherwise
 *   group          frames per histogram, trpx_decode_sum's rule: >= 1; groups are `group` consecutive frames, the last one holds
 *                  what is left (a group larger than the stack: one group).  group = 1: per frame; group = n_frames: the stack's
 *   lo, shift, n_bins
 *                  the bin rule above.  -2^32 <= lo <= 2^32, 0 <= shift <= 32, 1 <= n_bins <= 4096: with these v - lo cannot
 *                  leave int64 for any pixel type
 *   hist_out       DEVICE uint64_t[ceil(n_frames / group)][n_bins], 8-byte aligned.  EVERY element is written by every successful
 *                  call (a bin without pixels is 0): the caller clears nothing.  Integer counting throughout: bit-identical
 *                  across runs, input forms, sub-stacks and launch shapes
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  Word 0 = TRPX_ERR_CORRUPT in exactly the cases of trpx_decode_bins: a
 *                  256-block group does not end where the next group's offset (the last group: the frame's size) says, a block is
 *                  wider than dtype allows, a frame lies outside the stream or the index does not fit the offsets, with index ==
 *                  NULL also for a valid stream with restated widths (trpx_build_index's verdict).  EVERY group of EVERY frame is
 *                  walked and validated, also where no block of it is fetched.  The outputs are then unspecified
 * The stream is read in aligned 32-bit words: nothing outside terse[0 .. align4(terse_bytes)) is read, nothing outside hist_out,
 * status and the workspace is written, whatever the status.
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, frames of >= 2^32 bits, more
 * groups of 256 blocks than one call takes; TRPX_ERR_INVALID_ARG for an unknown or float dtype, zero sizes, group 0, n_bins 0 or
 * above 4096, shift above 32, |lo| above 2^32, null or misaligned pointers, an index without offsets, a NULL workspace where the
 * call's form needs one; TRPX_ERR_CAPACITY for a workspace that is too small for the call's own form.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape is decided on the
 * host from n_frames, n_values, group and n_bins alone, never from the data.
 * trpx_decode_hist_spans_per_group: the workgroups a group is cut into, with R = min(group, n_frames) * ceil(groups of 256 blocks
 * / 8) runs a group and G = ceil(n_frames / group) groups: max(ceil(R / 2^17), min(ceil(R / 4), max(1, ceil(1536 / G)))) -- pure
 * arithmetic, for tests and diagnostics (0 for sizes no call takes, the stacks beyond TRPX_MAX_TILES_PER_CALL included, as is
 * trpx_decode_hist_workspace_bytes()); above 1 the partial counts of the spans pass through the workspace.  The ragged last group is cut into the same number of (shorter, possibly empty) spans.
 * trpx_decode_hist_host: host terse / frame_offsets (or NULL) / hist_out; checks its arguments before a device is looked for,
 * stages, calls trpx_decode_hist and synchronises.
 */
size_t trpx_decode_hist_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                                        size_t group, unsigned n_bins);
unsigned trpx_decode_hist_spans_per_group(size_t n_values, size_t n_frames, size_t group);
int trpx_decode_hist(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                     size_t n_values, size_t n_frames, unsigned block, size_t group, int64_t lo, unsigned shift,
                     unsigned n_bins, uint64_t* hist_out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int trpx_decode_hist_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                          size_t n_values, size_t n_frames, unsigned block, size_t group, int64_t lo, unsigned shift,
                          unsigned n_bins, uint64_t* hist_out, int device);

/*
 * Corrected decode: every frame of a stack as float32 with the detector's dark reference subtracted and its gain reference
 * multiplied in, straight from the stream and its decode index -- the frames motion correction or any float processing starts
 * from, without the integer stack and the float temporaries of decode + convert + subtract + multiply.  It stands in for the
 * loop of Terse.hpp:352-389 / src/prolix.cpp:69-92 with the correction applied to every expanded image.
 *     out[f][p] = ((float) px[f][p] - dark[p]) * gain[p]
 * -- in numpy, everything float32, (px.astype(np.float32) - dark[None]) * gain[None]: three IEEE binary32 operations in this
 * order, each rounded once to nearest even: the conversion (exact for 8- and 16-bit pixels, rounds 32-bit pixels of magnitude
 * above 2^24), the subtraction, the multiplication.  Nothing is fused or re-associated.  The result equals numpy's bit for bit
 * wherever that is zero, a normal number, +-inf or NaN (a NaN's payload is not defined); results that are SUBNORMAL are
 * unspecified: the device may flush them to zero.  gain[p] == 0 blanks a bad pixel; non-finite map entries are legal and
 * propagate.  The twelve zeros of a width-0 block are pixels: they come out as (0 - dark[p]) * gain[p].
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32
 *   out_dtype      TRPX_F32; anything else is TRPX_ERR_UNSUPPORTED (the parameter is there so that TRPX_F64 can follow without a
 *                  new symbol)
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_sum, with its rules and status meanings: index given -- validated
 *                  against the frame sizes, no workspace needed (NULL is legal); offsets only -- the index is built in the
 *                  workspace by trpx_build_index's walk; offsets NULL -- the frames are located in the workspace first.
 *                  workspace: DEVICE, 8-byte aligned; trpx_decode_corrected_workspace_bytes() is the need with offsets and index
 *                  both NULL -- what the index needs, trpx_decode_roi_workspace_bytes(), and 0 for sizes no call takes, the
 *                  stacks beyond TRPX_MAX_TILES_PER_CALL included; the call checks against what its own form needs
 *   dark, gain     DEVICE const float[n_values], 4-byte aligned, read by the kernel when it runs: a captured graph is replayed
 *                  with new maps in the same buffers.  Either may be NULL: dark == NULL leaves the subtraction out, gain == NULL
 *                  the multiplication -- exactly the results of an all +0.0f and an all 1.0f map; both NULL: a plain float32
 *                  decode
 *   out            DEVICE float[n_frames][n_values], 4-byte aligned.  EVERY element is written by every successful call.  The
 *                  fast case is out and both maps 16-byte aligned with n_values % 4 == 0: whole 16-byte stores and map loads;
 *                  any other alignment runs on the same kernel with accesses that assume 4 bytes only
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  Word 0 = TRPX_ERR_CORRUPT: a tile does not fit its frame, a block is
 *                  wider than dtype allows, a frame lies outside the stream or the index does not fit the offsets, with index ==
 *                  NULL also for a valid stream with restated widths.  Every tile of every frame is validated.  `out` is then
 *                  unspecified
 * Nothing outside terse[0 .. align4(terse_bytes)), dark[0 .. n_values) and gain[0 .. n_values) is read -- a frame's partial last
 * block reads no map entry behind n_values --, nothing outside out, status and the workspace is written, whatever the status.
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, another out_dtype, frames of
 * >= 2^32 bits, more groups of 256 blocks than one call takes; TRPX_ERR_INVALID_ARG for an unknown or float dtype, zero sizes,
 * null or misaligned pointers, an index without offsets; TRPX_ERR_CAPACITY for a workspace too small for the call's own form.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); the launch shape is decided on the host
 * from n_frames and n_values alone, never from the data.
 * trpx_decode_corrected_host: host terse / frame_offsets (or NULL) / dark / gain (or NULL) / out; checks its arguments before a
 * device is looked for, stages, calls trpx_decode_corrected and synchronises.
 */
size_t trpx_decode_corrected_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block);
int trpx_decode_corrected(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                          const void* index, size_t n_values, size_t n_frames, unsigned block, const float* dark, const float* gain,
                          void* out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int trpx_decode_corrected_host(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                               size_t n_values, size_t n_frames, unsigned block, const float* dark, const float* gain, void* out,
                               int device);

/*
 * Binned decode: every frame summed over bins of bin_y x bin_x neighbouring pixels, straight from the stream and its decode
 * index, without expanding the frames -- previews, binned diffraction patterns for indexing, down-sampled movies.  A frame is
 * height = n_values / width rows of `width` pixels (as trpx_decode_roi); out_h = ceil(height / bin_y), out_w = ceil(width / bin_x),
 *     binned_out[f][Y][X] = sum of px[f][y][x] over Y * bin_y <= y < min((Y + 1) * bin_y, height),
 *                                                   X * bin_x <= x < min((X + 1) * bin_x, width):
 * the edge bins of a frame whose sides are no multiples of the bin sum the pixels that exist (a 1030 x 1065 frame bins by 2).
 * A width-0 block adds nothing and has no payload: it is never fetched.
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32
 *   out_dtype      TRPX_I32, TRPX_U32, TRPX_I64, TRPX_U64, TRPX_F32 or TRPX_F64, converted exactly as trpx_decode_sum does: the sum
 *                  is exact in integers and converted once -- 32-bit integers clamp, 64-bit integers keep the value, floats round
 *                  once to nearest even.  A signed stream into U32 / U64 is TRPX_ERR_UNSUPPORTED
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_roi: index given -- validated against the frame sizes as in
 *                  trpx_decode_indexed, the kernel alone, no workspace (NULL allowed); offsets only -- the index is built in the
 *                  workspace by trpx_build_index's walk; offsets NULL -- the frames are located in the workspace first.  The call
 *                  has no scratch of its own: trpx_decode_binned_workspace_bytes() = trpx_decode_roi_workspace_bytes(), the need
 *                  with offsets and index both NULL; the call checks against what its own form needs
 *   width          pixels per row; n_values % width == 0
 *   bin_y, bin_x   1 <= bin_y <= min(height, 64), 1 <= bin_x <= min(width, 64).  (1, 1) is legal: a widening decode.  The cap
 *                  bounds a band of one output row to 64 rows of pixels, and lets the pixel types of up to 16 bits accumulate in
 *                  32 bits (64 * 64 * 65535 < 2^32).  out_w > 8192 is TRPX_ERR_UNSUPPORTED: one output row of 64-bit sums has
 *                  to fit 64 KB of LDS
 *   binned_out     DEVICE out_dtype[n_frames][out_h][out_w], compact, aligned to its type.  EVERY element is written by every
 *                  successful call: the caller clears nothing.  Integer accumulation only: bit-identical across runs, input
 *                  forms and launch shapes
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  Word 0 = TRPX_ERR_CORRUPT in exactly the cases of trpx_decode_bins: a
 *                  256-block group does not end where the next group's offset (the last group: the frame's size) says, a block is
 *                  wider than dtype allows, a frame lies outside the stream or the index does not fit the offsets, with index ==
 *                  NULL also for a valid stream with restated widths (trpx_build_index's verdict).  EVERY group of EVERY frame is
 *                  walked and validated, also where every block of it has width 0.  The outputs are then unspecified
 * The stream is read in aligned 32-bit words: nothing outside terse[0 .. align4(terse_bytes)) is read, nothing outside
 * binned_out, status and the workspace is written, whatever the status.
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, frames of >= 2^32 bits, a
 * signed stream into an unsigned output, out_w > 8192; TRPX_ERR_INVALID_ARG for an unknown or float dtype, an out_dtype that is
 * none of the six, zero sizes, a width that does not divide n_values, a bin side of 0, above 64 or above the frame's, null or
 * misaligned pointers, an index without offsets; TRPX_ERR_CAPACITY for a workspace that is too small for the call's own form.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape is decided on the
 * host from n_frames, n_values, width, bin_y and bin_x alone, never from the data.
 * trpx_decode_binned_bands_per_frame: the workgroups a frame is cut into, each a band of whole output rows whose sums live in
 * LDS: rows = ceil(out_h / want), bands = ceil(out_h / rows), with want = min(out_h, max(ceil(out_h / max(1, 8192 / out_w)),
 * min(ceil(1536 / n_frames), ceil(groups / 8)))) and groups = ceil(ceil(n_values / 12) / 256) -- pure arithmetic, for tests and
 * diagnostics (0 for sizes no call takes).
 * trpx_decode_binned_host: host terse / frame_offsets (or NULL) / binned_out; checks its arguments before a device is looked
 * for, stages, calls trpx_decode_binned and synchronises.
 */
size_t trpx_decode_binned_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block);
unsigned trpx_decode_binned_bands_per_frame(size_t n_values, size_t width, unsigned bin_y, unsigned bin_x, size_t n_frames);
int trpx_decode_binned(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                       const void* index, size_t n_values, size_t n_frames, unsigned block, size_t width, unsigned bin_y,
                       unsigned bin_x, void* binned_out, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int trpx_decode_binned_host(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                            size_t n_values, size_t n_frames, unsigned block, size_t width, unsigned bin_y, unsigned bin_x,
                            void* binned_out, int device);

/*
 * Reducing decode: per pixel, one statistic over groups of consecutive frames, straight from the stream and its decode index,
 * without writing the decoded frames -- the companion of trpx_decode_sum for the statistics that are no sum of pixels: the
 * maximum pattern of a scan, the sum of squares behind a variance (noise) map, the hit-rate map of a counting detector.
 *   dtype          the stream's pixel type T, TRPX_U8 .. TRPX_I32
 *   op             TRPX_REDUCE_MAX / TRPX_REDUCE_MIN: out is T[n_out][n_values], exactly px[g0:g1].max(0) / .min(0).  The zeros of a
 *                  width-0 block take part: the max of negative frames and one blank frame is 0.
 *                  TRPX_REDUCE_SUMSQ: out is uint64_t, the sum of (int64)v * (int64)v modulo 2^64, accumulated in unsigned
 *                  arithmetic: always exact for 8- and 16-bit pixel types, for 32-bit types while the true sum is below 2^64 (the
 *                  precedent of trpx_decode_dot).
 *                  TRPX_REDUCE_COUNT_GE: out is uint32_t, the number of frames of the group with (int64)v >= threshold, the
 *                  comparison of trpx_decode_sparse: a threshold at or below the type's minimum counts every frame, one above its
 *                  maximum counts none.  count == frames of the group: a hot pixel.
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_sum: index given -- no workspace unless the launch plan splits the groups
 *                  into frame chunks; offsets only -- the index is built in the workspace by trpx_build_index's walk; offsets NULL
 *                  -- the frames are located in the workspace first.  workspace: DEVICE, 8-byte aligned, >=
 *                  trpx_decode_reduce_workspace_bytes() (the need with offsets and index both NULL; the call checks against what
 *                  its own form needs)
 *   group          frames per output, >= 1; n_out = ceil(n_frames / group); output j reduces frames [j * group, min((j + 1) * group,
 *                  n_frames)): a short last group reduces the frames that exist
 *   threshold      TRPX_REDUCE_COUNT_GE only; ignored by the other ops
 *   out            DEVICE, compact, aligned to its element type only.  EVERY element is written by every successful call: the
 *                  caller clears nothing.  Integer arithmetic, no atomics on the output: bit-identical across runs, input forms
 *                  and launch splits
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS]; word 0 = TRPX_ERR_CORRUPT in the cases of trpx_decode_sum, with index == NULL
 *                  also for a valid stream with restated widths; the outputs are then unspecified
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, frames of >= 2^32 bits;
 * TRPX_ERR_INVALID_ARG for an unknown or float dtype, an unknown op, group 0, bad sizes, null or misaligned pointers, an index
 * without offsets; TRPX_ERR_CAPACITY for a workspace that is too small for the call's own form.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape and split is decided
 * on the host from the geometry alone: trpx_decode_sum's plan.  trpx_decode_reduce_chunks: the frame chunks a group is split
 * into -- pure arithmetic, for tests and diagnostics (0 for sizes no call takes).
 * trpx_decode_reduce_host: host terse / frame_offsets (or NULL) / out; checks its arguments before a device is looked for,
 * stages, calls trpx_decode_reduce and synchronises.
 */
typedef enum trpx_reduce_op { TRPX_REDUCE_MAX = 0, TRPX_REDUCE_MIN = 1, TRPX_REDUCE_SUMSQ = 2, TRPX_REDUCE_COUNT_GE = 3 } trpx_reduce_op;
size_t trpx_decode_reduce_workspace_bytes(int dtype, int op, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                                          unsigned group);
unsigned trpx_decode_reduce_chunks(int dtype, size_t n_values, size_t n_frames, unsigned group);
int trpx_decode_reduce(int dtype, int op, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                       size_t n_values, size_t n_frames, unsigned block, unsigned group, int64_t threshold, void* out,
                       uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int trpx_decode_reduce_host(int dtype, int op, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                            size_t n_frames, unsigned block, unsigned group, int64_t threshold, void* out, int device);

/*
 * Labelled summing decode: the sum of the frames that carry the same label, one label per frame, straight from the stream and its
 * decode index, without writing the decoded frames -- trpx_decode_sum for frames that do not lie next to each other: the
 * real-space binning of a scan, the mean pattern of every cluster of scan positions, the sum of the hits alone.  The transpose of
 * trpx_decode_bins (one label per pixel).
 *   dtype          the stream's pixel type, TRPX_U8 .. TRPX_I32
 *   out_dtype      as trpx_decode_sum: TRPX_I32 / TRPX_U32 (clamped), TRPX_I64 / TRPX_U64 (exact), TRPX_F32 / TRPX_F64 (the exact
 *                  integer sum rounded once to nearest even); a signed stream into U32 / U64 is TRPX_ERR_UNSUPPORTED
 *   terse, frame_offsets, index, workspace
 *                  the three input forms of trpx_decode_sum: index given -- validated against the frame sizes as in
 *                  trpx_decode_indexed; offsets only -- the index is built in the workspace by trpx_build_index's walk; offsets NULL
 *                  -- the frames are located in the workspace first.  workspace: DEVICE, 8-byte aligned, NEVER NULL (the order
 *                  of the frames lives there), >= trpx_decode_sum_labelled_workspace_bytes() (the need with offsets and index both
 *                  NULL; the call checks against what its own form needs).  Own scratch: 16 bytes per output, 8 per frame, and two
 *                  frames' worth of raw accumulators for each of at most about 1024 chunks of the ordered frames
 *   labels         DEVICE const uint32_t[n_frames], 4-byte aligned.  labels[f] < n_out: frame f is added into output labels[f];
 *                  labels[f] >= n_out: frame f takes part in nothing (0xFFFFFFFF is the conventional mask) -- legal, not an error.
 *                  A device array on purpose: a captured graph is replayed with new labels in the same buffer, and nothing that
 *                  depends on the labels' contents is decided on the host
 *   n_out          1 .. 2^20 outputs (above: TRPX_ERR_UNSUPPORTED); may exceed n_frames
 *   sums_out       DEVICE [n_out][n_values] of out_dtype, compact, aligned to its element type only.  EVERY element is written by
 *                  every successful call, an output without frames is 0: the caller clears nothing
 *   counts_out     DEVICE uint32_t[n_out] or NULL: the frames of every output (for means)
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS]; word 0 = TRPX_ERR_CORRUPT in the cases of trpx_decode_sum, for the frames that
 *                  have an output.  A MASKED FRAME IS NEVER READ AND NEVER VALIDATED: status 0 says nothing about it.  With index ==
 *                  NULL trpx_build_index's verdict on the whole stack is reported (masked frames and valid streams with restated
 *                  widths included).  After a non-zero status the outputs are unspecified
 * Integer accumulation, no float atomics: bit-identical across runs, input forms, label orders and launch shapes.  Nothing outside
 * terse[0 .. align4(terse_bytes)), labels[0 .. n_frames), the offsets and the index is read; nothing outside sums_out, counts_out,
 * status and the workspace is written, whatever the labels hold.
 * Frames [a, b) of a stack alone: frame_offsets + a, n_frames = b - a, index = NULL; labels[0] is frame a's.
 * Errors returned before any device call, in trpx_decode_sum's order: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers,
 * frames of >= 2^32 bits, a signed stream into an unsigned output, n_out > 2^20; TRPX_ERR_INVALID_ARG for an unknown or float
 * dtype, an out_dtype that is none of the six, n_out 0, bad sizes, null or misaligned pointers (labels included), an index without
 * offsets, a NULL workspace; TRPX_ERR_CAPACITY for a workspace that is too small for the call's own form.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape and split is decided
 * on the host from n_frames, n_values, n_out and dtype alone.  trpx_decode_sum_labelled_frames_per_chunk: the length of the
 * chunks the ordered frames are cut into -- pure arithmetic, for tests and diagnostics (0 for sizes no call takes).
 * trpx_decode_sum_labelled_host: host terse / frame_offsets (or NULL) / labels / sums_out / counts_out (or NULL); checks its
 * arguments before a device is looked for, stages, calls trpx_decode_sum_labelled and synchronises.
 */
size_t trpx_decode_sum_labelled_workspace_bytes(int dtype, size_t terse_bytes, size_t n_values, size_t n_frames, unsigned block,
                                                size_t n_out);
unsigned trpx_decode_sum_labelled_frames_per_chunk(int dtype, size_t n_values, size_t n_frames);
int trpx_decode_sum_labelled(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                             const void* index, size_t n_values, size_t n_frames, unsigned block, const uint32_t* labels, size_t n_out,
                             void* sums_out, uint32_t* counts_out, uint32_t* status, void* workspace, size_t workspace_bytes,
                             void* stream);
int trpx_decode_sum_labelled_host(int dtype, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                                  size_t n_values, size_t n_frames, unsigned block, const uint32_t* labels, size_t n_out,
                                  void* sums_out, uint32_t* counts_out, int device);

/*
 * Encode from events: the stream of a stack given in CSR form -- what trpx_decode_sparse writes, what a counting detector or a
 * hit finder produces --, without a dense frame ever existing in memory.  Frame f is n_values zeros with
 * px[f][positions[i]] = values[i] for i in [row_offsets[f], row_offsets[f + 1]).  out, frame_offsets, status word 0 and word 1
 * (prolix_bits) are exactly what trpx_encode leaves for those frames, byte for byte, the zeroed bytes [total, align4(total))
 * included, bit-identical across runs and launch shapes.  The work is in proportion to events + output bits, never to
 * n_frames x n_values.
 *   dtype          the pixel type, TRPX_U8 .. TRPX_I32; `values` has that type
 *   row_offsets    DEVICE uint64_t[n_frames + 1], 8-byte aligned, non-decreasing: absolute indices into positions / values.
 *                  [0] need not be 0; [n_frames] <= n_events.  Frames [a, b) of a larger CSR alone: row_offsets + a, n_frames = b - a
 *   positions      DEVICE uint32_t[n_events]: strictly ascending inside a frame, < n_values
 *   values         DEVICE T[n_events], aligned to T: anything of the type -- an explicit 0 is a zero pixel, negative values of
 *                  signed types and the type's minimum are allowed
 *   n_events       elements of positions / values.  0 with positions = values = NULL is legal: a stack of empty frames (one NULL
 *                  without the other, or NULL with n_events > 0: TRPX_ERR_INVALID_ARG)
 *   out, out_capacity, frame_offsets
 *                  as for trpx_encode (out 16-byte aligned).  A stack that does not fit: status word 0 = TRPX_ERR_CAPACITY,
 *                  frame_offsets is still complete and valid, nothing at or behind out_capacity is touched; out_capacity ==
 *                  align4(total) is success.  A sizes-only query passes out = NULL with out_capacity 0.
 *                  trpx_encode_sparse_bound_bytes() is an upper bound from the event count alone, so that a sparse caller need
 *                  not allocate n_frames x trpx_worst_case_bytes: a block without events costs 1 bit (4 behind a block with
 *                  events), a block with events at most 12 + 12 x bits(T) bits, and there are at most n_events of those; a pad
 *                  byte per frame; clamped to n_frames x trpx_worst_case_bytes and rounded up to 16.  0 for what the call does
 *                  not support
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  BAD EVENTS ARE DETECTED ON THE DEVICE, ALWAYS: a position >= n_values,
 *                  two neighbours of one frame not strictly ascending, row_offsets decreasing or ending beyond n_events each set
 *                  word 0 = TRPX_ERR_INVALID_ARG; out and frame_offsets are then unspecified.  TRPX_ERR_INVALID_ARG wins over
 *                  TRPX_ERR_CAPACITY when both apply.  This encoder has no waits between tiles: never TRPX_ERR_TIMEOUT
 *   workspace      DEVICE, 8-byte aligned, trpx_encode_sparse_workspace_bytes(): 16 bytes per 256-block tile + 8 per frame,
 *                  arithmetic on n_frames and the number of tiles, never proportional to n_values
 * Whatever the lists hold, nothing outside positions / values [0, n_events) and row_offsets[0 .. n_frames] is read and nothing
 * outside out[0, out_capacity), frame_offsets[0 .. n_frames], status and the workspace is written: rows are clamped to the
 * lists, and every scatter is guarded by its own range check.
 * NO DECODE INDEX IS PRODUCED: it is one byte per block, several times the stream this call writes.  A caller who wants one
 * runs trpx_build_index on the result.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block != 12, 64-bit containers, n_values >= 2^32 (positions
 * are 32-bit); TRPX_ERR_INVALID_ARG for an unknown or float dtype, zero sizes, null or misaligned pointers, the NULL / n_events
 * rule above, out NULL with a capacity; TRPX_ERR_CAPACITY for a workspace that is too small.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape is decided on the host
 * from n_frames, n_values and n_events alone, never from the contents of the lists: a captured call is replayed with new events
 * in the same buffers.
 * trpx_encode_sparse_host: host row_offsets / positions / values / out; checks its arguments AND the events on the host, before a
 * device is looked for (TRPX_ERR_INVALID_ARG for the four conditions above), stages, calls trpx_encode_sparse, synchronises;
 * *total_bytes, frame_offsets (or NULL) and *prolix_bits (or NULL) as trpx_encode_host.
 */
size_t trpx_encode_sparse_workspace_bytes(int dtype, size_t n_values, size_t n_frames, unsigned block);
size_t trpx_encode_sparse_bound_bytes(int dtype, size_t n_values, size_t n_frames, size_t n_events, unsigned block);
int trpx_encode_sparse(int dtype, const uint64_t* row_offsets, const uint32_t* positions, const void* values,
                       size_t n_events, size_t n_values, size_t n_frames, unsigned block,
                       uint8_t* out, size_t out_capacity, uint64_t* frame_offsets, uint32_t* status,
                       void* workspace, size_t workspace_bytes, void* stream);
int trpx_encode_sparse_host(int dtype, const uint64_t* row_offsets, const uint32_t* positions, const void* values,
                            size_t n_events, size_t n_values, size_t n_frames, unsigned block,
                            uint8_t* out, size_t out_capacity, size_t* total_bytes, uint64_t* frame_offsets,
                            uint32_t* prolix_bits, int device);

/*
 * Select frames of a stack into a new stack without decoding them: keep the hits, drop the blanks, reorder or repeat frames -- the
 * stack -> stack step behind trpx_decode_dot / trpx_decode_sparse and in front of everything that takes a stack.  Every frame
 * starts byte aligned and its stream does not depend on its neighbours (Terse.hpp:502-505, :359), so the stack of any list of
 * frames is the concatenation of those frames' bytes: out, out_offsets and the zeroed bytes [total, align4(total)) are byte for
 * byte what trpx_encode leaves for pixels[frames].  Only bytes move -- no pixel is decoded --, so the call takes every block in
 * 1..4096 and every integer dtype, 64-bit containers included; dtype, n_values and block matter only for the index.
 *   terse          DEVICE const uint8_t[terse_bytes], 4-byte aligned
 *   frame_offsets  DEVICE const uint64_t[n_frames + 1], 8-byte aligned, MANDATORY as for trpx_decode_indexed (an index-free stack:
 *                  trpx_locate_frames first)
 *   frames         DEVICE const uint32_t[n_select], 4-byte aligned: the list, in any order, repeats allowed, n_select may exceed
 *                  n_frames (a repeated frame makes the result larger than the source).  A device array on purpose: a picker on
 *                  the GPU feeds it, and a captured graph is replayed with a new list in the same buffer
 *   index, out_index
 *                  both or neither (one without the other: TRPX_ERR_INVALID_ARG); both need block 12 and a dtype of up to 32 bits
 *                  (TRPX_ERR_UNSUPPORTED otherwise).  index: the source's decode index; out_index: DEVICE, 16-byte aligned,
 *                  trpx_index_bytes(dtype, n_values, n_select, block): receives the widths row and the group-offset row of each
 *                  selected frame, and is accepted by trpx_decode_indexed and by every consumer of an index
 *   out_offsets    DEVICE uint64_t[n_select + 1], 8-byte aligned: [i] = first byte of the i-th selected frame, [n_select] = total
 *   out, out_capacity
 *                  as for trpx_encode (out 16-byte aligned).  A stack that does not fit: status word 0 = TRPX_ERR_CAPACITY,
 *                  out_offsets is still complete and valid, nothing at or behind out_capacity is touched; out_capacity ==
 *                  align4(total) is success.  A sizes-only query passes out = NULL with out_capacity 0 (status word 0 is then
 *                  TRPX_ERR_CAPACITY, as trpx_encode's).  out MUST NOT OVERLAP terse: in-place compaction is not supported
 *   status         DEVICE uint32_t[TRPX_STATUS_WORDS].  THE LIST AND THE OFFSETS ARE CHECKED ON THE DEVICE, ALWAYS: word 0 =
 *                  TRPX_ERR_INVALID_ARG for a list entry >= n_frames, TRPX_ERR_CORRUPT for a selected frame whose offsets
 *                  decrease or end beyond terse_bytes (CORRUPT where both occur).  Such a frame counts as empty in out_offsets,
 *                  and `out` (and out_index) are then not written.  Both win over TRPX_ERR_CAPACITY.  Word 1 is 0: the call
 *                  does not know prolix_bits
 *   workspace      DEVICE, 8-byte aligned, trpx_select_frames_workspace_bytes(): the selected sizes and the scan's scratch, 8
 *                  bytes per list entry + 4 per 256 of them -- arithmetic on n_frames and n_select, never proportional to the
 *                  bytes moved (0 for sizes the call refuses)
 * The stream is read in aligned 32-bit words: nothing outside terse[0 .. align4(terse_bytes)), frame_offsets[0 .. n_frames], frames
 * and the index is read, nothing outside out[0, out_capacity), out_offsets[0 .. n_select], out_index, status and the workspace is
 * written, whatever the lists hold.
 * Errors returned before any device call: TRPX_ERR_UNSUPPORTED for block outside 1..4096 and the index rule above;
 * TRPX_ERR_INVALID_ARG for an unknown or float dtype, zero sizes, n_select 0 or above 2^31 - 1, n_frames > terse_bytes, null or
 * misaligned pointers, out NULL with a capacity; TRPX_ERR_CAPACITY for a workspace that is too small.
 * Stream-ordered, no allocation, no host synchronisation (capturable into a HIP graph); every launch shape is decided on the host
 * from n_select, n_frames, terse_bytes and out_capacity alone, never from the list or the offsets.  No atomics touch the output:
 * bit-identical from run to run.
 * trpx_select_frames_host: host terse / frame_offsets / frames / out / out_offsets (or NULL); checks its arguments AND the list on
 * the host, before a device is looked for (TRPX_ERR_INVALID_ARG for an entry out of range, TRPX_ERR_CORRUPT for offsets that decrease
 * or leave the stream, TRPX_ERR_CAPACITY for out_capacity < total), stages, calls trpx_select_frames, synchronises; sets
 * *total_bytes.
 */
size_t trpx_select_frames_workspace_bytes(size_t n_frames, size_t n_select);
int trpx_select_frames(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, const void* index,
                       size_t n_values, size_t n_frames, unsigned block, const uint32_t* frames, size_t n_select,
                       uint8_t* out, size_t out_capacity, uint64_t* out_offsets, void* out_index,
                       uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int trpx_select_frames_host(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                            size_t n_values, size_t n_frames, unsigned block, const uint32_t* frames, size_t n_select,
                            uint8_t* out, size_t out_capacity, uint64_t* out_offsets, size_t* total_bytes, int device);

/*
 * synth-v1 frame generator (SURVEY.md section 8 row d) -- bench/test utility so that the GPU
 * box regenerates exactly the pixels the oracle anchors were computed on.  dtype U16 or I32.
 */
int trpx_synth_fill(int dtype, uint64_t seed, uint64_t frame0, size_t n_frames, size_t n_values,
                    void* pixels_dev, void* stream);

/*
 * Workspaces between calls.  The single-pass encoder polls and ORs into ~1 MB of descriptor words inside the caller's
 * workspace that have to be zero when it starts; its last kernel leaves them zero again, and the library REMEMBERS
 * (device, address, geometry) of the workspaces whose last user, as far as it can know, was such a call, and then skips the
 * clearing launch in front of the next one (7 us of a 270 us call).  What it cannot see is what others do to that memory,
 * hence the rule: between two trpx_encode* calls a workspace belongs to the library.  Whoever writes into it, frees it or
 * hands its address to something else calls trpx_workspace_invalidate(workspace, workspace_bytes) first (NULL, 0: every
 * workspace the library remembers).  Entry points of this library that are given the memory for another purpose (trpx_decode
 * with the same workspace, another geometry, the two-pass pipeline, the *_host entry points' own buffers) do so by themselves;
 * a call that is captured into a HIP graph always clears and neither reads nor writes what the library remembers (replays and
 * eager calls may alternate on one workspace); the device that is current at the call is the one the kernels run on and has
 * to own the workspace; and the encoder's first tile checks a tag it left in the workspace: a workspace that is not what the
 * library remembers makes the call report TRPX_ERR_TIMEOUT in the status block, which trpx_encode_checked and the host
 * wrappers answer with the two-pass pipeline (identical stream, none of these words).  Host-side, thread safe, no device call.
 */
int trpx_workspace_invalidate(const void* workspace, size_t workspace_bytes);

/*
 * Measured memory ceilings for the benchmark's roofline block (SURVEY.md section 8 row d): one grid-stride streaming
 * kernel over `bytes` bytes, 16 bytes per lane, non-temporal.  mode 0 = read `src` (dst: a 4-byte device sink),
 * 1 = write `dst`, 2 = copy src -> dst.  Device pointers, 16-byte aligned; stream-ordered.  Bench utility, not codec.
 * 3 = write `dst` from a 2-byte aligned address (the shape of the decoder's stores when a frame starts inside a cache line;
 * the benchmark reports it next to mode 1 as the ceiling of the kernels that keep such stores).
 */
int trpx_bench_stream(int mode, const void* src, void* dst, size_t bytes, void* stream);

/*
 * Encoder selection: 0 = auto (default: the single-pass look-back encoder), 1 = always the two-pass pipeline.
 * Process-wide; also settable with the environment variable TRPX_ENCODE_PATH=twopass.
 */
int trpx_set_encode_path(int path);

/*
 * Decoder selection (trpx_decode and the entry points built on it): 0 = auto (default: the per-frame decoder for
 * frames of < 2^26 bits -- block = 12, frame offsets given, any pixel count per frame, pointers aligned to the pixel
 * type only --, the position-parallel walk + tiled extraction for larger frames, the basic kernels for other block
 * sizes and missing frame offsets), 1 = always the basic kernels, 2 = the tiled route whenever its preconditions hold,
 * 3 = the per-frame decoder whenever its preconditions hold (= auto for trpx_decode; trpx_decode_indexed, which takes
 * it from 1024 frames on, then uses it for any number), 4 = large frames by round 4's parts route, 5 = auto with the
 * header-dense frames the per-frame decoder hands over walked by the dense walk (decode_dense.hip: one speculative pass,
 * link walks, a verified write pass) instead of the fix-point rounds of decode_seg.hip.  Every route yields the same
 * pixels (Terse.hpp:352-389); the setter exists for tests and A/B measurements.
 * Process-wide; also settable with the environment variable TRPX_DECODE_PATH=basic|tiles|frames|parts|dense.
 * Frames of more than 32 K blocks are cut into parts (one walk of many short parts, then extraction through the decode
 * index it yields; a stack the walk's own vote finds header-dense -- more than one block in six with an explicit header --
 * is walked one workgroup per frame, lane per segment, instead: decode_seg.hip, k_seg_wg) unless the stack holds 768 frames
 * or more, which keep them whole on the per-frame decoder -- such a
 * stack fills the GPU by itself; TRPX_SINGLE_PART=<frames>,<blocks> moves that line for tuning runs (stacks of <frames>
 * frames and more keep frames of up to <blocks> blocks whole).
 * These three variables and TRPX_LOCATE_PATH (trpx_set_locate_path) are the only ones the library reads; further switches exist in -DTRPX_DIAGNOSTICS builds only.
 * The tuned kernels issue 8- and 16-byte accesses at addresses that are only aligned to the pixel type (frames of any
 * pixel count): they rely on the HSA unaligned-access mode, which ROCm enables on gfx950.
 */
int trpx_set_decode_path(int path);

/*
 * trpx_encode_indexed + the one thing a stream-ordered call cannot do for itself: it waits for `stream`, reads the
 * status block and, if a look-back wait of the single-pass encoder gave up (TRPX_ERR_TIMEOUT: tiles wait for earlier
 * tiles of the same launch -- bounded to 0.25 s of wall time, never seen with in-order workgroup dispatch, but the
 * hardware does not promise it), runs the call again through the two-pass pipeline, which has no inter-tile waits and
 * writes the identical stream (f_compress is deterministic, Terse.hpp:500-549).  Returns the final status as its
 * return value (TRPX_OK = stack complete) and, if host_status is not NULL, the 8 status words.  `index` may be NULL.
 * Callers that stay asynchronous use trpx_encode and apply the same rule when they read the status block.
 */
int trpx_encode_checked(int dtype, const void* pixels, size_t n_values, size_t n_frames, unsigned block, uint8_t* out,
                        size_t out_capacity, uint64_t* frame_offsets, uint32_t* status, void* index, void* workspace,
                        size_t workspace_bytes, void* stream, uint32_t* host_status);

/*
 * Per-kernel timing for bench.py's roofline leg.  While enabled (per calling thread), trpx_encode /
 * trpx_decode record a hipEvent on `stream` before their first and after each of their kernels;
 * trpx_profile_read waits for the last launch and returns the elapsed ms of each stage
 * (single-pass encode: memset (k_zero_words), encode_fused, stitch; two-pass encode: tile_bits, frame_scan,
 * stack_scan, zero_edges, pack; per-frame decode: decode_frames, deferred_frames; tiled decode: walk, unpack).
 * Returns the number of stages written.  Not graph-capturable while enabled.
 */
int trpx_profile_enable(int on);
int trpx_profile_read(float* stage_ms, int capacity);

/* ---- stream-serialise surface: the ASCII header of Terse::write (Terse.hpp:454-474) and its
 * reader (Terse.hpp:485-498 over XML_element.hpp:216-224, :296-307).  Host only. ------------ */
typedef struct trpx_header {
    unsigned prolix_bits;
    int      is_signed;
    unsigned block;
    uint64_t memory_size;       /* payload bytes following the header            */
    uint64_t number_of_values;  /* per frame                                     */
    uint64_t number_of_frames;
    unsigned n_dims;            /* 0 = no `dimensions` attribute                 */
    uint64_t dims[8];
} trpx_header;

/* Writes the exact header text of Terse::write into buf (NUL-terminated); returns its length
 * (excluding the NUL) or 0 if buf_cap is too small. */
size_t trpx_header_format(const trpx_header* h, char* buf, size_t buf_cap);
/* Finds "<Terse" in data[0..len), parses the attributes (unknown ones are ignored, as the
 * reference does) and sets *payload_offset to the byte after "/>".  number_of_frames is
 * mandatory. */
int trpx_header_parse(const char* data, size_t len, trpx_header* h, size_t* payload_offset);

/* Frame index side-channel in the FILE.  The reference's file stores no frame sizes
 * (Terse.hpp:454-474), so a reader has to walk every frame's header chain just to find the next frame
 * (Terse.hpp:562-585).  trpx_header_format_indexed writes the same header with one more attribute,
 *   frame_sizes="S_0 S_1 ... S_{F-1}"      (bytes per frame, their sum = memory_size),
 * in front of number_of_frames.  The reference reader looks attributes up by name and ignores the others
 * (XML_element.hpp:296-307), so such a file stays readable by the reference tools; trpx_header_frame_sizes returns
 * the number of sizes found (0: no such attribute) and fills at most `capacity` of them.  Returns 0 / leaves buf
 * untouched if buf_cap is too small (2000 frames need ~14 KB). */
size_t trpx_header_format_indexed(const trpx_header* h, const uint64_t* frame_sizes, size_t n_sizes, char* buf, size_t buf_cap);
size_t trpx_header_frame_sizes(const char* data, size_t len, uint64_t* frame_sizes, size_t capacity);

/* Group states (row f1, second half): even with the frame sizes a reader has to walk each frame's header chain before it can
 * expand anything (Terse.hpp:360-372: a block's position is only known after the header of the block before it).  The chain
 * state at every 256th block -- bit offset inside the frame and width of the block before it, packed as
 * offset | width << 40 -- lets every 256-block group be walked on its own: trpx_group_count(n_values, 12) states per frame.
 *   trpx_index_group_states          reads them off a decode index (device);
 *   trpx_index_from_group_states     rebuilds the decode index from them (device, one lane per group) and checks every
 *                                    group against its successor's state and the frame's size (TRPX_ERR_CORRUPT);
 *   trpx_group_states_host           the states of a stack in host memory (what `terse -index` writes);
 *   trpx_decode_host_grouped         trpx_decode_host with the states: no walk; falls back to trpx_decode_host when the
 *                                    output type needs conversion or the states do not fit the stream;
 *   trpx_header_format_grouped       the header text with frame_sizes="..." and group_bit_offsets="o:w o:w ..." (~0.8 % of a
 *                                    synth-v1 stack's size; ignored by the reference reader like any unknown attribute,
 *                                    XML_element.hpp:296-307), trpx_header_group_states reads the attribute back. */
size_t trpx_group_count(size_t n_values, unsigned block);
int trpx_index_group_states(const void* index, size_t n_values, size_t n_frames, unsigned block, uint64_t* group_states, void* stream);
int trpx_index_from_group_states(int dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                                 const uint64_t* group_states, size_t n_values, size_t n_frames, unsigned block, void* index,
                                 uint32_t* status, void* stream);
int trpx_group_states_host(const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets, size_t n_values,
                           size_t n_frames, unsigned block, unsigned max_bits, uint64_t* group_states, int device);
int trpx_decode_host_grouped(int stream_signed, int out_dtype, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                             const uint64_t* group_states, size_t n_values, size_t n_frames, unsigned block, void* pixels_out,
                             int device);
size_t trpx_header_format_grouped(const trpx_header* h, const uint64_t* frame_sizes, size_t n_sizes, const uint64_t* group_states,
                                  size_t n_states, char* buf, size_t buf_cap);
size_t trpx_header_group_states(const char* data, size_t len, uint64_t* group_states, size_t capacity);

/* ---- host callers that work frame by frame ---------------------------------------------
 * src/prolix.cpp:69-92 expands a .trpx file with one `trpx_data.prolix(image, i)` per frame, src/terse.cpp:63-69 pushes
 * one image at a time.  The *_host entry points keep their device buffers per calling thread between calls (no
 * allocation per frame; trpx_host_release frees them).  For the expanding loop a stack object keeps the compressed stack
 * on the device: trpx_stack_open uploads it once (frame_offsets may be NULL: the frames are then located on that copy by
 * trpx_locate_frames, Terse.hpp:562-585, max_bits as in trpx_frame_offsets_host; group_states, if the file carried them, make the
 * expansion walk-free), trpx_stack_read(frame) expands a window of frames
 * starting at `frame` in ONE device call on a miss (<= 64 MB of pixels) and afterwards only copies the frame asked for
 * -- any output type of trpx_decode_host.  Not thread safe per object (the reference's prolix is not const either,
 * Terse.hpp:387-388). */
typedef struct trpx_stack trpx_stack;
int trpx_stack_open(trpx_stack** handle, int stream_signed, const uint8_t* terse, size_t terse_bytes, const uint64_t* frame_offsets,
                    const uint64_t* group_states /* may be NULL */, size_t n_values, size_t n_frames, unsigned block,
                    unsigned max_bits, int device);
int trpx_stack_read(trpx_stack* stack, size_t frame, int out_dtype, void* pixels_out);
void trpx_stack_close(trpx_stack* stack);
void trpx_host_release(void);

/* ---- multi-GPU (SURVEY.md section 8 row e): frames shard across GPUs, one process per GPU ----------------------
 * A frame's stream does not depend on its neighbours -- the header state resets per frame and every frame starts byte
 * aligned (Terse.hpp:502-505, :359) -- so rank r encodes its contiguous frame range with trpx_encode and keeps its
 * bytes.  What the serial encoder's cursor (Terse.hpp:502-504) would have been for the WHOLE stack is recovered by
 * the one collective of the path: trpx_gather_frame_offsets all-gathers the per-frame sizes (S_f, Terse.hpp:547) of
 * every rank over RCCL / xGMI (ncclAllGather, 8 bytes per frame) on `stream` and writes
 *   global_offsets[0 .. F_total]  byte offset of every frame of the global stack (ranks in order) + its total size,
 *   *prolix_bits                  maximum over the ranks' d_prolix_bits (Terse.hpp:516; encode_status = the status
 *                                 block trpx_encode filled, may be NULL), may be NULL,
 *   rank_base[0 .. world)         first byte of every rank's local stack inside the global one, may be NULL.
 * comm is an ncclComm_t of the caller (or one made by trpx_comm_init); n_slot >= every rank's n_local is the common
 * message size (shards may be ragged); all pointers are device pointers; stream-ordered, no host sync, no allocation.
 * The payload never crosses xGMI.  RCCL is resolved at run time (TRPX_ERR_UNSUPPORTED without it). */
size_t trpx_gather_workspace_bytes(size_t n_slot, int world);
int trpx_gather_frame_offsets(void* comm, const uint64_t* local_offsets, size_t n_local, size_t n_slot,
                              const uint32_t* encode_status, uint64_t* global_offsets, uint32_t* prolix_bits,
                              uint64_t* rank_base, void* workspace, size_t workspace_bytes, void* stream);
/* The two kernels of that call for callers that move the messages themselves (MPI, a host gather): trpx_gather_pack
 * writes this rank's message, u64[n_slot + 2] = { S_0 .. S_{n_local-1}, 0 .., n_local, prolix_bits }; trpx_gather_scan
 * turns the `world` messages, concatenated in rank order, into global_offsets / prolix_bits / rank_base as above. */
int trpx_gather_pack(const uint64_t* local_offsets, size_t n_local, size_t n_slot, const uint32_t* encode_status, uint64_t* message,
                     void* stream);
int trpx_gather_scan(const uint64_t* all_messages, int world, size_t n_slot, uint64_t* global_offsets, uint32_t* prolix_bits,
                     uint64_t* rank_base, void* stream);
/* One rank's share of a sharded stack in ONE stream-ordered call (SURVEY.md section 8 row b: trpx_encode_sharded /
 * trpx_decode_sharded).  trpx_encode_sharded = trpx_encode of this rank's n_local frames (f_compress on its share of the stack,
 * Terse.hpp:500-549; `out`, `local_offsets`, `status` exactly as trpx_encode leaves them) + trpx_gather_frame_offsets on the
 * caller's communicator (`global_offsets`, `prolix_bits`, `rank_base` as above).  gather_stream: NULL -- the gather follows the
 * encode on `stream`; another stream of the same device -- the gather runs there, ordered behind the encode by an event, so
 * that what the caller enqueues on `stream` next (the decode of its own frames needs no global offset) overlaps the collective;
 * the caller joins the two streams where it reads the table.  workspace: trpx_encode_sharded_workspace_bytes().
 * trpx_decode_sharded expands this rank's frames -- frames [first_frame, first_frame + n_local) of the global stack, whose
 * bytes it holds as `local_terse` -- from the GLOBAL offset table (prolix(it, frame) for its share, Terse.hpp:352-389; frames
 * are independent, Terse.hpp:502-505): no collective, one small kernel in front of trpx_decode.  Errors of both:
 * trpx_shard_last_error(). */
size_t trpx_encode_sharded_workspace_bytes(int dtype, size_t n_values, size_t n_local, size_t n_slot, unsigned block, int world);
int trpx_encode_sharded(void* comm, int dtype, const void* pixels, size_t n_values, size_t n_local, size_t n_slot, unsigned block,
                        uint8_t* out, size_t out_capacity, uint64_t* local_offsets, uint32_t* status, uint64_t* global_offsets,
                        uint32_t* prolix_bits, uint64_t* rank_base, void* workspace, size_t workspace_bytes, void* stream,
                        void* gather_stream);
size_t trpx_decode_sharded_workspace_bytes(int dtype, size_t n_values, size_t n_local, unsigned block);
int trpx_decode_sharded(int stream_signed, int out_dtype, const uint8_t* local_terse, size_t local_bytes, const uint64_t* global_offsets,
                        size_t first_frame, size_t n_values, size_t n_local, unsigned block, void* pixels_out, uint32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream);
/* A communicator for callers that have none: rank 0 makes the 128-byte id, every rank gets it by its own means
 * (MPI, torch.distributed, a file) and calls trpx_comm_init with the GPU it will use already selected. */
int trpx_comm_unique_id(void* id128);
int trpx_comm_init(void** comm, int world, int rank, const void* id128);
int trpx_comm_destroy(void* comm);
/* What RCCL itself says about a communicator (ncclCommCount / ncclCommUserRank): a caller that reports a sharded run can state
 * how many ranks the size gather really spanned.  Either pointer may be NULL. */
int trpx_comm_info(void* comm, int* world, int* rank);
const char* trpx_shard_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TRPX_HIP_H */
