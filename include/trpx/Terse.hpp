// trpx::Terse -- C++ host-side mirror of the reference class jpa::Terse
// (senikm/trpx include/Terse.hpp:228-475) whose encode / decode bodies run on the MI355X through
// the C ABI of libtrpx_hip.so (include/trpx_hip.h).  Same constructors, push_back, prolix,
// accessors and write()/stream constructor, same argument meaning; a caller written against
// jpa::Terse (e.g. src/terse.cpp:107-125, src/prolix.cpp:69-92) compiles against this class after
// `namespace jpa = trpx;`.
//
// Deliberate differences:
//   * frames are located by the running sum of their sizes -- the intended semantics of
//     Terse.hpp:562-585 (reference defects D1/D2 make its own multi-frame decode wrong);
//   * argument errors throw std::invalid_argument where the reference assert()s (compiled out in
//     its Release build, CMakeLists.txt:13); device/runtime failures throw std::runtime_error;
//   * push_back(Iterator, size, n_frames) encodes a whole stack in one GPU call (the reference's
//     per-frame push_back is O(F^2), defect D6);
//   * pixel types: u8/i8/u16/i16/u32/i32 (src/terse.cpp:113-118) on the tuned kernels; 64-bit integers (what
//     src/terse.cpp:120-123 makes of float / double images) are narrowed when every value fits 32 bits (the stream is then
//     the same) and go through as 64-bit pixels otherwise (generic kernels, no decode index).
#ifndef TRPX_TERSE_HPP
#define TRPX_TERSE_HPP

#include <cstdint>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <numeric>
#include <span>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../trpx_hip.h"

namespace trpx {

namespace detail {
template <typename T> constexpr int dtype_of() {
    static_assert(std::is_integral_v<T> && sizeof(T) <= 8, "trpx::Terse: pixel type must be an integer of <= 64 bits");
    return (sizeof(T) == 1 ? TRPX_U8 : sizeof(T) == 2 ? TRPX_U16 : sizeof(T) == 4 ? TRPX_U32 : TRPX_U64) + (std::is_signed_v<T> ? 1 : 0);
}
// output types of prolix(): the pixel types plus float / double (Terse.hpp:379-383)
template <typename T> constexpr int out_dtype_of() {
    if constexpr (std::is_same_v<T, float>) return TRPX_F32;
    else if constexpr (std::is_same_v<T, double>) return TRPX_F64;
    else return dtype_of<T>();
}
// The header and the library it calls must be of one ABI version (opaque buffer layouts change between versions).
inline void require_abi() {
    static const bool ok = [] {
        if (trpx_abi_version() != TRPX_ABI_VERSION)
            throw std::runtime_error("libtrpx_hip.so ABI version " + std::to_string(trpx_abi_version()) + " != header's " +
                                     std::to_string(TRPX_ABI_VERSION));
        return true;
    }();
    (void)ok;
}
inline void check(int rc, const char* what) {
    if (rc == TRPX_OK) return;
    std::string msg = std::string(what) + ": " + trpx_last_error_string();
    if (rc == TRPX_ERR_INVALID_ARG || rc == TRPX_ERR_UNSUPPORTED) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}
}  // namespace detail

class Terse {
public:
    /// Empty object; the first pushed frame fixes size and signedness (Terse.hpp:237).
    Terse() {}

    /// From a container of integral values; captures data.dim() if present (Terse.hpp:249-253).
    template <typename Container>
        requires(requires(Container c) { c.begin(); c.size(); })
    Terse(Container const& data) : Terse(data.begin(), data.size()) {
        if constexpr (requires(Container & c) { c.dim(); })
            for (auto d : data.dim()) d_dim.push_back(d);
    }

    /// From an iterator/pointer and a size (Terse.hpp:263-270).
    template <typename Iterator>
    Terse(Iterator const data, std::size_t const size, unsigned int const block = 12)
        : d_signed(std::is_signed_v<typename std::iterator_traits<Iterator>::value_type>), d_block(block), d_size(size) {
        f_compress(data, 1);
    }

    /// Reads a Terse object written by write() / the reference (Terse.hpp:279, :485-498).
    explicit Terse(std::ifstream& istream) { f_read(istream); }

    /// Copyable and movable like the reference's class (Terse.hpp:228-475 declares neither: the compiler's apply).  The
    /// device-side copy of the stack (prolix(it, frame)) is never shared: a copy starts without one, a move takes it over.
    Terse(Terse const& o)
        : d_signed(o.d_signed), d_block(o.d_block), d_size(o.d_size), d_prolix_bits(o.d_prolix_bits), d_dim(o.d_dim),
          d_terse_data(o.d_terse_data), d_frame_sizes(o.d_frame_sizes), d_group_states(o.d_group_states) {}
    Terse(Terse&& o) noexcept
        : d_signed(o.d_signed), d_block(o.d_block), d_size(o.d_size), d_prolix_bits(o.d_prolix_bits), d_dim(std::move(o.d_dim)),
          d_terse_data(std::move(o.d_terse_data)), d_frame_sizes(std::move(o.d_frame_sizes)), d_stack(o.d_stack),
          d_group_states(std::move(o.d_group_states)) {
        o.d_stack = nullptr;
    }
    Terse& operator=(Terse const& o) {
        if (this != &o) { Terse tmp(o); swap(tmp); }
        return *this;
    }
    Terse& operator=(Terse&& o) noexcept {
        if (this != &o) { swap(o); o.f_drop_stack(); }
        return *this;
    }
    ~Terse() { f_drop_stack(); }
    void swap(Terse& o) noexcept {
        std::swap(d_signed, o.d_signed); std::swap(d_block, o.d_block); std::swap(d_size, o.d_size);
        std::swap(d_prolix_bits, o.d_prolix_bits); d_dim.swap(o.d_dim); d_terse_data.swap(o.d_terse_data);
        d_frame_sizes.swap(o.d_frame_sizes); std::swap(d_stack, o.d_stack); d_group_states.swap(o.d_group_states);
    }

    /// Appends one frame (Terse.hpp:290-302).
    template <typename Iterator>
    void push_back(Iterator const data, std::size_t const size) { push_back(data, size, 1); }

    /// Appends n_frames contiguous frames of `size` values each in ONE device call.
    template <typename Iterator>
    void push_back(Iterator const data, std::size_t const size, std::size_t const n_frames) {
        using V = typename std::iterator_traits<Iterator>::value_type;
        if (number_of_frames() == 0) {
            d_size = size;
            d_signed = std::is_signed_v<V>;
        } else {
            if (this->size() != size) throw std::invalid_argument("each frame of a multi-Terse object must have the same size");
            if (d_signed != std::is_signed_v<V>) throw std::invalid_argument("signedness differs from the first frame");
        }
        f_compress(data, n_frames);
    }

    /// Appends one frame given as a container (Terse.hpp:312-322).
    template <typename Container>
        requires requires(Container& c) { c.begin(), c.end(), c.size(); }
    void push_back(Container const& data) {
        if constexpr (requires(Container & c) { c.dim(); }) {
            for (std::size_t i = 0; i != data.dim().size(); ++i)
                if (number_of_frames() == 0) d_dim.push_back(data.dim()[i]);
                else if (d_dim[i] != data.dim()[i]) throw std::invalid_argument("frame dimensions differ");
        }
        push_back(data.begin(), data.size());
    }

    /// Unpacks a frame into a container, checking its size (Terse.hpp:333-341).
    template <typename Container>
        requires requires(Container& c) { c.begin(), c.end(), c.size(); }
    void prolix(Container& data, std::size_t frame = 0) {
        if (this->size() != data.size()) throw std::invalid_argument("prolix: container has the wrong size");
        prolix(data.begin(), frame);
    }

    /// Unpacks a frame to `begin` (Terse.hpp:352-389).  The output type is free: narrower integers clamp
    /// (Bit_pointer.hpp:747-763), float / double are exact (:379-383), unsigned data into a signed type keeps
    /// the value (the reference sign-extends wrongly there).
    template <typename Iterator>
        requires requires(Iterator& i) { *i; }
    void prolix(Iterator begin, std::size_t frame = 0) {
        using V = typename std::iterator_traits<Iterator>::value_type;
        if (frame >= number_of_frames()) throw std::invalid_argument("prolix: frame index out of range");
        if (d_signed && std::is_unsigned_v<V>)
            throw std::invalid_argument("signed data cannot be decompressed into unsigned data");
        std::vector<V> tmp;
        V* dst;
        if constexpr (std::is_pointer_v<Iterator>) dst = begin;
        else { tmp.resize(d_size); dst = tmp.data(); }
        // src/prolix.cpp:69-92 calls this once per frame: the compressed stack is uploaded once and kept on the device
        // (trpx_stack_*), a window of frames is expanded per device call, a call normally only copies its frame back
        if (!d_stack) {
            detail::require_abi();
            std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
            for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
            detail::check(trpx_stack_open(&d_stack, d_signed, d_terse_data.data(), d_terse_data.size(), offs.data(), f_states(), d_size,
                                          d_frame_sizes.size(), d_block, 0, -1), "Terse::prolix");
        }
        detail::check(trpx_stack_read(d_stack, frame, detail::out_dtype_of<V>(), dst), "Terse::prolix");
        if constexpr (!std::is_pointer_v<Iterator>) std::copy(tmp.begin(), tmp.end(), begin);
    }

    /// Unpacks EVERY frame into `out` (number_of_frames() x size() values) in one device call -- what src/prolix.cpp's
    /// per-frame loop (:69-92) amounts to.
    template <typename V>
    void prolix_all(V* out) {
        if (d_signed && std::is_unsigned_v<V>)
            throw std::invalid_argument("signed data cannot be decompressed into unsigned data");
        if (d_frame_sizes.empty()) return;
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        detail::check(trpx_decode_host_grouped(d_signed, detail::out_dtype_of<V>(), d_terse_data.data(), d_terse_data.size(), offs.data(),
                                               f_states(), d_size, d_frame_sizes.size(), d_block, out, -1), "Terse::prolix_all");
    }

    /// Sums of `group` consecutive frames into `out` (ceil(number_of_frames() / group) x size() values) in one device call,
    /// without expanding the frames (trpx_decode_sum_host).  A group that does not divide the frame count leaves a shorter last
    /// group.  V: int32 / uint32 (clamped), int64 / uint64 (exact), float / double (the exact sum rounded once).
    template <typename V>
    void prolix_sum(V* out, std::size_t group) {
        static_assert(std::is_same_v<V, std::int32_t> || std::is_same_v<V, std::uint32_t> || std::is_same_v<V, std::int64_t> ||
                          std::is_same_v<V, std::uint64_t> || std::is_same_v<V, float> || std::is_same_v<V, double>,
                      "prolix_sum: int32, uint32, int64, uint64, float or double sums");
        if (d_signed && std::is_unsigned_v<V>)
            throw std::invalid_argument("signed data cannot be decompressed into unsigned data");
        if (group == 0) throw std::invalid_argument("prolix_sum: group must be at least 1");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_sum: values of more than 32 bits are not supported");
        if (d_frame_sizes.empty()) return;
        group = std::min(group, d_frame_sizes.size());
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        const int bits = d_prolix_bits <= 8 ? TRPX_U8 : d_prolix_bits <= 16 ? TRPX_U16 : TRPX_U32;   // the narrowest stream type
        detail::check(trpx_decode_sum_host(bits + (d_signed ? 1 : 0), detail::out_dtype_of<V>(), d_terse_data.data(),
                                           d_terse_data.size(), offs.data(), d_size, d_frame_sizes.size(), d_block,
                                           (unsigned)group, out, -1), "Terse::prolix_sum");
    }

    /// Sums of the frames that carry the same label into `out` (n_out x size() values) in one device call, without expanding the
    /// frames (trpx_decode_sum_labelled_host).  labels: number_of_frames() of them; frame f is added into output labels[f], a label
    /// >= n_out (by convention 0xFFFFFFFF) takes the frame out of every sum.  An output without frames is 0.  counts: n_out values,
    /// the frames of every output, or nullptr.  V and the refusals: prolix_sum's.  An object without frames writes nothing.
    template <typename V>
    void prolix_sum_labelled(V* out, const std::uint32_t* labels, std::size_t n_out, std::uint32_t* counts = nullptr) {
        static_assert(std::is_same_v<V, std::int32_t> || std::is_same_v<V, std::uint32_t> || std::is_same_v<V, std::int64_t> ||
                          std::is_same_v<V, std::uint64_t> || std::is_same_v<V, float> || std::is_same_v<V, double>,
                      "prolix_sum_labelled: int32, uint32, int64, uint64, float or double sums");
        if (d_signed && std::is_unsigned_v<V>)
            throw std::invalid_argument("signed data cannot be decompressed into unsigned data");
        if (n_out == 0) throw std::invalid_argument("prolix_sum_labelled: n_out must be at least 1");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_sum_labelled: values of more than 32 bits are not supported");
        if (d_frame_sizes.empty()) return;
        if (!labels) throw std::invalid_argument("prolix_sum_labelled: no labels");
        detail::require_abi();
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        const int bits = d_prolix_bits <= 8 ? TRPX_U8 : d_prolix_bits <= 16 ? TRPX_U16 : TRPX_U32;   // the narrowest stream type
        detail::check(trpx_decode_sum_labelled_host(bits + (d_signed ? 1 : 0), detail::out_dtype_of<V>(), d_terse_data.data(),
                                                    d_terse_data.size(), offs.data(), d_size, d_frame_sizes.size(), d_block, labels,
                                                    n_out, out, counts, -1), "Terse::prolix_sum_labelled");
    }

    /// Per pixel, one statistic over `group` consecutive frames into `out` (ceil(number_of_frames() / group) x size() values) in
    /// one device call, without expanding the frames (trpx_decode_reduce_host).  op: TRPX_REDUCE_MAX / TRPX_REDUCE_MIN -- V is the
    /// narrowest integer type that holds the object's values ((u)int8_t for bits_per_val() <= 8, (u)int16_t for <= 16, (u)int32_t
    /// for <= 32, signed as is_signed()); TRPX_REDUCE_SUMSQ -- V is uint64_t, the sum of squares modulo 2^64;
    /// TRPX_REDUCE_COUNT_GE -- V is uint32_t, the frames with pixel >= threshold.  A V that is not what the op writes throws.
    template <typename V>
    void prolix_reduce(V* out, int op, std::size_t group, std::int64_t threshold = 0) {
        static_assert(std::is_integral_v<V> && !std::is_same_v<V, bool> && (sizeof(V) <= 4 || std::is_same_v<V, std::uint64_t>),
                      "prolix_reduce: the pixel type (max, min), uint64_t (sum of squares) or uint32_t (count)");
        if (op < TRPX_REDUCE_MAX || op > TRPX_REDUCE_COUNT_GE) throw std::invalid_argument("prolix_reduce: unknown op");
        if (group == 0) throw std::invalid_argument("prolix_reduce: group must be at least 1");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_reduce: values of more than 32 bits are not supported");
        const int bits = d_prolix_bits <= 8 ? TRPX_U8 : d_prolix_bits <= 16 ? TRPX_U16 : TRPX_U32;   // the narrowest stream type
        const int dtype = bits + (d_signed ? 1 : 0);
        const bool fits = op == TRPX_REDUCE_SUMSQ      ? std::is_same_v<V, std::uint64_t>
                          : op == TRPX_REDUCE_COUNT_GE ? std::is_same_v<V, std::uint32_t>
                                                       : sizeof(V) == trpx_dtype_size(dtype) && std::is_signed_v<V> == (d_signed != 0);
        if (!fits) throw std::invalid_argument("prolix_reduce: the output type is not what the op writes for this object");
        if (d_frame_sizes.empty()) return;
        detail::require_abi();
        group = std::min(group, d_frame_sizes.size());
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        detail::check(trpx_decode_reduce_host(dtype, op, d_terse_data.data(), d_terse_data.size(), offs.data(), d_size,
                                              d_frame_sizes.size(), d_block, (unsigned)group, threshold, out, -1), "Terse::prolix_reduce");
    }

    /// Every frame summed over bins of bin_y x bin_x neighbouring pixels into `out` (number_of_frames() x ceil(height / bin_y) x
    /// ceil(width / bin_x) values, frame by frame, row by row) in one device call, without expanding the frames
    /// (trpx_decode_binned_host).  dim() = {width, height} must be set; a bin side is 1 .. 64 and no larger than the frame's; the
    /// edge bins sum the pixels that exist.  V: int32 / uint32 (clamped), int64 / uint64 (exact), float / double (the exact sum
    /// rounded once).
    template <typename V>
    void prolix_binned(V* out, std::size_t bin_y, std::size_t bin_x) {
        static_assert(std::is_same_v<V, std::int32_t> || std::is_same_v<V, std::uint32_t> || std::is_same_v<V, std::int64_t> ||
                          std::is_same_v<V, std::uint64_t> || std::is_same_v<V, float> || std::is_same_v<V, double>,
                      "prolix_binned: int32, uint32, int64, uint64, float or double sums");
        if (d_signed && std::is_unsigned_v<V>)
            throw std::invalid_argument("signed data cannot be decompressed into unsigned data");
        if (d_dim.size() != 2 || d_dim[0] * d_dim[1] != d_size) throw std::invalid_argument("prolix_binned: dim() must be {width, height} of the frames");
        const std::size_t width = d_dim[0], height = d_dim[1];
        if (bin_y == 0 || bin_x == 0 || bin_y > 64 || bin_x > 64 || bin_y > height || bin_x > width)
            throw std::invalid_argument("prolix_binned: a bin side is 1 to 64 and no larger than the frame's");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_binned: values of more than 32 bits are not supported");
        if (d_frame_sizes.empty()) return;
        detail::require_abi();
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        const int bits = d_prolix_bits <= 8 ? TRPX_U8 : d_prolix_bits <= 16 ? TRPX_U16 : TRPX_U32;   // the narrowest stream type
        detail::check(trpx_decode_binned_host(bits + (d_signed ? 1 : 0), detail::out_dtype_of<V>(), d_terse_data.data(),
                                              d_terse_data.size(), offs.data(), d_size, d_frame_sizes.size(), d_block, width,
                                              (unsigned)bin_y, (unsigned)bin_x, out, -1), "Terse::prolix_binned");
    }
    template <typename V = std::int32_t>
    std::vector<V> prolix_binned(std::size_t bin_y, std::size_t bin_x) {
        if (d_dim.size() != 2 || bin_y == 0 || bin_x == 0) throw std::invalid_argument("prolix_binned: dim() must be set, a bin side is at least 1");
        std::vector<V> out(d_frame_sizes.size() * ((d_dim[1] + bin_y - 1) / bin_y) * ((d_dim[0] + bin_x - 1) / bin_x));
        prolix_binned(out.data(), bin_y, bin_x);
        return out;
    }

    /// The rectangle [y0, y0 + h) x [x0, x0 + w) of frames [first_frame, first_frame + n_frames) to `out` (n_frames x h x w
    /// values, frame by frame, row by row) in one device call, without expanding whole frames (trpx_decode_roi_host).
    /// dim() = {width, height} must be set.  The value type of `out` is the narrowest integer type that holds the object's
    /// values: (u)int8_t for bits_per_val() <= 8, (u)int16_t for <= 16, (u)int32_t for <= 32, signed as is_signed().
    template <typename Iterator>
        requires requires(Iterator& i) { *i; }
    void prolix_roi(Iterator out, std::size_t y0, std::size_t x0, std::size_t h, std::size_t w, std::size_t first_frame = 0,
                    std::size_t n_frames = std::size_t(-1)) {
        using V = typename std::iterator_traits<Iterator>::value_type;
        static_assert(std::is_integral_v<V> && sizeof(V) <= 4, "prolix_roi: an integer type of at most 32 bits");
        if (d_dim.size() != 2 || d_dim[0] * d_dim[1] != d_size) throw std::invalid_argument("prolix_roi: dim() must be {width, height} of the frames");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_roi: values of more than 32 bits are not supported");
        const unsigned bits = d_prolix_bits <= 8 ? 8 : d_prolix_bits <= 16 ? 16 : 32;
        if (8 * sizeof(V) != bits || std::is_signed_v<V> != d_signed)
            throw std::invalid_argument("prolix_roi: the output type must be the narrowest integer type that holds the values");
        if (first_frame > number_of_frames()) throw std::invalid_argument("prolix_roi: frame index out of range");
        n_frames = std::min(n_frames, number_of_frames() - first_frame);
        const std::size_t width = d_dim[0], height = d_dim[1];
        if (h == 0 || w == 0 || y0 > height || h > height - y0 || x0 > width || w > width - x0)
            throw std::invalid_argument("prolix_roi: the rectangle leaves the frame");
        if (n_frames == 0) return;
        detail::require_abi();
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        std::vector<std::uint32_t> boxes;
        for (std::size_t f = 0; f < n_frames; ++f) boxes.insert(boxes.end(), {std::uint32_t(first_frame + f), std::uint32_t(y0), std::uint32_t(x0)});
        std::vector<V> tmp;
        V* dst;
        if constexpr (std::is_pointer_v<Iterator>) dst = out;
        else { tmp.resize(n_frames * h * w); dst = tmp.data(); }
        detail::check(trpx_decode_roi_host(detail::dtype_of<V>(), d_terse_data.data(), d_terse_data.size(), offs.data(), d_size,
                                           d_frame_sizes.size(), d_block, width, boxes.data(), n_frames, (unsigned)h, (unsigned)w, dst, -1),
                      "Terse::prolix_roi");
        if constexpr (!std::is_pointer_v<Iterator>) std::copy(tmp.begin(), tmp.end(), out);
    }

    /// The pixels with value >= threshold of every frame, in CSR form, in two device calls (sizes, then events) without
    /// expanding the frames (trpx_decode_sparse_host): row_offsets[f] = events in the frames < f (number_of_frames() + 1
    /// entries), positions[i] = the pixel index of event i inside its frame, values[i] = its value; by frame, then by pixel.
    /// T is the narrowest integer type that holds the object's values, as for prolix_roi.
    template <typename T>
    void prolix_sparse(std::int64_t threshold, std::vector<std::uint64_t>& row_offsets, std::vector<std::uint32_t>& positions,
                       std::vector<T>& values) {
        static_assert(std::is_integral_v<T> && sizeof(T) <= 4, "prolix_sparse: an integer type of at most 32 bits");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_sparse: values of more than 32 bits are not supported");
        const unsigned bits = d_prolix_bits <= 8 ? 8 : d_prolix_bits <= 16 ? 16 : 32;
        if (8 * sizeof(T) != bits || std::is_signed_v<T> != d_signed)
            throw std::invalid_argument("prolix_sparse: the value type must be the narrowest integer type that holds the values");
        row_offsets.assign(d_frame_sizes.size() + 1, 0);
        positions.clear();
        values.clear();
        if (d_frame_sizes.empty()) return;
        detail::require_abi();
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        std::size_t found = 0;
        int rc = trpx_decode_sparse_host(detail::dtype_of<T>(), d_terse_data.data(), d_terse_data.size(), offs.data(), d_size,
                                         d_frame_sizes.size(), d_block, threshold, row_offsets.data(), nullptr, nullptr, 0, &found, -1);
        if (rc != TRPX_ERR_CAPACITY) detail::check(rc, "Terse::prolix_sparse");   // (CAPACITY: there are events, `found` of them)
        if (found == 0) return;
        positions.resize(found);
        values.resize(found);
        detail::check(trpx_decode_sparse_host(detail::dtype_of<T>(), d_terse_data.data(), d_terse_data.size(), offs.data(), d_size,
                                              d_frame_sizes.size(), d_block, threshold, row_offsets.data(), positions.data(), values.data(),
                                              found, &found, -1), "Terse::prolix_sparse");
    }

    /// Per frame the sums of its pixels weighted by n_maps integer maps, in one device call, without expanding the frames
    /// (trpx_decode_dot_host): weights = n_maps x size() values, map after map; out[f * n_maps + k] = sum_p px[f][p] *
    /// weights[k * size() + p] in int64, modulo 2^64.  A mask gives a virtual detector image, the maps x, y and 1 the centre
    /// of mass.  1 <= n_maps <= 16.
    void prolix_dot(std::int32_t const* weights, std::size_t n_maps, std::int64_t* out) {
        if (n_maps == 0 || n_maps > 16) throw std::invalid_argument("prolix_dot: 1 to 16 maps");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_dot: values of more than 32 bits are not supported");
        if (d_frame_sizes.empty()) return;
        detail::require_abi();
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        const int bits = d_prolix_bits <= 8 ? TRPX_U8 : d_prolix_bits <= 16 ? TRPX_U16 : TRPX_U32;   // the narrowest stream type
        detail::check(trpx_decode_dot_host(bits + (d_signed ? 1 : 0), d_terse_data.data(), d_terse_data.size(), offs.data(), d_size,
                                           d_frame_sizes.size(), d_block, weights, (unsigned)n_maps, out, -1), "Terse::prolix_dot");
    }
    std::vector<std::int64_t> prolix_dot(std::vector<std::int32_t> const& weights, std::size_t n_maps) {
        if (n_maps == 0 || weights.size() != n_maps * d_size) throw std::invalid_argument("prolix_dot: weights must hold n_maps x size() values");
        std::vector<std::int64_t> out(d_frame_sizes.size() * n_maps);
        prolix_dot(weights.data(), n_maps, out.data());
        return out;
    }

    /// Per frame the sums of its pixels over the bins of a label map, in one device call, without expanding the frames
    /// (trpx_decode_bins_host): labels = size() values, one per pixel; out[f * n_bins + b] = the sum of px[f][p] over the pixels
    /// with labels[p] == b, in int64, exact.  A label >= n_bins belongs to no bin (mask with 0xFFFF).  The radial profile of
    /// every frame.  1 <= n_bins <= 4096.
    void prolix_bins(std::uint16_t const* labels, std::size_t n_bins, std::int64_t* out) {
        if (n_bins == 0 || n_bins > 4096) throw std::invalid_argument("prolix_bins: 1 to 4096 bins");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_bins: values of more than 32 bits are not supported");
        if (d_frame_sizes.empty()) return;
        detail::require_abi();
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        const int bits = d_prolix_bits <= 8 ? TRPX_U8 : d_prolix_bits <= 16 ? TRPX_U16 : TRPX_U32;   // the narrowest stream type
        detail::check(trpx_decode_bins_host(bits + (d_signed ? 1 : 0), d_terse_data.data(), d_terse_data.size(), offs.data(), d_size,
                                            d_frame_sizes.size(), d_block, labels, (unsigned)n_bins, out, -1), "Terse::prolix_bins");
    }
    std::vector<std::int64_t> prolix_bins(std::vector<std::uint16_t> const& labels, std::size_t n_bins) {
        if (labels.size() != d_size) throw std::invalid_argument("prolix_bins: labels must hold size() values");
        if (n_bins == 0 || n_bins > 4096) throw std::invalid_argument("prolix_bins: 1 to 4096 bins");
        std::vector<std::int64_t> out(d_frame_sizes.size() * n_bins);
        prolix_bins(labels.data(), n_bins, out.data());
        return out;
    }

    /// Per group of `group` consecutive frames the histogram of its pixel values, in one device call, without expanding the
    /// frames (trpx_decode_hist_host): out[g * n_bins + b] = the number of pixels of group g with bin(v) == b,
    /// bin(v) = clamp(floor((v - lo) / 2^shift), 0, n_bins - 1) -- the first and the last bin take everything below and above,
    /// so every row sums to size() x the group's frames.  The last group holds what is left.  group >= 1, 1 <= n_bins <= 4096,
    /// shift <= 32, |lo| <= 2^32.
    std::vector<std::uint64_t> prolix_hist(std::size_t group, std::int64_t lo, unsigned shift, std::size_t n_bins) {
        if (n_bins == 0 || n_bins > 4096) throw std::invalid_argument("prolix_hist: 1 to 4096 bins");
        if (group == 0) throw std::invalid_argument("prolix_hist: group >= 1");
        if (shift > 32 || lo > (std::int64_t(1) << 32) || lo < -(std::int64_t(1) << 32))
            throw std::invalid_argument("prolix_hist: shift <= 32 and |lo| <= 2^32");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_hist: values of more than 32 bits are not supported");
        const std::size_t f = d_frame_sizes.size();
        if (f == 0) return {};
        detail::require_abi();
        std::vector<std::uint64_t> out((f + std::min(group, f) - 1) / std::min(group, f) * n_bins);
        std::vector<std::uint64_t> offs(f + 1, 0);
        for (std::size_t i = 0; i < f; ++i) offs[i + 1] = offs[i] + d_frame_sizes[i];
        const int bits = d_prolix_bits <= 8 ? TRPX_U8 : d_prolix_bits <= 16 ? TRPX_U16 : TRPX_U32;   // the narrowest stream type
        detail::check(trpx_decode_hist_host(bits + (d_signed ? 1 : 0), d_terse_data.data(), d_terse_data.size(), offs.data(), d_size, f,
                                            d_block, group, lo, shift, (unsigned)n_bins, out.data(), -1), "Terse::prolix_hist");
        return out;
    }

    /// Frames [first_frame, first_frame + n_frames) (clipped to the stack) as float32 with the dark reference subtracted and the
    /// gain reference multiplied in, in one device call (trpx_decode_corrected_host): out[f * size() + p] =
    /// ((float) px[f][p] - dark[p]) * gain[p], three float operations in this order, each rounded once; subnormal results are
    /// unspecified.  dark / gain: size() values, or nullptr to leave the operation out (both: a plain float decode).
    std::vector<float> prolix_corrected(const float* dark, const float* gain, std::size_t first_frame = 0,
                                        std::size_t n_frames = static_cast<std::size_t>(-1)) {
        if (first_frame > number_of_frames()) throw std::invalid_argument("prolix_corrected: frame index out of range");
        if (d_prolix_bits > 32) throw std::invalid_argument("prolix_corrected: values of more than 32 bits are not supported");
        n_frames = std::min(n_frames, number_of_frames() - first_frame);
        if (n_frames == 0) return {};
        detail::require_abi();
        std::vector<float> out(n_frames * d_size);
        std::size_t start = 0;
        for (std::size_t i = 0; i < first_frame; ++i) start += d_frame_sizes[i];
        std::vector<std::uint64_t> offs(n_frames + 1, 0);
        for (std::size_t i = 0; i < n_frames; ++i) offs[i + 1] = offs[i] + d_frame_sizes[first_frame + i];
        const int bits = d_prolix_bits <= 8 ? TRPX_U8 : d_prolix_bits <= 16 ? TRPX_U16 : TRPX_U32;   // the narrowest stream type
        detail::check(trpx_decode_corrected_host(bits + (d_signed ? 1 : 0), TRPX_F32, d_terse_data.data() + start, offs[n_frames], offs.data(), d_size,
                                                 n_frames, d_block, dark, gain, out.data(), -1), "Terse::prolix_corrected");
        return out;
    }
    std::vector<float> prolix_corrected(std::vector<float> const& dark, std::vector<float> const& gain, std::size_t first_frame = 0,
                                        std::size_t n_frames = static_cast<std::size_t>(-1)) {
        if (dark.size() != d_size || gain.size() != d_size) throw std::invalid_argument("prolix_corrected: dark and gain must hold size() values");
        return prolix_corrected(dark.data(), gain.data(), first_frame, n_frames);
    }

    /// A new object holding the frames `frames` of this one -- any order, repeats allowed, possibly more than the stack has --
    /// in one device call, without decoding them (trpx_select_frames_host): the frames' bytes are copied, so the result is
    /// what push_back of those frames' pixels makes.  dim(), signedness and block are copied; bits_per_val() is kept from the
    /// source and is therefore an upper bound for the selected frames.  An entry that is no frame: std::invalid_argument.
    Terse select(std::span<const std::uint32_t> frames) const {
        Terse t;
        t.d_signed = d_signed; t.d_block = d_block; t.d_size = d_size; t.d_prolix_bits = d_prolix_bits; t.d_dim = d_dim;
        std::size_t bytes = 0;
        for (std::uint32_t f : frames) {
            if (f >= d_frame_sizes.size()) throw std::invalid_argument("select: frame index out of range");
            bytes += d_frame_sizes[f];
        }
        if (frames.empty()) return t;
        detail::require_abi();
        std::vector<std::uint64_t> offs(d_frame_sizes.size() + 1, 0), out_offs(frames.size() + 1, 0);
        for (std::size_t f = 0; f < d_frame_sizes.size(); ++f) offs[f + 1] = offs[f] + d_frame_sizes[f];
        t.d_terse_data.resize(bytes);
        std::size_t total = 0;
        detail::check(trpx_select_frames_host(TRPX_U8 + (d_signed ? 1 : 0), d_terse_data.data(), d_terse_data.size(), offs.data(), d_size,
                                              d_frame_sizes.size(), d_block, frames.data(), frames.size(), t.d_terse_data.data(), bytes,
                                              out_offs.data(), &total, -1), "Terse::select");
        t.d_terse_data.resize(total);
        for (std::size_t i = 0; i < frames.size(); ++i) t.d_frame_sizes.push_back(std::size_t(out_offs[i + 1] - out_offs[i]));
        if (const std::uint64_t* gs = f_states()) {                                // the group states travel with their frames
            const std::size_t groups = d_group_states.size() / d_frame_sizes.size();
            for (std::uint32_t f : frames) t.d_group_states.insert(t.d_group_states.end(), gs + f * groups, gs + (f + 1) * groups);
        }
        return t;
    }

    /// Appends row_offsets.size() - 1 frames given as their events in CSR form -- what prolix_sparse returns -- in one device
    /// call, without building the dense frames (trpx_encode_sparse_host): frame k is size() zeros with px[positions[i]] =
    /// values[i] for row_offsets[k] <= i < row_offsets[k + 1].  Positions ascend strictly inside a frame and stay below the
    /// frame size (std::invalid_argument otherwise).  The first push fixes size() -- `size`, or the product of dim() -- and the
    /// signedness, as push_back does; afterwards the object is what push_back of the dense frames makes of it.
    template <typename T>
    void push_back_sparse(std::vector<std::uint64_t> const& row_offsets, std::vector<std::uint32_t> const& positions,
                          std::vector<T> const& values, std::size_t size = 0) {
        static_assert(std::is_integral_v<T> && sizeof(T) <= 4, "push_back_sparse: an integer type of at most 32 bits");
        if (row_offsets.empty() || positions.size() != values.size())
            throw std::invalid_argument("push_back_sparse: row_offsets [n_frames + 1], positions and values of one length");
        const std::size_t n_frames = row_offsets.size() - 1;
        if (n_frames == 0) return;
        std::size_t n = d_size;
        if (number_of_frames() == 0) {
            n = size;
            if (!n && !d_dim.empty()) { n = 1; for (std::size_t d : d_dim) n *= d; }
            if (!n) throw std::invalid_argument("push_back_sparse: the first push needs the frame size (size, or dim())");
        } else {
            if (size && size != d_size) throw std::invalid_argument("each frame of a multi-Terse object must have the same size");
            if (d_signed != std::is_signed_v<T>) throw std::invalid_argument("signedness differs from the first frame");
        }
        detail::require_abi();
        const std::size_t cap = trpx_encode_sparse_bound_bytes(detail::dtype_of<T>(), n, n_frames, positions.size(), d_block);
        if (!cap) throw std::invalid_argument("push_back_sparse: block 12 and frames of < 2^32 values only");
        const std::size_t prev = d_terse_data.size();
        d_terse_data.resize(prev + cap);
        std::size_t total = 0;
        unsigned pb = 0;
        std::vector<std::uint64_t> offs(n_frames + 1);
        const int rc = trpx_encode_sparse_host(detail::dtype_of<T>(), row_offsets.data(), positions.empty() ? nullptr : positions.data(),
                                               positions.empty() ? nullptr : values.data(), positions.size(), n, n_frames, d_block,
                                               d_terse_data.data() + prev, cap, &total, offs.data(), &pb, -1);
        if (rc != TRPX_OK) d_terse_data.resize(prev);
        detail::check(rc, "Terse::push_back_sparse");
        f_drop_stack();
        d_group_states.clear();
        if (number_of_frames() == 0) {
            d_size = n;
            d_signed = std::is_signed_v<T>;
        }
        d_terse_data.resize(prev + total);
        for (std::size_t f = 0; f < n_frames; ++f) d_frame_sizes.push_back(std::size_t(offs[f + 1] - offs[f]));
        d_prolix_bits = std::max(d_prolix_bits, pb);                              // Terse.hpp:516
    }

    std::size_t size() const { return d_size; }                                   // Terse.hpp:396
    std::size_t number_of_frames() const { return d_frame_sizes.size(); }         // :403
    std::vector<std::size_t> const& dim() const { return d_dim; }                 // :410
    std::vector<std::size_t> const& dim(std::vector<std::size_t> const& dim) {    // :418-421
        if (!d_dim.empty()) throw std::invalid_argument("you cannot overwrite the dimensionality of a frame");
        return d_dim = dim;
    }
    bool is_signed() const { return d_signed; }                                   // :428
    unsigned bits_per_val() const { return d_prolix_bits; }                       // :435
    std::size_t terse_size() const { return d_terse_data.size(); }                // :444
    /// True if the reference's ImageJ plugin accepts a file written from this object (ImageJ/TRPX_Reader.java:94-98:
    /// unsigned data of at most 16 bits per value; the file must fit a Java byte array).
    bool imagej_readable() const { return !d_signed && d_prolix_bits <= 16 && d_terse_data.size() < (std::size_t(1) << 31) - 4096; }
    std::vector<std::size_t> const& frame_sizes() const { return d_frame_sizes; }
    std::vector<std::uint8_t> const& data() const { return d_terse_data; }

    /// True if the object knows the chain state at every 256th block of every frame (read from a file written with
    /// frame_index = true, or computed by that write): its frames are then expanded without any header walk.
    bool has_group_index() const { return f_states() != nullptr; }

    /// XML-ish header + raw stack (Terse.hpp:454-474), byte-identical header text.  frame_index = true adds the
    /// frame_sizes and group_bit_offsets attributes: the reference reader ignores them, this
    /// reader then needs neither a device walk to locate the frames nor one to expand them.
    void write(std::ostream& ostream, bool frame_index = false) const {
        trpx_header h{};
        h.prolix_bits = d_prolix_bits;
        h.is_signed = d_signed;
        h.block = d_block;
        h.memory_size = d_terse_data.size();
        h.number_of_values = d_size;
        h.number_of_frames = d_frame_sizes.size();
        h.n_dims = (unsigned)std::min<std::size_t>(d_dim.size(), 8);
        for (unsigned i = 0; i < h.n_dims; ++i) h.dims[i] = d_dim[i];
        std::vector<std::uint64_t> sizes(d_frame_sizes.begin(), d_frame_sizes.end());
        // 0: block != 12, or values of more than 32 bits (64-bit containers run on the generic kernels, which have no decode
        // index): such files carry frame_sizes only
        const std::size_t groups = frame_index && d_prolix_bits <= 32 ? trpx_group_count(d_size, d_block) : 0;
        if (groups && d_group_states.size() != groups * sizes.size() && !sizes.empty()) {
            std::vector<std::uint64_t> offs(sizes.size() + 1, 0);
            for (std::size_t f = 0; f < sizes.size(); ++f) offs[f + 1] = offs[f] + sizes[f];
            // computed into a local and then moved into the cache (write() is const like the reference's, Terse.hpp:454; the
            // cache makes it -- like prolix(), Terse.hpp:387-388 -- unsafe to call on ONE object from two threads at once)
            std::vector<std::uint64_t> states(groups * sizes.size(), 0);
            const unsigned max_bits = d_prolix_bits <= 8 ? 8 : d_prolix_bits <= 16 ? 16 : 32;
            const int rc = trpx_group_states_host(d_terse_data.data(), d_terse_data.size(), offs.data(), d_size, sizes.size(), d_block,
                                                  max_bits, states.data(), -1);
            if (rc == TRPX_OK) d_group_states = std::move(states);
            else if (rc == TRPX_ERR_UNSUPPORTED) d_group_states.clear();             // no group index for this stack: the file still gets its frame sizes
            else detail::check(rc, "Terse::write (group states)");                   // device fault, no device, corrupt stack: not "no index"
        }
        const bool with_groups = groups && d_group_states.size() == groups * sizes.size();
        std::vector<char> buf(512 + (frame_index ? 21 * d_frame_sizes.size() + (with_groups ? 16 * d_group_states.size() : 0) : 0));
        const std::size_t n = !frame_index ? trpx_header_format(&h, buf.data(), buf.size())
                              : with_groups ? trpx_header_format_grouped(&h, sizes.data(), sizes.size(), d_group_states.data(),
                                                                         d_group_states.size(), buf.data(), buf.size())
                                            : trpx_header_format_indexed(&h, sizes.data(), sizes.size(), buf.data(), buf.size());
        ostream.write(buf.data(), (std::streamsize)n);
        ostream.write(reinterpret_cast<const char*>(d_terse_data.data()), (std::streamsize)d_terse_data.size());
        ostream.flush();
    }

private:
    bool d_signed = false;
    unsigned d_block = 12;
    std::size_t d_size = 0;
    unsigned d_prolix_bits = 0;
    std::vector<std::size_t> d_dim;
    std::vector<std::uint8_t> d_terse_data;
    std::vector<std::size_t> d_frame_sizes;
    mutable trpx_stack* d_stack = nullptr;             // the stack on the device, for prolix(it, frame); dropped when frames are added
    mutable std::vector<std::uint64_t> d_group_states; // chain state at every 256th block of every frame (row f1), or empty (a cache: write() const fills it)

    const std::uint64_t* f_states() const {
        const std::size_t groups = trpx_group_count(d_size, d_block);
        return groups && !d_frame_sizes.empty() && d_group_states.size() == groups * d_frame_sizes.size() ? d_group_states.data() : nullptr;
    }

    void f_drop_stack() {
        if (d_stack) trpx_stack_close(d_stack);
        d_stack = nullptr;
    }

    template <typename Iterator>
    void f_compress(Iterator data, std::size_t n_frames) {                        // Terse.hpp:500-549 -> device
        detail::require_abi();
        using V = typename std::iterator_traits<Iterator>::value_type;
        f_drop_stack();
        d_group_states.clear();
        bool narrowed = false;
        if constexpr (sizeof(V) == 8) {
            // 64-bit integers (what src/terse.cpp:120-123 makes of float / double images): the stream of values that fit
            // 32 bits is the same whatever the container's type, so they are narrowed here and take the tuned kernels;
            // a stack with wider values goes through as 64-bit pixels (generic kernels, fields of up to 64 bits).
            static_assert(std::is_integral_v<V>, "trpx::Terse: pixel type must be integral");
            using N = std::conditional_t<std::is_signed_v<V>, std::int32_t, std::uint32_t>;
            std::vector<N> narrow(d_size * n_frames);
            Iterator it = data;
            bool fits = true;
            for (N& x : narrow) {
                const V v = *it++;
                if (v < (V)std::numeric_limits<N>::min() || v > (V)std::numeric_limits<N>::max()) { fits = false; break; }
                x = (N)v;
            }
            if (fits) {
                f_compress(narrow.data(), n_frames);
                narrowed = true;
            }
        }
        if (!narrowed) {
        std::vector<V> tmp;
        const V* src;
        if constexpr (std::is_pointer_v<Iterator>) src = data;
        else { tmp.assign(data, data + d_size * n_frames); src = tmp.data(); }
        const std::size_t cap = n_frames * trpx_worst_case_bytes(detail::dtype_of<V>(), d_size, d_block);
        const std::size_t prev = d_terse_data.size();
        d_terse_data.resize(prev + cap);
        std::size_t total = 0;
        unsigned pb = 0;
        std::vector<std::uint64_t> offs(n_frames + 1);
        const int rc = trpx_encode_host(detail::dtype_of<V>(), src, d_size, n_frames, d_block, d_terse_data.data() + prev,
                                        cap, &total, offs.data(), &pb, -1);
        if (rc != TRPX_OK) d_terse_data.resize(prev);
        detail::check(rc, "Terse::push_back");
        d_terse_data.resize(prev + total);
        for (std::size_t f = 0; f < n_frames; ++f) d_frame_sizes.push_back(std::size_t(offs[f + 1] - offs[f]));
        d_prolix_bits = std::max(d_prolix_bits, pb);                              // Terse.hpp:516
        }
    }

    void f_read(std::ifstream& istream) {
        const std::streampos pos = istream.tellg();
        std::vector<char> blob;
        std::size_t got = 0, off = 0;
        trpx_header h;
        for (std::size_t want = 4096;; want <<= 4) {                               // an indexed header can be long
            blob.resize(want);
            istream.clear();
            istream.seekg(pos);
            istream.read(blob.data(), (std::streamsize)want);
            got = (std::size_t)istream.gcount();
            istream.clear();
            if (trpx_header_parse(blob.data(), got, &h, &off) == TRPX_OK) break;
            if (got < want || want >= (std::size_t(1) << 28)) throw std::invalid_argument("no valid <Terse .../> header");
        }
        // nothing of the header is believed before it is checked against the file: every frame is at least one byte
        // (Terse.hpp:547), the payload cannot be longer than what follows the header
        istream.seekg(0, std::ios::end);
        const std::streamoff file_end = istream.tellg();
        istream.clear();
        const std::uint64_t avail = file_end >= std::streamoff(pos) + std::streamoff(off) ? std::uint64_t(file_end - std::streamoff(pos) - std::streamoff(off)) : 0;
        if (h.memory_size > avail) throw std::runtime_error("truncated .trpx payload");
        if (h.number_of_frames > h.memory_size || h.number_of_values == 0 || h.block == 0 || h.block > 4096 || h.prolix_bits > 64)
            throw std::invalid_argument("inconsistent <Terse .../> header");
        d_prolix_bits = h.prolix_bits;
        d_signed = h.is_signed;
        d_block = h.block;
        d_size = h.number_of_values;
        for (unsigned i = 0; i < h.n_dims; ++i) d_dim.push_back(h.dims[i]);
        d_terse_data.resize(h.memory_size);
        istream.seekg(pos + std::streamoff(off));
        istream.read(reinterpret_cast<char*>(d_terse_data.data()), (std::streamsize)d_terse_data.size());
        if ((std::size_t)istream.gcount() != d_terse_data.size()) throw std::runtime_error("truncated .trpx payload");
        std::vector<std::uint64_t> sizes(h.number_of_frames ? h.number_of_frames : 1);
        const std::size_t have = trpx_header_frame_sizes(blob.data(), got, sizes.data(), sizes.size());
        std::uint64_t sum = 0;
        bool positive = true;
        for (std::size_t i = 0; i < have && i < sizes.size(); ++i) { sum += sizes[i]; positive = positive && sizes[i] > 0; }
        if (h.number_of_frames == 1) d_frame_sizes = {d_terse_data.size()};
        else if (h.number_of_frames > 1 && have == h.number_of_frames && positive && sum == d_terse_data.size())
            d_frame_sizes.assign(sizes.begin(), sizes.end());                      // row f1: the file carries its frame index
        else if (h.number_of_frames > 1) {
            std::vector<std::uint64_t> offs(h.number_of_frames + 1);
            const unsigned max_bits = h.prolix_bits <= 8 ? 8 : h.prolix_bits <= 16 ? 16 : h.prolix_bits <= 32 ? 32 : 64;
            detail::check(trpx_frame_offsets_host(d_terse_data.data(), d_terse_data.size(), d_size, h.number_of_frames,
                                                  d_block, max_bits, offs.data(), -1), "Terse(std::ifstream&)");
            for (std::size_t f = 0; f < h.number_of_frames; ++f) d_frame_sizes.push_back(std::size_t(offs[f + 1] - offs[f]));
        }
        const std::size_t groups = trpx_group_count(d_size, d_block);               // row f1: group states, if the file has them
        if (groups && groups * d_frame_sizes.size() < (std::size_t(1) << 32)) {
            std::vector<std::uint64_t> st(groups * d_frame_sizes.size());
            if (trpx_header_group_states(blob.data(), off, st.data(), st.size()) == st.size()) d_group_states.swap(st);   // (checked on the device when used)
        }
    }
};

}  // namespace trpx
#endif
