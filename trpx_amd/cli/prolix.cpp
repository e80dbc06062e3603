// prolix -- expands .trpx files to greyscale TIFF stacks on the MI355X.
// Command line and behaviour of the reference tool (senikm/trpx src/prolix.cpp:18-128):
//   prolix [-help] [-verbose] [-delete] [-sum N] [-max N] [file ...]
// every argument with a .trpx extension is read (Terse(std::ifstream&)), the pixel type is chosen from bits_per_val() and
// is_signed() (16-bit up to 16 bits, else 32-bit; :69-92), all frames are decoded in one device call into a TIFF stack
// written next to it as <name>.tif.  Differences: 32-bit stacks are decoded into 32-bit images (the reference passes
// image<int16_t> there, defect D5), frames >= 2 of a stack are located correctly (D1/D2), and the input is kept unless
// -delete is given (the reference always deletes it, :111).  -sum N (not in the reference) writes the sums of N consecutive
// frames instead of the frames (Terse::prolix_sum): a 32-bit TIFF stack, int32 for signed data, uint32 otherwise, clamped.
// -max N (not in the reference) writes the per-pixel maximum of N consecutive frames (Terse::prolix_reduce): a TIFF stack of the
// type the frames themselves would have.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "trpx/Grey_tif.hpp"
#include "trpx/Terse.hpp"

namespace fs = std::filesystem;

template <typename T>
static void expand_stack(trpx::Terse& data, std::uint32_t w, std::uint32_t h, trpx::Grey_tif& tif) {
    const std::size_t n = data.size(), frames = data.number_of_frames();
    std::vector<T> stack(n * frames);
    data.prolix_all(stack.data());
    for (std::size_t i = 0; i < frames; ++i) {
        T* dst = tif.push_back<T>(w, h);
        std::memcpy(dst, stack.data() + i * n, n * sizeof(T));
    }
}

template <typename T>
static void sum_stack(trpx::Terse& data, std::size_t group, std::uint32_t w, std::uint32_t h, trpx::Grey_tif& tif) {
    const std::size_t n = data.size(), frames = data.number_of_frames(), n_out = (frames + group - 1) / group;
    std::vector<T> sums(n * n_out);
    data.prolix_sum(sums.data(), group);
    for (std::size_t i = 0; i < n_out; ++i) {
        T* dst = tif.push_back<T>(w, h);
        std::memcpy(dst, sums.data() + i * n, n * sizeof(T));
    }
}

// T: the type the frames would be expanded to; N: the narrowest type that holds the values, which is what prolix_reduce writes
template <typename T, typename N>
static void max_stack(trpx::Terse& data, std::size_t group, std::uint32_t w, std::uint32_t h, trpx::Grey_tif& tif) {
    const std::size_t n = data.size(), frames = data.number_of_frames(), n_out = (frames + group - 1) / group;
    std::vector<N> maxima(n * n_out);
    data.prolix_reduce(maxima.data(), TRPX_REDUCE_MAX, group);
    for (std::size_t i = 0; i < n_out; ++i) {
        T* dst = tif.push_back<T>(w, h);
        for (std::size_t p = 0; p < n; ++p) dst[p] = (T)maxima[i * n + p];
    }
}

// "-sum N" / "-max N": N from 1 to 4294967295, or 0 with a message
static std::size_t frame_count_arg(const char* key, int i, int argc, char const* argv[]) {
    char* end = nullptr;
    const unsigned long long v = i + 1 < argc ? std::strtoull(argv[i + 1], &end, 10) : 0;
    if (i + 1 >= argc || !end || *end || v == 0 || v > 0xFFFFFFFFull) {
        std::cerr << "prolix: " << key << " needs a frame count from 1 to 4294967295" << std::endl;
        return 0;
    }
    return (std::size_t)v;
}

int main(int argc, char const* argv[]) {
    bool help = false, verbose = false, del = false;
    std::size_t sum = 0;                                      // -sum N: frames per summed image (0: expand the frames)
    std::size_t max = 0;                                      // -max N: frames per maximum image
    std::vector<fs::path> params;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-help") help = true;
        else if (a == "-verbose") verbose = true;
        else if (a == "-delete") del = true;
        else if (a == "-sum" || a == "-max") {
            const std::size_t v = frame_count_arg(a.c_str(), i, argc, argv);
            if (!v) return 1;
            (a == "-sum" ? sum : max) = v;
            ++i;
        } else params.emplace_back(a);
    }
    if (sum && max) {
        std::cerr << "prolix: -sum and -max exclude each other" << std::endl;
        return 1;
    }
    if (help) {
        std::cout << "prolix [-help] [-verbose] [-delete] [-sum N] [-max N] [file ...]\n"
                     "  expands trpx files to tiff files (on the GPU).\n"
                     "Examples:\n"
                     "   prolix *              // all TRPX files with .trpx extensions are expanded to tiff files with .tif extensions.\n"
                     "   prolix ~/dir/my_img*  // decompresses all trpx files in the directory ~/dir that start with my_img\n"
                     "\nkeywords:\n"
                     "  -help      print help\n"
                     "  -verbose   print expanded file names and compute times\n"
                     "  -delete    delete each trpx file after it has been expanded (the reference tool always does)\n"
                     "  -sum N     write the sums of N consecutive frames instead of the frames (the last sum may cover fewer):\n"
                     "             a 32-bit tiff stack, int32 for signed data, uint32 otherwise, clamped\n"
                     "  -max N     write the per-pixel maximum of N consecutive frames instead of the frames (the last may cover\n"
                     "             fewer): a tiff stack of the frames' own type.  Not together with -sum\n";
        return 0;
    }
    std::chrono::duration<double> user_time(0), io_time(0);
    std::size_t expanded_files = 0;
    int rc = 0;
    for (fs::path const& name : params) {
        if (!fs::is_regular_file(name) || name.extension() != ".trpx") continue;
        try {
            auto t0 = std::chrono::high_resolution_clock::now();
            std::ifstream in(name, std::ios::binary);
            if (!in.is_open()) {
                std::cerr << "Failed to open input file " << name << std::endl;
                rc = 1;
                continue;
            }
            trpx::Terse data(in);
            in.close();
            io_time += std::chrono::high_resolution_clock::now() - t0;
            const auto t1 = std::chrono::high_resolution_clock::now();
            std::uint32_t w, h;
            if (data.dim().empty()) w = h = (std::uint32_t)std::sqrt((double)data.size());   // no dimensions: assume a square image (:64-65)
            else if (data.dim().size() >= 2) { w = (std::uint32_t)data.dim()[0]; h = (std::uint32_t)data.dim()[1]; }
            else { w = (std::uint32_t)data.dim()[0]; h = 1; }
            if ((std::size_t)w * h != data.size()) throw std::runtime_error("frame dimensions do not match the number of values.");
            trpx::Grey_tif tif;
            if (sum && data.bits_per_val() <= 32) {
                if (data.is_signed()) sum_stack<std::int32_t>(data, sum, w, h, tif);
                else sum_stack<std::uint32_t>(data, sum, w, h, tif);
            } else if (max && data.bits_per_val() <= 8) {
                if (data.is_signed()) max_stack<std::int16_t, std::int8_t>(data, max, w, h, tif);
                else max_stack<std::uint16_t, std::uint8_t>(data, max, w, h, tif);
            } else if (max && data.bits_per_val() <= 16) {
                if (data.is_signed()) max_stack<std::int16_t, std::int16_t>(data, max, w, h, tif);
                else max_stack<std::uint16_t, std::uint16_t>(data, max, w, h, tif);
            } else if (max && data.bits_per_val() <= 32) {
                if (data.is_signed()) max_stack<std::int32_t, std::int32_t>(data, max, w, h, tif);
                else max_stack<std::uint32_t, std::uint32_t>(data, max, w, h, tif);
            } else if (data.bits_per_val() <= 16) {
                if (data.is_signed()) expand_stack<std::int16_t>(data, w, h, tif);
                else expand_stack<std::uint16_t>(data, w, h, tif);
            } else if (data.bits_per_val() <= 32) {
                if (data.is_signed()) expand_stack<std::int32_t>(data, w, h, tif);
                else expand_stack<std::uint32_t>(data, w, h, tif);
            } else {
                std::cerr << "Terse file " << name << " encodes data that requires 64 bits per pixel." << std::endl;
                std::cerr << "Prolix cannot process such trpx-stacks." << std::endl;
                rc = 1;
                continue;
            }
            user_time += std::chrono::high_resolution_clock::now() - t1;
            t0 = std::chrono::high_resolution_clock::now();
            fs::path tif_name = name;
            tif_name.replace_extension(".tif");
            std::ofstream out(tif_name, std::ios::binary);
            if (!out.is_open()) throw std::runtime_error("Failed to open tiff file for output.");
            tif.write(out);
            out.close();
            if (del) fs::remove(name);
            ++expanded_files;
            io_time += std::chrono::high_resolution_clock::now() - t0;
        } catch (std::exception const& e) {
            std::cerr << "Error processing " << name << ": " << e.what() << std::endl;
            rc = 1;
        }
    }
    if (verbose) {
        for (fs::path const& p : params) std::cout << "Expanded: " << p << std::endl;
        std::cout << "Prolix expanded : " << expanded_files << " files\n";
        std::cout << "User time       : " << user_time.count() << " seconds\n";
        std::cout << "IO time         : " << io_time.count() << " seconds\n";
    }
    return rc;
}
