# Builds hist_example (Terse::prolix_hist from C++; needs a GPU at run time) and hist_sanitize (the bin rule of trpx_decode_hist,
# trpx_amd/csrc/hist_bin.hpp, under ASan + UBSan; CPU only) beside the examples of ./Makefile:
#     make -C tests/cpp -f hist_example.mk
CXX ?= g++
ROOT = ../..
all: hist_example hist_sanitize
hist_example: hist_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
hist_sanitize: hist_sanitize.cpp $(ROOT)/trpx_amd/csrc/hist_bin.hpp $(ROOT)/trpx_amd/csrc/bins_merge.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f hist_example hist_sanitize
.PHONY: all clean
