# Builds bins_example (Terse::prolix_bins from C++; needs a GPU at run time) and bins_sanitize (what a lane of trpx_decode_bins
# does with a block, trpx_amd/csrc/bins_merge.hpp, under ASan + UBSan; CPU only) beside the examples of ./Makefile:
#     make -C tests/cpp -f bins_example.mk
CXX ?= g++
ROOT = ../..
all: bins_example bins_sanitize
bins_example: bins_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
bins_sanitize: bins_sanitize.cpp $(ROOT)/trpx_amd/csrc/bins_merge.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f bins_example bins_sanitize
.PHONY: all clean
