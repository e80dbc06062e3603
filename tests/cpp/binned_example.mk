# Builds binned_example (Terse::prolix_binned from C++; needs a GPU at run time) and binned_sanitize (what a lane of
# trpx_decode_binned does with a block and how a frame is cut into bands, trpx_amd/csrc/binned_map.hpp, under ASan + UBSan; CPU
# only) beside the examples of ./Makefile:
#     make -C tests/cpp -f binned_example.mk
CXX ?= g++
ROOT = ../..
all: binned_example binned_sanitize
binned_example: binned_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
binned_sanitize: binned_sanitize.cpp $(ROOT)/trpx_amd/csrc/binned_map.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f binned_example binned_sanitize
.PHONY: all clean
