# Builds reduce_example (Terse::prolix_reduce from C++; needs a GPU at run time) and reduce_sanitize (what the op of
# trpx_decode_reduce decides -- identity, step, merge, conversion: trpx_amd/csrc/reduce_ops.hpp -- under ASan + UBSan; CPU only)
# beside the examples of ./Makefile:
#     make -C tests/cpp -f reduce_example.mk
CXX ?= g++
ROOT = ../..
all: reduce_example reduce_sanitize
reduce_example: reduce_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
reduce_sanitize: reduce_sanitize.cpp $(ROOT)/trpx_amd/csrc/reduce_ops.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f reduce_example reduce_sanitize
.PHONY: all clean
