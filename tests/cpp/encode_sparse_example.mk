# Builds encode_sparse_example (Terse::push_back_sparse from C++; needs a GPU at run time) and encode_sparse_sanitize (the host-only
# code of trpx_encode_sparse_host under ASan + UBSan; CPU only) beside the examples of ./Makefile:
#     make -C tests/cpp -f encode_sparse_example.mk
CXX ?= g++
ROOT = ../..
all: encode_sparse_example encode_sparse_sanitize
encode_sparse_example: encode_sparse_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
encode_sparse_sanitize: encode_sparse_sanitize.cpp $(ROOT)/trpx_amd/csrc/sparse_events.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f encode_sparse_example encode_sparse_sanitize
.PHONY: all clean
