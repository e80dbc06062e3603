# Builds dot_example (Terse::prolix_dot from C++; needs a GPU at run time) beside the examples of ./Makefile:
#     make -C tests/cpp -f dot_example.mk
CXX ?= g++
ROOT = ../..
dot_example: dot_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
clean:
	rm -f dot_example
.PHONY: clean
