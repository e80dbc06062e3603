# Builds sum_labelled_example (Terse::prolix_sum_labelled from C++; needs a GPU at run time) and sum_labelled_sanitize (what
# trpx_decode_sum_labelled decides about runs -- direct flushes, slab slots, the merge: trpx_amd/csrc/label_runs.hpp -- under
# ASan + UBSan; CPU only) beside the examples of ./Makefile:
#     make -C tests/cpp -f sum_labelled_example.mk
CXX ?= g++
ROOT = ../..
all: sum_labelled_example sum_labelled_sanitize
sum_labelled_example: sum_labelled_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
sum_labelled_sanitize: sum_labelled_sanitize.cpp $(ROOT)/trpx_amd/csrc/label_runs.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f sum_labelled_example sum_labelled_sanitize
.PHONY: all clean
