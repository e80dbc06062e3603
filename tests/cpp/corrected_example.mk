# Builds corrected_example (Terse::prolix_corrected from C++; needs a GPU at run time) and corrected_sanitize (the pixel rule and the
# store step's index arithmetic of trpx_decode_corrected, trpx_amd/csrc/correct_px.hpp, under ASan + UBSan; CPU only) beside the
# examples of ./Makefile:
#     make -C tests/cpp -f corrected_example.mk
CXX ?= g++
ROOT = ../..
all: corrected_example corrected_sanitize
corrected_example: corrected_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
corrected_sanitize: corrected_sanitize.cpp $(ROOT)/trpx_amd/csrc/correct_px.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f corrected_example corrected_sanitize
.PHONY: all clean
