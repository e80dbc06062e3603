# Builds select_example (Terse::select from C++; needs a GPU at run time) and select_sanitize (the output map of
# trpx_select_frames, trpx_amd/csrc/select_map.hpp, under ASan + UBSan; CPU only) beside the examples of ./Makefile:
#     make -C tests/cpp -f select_example.mk
CXX ?= g++
ROOT = ../..
all: select_example select_sanitize
select_example: select_example.cpp $(ROOT)/include/trpx/Terse.hpp $(ROOT)/include/trpx_hip.h $(ROOT)/trpx_amd/libtrpx_hip.so
	$(CXX) -std=c++20 -O2 -Wall -I$(ROOT)/include -o $@ $< -L$(ROOT)/trpx_amd -ltrpx_hip \
	    -Wl,-rpath,'$$ORIGIN/../../trpx_amd' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64
select_sanitize: select_sanitize.cpp $(ROOT)/trpx_amd/csrc/select_map.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f select_example select_sanitize
.PHONY: all clean
