# Builds decode_plan_test: the decode routes of trpx_amd/csrc/decode_plan.hpp under ASan + UBSan (host code only, CPU only):
#     make -C tests/cpp -f decode_plan_test.mk
CXX ?= g++
ROOT = ../..
all: decode_plan_test
decode_plan_test: decode_plan_test.cpp $(ROOT)/trpx_amd/csrc/decode_plan.hpp
	$(CXX) -std=c++20 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -I$(ROOT)/trpx_amd/csrc -o $@ $<
clean:
	rm -f decode_plan_test
.PHONY: all clean
