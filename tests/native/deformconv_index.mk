# test-only: deformconv_index -- the DeformConv kernels' coordinate function (infera_amd/csrc/host/deformconv.hpp) swept over edge values and bit
# patterns on the CPU, under AddressSanitizer + UndefinedBehaviorSanitizer with float-cast-overflow (a float that reaches int() outside int's range is a report).  A host program with its own main: no library, no GPU, never loaded into Python.
#   make -C tests/native -f deformconv_index.mk && tests/native/deformconv_index
ROOT := ../..
deformconv_index: deformconv_index.cpp $(ROOT)/infera_amd/csrc/host/deformconv.hpp
	g++ -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -fno-omit-frame-pointer -o $@ $<
clean:
	rm -f deformconv_index
.PHONY: clean
