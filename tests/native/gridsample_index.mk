# test-only: gridsample_index -- the GridSample kernel's coordinate function (infera_amd/csrc/host/gridsample.hpp) swept over edge values on the
# CPU, under AddressSanitizer + UndefinedBehaviorSanitizer with float-cast-overflow (a float that reaches int() outside int's range is a report).  A host program with its own main: no library, no GPU, never loaded into Python.
#   make -C tests/native -f gridsample_index.mk && tests/native/gridsample_index
ROOT := ../..
gridsample_index: gridsample_index.cpp $(ROOT)/infera_amd/csrc/host/gridsample.hpp
	g++ -std=c++17 -O1 -g -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all -fno-omit-frame-pointer -o $@ $<
clean:
	rm -f gridsample_index
.PHONY: clean
