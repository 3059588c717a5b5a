# oracle/ref_run.mk -- run the reference's own program text: its three source files, read where they lie under $(REF) and
# unchanged, compiled over the stand-in headers of cvshim/ (our text, not OpenCV) and the oracle's C primitives, driven by
# tests/cpp/ref_sequence.cpp.  The binary goes to oracle/_ref/ only (git-ignored); what it WRITES is committed as data under
# tests/golden/ref_run/.  Run:  make -f ref_run.mk [golden]
REF ?= /root/reference
OUT := _ref
CXX ?= g++
CC  ?= gcc
FP  := -O1 -ffp-contract=off -fno-fast-math

$(OUT)/ref_run: ../tests/cpp/ref_sequence.cpp cvshim/opencv2/core/core.hpp cvshim/opencv2/imgproc/imgproc.hpp cvsteer_oracle.h \
		oracle_filter.c oracle_taps.c $(REF)/cvsteer/SteerableFilters.cpp $(REF)/cvsteer/SteerableFiltersG2.cpp $(REF)/cvsteer/SteerableFiltersG4.cpp
	mkdir -p $(OUT)/ref_run_obj
	$(CC) -std=c11 $(FP) -c oracle_filter.c -o $(OUT)/ref_run_obj/oracle_filter.o
	$(CC) -std=c11 $(FP) -c oracle_taps.c -o $(OUT)/ref_run_obj/oracle_taps.o
	for s in SteerableFilters SteerableFiltersG2 SteerableFiltersG4; do \
		$(CXX) -std=c++11 $(FP) -w -Icvshim -I. -I$(REF) -c $(REF)/cvsteer/$$s.cpp -o $(OUT)/ref_run_obj/$$s.o || exit 1; done
	$(CXX) -std=c++11 $(FP) -Wall -Wextra -Icvshim -I. -I$(REF) -c ../tests/cpp/ref_sequence.cpp -o $(OUT)/ref_run_obj/ref_sequence.o
	$(CXX) -o $@ $(OUT)/ref_run_obj/ref_sequence.o $(OUT)/ref_run_obj/SteerableFilters.o $(OUT)/ref_run_obj/SteerableFiltersG2.o \
		$(OUT)/ref_run_obj/SteerableFiltersG4.o $(OUT)/ref_run_obj/oracle_filter.o $(OUT)/ref_run_obj/oracle_taps.o -lm -lpthread

# inputs from numpy (fixed seed), outputs from the binary, both packed into tests/golden/ref_run/
golden: $(OUT)/ref_run
	python3 ../tests/golden/make_fixtures.py ref_run $(abspath $(OUT)/ref_run)
