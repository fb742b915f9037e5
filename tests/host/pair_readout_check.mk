# csrc/pair_readout.h (the bank read-out of the pair carrier objects) on the CPU, stand-alone: plainly and under ASan + UBSan.
#   make -C tests/host -f pair_readout_check.mk        builds both; `run` runs both
# (tests/test_pair_readout_host.py builds the same two programs itself and feeds them its cases)
CXX ?= g++
CSRC = ../../stabilizer-stream_amd/csrc
SAN ?= -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
PAIR_HDRS = $(CSRC)/pair_readout.h $(CSRC)/carrier_readout.h $(CSRC)/cross_readout.h $(CSRC)/bank_readout.h ../../include/psdcascade.h
all: pair_readout_check pair_readout_check_san
pair_readout_check: pair_readout_check.cpp $(PAIR_HDRS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(CSRC) pair_readout_check.cpp -o $@
pair_readout_check_san: pair_readout_check.cpp $(PAIR_HDRS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra $(SAN) -I$(CSRC) pair_readout_check.cpp -o $@
run: all
	./pair_readout_check && ./pair_readout_check_san
clean:
	rm -f pair_readout_check pair_readout_check_san
.PHONY: all run clean
