# The rules of the stand-alone host emulations (tests/emu_*/Makefile set NAME and HEADERS and include this): one kernel's header
# run as a plain program under AddressSanitizer / UBSan -- test harness only.  OUT: where the program goes.  SAN= OPT=-O2 gives a
# plain build.  CSRC: the directory the headers named in HEADERS are taken from (tests/mutation_audit.py builds changed copies of
# one); what they include comes from there when it is there, else from the library's sources.
CXX ?= g++
OUT ?= $(NAME)
LIB_CSRC = ../../graphtyper_amd/csrc
CSRC ?= $(LIB_CSRC)
SAN ?= address,undefined
OPT ?= -O1 -g
SANFLAGS = $(if $(SAN),-fsanitize=$(SAN) -fno-sanitize-recover=all -fno-omit-frame-pointer,)
all: $(OUT)
$(OUT): $(NAME).cpp ../wave_seq.hpp $(addprefix $(CSRC)/,$(HEADERS)) $(LIB_CSRC)/graph_dev.hpp $(LIB_CSRC)/gtx_flat.hpp ../../include/gtx.h
	$(CXX) -std=c++17 $(OPT) -Wall -Wno-unused-function -Wno-unknown-pragmas $(SANFLAGS) -I$(CSRC) -I$(LIB_CSRC) -o $@ $(NAME).cpp
