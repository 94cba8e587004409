# The build of one side library, libtomo_$(NAME).so (gfx950 only), from csrc/$(NAME)/tomo_$(NAME).hip: included by csrc/<name>/Makefile,
# which sets NAME and, for a library that uses hipFFT, LIBS = $(HIPFFT).  Same compiler flags as ../Makefile.  Each is a library of its
# own so that the projector's sources (and the kernel-source hash they define) stay as they are.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFFT = -L/opt/rocm/lib -lhipfft -Wl,-rpath,/opt/rocm/lib
CXXFLAGS ?= -O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=$(ARCH) -munsafe-fp-atomics -ffp-contract=fast -fno-slp-vectorize \
            -Wall -Wno-unused-function -DTOMO_$(shell echo $(NAME) | tr a-z A-Z)_BUILD
LDFLAGS ?= $(strip -shared $(LIBS))
SRCS = tomo_$(NAME).hip
HDRS = ../../../include/tomo_$(NAME).h ../tomo_side_host.h ../tomo_side_fft.h ../tomo_side_zgroups.h ../tomo_side_reduce.h ../tomo_side_lines.h ../tomo_side_tets.h
OUT = ../../libtomo_$(NAME).so
all: $(OUT)
$(OUT): $(SRCS) $(HDRS)
	$(HIPCC) $(CXXFLAGS) $(EXTRA) $(SRCS) -o $@ $(LDFLAGS)
# the device assembly and the kernels' register, LDS and scratch use, as `make asm` of ../Makefile
asm: $(SRCS) $(HDRS)
	mkdir -p ../../../build/asm && $(HIPCC) $(CXXFLAGS) $(EXTRA) -S --cuda-device-only -Rpass-analysis=kernel-resource-usage $(SRCS) \
	    -o ../../../build/asm/$(SRCS).s 2> ../../../build/asm/$(SRCS).usage.txt
clean:
	rm -f $(OUT)
.PHONY: all asm clean
