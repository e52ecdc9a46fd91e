# Builds the HIP library (C-ABI: include/phylomap_hip.h) and the CPU oracle.
# -ffp-contract=off is part of the arithmetic spec (no fused multiply-add on either side unless written as one).
# One object per source so that `make -j` compiles the kernels side by side.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CSRC    := phylomap_amd/csrc
LIB     := phylomap_amd/libphylomap_hip.so
OBJDIR  := build/obj
BLOCKS  := build/tests/libphm_device_blocks.so
SRCS    := $(CSRC)/phm_engine.cpp $(CSRC)/phm_drivers.cpp $(CSRC)/phm_expm_api.cpp $(CSRC)/phm_sched.cpp $(CSRC)/phm_qupdate.cpp $(CSRC)/phm_rtc.cpp $(CSRC)/phm_sim_api.cpp $(CSRC)/phm_sim_models_api.cpp $(CSRC)/phm_expect_api.cpp $(CSRC)/phm_expect_time.cpp $(CSRC)/phm_loglik_host.cpp $(CSRC)/phm_loglik_api.cpp $(CSRC)/phm_scores_api.cpp $(CSRC)/phm_scores_wide_api.cpp $(CSRC)/phm_branch_rows_api.cpp $(CSRC)/phm_time_models_api.cpp $(CSRC)/phm_time_models_wide_api.cpp $(CSRC)/phm_sample_host.cpp $(CSRC)/phm_sample_api.cpp $(CSRC)/phm_sample_wide_api.cpp $(CSRC)/phm_gibbs_api.cpp $(CSRC)/phm_gibbs_wide_api.cpp $(CSRC)/phm_ancestral_api.cpp $(CSRC)/phm_ancestral_wide_host.cpp $(CSRC)/phm_ancestral_wide_api.cpp $(CSRC)/phm_mcmc.hip $(CSRC)/phm_wide.hip $(CSRC)/phm_narrow.hip $(CSRC)/phm_tiles.hip $(CSRC)/phm_wbranch.hip $(CSRC)/phm_wtiles.hip $(CSRC)/phm_exp.hip $(CSRC)/phm_sim.hip $(CSRC)/phm_simm.hip $(CSRC)/phm_expect.hip $(CSRC)/phm_maps.hip $(CSRC)/phm_mcmc_maps.hip $(CSRC)/phm_loglik.hip $(CSRC)/phm_scores.hip $(CSRC)/phm_scores_wide.hip $(CSRC)/phm_branch_rows.hip $(CSRC)/phm_branch_rows_wide.hip $(CSRC)/phm_time_models.hip $(CSRC)/phm_time_models_wide.hip $(CSRC)/phm_sample.hip $(CSRC)/phm_sample_wide.hip $(CSRC)/phm_ancestral.hip $(CSRC)/phm_ancestral_wide.hip
OBJS    := $(patsubst $(CSRC)/%,$(OBJDIR)/%.o,$(SRCS))
HDRS    := $(wildcard $(CSRC)/*.h) include/phylomap_hip.h include/phylomap_hip_ext.h include/phylomap_hip_ext2.h include/phylomap_hip_ext3.h include/phylomap_hip_ext4.h include/phylomap_hip_ext5.h include/phylomap_hip_ext6.h
# EXTRA: experiment switches (e.g. make LIB=scratch/libv1.so OBJDIR=build/v1 EXTRA=-DWT_BRANCH_WAVES=8)
EXTRA   ?=
FLAGS   := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function $(EXTRA)

all:
	$(MAKE) -j8 $(LIB) $(BLOCKS)
	$(MAKE) oracle

$(OBJDIR)/%.o: $(CSRC)/% $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(FLAGS) -x hip -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -lhiprtc

# test-only harness of the device building blocks (tests/test_gpu_device_blocks.py): the shared headers, unchanged, under
# exactly the library's FLAGS; a library of its own, never linked into $(LIB)
$(BLOCKS): tests/native/device_blocks.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(FLAGS) -I$(CSRC) -shared -x hip -o $@ $<

blocks: $(BLOCKS)

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(LIB) build; $(MAKE) -C oracle clean

.PHONY: all blocks oracle clean
