# CPU-only: the emulator's farm build under the sanitizers (tests/test_emu_kernel.py runs it in a subprocess with the
# sanitizer runtime preloaded).  Kept out of the Makefile: sanitizer builds are for the CPU.  LLVM's clang compiles the
# kernel source as plain host C++ (no offload target); -fno-gpu-sanitize states that no device code is sanitized.
CLANGXX ?= /opt/rocm/llvm/bin/clang++
CSRC := ../../slip_lu_amd/csrc
libslip_emu_san.so: $(CSRC)/slip_hip.hip $(CSRC)/ref_lu_pipe.h $(CSRC)/ref_lu_pipe_cols.h $(CSRC)/ref_lu_pipe_commit.h $(CSRC)/wave_bigint.h $(CSRC)/wave_bigint_reg.h $(CSRC)/wave_shim.h fiber_emu.h hip_rt_emu.h
	$(CLANGXX) -O1 -g -fPIC -shared -shared-libsan -fsanitize=address,undefined -fno-gpu-sanitize -fno-sanitize-recover=undefined -fno-omit-frame-pointer -Wno-unused-command-line-argument -DSLIP_EMULATE -DSLIP_FARM_MIN_COST=0 -DSLIP_FARM_MIN_ITEMS=2 -DSLIP_FARM_NEAR_DIV=0 -DSLIP_FARM_KIND2_COST=0 -I. -I$(CSRC) -x c++ $(CSRC)/slip_hip.hip -o $@
# the sanitizer runtime that libslip_emu_san.so needs (preloaded into the test's subprocess)
print-runtime:
	@$(CLANGXX) -print-file-name=libclang_rt.asan-x86_64.so
.PHONY: print-runtime
