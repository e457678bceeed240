# Top-level build: the HIP library behind include/aidax.h (gfx950 only), the LV2
# shell, and the CPU oracle (test infrastructure). `python -c "import
# __graft_entry__ as g; g.build()"` runs `make all`.
#
# -ffp-contract=off everywhere in the product: the fp64 biquads and fp32
# smoothers must round step by step like the reference built without FMA
# contraction; the NN kernels ask for FMAs explicitly (__builtin_fmaf).

HIPCC   ?= hipcc
ROCM    ?= /opt/rocm
CXX     := g++
ARCH    ?= gfx950
PKG     := aidadsp-lv2_amd
SRC     := $(PKG)/csrc
LIBDIR  := $(PKG)/lib
OBJDIR  := build/obj
# EXTRA: measurement builds only (scratch/: e.g. EXTRA=-DAIDAX_LP_TRACE into another LIBDIR / OBJDIR)
CXXFLAGS := -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -Wall -Wextra -Iinclude $(EXTRA)
# -fno-slp-vectorize: clang's SLP pass pairs scalar fp32 FMAs/adds into v_pk_fma_f32 / v_pk_add_f32, which
# cost as much as the two scalar instructions on gfx950 plus the moves that build the pairs (measured:
# GRU-24 pipeline 88.5 -> 84.1 us, cfg3 478 -> 464 us, nothing slower by more than noise)
HIPFLAGS := --offload-arch=$(ARCH) $(CXXFLAGS) -fno-slp-vectorize

HOST_SRCS := $(SRC)/aidax_model.cpp $(SRC)/aidax_dsp_host.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_pool.cpp $(SRC)/aidax_pool_stages.cpp $(SRC)/aidax_pool_model.cpp $(SRC)/aidax_pool_io.cpp $(SRC)/aidax_hub.cpp $(SRC)/aidax_ir.cpp $(SRC)/aidax_ir_stage.cpp $(SRC)/aidax_model_bank.cpp $(SRC)/aidax_rate.cpp $(SRC)/aidax_mix_book.cpp
HOST_OBJS := $(patsubst $(SRC)/%.cpp,$(OBJDIR)/%.o,$(HOST_SRCS))
KERN_OBJS := $(OBJDIR)/aidax_kernels.o $(OBJDIR)/aidax_stack.o $(OBJDIR)/aidax_mfma.o $(OBJDIR)/aidax_mfmalp.o $(OBJDIR)/aidax_tick.o $(OBJDIR)/aidax_mfmals.o $(OBJDIR)/aidax_mfmals2.o $(OBJDIR)/aidax_convm.o $(OBJDIR)/aidax_convs.o $(OBJDIR)/aidax_quad.o $(OBJDIR)/aidax_q4.o $(OBJDIR)/aidax_ir_mfma.o $(OBJDIR)/aidax_resample.o $(OBJDIR)/aidax_meter.o $(OBJDIR)/aidax_gate.o $(OBJDIR)/aidax_tune.o $(OBJDIR)/aidax_mix.o $(OBJDIR)/aidax_bus_limit.o $(OBJDIR)/aidax_bus_reverb.o $(OBJDIR)/aidax_delay.o
HDRS      := $(wildcard $(SRC)/*.h) include/aidax.h

LV2SO := $(PKG)/lv2/rt-neural-generic.so
# Two builds of the library from the same sources (aidax_layout.h: AIDAX_TEST_HOOKS):
#   $(PKG)/lib/libaidax_hip.so        the SHIPPED one — bench.py, smoke(), the LV2 shell, the bundle. No test or measurement switch in it.
#   $(PKG)/lib/hooks/libaidax_hip.so  the same with -DAIDAX_TEST_HOOKS: what tests/conftest.py points AIDAX_LIB at (the suite forces
#                                     kernel forms, injects faults, ...) and what scratch/ measures with.
HOOKS_LIBDIR := $(PKG)/lib/hooks
HOOKS_OBJDIR := build/obj_hooks

all: $(LIBDIR)/libaidax_hip.so hooks $(LV2SO) oracle

hooks:
	$(MAKE) OBJDIR=$(HOOKS_OBJDIR) LIBDIR=$(HOOKS_LIBDIR) EXTRA="-DAIDAX_TEST_HOOKS $(EXTRA)" $(HOOKS_LIBDIR)/libaidax_hip.so

$(OBJDIR)/%.o: $(SRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(CXX) $(CXXFLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ -c $< -o $@

# every kernel's register / scratch report is kept next to its object; the library is linked only after
# tools/check_scratch.py has found no kernel with ScratchSize > 0
# (object and report are ONE grouped target: a deleted .remarks file is rebuilt with its object; the compiler's warnings
# are shown on every build — only the per-kernel resource remarks stay in the file)
$(OBJDIR)/%.o $(OBJDIR)/%.remarks &: $(SRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $(OBJDIR)/$*.o 2> $(OBJDIR)/$*.remarks || (cat $(OBJDIR)/$*.remarks; exit 1)
	@grep -A3 -E "warning:" $(OBJDIR)/$*.remarks >&2 || true

$(OBJDIR)/scratch.ok: $(KERN_OBJS) $(KERN_OBJS:.o=.remarks) tools/check_scratch.py
	python3 tools/check_scratch.py $(KERN_OBJS:.o=.remarks)
	@touch $@

$(LIBDIR)/libaidax_hip.so: $(HOST_OBJS) $(KERN_OBJS) $(OBJDIR)/scratch.ok
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -Wl,-soname,libaidax_hip.so -o $@ $(HOST_OBJS) $(KERN_OBJS)

# The LV2 plugin shell (no lib prefix, like the reference's binary: rt-neural-generic/CMakeLists.txt:47)
$(LV2SO): $(PKG)/lv2/rt_neural_generic_lv2.cpp $(PKG)/lv2/lv2_min.h include/aidax.h $(LIBDIR)/libaidax_hip.so
	$(CXX) $(CXXFLAGS) -shared $< -o $@ -L$(LIBDIR) -laidax_hip -Wl,-rpath,'$$ORIGIN/../lib'

# An installable LV2 bundle (build/rt-neural-generic.lv2): generated TTL, the plugin binary linked with
# rpath $$ORIGIN, the HIP library next to it, the bundled models (tools/make_bundle.py does all of it).
bundle: $(LIBDIR)/libaidax_hip.so
	python3 tools/make_bundle.py --out build

# What every sanitizer harness below is compiled with (a stand-alone program each; those that see a HIP header add its include path)
ASAN_FLAGS := -O1 -g -std=c++17 -ffp-contract=off -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra -Iinclude

# The host-only sources (json parser + loader, packers, control-rate DSP) under ASan + UBSan, driven by
# tests/asan_harness.cpp over a corpus of model files (tests/test_asan.py). CPU only: never built or run on the GPU box.
ASAN_SRCS := tests/asan_harness.cpp $(SRC)/aidax_model.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_dsp_host.cpp
build/asan/asan_harness: $(ASAN_SRCS) $(HDRS) $(SRC)/json_min.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) $(ASAN_SRCS) -o $@
asan: build/asan/asan_harness

# ... and the IR stage's host side (aidax_ir_resample, the fragment packer, IrPlan) the same way: tests/asan_ir_harness.cpp, tests/test_asan_ir.py
ASAN_IR_SRCS := tests/asan_ir_harness.cpp $(SRC)/aidax_ir.cpp $(SRC)/aidax_model.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_dsp_host.cpp
build/asan/asan_ir_harness: $(ASAN_IR_SRCS) $(HDRS) $(SRC)/json_min.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ $(ASAN_IR_SRCS) -o $@
asan_ir: build/asan/asan_ir_harness

# ... and the IR blend's rules (IrPlan's second assignment, ramps, blend section and list): tests/asan_ir_blend_harness.cpp, tests/test_asan_ir_blend.py
ASAN_IR_BLEND_SRCS := tests/asan_ir_blend_harness.cpp $(SRC)/aidax_ir.cpp $(SRC)/aidax_model.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_dsp_host.cpp
build/asan/asan_ir_blend_harness: $(ASAN_IR_BLEND_SRCS) $(HDRS) $(SRC)/json_min.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ $(ASAN_IR_BLEND_SRCS) -o $@
asan_ir_blend: build/asan/asan_ir_blend_harness

# ... and the model bank's host half (ModelBank: who plays which slot, the per-stream records, the commit rules): tests/asan_bank_harness.cpp, tests/test_asan_bank.py
ASAN_BANK_SRCS := tests/asan_bank_harness.cpp $(SRC)/aidax_model_bank.cpp $(SRC)/aidax_model.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_dsp_host.cpp
build/asan/asan_bank_harness: $(ASAN_BANK_SRCS) $(HDRS) $(SRC)/json_min.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ $(ASAN_BANK_SRCS) -o $@
asan_bank: build/asan/asan_bank_harness

# the fixed case of the off-to-on rule that the gate, tuner and delay harnesses share: a prerequisite of theirs where it is there (a harness
# source that does not include it builds without it)
ON_RUNS_CASE := $(wildcard tests/asan_on_runs_case.h)

# ... and the noise gate's host half (GateBook, aidax_stream_stages.h: which gates are on, the runs that restart, the dirty range): tests/asan_gate_harness.cpp, tests/test_asan_gate.py
ASAN_GATE_SRCS := tests/asan_gate_harness.cpp $(SRC)/aidax_model.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_dsp_host.cpp
build/asan/asan_gate_harness: $(ASAN_GATE_SRCS) $(ON_RUNS_CASE) $(HDRS) $(SRC)/json_min.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ $(ASAN_GATE_SRCS) -o $@
asan_gate: build/asan/asan_gate_harness

# ... and the mix buses' host half (MixBook, aidax_mix_stage.h: the sends, their ramps, the CSR plan, the advance per pass and per prefix): tests/asan_mix_harness.cpp, tests/test_asan_mix.py
ASAN_MIX_SRCS := tests/asan_mix_harness.cpp $(SRC)/aidax_mix_book.cpp $(SRC)/aidax_model.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_dsp_host.cpp
build/asan/asan_mix_harness: $(ASAN_MIX_SRCS) $(HDRS) $(SRC)/json_min.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ $(ASAN_MIX_SRCS) -o $@
asan_mix: build/asan/asan_mix_harness

# ... and the bus limiters' host half (LimitBook, aidax_limit_stage.h: the records, the capacities, the dirty range, the ring position and row): tests/asan_limit_harness.cpp, tests/test_asan_limit.py
ASAN_LIMIT_SRCS := tests/asan_limit_harness.cpp $(SRC)/aidax_model.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_dsp_host.cpp
build/asan/asan_limit_harness: $(ASAN_LIMIT_SRCS) $(HDRS) $(SRC)/json_min.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ $(ASAN_LIMIT_SRCS) -o $@
asan_limit: build/asan/asan_limit_harness

# ... and the bus reverbs' host half (ReverbBook, aidax_reverb_stage.h: the records, the capacity, the dirty range, the position, the epochs and their refresh): tests/asan_reverb_harness.cpp, tests/test_asan_reverb.py
ASAN_REVERB_SRCS := tests/asan_reverb_harness.cpp $(SRC)/aidax_model.cpp $(SRC)/aidax_pack.cpp $(SRC)/aidax_dsp_host.cpp
build/asan/asan_reverb_harness: $(ASAN_REVERB_SRCS) $(HDRS) $(SRC)/json_min.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ $(ASAN_REVERB_SRCS) -o $@
asan_reverb: build/asan/asan_reverb_harness

# ... and the owning types (aidax_hip_host.h: DevBuf, PinnedBuf, Event, Stream; SnapshotRing and GateStage::enable built from them) over a
# stub runtime that the harness itself defines, so no HIP library is linked: tests/asan_own_harness.cpp, tests/test_asan_own.py
build/asan/asan_own_harness: tests/asan_own_harness.cpp $(HDRS)
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ tests/asan_own_harness.cpp -o $@
asan_own: build/asan/asan_own_harness

# ... and the two form decisions (aidax_load_form.h: load_kind, conv_family / conv_form, mfma_form and the one-layer rule; aidax_pass_form.h:
# resolve_pass — headers without HIP): tests/form_harness.cpp, tests/test_pass_form_host.py
build/asan/form_harness: tests/form_harness.cpp $(SRC)/aidax_load_form.h $(SRC)/aidax_pass_form.h $(SRC)/aidax_layout.h include/aidax.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) -I$(SRC) tests/form_harness.cpp -o $@
asan_form: build/asan/form_harness

# ... and the hub's host half (HubBook, aidax_hub_book.h — a header without HIP: seats, the rotating buffers, early closes, dropped periods, the
# give-up mapping): tests/asan_hub_harness.cpp, tests/test_asan_hub.py
build/asan/asan_hub_harness: tests/asan_hub_harness.cpp $(SRC)/aidax_hub_book.h include/aidax.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) tests/asan_hub_harness.cpp -o $@
asan_hub: build/asan/asan_hub_harness

# ... and the stream tuners' host half (TunerBook, aidax_tuner_book.h — a header without HIP: which tuners are on, the frame counts, the boundary
# rule, the dirty range, the runs that restart): tests/asan_tuner_harness.cpp, tests/test_asan_tuner.py
build/asan/asan_tuner_harness: tests/asan_tuner_harness.cpp $(ON_RUNS_CASE) $(SRC)/aidax_tuner_book.h $(SRC)/aidax_stage_book.h include/aidax.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) tests/asan_tuner_harness.cpp -o $@
asan_tuner: build/asan/asan_tuner_harness

# ... and the stream delays' host half (DelayBook, aidax_delay_book.h — a header without HIP: the capacity and what fits it, the records and
# parameters, which delays are on, the dirty range, the runs that restart): tests/asan_delay_harness.cpp, tests/test_asan_delay.py
build/asan/asan_delay_harness: tests/asan_delay_harness.cpp $(ON_RUNS_CASE) $(SRC)/aidax_delay_book.h $(SRC)/aidax_stage_book.h include/aidax.h
	@mkdir -p build/asan
	$(CXX) $(ASAN_FLAGS) tests/asan_delay_harness.cpp -o $@
asan_delay: build/asan/asan_delay_harness

oracle:
	$(MAKE) -s -C oracle all
	$(MAKE) -s -C oracle _ref

clean:
	rm -rf build $(LIBDIR) $(HOOKS_LIBDIR) $(LV2SO)
	$(MAKE) -s -C oracle clean

.PHONY: all hooks oracle bundle clean asan asan_ir asan_ir_blend asan_bank asan_gate asan_mix asan_limit asan_reverb asan_own asan_form asan_hub asan_tuner asan_delay
