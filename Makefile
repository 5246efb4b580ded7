# Builds the product's shared libraries in-tree (they travel to the GPU box with the snapshot).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
# -ffp-contract=off: the reference (Rust/LLVM) never fuses a*b+c; parity depends on it.
# (-Wall ... since round 5: the device code is warning-clean under them)
HIPFLAGS ?= --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wuninitialized -Wconditional-uninitialized -Wno-unused-value -Wno-unused-function -Wno-unused-command-line-argument $(EXTRA_HIPFLAGS)
CSRC := portrayer_amd/csrc
HIP_HDRS := $(wildcard $(CSRC)/*.h) include/portrayer_hip.h

CXX ?= g++
CXXFLAGS ?= -O2 -std=c++20 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wextra -Wno-unused-parameter -Wno-missing-field-initializers
HOST := portrayer_amd/host
HOST_SRCS := $(HOST)/portrayer.cpp $(HOST)/jpeg.cpp $(HOST)/capi.cpp $(wildcard examples/*.cpp)
HOST_HDRS := $(wildcard $(HOST)/*.hpp) examples/examples.hpp include/portrayer_host.h include/portrayer_hip.h
EXAMPLES := single-triangle primitives-simple macho-cows entering-the-mirror-dimension big-scene smooth-shading glossy-reflection soft-shadows hier instance antialiasing fish normal-mapping transmission-refraction water-glass \
            simple nonhier nonhier2 four-shapes graphics-poster simple-cows primitives texture-mapping cube-mapping graphics-castle graphics-temple monkeys-making-monkeys robot-alarm-clock

all: portrayer_amd/libportrayer_hip.so portrayer_amd/libportrayer_host.so $(addprefix examples/bin/,$(EXAMPLES))

# C++ host layer (scene API, flatten, k-d build, camera, Image) + the transliterated example scenes
portrayer_amd/libportrayer_host.so: $(HOST_SRCS) $(HOST_HDRS) portrayer_amd/libportrayer_hip.so
	$(CXX) $(CXXFLAGS) -shared $(HOST_SRCS) -o $@ -Lportrayer_amd -lportrayer_hip -lz -Wl,-rpath,'$$ORIGIN'

examples/bin/%: examples/%.cpp portrayer_amd/libportrayer_host.so
	@mkdir -p examples/bin
	$(CXX) $(CXXFLAGS) -fPIE -DPORTRAYER_EXAMPLE_MAIN $< -o $@ -Lportrayer_amd -lportrayer_host -lportrayer_hip -Wl,-rpath,'$$ORIGIN/../../portrayer_amd'

# Device objects: the C ABI + small kernels (pt_api: context, render, passes; pt_scene: upload, update, deform), the device-side tree build, and the render kernel instantiated per
# traversal mode (one source, nine objects) - compiled side by side under make -j.
OBJDIR ?= $(CSRC)
HIPLIB ?= portrayer_amd/libportrayer_hip.so
RENDER_MODES := 1 2 3 4 5 6 7 8 9
HIP_OBJS := $(OBJDIR)/pt_api.o $(OBJDIR)/pt_scene.o $(OBJDIR)/pt_build.o $(OBJDIR)/pt_node.o $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_render_m$(m).o) \
            $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_aov_m$(m).o) \
            $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_guides_m$(m).o) \
            $(OBJDIR)/pt_rays_sort.o $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_rays_m$(m).o) \
            $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_radiance_m$(m).o) \
            $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_segments_m$(m).o) \
            $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_ao_m$(m).o) \
            $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_gather_m$(m).o) \
            $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_direct_m$(m).o) \
            $(OBJDIR)/pt_probe.o $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_probe_m$(m).o) \
            $(OBJDIR)/pt_film.o $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_film_m$(m).o) \
            $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_lens_m$(m).o) \
            $(OBJDIR)/pt_film_map.o $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_film_map_m$(m).o) \
            $(OBJDIR)/pt_denoise.o $(OBJDIR)/pt_denoise_albedo.o $(OBJDIR)/pt_chart.o

# Every HIP translation unit is built in four steps instead of one `hipcc -c`, so that the device code can be CHECKED and REPAIRED between
# the compiler and the assembler (tools/check_exec_prologue.py; profiles/r05/notes.md section 1: the AMDGPU backend of this toolchain can put
# vector spill code in front of the instruction that re-converges a block's lanes - the wrong render of round 4, the hang of round 3):
#   1. device code to assembly            hipcc --offload-device-only -S
#   2. check + repair                     tools/check_exec_prologue.py --fix   (fails the build if a defect it cannot repair is left)
#   3. assemble, link, bundle             clang -x assembler, lld, clang-offload-bundler  - exactly what hipcc itself runs after its code generator
#   4. host code with the bundle embedded hipcc --cuda-host-only -Xclang -fcuda-include-gpubinary
LLVM_BIN ?= /opt/rocm/lib/llvm/bin
PYTHON ?= python3
define hip_four_steps
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(1) --offload-device-only -S $< -o $(basename $@).raw.s
	$(PYTHON) tools/check_exec_prologue.py --fix $(basename $@).raw.s -o $(basename $@).s
	$(LLVM_BIN)/clang -x assembler -target amdgcn-amd-amdhsa -mcpu=$(ARCH) -c $(basename $@).s -o $(basename $@).dev.o
	$(LLVM_BIN)/lld -flavor gnu -m elf64_amdgpu --no-undefined -shared -o $(basename $@).co $(basename $@).dev.o
	$(LLVM_BIN)/clang-offload-bundler -type=o -bundle-align=4096 -targets=host-x86_64-unknown-linux-gnu,hipv4-amdgcn-amd-amdhsa--$(ARCH) -input=/dev/null -input=$(basename $@).co -output=$(basename $@).hipfb
	$(HIPCC) $(HIPFLAGS) $(1) --cuda-host-only -Xclang -fcuda-include-gpubinary -Xclang $(basename $@).hipfb -c $< -o $@
	@if [ -n "$(KEEP_ASM)" ]; then mkdir -p build/asm && cp $(basename $@).s build/asm/$(notdir $(basename $@)).s; fi
	@rm -f $(basename $@).raw.s $(basename $@).s $(basename $@).dev.o $(basename $@).co $(basename $@).hipfb
endef

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HIP_HDRS) tools/check_exec_prologue.py
	$(call hip_four_steps,)

# The kernels instantiated per traversal mode - one source, nine objects per pass: pt_<pass>_m<mode>.o from pt_<pass>_inst.hip with -DPT_INST_MODE=<mode>.
#   render    the render kernel (pt_render_kernel.h)
#   aov       the primary-visibility pass (pt_aov.h)
#   guides    the guides pass (pt_guides.h): the primary-visibility pass with the albedo, <TEX> instantiations per mode
#   rays      the ray-query pass (pt_rays.h); its keying + sort step (pt_rays_sort.hip) is built by the %.o rule
#   segments  the bounded-segment ray queries (pt_segments.h): pt_rays_kernel with a t_max per ray, and the one unit whose walks start at that bound (PT_WALK_ENTRY_T)
#   ao        the ambient-occlusion pass (pt_ao_inst.hip): a point's rays made in registers (pt_ao.h), pt_segments' walks, both work layouts per mode
#   radiance  the radiance pass (pt_radiance.h): the interpreter over the caller's rays, <TEX, PARK> instantiations per mode
#   gather    the gather pass (pt_gather.h): the same interpreter over the ambient-occlusion contract's rays, made in registers (pt_ao.h), summed per point; <TEX, PARK> per mode
#   direct    the direct-light pass (pt_direct_inst.hip): a point's shadow rays at the scene's lights made in registers (pt_direct.h), pt_segments' walks, summed per point
#   probe     the probe pass (pt_probe_inst.hip): the same interpreter over the probe contract's rays, a sphere about a point made in registers (pt_probe.h), weighted with the
#             order-2 spherical-harmonic basis and summed per probe and round of 64; <TEX, PARK> per mode; the fold over a probe's rounds (pt_probe.hip): the %.o rule
#   film      the film's sampling kernel (pt_film.h): the shading passes' frame (pt_shade_frame.h) with the camera as its source; its fold and resolve kernels (pt_film.hip): the %.o rule
#   lens      the film's sampling kernel behind a lens (pt_lens_inst.hip): the film's policy on that frame with the lens contract's primary rays (pt_lens.h); the fold behind it is the film's
#   (chart    the chart pass has no tree walk and no modes: its three kernels and the host replay of its contract, pt_chart.hip, are built by the %.o rule)
#   film_map  the film's per-pixel budget (pt_film_map.h): the same frame over a list of samples, its length read on the device; its plan, fold, error and budget kernels (pt_film_map.hip): the %.o rule
# Static pattern rules, each over its own nine objects: as a plain pattern, pt_film_m%.o would match pt_film_map.o and pt_film_map_m1.o too.
PASSES := render aov guides rays segments ao radiance gather direct probe film film_map lens
define mode_rule
$(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_$(1)_m$(m).o): $(OBJDIR)/pt_$(1)_m%.o: $(CSRC)/pt_$(1)_inst.hip $(HIP_HDRS) tools/check_exec_prologue.py
	$$(call hip_four_steps,-DPT_INST_MODE=$$*)
endef
$(foreach p,$(PASSES),$(eval $(call mode_rule,$(p))))

$(HIPLIB): $(HIP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared $^ -o $@ -ldl

# the device objects alone (`make -B hipobjs` = the forced recompile of __graft_entry__.build())
hipobjs: $(HIP_OBJS)

# A/B builds made HERE (hipcc cross-compiles) and swapped in on the GPU box by profiles/*.sh:
#   make variant NAME=diag EXTRA_HIPFLAGS=-DPT_DIAG  ->  build/variants/diag/libportrayer_hip.so
variant:
	$(MAKE) OBJDIR=build/variants/$(NAME) HIPLIB=build/variants/$(NAME)/libportrayer_hip.so EXTRA_HIPFLAGS="$(EXTRA_HIPFLAGS)" build/variants/$(NAME)/libportrayer_hip.so

oracle:
	$(MAKE) -C oracle

# `make verify`: every HIP object rebuilt with its checked assembly kept (build/asm/*.s) and the checker run over all of it once more;
# `make verify-mi`: the nine render objects compiled under LLVM's machine verifier.
verify:
	$(MAKE) -B hipobjs KEEP_ASM=1
	$(PYTHON) tools/check_exec_prologue.py $(foreach o,$(HIP_OBJS),build/asm/$(notdir $(basename $(o))).s)
verify-mi:
	for m in $(RENDER_MODES); do $(HIPCC) $(HIPFLAGS) --offload-device-only -mllvm -verify-machineinstrs -DPT_INST_MODE=$$m -c $(CSRC)/pt_render_inst.hip -o /dev/null || exit 1; done

# The switches a build may set (EXTRA_HIPFLAGS, `make variant`); this list is the one place that says which exist. Instrumentation that a driver script
# under profiles/ builds - PT_DIAG (diag.sh), PT_CYCLES (cycles.sh), PT_TIMELINE (timeline.sh), PT_OCCLUDER_STATS (occluder_stats.py), PT_PIXEL_LIST_STATS (pixel_list_stats.py), PT_ABLATE
# (light_slope.py) - and the off switches of shipped optimisations whose gain hangs on this toolchain's register allocation and is measured again after a
# ROCm update (DESIGN.md names each as its A/B). PT_MIN_WAVES=<n> (profiles/ab.sh) takes a value of the user's and is not listed.
# PT_PL_DEPTH_FIRST (the list kernel as it was before round 13, for the timing A/B) changes pt_api.hip alone, which `switches` does not compile:
# `make variant NAME=depthfirst EXTRA_HIPFLAGS=-DPT_PL_DEPTH_FIRST` is its check.
# `make -j8 switches` compiles each switch alone, device-only, to /dev/null (the pattern of verify-mi, the same HIPFLAGS) for the render modes whose object
# it changes - MODES_<switch>, all nine where nothing says so: a switch that stops compiling is noticed. Not part of `all`, and no test runs it.
SWITCHES := PT_DIAG PT_CYCLES PT_TIMELINE PT_OCCLUDER_STATS=1 PT_OCCLUDER_STATS=2 PT_ABLATE=1 PT_ABLATE=2 PT_ABLATE=3 PT_ABLATE=5 PT_ABLATE=6 \
            PT_NO_UNIFORM_HIT PT_NO_EYE_TABLE PT_NO_CERTAIN_SHADOW PT_NO_DARK_LIGHTS PT_NO_PIXEL_LISTS PT_NO_BACKGROUND_SKIP PT_PIXEL_LIST_STATS PT_POW_OCML
MODES_PT_OCCLUDER_STATS := 3 6
MODES_PT_NO_PIXEL_LISTS := 3
MODES_PT_NO_BACKGROUND_SKIP := 3
MODES_PT_PIXEL_LIST_STATS := 3
MODES_PT_NO_UNIFORM_HIT := 3
MODES_PT_NO_EYE_TABLE := 3
MODES_PT_NO_CERTAIN_SHADOW := 3
MODES_PT_NO_DARK_LIGHTS := 3
switch_modes = $(or $(MODES_$(firstword $(subst =, ,$(1)))),$(RENDER_MODES))
switch_target = switch-$(subst =,.,$(1))-m$(2)
define switch_rule
$(call switch_target,$(1),$(2)):
	$$(HIPCC) $$(HIPFLAGS) --offload-device-only -D$(1) -DPT_INST_MODE=$(2) -c $$(CSRC)/pt_render_inst.hip -o /dev/null
endef
SWITCH_TARGETS := $(foreach s,$(SWITCHES),$(foreach m,$(call switch_modes,$(s)),$(call switch_target,$(s),$(m))))
$(foreach s,$(SWITCHES),$(foreach m,$(call switch_modes,$(s)),$(eval $(call switch_rule,$(s),$(m)))))
switches: $(SWITCH_TARGETS)

# `make sanitize-raypk`: the host code of pt_api.hip (the slab-test hook pt_test_raypk and everything beside it) under AddressSanitizer + UBSan, driven by
# tools/raypk_sanitize.cpp as a program of its own on the CPU. Only the HOST side is instrumented (-Xarch_host); the object is built through the same four
# steps as every other one, the remaining objects are the library's. The program launches nothing.
comma := ,
SANITIZE := -fsanitize=address$(comma)undefined
build/sanitize/pt_api.o: $(CSRC)/pt_api.hip $(HIP_HDRS) tools/check_exec_prologue.py
	@mkdir -p build/sanitize
	$(call hip_four_steps,-Xarch_host $(SANITIZE) -Xarch_host -fno-omit-frame-pointer)
sanitize-raypk: build/sanitize/pt_api.o $(HIP_OBJS)
	$(LLVM_BIN)/clang++ -O1 -g -std=c++17 $(SANITIZE) -fno-omit-frame-pointer -c tools/raypk_sanitize.cpp -o build/sanitize/raypk_sanitize.o
	$(HIPCC) --offload-arch=$(ARCH) -Xarch_host $(SANITIZE) build/sanitize/raypk_sanitize.o build/sanitize/pt_api.o $(filter-out $(OBJDIR)/pt_api.o,$(HIP_OBJS)) -o build/sanitize/raypk_sanitize -ldl
	build/sanitize/raypk_sanitize

# `make sanitize-chart`: the host code of pt_chart.hip (the contract's host replay pt_test_chart_host) under AddressSanitizer + UBSan, driven by
# tools/chart_sanitize.cpp as a program of its own on the CPU, built like sanitize-raypk. The program launches nothing.
build/sanitize/pt_chart.o: $(CSRC)/pt_chart.hip $(HIP_HDRS) tools/check_exec_prologue.py
	@mkdir -p build/sanitize
	$(call hip_four_steps,-Xarch_host $(SANITIZE) -Xarch_host -fno-omit-frame-pointer)
sanitize-chart: build/sanitize/pt_chart.o $(HIP_OBJS)
	$(LLVM_BIN)/clang++ -O1 -g -std=c++17 $(SANITIZE) -fno-omit-frame-pointer -c tools/chart_sanitize.cpp -o build/sanitize/chart_sanitize.o
	$(HIPCC) --offload-arch=$(ARCH) -Xarch_host $(SANITIZE) build/sanitize/chart_sanitize.o build/sanitize/pt_chart.o $(filter-out $(OBJDIR)/pt_chart.o,$(HIP_OBJS)) -o build/sanitize/chart_sanitize -ldl
	build/sanitize/chart_sanitize

clean:
	rm -f portrayer_amd/*.so $(CSRC)/*.o
	rm -rf build/asm
	rm -rf build/variants
	rm -rf build/sanitize
	rm -rf examples/bin
	$(MAKE) -C oracle clean
.PHONY: all oracle clean hipobjs variant verify verify-mi sanitize-raypk sanitize-chart switches $(SWITCH_TARGETS)
