# Build of the MI355X-native megapath framework.
#   make host    -> luisarender_amd/lib/liblrhost.so   (scene description, flattening, BVH, image IO)
#   make hip     -> luisarender_amd/lib/liblrhip.so    (HIP megakernel path tracer, C ABI include/lrhip.h)
#   make oracle  -> oracle/liboracle.so                (CPU checker; tests/bench only)
#   make cli     -> luisarender_amd/bin/luisa-render-cli + plugin libluisa-render-integrator-megapath.so
CXX      ?= g++
HIPCC    ?= /opt/rocm/bin/hipcc
CXXFLAGS ?= -std=c++17 -O2 -fPIC -Wall -Wextra
ORACLE_FLAGS ?= -std=c++17 -O3 -march=x86-64-v3 -ffp-contract=off -fPIC -Wall -Wextra -pthread
# fp32 division/sqrt use the hardware approximations (+6 %): the estimator is a Monte-Carlo sum compared with the
# oracle under a stated tolerance, not a bit-exact integer pipeline.  -fapprox-func drops the denormal-range rescaling
# around every v_rcp / v_sqrt / v_rsq (-18 % VALU instructions in the kernel, +5 % throughput) without touching
# the denormal mode.  Denormal flushing itself was measured and REJECTED: it moved the C2 image mean by 0.8 %
# against the oracle (tools/dbg_c2.py); these flags do not (tests/test_gpu_parity.py bias checks).
# -fno-slp-vectorize (round 2): the SLP vectorizer pairs scalar fp32 operations into v_pk_* instructions.  On gfx950 a wave64
# v_pk_fma_f32 issues in ~4.2 cycles against ~2.4 for a v_fma_f32 (tools/valu_peak.hip), so a pair gains little, and the packing
# costs v_mov shuffles into consecutive registers plus register pressure.  Off: C2 689 -> 774 Msamples/s (+12 %), C3 651 -> 758,
# C4 683 -> 747, C5 255 -> 276 at the A/B sizes (profiles/archive/r02f_ab_compiler_flags.txt).  The slab test's hand-written v2f FMAs stay.
# Same arithmetic per lane.  -fno-vectorize (loop vectorizer), -O2, -fno-unroll-loops, relaxed-occupancy scheduling: no change.
HIPFLAGS ?= --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -fno-hip-fp32-correctly-rounded-divide-sqrt -fapprox-func -fno-slp-vectorize

LIBDIR := luisarender_amd/lib
BINDIR := luisarender_amd/bin
HOSTDIR := luisarender_amd/csrc/host
HIPDIR := luisarender_amd/csrc/hip

HOST_SRC := $(HOSTDIR)/sdl.cpp $(HOSTDIR)/scene.cpp $(HOSTDIR)/mesh_io.cpp $(HOSTDIR)/subdiv.cpp $(HOSTDIR)/catmull_clark.cpp $(HOSTDIR)/image_io.cpp $(HOSTDIR)/image_codecs.cpp $(HOSTDIR)/environment.cpp \
            $(HOSTDIR)/accel.cpp $(HOSTDIR)/host_api.cpp $(HOSTDIR)/luisa_render_shim.cpp
HOST_HDR := $(wildcard $(HOSTDIR)/*.h) $(wildcard include/*.h)
# the host sources of liblrhip.so, one object each (lrhip_internal.h: which holds what); the kernels: megapath_variant.hip, heavy_variant.hip
HIP_SRC := $(wildcard $(HIPDIR)/lrhip_*.hip)
HIP_HDR := $(wildcard $(HIPDIR)/*.h) $(wildcard include/*.h)

.PHONY: all host hip oracle oracle-ulp cli clean hip-variant variant-lib ref ieee shallow noearly nopair noride nostash nostraight nolightrec
all: host oracle hip cli ieee shallow noearly nopair noride nostash nostraight nolightrec

# oracle/_ref: the reference's OWN sources compiled in place against the scalar LuisaCompute stand-in of oracle/ref_shim
# (test infrastructure: pins oracle/ to the reference; needs /root/reference, so only where the reference tree exists)
ref:
	$(MAKE) -f oracle/Makefile.ref ref

host: $(LIBDIR)/liblrhost.so
$(LIBDIR)/liblrhost.so: $(HOST_SRC) $(HOST_HDR) Makefile
	@mkdir -p $(LIBDIR)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRC) -ldl -pthread -lz

oracle: oracle/liboracle.so oracle/liboracle_fma.so
oracle/liboracle.so: oracle/oracle.cpp $(wildcard oracle/*.h) include/lr_scene.h Makefile
	$(CXX) $(ORACLE_FLAGS) -shared -o $@ oracle/oracle.cpp
# the same oracle with fused multiply-adds allowed: TEST INFRASTRUCTURE for the one test that measures how far contraction alone moves
# the oracle's own frames (the lamp-lit fog case of the volumetric integrator, tests/test_gpu_parity.py); never a reference for anything else
oracle/liboracle_fma.so: oracle/oracle.cpp $(wildcard oracle/*.h) include/lr_scene.h Makefile
	$(CXX) $(ORACLE_FLAGS) -ffp-contract=fast -shared -o $@ oracle/oracle.cpp
# the same oracle with every cosine and sine one ulp up (oracle_math.h: ORACLE_NUDGE_TRIG): TEST INFRASTRUCTURE for tests/vpt_paths.py, which
# takes the paths that this moves out of its judgement of the `layered` case; never a reference for anything else
oracle-ulp: oracle/liboracle_ulp.so
oracle/liboracle_ulp.so: oracle/oracle.cpp $(wildcard oracle/*.h) include/lr_scene.h Makefile
	$(CXX) $(ORACLE_FLAGS) -DORACLE_NUDGE_TRIG=1 -shared -o $@ oracle/oracle.cpp

# The megakernel is precompiled for a curated set of feature masks, one object per mask so that they build in parallel (make -j).
# csrc/hip/variants.h is the only place where the masks are written: the lists are read off its X-macros with the host preprocessor.
# VARIANT_MASKS may be narrowed for experiments (a missing variant is a run-time error of lrhip_render, never a fallback).
variants_h_list = $(shell echo '$(1)(X)' | $(CXX) -E -P -x c++ -include $(HIPDIR)/variants.h '-DX(mask)=mask' -)
ifeq ($(origin VARIANT_MASKS),undefined)
VARIANT_MASKS := $(call variants_h_list,LR_MEGAKERNEL_LIST)
endif
# the heavy-closure kernels of wavefront mode (csrc/hip/heavy_kernel.h; mask: 1 counters, 2 generic sampler, 4 Mix / 8 Layered instead of
# Disney, 512 nested Mix / Layered)
ifeq ($(origin HEAVY_MASKS),undefined)
HEAVY_MASKS := $(call variants_h_list,LR_HEAVY_LIST)
endif
OBJDIR := $(LIBDIR)/obj
VARIANT_OBJ := $(foreach m,$(VARIANT_MASKS),$(OBJDIR)/variant_$(m).o) $(foreach m,$(HEAVY_MASKS),$(OBJDIR)/heavy_$(m).o)

hip: $(LIBDIR)/liblrhip.so
# The volumetric megakernel (variants 256+) is built with IEEE arithmetic: no fp contraction, correctly rounded division / sqrt, no
# approximate functions.  MegaVPTNaive is chaotic where the reference's algorithm puts a ray origin ON a surface (after a medium
# "hit surface" event, src/media/homogeneous.cpp:64, the next shadow segment starts in the surface it just reached): whether that
# segment re-hits the surface is decided by the last bit, and one flipped decision desynchronises the path's PCG32 stream for
# good.  With the arithmetic of the reference-pinned oracle the device takes the same decisions (tests/test_ref_golden.py,
# test_gpu_parity.py::test_volumetric_megakernel); with contraction it renders the lamp-lit fog scenes 30 % darker than the
# reference's own code does (measured, round 2).  It is a feature row, not the benchmarked path.
VPT_HIPFLAGS ?= --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize -DLR_EXACT_LEAF=1
# EVERY variant is built with -mllvm -amdgpu-spill-sgpr-to-vgpr=0.  With the default (SGPRs spilled into lanes of a VGPR) the kernels that
# make REAL CALLS (out-of-line closures: every mask with Mix, Layered or the volumetric kernel) come out miscompiled or not depending on
# unrelated code, flags and the register budget: NaN / lost samples in <124> at 3 waves per SIMD in round 1, fine after round 2's changes,
# broken again without the SLP vectorizer, <124> (not <125>) non-deterministic at 4 waves after one more change -- each time
# bit-identical to the good builds with this flag.  Some scenes pass on a broken binary (the kitchen parity test did), so tests cannot
# establish that a fast build is sound; the flag removes the mechanism.  Cost: kitchen stand-in 275 -> 256 Msamples/s, <60> 350 -> 298
# (profiles/archive/r02f_ab_compiler_flags.txt).  Round 4: the LEAN variants too -- since round 3 they make a real call of their own
# (the texture callback of load_lobe, dev_math.h: LR_TEX_LAMBDA, is out of line) and spill SGPRs, i.e. they hold exactly the
# ingredients; no binary of theirs was ever caught wrong (profiles/archive/r03s_sgpr_spill_repro.txt: bit-identical with and without the
# flag), but the same was true of <124> for two rounds.  Cost, same box: C2 782.3 -> 777.0, C3 809.6 -> 803.4, C4 875.6 -> 876.2
# Msamples/s at 64 spp, films bit-identical (profiles/r04_ab_call_safe_lean.txt).
CALL_SAFE_FLAGS ?= -mllvm -amdgpu-spill-sgpr-to-vgpr=0
# (the choice follows the kFeatVpt bit, 256, by design: whatever mask instantiates the volumetric kernel -- megapath_variant.hip tests the
# same bit -- takes its arithmetic; today these are 256-259)
# The gather kernels (kFeatGather, 131072: lrhip_gather_irradiance) take that arithmetic too: one of their samples is held to the plan query's
# answer continued by the caller (tests/test_gpu_gather.py), and lrhip_gather.o, which holds the plan kernel, is built with it
variant_flags = $(if $(filter-out 0,$(shell echo $$(( $(1) & (256 | 131072) )))),$(VPT_HIPFLAGS),$(HIPFLAGS)) $(CALL_SAFE_FLAGS)
$(OBJDIR)/variant_%.o: $(HIPDIR)/megapath_variant.hip $(HIP_HDR) Makefile
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(call variant_flags,$*) -DLR_VARIANT=$* -c -o $@ $(HIPDIR)/megapath_variant.hip
# (they make real calls -- the closure interpreters stay out of line -- so they take the same safe flag)
HEAVY_DEFS ?=
$(OBJDIR)/heavy_%.o: $(HIPDIR)/heavy_variant.hip $(HIP_HDR) Makefile
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(CALL_SAFE_FLAGS) $(HEAVY_DEFS) -DLR_HVARIANT=$* -c -o $@ $(HIPDIR)/heavy_variant.hip
HIP_OBJ := $(patsubst $(HIPDIR)/%.hip,$(OBJDIR)/%.o,$(HIP_SRC))
# lrhip_raycast.o holds kernels of its own (csrc/hip/raycast_kernel.h: ray queries); the one with the alpha test calls the texture code, so it takes
# the variants' safe flag.  RAYCAST_DEFS: its A/B builds (make hip-variant NAME=r64 RAYCAST_DEFS=-DLR_RAYCAST_REFILL=64 VARIANT_MASKS=0 HEAVY_MASKS=)
RAYCAST_DEFS ?=
lrhip_raycast_FLAGS = $(CALL_SAFE_FLAGS) $(RAYCAST_DEFS)
# lrhip_instance_update.o holds the kernels that move instances on the device (csrc/hip/instance_update_kernels.h).  Their tables are held to the
# host's unfused fp32 code bit for bit (tests/test_gpu_instance_transforms.py), and HIPFLAGS gives none of what that takes: no fp contraction,
# correctly rounded fp32 division (normal_matrix's 1 / det, quantise_node's scale), no approximate functions (-fapprox-func also marks divisions)
lrhip_instance_update_FLAGS = -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-approx-func
# lrhip_mesh_update.o holds the kernels that deform a mesh in front of those (csrc/hip/mesh_update_kernels.h); its normal recompute -- sums of cross
# products, one square root, three divisions -- is held to the host's bits in the same way (tests/test_gpu_mesh_vertices.py)
lrhip_mesh_update_FLAGS = $(lrhip_instance_update_FLAGS)
# lrhip_surface.o holds the kernels of the surface queries (csrc/hip/surface_kernel.h); the full one makes real calls -- the texture lookup, the
# out-of-line albedo / roughness of Disney, Mix and Layered surfaces -- so it takes the variants' safe flag
lrhip_surface_FLAGS = $(CALL_SAFE_FLAGS)
# lrhip_bsdf.o holds the kernels of the BSDF queries (csrc/hip/bsdf_kernel.h): the texture lookup and the out-of-line evaluate / sample of Disney,
# Mix and Layered surfaces are real calls, so it takes the variants' safe flag.  It is also built with the arithmetic of the reference-pinned
# oracle, like the volumetric kernel: a query hands ONE closure answer to the caller, where a render sums millions, and HIPFLAGS' arithmetic
# shows in single answers -- r / r of Glass' reflection probability under total internal reflection comes out of the approximate division as
# 1 - 2^-24, which leaves a pdf of 1e-8 where the reference has 0, and the cancellations of the visible-normal slope sampling (ggx_sample11)
# turn last-bit differences of v_rcp / v_sqrt and of contraction into sampled directions 2e-3 away from the oracle's (measured)
lrhip_bsdf_FLAGS = $(CALL_SAFE_FLAGS) -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-approx-func
# lrhip_light.o holds the kernels of the light queries (csrc/hip/light_kernel.h): the texture lookup and the environment's evaluate / sample are
# real calls, and a query hands ONE light sample to its caller, so it is built as lrhip_bsdf.o is, for the reason given there
lrhip_light_FLAGS = $(lrhip_bsdf_FLAGS)
# lrhip_camera.o holds the kernels of the camera, sampler and film queries (csrc/hip/camera_kernel.h).  They make no real call, so they need no safe
# flag; they are built with the oracle's arithmetic because a query hands ONE number, ray or weight to its caller: the Sobol sampler's pixel draw has
# a multiply-subtract that contraction would fuse, the camera's normalize a division and the filter's weight another
lrhip_camera_FLAGS = -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-approx-func
# lrhip_lightmap.o holds the kernels of the UV rasteriser (csrc/hip/lightmap_kernels.h).  They decide coverage in float64 and are held, texel by texel,
# to a float64 numpy rasteriser (tests/gather_reference.py): no fp contraction, and none of -fapprox-func's marks on the divisions
lrhip_lightmap_FLAGS = $(lrhip_camera_FLAGS)
# lrhip_gather.o holds the kernels of the gather vertex query (csrc/hip/gather_kernel.h): the light sample and the white Lambert closure of a path that
# starts at a surface point.  It makes lrhip_light.o's real calls and its answers are held to the light and BSDF queries' bits, so it is built as they are
lrhip_gather_FLAGS = $(lrhip_bsdf_FLAGS)
$(HIP_OBJ): $(OBJDIR)/%.o: $(HIPDIR)/%.hip $(HIP_HDR) Makefile
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $($*_FLAGS) -c -o $@ $<
$(LIBDIR)/liblrhip.so: $(HIP_OBJ) $(VARIANT_OBJ)
	$(HIPCC) --offload-arch=gfx950 -shared -o $@ $^

# experimental kernel builds for A/B runs on the GPU box:
#   make hip-variant NAME=w3 DEFS="-DLR_WAVES_LAYERED=3" [VARIANT_MASKS="0 1"]
VOBJDIR := $(LIBDIR)/variants/obj_$(NAME)
hip-variant:
	@mkdir -p $(VOBJDIR)
	$(MAKE) --no-print-directory OBJDIR=$(VOBJDIR) HIPFLAGS='$(HIPFLAGS) $(DEFS)' VARIANT_MASKS='$(VARIANT_MASKS)' HEAVY_MASKS='$(HEAVY_MASKS)' RAYCAST_DEFS='$(RAYCAST_DEFS)' \
	    LIBDIR_OUT=$(LIBDIR)/variants/liblrhip_$(NAME).so variant-lib
variant-lib: $(HIP_OBJ) $(VARIANT_OBJ)
	$(HIPCC) --offload-arch=gfx950 -shared -o $(LIBDIR_OUT) $^

# The lean kernel <0> / <1> once more with the oracle's arithmetic (no fp contraction, correctly rounded division / sqrt, exact
# functions, 1 / det in the triangle test): TEST INFRASTRUCTURE (MegaPathRenderer(lib_path=...)).  Round 3 used it to test the claim
# that fast math is what separates the device from the oracle on the C2 stand-in: only where both sides intersect identical vertices
# (tests/test_gpu_parity.py::test_what_separates_c2_from_the_oracle).
ieee: $(LIBDIR)/variants/liblrhip_ieee.so
$(LIBDIR)/variants/liblrhip_ieee.so: $(HIP_SRC) $(HIPDIR)/megapath_variant.hip $(HIP_HDR) Makefile
	$(MAKE) --no-print-directory hip-variant NAME=ieee HIPFLAGS='$(VPT_HIPFLAGS) -DLR_EXACT_LEAF=1' DEFS= VARIANT_MASKS='0 1' HEAVY_MASKS=

# The lean kernels of both schedulers once more with a FOUR-entry LDS traversal stack: every ray of every scene goes through the HBM
# overflow area of the stack (dev_trace.h: TraversalStack::push / pop beyond kStackLds, the wave-level `deep` paths of the node step,
# and the words a pool kernel parks on top of a lane's stack across the shading block).  TEST INFRASTRUCTURE: its frames must equal the
# shipped library's bit for bit (tests/test_gpu_pool.py::test_the_overflow_area_of_the_traversal_stack).
shallow: $(LIBDIR)/variants/liblrhip_shallow.so
$(LIBDIR)/variants/liblrhip_shallow.so: $(HIP_SRC) $(HIPDIR)/megapath_variant.hip $(HIP_HDR) Makefile
	$(MAKE) --no-print-directory hip-variant NAME=shallow DEFS='-DLR_STACK_LDS=4' VARIANT_MASKS='0 1 4096 4097' HEAVY_MASKS=

# The lean pool kernels once more with the round 5-6 order of an iteration: its fetch requests BEHIND the tail of the iteration before
# (megapool_kernel.h: LR_POOL_EARLY_FETCH).  TEST INFRASTRUCTURE: the shipped order moves memory requests and nothing else, so its frames
# and its ray / node / triangle counters must equal this library's (tests/test_gpu_early_fetch.py).
noearly: $(LIBDIR)/variants/liblrhip_noearly.so
$(LIBDIR)/variants/liblrhip_noearly.so: $(HIP_SRC) $(HIPDIR)/megapath_variant.hip $(HIP_HDR) Makefile
	$(MAKE) --no-print-directory hip-variant NAME=noearly DEFS='-DLR_POOL_EARLY_FETCH=0' VARIANT_MASKS='4096 4097 4100 4101' HEAVY_MASKS=

# The lean pool kernels once more WITHOUT the leaf / node pairing of the traversal loop (megapool_kernel.h: LR_POOL_LEAF_NODE_PAIR): a lane at a
# leaf spends the iteration on its triangle alone.  TEST INFRASTRUCTURE: the pairing regroups a lane's steps into wave iterations and nothing
# else, so the shipped library's frames and its ray / node / triangle counters must equal this library's (tests/test_gpu_leaf_pair.py).
nopair: $(LIBDIR)/variants/liblrhip_nopair.so
$(LIBDIR)/variants/liblrhip_nopair.so: $(HIP_SRC) $(HIPDIR)/megapath_variant.hip $(HIP_HDR) Makefile
	$(MAKE) --no-print-directory hip-variant NAME=nopair DEFS='-DLR_POOL_LEAF_NODE_PAIR=0' VARIANT_MASKS='4096 4097 4100 4101' HEAVY_MASKS=

# Pool kernels once more WITHOUT the shadow ride (megapool_kernel.h: LR_POOL_SHADOW_RIDE): a path whose last vertex has a light sample stays open for
# a job that holds that shadow ray alone.  The lean kernels, the environment set, Disney with an environment, the run-time generic sampler, PaddedSobol
# and the 8-bit-texel Disney set, each with its counting twin.  TEST INFRASTRUCTURE: the ride changes which batch starts which sample and when a
# finished sample joins the film, nothing else, so the shipped library's frames and its path / ray / node / triangle / shaded-vertex counters must equal
# this library's (tests/test_gpu_shadow_ride.py).
noride: $(LIBDIR)/variants/liblrhip_noride.so
$(LIBDIR)/variants/liblrhip_noride.so: $(HIP_SRC) $(HIPDIR)/megapath_variant.hip $(HIP_HDR) Makefile
	$(MAKE) --no-print-directory hip-variant NAME=noride DEFS='-DLR_POOL_SHADOW_RIDE=0' VARIANT_MASKS='4096 4097 4098 4099 4100 4101 4102 4103 4116 4117 20482 20483 12308 12309' HEAVY_MASKS=

# Pool kernels once more WITHOUT the path stash (megapool_kernel.h: LR_POOL_PATH_STASH): a context without a path starts one inside the shading block,
# the hand-out loop and the camera code in nearly every batch for a quarter of its lanes.  The masks of `noride`.  TEST INFRASTRUCTURE: the stash changes
# which lane and which batch start which sample number and nothing else, so the shipped library's frames and its path / ray / node / triangle /
# shaded-vertex counters must equal this library's (tests/test_gpu_path_stash.py).
nostash: $(LIBDIR)/variants/liblrhip_nostash.so
$(LIBDIR)/variants/liblrhip_nostash.so: $(HIP_SRC) $(HIPDIR)/megapath_variant.hip $(HIP_HDR) Makefile
	$(MAKE) --no-print-directory hip-variant NAME=nostash DEFS='-DLR_POOL_PATH_STASH=0' VARIANT_MASKS='4096 4097 4098 4099 4100 4101 4102 4103 4116 4117 20482 20483 12308 12309' HEAVY_MASKS=

# Kernels once more WITHOUT the straight-line control flow of the traversal loop (dev_trace.h: LR_STRAIGHT_TAIL): the three pushes of a node step are
# EXEC regions again and a closest hit is committed by selects on VCC.  The lean one-path kernels and every pool kernel but the continuation passes
# take the shipped form; this library holds the kernels <0> / <1> and the pool kernels that the suite's scenes and the benchmark's configurations
# select (the masks of `noride`).  TEST INFRASTRUCTURE: the shipped form lays an iteration's instructions
# out differently and nothing else, so the shipped library's frames and its path / ray / node / triangle counters must equal this
# library's (tests/test_gpu_straight_tail.py).  `make shallow` is built WITH the shipped form: the same test holds its pool kernel, whose node steps
# stand at the boundary to the overflow area, to the shipped film.
nostraight: $(LIBDIR)/variants/liblrhip_nostraight.so
$(LIBDIR)/variants/liblrhip_nostraight.so: $(HIP_SRC) $(HIPDIR)/megapath_variant.hip $(HIP_HDR) Makefile
	$(MAKE) --no-print-directory hip-variant NAME=nostraight DEFS='-DLR_STRAIGHT_TAIL=0' VARIANT_MASKS='0 1 4096 4097 4098 4099 4100 4101 4102 4103 4116 4117 20482 20483 12308 12309' HEAVY_MASKS=

# Kernels once more WITHOUT the light sample's records (dev_shade.h: LR_LIGHT_RECORDS): a light sample walks light instance -> instance -> alias
# entry -> triangle indices -> three vertices and computes the emissive triangle's normal and area per sample.  TEST INFRASTRUCTURE: the records hold
# what that code computes, from the same function (dev_shade.h: triangle_constants), so the shipped library's frames, its counters and its queries must
# equal this library's (tests/test_gpu_light_records.py).  It holds one record-reading kernel of every family, with its counting twin where the test
# compares counters: the lean one-path kernels <0> - <3> (of them <2> and <3> take the records in the shipped library, kernel_forms.h) and the masks of
# `noride` (of them <20482> is the PaddedSobol pool kernel the test runs); lean + alpha <8>, lean + Disney <16>, environment + Disney <20>; <60>, <124>,
# nested <636>; the sibling integrators <252>; AOV <32892>; the volumetric kernel <256>; the camera and continuation passes of wavefront mode
# <1024> <3072> with the heavy kernels of the three closure kinds, and the pool's <5120> <7168>; the gather kernel <196734>; the radiance query
# kernel <65660>.  The define goes to the units built with VPT_HIPFLAGS too (the volumetric and gather kernels: variant_flags), which HIPFLAGS does not reach.
NOLIGHTREC_MASKS := 0 1 2 3 4096 4097 4098 4099 4100 4101 4102 4103 4116 4117 20482 20483 12308 12309 \
    8 9 16 17 20 21 60 61 124 125 636 252 32892 256 1024 1025 3072 3073 5120 7168 196734 65660
NOLIGHTREC_HEAVY := 0 1 4 5 8 9
nolightrec: $(LIBDIR)/variants/liblrhip_nolightrec.so
$(LIBDIR)/variants/liblrhip_nolightrec.so: $(HIP_SRC) $(HIPDIR)/megapath_variant.hip $(HIPDIR)/heavy_variant.hip $(HIP_HDR) Makefile
	$(MAKE) --no-print-directory hip-variant NAME=nolightrec DEFS='-DLR_LIGHT_RECORDS=0' VPT_HIPFLAGS='$(VPT_HIPFLAGS) -DLR_LIGHT_RECORDS=0' \
	    VARIANT_MASKS='$(NOLIGHTREC_MASKS)' HEAVY_MASKS='$(NOLIGHTREC_HEAVY)'

cli: $(BINDIR)/luisa-render-cli
$(BINDIR)/luisa-render-cli: $(HOSTDIR)/cli.cpp $(HOSTDIR)/plugin_megapath.cpp $(LIBDIR)/liblrhost.so $(HOST_HDR)
	@mkdir -p $(BINDIR)
	for impl in megapath direct normal megavptnaive aov; do \
	  $(CXX) $(CXXFLAGS) -DLR_PLUGIN_IMPL=\"$$impl\" -shared -o $(BINDIR)/libluisa-render-integrator-$$impl.so $(HOSTDIR)/plugin_megapath.cpp \
	    -L$(LIBDIR) -llrhost -ldl -Wl,-rpath,'$$ORIGIN/../lib' || exit 1; done
	$(CXX) $(CXXFLAGS) -o $@ $(HOSTDIR)/cli.cpp -L$(LIBDIR) -llrhost -ldl -pthread -Wl,-rpath,'$$ORIGIN/../lib'

clean:
	rm -rf $(LIBDIR)/*.so $(LIBDIR)/obj $(LIBDIR)/variants $(BINDIR)/* oracle/liboracle.so
