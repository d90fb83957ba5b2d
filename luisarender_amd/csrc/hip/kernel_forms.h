// kernel_forms.h — the ONE place where a kernel's feature mask becomes code forms.
//
// Every megakernel variant is its own translation unit (megapath_variant.hip, -DLR_VARIANT=<mask>), so which form of a piece of code a kernel
// takes is a preprocessor choice.  The groups of feature bits behind those choices, the choices themselves and their constexpr twins for the
// host (lrhip_kernels.hip: which kernels will do for a scene) stand here and nowhere else; the measurements behind a form stay next to the
// code it selects.  A unit compiled without LR_VARIANT (the query units lrhip_*.hip, the heavy kernels) takes the right-hand default of
// every form below: none of the per-variant groups holds for it.  megapath_variant.hip asserts that each default equals its twin.
#pragma once
#include <cstdint>

// ---- the feature bits as preprocessor numbers (dev_wavefront.h: the kFeat* enumerators, which describe them, one static_assert each)
#define LR_FEAT_COUNT 1
#define LR_FEAT_GENERIC 2
#define LR_FEAT_ENV 4
#define LR_FEAT_ALPHA 8
#define LR_FEAT_DISNEY 16
#define LR_FEAT_MIX 32
#define LR_FEAT_LAYERED 64
#define LR_FEAT_VPT 256
#define LR_FEAT_NEST 512
#define LR_FEAT_WF 1024
#define LR_FEAT_CONT 2048
#define LR_FEAT_POOL 4096
#define LR_FEAT_BYTE_TEX 8192
#define LR_FEAT_PADDED 16384
#define LR_FEAT_GATHER 131072

// ---- groups of kernels, as predicates of a mask M (numbers only: good in #if and in constant expressions alike)
// the Mix / Layered interpreters: out-of-line closures (dev_heavy.h)
#define LR_MASK_HEAVY_CLOSURES(M) (((M) & (LR_FEAT_MIX | LR_FEAT_LAYERED)) != 0)
// makes real calls: the kernels with those interpreters and the volumetric kernel; every other megakernel variant is LEAN.  (kFeatAux is
// not asked: the sibling integrators exist on the all-closures masks only, which lrhip_kernels.hip asserts of the listed variants)
#define LR_MASK_MAKES_CALLS(M) (((M) & (LR_FEAT_MIX | LR_FEAT_LAYERED | LR_FEAT_VPT)) != 0)
#define LR_MASK_LEAN(M) (!LR_MASK_MAKES_CALLS(M))
#define LR_MASK_LEAN_WITH_DISNEY(M) ((((M) & LR_FEAT_DISNEY) != 0) && LR_MASK_LEAN(M))// what textured scenes of the camera class' kind render on
#define LR_MASK_LEAN_WAVEFRONT_PASS(M) ((((M) & LR_FEAT_WF) != 0) && LR_MASK_LEAN(M))  // the camera and continuation passes of wavefront mode
#define LR_MASK_LEAN_FLOAT_TEXELS(M) (LR_MASK_LEAN(M) && ((M) & LR_FEAT_BYTE_TEX) == 0)// lean and without the kFeatByteTex bit
#define LR_MASK_NESTED_CLOSURES(M) ((((M) & LR_FEAT_NEST) != 0) && ((M) & LR_FEAT_VPT) == 0)
#define LR_MASK_POOL(M) (((M) & LR_FEAT_POOL) != 0)
#define LR_MASK_POOL_WITHOUT_CONT(M) (LR_MASK_POOL(M) && ((M) & LR_FEAT_CONT) == 0)     // every pool kernel but the continuation passes
// built with the library's own arithmetic (Makefile: HIPFLAGS): every kernel but the volumetric and the gather kernels (variant_flags)
#define LR_MASK_LIBRARY_ARITHMETIC(M) (((M) & (LR_FEAT_VPT | LR_FEAT_GATHER)) == 0)
// a kernel or its counting twin, by number: the sets that a measurement names kernel by kernel
#define LR_MASK_OR_TWIN(M, K) (((M) & ~LR_FEAT_COUNT) == (K))
// spill more VGPRs with the light sample's records than without (profiles/light_records_ab.txt, section 3)
#define LR_MASK_KEEPS_LIGHT_GATHERS(M)                                                                                                           \
    (LR_MASK_OR_TWIN(M, 0) || LR_MASK_OR_TWIN(M, 4) || LR_MASK_OR_TWIN(M, 6) || LR_MASK_OR_TWIN(M, 12) || LR_MASK_OR_TWIN(M, 258) ||             \
     LR_MASK_OR_TWIN(M, 1028) ||                                                                                                                 \
     LR_MASK_OR_TWIN(M, 1036) || LR_MASK_OR_TWIN(M, 1038) || LR_MASK_OR_TWIN(M, 3074) || LR_MASK_OR_TWIN(M, 3084) || LR_MASK_OR_TWIN(M, 4110) || \
     LR_MASK_OR_TWIN(M, 4112) || LR_MASK_OR_TWIN(M, 4114) || LR_MASK_OR_TWIN(M, 4116) || LR_MASK_OR_TWIN(M, 5128) || LR_MASK_OR_TWIN(M, 5132) || \
     LR_MASK_OR_TWIN(M, 8210) || LR_MASK_OR_TWIN(M, 20486) || LR_MASK_OR_TWIN(M, 20490) || LR_MASK_OR_TWIN(M, 20498) ||                          \
     LR_MASK_OR_TWIN(M, 28690) || LR_MASK_OR_TWIN(M, 28694) || LR_MASK_OR_TWIN(M, 32894) || LR_MASK_OR_TWIN(M, 196732) ||                        \
     LR_MASK_OR_TWIN(M, 197244))
#define LR_MASK_LEAN_ONE_PATH(M)(((M) & ~(LR_FEAT_COUNT | LR_FEAT_GENERIC | LR_FEAT_ENV | LR_FEAT_ALPHA)) == 0)// the one-path kernels of masks 0 - 15

// LR_IS(group): whether this translation unit's kernel is of the group
#ifdef LR_VARIANT
#define LR_IS(GROUP) (GROUP(LR_VARIANT))
#else
#define LR_IS(GROUP) 0
#endif

// ---- the forms.  LR_DEFAULT_<form> is the rule; the form itself can still be given on the command line (A/B builds, the twin libraries).
// LR_CALL: the texture lookup and the environment's evaluate / sample are real calls in the kernels that make real calls anyway, inline in
// the lean ones (dev_math.h; profiles/archive/r03ae_texture_lambda_ab.txt).  A unit without a mask defines LR_CALL itself.
#ifndef LR_CALL
#if LR_IS(LR_MASK_MAKES_CALLS)
#define LR_CALL __device__ __noinline__
#else
#define LR_CALL __device__ __forceinline__
#endif
#endif
// LR_TEX_LAMBDA_ATTR: load_lobe's lookup of a looked-up slot is the one real call of the lean megakernel variants (dev_math.h;
// profiles/archive/r03ae_texture_lambda_ab.txt)
#ifndef LR_TEX_LAMBDA_ATTR
#if LR_IS(LR_MASK_LEAN)
#define LR_TEX_LAMBDA_ATTR __attribute__((noinline))
#else
#define LR_TEX_LAMBDA_ATTR
#endif
#endif
// LR_LOBE_FORM: 2 the lean kernels with Disney, 3 the lean passes of wavefront mode, 1 everyone else (dev_heavy.h; profiles/r06i_lobe_forms.txt,
// profiles/r06q_lobe_form3.txt)
#define LR_DEFAULT_LOBE_FORM (LR_IS(LR_MASK_LEAN_WITH_DISNEY) ? 2 : LR_IS(LR_MASK_LEAN_WAVEFRONT_PASS) ? 3 : 1)
#ifndef LR_LOBE_FORM
#define LR_LOBE_FORM LR_DEFAULT_LOBE_FORM
#endif
// LR_BYTE_TEXELS: every kernel decodes packed 8-bit texels but the lean ones without the kFeatByteTex bit (dev_shade.h; profiles/r06k_byte_texel_bit.txt)
#define LR_DEFAULT_BYTE_TEXELS (LR_IS(LR_MASK_LEAN_FLOAT_TEXELS) ? 0 : 1)
#ifndef LR_BYTE_TEXELS
#define LR_BYTE_TEXELS LR_DEFAULT_BYTE_TEXELS
#endif
// LR_TEX_WIDE_RECORD: the lean kernels with Disney read a texture's record in one round trip (dev_shade.h; profiles/r06u_texture_record_loads.txt)
#define LR_DEFAULT_TEX_WIDE_RECORD (LR_IS(LR_MASK_LEAN_WITH_DISNEY) ? 1 : 0)
#ifndef LR_TEX_WIDE_RECORD
#define LR_TEX_WIDE_RECORD LR_DEFAULT_TEX_WIDE_RECORD
#endif
// LR_LIGHT_OUT_OF_LINE: the pool kernels with Disney sample a vertex's light in one real call (megapool_kernel.h; profiles/r06zd_light_sample_out_of_line.txt)
#define LR_DEFAULT_LIGHT_OUT_OF_LINE (LR_IS(LR_MASK_LEAN_WITH_DISNEY) ? 1 : 0)
#ifndef LR_LIGHT_OUT_OF_LINE
#define LR_LIGHT_OUT_OF_LINE LR_DEFAULT_LIGHT_OUT_OF_LINE
#endif
// LR_ENV_TREE: the walk of nested Combined environments exists in the kernels that make real calls, and in a unit that asks for it with
// LR_ENV_TREE_WALK (the light and gather queries) (dev_shade.h; no measurement: the lean kernels' allocation is never to see it)
#define LR_DEFAULT_ENV_TREE (LR_IS(LR_MASK_MAKES_CALLS) ? 1 : 0)
#if !defined(LR_ENV_TREE) && (LR_DEFAULT_ENV_TREE || defined(LR_ENV_TREE_WALK))
#define LR_ENV_TREE 1
#endif
// LR_NEST: Mix / Layered nested in each other in the kernels of the kFeatNest bit but the volumetric one (dev_layered.h; a heavy kernel's
// unit defines it from its own mask, heavy_variant.hip)
#define LR_DEFAULT_NEST (LR_IS(LR_MASK_NESTED_CLOSURES) ? 1 : 0)
#ifndef LR_NEST
#define LR_NEST LR_DEFAULT_NEST
#endif
// LR_STRAIGHT_TAIL: both bits in the lean one-path kernels and the pool kernels but the continuation passes (dev_trace.h; profiles/straight_tail_ab.txt)
#define LR_DEFAULT_STRAIGHT_TAIL (LR_IS(LR_MASK_POOL_WITHOUT_CONT) || LR_IS(LR_MASK_LEAN_ONE_PATH) ? 3 : 0)
#ifndef LR_STRAIGHT_TAIL
#define LR_STRAIGHT_TAIL LR_DEFAULT_STRAIGHT_TAIL
#endif
// LR_LEAF_TAIL_ONE_COMPARE: the pool kernels (of them, the ones without the alpha test: dev_trace.h; profiles/r06zq_leaf_tail.txt)
#define LR_DEFAULT_LEAF_TAIL_ONE_COMPARE (LR_IS(LR_MASK_POOL) ? 1 : 0)
#ifndef LR_LEAF_TAIL_ONE_COMPARE
#define LR_LEAF_TAIL_ONE_COMPARE LR_DEFAULT_LEAF_TAIL_ONE_COMPARE
#endif
// LR_LIGHT_RECORDS: the light sample reads the light instance's and the emissive triangle's baked records in every kernel that samples a
// light -- megakernel variants, heavy kernels, the light and gather query units (dev_shade.h: sample_one_light; profiles/light_records_ab.txt)
// -- but the megakernel variants whose code object came out with MORE spilled VGPRs on the records than on the chain of gathers: they keep
// the chain, each with its counting twin, and their code objects are what they were (the table: section 3 of that file).
// 0 everywhere: `make nolightrec`
#define LR_DEFAULT_LIGHT_RECORDS (LR_IS(LR_MASK_KEEPS_LIGHT_GATHERS) ? 0 : 1)
#ifndef LR_LIGHT_RECORDS
#define LR_LIGHT_RECORDS LR_DEFAULT_LIGHT_RECORDS
#endif
// LR_LIGHT_TRIS: WHICH table of triangle records.  A record's ng and area must be the bits the reading kernel computed per sample, so there is
// one table per arithmetic the library is built with (Makefile): light_tris, baked by lrhip_tables.hip under HIPFLAGS, for everything built
// with those; light_tris_exact, baked by lrhip_instance_update.hip -- no contraction, correctly rounded division and square root -- for the
// volumetric and the gather kernels (variant_flags) and for a unit that says it is built that way (LR_EXACT_ARITHMETIC_UNIT: lrhip_light.hip,
// lrhip_gather.hip)
#ifndef LR_LIGHT_TRIS
#if defined(LR_EXACT_ARITHMETIC_UNIT) || (defined(LR_VARIANT) && !LR_IS(LR_MASK_LIBRARY_ARITHMETIC))
#define LR_LIGHT_TRIS light_tris_exact
#else
#define LR_LIGHT_TRIS light_tris
#endif
#endif

// ---- the same rules for the host, of any mask
namespace lrd::forms {
constexpr bool holds_heavy_closures(uint32_t m) { return LR_MASK_HEAVY_CLOSURES(m); }
constexpr bool makes_calls(uint32_t m) { return LR_MASK_MAKES_CALLS(m); }
constexpr bool lean_with_disney(uint32_t m) { return LR_MASK_LEAN_WITH_DISNEY(m); }
constexpr int lobe_form(uint32_t m) { return lean_with_disney(m) ? 2 : LR_MASK_LEAN_WAVEFRONT_PASS(m) ? 3 : 1; }
constexpr bool decodes_byte_texels(uint32_t m) { return !(LR_MASK_LEAN_FLOAT_TEXELS(m)); }
constexpr bool wide_texture_record(uint32_t m) { return lean_with_disney(m); }
constexpr bool light_out_of_line(uint32_t m) { return lean_with_disney(m); }
constexpr bool walks_env_tree(uint32_t m) { return makes_calls(m); }
constexpr bool nests_closures(uint32_t m) { return LR_MASK_NESTED_CLOSURES(m); }
constexpr int straight_tail(uint32_t m) { return LR_MASK_POOL_WITHOUT_CONT(m) || LR_MASK_LEAN_ONE_PATH(m) ? 3 : 0; }
constexpr bool leaf_tail_one_compare(uint32_t m) { return LR_MASK_POOL(m); }
constexpr bool light_records(uint32_t m) { return !(LR_MASK_KEEPS_LIGHT_GATHERS(m)); }
constexpr bool exact_light_triangles(uint32_t m) { return !(LR_MASK_LIBRARY_ARITHMETIC(m)); }
}// namespace lrd::forms
