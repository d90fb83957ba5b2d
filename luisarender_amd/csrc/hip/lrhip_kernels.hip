// lrhip_kernels.hip — the table of the kernels compiled into this library (variants.h), the rule that picks the kernels of a call
// (plan_kernels: the only place that decides) and their occupancy.
#include "lrhip_internal.h"

// one translation unit per precompiled kernel (megapath_variant.hip, -DLR_VARIANT=<mask>; heavy_variant.hip, -DLR_HVARIANT=<mask>)
#define LR_DECLARE_KERNEL(family, mask)                                                                                     \
    extern "C" __attribute__((weak)) hipError_t lrhip_##family##_launch_##mask(unsigned, hipStream_t, const lrd::DScene *,         \
                                                                              const lrd::RenderArgs *, unsigned);                \
    extern "C" __attribute__((weak)) hipError_t lrhip_##family##_occupancy_##mask(int *, unsigned);
#define LR_DECLARE_VARIANT(mask) LR_DECLARE_KERNEL(variant, mask)
#define LR_DECLARE_HEAVY(mask) LR_DECLARE_KERNEL(heavy, mask)
LR_MEGAKERNEL_LIST(LR_DECLARE_VARIANT)
LR_HEAVY_LIST(LR_DECLARE_HEAVY)

namespace lrh {

#define LR_VARIANT_ENTRY(mask) KernelEntry{mask##u, false, lrhip_variant_launch_##mask, lrhip_variant_occupancy_##mask},
#define LR_HEAVY_ENTRY(mask) KernelEntry{mask##u, true, lrhip_heavy_launch_##mask, lrhip_heavy_occupancy_##mask},
const KernelEntry kKernels[kKernelCount] = {LR_MEGAKERNEL_LIST(LR_VARIANT_ENTRY) LR_HEAVY_LIST(LR_HEAVY_ENTRY)};

// variants.h against lrd::kSceneVariants, at compile time: the search below may name any kSceneVariants[i] x {counters} x {generic sampler},
// and the padded / AOV / query kernels are asked for by their defining bit
namespace {
#define LR_MASK(mask) mask##u,
constexpr uint32_t kListedVariants[] = {LR_VARIANT_LIST(LR_MASK)};
constexpr uint32_t kListedPadded[] = {LR_PADDED_LIST(LR_MASK)};
constexpr uint32_t kListedAov[] = {LR_AOV_LIST(LR_MASK)};
constexpr uint32_t kListedQuery[] = {LR_QUERY_LIST(LR_MASK)};
constexpr uint32_t kListedGather[] = {LR_GATHER_LIST(LR_MASK)};
#undef LR_MASK
constexpr bool scene_variants_are_listed() {
    for (auto scene : lrd::kSceneVariants) {
        for (uint32_t twin : {0u, 0u + lrd::kFeatCount, 0u + lrd::kFeatGeneric, lrd::kFeatCount | lrd::kFeatGeneric}) {
            auto found = false;
            for (auto listed : kListedVariants) { found = found || listed == (scene | twin); }
            if (!found) { return false; }
        }
    }
    return true;
}
template<size_t N>
constexpr bool all_carry(const uint32_t (&list)[N], uint32_t bits) {
    for (auto mask : list) {
        if ((mask & bits) != bits) { return false; }
    }
    return true;
}
static_assert(scene_variants_are_listed(), "variants.h: LR_VARIANT_LIST lacks a mask of lrd::kSceneVariants x {kFeatCount} x {kFeatGeneric}");
static_assert(all_carry(kListedPadded, lrd::kFeatPadded | lrd::kFeatGeneric | lrd::kFeatPool),
    "variants.h: LR_PADDED_LIST holds PaddedSobol pool kernels");
static_assert(all_carry(kListedAov, lrd::kFeatAov | lrd::kFeatSceneMask),
    "variants.h: LR_AOV_LIST holds kFeatAov kernels on the all-closures mask");
static_assert(all_carry(kListedQuery, lrd::kFeatQuery | lrd::kFeatSceneMask),
    "variants.h: LR_QUERY_LIST holds kFeatQuery kernels on the all-closures mask");
static_assert(all_carry(kListedGather, lrd::kFeatGather | lrd::kFeatQuery | lrd::kFeatSceneMask) && !all_carry(kListedGather, lrd::kFeatCount) &&
                  sizeof(kListedGather) / sizeof(kListedGather[0]) == 4u,
    "variants.h: LR_GATHER_LIST holds the four kFeatGather kernels on top of the query kernels' all-closures mask, without counting twins");
}// namespace

const KernelEntry *find_kernel(uint32_t mask, bool heavy) {
    for (auto &k : kKernels) {
        if (k.mask == mask && k.heavy == heavy) { return k.launch != nullptr && k.occupancy != nullptr ? &k : nullptr; }
    }
    return nullptr;
}

int kernel_blocks(lrhip_ctx *ctx, const KernelEntry &entry, unsigned lds_bytes, uint32_t &blocks_per_cu) {
    auto &cached = ctx->kernel_blocks[&entry - kKernels];
    if (cached < 0) {
        int per_cu = 0;
        LR_HIP_CHECK(entry.occupancy(&per_cu, lds_bytes));
        cached = std::max(1, std::min(per_cu, static_cast<int>(kMaxBlocksPerCu)));
    }
    blocks_per_cu = static_cast<uint32_t>(cached);
    return LRHIP_OK;
}

namespace {

// Which code forms a kernel of a mask holds -- out-of-line closures, real calls, the decode of packed 8-bit texels -- is kernel_forms.h's to say
// (lrd::forms: the rules the kernels themselves are compiled by).  The sibling integrators and the volumetric kernel are a selection concept:
constexpr uint32_t kSiblingBits = lrd::kFeatAux | lrd::kFeatVpt;
// (a sibling integrator's kernel is never lean: the device's rule for "makes real calls" does not ask kFeatAux, the search below relies on it)
constexpr bool siblings_make_calls() {
    for (auto v : lrd::kSceneVariants) {
        if ((v & kSiblingBits) != 0u && !lrd::forms::makes_calls(v)) { return false; }
    }
    return true;
}
static_assert(siblings_make_calls(), "lrd::kSceneVariants: a kFeatAux / kFeatVpt feature set without Mix, Layered or the volumetric kernel");

// smallest precompiled superset of the scene's feature bits among the feature sets of one scheduler (lrd::kSceneVariants, first superset wins):
// `pool` = the path-pool kernels of round 4 (megapool_kernel.h), otherwise the one-path-per-lane kernels.  `byte_texels`: see above; a scene
// without packed texels never takes a kFeatByteTex kernel.  kNoKernel: no feature set covers the scene.
uint32_t pick_scene_variant(uint32_t scene_features, bool pool, bool byte_texels) {
    for (auto v : lrd::kSceneVariants) {
        if (((v & lrd::kFeatPool) != 0u) != pool) { continue; }
        if (byte_texels ? !lrd::forms::decodes_byte_texels(v) : (v & lrd::kFeatByteTex) != 0u) { continue; }
        if ((v & scene_features) == scene_features) { return v; }
    }
    return kNoKernel;
}

}// namespace

// Which kernels a call of lrhip_render runs on.  A function of its inputs and of which kernels are in the loaded library, in two places only:
// a scene whose POOL twin or PaddedSobol twin is not compiled in takes the plain kernel instead; every other missing kernel is the caller's
// LRHIP_ERROR_UNSUPPORTED when it resolves the plan's masks (find_kernel).  Every call of a frame must land in the same family -- their film
// sums differ in their last bits -- so nothing here depends on a call's sample range except `fixed_fits`, and lrhip_render cuts a call
// that does not fit into sub-ranges that do wherever `fixed_point` would hold for them.
KernelPlan plan_kernels(const PlanInputs &in) {
    KernelPlan plan{LRHIP_FAMILY_NONE, kNoKernel, kNoKernel, {kNoKernel, kNoKernel, kNoKernel}, false};
    static_assert(lrd::kWfKinds == 3u, "KernelPlan::heavy");
    const auto generic = in.sampler_kind != LR_SAMPLER_INDEPENDENT;// generic-sampler instantiation
    const auto twin = (in.count ? lrd::kFeatCount : 0u) | (generic ? lrd::kFeatGeneric : 0u);
    // the AOV integrator: kernels of its own on top of the all-closures mask, fp32 sums like the film of rounds 1-3
    if ((in.features & lrd::kFeatAov) != 0u) {
        plan.family = LRHIP_FAMILY_AOV, plan.main = lrd::kFeatSceneMask | lrd::kFeatAov | twin;
        return plan;
    }
    // lrhip_set_diagnostics: A/B of a variant on a scene that does not need it
    auto features = in.features | (in.force_features & lrd::kFeatSceneMask);
    const auto sibling = (features & kSiblingBits) != 0u;
    // nested Combined environments are walked by out-of-line code (dev_shade.h: LR_ENV_TREE), which the variants that make real calls
    // anyway hold -- the ones with the Mix interpreter (the auxiliary and volumetric kernels are such variants already)
    static_assert(lrd::forms::walks_env_tree(lrd::kFeatMix), "kernel_forms.h: a kernel with the Mix interpreter walks nested environments");
    if (in.env_tree && !sibling) { features |= lrd::kFeatMix; }
    const auto plain = pick_scene_variant(features, false, in.byte_texels);
    if (plain == kNoKernel) { return plan; }
    auto pool = false;
    // Wavefront mode (lrhip_wavefront.hip) for every MegaPath scene that would otherwise land in an all-in-one variant with
    // out-of-line closures: Mix / Layered surfaces, and Disney together with an alpha test (no lean <Alpha | Disney> variant is
    // precompiled; such a scene ran at 433 Msamples/s on <60> where its Mix-holding sibling ran at 480 in wavefront mode).
    // (it needs the film's fixed-point sums: a frame they cannot hold -- fixed_point_bits -- takes the float-accumulating kernels)
    if (in.fixed_fits && in.wf_mode != 1u && in.force_features == 0u && !in.env_tree && !sibling && lrd::forms::holds_heavy_closures(plain)) {
        // kernels: the lean camera pass + continuation pass with the scene's environment / alpha needs, the heavy kernel with its nesting
        // (the alpha-tested traversal only where a surface may be non-opaque: the kitchen stand-in with its lace made opaque runs at 530.6
        // instead of 520.5 Msamples/s on the lean kernels without it, profiles/archive/r03ar_wavefront_without_alpha_ab.txt)
        const auto lean = (in.features & (lrd::kFeatEnv | lrd::kFeatAlpha)) | lrd::kFeatWf | twin;
        // round 4: both lean passes under the path-pool scheduler (megapool_kernel.h) where those kernels are in the library
        pool = in.wants_pool && find_kernel(lean | lrd::kFeatPool) != nullptr && find_kernel(lean | lrd::kFeatPool | lrd::kFeatCont) != nullptr;
        plan.family = LRHIP_FAMILY_WAVEFRONT, plan.fixed_point = true;
        plan.main = lean | (pool ? lrd::kFeatPool : 0u), plan.cont = plan.main | lrd::kFeatCont;
        const auto nest = (in.features & lrd::kFeatNest) != 0u ? 512u : 0u;
        for (auto k = 0u; k < lrd::kWfKinds; k++) {// (LR_HEAVY_LIST's numbering; Disney, k = 0, has no nested form)
            plan.heavy[k] = (k << 2u) | (k != 0u ? nest : 0u) | (in.count ? 1u : 0u) | (generic ? 2u : 0u);
        }
    } else {
        // round 4: the path-pool scheduler where a pool kernel is compiled for a scene the search gives a lean kernel (no out-of-line
        // closures, no sibling integrator), and the fixed-point film can hold the frame
        if (in.wants_pool && in.fixed_fits && in.max_depth < 65536u && !lrd::forms::makes_calls(plain)) {
            const auto pooled = pick_scene_variant(features, true, in.byte_texels);
            pool = pooled != kNoKernel && (pooled & lrd::kFeatWf) == 0u && find_kernel(pooled | twin) != nullptr;
            if (pool) { plan.main = pooled | twin; }
        }
        if (!pool) { plan.main = plain | twin; }
        plan.family = pool ? LRHIP_FAMILY_POOL : LRHIP_FAMILY_LANE, plan.fixed_point = pool;
    }
    // round 6: the pool kernels compiled for the PaddedSobol sampler (variants.h: LR_PADDED_LIST), where the scene's sampler is that and
    // such a kernel exists for every lean kernel of the plan
    if (pool && in.sampler_kind == LR_SAMPLER_PADDED_SOBOL && find_kernel(plan.main | lrd::kFeatPadded) != nullptr &&
        (plan.cont == kNoKernel || find_kernel(plan.cont | lrd::kFeatPadded) != nullptr)) {
        plan.main |= lrd::kFeatPadded;
        if (plan.cont != kNoKernel) { plan.cont |= lrd::kFeatPadded; }
    }
    return plan;
}

// Whether the kernels a scene renders on decode packed 8-bit texels, from what lrhip_upload_scene knows BEFORE it packs (the feature bits do not
// exist yet).  It must agree with plan_kernels above -- a packed scene must land on decoding kernels, never in wavefront mode -- which
// tests/test_ffi_abi.py checks over the whole input space through lrhip_plan_kernels.  Round 6: the decode is compiled into the lean kernels of
// the kFeatByteTex bit only, which exist for the Disney feature sets of both schedulers (dev_wavefront.h): a scene with alpha-tested surfaces,
// Mix or Layered surfaces (wavefront mode: lean passes without the decode) or nested Combined environments keeps float texels.  The sibling
// integrators and the volumetric kernel run on variants that always decode.
bool scene_kernels_decode_byte_texels(bool alpha_tested, bool mix_or_layered, bool env_tree, bool megapath) {
    return !megapath || !(alpha_tested || mix_or_layered || env_tree);
}

}// namespace lrh

extern "C" int lrhip_plan_kernels(uint32_t features, uint32_t force_features, uint32_t flags, uint32_t sampler_kind, uint32_t wf_mode,
                                  uint32_t max_depth, uint32_t out[LRHIP_PLAN_WORDS]) {
    using namespace lrh;
    if (out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_plan_kernels: out is NULL"); }
    PlanInputs in{};
    in.features = features, in.force_features = force_features, in.sampler_kind = sampler_kind, in.wf_mode = wf_mode, in.max_depth = max_depth;
    in.count = (flags & LRHIP_PLAN_FLAG_COUNTERS) != 0u, in.env_tree = (flags & LRHIP_PLAN_FLAG_ENV_TREE) != 0u;
    in.byte_texels = (flags & LRHIP_PLAN_FLAG_PACKED_TEXELS) != 0u, in.wants_pool = (flags & LRHIP_PLAN_FLAG_WANTS_POOL) != 0u;
    in.fixed_fits = (flags & LRHIP_PLAN_FLAG_FIXED_FITS) != 0u;
    const auto plan = plan_kernels(in);
    out[0] = plan.family, out[1] = plan.main, out[2] = plan.cont;
    for (auto k = 0u; k < lrd::kWfKinds; k++) { out[3u + k] = plan.heavy[k]; }
    out[6] = plan.fixed_point ? 1u : 0u;
    const auto megapath = (features & (kSiblingBits | lrd::kFeatAov)) == 0u;
    const auto packs = scene_kernels_decode_byte_texels((features & lrd::kFeatAlpha) != 0u, lrd::forms::holds_heavy_closures(features), in.env_tree, megapath);
    out[7] = packs ? 1u : 0u;
    auto compiled = plan.family != LRHIP_FAMILY_NONE;
    for (auto mask : {plan.main, plan.cont}) { compiled = compiled && (mask == kNoKernel || find_kernel(mask) != nullptr); }
    for (auto mask : plan.heavy) { compiled = compiled && (mask == kNoKernel || find_kernel(mask, true) != nullptr); }
    if (!compiled) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_plan_kernels: a kernel of the plan is not compiled into this library"); }
    return LRHIP_OK;
}
