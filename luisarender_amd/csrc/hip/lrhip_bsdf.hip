// lrhip_bsdf.hip — C ABI of the BSDF queries (include/lrhip.h: lrhip_query_bsdf, lrhip_last_bsdf_ms).  Holds the six
// instantiations of bsdf_kernel.h (evaluate / sample x no heavy closure / Mix / Mix and Layered) and their launches on the context's stream.
// The texture lookup is ONE real call in this translation unit (as in heavy_variant.hip and lrhip_surface.hip).  The object is built with the
// oracle's arithmetic -- no fp contraction, correctly rounded division and square root, no approximate functions (Makefile: lrhip_bsdf_FLAGS) --
// because a query hands single closure answers to its caller: with the renderers' flags Glass' pdf under total internal reflection came out
// 1e-8 for the reference's 0 and the visible-normal sampling 2e-3 away from the oracle's direction
#define LR_CALL __device__ __noinline__
#include "lrhip_internal.h"
#include "bsdf_kernel.h"

static_assert(sizeof(lrhip_bsdf_result) == 32u && offsetof(lrhip_bsdf_result, pdf) == 12u && offsetof(lrhip_bsdf_result, wi) == 16u &&
                  offsetof(lrhip_bsdf_result, event) == 28u,
              "lrhip_bsdf_result = the two float4 bsdf_kernel stores");
static_assert(LRHIP_BSDF_EVALUATE == lrd::kBsdfEvaluate && LRHIP_BSDF_SAMPLE == lrd::kBsdfSample, "lrhip.h's modes are the kernel's");
// (dev_bsdf.h writes Surface::event_through as the literal 4 where the thin Disney closure samples its transmission)
static_assert(LRHIP_BSDF_EVENT_REFLECT == lrd::kEventReflect && LRHIP_BSDF_EVENT_ENTER == lrd::kEventEnter &&
                  LRHIP_BSDF_EVENT_EXIT == lrd::kEventExit && LRHIP_BSDF_EVENT_THROUGH == 4u,
              "lrhip.h's event codes are dev_bsdf.h's");
static_assert(sizeof(lrhip_ray_hit) == 32u && offsetof(lrhip_ray_hit, u) == 4u && offsetof(lrhip_ray_hit, inst) == 12u &&
                  offsetof(lrhip_ray_hit, prim) == 16u && offsetof(lrhip_ray_hit, tri) == 20u,
              "a hit record is two dwordx4 loads (bsdf_kernel.h)");

namespace lrd {
template __global__ void bsdf_kernel<kBsdfEvaluate, false, false>(DScenePtr, BsdfArgs);
template __global__ void bsdf_kernel<kBsdfEvaluate, true, false>(DScenePtr, BsdfArgs);
template __global__ void bsdf_kernel<kBsdfEvaluate, true, true>(DScenePtr, BsdfArgs);
template __global__ void bsdf_kernel<kBsdfSample, false, false>(DScenePtr, BsdfArgs);
template __global__ void bsdf_kernel<kBsdfSample, true, false>(DScenePtr, BsdfArgs);
template __global__ void bsdf_kernel<kBsdfSample, true, true>(DScenePtr, BsdfArgs);
}

namespace lrh {

namespace {

template<uint32_t MODE>
void launch(uint32_t features, uint32_t blocks, hipStream_t stream, lrd::DScenePtr scene, const lrd::BsdfArgs &args) {
    // which interpreters the scene needs (bsdf_kernel.h): anything with Layered takes the kernel that holds both
    if ((features & lrd::kFeatLayered) != 0u) {
        hipLaunchKernelGGL((lrd::bsdf_kernel<MODE, true, true>), dim3(blocks), dim3(lrd::kBlockThreads), 0, stream, scene, args);
    } else if ((features & lrd::kFeatMix) != 0u) {
        hipLaunchKernelGGL((lrd::bsdf_kernel<MODE, true, false>), dim3(blocks), dim3(lrd::kBlockThreads), 0, stream, scene, args);
    } else {
        hipLaunchKernelGGL((lrd::bsdf_kernel<MODE, false, false>), dim3(blocks), dim3(lrd::kBlockThreads), 0, stream, scene, args);
    }
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_query_bsdf(lrhip_ctx *ctx, const lrhip_bsdf_query_params *p) {
    if (auto r = screen("lrhip_query_bsdf", ctx, p, LRHIP_RAY_DEVICE_POINTERS, "records"); r != LRHIP_OK) { return r; }
    if (p->mode != LRHIP_BSDF_EVALUATE && p->mode != LRHIP_BSDF_SAMPLE) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: unknown mode"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->hits == nullptr || p->dirs == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: hits / dirs / out is NULL"); }
        if (device_pointers && misaligned({{p->hits, 15u}, {p->rays, 15u}, {p->dirs, 15u}, {p->out, 15u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: device pointers must be 16-byte aligned");
        }
    }
    if ((ctx->features & lrd::kFeatNest) != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_query_bsdf: Mix / Layered surfaces nested in each other are not supported");
    }
    if (auto r = timer_start(ctx, ctx->bsdf_timer, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    // the closures of the scene's surfaces themselves -- not ctx->features, which the volumetric integrator clears of them and the sibling
    // integrators fill with all of them --, and what lrhip_set_diagnostics forces on top (the twin tests: a lean scene on the heavier kernels)
    const auto features = ctx->closure_features | (ctx->diag_force_features & lrd::kFeatSceneMask);
    return staged_call(ctx, ctx->bsdf_timer, p->count, device_pointers,
                       {column_out(p->out, sizeof(lrhip_bsdf_result)), column_in(p->rays, sizeof(lrhip_ray)), column_in(p->hits, sizeof(lrhip_ray_hit)),
                        column_in(p->dirs, sizeof(float4))},
                       [&](uint32_t n, uint64_t, void *const *d) {
        if (auto r = resident_meshes(ctx); r != LRHIP_OK) { return r; }
        lrd::BsdfArgs args{};
        fill_hit_table(ctx, args, d[2], d[1], n);
        args.dirs = static_cast<const float4 *>(d[3]), args.out = static_cast<float4 *>(d[0]);
        lrd::DScenePtr device_scene{};
        if (auto r = upload_scene_record(ctx, device_scene); r != LRHIP_OK) { return r; }
        if (auto r = timer_begin(ctx, ctx->bsdf_timer); r != LRHIP_OK) { return r; }
        if (p->mode == LRHIP_BSDF_EVALUATE) { launch<lrd::kBsdfEvaluate>(features, blocks_of(n), ctx->stream, device_scene, args); }
        else { launch<lrd::kBsdfSample>(features, blocks_of(n), ctx->stream, device_scene, args); }
        LR_HIP_CHECK(hipGetLastError());
        return timer_end(ctx, ctx->bsdf_timer);
    });
}

double lrhip_last_bsdf_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->bsdf_timer) : 0.0; }

}// extern "C"
