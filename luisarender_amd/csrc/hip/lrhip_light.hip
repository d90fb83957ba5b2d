// lrhip_light.hip — C ABI of the light queries (include/lrhip.h: lrhip_query_light, lrhip_last_light_ms).  Holds the three
// instantiations of light_kernel.h (sample from hits, sample from bare points, evaluate) and their launches on the context's stream.  The
// texture lookup is ONE real call in this translation unit, and so are the environment's evaluate / sample (as in heavy_variant.hip and
// lrhip_bsdf.hip).  LR_ENV_TREE_WALK: this unit holds dev_shade.h's walk of Combined environments nested in each other, which only the
// call-making megakernel variants compile otherwise -- a query serves every scene.  The object is built with the oracle's arithmetic, as
// lrhip_bsdf.o and for its reason (Makefile: lrhip_light_FLAGS): a query hands single answers to its caller
#define LR_CALL __device__ __noinline__
#define LR_ENV_TREE_WALK 1
#define LR_EXACT_ARITHMETIC_UNIT 1// (Makefile: this unit's flags; kernel_forms.h: LR_LIGHT_TRIS)
#include "lrhip_internal.h"
#include "light_kernel.h"

static_assert(sizeof(lrhip_light_result) == 32u && offsetof(lrhip_light_result, pdf) == 12u && offsetof(lrhip_light_result, kind) == 16u &&
                  offsetof(lrhip_light_result, reserved) == 20u,
              "lrhip_light_result = the two float4 light_kernel stores");
static_assert(LRHIP_LIGHT_SAMPLE == lrd::kLightSample && LRHIP_LIGHT_EVALUATE == lrd::kLightEvaluate, "lrhip.h's modes are the kernel's");
static_assert(LRHIP_LIGHT_KIND_AREA == lrd::kLightKindArea && LRHIP_LIGHT_KIND_ENVIRONMENT == lrd::kLightKindEnvironment &&
                  LRHIP_LIGHT_KIND_NONE == lrd::kLightKindNone,
              "lrhip.h's kinds are the kernel's");
static_assert(sizeof(lrhip_ray) == 32u && offsetof(lrhip_ray, t_min) == 12u && offsetof(lrhip_ray, d) == 16u && offsetof(lrhip_ray, t_max) == 28u,
              "a shadow ray is two dwordx4 stores (light_kernel.h)");
static_assert((LRHIP_LIGHT_FROM_POINTS & (LRHIP_RAY_DEVICE_POINTERS | LRHIP_RAY_ALPHA_TEST | LRHIP_RADIANCE_ACCUMULATE | LRHIP_RADIANCE_COUNTERS |
                                          LRHIP_MESH_RECOMPUTE_NORMALS | LRHIP_SURFACE_GEOMETRY_ONLY)) == 0u,
              "the queries' flags share one word");

namespace lrd {
template __global__ void light_kernel<kLightSample, false>(DScenePtr, LightArgs);
template __global__ void light_kernel<kLightSample, true>(DScenePtr, LightArgs);
template __global__ void light_kernel<kLightEvaluate, false>(DScenePtr, LightArgs);
}

using namespace lrh;

extern "C" {

int lrhip_query_light(lrhip_ctx *ctx, const lrhip_light_query_params *p) {
    if (auto r = screen("lrhip_query_light", ctx, p, LRHIP_RAY_DEVICE_POINTERS | LRHIP_LIGHT_FROM_POINTS, "records"); r != LRHIP_OK) { return r; }
    if (p->mode != LRHIP_LIGHT_SAMPLE && p->mode != LRHIP_LIGHT_EVALUATE) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: unknown mode"); }
    const auto sample = p->mode == LRHIP_LIGHT_SAMPLE;
    const auto points = (p->flags & LRHIP_LIGHT_FROM_POINTS) != 0u;
    if (points && !sample) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: LRHIP_LIGHT_FROM_POINTS is for LRHIP_LIGHT_SAMPLE only"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    // what the mode does not read or write is not looked at
    const auto rays = sample ? nullptr : p->rays;
    const auto dirs = sample ? p->dirs : nullptr;
    const auto out_rays = sample ? p->out_rays : nullptr;
    if (p->count != 0u) {
        if (p->hits == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: hits / out is NULL"); }
        if (sample && (dirs == nullptr || out_rays == nullptr)) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: dirs / out_rays is NULL in sample mode"); }
        if (!sample && rays == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: rays is NULL in evaluate mode"); }
        if (device_pointers && misaligned({{p->hits, 15u}, {rays, 15u}, {dirs, 15u}, {out_rays, 15u}, {p->out, 15u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: device pointers must be 16-byte aligned");
        }
    }
    if (auto r = timer_start(ctx, ctx->light_timer, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    return staged_call(ctx, ctx->light_timer, p->count, device_pointers,
                       {column_out(p->out, sizeof(lrhip_light_result)), column_in(rays, sizeof(lrhip_ray)),
                        column_in(p->hits, points ? sizeof(float4) : sizeof(lrhip_ray_hit)), column_in(dirs, sizeof(float4)),
                        column_out(out_rays, sizeof(lrhip_ray))},
                       [&](uint32_t n, uint64_t, void *const *d) {
        if (auto r = resident_meshes(ctx); r != LRHIP_OK) { return r; }
        lrd::LightArgs args{};
        fill_hit_table(ctx, args, d[2], d[1], n);
        args.dirs = static_cast<const float4 *>(d[3]), args.out_rays = static_cast<float4 *>(d[4]), args.out = static_cast<float4 *>(d[0]);
        lrd::DScenePtr device_scene{};
        if (auto r = upload_scene_record(ctx, device_scene); r != LRHIP_OK) { return r; }
        if (auto r = timer_begin(ctx, ctx->light_timer); r != LRHIP_OK) { return r; }
        const dim3 grid(blocks_of(n)), block(lrd::kBlockThreads);
        if (!sample) { hipLaunchKernelGGL((lrd::light_kernel<lrd::kLightEvaluate, false>), grid, block, 0, ctx->stream, device_scene, args); }
        else if (points) { hipLaunchKernelGGL((lrd::light_kernel<lrd::kLightSample, true>), grid, block, 0, ctx->stream, device_scene, args); }
        else { hipLaunchKernelGGL((lrd::light_kernel<lrd::kLightSample, false>), grid, block, 0, ctx->stream, device_scene, args); }
        LR_HIP_CHECK(hipGetLastError());
        return timer_end(ctx, ctx->light_timer);
    });
}

double lrhip_last_light_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->light_timer) : 0.0; }

}// extern "C"
