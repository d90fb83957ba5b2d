// lrhip_light.hip — C ABI of the light queries (include/lrhip.h: lrhip_query_light, lrhip_last_light_ms).  Holds the three
// instantiations of light_kernel.h (sample from hits, sample from bare points, evaluate) and their launches on the context's stream.  The
// texture lookup is ONE real call in this translation unit, and so are the environment's evaluate / sample (as in heavy_variant.hip and
// lrhip_bsdf.hip).  LR_ENV_TREE_WALK: this unit holds dev_shade.h's walk of Combined environments nested in each other, which only the
// call-making megakernel variants compile otherwise -- a query serves every scene.  The object is built with the oracle's arithmetic, as
// lrhip_bsdf.o and for its reason (Makefile: lrhip_light_FLAGS): a query hands single answers to its caller
#define LR_CALL __device__ __noinline__
#define LR_ENV_TREE_WALK 1
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

namespace lrh {

namespace {

// records per chunk of a host-pointer call: 32 MiB each of hits, rays and results and 16 MiB of dirs in the staging buffers, whatever the
// count; every host-pointer call synchronises per chunk
constexpr uint64_t kLightChunk = 1ull << 20u;
// blocks of a launch, at most: 2^20 blocks of 256 lanes cover 2^28 records in one pass; a larger batch strides
constexpr uint32_t kLightMaxBlocks = 1u << 20u;

// one launch over `count` records in device memory, between the context's light events
int query_device(lrhip_ctx *ctx, const void *hits, const void *rays, const void *dirs, void *out_rays, void *out, uint32_t count, uint32_t mode,
                 bool points) {
    // the lr_mesh table of the uploaded scene, shared with the surface and BSDF queries: copied once per upload
    if (!ctx->surface_meshes_ready) {
        const auto bytes = ctx->meshes.size() * sizeof(lr_mesh);
        if (auto r = ensure(ctx->surface_meshes, std::max<size_t>(bytes, 16u)); r != LRHIP_OK) { return r; }
        if (bytes != 0u) { LR_HIP_CHECK(hipMemcpyAsync(ctx->surface_meshes.ptr, ctx->meshes.data(), bytes, hipMemcpyHostToDevice, ctx->stream)); }
        ctx->surface_meshes_ready = true;
    }
    lrd::LightArgs args{};
    args.hits = static_cast<const float4 *>(hits), args.rays = static_cast<const float4 *>(rays), args.dirs = static_cast<const float4 *>(dirs);
    args.out_rays = static_cast<float4 *>(out_rays), args.out = static_cast<float4 *>(out);
    args.meshes = static_cast<const lr_mesh *>(ctx->surface_meshes.ptr);
    args.count = count;
    args.triangle_count = ctx->update_counts[1], args.instance_count = ctx->update_counts[2];
    args.mesh_count = static_cast<uint32_t>(ctx->meshes.size());
    const auto blocks = std::min(kLightMaxBlocks, (count + lrd::kBlockThreads - 1u) / lrd::kBlockThreads);
    // the scene record as the host holds it now (lrhip_render writes one per launch; none exists before the first render)
    if (auto r = ensure(ctx->scene_record, sizeof(lrd::DScene)); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemcpyAsync(ctx->scene_record.ptr, &ctx->scene, sizeof(lrd::DScene), hipMemcpyHostToDevice, ctx->stream));
    const auto device_scene = (lrd::DScenePtr) static_cast<const lrd::DScene *>(ctx->scene_record.ptr);
    LR_HIP_CHECK(hipEventRecord(ctx->light_begin, ctx->stream));
    if (mode == LRHIP_LIGHT_EVALUATE) {
        hipLaunchKernelGGL((lrd::light_kernel<lrd::kLightEvaluate, false>), dim3(blocks), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args);
    } else if (points) {
        hipLaunchKernelGGL((lrd::light_kernel<lrd::kLightSample, true>), dim3(blocks), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args);
    } else {
        hipLaunchKernelGGL((lrd::light_kernel<lrd::kLightSample, false>), dim3(blocks), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args);
    }
    LR_HIP_CHECK(hipGetLastError());
    LR_HIP_CHECK(hipEventRecord(ctx->light_end, ctx->stream));
    ctx->light_pending = true;
    return LRHIP_OK;
}

// the pending launch's time joins the call's sum (synchronises with it)
int collect_time(lrhip_ctx *ctx) {
    if (!ctx->light_pending) { return LRHIP_OK; }
    float ms = 0.f;
    LR_HIP_CHECK(hipEventSynchronize(ctx->light_end));
    LR_HIP_CHECK(hipEventElapsedTime(&ms, ctx->light_begin, ctx->light_end));
    ctx->light_ms += static_cast<double>(ms);
    ctx->light_pending = false;
    return LRHIP_OK;
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_query_light(lrhip_ctx *ctx, const lrhip_light_query_params *p) {
    if (ctx == nullptr || p == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: NULL argument"); }
    if ((p->flags & ~(LRHIP_RAY_DEVICE_POINTERS | LRHIP_LIGHT_FROM_POINTS)) != 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: unknown flags"); }
    if (p->mode != LRHIP_LIGHT_SAMPLE && p->mode != LRHIP_LIGHT_EVALUATE) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: unknown mode"); }
    const auto sample = p->mode == LRHIP_LIGHT_SAMPLE;
    const auto points = (p->flags & LRHIP_LIGHT_FROM_POINTS) != 0u;
    if (points && !sample) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: LRHIP_LIGHT_FROM_POINTS is for LRHIP_LIGHT_SAMPLE only"); }
    if (p->count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: more than 2^31 - 1 records"); }
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: no scene uploaded"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    // what the mode does not read or write is not looked at
    const auto rays = sample ? nullptr : p->rays;
    const auto dirs = sample ? p->dirs : nullptr;
    const auto out_rays = sample ? p->out_rays : nullptr;
    if (p->count != 0u) {
        if (p->hits == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: hits / out is NULL"); }
        if (sample && (dirs == nullptr || out_rays == nullptr)) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: dirs / out_rays is NULL in sample mode"); }
        if (!sample && rays == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: rays is NULL in evaluate mode"); }
        if (device_pointers && ((reinterpret_cast<uintptr_t>(p->hits) | reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(dirs) |
                                 reinterpret_cast<uintptr_t>(out_rays) | reinterpret_cast<uintptr_t>(p->out)) & 15u) != 0u) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_light: device pointers must be 16-byte aligned");
        }
    }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->light_ms = 0.0, ctx->light_pending = false;
    if (p->count == 0u) { return LRHIP_OK; }
    if (ctx->light_begin == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->light_begin)); }
    if (ctx->light_end == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->light_end)); }
    if (device_pointers) { return query_device(ctx, p->hits, rays, dirs, out_rays, p->out, static_cast<uint32_t>(p->count), p->mode, points); }
    // host pointers: chunk by chunk through the staging buffers
    const auto chunk = std::min<uint64_t>(p->count, kLightChunk);
    const auto hit_bytes = points ? sizeof(float4) : sizeof(lrhip_ray_hit);
    if (auto r = ensure(ctx->surface_hits, chunk * hit_bytes); r != LRHIP_OK) { return r; }
    if (sample) {
        if (auto r = ensure(ctx->bsdf_dirs, chunk * sizeof(float4)); r != LRHIP_OK) { return r; }
        if (auto r = ensure(ctx->light_rays, chunk * sizeof(lrhip_ray)); r != LRHIP_OK) { return r; }
    } else {
        if (auto r = ensure(ctx->raycast_rays, chunk * sizeof(lrhip_ray)); r != LRHIP_OK) { return r; }
    }
    if (auto r = ensure(ctx->light_out, chunk * sizeof(lrhip_light_result)); r != LRHIP_OK) { return r; }
    for (uint64_t first = 0u; first < p->count; first += chunk) {
        const auto n = std::min<uint64_t>(chunk, p->count - first);
        LR_HIP_CHECK(hipMemcpyAsync(ctx->surface_hits.ptr, static_cast<const char *>(p->hits) + first * hit_bytes, n * hit_bytes, hipMemcpyHostToDevice,
                                    ctx->stream));
        if (sample) {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->bsdf_dirs.ptr, static_cast<const float4 *>(dirs) + first, n * sizeof(float4), hipMemcpyHostToDevice,
                                        ctx->stream));
        } else {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->raycast_rays.ptr, static_cast<const lrhip_ray *>(rays) + first, n * sizeof(lrhip_ray),
                                        hipMemcpyHostToDevice, ctx->stream));
        }
        if (auto r = query_device(ctx, ctx->surface_hits.ptr, sample ? nullptr : ctx->raycast_rays.ptr, sample ? ctx->bsdf_dirs.ptr : nullptr,
                                  sample ? ctx->light_rays.ptr : nullptr, ctx->light_out.ptr, static_cast<uint32_t>(n), p->mode, points);
            r != LRHIP_OK) { return r; }
        if (sample) {
            LR_HIP_CHECK(hipMemcpyAsync(static_cast<lrhip_ray *>(out_rays) + first, ctx->light_rays.ptr, n * sizeof(lrhip_ray), hipMemcpyDeviceToHost,
                                        ctx->stream));
        }
        LR_HIP_CHECK(hipMemcpyAsync(static_cast<lrhip_light_result *>(p->out) + first, ctx->light_out.ptr, n * sizeof(lrhip_light_result),
                                    hipMemcpyDeviceToHost, ctx->stream));
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = collect_time(ctx); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

double lrhip_last_light_ms(lrhip_ctx *ctx) {
    if (ctx == nullptr) { return 0.0; }
    if (hipSetDevice(ctx->device) != hipSuccess || collect_time(ctx) != LRHIP_OK) { return -1.0; }
    return ctx->light_ms;
}

}// extern "C"
