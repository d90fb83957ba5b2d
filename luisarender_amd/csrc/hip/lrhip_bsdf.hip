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

// records per chunk of a host-pointer call: 32 MiB each of hits, rays and results and 16 MiB of dirs in the staging buffers, whatever the
// count.  Hit records and rays go through the surface and ray queries' staging buffers: every host-pointer call synchronises per chunk
constexpr uint64_t kBsdfChunk = 1ull << 20u;
// blocks of a launch, at most: 2^20 blocks of 256 lanes cover 2^28 records in one pass; a larger batch strides
constexpr uint32_t kBsdfMaxBlocks = 1u << 20u;

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

// one launch over `count` records in device memory, between the context's bsdf events
int query_device(lrhip_ctx *ctx, const void *hits, const void *rays, const void *dirs, void *out, uint32_t count, uint32_t mode) {
    // the lr_mesh table of the uploaded scene, shared with the surface queries: copied once per upload
    if (!ctx->surface_meshes_ready) {
        const auto bytes = ctx->meshes.size() * sizeof(lr_mesh);
        if (auto r = ensure(ctx->surface_meshes, std::max<size_t>(bytes, 16u)); r != LRHIP_OK) { return r; }
        if (bytes != 0u) { LR_HIP_CHECK(hipMemcpyAsync(ctx->surface_meshes.ptr, ctx->meshes.data(), bytes, hipMemcpyHostToDevice, ctx->stream)); }
        ctx->surface_meshes_ready = true;
    }
    lrd::BsdfArgs args{};
    args.hits = static_cast<const float4 *>(hits), args.rays = static_cast<const float4 *>(rays), args.dirs = static_cast<const float4 *>(dirs);
    args.out = static_cast<float4 *>(out);
    args.meshes = static_cast<const lr_mesh *>(ctx->surface_meshes.ptr);
    args.count = count;
    args.triangle_count = ctx->update_counts[1], args.instance_count = ctx->update_counts[2];
    args.mesh_count = static_cast<uint32_t>(ctx->meshes.size());
    const auto blocks = std::min(kBsdfMaxBlocks, (count + lrd::kBlockThreads - 1u) / lrd::kBlockThreads);
    // the scene record as the host holds it now (lrhip_render writes one per launch; none exists before the first render)
    if (auto r = ensure(ctx->scene_record, sizeof(lrd::DScene)); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemcpyAsync(ctx->scene_record.ptr, &ctx->scene, sizeof(lrd::DScene), hipMemcpyHostToDevice, ctx->stream));
    const auto device_scene = (lrd::DScenePtr) static_cast<const lrd::DScene *>(ctx->scene_record.ptr);
    // the closures of the scene's surfaces themselves -- not ctx->features, which the volumetric integrator clears of them and the sibling
    // integrators fill with all of them --, and what lrhip_set_diagnostics forces on top (the twin tests: a lean scene on the heavier kernels)
    const auto features = ctx->closure_features | (ctx->diag_force_features & lrd::kFeatSceneMask);
    LR_HIP_CHECK(hipEventRecord(ctx->bsdf_begin, ctx->stream));
    if (mode == LRHIP_BSDF_EVALUATE) { launch<lrd::kBsdfEvaluate>(features, blocks, ctx->stream, device_scene, args); }
    else { launch<lrd::kBsdfSample>(features, blocks, ctx->stream, device_scene, args); }
    LR_HIP_CHECK(hipGetLastError());
    LR_HIP_CHECK(hipEventRecord(ctx->bsdf_end, ctx->stream));
    ctx->bsdf_pending = true;
    return LRHIP_OK;
}

// the pending launch's time joins the call's sum (synchronises with it)
int collect_time(lrhip_ctx *ctx) {
    if (!ctx->bsdf_pending) { return LRHIP_OK; }
    float ms = 0.f;
    LR_HIP_CHECK(hipEventSynchronize(ctx->bsdf_end));
    LR_HIP_CHECK(hipEventElapsedTime(&ms, ctx->bsdf_begin, ctx->bsdf_end));
    ctx->bsdf_ms += static_cast<double>(ms);
    ctx->bsdf_pending = false;
    return LRHIP_OK;
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_query_bsdf(lrhip_ctx *ctx, const lrhip_bsdf_query_params *p) {
    if (ctx == nullptr || p == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: NULL argument"); }
    if ((p->flags & ~LRHIP_RAY_DEVICE_POINTERS) != 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: unknown flags"); }
    if (p->mode != LRHIP_BSDF_EVALUATE && p->mode != LRHIP_BSDF_SAMPLE) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: unknown mode"); }
    if (p->count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: more than 2^31 - 1 records"); }
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: no scene uploaded"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->hits == nullptr || p->dirs == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: hits / dirs / out is NULL"); }
        if (device_pointers && ((reinterpret_cast<uintptr_t>(p->hits) | reinterpret_cast<uintptr_t>(p->rays) | reinterpret_cast<uintptr_t>(p->dirs) |
                                 reinterpret_cast<uintptr_t>(p->out)) & 15u) != 0u) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_bsdf: device pointers must be 16-byte aligned");
        }
    }
    if ((ctx->features & lrd::kFeatNest) != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_query_bsdf: Mix / Layered surfaces nested in each other are not supported");
    }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->bsdf_ms = 0.0, ctx->bsdf_pending = false;
    if (p->count == 0u) { return LRHIP_OK; }
    if (ctx->bsdf_begin == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->bsdf_begin)); }
    if (ctx->bsdf_end == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->bsdf_end)); }
    if (device_pointers) { return query_device(ctx, p->hits, p->rays, p->dirs, p->out, static_cast<uint32_t>(p->count), p->mode); }
    // host pointers: chunk by chunk through the staging buffers
    const auto chunk = std::min<uint64_t>(p->count, kBsdfChunk);
    if (auto r = ensure(ctx->surface_hits, chunk * sizeof(lrhip_ray_hit)); r != LRHIP_OK) { return r; }
    if (p->rays != nullptr) {
        if (auto r = ensure(ctx->raycast_rays, chunk * sizeof(lrhip_ray)); r != LRHIP_OK) { return r; }
    }
    if (auto r = ensure(ctx->bsdf_dirs, chunk * sizeof(float4)); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->bsdf_out, chunk * sizeof(lrhip_bsdf_result)); r != LRHIP_OK) { return r; }
    for (uint64_t first = 0u; first < p->count; first += chunk) {
        const auto n = std::min<uint64_t>(chunk, p->count - first);
        LR_HIP_CHECK(hipMemcpyAsync(ctx->surface_hits.ptr, static_cast<const lrhip_ray_hit *>(p->hits) + first, n * sizeof(lrhip_ray_hit),
                                    hipMemcpyHostToDevice, ctx->stream));
        if (p->rays != nullptr) {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->raycast_rays.ptr, static_cast<const lrhip_ray *>(p->rays) + first, n * sizeof(lrhip_ray),
                                        hipMemcpyHostToDevice, ctx->stream));
        }
        LR_HIP_CHECK(hipMemcpyAsync(ctx->bsdf_dirs.ptr, static_cast<const float4 *>(p->dirs) + first, n * sizeof(float4), hipMemcpyHostToDevice,
                                    ctx->stream));
        if (auto r = query_device(ctx, ctx->surface_hits.ptr, p->rays != nullptr ? ctx->raycast_rays.ptr : nullptr, ctx->bsdf_dirs.ptr, ctx->bsdf_out.ptr,
                                  static_cast<uint32_t>(n), p->mode); r != LRHIP_OK) { return r; }
        LR_HIP_CHECK(hipMemcpyAsync(static_cast<lrhip_bsdf_result *>(p->out) + first, ctx->bsdf_out.ptr, n * sizeof(lrhip_bsdf_result),
                                    hipMemcpyDeviceToHost, ctx->stream));
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = collect_time(ctx); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

double lrhip_last_bsdf_ms(lrhip_ctx *ctx) {
    if (ctx == nullptr) { return 0.0; }
    if (hipSetDevice(ctx->device) != hipSuccess || collect_time(ctx) != LRHIP_OK) { return -1.0; }
    return ctx->bsdf_ms;
}

}// extern "C"
