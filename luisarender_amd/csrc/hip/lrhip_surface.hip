// lrhip_surface.hip — C ABI of the surface queries (include/lrhip.h: lrhip_query_surface, lrhip_last_surface_ms).  Holds the two
// instantiations of surface_kernel.h (geometry only / full) and their launches on the context's stream.
// The texture lookup is ONE real call in this translation unit (as in heavy_variant.hip): the closure code asks for it in some twenty places
#define LR_CALL __device__ __noinline__
#include "lrhip_internal.h"
#include "surface_kernel.h"

static_assert(sizeof(lrhip_surface_point) == 128u, "a surface point is eight dwordx4 stores");
static_assert(offsetof(lrhip_surface_point, area) == 12u && offsetof(lrhip_surface_point, ng) == 16u && offsetof(lrhip_surface_point, flags) == 28u &&
                  offsetof(lrhip_surface_point, ns) == 32u && offsetof(lrhip_surface_point, inst) == 44u && offsetof(lrhip_surface_point, tangent) == 48u &&
                  offsetof(lrhip_surface_point, prim) == 60u && offsetof(lrhip_surface_point, n_closure) == 64u &&
                  offsetof(lrhip_surface_point, closure_kind) == 76u && offsetof(lrhip_surface_point, uv) == 80u &&
                  offsetof(lrhip_surface_point, roughness) == 88u && offsetof(lrhip_surface_point, albedo) == 96u &&
                  offsetof(lrhip_surface_point, surface) == 108u && offsetof(lrhip_surface_point, emission) == 112u &&
                  offsetof(lrhip_surface_point, light) == 124u,
              "lrhip_surface_point = the eight float4 surface_kernel stores");
static_assert(LRHIP_SURFACE_VALID == lrd::kSurfaceValid && LRHIP_SURFACE_BACK_FACING == lrd::kSurfaceBackFacing &&
                  LRHIP_SURFACE_HAS_SURFACE == lrd::kSurfaceHasSurface && LRHIP_SURFACE_HAS_LIGHT == lrd::kSurfaceHasLight,
              "lrhip.h's flag bits are the kernel's");
static_assert(sizeof(lrhip_ray_hit) == 32u && offsetof(lrhip_ray_hit, u) == 4u && offsetof(lrhip_ray_hit, inst) == 12u &&
                  offsetof(lrhip_ray_hit, prim) == 16u && offsetof(lrhip_ray_hit, tri) == 20u,
              "a hit record is two dwordx4 loads (surface_kernel.h)");
static_assert(offsetof(lrd::DShadeTri, inst) == 112u && offsetof(lrd::DShadeTri, prim) == 116u, "surface_kernel.h reads words 28 and 29 of a shading record");

namespace lrd {
template __global__ void surface_kernel<false>(DScenePtr, SurfaceArgs);
template __global__ void surface_kernel<true>(DScenePtr, SurfaceArgs);
}

namespace lrh {

namespace {

// records per chunk of a host-pointer call: 32 MiB of hits, as much of rays and 128 MiB of results in the staging buffers, whatever the count
constexpr uint64_t kSurfaceChunk = 1ull << 20u;
// blocks of a launch, at most: 2^20 blocks of 256 lanes cover 2^28 records in one pass; a larger batch strides
constexpr uint32_t kSurfaceMaxBlocks = 1u << 20u;

// one launch over `count` records in device memory, between the context's surface events
int query_device(lrhip_ctx *ctx, const void *hits, const void *rays, void *out, uint32_t count, bool full) {
    // the lr_mesh table of the uploaded scene: copied once per upload (the host copy is lrhip_set_mesh_vertices')
    if (!ctx->surface_meshes_ready) {
        const auto bytes = ctx->meshes.size() * sizeof(lr_mesh);
        if (auto r = ensure(ctx->surface_meshes, std::max<size_t>(bytes, 16u)); r != LRHIP_OK) { return r; }
        if (bytes != 0u) { LR_HIP_CHECK(hipMemcpyAsync(ctx->surface_meshes.ptr, ctx->meshes.data(), bytes, hipMemcpyHostToDevice, ctx->stream)); }
        ctx->surface_meshes_ready = true;
    }
    lrd::SurfaceArgs args{};
    args.hits = static_cast<const float4 *>(hits), args.rays = static_cast<const float4 *>(rays), args.out = static_cast<float4 *>(out);
    args.meshes = static_cast<const lr_mesh *>(ctx->surface_meshes.ptr);
    args.count = count;
    args.triangle_count = ctx->update_counts[1], args.instance_count = ctx->update_counts[2];
    args.mesh_count = static_cast<uint32_t>(ctx->meshes.size());
    const auto blocks = std::min(kSurfaceMaxBlocks, (count + lrd::kBlockThreads - 1u) / lrd::kBlockThreads);
    // the scene record as the host holds it now (lrhip_render writes one per launch; none exists before the first render)
    if (auto r = ensure(ctx->scene_record, sizeof(lrd::DScene)); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemcpyAsync(ctx->scene_record.ptr, &ctx->scene, sizeof(lrd::DScene), hipMemcpyHostToDevice, ctx->stream));
    const auto device_scene = (lrd::DScenePtr) static_cast<const lrd::DScene *>(ctx->scene_record.ptr);
    LR_HIP_CHECK(hipEventRecord(ctx->surface_begin, ctx->stream));
    if (full) { hipLaunchKernelGGL(lrd::surface_kernel<true>, dim3(blocks), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args); }
    else { hipLaunchKernelGGL(lrd::surface_kernel<false>, dim3(blocks), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args); }
    LR_HIP_CHECK(hipGetLastError());
    LR_HIP_CHECK(hipEventRecord(ctx->surface_end, ctx->stream));
    ctx->surface_pending = true;
    return LRHIP_OK;
}

// the pending launch's time joins the call's sum (synchronises with it)
int collect_time(lrhip_ctx *ctx) {
    if (!ctx->surface_pending) { return LRHIP_OK; }
    float ms = 0.f;
    LR_HIP_CHECK(hipEventSynchronize(ctx->surface_end));
    LR_HIP_CHECK(hipEventElapsedTime(&ms, ctx->surface_begin, ctx->surface_end));
    ctx->surface_ms += static_cast<double>(ms);
    ctx->surface_pending = false;
    return LRHIP_OK;
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_query_surface(lrhip_ctx *ctx, const lrhip_surface_query_params *p) {
    if (ctx == nullptr || p == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_surface: NULL argument"); }
    if ((p->flags & ~(LRHIP_RAY_DEVICE_POINTERS | LRHIP_SURFACE_GEOMETRY_ONLY)) != 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_surface: unknown flags"); }
    if (p->count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_surface: more than 2^31 - 1 records"); }
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_surface: no scene uploaded"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->hits == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_surface: hits / out is NULL"); }
        if (device_pointers &&
            ((reinterpret_cast<uintptr_t>(p->hits) | reinterpret_cast<uintptr_t>(p->rays) | reinterpret_cast<uintptr_t>(p->out)) & 15u) != 0u) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_surface: device pointers must be 16-byte aligned");
        }
    }
    const auto full = (p->flags & LRHIP_SURFACE_GEOMETRY_ONLY) == 0u;
    if (full && (ctx->features & lrd::kFeatNest) != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_query_surface: albedo and roughness of Mix / Layered surfaces nested in each other are not "
                                             "supported (LRHIP_SURFACE_GEOMETRY_ONLY serves the scene)");
    }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->surface_ms = 0.0, ctx->surface_pending = false;
    if (p->count == 0u) { return LRHIP_OK; }
    if (ctx->surface_begin == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->surface_begin)); }
    if (ctx->surface_end == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->surface_end)); }
    if (device_pointers) { return query_device(ctx, p->hits, p->rays, p->out, static_cast<uint32_t>(p->count), full); }
    // host pointers: chunk by chunk through the staging buffers
    const auto chunk = std::min<uint64_t>(p->count, kSurfaceChunk);
    if (auto r = ensure(ctx->surface_hits, chunk * sizeof(lrhip_ray_hit)); r != LRHIP_OK) { return r; }
    if (p->rays != nullptr) {
        if (auto r = ensure(ctx->raycast_rays, chunk * sizeof(lrhip_ray)); r != LRHIP_OK) { return r; }
    }
    if (auto r = ensure(ctx->surface_out, chunk * sizeof(lrhip_surface_point)); r != LRHIP_OK) { return r; }
    for (uint64_t first = 0u; first < p->count; first += chunk) {
        const auto n = std::min<uint64_t>(chunk, p->count - first);
        LR_HIP_CHECK(hipMemcpyAsync(ctx->surface_hits.ptr, static_cast<const lrhip_ray_hit *>(p->hits) + first, n * sizeof(lrhip_ray_hit),
                                    hipMemcpyHostToDevice, ctx->stream));
        if (p->rays != nullptr) {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->raycast_rays.ptr, static_cast<const lrhip_ray *>(p->rays) + first, n * sizeof(lrhip_ray),
                                        hipMemcpyHostToDevice, ctx->stream));
        }
        if (auto r = query_device(ctx, ctx->surface_hits.ptr, p->rays != nullptr ? ctx->raycast_rays.ptr : nullptr, ctx->surface_out.ptr,
                                  static_cast<uint32_t>(n), full); r != LRHIP_OK) { return r; }
        LR_HIP_CHECK(hipMemcpyAsync(static_cast<lrhip_surface_point *>(p->out) + first, ctx->surface_out.ptr, n * sizeof(lrhip_surface_point),
                                    hipMemcpyDeviceToHost, ctx->stream));
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = collect_time(ctx); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

double lrhip_last_surface_ms(lrhip_ctx *ctx) {
    if (ctx == nullptr) { return 0.0; }
    if (hipSetDevice(ctx->device) != hipSuccess || collect_time(ctx) != LRHIP_OK) { return -1.0; }
    return ctx->surface_ms;
}

}// extern "C"
