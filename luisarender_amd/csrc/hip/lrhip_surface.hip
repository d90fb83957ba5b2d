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

using namespace lrh;

extern "C" {

int lrhip_query_surface(lrhip_ctx *ctx, const lrhip_surface_query_params *p) {
    if (auto r = screen("lrhip_query_surface", ctx, p, LRHIP_RAY_DEVICE_POINTERS | LRHIP_SURFACE_GEOMETRY_ONLY, "records"); r != LRHIP_OK) { return r; }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->hits == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_surface: hits / out is NULL"); }
        if (device_pointers && misaligned({{p->hits, 15u}, {p->rays, 15u}, {p->out, 15u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_surface: device pointers must be 16-byte aligned");
        }
    }
    const auto full = (p->flags & LRHIP_SURFACE_GEOMETRY_ONLY) == 0u;
    if (full && (ctx->features & lrd::kFeatNest) != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_query_surface: albedo and roughness of Mix / Layered surfaces nested in each other are not "
                                             "supported (LRHIP_SURFACE_GEOMETRY_ONLY serves the scene)");
    }
    if (auto r = timer_start(ctx, ctx->surface_timer, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    return staged_call(ctx, ctx->surface_timer, p->count, device_pointers,
                       {column_out(p->out, sizeof(lrhip_surface_point)), column_in(p->rays, sizeof(lrhip_ray)), column_in(p->hits, sizeof(lrhip_ray_hit))},
                       [&](uint32_t n, uint64_t, void *const *d) {
        if (auto r = resident_meshes(ctx); r != LRHIP_OK) { return r; }
        lrd::SurfaceArgs args{};
        fill_hit_table(ctx, args, d[2], d[1], n);
        args.out = static_cast<float4 *>(d[0]);
        lrd::DScenePtr device_scene{};
        if (auto r = upload_scene_record(ctx, device_scene); r != LRHIP_OK) { return r; }
        if (auto r = timer_begin(ctx, ctx->surface_timer); r != LRHIP_OK) { return r; }
        if (full) { hipLaunchKernelGGL(lrd::surface_kernel<true>, dim3(blocks_of(n)), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args); }
        else { hipLaunchKernelGGL(lrd::surface_kernel<false>, dim3(blocks_of(n)), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args); }
        LR_HIP_CHECK(hipGetLastError());
        return timer_end(ctx, ctx->surface_timer);
    });
}

double lrhip_last_surface_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->surface_timer) : 0.0; }

}// extern "C"
