// lrhip_lightmap.hip — C ABI of the UV rasteriser of lightmap baking (include/lrhip.h: lrhip_lightmap_texels, lrhip_last_lightmap_ms;
// DESIGN §4.18).  Holds the two kernels of lightmap_kernels.h and their launches on the context's stream, through the queries' one host path
// (lrhip_query.hip: screen_call, staged_call, the timer).  The kernels decide in float64 and are held to a float64 numpy rasteriser
// (tests/gather_reference.py), so this object is built without fp contraction and approximate division (Makefile: lrhip_lightmap_FLAGS).
#include "lrhip_internal.h"
#include "lightmap_kernels.h"

static_assert(sizeof(lrhip_ray_hit) == 32u && offsetof(lrhip_ray_hit, inst) == 12u && offsetof(lrhip_ray_hit, prim) == 16u &&
                  offsetof(lrhip_ray_hit, tri) == 20u && offsetof(lrhip_ray_hit, reserved) == 24u,
              "a texel record is the two float4 lightmap_record_kernel stores");
static_assert(LRHIP_LIGHTMAP_TEXEL_CENTRE == lrd::kLightmapFlagCentre && LRHIP_LIGHTMAP_TEXEL_TOUCHED == lrd::kLightmapFlagTouched,
              "lrhip.h's texel flags are the kernel's");
static_assert((LRHIP_LIGHTMAP_CONSERVATIVE & (LRHIP_RAY_DEVICE_POINTERS | LRHIP_RAY_ALPHA_TEST | LRHIP_RADIANCE_ACCUMULATE | LRHIP_RADIANCE_COUNTERS |
                                              LRHIP_MESH_RECOMPUTE_NORMALS | LRHIP_SURFACE_GEOMETRY_ONLY | LRHIP_LIGHT_FROM_POINTS | LRHIP_SAMPLER_START)) == 0u,
              "the queries' flags share one word");
static_assert(sizeof(lr_vertex) == 32u && offsetof(lr_vertex, u) == 24u && sizeof(lr_triangle) == 12u, "lightmap_load reads u v of three indexed vertices");

using namespace lrh;

namespace {

// texels one wave of the owner pass should take of a triangle that covers its share of the map: 64 iterations
constexpr uint64_t kLightmapWaveTexels = 4096u;
constexpr uint64_t kLightmapMaxSlices = 1024u;

}// namespace

extern "C" {

int lrhip_lightmap_texels(lrhip_ctx *ctx, uint32_t instance, uint32_t width, uint32_t height, uint32_t flags, void *out) {
    const std::string what{"lrhip_lightmap_texels: "};
    const auto count = static_cast<uint64_t>(width) * height;
    // (no parameter block: the context stands in for it in the NULL check)
    if (auto r = screen_call("lrhip_lightmap_texels", ctx, ctx, flags, LRHIP_RAY_DEVICE_POINTERS | LRHIP_LIGHTMAP_CONSERVATIVE, count, "texels"); r != LRHIP_OK) {
        return r;
    }
    if (instance >= ctx->update_counts[2]) {
        return fail(LRHIP_ERROR_INVALID, what + "instance " + std::to_string(instance) + " out of range (" + std::to_string(ctx->update_counts[2]) + " instances)");
    }
    const auto device_pointers = (flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (count != 0u) {
        if (out == nullptr) { return fail(LRHIP_ERROR_INVALID, what + "out is NULL"); }
        if (device_pointers && misaligned({{out, 15u}})) { return fail(LRHIP_ERROR_INVALID, what + "device pointers must be 16-byte aligned"); }
    }
    // the instance's handle as the uploads wrote it (the host's copy: a device-pointer call stays asynchronous)
    if (instance >= ctx->instance_handles.size()) { return fail(LRHIP_ERROR_INVALID, what + "instance " + std::to_string(instance) + " has no record"); }
    const auto handle = ctx->instance_handles[instance];
    const auto mesh_id = handle >> 10u;
    if (mesh_id >= ctx->meshes.size()) { return fail(LRHIP_ERROR_INVALID, what + "instance " + std::to_string(instance) + " has no mesh"); }
    const auto &mesh = ctx->meshes[mesh_id];
    if (static_cast<uint64_t>(mesh.vertex_offset) + mesh.vertex_count > ctx->vertex_count ||
        static_cast<uint64_t>(mesh.triangle_offset) + mesh.triangle_count > ctx->update_counts[3]) {
        return fail(LRHIP_ERROR_INVALID, what + "mesh " + std::to_string(mesh_id) + " of the uploaded scene does not lie inside its vertex and triangle tables");
    }
    if ((handle & LR_SHAPE_HAS_VERTEX_UV) == 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, what + "the mesh of instance " + std::to_string(instance) + " has no vertex UVs: there is no chart to rasterise");
    }
    if (mesh.triangle_count >= lrd::kLightmapTouched) { return fail(LRHIP_ERROR_UNSUPPORTED, what + "a mesh of 2^31 triangles or more"); }
    if (auto r = timer_start(ctx, ctx->lightmap_timer, count != 0u); r != LRHIP_OK) { return r; }
    if (count == 0u) { return LRHIP_OK; }
    // ONE owner array per context, overwritten by every call: safe because every call's memset, owner pass and record pass are ordered on the
    // one context stream (a call that grows the array frees the old one only after hipFree's implicit synchronisation)
    if (auto r = ensure(ctx->lightmap_owner, static_cast<size_t>(count) * sizeof(uint32_t)); r != LRHIP_OK) { return r; }
    lrd::LightmapArgs args{};
    args.vertices = ctx->scene.vertices, args.triangles = ctx->scene.triangles;
    args.owner = static_cast<uint32_t *>(ctx->lightmap_owner.ptr);
    args.instance = instance;
    args.vertex_offset = mesh.vertex_offset, args.vertex_count = mesh.vertex_count;
    args.triangle_offset = mesh.triangle_offset, args.triangle_count = mesh.triangle_count;
    args.width = width, args.height = height;
    args.conservative = (flags & LRHIP_LIGHTMAP_CONSERVATIVE) != 0u ? 1u : 0u;
    const auto share = kLightmapWaveTexels * std::max<uint64_t>(mesh.triangle_count, 1u);
    args.slices = static_cast<uint32_t>(std::min(kLightmapMaxSlices, std::max<uint64_t>((count + share - 1u) / share, 1u)));
    return staged_call(ctx, ctx->lightmap_timer, count, device_pointers, {column_out(out, sizeof(lrhip_ray_hit))},
                       [&](uint32_t n, uint64_t first, void *const *d) {
        auto a = args;
        a.out = static_cast<float4 *>(d[0]), a.first = static_cast<uint32_t>(first), a.count = n;
        if (auto r = timer_begin(ctx, ctx->lightmap_timer); r != LRHIP_OK) { return r; }
        if (first == 0u) {// the owners of the whole map, once per call, in front of the first chunk's records
            LR_HIP_CHECK(hipMemsetAsync(a.owner, 0xff, static_cast<size_t>(count) * sizeof(uint32_t), ctx->stream));
            if (a.triangle_count != 0u) {
                const auto waves_per_block = lrd::kLightmapBlock / 64u;
                const dim3 grid((a.triangle_count + waves_per_block - 1u) / waves_per_block, a.slices);
                hipLaunchKernelGGL(lrd::lightmap_owner_kernel, grid, dim3(lrd::kLightmapBlock), 0, ctx->stream, a);
                LR_HIP_CHECK(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(lrd::lightmap_record_kernel, dim3((n + lrd::kLightmapBlock - 1u) / lrd::kLightmapBlock), dim3(lrd::kLightmapBlock), 0,
                           ctx->stream, a);
        LR_HIP_CHECK(hipGetLastError());
        return timer_end(ctx, ctx->lightmap_timer);
    });
}

double lrhip_last_lightmap_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->lightmap_timer) : 0.0; }

}// extern "C"
