// surface_kernel.h — surface queries (include/lrhip.h: lrhip_query_surface): what is AT a hit the caller names -- world
// position, normals, uv, the closure's albedo / roughness and the light's emission -- as one 128-byte lrhip_surface_point per record.
//
// One lane per record, no LDS, no queue: lanes are independent and the work per record is short, so the grid simply covers the batch (a
// grid-stride loop if the launch is capped).  The lane loads its 32-byte hit record as two dwordx4 (and its ray as two more), checks every
// index the record names BEFORE it is used -- a malformed record becomes the invalid record, it never faults --, reconstructs the point with
// the renderers' own code (dev_shade.h: reconstruct_baked for a BVH triangle index, reconstruct<true> for (inst, prim)), resolves the
// closure as the shading block does (dev_heavy.h: load_lobe, then closure_albedo_roughness / heavy_albedo_roughness), evaluates the light
// (light_evaluate) and stores eight dwordx4.  This file holds no shading arithmetic of its own: a record's result is what a render computes
// at that hit, and a function of (record, ray, scene) only.
//
// FULL = false (LRHIP_SURFACE_GEOMETRY_ONLY) compiles none of the texture, closure or light code, as raycast_kernel<false> holds no alpha test.
#pragma once
#include "raycast_kernel.h"

namespace lrd {

struct SurfaceArgs {
    const float4 *hits;     // lrhip_ray_hit[count]: (t, u, v, inst), (prim, tri, -, -)
    const float4 *rays;     // lrhip_ray[count]: (o, t_min), (d, t_max); nullptr: every point is seen from its front
    float4 *out;            // lrhip_surface_point[count], eight float4 each
    const lr_mesh *meshes;  // [mesh_count]: bounds `prim` of a record that names an instance
    uint32_t count;
    uint32_t triangle_count;// BVH triangles = shading records
    uint32_t instance_count;
    uint32_t mesh_count;
};

// lrhip_surface_point::flags (lrhip.h: LRHIP_SURFACE_*)
enum : uint32_t { kSurfaceValid = 1u, kSurfaceBackFacing = 2u, kSurfaceHasSurface = 4u, kSurfaceHasLight = 8u };

// wo of a caller's ray: -d / |d| by the rule of the radiance queries (megapath_kernel.h, the kFeatQuery prologue) -- a direction that is unit
// length to within rounding is taken bit for bit; any other finite non-zero one is scaled by a power of two first, so that neither the
// squares nor the hardware's reciprocal and square root meet a denormal or overflow
LR_D f3 surface_unit_direction(f3 d) {
    if (!(fabsf(dot(d, d) - 1.f) <= 4e-7f)) {
        const auto m = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
        const auto pre = m < 0x1p-40f ? 0x1p100f : (m > 0x1p40f ? 0x1p-100f : 1.f);
        const auto dp = d * pre;
        const auto len = sqrtf(dot(dp, dp));
        d = dp * (1.f / len);
    }
    return d;
}

template<bool FULL>
__global__ __launch_bounds__(kBlockThreads) void surface_kernel(DScenePtr scene_ptr, SurfaceArgs args) {
    const DScene &scene = *(const DScene *)scene_ptr;
    const auto stride = gridDim.x * kBlockThreads;
    for (auto k = blockIdx.x * kBlockThreads + threadIdx.x; k < args.count; k += stride) {
        const auto hp = args.hits + static_cast<size_t>(k) * 2u;
        const auto h0 = hp[0], h1 = hp[1];
        const auto u = h0.y, v = h0.z;
        auto inst = __float_as_uint(h0.w), prim = __float_as_uint(h1.x);
        const auto tri = __float_as_uint(h1.y);
        auto valid = raycast_finite(u) && raycast_finite(v);
        f3 origin = mk3(0.f), wo = mk3(0.f);
        if (args.rays != nullptr) {
            const auto rp = args.rays + static_cast<size_t>(k) * 2u;
            const auto a = rp[0], b = rp[1];
            valid = valid && raycast_ray_valid(a, b);
            if (valid) { origin = mk3(a.x, a.y, a.z), wo = -surface_unit_direction(mk3(b.x, b.y, b.z)); }
        }
        // ---- which triangle: every index is checked before it is used
        SurfacePoint it;
        if (valid) {
            if (tri < args.triangle_count) {// the renderer's path: the baked shading record, which names its instance and primitive
                reconstruct_baked(scene, tri, u, v, it);
                const auto ids = reinterpret_cast<const uint32_t *>(scene.shade_tris + tri);
                inst = ids[28], prim = ids[29];// DShadeTri::inst, prim: the BVH triangle's (lrhip_tables.hip: build_shade_tris)
            } else if (tri == kInvalid && inst < args.instance_count) {// a texel's (inst, prim, u, v)
                const auto mesh = scene.instances[inst].handle[0] >> 10u;
                valid = mesh < args.mesh_count && prim < args.meshes[mesh].triangle_count;
                if (valid) { reconstruct<true>(scene, inst, prim, mk3(1.f - u - v, u, v), it); }
            } else {
                valid = false;
            }
        }
        const auto record = args.out + static_cast<size_t>(k) * 8u;
        if (!valid) {// the invalid record: zeros, and every id LR_INVALID_ID
            const auto none = __uint_as_float(kInvalid);
            record[0] = make_float4(0.f, 0.f, 0.f, 0.f), record[1] = make_float4(0.f, 0.f, 0.f, 0.f);
            record[2] = make_float4(0.f, 0.f, 0.f, none), record[3] = make_float4(0.f, 0.f, 0.f, none);
            record[4] = make_float4(0.f, 0.f, 0.f, none), record[5] = make_float4(0.f, 0.f, 0.f, 0.f);
            record[6] = make_float4(0.f, 0.f, 0.f, none), record[7] = make_float4(0.f, 0.f, 0.f, none);
            continue;
        }
        // ---- viewing direction (megapath_kernel.h: the shading block's wo and back_facing)
        if (args.rays == nullptr) { wo = it.ng, origin = it.p + it.ng; }
        it.back_facing = dot(wo, it.ng) < 0.0f;
        const auto has_surface = (it.flags & LR_SHAPE_HAS_SURFACE) != 0u;
        const auto has_light = (it.flags & LR_SHAPE_HAS_LIGHT) != 0u;
        const auto surface = (it.tags >> 12u) & 4095u;
        auto n_closure = it.shading.n;
        auto closure_kind = kInvalid;
        f3 albedo = mk3(0.f), emission = mk3(0.f);
        f2 roughness{0.f, 0.f};
        if constexpr (FULL) {
            if (scene.has_lights && has_light) {// hit light, mega_path.cpp:79-86
                float pdf;
                light_evaluate(scene, it, prim, origin, emission, pdf);
            }
            if (has_surface) {// the shading block's material, megapath_kernel.h (mega_path.cpp:111-143), as far as the AOV buffers need it
                const LobeTables tables{scene.closures, scene.surfaces, scene.textures, scene.texels};
                DClosure closure;
                Frame sh;
                load_lobe(tables, it.uv, it.ng, wo, surface, it.shading, closure, sh);
                if (closure.kind >= LR_SURFACE_DISNEY) {
                    HeavyCtx heavy;
                    heavy.tb = tables, heavy.uv = it.uv, heavy.ng = it.ng, heavy.p = it.p, heavy.wo = wo;
                    heavy.shading = sh, heavy.closure = closure;
                    heavy_albedo_roughness<true, true>(&heavy, &albedo, &roughness);
                } else {
                    closure_albedo_roughness(closure, albedo, roughness);
                }
                n_closure = sh.n, closure_kind = closure.kind;
            }
        }
        const auto flags = kSurfaceValid | (it.back_facing ? kSurfaceBackFacing : 0u) | (has_surface ? kSurfaceHasSurface : 0u) |
                           (has_light ? kSurfaceHasLight : 0u);
        record[0] = make_float4(it.p.x, it.p.y, it.p.z, it.area);
        record[1] = make_float4(it.ng.x, it.ng.y, it.ng.z, __uint_as_float(flags));
        record[2] = make_float4(it.shading.n.x, it.shading.n.y, it.shading.n.z, __uint_as_float(inst));
        record[3] = make_float4(it.shading.s.x, it.shading.s.y, it.shading.s.z, __uint_as_float(prim));
        record[4] = make_float4(n_closure.x, n_closure.y, n_closure.z, __uint_as_float(closure_kind));
        record[5] = make_float4(it.uv.x, it.uv.y, roughness.x, roughness.y);
        record[6] = make_float4(albedo.x, albedo.y, albedo.z, __uint_as_float(has_surface ? surface : kInvalid));
        record[7] = make_float4(emission.x, emission.y, emission.z, __uint_as_float(has_light ? (it.tags & 4095u) : kInvalid));
    }
}

}// namespace lrd
