// bsdf_kernel.h — BSDF queries (include/lrhip.h: lrhip_query_bsdf): the closure's answer at a hit the caller names -- its value
// and pdf for a direction the caller gives (MODE = kBsdfEvaluate), or a sampled direction with its value, pdf and event for three random
// numbers the caller gives (MODE = kBsdfSample) -- as one 32-byte lrhip_bsdf_result per record.
//
// One lane per record, no LDS, no queue, as surface_kernel.h: the lane loads its hit record, its ray and its float4 of `dirs` as dwordx4,
// checks every index the record names BEFORE it is used, reconstructs the point with the renderers' own code (bsdf_resolve_hit: the front
// half of surface_kernel, to the letter), resolves the closure with load_lobe and then makes exactly the calls the MegaPath shading block
// makes (megapath_kernel.h: closure_evaluate / closure_sample inline for the basic closures, heavy_evaluate / heavy_sample through a
// HeavyCtx for Disney / Mix / Layered surfaces when this instantiation holds Mix or Layered -- the inline interpreter then leaves Disney
// out, <DISNEY && !HEAVY_CALL> as there), for radiance transport with eta_i = 1, and stores two dwordx4.  This file holds no shading
// arithmetic of its own.
//
// MIX / LAYERED: which interpreters the instantiation holds, as in the megakernel's variants.  The host picks <false, false> for scenes
// without Mix and Layered surfaces (Disney inline, no HeavyCtx, no out-of-line closure), <true, false> for scenes with Mix and <true, true>
// for anything with Layered: the Layered interpreter's LayerStack and walk state live in scratch, and a scene without such a surface
// should not reserve that frame in every wave.
#pragma once
#include "surface_kernel.h"

namespace lrd {

struct BsdfArgs {
    const float4 *hits;     // lrhip_ray_hit[count]: (t, u, v, inst), (prim, tri, -, -)
    const float4 *rays;     // lrhip_ray[count]: (o, t_min), (d, t_max); nullptr: wo = ng
    const float4 *dirs;     // [count]: (wi, -) or (u_lobe, u_x, u_y, -)
    float4 *out;            // lrhip_bsdf_result[count], two float4 each
    const lr_mesh *meshes;  // [mesh_count]: bounds `prim` of a record that names an instance
    uint32_t count;
    uint32_t triangle_count;// BVH triangles = shading records
    uint32_t instance_count;
    uint32_t mesh_count;
};

enum : uint32_t { kBsdfEvaluate = 0u, kBsdfSample = 1u };// lrhip.h: LRHIP_BSDF_EVALUATE / LRHIP_BSDF_SAMPLE

// hit record k -> the point and its viewing direction, exactly as surface_kernel resolves them: a non-finite u or v, a ray the ray queries
// would screen, a miss or an id out of range give false, and nothing the record names is read before it is checked
LR_D bool bsdf_resolve_hit(const DScene &scene, const BsdfArgs &args, uint32_t k, SurfacePoint &it, f3 &wo) {
    const auto hp = args.hits + static_cast<size_t>(k) * 2u;
    const auto h0 = hp[0], h1 = hp[1];
    const auto u = h0.y, v = h0.z;
    const auto inst = __float_as_uint(h0.w), prim = __float_as_uint(h1.x), tri = __float_as_uint(h1.y);
    auto valid = raycast_finite(u) && raycast_finite(v);
    wo = mk3(0.f);
    if (args.rays != nullptr) {
        const auto rp = args.rays + static_cast<size_t>(k) * 2u;
        const auto a = rp[0], b = rp[1];
        valid = valid && raycast_ray_valid(a, b);
        if (valid) { wo = -surface_unit_direction(mk3(b.x, b.y, b.z)); }
    }
    if (!valid) { return false; }
    if (tri < args.triangle_count) {// the renderer's path: the baked shading record
        reconstruct_baked(scene, tri, u, v, it);
    } else if (tri == kInvalid && inst < args.instance_count) {// a texel's (inst, prim, u, v)
        const auto mesh = scene.instances[inst].handle[0] >> 10u;
        if (!(mesh < args.mesh_count && prim < args.meshes[mesh].triangle_count)) { return false; }
        reconstruct<true>(scene, inst, prim, mk3(1.f - u - v, u, v), it);
    } else {
        return false;
    }
    if (args.rays == nullptr) { wo = it.ng; }
    it.back_facing = dot(wo, it.ng) < 0.0f;
    return true;
}

template<uint32_t MODE, bool MIX, bool LAYERED>
__global__ __launch_bounds__(kBlockThreads) void bsdf_kernel(DScenePtr scene_ptr, BsdfArgs args) {
    const DScene &scene = *(const DScene *)scene_ptr;
    const auto stride = gridDim.x * kBlockThreads;
    for (auto k = blockIdx.x * kBlockThreads + threadIdx.x; k < args.count; k += stride) {
        const auto q = args.dirs[k];
        const auto record = args.out + static_cast<size_t>(k) * 2u;
        SurfacePoint it;
        f3 wo;
        auto valid = raycast_finite(q.x) && raycast_finite(q.y) && raycast_finite(q.z);
        if (MODE == kBsdfEvaluate) { valid = valid && ((__float_as_uint(q.x) | __float_as_uint(q.y) | __float_as_uint(q.z)) & 0x7fffffffu) != 0u; }
        valid = valid && bsdf_resolve_hit(scene, args, k, it, wo);
        valid = valid && (it.flags & LR_SHAPE_HAS_SURFACE) != 0u;
        if (!valid) {// the invalid record: zeros, event LR_INVALID_ID
            record[0] = make_float4(0.f, 0.f, 0.f, 0.f), record[1] = make_float4(0.f, 0.f, 0.f, __uint_as_float(kInvalid));
            continue;
        }
        // ---- material, as the shading block reaches it (megapath_kernel.h; mega_path.cpp:111-143)
        constexpr bool HEAVY_CALL = MIX || LAYERED;
        const LobeTables tables{scene.closures, scene.surfaces, scene.textures, scene.texels};
        DClosure closure;
        Frame sh;
        load_lobe(tables, it.uv, it.ng, wo, (it.tags >> 12u) & 4095u, it.shading, closure, sh);
        const auto is_heavy = HEAVY_CALL && closure.kind >= LR_SURFACE_DISNEY;
        HeavyCtx heavy;
        if (is_heavy) {
            heavy.tb = tables, heavy.uv = it.uv, heavy.ng = it.ng, heavy.p = it.p, heavy.wo = wo;
            heavy.shading = sh, heavy.closure = closure;
        }
        if (MODE == kBsdfEvaluate) {
            const auto wi = surface_unit_direction(mk3(q.x, q.y, q.z));
            BsdfEval eval;
            if (is_heavy) { eval = heavy_evaluate<MIX, LAYERED>(&heavy, wi); }
            else { eval = closure_evaluate<!HEAVY_CALL>(closure, sh, it.ng, wo, wi); }
            record[0] = make_float4(eval.f.x, eval.f.y, eval.f.z, eval.pdf);
            record[1] = make_float4(wi.x, wi.y, wi.z, __uint_as_float(kEventReflect));
        } else {
            BsdfSample bs;
            if (is_heavy) { bs = heavy_sample<MIX, LAYERED>(&heavy, q.x, f2{q.y, q.z}).bs; }
            else { bs = closure_sample<!HEAVY_CALL>(closure, sh, it.ng, wo, q.x, f2{q.y, q.z}); }
            record[0] = make_float4(bs.f.x, bs.f.y, bs.f.z, bs.pdf);
            record[1] = make_float4(bs.wi.x, bs.wi.y, bs.wi.z, __uint_as_float(bs.event));
        }
    }
}

}// namespace lrd
