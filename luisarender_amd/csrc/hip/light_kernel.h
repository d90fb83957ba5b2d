// light_kernel.h — light queries (include/lrhip.h: lrhip_query_light): the scene's emitters as seen from a point the caller
// names -- one light or the environment sampled for three random numbers the caller gives, with its radiance, its pdf and the shadow ray
// (MODE = kLightSample; POINTS: the point is a bare position instead of a hit record), or what a ray the caller traced found at its end,
// an emitter's radiance or the environment's, with the pdf light sampling would have had for it (MODE = kLightEvaluate) -- as one 32-byte
// lrhip_light_result per record, and in sample mode one 32-byte lrhip_ray beside it.
//
// One lane per record, no LDS, no queue, as bsdf_kernel.h: the lane loads its record(s) as dwordx4, checks every index the record names
// BEFORE it is used (bsdf_resolve_hit, the BSDF queries' own), and then makes exactly the calls the MegaPath shading block makes
// (megapath_kernel.h: sample_one_light for the light sample; light_evaluate with the selection probability for a hit on an emitter;
// env_evaluate, with the shortcut for a constant environment, for a miss).  This file holds no sampling arithmetic of its own.
//
// A scene with neither lights nor an environment (wave-uniform, tested first) answers kLightKindNone for every record and reads no light
// table: sample_one_light must not be called without anything to pick.
#pragma once
#include "bsdf_kernel.h"

namespace lrd {

struct LightArgs {
    const float4 *hits;     // lrhip_ray_hit[count]: (t, u, v, inst), (prim, tri, -, -); POINTS: float4[count] = (p, -)
    const float4 *rays;     // evaluate: lrhip_ray[count], the rays whose hits these are; sample: not read
    const float4 *dirs;     // sample: [count] (u_light_selection, u_surface_x, u_surface_y, -); evaluate: not read
    float4 *out_rays;       // sample: lrhip_ray[count], the shadow rays, two float4 each; evaluate: not written
    float4 *out;            // lrhip_light_result[count], two float4 each
    const lr_mesh *meshes;  // [mesh_count]: bounds `prim` of a record that names an instance
    uint32_t count;
    uint32_t triangle_count;// BVH triangles = shading records
    uint32_t instance_count;
    uint32_t mesh_count;
};

enum : uint32_t { kLightSample = 0u, kLightEvaluate = 1u };                  // lrhip.h: LRHIP_LIGHT_SAMPLE / LRHIP_LIGHT_EVALUATE
enum : uint32_t { kLightKindArea = 0u, kLightKindEnvironment = 1u, kLightKindNone = 2u };// lrhip.h: LRHIP_LIGHT_KIND_*

template<uint32_t MODE, bool POINTS>
__global__ __launch_bounds__(kBlockThreads) void light_kernel(DScenePtr scene_ptr, LightArgs args) {
    static_assert(MODE == kLightSample || !POINTS, "bare points are sampled from, never evaluated");
    const DScene &scene = *(const DScene *)scene_ptr;
    const auto stride = gridDim.x * kBlockThreads;
    const auto lit = scene.has_lights != 0u || scene.env_kind != kEnvNone;
    const BsdfArgs hit_args{args.hits, MODE == kLightEvaluate ? args.rays : nullptr, nullptr, nullptr, args.meshes,
                            args.count, args.triangle_count, args.instance_count, args.mesh_count};
    const auto zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (auto k = blockIdx.x * kBlockThreads + threadIdx.x; k < args.count; k += stride) {
        const auto record = args.out + static_cast<size_t>(k) * 2u;
        const auto shadow = MODE == kLightSample ? args.out_rays + static_cast<size_t>(k) * 2u : nullptr;
        if (!lit) {// nothing to sample, nothing to find: a valid answer
            if (MODE == kLightSample) { shadow[0] = zero, shadow[1] = zero; }
            record[0] = zero, record[1] = make_float4(__uint_as_float(kLightKindNone), 0.f, 0.f, 0.f);
            continue;
        }
        SurfacePoint it{};
        f3 wo = mk3(0.f);// (bsdf_resolve_hit's; the light code reads it.back_facing, set from it)
        if (MODE == kLightSample) {
            const auto q = args.dirs[k];
            auto valid = raycast_finite(q.x) && raycast_finite(q.y) && raycast_finite(q.z);
            if (POINTS) {// Interaction{p} of a medium point: sample_one_light<ENV, NULL_SHAPE = true> reads p alone
                const auto p = args.hits[k];
                valid = valid && raycast_finite(p.x) && raycast_finite(p.y) && raycast_finite(p.z);
                it.p = mk3(p.x, p.y, p.z);
            } else {
                valid = valid && bsdf_resolve_hit(scene, hit_args, k, it, wo);
            }
            if (!valid) {// the invalid record: zeros, kind LR_INVALID_ID
                shadow[0] = zero, shadow[1] = zero;
                record[0] = zero, record[1] = make_float4(__uint_as_float(kInvalid), 0.f, 0.f, 0.f);
                continue;
            }
            // ---- sample one light, as the shading block does (megapath_kernel.h; uniform.cpp:78-137 + light_sampler.cpp:57-63)
            auto pick = sample_one_light<true, POINTS>(scene, it, q.x, f2{q.y, q.z});
            if (pick.pdf == 0.f) { pick.L = mk3(0.f); }// a failed sample carries no radiance
            const auto kind = pick.shadow.t_max == kFloatMax ? kLightKindEnvironment : kLightKindArea;// read off the pick
            shadow[0] = make_float4(pick.shadow.o.x, pick.shadow.o.y, pick.shadow.o.z, pick.shadow.t_min);
            shadow[1] = make_float4(pick.shadow.d.x, pick.shadow.d.y, pick.shadow.d.z, pick.shadow.t_max);
            record[0] = make_float4(pick.L.x, pick.L.y, pick.L.z, pick.pdf);
            record[1] = make_float4(__uint_as_float(kind), 0.f, 0.f, 0.f);
        } else {
            const auto hp = args.hits + static_cast<size_t>(k) * 2u;
            const auto rp = args.rays + static_cast<size_t>(k) * 2u;
            const auto h0 = hp[0], h1 = hp[1], a = rp[0], b = rp[1];
            const auto inst = __float_as_uint(h0.w), tri = __float_as_uint(h1.y);
            f3 L = mk3(0.f);
            auto pdf = 0.f;
            uint32_t kind = kLightKindNone;
            auto valid = true;
            if (inst == kInvalid && tri == kInvalid) {// what lrhip_trace_rays writes for a miss
                valid = raycast_finite(h0.y) && raycast_finite(h0.z) && raycast_ray_valid(a, b);
                if (valid && scene.env_kind != kEnvNone) {// mega_path.cpp:70-76 -> evaluate_miss, uniform.cpp:67-76
                    L = mk3(scene.env_L[0], scene.env_L[1], scene.env_L[2]);
                    pdf = kInvPi * 0.25f;
                    if (scene.env_kind != kEnvConstant) { env_evaluate(scene, surface_unit_direction(mk3(b.x, b.y, b.z)), L, pdf); }
                    pdf *= scene.env_prob;
                    kind = kLightKindEnvironment;
                }
            } else {
                valid = bsdf_resolve_hit(scene, hit_args, k, it, wo);
                if (valid && scene.has_lights && (it.flags & LR_SHAPE_HAS_LIGHT)) {// hit light, mega_path.cpp:79-86
                    // the primitive within its mesh: the baked record's own on the renderer's path (as surface_kernel reads it), else the caller's
                    const auto prim = tri < args.triangle_count ? reinterpret_cast<const uint32_t *>(scene.shade_tris + tri)[29] : __float_as_uint(h1.x);
                    light_evaluate(scene, it, prim, mk3(a.x, a.y, a.z), L, pdf);
                    pdf *= (1.f - scene.env_prob) / static_cast<float>(scene.light_count);
                    kind = kLightKindArea;
                }
            }
            if (!valid) { kind = kInvalid; }
            record[0] = make_float4(L.x, L.y, L.z, pdf);
            record[1] = make_float4(__uint_as_float(kind), 0.f, 0.f, 0.f);
        }
    }
}

}// namespace lrd
