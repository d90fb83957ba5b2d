// gather_vertex.h — the first vertex of a path that starts AT a surface point instead of along a camera ray (lrhip.h:
// lrhip_query_gather_vertex): the MegaPath shading block's vertex (megapath_kernel.h, mega_path.cpp:90-153) for a VIRTUAL WHITE
// LAMBERT SURFACE at the point -- a DClosure of kind Matte with Kd = 1, sigma = 0 on the record's shading frame, seen from its front
// (wo = ng, as every record without a ray is).  The throughput starts as (pi, pi, pi), so that the path's Li IS the irradiance sample:
// E = pi L_o of a white Lambert surface.  The point's own emission is not part of it: irradiance is what arrives.
//
// One device function, and it holds no shading arithmetic of its own: sample_one_light, closure_evaluate, closure_sample, robust_origin
// and balance are the shading block's, in the shading block's order, with its "1212" draws (light selection, light surface, lobe -- drawn
// and not used: Matte has one lobe -- direction).  The texel is the path's camera end: depth 0 for the continuation ray, no Russian
// roulette here, want_closest = alive && 0 < max_depth; with max_depth = 0 the light sample adds nothing either (nee = 0, no shadow ray).
//
// POINTS: `it` is a bare position with a normal the caller gave (ng = shading.n); both rays start at the point itself, as the light
// queries' bare points do (sample_one_light<ENV, NULL_SHAPE = true>).
//
// The caller has tested that the scene has a light or an environment: sample_one_light must not be called with nothing to pick.
#pragma once
#include "dev_shade.h"
#include "dev_wavefront.h"

namespace lrd {

// what a kFeatGather launch reads beside RenderArgs' query columns (megapath_kernel.h: RenderArgs::pool points to one, in device memory)
struct GatherTable {
    const float4 *normals;  // bare points: float4[count] = (n, -); nullptr: the records are lrhip_ray_hit
    const lr_mesh *meshes;  // [mesh_count]: bounds `prim` of a record that names an instance
    uint32_t triangle_count, instance_count, mesh_count, pad;
};

struct GatherVertex {
    Ray ray;         // the continuation ray: (robust_origin(it, wi), wi, 0, FLT_MAX)
    Ray shadow;      // the light sample's shadow ray
    f3 nee;          // what the light sample adds if the shadow ray is free
    f3 beta;         // the throughput behind the vertex: pi f / pdf
    float light_pdf; // of the light sample (x the selection probability); 0: it failed
    float pdf_bsdf;  // of the continuation direction: what MIS weighs an emitter or environment it finds with
    bool want_shadow, want_closest;
};

// the sampler stream of a record, as the kFeatQuery prologue starts it (megapath_kernel.h): stream j is pixel (j mod W, (j div W) mod H)'s,
// moved past what Li draws before its first vertex -- the pixel sample and, for a thin lens, the lens sample
template<typename Sampler>
LR_D void gather_start_stream(const DScene &scene, Sampler &sampler, uint32_t j, uint32_t s) {
    sampler.start(scene, j % scene.camera.width, (j / scene.camera.width) % scene.camera.height, s);
    (void)sampler.next_pixel_2d();
    if (scene.camera.kind == LR_CAMERA_THIN_LENS) { (void)sampler.next_2d(); }
}

template<bool POINTS, typename Sampler>
LR_D GatherVertex gather_vertex(const DScene &scene, const SurfacePoint &it, Sampler &sampler) {
    GatherVertex g;
    DClosure white{};
    white.kind = LR_SURFACE_MATTE;
    white.c0[0] = 1.f, white.c0[1] = 1.f, white.c0[2] = 1.f;
    const auto wo = it.ng;
    auto beta = mk3(kPi);
    // ---- sample one light
    const auto u_light_selection = sampler.next_1d();
    const auto u_light_surface = sampler.next_2d();
    const auto pick = sample_one_light<true, POINTS>(scene, it, u_light_selection, u_light_surface);
    g.shadow = pick.shadow, g.light_pdf = pick.pdf;
    g.nee = mk3(0.f), g.want_shadow = false;
    // (a scene whose paths have no segment, max_depth = 0, starts no ray at all, the shadow ray included: its render is black, and so is
    // its irradiance)
    if (pick.pdf > 0.0f && 0u < scene.max_depth) {
        const auto eval = closure_evaluate<false>(white, it.shading, it.ng, wo, pick.shadow.d);
        const auto w = balance(pick.pdf, eval.pdf) / pick.pdf;
        g.nee = w * beta * eval.f * pick.L;
        g.want_shadow = g.nee.x != 0.f || g.nee.y != 0.f || g.nee.z != 0.f;
    }
    // ---- the continuation
    const auto u_lobe = sampler.next_1d();
    const auto u_bsdf = sampler.next_2d();
    const auto bs = closure_sample<false>(white, it.shading, it.ng, wo, u_lobe, u_bsdf);
    // (POINTS: the point itself, as sample_one_light<ENV, NULL_SHAPE = true> starts both of its shadow rays -- `NULL_SHAPE ? it.p : robust_origin`,
    // dev_shade.h; it reads neither ng nor the offset bits there)
    g.ray.o = POINTS ? it.p : robust_origin(it, bs.wi);
    g.ray.d = bs.wi;
    g.ray.t_min = 0.f, g.ray.t_max = kFloatMax;
    g.pdf_bsdf = bs.pdf;
    beta *= (bs.pdf > 0.f ? 1.f / bs.pdf : 0.f) * bs.f;
    if (any_nan(beta)) { beta = mk3(0.f); }
    g.beta = beta;
    const auto alive = !(beta.x <= 0.f && beta.y <= 0.f && beta.z <= 0.f);
    g.want_closest = alive && 0u < scene.max_depth;
    return g;
}

}// namespace lrd
