// gather_kernel.h — the plan of ONE irradiance sample at points the caller names (include/lrhip.h: lrhip_query_gather_vertex):
// the gather vertex of gather_vertex.h for sample index s of each record's stream, stored as 96 bytes per record -- the continuation ray, the
// shadow ray, (nee rgb, light_pdf), (beta rgb, pdf_bsdf) -- for a caller who continues the texel's path with an estimator of their own:
// sample = (shadow ray free ? nee : 0) + beta x (what the continuation ray finds, MIS-weighted by pdf_bsdf).
//
// One lane per record, no LDS, no queue, as light_kernel.h: the lane loads its record(s) as dwordx4, checks every index the record names
// BEFORE it is used (bsdf_resolve_hit, the BSDF queries' own), starts the record's stream and makes ONE call to gather_vertex.  This file
// holds no sampling or shading arithmetic of its own.  POINTS: the record is a bare position and a normal, two float4.
//
// The invalid record -- a non-finite u, v, point or normal, a zero normal, ids out of range, a miss, an instance without geometry -- gives
// zero rays, zeros and pdf = 0.  A scene with neither lights nor an environment (wave-uniform, tested first) gives it for every record.
#pragma once
#include "bsdf_kernel.h"
#include "gather_vertex.h"

namespace lrd {

struct GatherArgs {
    const float4 *hits;     // lrhip_ray_hit[count]: (t, u, v, inst), (prim, tri, -, -); POINTS: float4[count] = (p, -)
    const float4 *rays;     // not read (fill_hit_table's field): every record is seen from its front
    const float4 *normals;  // POINTS: float4[count] = (n, -), any length but 0
    const uint32_t *streams;// stream id of each record, or nullptr: record k has stream stream_base + k
    float4 *out;            // [count][6]: ray (o, t_min), (d, t_max); shadow (o, t_min), (d, t_max); (nee, light_pdf); (beta, pdf_bsdf)
    const lr_mesh *meshes;  // [mesh_count]: bounds `prim` of a record that names an instance
    uint32_t count;
    uint32_t triangle_count;// BVH triangles = shading records
    uint32_t instance_count;
    uint32_t mesh_count;
    uint32_t stream_base;   // (a host-pointer call goes through the staging buffers chunk by chunk: the chunk's first record)
    uint32_t sample_index;
};

constexpr uint32_t kGatherVertexFloat4s = 6u;// lrhip.h: lrhip_gather_vertex

// GENERIC = false: the Independent sampler; true: PCG32 / Sobol / PaddedSobol at run time -- the split the renderers make
template<bool POINTS, bool GENERIC>
__global__ __launch_bounds__(kBlockThreads) void gather_vertex_kernel(DScenePtr scene_ptr, GatherArgs args) {
    const DScene &scene = *(const DScene *)scene_ptr;
    const auto stride = gridDim.x * kBlockThreads;
    const auto lit = scene.has_lights != 0u || scene.env_kind != kEnvNone;
    const BsdfArgs hit_args{args.hits, nullptr, nullptr, nullptr, args.meshes, args.count, args.triangle_count, args.instance_count, args.mesh_count};
    const auto zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (auto k = blockIdx.x * kBlockThreads + threadIdx.x; k < args.count; k += stride) {
        const auto record = args.out + static_cast<size_t>(k) * kGatherVertexFloat4s;
        SurfacePoint it{};
        auto valid = lit;
        if (valid) {
            if (POINTS) {
                const auto p = args.hits[k], n = args.normals[k];
                valid = raycast_finite(p.x) && raycast_finite(p.y) && raycast_finite(p.z) && raycast_finite(n.x) && raycast_finite(n.y) && raycast_finite(n.z) &&
                        ((__float_as_uint(n.x) | __float_as_uint(n.y) | __float_as_uint(n.z)) & 0x7fffffffu) != 0u;
                if (valid) {
                    it.p = mk3(p.x, p.y, p.z);
                    it.ng = surface_unit_direction(mk3(n.x, n.y, n.z));
                    it.shading = frame_from_normal(it.ng);
                }
            } else {
                f3 wo;
                valid = bsdf_resolve_hit(scene, hit_args, k, it, wo);
            }
        }
        if (!valid) {
#pragma unroll
            for (auto i = 0u; i < kGatherVertexFloat4s; i++) { record[i] = zero; }
            continue;
        }
        PathSampler<GENERIC> sampler{};
        gather_start_stream(scene, sampler, args.streams != nullptr ? args.streams[k] : args.stream_base + k, args.sample_index);
        const auto g = gather_vertex<POINTS>(scene, it, sampler);// (light_pdf = 0 marks a failed light sample, whose ray may be non-finite)
        record[0] = make_float4(g.ray.o.x, g.ray.o.y, g.ray.o.z, g.ray.t_min);
        record[1] = make_float4(g.ray.d.x, g.ray.d.y, g.ray.d.z, g.ray.t_max);
        record[2] = make_float4(g.shadow.o.x, g.shadow.o.y, g.shadow.o.z, g.shadow.t_min);
        record[3] = make_float4(g.shadow.d.x, g.shadow.d.y, g.shadow.d.z, g.shadow.t_max);
        record[4] = make_float4(g.nee.x, g.nee.y, g.nee.z, g.light_pdf);
        record[5] = make_float4(g.beta.x, g.beta.y, g.beta.z, g.pdf_bsdf);
    }
}

}// namespace lrd
