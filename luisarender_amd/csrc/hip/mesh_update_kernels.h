// mesh_update_kernels.h — deforming a mesh on the device (lrhip.h: lrhip_set_mesh_vertices): the kernels in front of the re-bake
// and refit of instance_update_kernels.h.  They write the caller's positions (and normals) into the object-space vertex table, recompute
// a mesh's vertex normals, and mark the instances of the mesh in the `moved` mask that instance_triangle_kernel reads.
//
// THE YARDSTICK IS THE HOST CODE, BIT FOR BIT: set_scene_mesh_vertices (csrc/host/scene.cpp) is plain fp32 in a written order, compiled
// without FMA.  mesh_normal_kernel restates its normal recompute in the same order, and the translation unit that holds these kernels is
// built with -ffp-contract=off and correctly rounded fp32 division and square root (Makefile: lrhip_mesh_update_FLAGS).  Change an expression
// here only together with its host twin.
#pragma once
#include "dev_scene.h"

namespace lrd {

constexpr uint32_t kMeshUpdateBlock = 256u;

struct MeshUpdateArgs {
    // the caller's arrays (device memory), packed float[count][3]
    const float *positions;
    const float *normals;    // or nullptr: the normals stay
    uint32_t count;
    uint32_t first;          // index into the vertex table of the first vertex written (the mesh's vertex_offset + first_vertex)
    // the scene's object-space tables; the vertices are written in place
    lr_vertex *vertices;          uint32_t vertex_count;
    const lr_triangle *triangles; uint32_t triangle_count;
    // the mesh (lr_mesh) and its corner lists: the triangles that name vertex v, once per naming corner, in ascending order, are
    // corners[offsets[v] .. offsets[v + 1])
    uint32_t mesh, mesh_vertex_offset, mesh_vertex_count, mesh_triangle_offset, mesh_triangle_count;
    const uint32_t *offsets; // [mesh_vertex_count + 1]
    const uint32_t *corners; // [3 mesh_triangle_count]
    const DInstance *instances;   uint32_t instance_count;
    uint32_t *moved;         // bit per instance (the scratch of instance_update_kernels.h, cleared by the host before the first kernel)
};

// ---- one thread per supplied vertex: consecutive lanes read consecutive 12-byte records; three or six floats of the 32-byte vertex are
// stored, u and v stay
__global__ void __launch_bounds__(kMeshUpdateBlock) mesh_vertex_kernel(MeshUpdateArgs a) {
    const auto i = blockIdx.x * kMeshUpdateBlock + threadIdx.x;
    if (i >= a.count) { return; }
    const auto vi = static_cast<uint64_t>(a.first) + i;
    if (vi >= a.vertex_count) { return; }
    const auto p = a.positions + static_cast<size_t>(i) * 3u;
    auto &v = a.vertices[vi];
    v.px = p[0], v.py = p[1], v.pz = p[2];
    if (a.normals != nullptr) {
        const auto n = a.normals + static_cast<size_t>(i) * 3u;
        v.nx = n[0], v.ny = n[1], v.nz = n[2];
    }
}

// ---- one thread per vertex of the mesh: the area-weighted normal, summed over the vertex's corner list in the list's order.  Positions are
// read and normals written field by field: other threads read px py pz of this vertex while this one stores nx ny nz
__global__ void __launch_bounds__(kMeshUpdateBlock) mesh_normal_kernel(MeshUpdateArgs a) {
    const auto v = blockIdx.x * kMeshUpdateBlock + threadIdx.x;
    if (v >= a.mesh_vertex_count) { return; }
    const auto self = static_cast<uint64_t>(a.mesh_vertex_offset) + v;
    if (self >= a.vertex_count) { return; }
    const auto corner_count = static_cast<uint64_t>(a.mesh_triangle_count) * 3u;
    const auto begin = a.offsets[v], end = a.offsets[v + 1u];
    float s[3] = {0.f, 0.f, 0.f};
    for (auto e = begin; e < end && e < corner_count; e++) {
        const auto t = a.corners[e];
        const auto ti = static_cast<uint64_t>(a.mesh_triangle_offset) + t;
        if (t >= a.mesh_triangle_count || ti >= a.triangle_count) { continue; }
        const auto tri = a.triangles[ti];
        const uint32_t index[3] = {tri.i0, tri.i1, tri.i2};
        float p[3][3];
        auto inside = true;
        for (auto k = 0; k < 3; k++) {
            const auto vi = static_cast<uint64_t>(a.mesh_vertex_offset) + index[k];
            inside = inside && index[k] < a.mesh_vertex_count && vi < a.vertex_count;
            if (!inside) { break; }
            const auto &q = a.vertices[vi];
            p[k][0] = q.px, p[k][1] = q.py, p[k][2] = q.pz;
        }
        if (!inside) { continue; }
        const float ea[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const float eb[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const float c[3] = {ea[1] * eb[2] - ea[2] * eb[1], ea[2] * eb[0] - ea[0] * eb[2], ea[0] * eb[1] - ea[1] * eb[0]};
        s[0] = s[0] + c[0], s[1] = s[1] + c[1], s[2] = s[2] + c[2];
    }
    const auto l2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
    if (l2 > 0.f && l2 <= 3.402823466e+38f) {// (a sum of zero, an overflow or a NaN: the normal stays)
        const auto l = sqrtf(l2);
        auto &out = a.vertices[self];
        out.nx = s[0] / l, out.ny = s[1] / l, out.nz = s[2] / l;
    }
}

// ---- one thread per instance: the instances of the mesh are the ones instance_triangle_kernel re-bakes
__global__ void __launch_bounds__(kMeshUpdateBlock) mesh_mark_kernel(MeshUpdateArgs a) {
    const auto i = blockIdx.x * kMeshUpdateBlock + threadIdx.x;
    if (i >= a.instance_count) { return; }
    if ((a.instances[i].handle[0] >> 10u) == a.mesh) { atomicOr(a.moved + (i >> 5u), 1u << (i & 31u)); }
}

}// namespace lrd
