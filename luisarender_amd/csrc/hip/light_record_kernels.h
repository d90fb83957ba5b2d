// light_record_kernels.h — the light sample's records (dev_scene.h: DLightInstance, DLightTri), built on the device: at upload, after
// lrhip_update_scene, and for the instances a device update marked (lrhip_set_instance_transforms, lrhip_set_mesh_vertices) -- in stream
// order in front of the next render.
//
// THE YARDSTICK IS THE RENDER KERNELS' OWN CODE, BIT FOR BIT: a record's ng and area come out of dev_shade.h: triangle_constants, the function
// reconstruct<false> evaluates per sample where a kernel keeps the chain of gathers (LR_LIGHT_RECORDS 0, `make nolightrec`), from the same
// quads of the same tables; everything else in a record is a copy.  The unit that holds these kernels (lrhip_tables.hip) is built with the
// library's own flags like most kernels that read the records; the kernels built without contraction and with correctly rounded division
// and square root read a second table of triangle records, baked by a unit that is built as they are (kernel_forms.h: LR_LIGHT_TRIS).  The
// __global__ functions, one thread per record, stand in those two units: lrhip_tables.hip and lrhip_instance_update.hip.
#pragma once
#include "dev_shade.h"

namespace lrd {

constexpr uint32_t kLightRecordBlock = 256u;

struct LightRecordArgs {
    DLightInstance *records;   uint32_t record_count;  // [record_count]; the first quad (ids, bases) is the host's and is kept
    DLightTri *tris;           uint32_t tri_count;     // [tri_count]
    const uint32_t *tri_owner; // [tri_count]: the light instance of every triangle record
    const DInstance *instances; uint32_t instance_count;
    const lr_vertex *vertices;  uint32_t vertex_count;
    const lr_triangle *triangles; uint32_t mesh_triangle_count;
    const float *tri_pdf;
    const uint32_t *moved;     // bit per instance, or nullptr: every record
};

LR_D bool light_record_moved(const LightRecordArgs &a, uint32_t inst) {
    return a.moved == nullptr || ((a.moved[inst >> 5u] >> (inst & 31u)) & 1u) != 0u;
}

// light instance i: the handle words and the four columns of its instance's record
LR_D void light_instance_record(const LightRecordArgs &a, uint32_t i) {
    if (i >= a.record_count) { return; }
    auto rec = reinterpret_cast<float4 *>(a.records + i);
    const auto inst = reinterpret_cast<const uint4 *>(rec)[0].x;
    if (inst >= a.instance_count || !light_record_moved(a, inst)) { return; }
    const auto ip = reinterpret_cast<const float4 *>(a.instances + inst);
    const auto h = reinterpret_cast<const uint4 *>(ip)[0];
    reinterpret_cast<uint4 *>(rec)[1] = make_uint4(h.x & 1023u, h.y, h.w, 0u);
    const auto q0 = ip[1], q1 = ip[2], q2 = ip[3], q3 = ip[4];
    rec[2] = make_float4(q0.x, q0.y, q0.z, 0.f), rec[3] = make_float4(q1.x, q1.y, q1.z, 0.f);
    rec[4] = make_float4(q2.x, q2.y, q2.z, 0.f), rec[5] = make_float4(q3.x, q3.y, q3.z, 0.f);
}

// triangle record t, one (light instance, primitive): the loads of reconstruct<false>, triangle_constants, the record.  An index outside its
// table leaves the record as it is (all zero from the upload): nothing here reads or writes out of bounds.
LR_D void light_triangle_record(const LightRecordArgs &a, uint32_t t) {
    if (t >= a.tri_count) { return; }
    const auto owner = a.tri_owner[t];
    if (owner >= a.record_count) { return; }
    const auto h0 = reinterpret_cast<const uint4 *>(a.records + owner)[0];
    const auto inst = h0.x;
    if (inst >= a.instance_count || t < h0.w || !light_record_moved(a, inst)) { return; }
    const auto prim = t - h0.w;
    const auto ip = reinterpret_cast<const float4 *>(a.instances + inst);
    const auto q0 = ip[1], q1 = ip[2], q2 = ip[3];
    const auto vertex_offset = __float_as_uint(q0.w), tri_offset = __float_as_uint(q1.w);
    const auto ti = static_cast<uint64_t>(tri_offset) + prim;
    if (ti >= a.mesh_triangle_count) { return; }
    const auto tri = a.triangles[ti];
    if (static_cast<uint64_t>(vertex_offset) + tri.i0 >= a.vertex_count || static_cast<uint64_t>(vertex_offset) + tri.i1 >= a.vertex_count ||
        static_cast<uint64_t>(vertex_offset) + tri.i2 >= a.vertex_count) { return; }
    const auto vp = reinterpret_cast<const float4 *>(a.vertices + vertex_offset);
    const auto a0 = vp[tri.i0 * 2u], a1 = vp[tri.i0 * 2u + 1u];
    const auto b0 = vp[tri.i1 * 2u], b1 = vp[tri.i1 * 2u + 1u];
    const auto c0 = vp[tri.i2 * 2u], c1 = vp[tri.i2 * 2u + 1u];
    const auto k = triangle_constants(mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z), mk3(q2.x, q2.y, q2.z), a0, a1, b0, b1, c0, c1);
    auto out = reinterpret_cast<float4 *>(a.tris + t);
    out[0] = make_float4(k.p0.x, k.p0.y, k.p0.z, k.ng.x);
    out[1] = make_float4(k.p1.x, k.p1.y, k.p1.z, k.ng.y);
    out[2] = make_float4(k.p2.x, k.p2.y, k.p2.z, k.ng.z);
    out[3] = make_float4(k.uv0.x, k.uv0.y, k.uv1.x, k.uv1.y);
    out[4] = make_float4(k.uv2.x, k.uv2.y, k.area, a.tri_pdf[ti]);
}

}// namespace lrd
