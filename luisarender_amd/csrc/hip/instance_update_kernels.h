// instance_update_kernels.h — moving instances on the device (lrhip.h: lrhip_set_instance_transforms): the kernels that rewrite
// the four tables lrhip_update_scene rewrites for moved geometry -- instance records, baked triangles with their shading records, and the
// refitted, re-quantised BVH packets -- from the caller's matrices and tables that are already in HBM.
//
// THE YARDSTICK IS THE HOST CODE, BIT FOR BIT: build_instances / normal_matrix / build_shade_tris / quantise_node (lrhip_tables.hip) and
// refit_accel (csrc/host/accel.cpp) are plain fp32 in a written order, compiled without FMA; their only fused operations are the explicit
// fmaf calls of quantise_node.  Everything here is written in the same order, with the same comparison forms ((b < a) ? b : a, so that a
// signed zero and a NaN come out alike), and the translation unit that holds these kernels is built with -ffp-contract=off and correctly
// rounded fp32 division (Makefile: lrhip_instance_update_FLAGS).  Change an expression here only together with its host twin.
#pragma once
#include "dev_scene.h"
#include "dev_trace.h"// kLeafFlag

namespace lrd {

constexpr uint32_t kUpdateBlock = 256u;

struct InstanceUpdateArgs {
    // the caller's arrays (device memory)
    const float4 *matrices;  // [count][4]: object_to_world, column-major
    const uint32_t *ids;     // [count] or nullptr (ids 0 .. count-1)
    uint32_t count;
    // the scene's tables, written in place
    DInstance *instances;    uint32_t instance_count;
    lr_bvh_triangle *bvh_tris; uint32_t triangle_count;// (the sentinel behind the last triangle is never touched)
    DShadeTri *shade_tris;
    DNodeQ *nodes;           uint32_t node_count;
    lr_bvh4_node *nodes32;   // the fp32 boxes the packets are quantised from (refit in place)
    const lr_vertex *vertices;   uint32_t vertex_count;
    const lr_triangle *triangles; uint32_t mesh_triangle_count;
    // scratch of the call (cleared by the host before the first kernel)
    uint32_t *owner;         // [instance_count]: 1 + the last list entry that names the instance
    uint32_t *moved;         // bit per instance
};

// std::min(a, b) / std::max(a, b) as the host's Box::grow and quantise_node use them
__device__ __forceinline__ float host_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float host_max(float a, float b) { return (a < b) ? b : a; }

// ---- stage 1a: of the list entries that name one instance the LAST one owns it (device-pointer calls may hold duplicates; a host-pointer call
// was checked).  An id out of range is skipped here and in 1b.
__global__ void __launch_bounds__(kUpdateBlock) instance_claim_kernel(InstanceUpdateArgs a) {
    const auto i = blockIdx.x * kUpdateBlock + threadIdx.x;
    if (i >= a.count) { return; }
    const auto id = a.ids != nullptr ? a.ids[i] : i;
    if (id >= a.instance_count) { return; }
    atomicMax(a.owner + id, i + 1u);
}

// ---- stage 1b: one thread per listed instance: DInstance's columns and transpose(inverse(M3)) in normal_matrix's operation order
__global__ void __launch_bounds__(kUpdateBlock) instance_record_kernel(InstanceUpdateArgs a) {
    const auto i = blockIdx.x * kUpdateBlock + threadIdx.x;
    if (i >= a.count) { return; }
    const auto id = a.ids != nullptr ? a.ids[i] : i;
    if (id >= a.instance_count || a.owner[id] != i + 1u) { return; }
    const float4 col[4] = {a.matrices[i * 4u], a.matrices[i * 4u + 1u], a.matrices[i * 4u + 2u], a.matrices[i * 4u + 3u]};
    float m[3][3];// m[c][r]
    for (auto c = 0; c < 3; c++) { m[c][0] = col[c].x, m[c][1] = col[c].y, m[c][2] = col[c].z; }
    const auto one_over_det = 1.0f / (m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) -
                                      m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2]) +
                                      m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]));
    float inv[3][3];// inv[c][r]
    inv[0][0] = (m[1][1] * m[2][2] - m[2][1] * m[1][2]) * one_over_det;
    inv[0][1] = (m[2][1] * m[0][2] - m[0][1] * m[2][2]) * one_over_det;
    inv[0][2] = (m[0][1] * m[1][2] - m[1][1] * m[0][2]) * one_over_det;
    inv[1][0] = (m[2][0] * m[1][2] - m[1][0] * m[2][2]) * one_over_det;
    inv[1][1] = (m[0][0] * m[2][2] - m[2][0] * m[0][2]) * one_over_det;
    inv[1][2] = (m[1][0] * m[0][2] - m[0][0] * m[1][2]) * one_over_det;
    inv[2][0] = (m[1][0] * m[2][1] - m[2][0] * m[1][1]) * one_over_det;
    inv[2][1] = (m[2][0] * m[0][1] - m[0][0] * m[2][1]) * one_over_det;
    inv[2][2] = (m[0][0] * m[1][1] - m[1][0] * m[0][1]) * one_over_det;
    auto &d = a.instances[id];// handle, vertex_offset, triangle_offset stay; the pads stay zero
    for (auto r = 0; r < 3; r++) {
        d.c0[r] = m[0][r], d.c1[r] = m[1][r], d.c2[r] = m[2][r];
        d.n0[r] = inv[r][0], d.n1[r] = inv[r][1], d.n2[r] = inv[r][2];// column c of the result = row c of inv
    }
    d.t[0] = col[3].x, d.t[1] = col[3].y, d.t[2] = col[3].z;
    atomicOr(a.moved + (id >> 5u), 1u << (id & 31u));
}

// ---- stage 2: one thread per baked BVH triangle of a moved instance: the 48-byte record and the six quads of the shading record that hold
// positions and normals; the fourth word of each quad (instance, primitive, flags, tags, offset bits, uvs) is kept from what is there
__global__ void __launch_bounds__(kUpdateBlock) instance_triangle_kernel(InstanceUpdateArgs a) {
    const auto t = blockIdx.x * kUpdateBlock + threadIdx.x;
    if (t >= a.triangle_count) { return; }
    auto bt = reinterpret_cast<float4 *>(a.bvh_tris + t);
    auto q0 = bt[0];
    const auto inst = __float_as_uint(q0.w);
    if (inst >= a.instance_count || ((a.moved[inst >> 5u] >> (inst & 31u)) & 1u) == 0u) { return; }
    auto q1 = bt[1], q2 = bt[2];
    const auto prim = __float_as_uint(q1.w);
    const auto di = reinterpret_cast<const float4 *>(a.instances + inst);
    const auto c0 = di[1], c1 = di[2], c2 = di[3], c3 = di[4], n0 = di[5], n1 = di[6], n2 = di[7];
    const auto vertex_offset = __float_as_uint(c0.w), triangle_offset = __float_as_uint(c1.w);
    const auto ti = static_cast<uint64_t>(triangle_offset) + prim;
    if (ti >= a.mesh_triangle_count) { return; }
    const auto tri = a.triangles[ti];
    const uint32_t index[3] = {tri.i0, tri.i1, tri.i2};
    float p[3][3], n[3][3];
    for (auto k = 0; k < 3; k++) {
        const auto vi = static_cast<uint64_t>(vertex_offset) + index[k];
        if (vi >= a.vertex_count) { return; }
        const auto v = reinterpret_cast<const float4 *>(a.vertices + vi);
        const auto va = v[0], vb = v[1];// (px py pz nx) (ny nz u v)
        // lr_math.h: operator*(float4x4, float4) with w = 1: ((c0 x + c1 y) + c2 z) + c3
        p[k][0] = ((c0.x * va.x + c1.x * va.y) + c2.x * va.z) + c3.x;
        p[k][1] = ((c0.y * va.x + c1.y * va.y) + c2.y * va.z) + c3.y;
        p[k][2] = ((c0.z * va.x + c1.z * va.y) + c2.z * va.z) + c3.z;
        // build_shade_tris: n[c] = (n0[c] nx + n1[c] ny) + n2[c] nz
        n[k][0] = (n0.x * va.w + n1.x * vb.x) + n2.x * vb.y;
        n[k][1] = (n0.y * va.w + n1.y * vb.x) + n2.y * vb.y;
        n[k][2] = (n0.z * va.w + n1.z * vb.x) + n2.z * vb.y;
    }
    q0.x = p[0][0], q0.y = p[0][1], q0.z = p[0][2];
    q1.x = p[1][0] - p[0][0], q1.y = p[1][1] - p[0][1], q1.z = p[1][2] - p[0][2];
    q2.x = p[2][0] - p[0][0], q2.y = p[2][1] - p[0][1], q2.z = p[2][2] - p[0][2];
    bt[0] = q0, bt[1] = q1, bt[2] = q2;
    auto st = reinterpret_cast<float4 *>(a.shade_tris + t);
    st[0] = make_float4(q0.x, q0.y, q0.z, st[0].w);
    st[1] = make_float4(q1.x, q1.y, q1.z, st[1].w);
    st[2] = make_float4(q2.x, q2.y, q2.z, st[2].w);
    st[3] = make_float4(n[0][0], n[0][1], n[0][2], st[3].w);
    st[4] = make_float4(n[1][0], n[1][1], n[1][2], st[4].w);
    st[5] = make_float4(n[2][0], n[2][1], n[2][2], st[5].w);
}

// ---- stage 3: refit and quantise the nodes of ONE level of the tree (the host launches the levels from the deepest up: a node's inner children
// are one level down and done).  One quad of lanes per node, lane c for child c: the child's fp32 box as refit_accel forms it, then the packet
// by quantise_node's rule, each lane storing its 16 bytes of the 64.
__global__ void __launch_bounds__(kUpdateBlock) instance_refit_kernel(InstanceUpdateArgs a, const uint32_t *level_nodes, uint32_t level_count) {
    const auto thread = blockIdx.x * kUpdateBlock + threadIdx.x;
    const auto quad = thread >> 2u;
    const auto lane = thread & 3u;
    if (quad >= level_count) { return; }// (whole quads leave together: kUpdateBlock is a multiple of 4)
    const auto ni = level_nodes[quad];
    if (ni >= a.node_count) { return; }
    auto &node = a.nodes32[ni];
    const auto children = *reinterpret_cast<const uint4 *>(node.child);
    const uint32_t child[4] = {children.x, children.y, children.z, children.w};
    const auto c = child[lane];
    const auto valid = c != LR_INVALID_ID;
    constexpr auto kMax = 3.402823466e+38f;
    float lo[3] = {kMax, kMax, kMax}, hi[3] = {-kMax, -kMax, -kMax};
    auto refitted = false;
    if (valid) {
        if ((c & 0x80000000u) != 0u) {
            const auto ti = c & ((1u << 27u) - 1u);
            if (ti < a.triangle_count) {
                const auto bt = reinterpret_cast<const float4 *>(a.bvh_tris + ti);
                const auto v0 = bt[0], e1 = bt[1], e2 = bt[2];
                const float pa[3] = {v0.x, v0.y, v0.z};
                const float pb[3] = {v0.x + e1.x, v0.y + e1.y, v0.z + e1.z};// (p0 + e1, not the p1 it was formed from: as refit_accel does)
                const float pc[3] = {v0.x + e2.x, v0.y + e2.y, v0.z + e2.z};
                for (auto k = 0; k < 3; k++) {
                    lo[k] = host_min(lo[k], pa[k]), hi[k] = host_max(hi[k], pa[k]);
                    lo[k] = host_min(lo[k], pb[k]), hi[k] = host_max(hi[k], pb[k]);
                    lo[k] = host_min(lo[k], pc[k]), hi[k] = host_max(hi[k], pc[k]);
                }
                refitted = true;
            }
        } else if (c < a.node_count) {
            const auto &ch = a.nodes32[c];
            const auto rows = reinterpret_cast<const float4 *>(&ch);// lo_x lo_y lo_z hi_x hi_y hi_z child
            const float4 r[6] = {rows[0], rows[1], rows[2], rows[3], rows[4], rows[5]};
            const auto cc = *reinterpret_cast<const uint4 *>(ch.child);
            const uint32_t grand[4] = {cc.x, cc.y, cc.z, cc.w};
            const float *f[6] = {&r[0].x, &r[1].x, &r[2].x, &r[3].x, &r[4].x, &r[5].x};
            for (auto k = 0; k < 4; k++) {
                if (grand[k] == LR_INVALID_ID) { continue; }
                for (auto ax = 0; ax < 3; ax++) {// Box::grow(lo point), Box::grow(hi point)
                    lo[ax] = host_min(lo[ax], f[ax][k]), hi[ax] = host_max(hi[ax], f[ax][k]);
                    lo[ax] = host_min(lo[ax], f[3 + ax][k]), hi[ax] = host_max(hi[ax], f[3 + ax][k]);
                }
            }
            refitted = true;
        }
        if (refitted) {
            node.lo_x[lane] = lo[0], node.lo_y[lane] = lo[1], node.lo_z[lane] = lo[2];
            node.hi_x[lane] = hi[0], node.hi_y[lane] = hi[1], node.hi_z[lane] = hi[2];
        } else {// (a reference outside the tables: the box stays what the upload holds)
            lo[0] = node.lo_x[lane], lo[1] = node.lo_y[lane], lo[2] = node.lo_z[lane];
            hi[0] = node.hi_x[lane], hi[1] = node.hi_y[lane], hi[2] = node.hi_z[lane];
        }
    }
    // quantise_node: per axis the origin and scale over the valid children, in slot order
    float origin[3], scale[3];
    uint32_t plo[3], phi[3];
    for (auto ax = 0; ax < 3; ax++) {
        auto mn = kMax, mx = -kMax;
        for (auto k = 0; k < 4; k++) {
            const auto l = __shfl(lo[ax], k, 4), h = __shfl(hi[ax], k, 4);
            if (child[k] == LR_INVALID_ID) { continue; }
            mn = host_min(mn, l), mx = host_max(mx, h);
        }
        if (mn > mx) { mn = mx = 0.f; }
        origin[ax] = mn;
        auto sc = (mx - mn) / 255.f;
        // (the host's loop has no bound; a scale next to FLT_MAX or a box of infinities is not a scene, but nothing here may hang)
        for (auto guard = 0; guard < 64 && sc > 0.f && sc < kMax && fmaf(255.f, sc, mn) < mx; guard++) {
            sc = __uint_as_float(__float_as_uint(sc) + 1u);// nextafter(sc, FLT_MAX) of a positive finite sc
        }
        scale[ax] = sc;
        uint32_t ql = 255u, qh = 0u;// empty slot: inverted
        if (valid) {
            if (sc > 0.f) {
                const auto fl = floor((static_cast<double>(lo[ax]) - mn) / sc), fh = ceil((static_cast<double>(hi[ax]) - mn) / sc);
                const auto cl = (fl < 0.0) ? 0.0 : (255.0 < fl) ? 255.0 : fl, chh = (fh < 0.0) ? 0.0 : (255.0 < fh) ? 255.0 : fh;
                ql = (cl == cl) ? static_cast<uint32_t>(cl) : 0u, qh = (chh == chh) ? static_cast<uint32_t>(chh) : 0u;
                while (ql > 0u && fmaf(static_cast<float>(ql), sc, mn) > lo[ax]) { ql--; }
                while (qh < 255u && fmaf(static_cast<float>(qh), sc, mn) < hi[ax]) { qh++; }
            } else {
                ql = qh = 0u;
            }
        }
        auto wl = ql << (8u * lane), wh = qh << (8u * lane);
        wl |= __shfl_xor(wl, 1, 4), wh |= __shfl_xor(wh, 1, 4);
        wl |= __shfl_xor(wl, 2, 4), wh |= __shfl_xor(wh, 2, 4);
        plo[ax] = wl, phi[ax] = wh;
    }
    const auto empty_ref = kLeafFlag | a.triangle_count;// the sentinel of build_padded_triangles
    uint4 word;
    if (lane == 0u) {
        word = make_uint4(__float_as_uint(origin[0]), __float_as_uint(origin[1]), __float_as_uint(origin[2]), __float_as_uint(scale[0]));
    } else if (lane == 1u) {
        word = make_uint4(plo[0], plo[1], plo[2], phi[0]);
    } else if (lane == 2u) {
        word = make_uint4(phi[1], phi[2], __float_as_uint(scale[1]), __float_as_uint(scale[2]));
    } else {
        word = make_uint4(child[0] == LR_INVALID_ID ? empty_ref : child[0], child[1] == LR_INVALID_ID ? empty_ref : child[1],
                          child[2] == LR_INVALID_ID ? empty_ref : child[2], child[3] == LR_INVALID_ID ? empty_ref : child[3]);
    }
    reinterpret_cast<uint4 *>(a.nodes + ni)[lane] = word;
}

}// namespace lrd
