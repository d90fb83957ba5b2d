// lightmap_kernels.h — the UV rasteriser of lightmap baking (lrhip.h: lrhip_lightmap_texels): which point of one instance's mesh
// each texel of a W x H lightmap over the mesh's UV chart stands for, as the texel record (inst, prim, u, v) with tri = 0xffffffff that the
// surface, BSDF and light queries take.  Texel (i, j) has its centre at uv = ((i + 1/2) / W, (j + 1/2) / H), row 0 at v = 0; nothing wraps.
//
// Two passes.  lightmap_owner_kernel: one WAVE per mesh triangle (and per slice of its texels, blockIdx.y), the lanes stride over the texels
// of the triangle's UV bounding box, clamped to the map, and every candidate does an atomicMin on the texel's owner word
//     ((centre covered ? 0 : 1) << 31) | prim
// so that centre coverage beats touching and the lowest prim wins within each class: the result is a function of the chart alone, whatever
// the launch geometry and the order the waves run in.  lightmap_record_kernel: one lane per texel, the owner word -> the 32-byte record.
//
// THE YARDSTICK IS tests/gather_reference.py, a numpy rasteriser in float64.  Everything a decision hangs on -- texel centres, edge
// functions, the box / triangle overlap, the nearest point -- is float64 here too, in the same written order, and the translation unit is
// built without fp contraction and approximate division (Makefile: lrhip_lightmap_FLAGS): fp32 edge functions are off by 2^-17 of a UV unit
// for a triangle 1 / 100 of the chart long, more than a texel's centre may be from an edge before the two sides have to agree.  The inputs
// are the fp32 u v of the device vertex table, exact in float64.  Only u, v of the record are rounded to fp32, at the end.
//
// Every index is checked before it is used: a triangle that names a vertex outside its mesh, has a non-finite u v or no area in UV space
// owns nothing, and an owner word that names no triangle of the mesh gives the miss record.
#pragma once
#include "dev_scene.h"

namespace lrd {

constexpr uint32_t kLightmapBlock = 256u;                 // four waves
constexpr uint32_t kLightmapNoOwner = 0xffffffffu;        // the owner word nobody has written
constexpr uint32_t kLightmapTouched = 0x80000000u;        // owner word: the texel's square meets the triangle, its centre is outside
enum : uint32_t { kLightmapFlagCentre = 1u, kLightmapFlagTouched = 2u };// lrhip.h: LRHIP_LIGHTMAP_TEXEL_*, word 6 of the record

struct LightmapArgs {
    const lr_vertex *vertices;    // the scene's object-space vertex table; only u v are read
    const lr_triangle *triangles;
    uint32_t *owner;              // [width * height], kLightmapNoOwner before the owner pass
    float4 *out;                  // record pass: lrhip_ray_hit[count], two float4 each, texels [first, first + count)
    uint32_t instance;
    // the instance's mesh (lr_mesh); the host has checked that both ranges lie inside the tables
    uint32_t vertex_offset, vertex_count, triangle_offset, triangle_count;
    uint32_t width, height;       // width * height < 2^31
    uint32_t conservative;
    uint32_t slices;              // owner pass: gridDim.y, waves that share one triangle's texels
    uint32_t first, count;        // record pass
};

// a mesh triangle in UV space; `area` is twice its signed area
struct LightmapTriangle {
    double ax, ay, bx, by, cx, cy, area;
};

// (b - a) x (p - a): positive where p lies to the left of a -> b
LR_D double lightmap_edge(double ax, double ay, double bx, double by, double px, double py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

LR_D bool lightmap_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// triangle `prim` of the mesh; false: it owns nothing
LR_D bool lightmap_load(const LightmapArgs &a, uint32_t prim, LightmapTriangle &t) {
    if (prim >= a.triangle_count) { return false; }
    const auto tri = a.triangles[static_cast<size_t>(a.triangle_offset) + prim];
    if (tri.i0 >= a.vertex_count || tri.i1 >= a.vertex_count || tri.i2 >= a.vertex_count) { return false; }
    const auto v = a.vertices + a.vertex_offset;
    const auto au = v[tri.i0].u, av = v[tri.i0].v, bu = v[tri.i1].u, bv = v[tri.i1].v, cu = v[tri.i2].u, cv = v[tri.i2].v;
    if (!(lightmap_finite(au) && lightmap_finite(av) && lightmap_finite(bu) && lightmap_finite(bv) && lightmap_finite(cu) && lightmap_finite(cv))) { return false; }
    t.ax = au, t.ay = av, t.bx = bu, t.by = bv, t.cx = cu, t.cy = cv;
    t.area = lightmap_edge(t.ax, t.ay, t.bx, t.by, t.cx, t.cy);
    return t.area != 0.0;
}

// the three edge functions at p, signed so that the inside is >= 0 whichever way the chart is wound
LR_D bool lightmap_covers(const LightmapTriangle &t, double px, double py) {
    const auto s = t.area > 0.0 ? 1.0 : -1.0;
    return s * lightmap_edge(t.bx, t.by, t.cx, t.cy, px, py) >= 0.0 && s * lightmap_edge(t.cx, t.cy, t.ax, t.ay, px, py) >= 0.0 &&
           s * lightmap_edge(t.ax, t.ay, t.bx, t.by, px, py) >= 0.0;
}

// the closed box [x0, x1] x [y0, y1] meets the closed triangle: no axis of either separates them (the box's: the bounding boxes overlap;
// the triangle's: the box has a corner on the inner side of every edge)
LR_D bool lightmap_touches(const LightmapTriangle &t, double x0, double y0, double x1, double y1) {
    const auto lo_x = fmin(t.ax, fmin(t.bx, t.cx)), hi_x = fmax(t.ax, fmax(t.bx, t.cx));
    const auto lo_y = fmin(t.ay, fmin(t.by, t.cy)), hi_y = fmax(t.ay, fmax(t.by, t.cy));
    if (!(x0 <= hi_x && x1 >= lo_x && y0 <= hi_y && y1 >= lo_y)) { return false; }
    const auto s = t.area > 0.0 ? 1.0 : -1.0;
    auto inner = [&](double px, double py, double qx, double qy) {
        const auto e = fmax(fmax(lightmap_edge(px, py, qx, qy, x0, y0) * s, lightmap_edge(px, py, qx, qy, x1, y0) * s),
                            fmax(lightmap_edge(px, py, qx, qy, x0, y1) * s, lightmap_edge(px, py, qx, qy, x1, y1) * s));
        return e >= 0.0;
    };
    return inner(t.bx, t.by, t.cx, t.cy) && inner(t.cx, t.cy, t.ax, t.ay) && inner(t.ax, t.ay, t.bx, t.by);
}

// the parameter of the point of segment p -> q nearest to c, and its squared distance
LR_D double lightmap_nearest(double px, double py, double qx, double qy, double cx, double cy, double &d2) {
    const auto ex = qx - px, ey = qy - py;
    const auto l2 = ex * ex + ey * ey;
    auto s = l2 > 0.0 ? ((cx - px) * ex + (cy - py) * ey) / l2 : 0.0;
    s = fmin(fmax(s, 0.0), 1.0);
    const auto dx = cx - (px + s * ex), dy = cy - (py + s * ey);
    d2 = dx * dx + dy * dy;
    return s;
}

// ---- the owner pass
__global__ void __launch_bounds__(kLightmapBlock) lightmap_owner_kernel(LightmapArgs a) {
    const auto prim = blockIdx.x * (kLightmapBlock / 64u) + (threadIdx.x >> 6u);
    const auto lane = threadIdx.x & 63u;
    LightmapTriangle t;
    if (!lightmap_load(a, prim, t)) { return; }
    const auto w = static_cast<double>(a.width), h = static_cast<double>(a.height);
    // the texels around the bounding box, one more on every side than it reaches; clamped while still float64, so that any finite u v is safe
    const auto lo_x = fmin(t.ax, fmin(t.bx, t.cx)), hi_x = fmax(t.ax, fmax(t.bx, t.cx));
    const auto lo_y = fmin(t.ay, fmin(t.by, t.cy)), hi_y = fmax(t.ay, fmax(t.by, t.cy));
    const auto i_lo = static_cast<uint32_t>(fmin(fmax(floor(lo_x * w) - 1.0, 0.0), w));
    const auto j_lo = static_cast<uint32_t>(fmin(fmax(floor(lo_y * h) - 1.0, 0.0), h));
    const auto i_end = static_cast<uint32_t>(fmin(fmax(floor(hi_x * w) + 2.0, 0.0), w));// one past the last column
    const auto j_end = static_cast<uint32_t>(fmin(fmax(floor(hi_y * h) + 2.0, 0.0), h));
    if (i_lo >= i_end || j_lo >= j_end) { return; }
    const auto columns = i_end - i_lo;
    const auto n = columns * (j_end - j_lo);// <= width * height < 2^31
    for (auto k = blockIdx.y * 64u + lane; k < n; k += 64u * a.slices) {
        const auto row = k / columns;
        const auto i = i_lo + (k - row * columns), j = j_lo + row;
        const auto texel = j * a.width + i;
        if (lightmap_covers(t, (i + 0.5) / w, (j + 0.5) / h)) {
            atomicMin(a.owner + texel, prim);
        } else if (a.conservative != 0u && lightmap_touches(t, i / w, j / h, (i + 1.0) / w, (j + 1.0) / h)) {
            atomicMin(a.owner + texel, kLightmapTouched | prim);
        }
    }
}

// ---- the record pass: (0, u, v, inst), (prim, 0xffffffff, flags, 0), or the miss record
__global__ void __launch_bounds__(kLightmapBlock) lightmap_record_kernel(LightmapArgs a) {
    const auto k = blockIdx.x * kLightmapBlock + threadIdx.x;
    if (k >= a.count) { return; }
    const auto texel = a.first + k;
    const auto word = a.owner[texel];
    const auto prim = word & ~kLightmapTouched;
    const auto record = a.out + static_cast<size_t>(k) * 2u;
    LightmapTriangle t;
    if (word == kLightmapNoOwner || !lightmap_load(a, prim, t)) {
        record[0] = make_float4(0.f, 0.f, 0.f, __uint_as_float(LR_INVALID_ID));
        record[1] = make_float4(__uint_as_float(LR_INVALID_ID), __uint_as_float(LR_INVALID_ID), 0.f, 0.f);
        return;
    }
    const auto i = texel % a.width, j = texel / a.width;
    const auto cx = (i + 0.5) / static_cast<double>(a.width), cy = (j + 0.5) / static_cast<double>(a.height);
    double u, v;
    if ((word & kLightmapTouched) == 0u) {// the centre's barycentrics: p = (1 - u - v) a + u b + v c
        u = lightmap_edge(t.cx, t.cy, t.ax, t.ay, cx, cy) / t.area;
        v = lightmap_edge(t.ax, t.ay, t.bx, t.by, cx, cy) / t.area;
    } else {// the centre is outside: the nearest point lies on an edge; the first of equally near edges
        double d_ab, d_bc, d_ca;
        const auto s_ab = lightmap_nearest(t.ax, t.ay, t.bx, t.by, cx, cy, d_ab);
        const auto s_bc = lightmap_nearest(t.bx, t.by, t.cx, t.cy, cx, cy, d_bc);
        const auto s_ca = lightmap_nearest(t.cx, t.cy, t.ax, t.ay, cx, cy, d_ca);
        u = s_ab, v = 0.0;
        auto d = d_ab;
        if (d_bc < d) { u = 1.0 - s_bc, v = s_bc, d = d_bc; }
        if (d_ca < d) { u = 0.0, v = 1.0 - s_ca; }
    }
    // fp32, inside the triangle: u, v >= 0 and u + v <= 1
    auto uf = fmaxf(static_cast<float>(u), 0.f), vf = fmaxf(static_cast<float>(v), 0.f);
    uf = fminf(uf, 1.f);
    if (uf + vf > 1.f) { vf = 1.f - uf; }
    const auto flags = (word & kLightmapTouched) == 0u ? kLightmapFlagCentre : kLightmapFlagTouched;
    record[0] = make_float4(0.f, uf, vf, __uint_as_float(a.instance));
    record[1] = make_float4(__uint_as_float(prim), __uint_as_float(LR_INVALID_ID), __uint_as_float(flags), 0.f);
}

}// namespace lrd
