// lrhip_tables.hip — what lrhip_upload_scene / lrhip_update_scene put on the device, built on the host: the check of every index a
// scene table holds into another, the 8-bit texel packing, and the tables that depend on the scene time; and the one pair of tables that is
// built ON THE DEVICE, the light sample's records (light_record_kernels.h), whose kernels stand here because this unit is built with the
// library's own flags.
#include "lrhip_internal.h"

#include <limits>

namespace lrd {
// one thread per record (light_record_kernels.h), with this unit's arithmetic: the library's own (DScene::light_tris)
__global__ void __launch_bounds__(kLightRecordBlock) light_instance_record_kernel(LightRecordArgs a) {
    light_instance_record(a, blockIdx.x * kLightRecordBlock + threadIdx.x);
}
__global__ void __launch_bounds__(kLightRecordBlock) light_triangle_record_kernel(LightRecordArgs a) {
    light_triangle_record(a, blockIdx.x * kLightRecordBlock + threadIdx.x);
}
}// namespace lrd

namespace lrh {

namespace {
// 3x3 inverse-transpose, same arithmetic as luisa::inverse(float3x3) + transpose (geometry.cpp:378)
void normal_matrix(const float *m, float out[9]) {
    float a[3][3];// a[c][r]
    for (auto c = 0; c < 3; c++) {
        for (auto r = 0; r < 3; r++) { a[c][r] = m[c * 4 + r]; }
    }
    auto one_over_det = 1.0f / (a[0][0] * (a[1][1] * a[2][2] - a[2][1] * a[1][2]) -
                                a[1][0] * (a[0][1] * a[2][2] - a[2][1] * a[0][2]) +
                                a[2][0] * (a[0][1] * a[1][2] - a[1][1] * a[0][2]));
    float inv[3][3];// inv[c][r]
    inv[0][0] = (a[1][1] * a[2][2] - a[2][1] * a[1][2]) * one_over_det;
    inv[0][1] = (a[2][1] * a[0][2] - a[0][1] * a[2][2]) * one_over_det;
    inv[0][2] = (a[0][1] * a[1][2] - a[1][1] * a[0][2]) * one_over_det;
    inv[1][0] = (a[2][0] * a[1][2] - a[1][0] * a[2][2]) * one_over_det;
    inv[1][1] = (a[0][0] * a[2][2] - a[2][0] * a[0][2]) * one_over_det;
    inv[1][2] = (a[1][0] * a[0][2] - a[0][0] * a[1][2]) * one_over_det;
    inv[2][0] = (a[1][0] * a[2][1] - a[2][0] * a[1][1]) * one_over_det;
    inv[2][1] = (a[2][0] * a[0][1] - a[0][0] * a[2][1]) * one_over_det;
    inv[2][2] = (a[0][0] * a[1][1] - a[1][0] * a[0][1]) * one_over_det;
    for (auto c = 0; c < 3; c++) {// transpose: column c of the result = row c of inv
        for (auto r = 0; r < 3; r++) { out[c * 3 + r] = inv[r][c]; }
    }
}

// fp32 child boxes -> 64-byte quantised packet; conservative: decoded lo <= lo, decoded hi >= hi in the
// same fp32 fma the kernel uses (dev_trace.h)
// An empty slot gets inverted planes (lo 255, hi 0) AND the reference of the sentinel leaf (`empty_ref`: a triangle nothing hits, behind
// the last baked triangle): the kernel tests no child word, an empty slot misses wherever the node has an extent and costs one
// wasted triangle test where it has none.
lrd::DNodeQ quantise_node(const lr_bvh4_node &n, uint32_t empty_ref) {
    lrd::DNodeQ q{};
    const float *lo[3] = {n.lo_x, n.lo_y, n.lo_z};
    const float *hi[3] = {n.hi_x, n.hi_y, n.hi_z};
    float origin[3], scale[3];
    uint32_t plo[3] = {0u, 0u, 0u}, phi[3] = {0u, 0u, 0u};
    for (auto a = 0; a < 3; a++) {
        auto mn = std::numeric_limits<float>::max(), mx = -std::numeric_limits<float>::max();
        for (auto c = 0; c < 4; c++) {
            if (n.child[c] == LR_INVALID_ID) { continue; }
            mn = std::min(mn, lo[a][c]), mx = std::max(mx, hi[a][c]);
        }
        if (mn > mx) { mn = mx = 0.f; }
        origin[a] = mn;
        auto sc = (mx - mn) / 255.f;
        while (sc > 0.f && std::fmaf(255.f, sc, mn) < mx) { sc = std::nextafter(sc, std::numeric_limits<float>::max()); }
        scale[a] = sc;
        for (auto c = 0; c < 4; c++) {
            uint32_t ql = 255u, qh = 0u;// empty slot: inverted
            if (n.child[c] != LR_INVALID_ID) {
                if (sc > 0.f) {
                    auto fl = std::floor((static_cast<double>(lo[a][c]) - mn) / sc), fh = std::ceil((static_cast<double>(hi[a][c]) - mn) / sc);
                    ql = static_cast<uint32_t>(std::clamp(fl, 0.0, 255.0)), qh = static_cast<uint32_t>(std::clamp(fh, 0.0, 255.0));
                    while (ql > 0u && std::fmaf(static_cast<float>(ql), sc, mn) > lo[a][c]) { ql--; }
                    while (qh < 255u && std::fmaf(static_cast<float>(qh), sc, mn) < hi[a][c]) { qh++; }
                } else {
                    ql = qh = 0u;
                }
            }
            plo[a] |= ql << (8u * static_cast<uint32_t>(c));
            phi[a] |= qh << (8u * static_cast<uint32_t>(c));
        }
    }
    q.origin[0] = origin[0], q.origin[1] = origin[1], q.origin[2] = origin[2];
    q.scale_x = scale[0], q.scale_y = scale[1], q.scale_z = scale[2];
    q.lo_x = plo[0], q.lo_y = plo[1], q.lo_z = plo[2];
    q.hi_x = phi[0], q.hi_y = phi[1], q.hi_z = phi[2];
    for (auto c = 0; c < 4; c++) { q.child[c] = n.child[c] == LR_INVALID_ID ? empty_ref : n.child[c]; }
    return q;
}

}// namespace

// depth of the tree; 0 if a leaf holds more than one triangle (the kernel's leaf step tests exactly one)
uint32_t bvh_depth(const lr_accel &accel) {
    std::vector<std::pair<uint32_t, uint32_t>> stack{{0u, 1u}};
    auto depth = 0u;
    while (!stack.empty()) {
        auto [node, d] = stack.back();
        stack.pop_back();
        depth = std::max(depth, d);
        for (auto c : accel.nodes[node].child) {
            if (c == LR_INVALID_ID) { continue; }
            if (!(c & 0x80000000u)) { stack.emplace_back(c, d + 1u); }
            else if (((c >> 27u) & 15u) != 0u) { return 0u; }
        }
    }
    return depth;
}

// ---- the tables that depend on the scene time (Pipeline::update / Geometry::update): built once per upload and again per
// lrhip_update_scene, which copies them over the existing device buffers
std::vector<lrd::DNodeQ> build_packed_nodes(const lr_scene *s) {
    std::vector<lrd::DNodeQ> packed(s->accel.node_count);
    const auto empty_ref = lrd::kLeafFlag | s->accel.triangle_count;// the sentinel of build_padded_triangles
    for (uint32_t i = 0; i < s->accel.node_count; i++) { packed[i] = quantise_node(s->accel.nodes[i], empty_ref); }
    return packed;
}

// the baked triangles + the all-zero sentinel the empty node slots name (flags 0: never hit)
std::vector<uint8_t> build_padded_triangles(const lr_scene *s) {
    std::vector<uint8_t> out((static_cast<size_t>(s->accel.triangle_count) + 1u) * sizeof(lr_bvh_triangle), 0u);
    std::memcpy(out.data(), s->accel.triangles, static_cast<size_t>(s->accel.triangle_count) * sizeof(lr_bvh_triangle));
    return out;
}

std::vector<lrd::DInstance> build_instances(const lr_scene *s) {// one 128-byte line each
    std::vector<lrd::DInstance> instances(s->instance_count);
    for (uint32_t i = 0; i < s->instance_count; i++) {
        auto &src = s->instances[i];
        auto &dst = instances[i];
        std::memset(&dst, 0, sizeof(dst));
        dst.handle[0] = src.handle.x, dst.handle[1] = src.handle.y, dst.handle[2] = src.handle.z, dst.handle[3] = src.handle.w;
        auto m = src.object_to_world;
        for (auto r = 0; r < 3; r++) { dst.c0[r] = m[r], dst.c1[r] = m[4 + r], dst.c2[r] = m[8 + r], dst.t[r] = m[12 + r]; }
        float nm[9];
        normal_matrix(m, nm);
        for (auto r = 0; r < 3; r++) { dst.n0[r] = nm[r], dst.n1[r] = nm[3 + r], dst.n2[r] = nm[6 + r]; }
        auto &mesh = s->meshes[src.handle.x >> 10u];
        dst.vertex_offset = mesh.vertex_offset;
        dst.triangle_offset = mesh.triangle_offset;
    }
    return instances;
}

// shading records of the baked triangles (dev_scene.h: DShadeTri), in BVH triangle order; empty + error text on bad references
std::vector<lrd::DShadeTri> build_shade_tris(const lr_scene *s, const std::vector<lrd::DInstance> &instances, std::string &error) {
    std::vector<lrd::DShadeTri> shade(s->accel.triangle_count);
    for (uint32_t i = 0; i < s->accel.triangle_count; i++) {
        auto &bt = s->accel.triangles[i];
        if (bt.inst >= s->instance_count) { error = "BVH triangle references an unknown instance"; return {}; }
        auto &inst = s->instances[bt.inst];
        auto &di = instances[bt.inst];
        auto &mesh = s->meshes[inst.handle.x >> 10u];
        if (bt.prim >= mesh.triangle_count) { error = "BVH triangle references an unknown primitive"; return {}; }
        auto tri = s->triangles[mesh.triangle_offset + bt.prim];
        const lr_vertex *v[3] = {s->vertices + mesh.vertex_offset + tri.i0, s->vertices + mesh.vertex_offset + tri.i1,
            s->vertices + mesh.vertex_offset + tri.i2};
        auto &r = shade[i];
        std::memset(&r, 0, sizeof(r));
        for (auto c = 0; c < 3; c++) { r.p0[c] = bt.v0[c], r.e1[c] = bt.e1[c], r.e2[c] = bt.e2[c]; }
        float *n[3] = {r.n0, r.n1, r.n2};
        for (auto k = 0; k < 3; k++) {
            for (auto c = 0; c < 3; c++) { n[k][c] = di.n0[c] * v[k]->nx + di.n1[c] * v[k]->ny + di.n2[c] * v[k]->nz; }
        }
        r.uv0x = v[0]->u, r.uv0y = v[0]->v, r.uv1x = v[1]->u, r.uv1y = v[1]->v, r.uv2x = v[2]->u, r.uv2y = v[2]->v;
        r.flags = inst.handle.x & 1023u, r.tags = inst.handle.y, r.offset_bits = inst.handle.w;
        // (round 6) bits 10-11: 1 + the heavy-closure kind of the triangle's surface (Disney 1, Mix 2, Layered 3; 0: a basic closure) --
        // what the lean passes of wavefront mode park a hit by, read with the record instead of through a dependent gather of the closure
        // table
        if ((r.flags & LR_SHAPE_HAS_SURFACE) != 0u) {
            const auto tag = (inst.handle.y >> 12u) & 4095u;
            if (tag < s->surface_count && s->surfaces[tag].kind >= LR_SURFACE_DISNEY) {
                r.flags |= (s->surfaces[tag].kind - LR_SURFACE_DISNEY + 1u) << 10u;
            }
        }
        r.tri_pdf = s->tri_pdf[mesh.triangle_offset + bt.prim];
        r.inst = bt.inst, r.prim = bt.prim, r.tri_offset = mesh.triangle_offset;
    }
    return shade;
}

// ---- the light sample's records (dev_scene.h: DLightInstance, DLightTri): laid out here, filled on the device
int upload_light_records(lrhip_ctx *ctx, const lr_scene *s) {
    auto &d = ctx->scene;
    std::vector<lrd::DLightInstance> records(s->light_instance_count);
    std::vector<uint32_t> owner;
    for (uint32_t i = 0u; i < s->light_instance_count; i++) {
        auto &r = records[i];
        std::memset(&r, 0, sizeof(r));
        const auto id = s->light_instances[i].instance_id;// (validate_indices: inside the instance table, its mesh inside the mesh table)
        const auto &handle = s->instances[id].handle;
        const auto &mesh = s->meshes[handle.x >> 10u];
        r.instance_id = id, r.alias_base = mesh.triangle_offset, r.alias_count = handle.z;
        r.tri_base = static_cast<uint32_t>(owner.size());
        // one record per slot the alias table can name: the mesh's triangles (handle.z is their number in every scene the host library builds)
        const auto count = std::max(mesh.triangle_count, handle.z);
        if (owner.size() + count > 0x7fffffffull / sizeof(lrd::DLightTri)) {
            return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_upload_scene: more than 2 GiB of emissive triangle records");
        }
        owner.insert(owner.end(), count, i);
    }
    auto upload = [&](const void *host, size_t bytes, const void **device) {
        DeviceBuffer b;
        b.bytes = std::max<size_t>(bytes, 16u);
        LR_HIP_CHECK(hipMalloc(&b.ptr, b.bytes));
        ctx->scene_buffers.emplace_back(b);
        if (host == nullptr) { LR_HIP_CHECK(hipMemset(b.ptr, 0, b.bytes)); }
        else if (bytes != 0u) { LR_HIP_CHECK(hipMemcpy(b.ptr, host, bytes, hipMemcpyHostToDevice)); }
        *device = b.ptr;
        return static_cast<int>(LRHIP_OK);
    };
    const void *dev_records = nullptr, *dev_tris = nullptr, *dev_exact = nullptr, *dev_owner = nullptr;
    if (auto r = upload(records.data(), records.size() * sizeof(records[0]), &dev_records); r != LRHIP_OK) { return r; }
    if (auto r = upload(nullptr, owner.size() * sizeof(lrd::DLightTri), &dev_tris); r != LRHIP_OK) { return r; }
    if (auto r = upload(nullptr, owner.size() * sizeof(lrd::DLightTri), &dev_exact); r != LRHIP_OK) { return r; }
    if (auto r = upload(owner.data(), owner.size() * sizeof(uint32_t), &dev_owner); r != LRHIP_OK) { return r; }
    d.light_records = static_cast<const lrd::DLightInstance *>(dev_records), d.light_tris = static_cast<const lrd::DLightTri *>(dev_tris);
    d.light_tris_exact = static_cast<const lrd::DLightTri *>(dev_exact);
    ctx->light_tri_owner = static_cast<const uint32_t *>(dev_owner);
    ctx->light_record_count = s->light_instance_count, ctx->light_tri_count = static_cast<uint32_t>(owner.size());
    // (the tables the kernels read are on the device: instances, vertices, triangles, tri_pdf; update_counts is not set yet)
    ctx->update_counts[2] = s->instance_count, ctx->update_counts[3] = static_cast<uint32_t>(s->triangle_count), ctx->vertex_count = s->vertex_count;
    if (auto r = bake_light_records(ctx, nullptr); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return LRHIP_OK;
}

int bake_light_records(lrhip_ctx *ctx, const uint32_t *moved) {
    if (ctx->light_record_count == 0u) { return LRHIP_OK; }
    const auto &d = ctx->scene;
    lrd::LightRecordArgs a{};
    a.records = const_cast<lrd::DLightInstance *>(d.light_records), a.record_count = ctx->light_record_count;
    a.tris = const_cast<lrd::DLightTri *>(d.light_tris), a.tri_count = ctx->light_tri_count;
    a.tri_owner = ctx->light_tri_owner;
    a.instances = d.instances, a.instance_count = ctx->update_counts[2];
    a.vertices = d.vertices, a.vertex_count = static_cast<uint32_t>(std::min<uint64_t>(ctx->vertex_count, 0xffffffffull));
    a.triangles = d.triangles, a.mesh_triangle_count = ctx->update_counts[3];
    a.tri_pdf = d.tri_pdf;
    a.moved = moved;
    const dim3 block(lrd::kLightRecordBlock);
    const auto blocks_for = [](uint32_t n) { return dim3((n + lrd::kLightRecordBlock - 1u) / lrd::kLightRecordBlock); };
    hipLaunchKernelGGL(lrd::light_instance_record_kernel, blocks_for(a.record_count), block, 0, ctx->stream, a);
    LR_HIP_CHECK(hipGetLastError());
    if (a.tri_count != 0u) {
        hipLaunchKernelGGL(lrd::light_triangle_record_kernel, blocks_for(a.tri_count), block, 0, ctx->stream, a);
        LR_HIP_CHECK(hipGetLastError());
        // the same records once more for the kernels built without contraction, by a unit that is built as they are
        a.tris = const_cast<lrd::DLightTri *>(d.light_tris_exact);
        LR_HIP_CHECK(launch_light_triangles_exact(ctx, a));
    }
    return LRHIP_OK;
}

void set_camera(lrd::DScene &d, const lr_scene *s) {
    auto &cam = d.camera;
    cam.kind = s->camera.kind, cam.width = s->camera.width, cam.height = s->camera.height;
    std::memcpy(cam.c2w, s->camera.camera_to_world, sizeof(cam.c2w));
    cam.tan_half_fov = s->camera.tan_half_fov, cam.focus_distance = s->camera.focus_distance;
    cam.lens_radius = s->camera.lens_radius, cam.projected_pixel_size = s->camera.projected_pixel_size;
    cam.ortho_scale = s->camera.ortho_scale, cam.clip_near = s->camera.clip_near, cam.clip_far = s->camera.clip_far;
}

// Images whose every texel is an 8-bit code's float are kept as 8-bit texels on the device (dev_shade.h: texel_at): one 32-bit word per
// texel, appended behind the float texels of the scene (offsets in 32-bit words from the same base pointer).  A channel qualifies if all
// its texels are b * (1 / 255.f) (form 1), all are b / 255.f (form 2), or all hold one value (a padded alpha); an image qualifies if
// all four channels do and the coded ones agree on the form.  The device's decode reproduces the host's floats bit for bit: form 1 is
// the same multiplication, form 2 is checked against the division for all 256 codes first.  Returns the packed words; `textures` (the
// copy that goes to the device) gets the new offsets, the form and the constant channels.
// Offsets of packed images come out relative to the packed area.
std::vector<uint32_t> pack_byte_textures(const lr_scene *s, std::vector<lr_texture> &textures) {
    std::vector<uint32_t> packed;
    auto division_ok = true;
    for (auto b = 0u; b < 256u; b++) { division_ok = division_ok && lrd::byte_over_255(static_cast<float>(b)) == static_cast<float>(b) / 255.f; }
    for (auto &t : textures) {
        t.pad = 0u;
        const auto count = static_cast<uint64_t>(t.width) * t.height;
        if (t.kind != LR_TEX_IMAGE || count == 0u || t.texel_offset + count > s->texel_count) { continue; }
        const auto px = s->texels + t.texel_offset * 4u;
        bool same[4], product[4], quotient[4];
        for (auto c = 0u; c < 4u; c++) {
            same[c] = true, product[c] = true, quotient[c] = division_ok;
            for (uint64_t i = 0u; i < count && (same[c] || product[c] || quotient[c]); i++) {
                const auto v = px[i * 4u + c];
                same[c] = same[c] && v == px[c];
                const auto code = v >= 0.f && v <= 1.f ? std::floor(v * 255.f + .5f) : -1.f;
                product[c] = product[c] && code >= 0.f && code * (1.f / 255.f) == v;
                quotient[c] = quotient[c] && code >= 0.f && code / 255.f == v;
            }
        }
        auto use = 0u, constant = 0u;
        for (auto f = 1u; f <= 2u && use == 0u; f++) {// the form under which every channel is either coded or one value
            auto all = true;
            auto mask = 0u;
            for (auto c = 0u; c < 4u; c++) {
                const auto coded = f == 1u ? product[c] : quotient[c];
                if (!coded && same[c]) { mask |= 1u << c; }
                all = all && (coded || same[c]);
            }
            if (all && mask != 15u) { use = f, constant = mask; }
        }
        if (use == 0u) { continue; }
        t.pad = use | (constant << 4u);
        for (auto c = 0u; c < 4u; c++) { if ((constant >> c) & 1u) { t.v[c] = px[c]; } }
        t.texel_offset = packed.size();// (relative to the packed area: lrhip_upload_scene adds its base)
        for (uint64_t i = 0u; i < count; i++) {
            auto word = 0u;
            for (auto c = 0u; c < 4u; c++) {
                const auto v = px[i * 4u + c];
                const auto code = (constant >> c) & 1u ? 0u : static_cast<uint32_t>(std::floor(v * 255.f + .5f));
                word |= (code & 255u) << (8u * c);
            }
            packed.push_back(word);
        }
    }
    return packed;
}

// Every index one table holds into another, checked once: the caller may be a third party, and nothing may read out of bounds
// on either side of the boundary (lrhip.h: "nothing throws or aborts across the boundary").
std::string validate_indices(const lr_scene *s) {
    auto tex_ok = [&](int32_t id) { return id < 0 || static_cast<uint32_t>(id) < s->texture_count; };
    for (uint32_t i = 0; i < s->texture_count; i++) {
        auto &t = s->textures[i];
        if (t.kind == LR_TEX_CHECKERBOARD && (!tex_ok(t.child[0]) || !tex_ok(t.child[1]))) {
            return "texture " + std::to_string(i) + ": child texture out of range";
        }
    }
    for (uint32_t i = 0; i < s->surface_count; i++) {
        auto &f = s->surfaces[i];
        for (auto t : f.tex) { if (!tex_ok(t)) { return "surface " + std::to_string(i) + ": texture id out of range"; } }
        if (!tex_ok(f.normal_tex) || !tex_ok(f.alpha_tex)) {
            return "surface " + std::to_string(i) + ": normal / alpha texture id out of range";
        }
        if ((f.kind == LR_SURFACE_MIX || f.kind == LR_SURFACE_LAYERED) && (f.u[0] >= s->surface_count || f.u[1] >= s->surface_count)) {
            return "surface " + std::to_string(i) + ": child surface out of range";
        }
    }
    for (uint32_t i = 0; i < s->light_count; i++) {
        auto e = s->lights[i].emission_tex;
        if (e < 0 || static_cast<uint32_t>(e) >= s->texture_count) { return "light " + std::to_string(i) + ": emission texture out of range"; }
    }
    for (uint32_t i = 0; i < s->instance_count; i++) {
        auto &h = s->instances[i].handle;
        if ((h.x >> 10u) >= s->mesh_count) { return "instance " + std::to_string(i) + ": mesh index out of range"; }
        auto flags = h.x & 1023u;
        if ((flags & LR_SHAPE_HAS_SURFACE) && ((h.y >> 12u) & 4095u) >= s->surface_count) {
            return "instance " + std::to_string(i) + ": surface tag out of range";
        }
        if ((flags & LR_SHAPE_HAS_LIGHT) && (h.y & 4095u) >= s->light_count) {
            return "instance " + std::to_string(i) + ": light tag out of range";
        }
    }
    for (uint32_t i = 0; i < s->light_instance_count; i++) {
        if (s->light_instances[i].instance_id >= s->instance_count) {
            return "light instance " + std::to_string(i) + ": instance id out of range";
        }
    }
    // a tree of Combined nodes over Spherical / Directional leaves (lr_scene.h: children before parents)
    if (s->environment.kind == LR_ENV_COMBINED) {
        std::vector<uint32_t> depth(s->environment_child_count, 0u);// Combined nodes from the record down, itself included
        auto check_node = [&](const lr_environment &c, uint32_t limit, uint32_t &d) -> std::string {
            d = 0u;
            if (c.kind != LR_ENV_COMBINED) { return {}; }
            for (auto k = 0; k < 2; k++) {
                if (c.child[k] >= limit) { return "child index out of range (children precede their parents in environment_children)"; }
                if (!(c.child_scale[k] > 0.f)) {
                    return "child scales must be positive (a Combined node with one live child is flattened by the host)";
                }
                d = std::max(d, depth[c.child[k]]);
            }
            d += 1u;
            return {};
        };
        for (uint32_t i = 0; i < s->environment_child_count; i++) {
            auto &c = s->environment_children[i];
            if (c.kind != LR_ENV_SPHERICAL && c.kind != LR_ENV_DIRECTIONAL && c.kind != LR_ENV_COMBINED) {
                return "environment child " + std::to_string(i) + ": invalid kind";
            }
            if (c.kind != LR_ENV_COMBINED && (c.emission_tex < 0 || static_cast<uint32_t>(c.emission_tex) >= s->texture_count)) {
                return "environment child " + std::to_string(i) + ": emission texture out of range";
            }
            if (auto bad = check_node(c, i, depth[i]); !bad.empty()) { return "environment child " + std::to_string(i) + ": " + bad; }
        }
        uint32_t root_depth = 0u;
        if (auto bad = check_node(s->environment, s->environment_child_count, root_depth); !bad.empty()) { return "environment: " + bad; }
        if (root_depth > static_cast<uint32_t>(LR_ENV_MAX_COMBINED_DEPTH)) {
            return "environment: Combined nodes nested deeper than LR_ENV_MAX_COMBINED_DEPTH";
        }
    }
    return {};
}

}// namespace lrh
