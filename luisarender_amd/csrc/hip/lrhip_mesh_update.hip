// lrhip_mesh_update.hip — C ABI of deforming a mesh on the device (include/lrhip.h: lrhip_set_mesh_vertices, lrhip_last_mesh_update_ms;
// DESIGN §4.12).  Holds the kernels of mesh_update_kernels.h; the re-bake of the marked instances and the refit behind them are the kernels of
// lrhip_instance_update.hip (rebake_and_refit).  This object is held to unfused host code bit for bit like that one, and is built with
// the same flags: no fp contraction, correctly rounded fp32 division and square root (Makefile: lrhip_mesh_update_FLAGS).
#include "lrhip_internal.h"
#include "mesh_update_kernels.h"

static_assert(sizeof(lr_vertex) == 32u && offsetof(lr_vertex, nx) == 12u && offsetof(lr_vertex, u) == 24u, "a vertex is px py pz nx ny nz u v");
static_assert(sizeof(lr_triangle) == 12u, "mesh_normal_kernel reads a triangle as three indices");

namespace lrh {

namespace {

unsigned blocks_for(uint64_t threads) { return static_cast<unsigned>((threads + lrd::kMeshUpdateBlock - 1u) / lrd::kMeshUpdateBlock); }

// The corner lists of mesh `m` (mesh_update_kernels.h: offsets, then corners, in one buffer), built on the first call that recomputes the
// mesh's normals and kept until the scene is released.  The mesh's index range is READ BACK from the device table -- no call writes it
// after the upload -- rather than kept in host memory from the upload on for every mesh of every scene: 12 B per triangle that most
// contexts would never use.  The read-back and the copy of the lists synchronise.
int ensure_adjacency(lrhip_ctx *ctx, uint32_t m) {
    auto &buffer = ctx->mesh_adjacency[m];
    if (buffer.ptr != nullptr) { return LRHIP_OK; }
    const auto &mesh = ctx->meshes[m];
    std::vector<lr_triangle> tris(mesh.triangle_count);
    if (!tris.empty()) {
        LR_HIP_CHECK(hipMemcpy(tris.data(), ctx->scene.triangles + mesh.triangle_offset, tris.size() * sizeof(lr_triangle), hipMemcpyDeviceToHost));
    }
    // a counting sort of the corners by vertex: ascending triangle, then ascending corner, within every list
    std::vector<uint32_t> lists(static_cast<size_t>(mesh.vertex_count) + 1u + tris.size() * 3u, 0u);
    const auto offsets = lists.data(), corners = lists.data() + mesh.vertex_count + 1u;
    for (auto &t : tris) {
        for (auto i : {t.i0, t.i1, t.i2}) {
            if (i < mesh.vertex_count) { offsets[i + 1u]++; }// (an index outside the mesh names no vertex of it: the kernel skips such a triangle)
        }
    }
    for (uint32_t v = 0u; v < mesh.vertex_count; v++) { offsets[v + 1u] += offsets[v]; }
    std::vector<uint32_t> next(offsets, offsets + mesh.vertex_count);
    for (uint32_t t = 0u; t < tris.size(); t++) {
        for (auto i : {tris[t].i0, tris[t].i1, tris[t].i2}) {
            if (i < mesh.vertex_count) { corners[next[i]++] = t; }
        }
    }
    if (auto r = ensure(buffer, lists.size() * sizeof(uint32_t)); r != LRHIP_OK) { return r; }
    if (auto err = hipMemcpy(buffer.ptr, lists.data(), lists.size() * sizeof(uint32_t), hipMemcpyHostToDevice); err != hipSuccess) {
        buffer.release();// (a buffer that is there counts as built)
        return fail(LRHIP_ERROR_DEVICE, std::string{"lrhip_set_mesh_vertices: copying the corner lists: "} + hipGetErrorString(err));
    }
    return LRHIP_OK;
}

// the kernels of one call over `count` vertices in device memory, between the events of the context's mesh timer
int update_device(lrhip_ctx *ctx, const lrhip_mesh_update_params *p, const void *positions, const void *normals) {
    const auto &d = ctx->scene;
    const auto &mesh = ctx->meshes[p->mesh];
    const auto recompute = (p->flags & LRHIP_MESH_RECOMPUTE_NORMALS) != 0u;
    if (recompute) {
        if (auto r = ensure_adjacency(ctx, p->mesh); r != LRHIP_OK) { return r; }
    }
    lrd::MeshUpdateArgs a{};
    a.positions = static_cast<const float *>(positions), a.normals = static_cast<const float *>(normals);
    a.count = static_cast<uint32_t>(p->count), a.first = mesh.vertex_offset + p->first_vertex;
    a.vertices = const_cast<lr_vertex *>(d.vertices), a.vertex_count = static_cast<uint32_t>(std::min<uint64_t>(ctx->vertex_count, 0xffffffffull));
    a.triangles = d.triangles, a.triangle_count = ctx->update_counts[3];
    a.mesh = p->mesh, a.mesh_vertex_offset = mesh.vertex_offset, a.mesh_vertex_count = mesh.vertex_count;
    a.mesh_triangle_offset = mesh.triangle_offset, a.mesh_triangle_count = mesh.triangle_count;
    if (recompute) {
        a.offsets = static_cast<const uint32_t *>(ctx->mesh_adjacency[p->mesh].ptr);
        a.corners = a.offsets + mesh.vertex_count + 1u;
    }
    a.instances = d.instances, a.instance_count = ctx->update_counts[2];
    if (auto r = clear_update_scratch(ctx); r != LRHIP_OK) { return r; }
    a.moved = update_moved_mask(ctx);
    const dim3 block(lrd::kMeshUpdateBlock);
    if (auto r = timer_begin(ctx, ctx->mesh_timer); r != LRHIP_OK) { return r; }
    hipLaunchKernelGGL(lrd::mesh_vertex_kernel, dim3(blocks_for(a.count)), block, 0, ctx->stream, a);
    LR_HIP_CHECK(hipGetLastError());
    if (recompute && mesh.vertex_count != 0u) {
        hipLaunchKernelGGL(lrd::mesh_normal_kernel, dim3(blocks_for(mesh.vertex_count)), block, 0, ctx->stream, a);
        LR_HIP_CHECK(hipGetLastError());
    }
    if (a.instance_count != 0u) {
        hipLaunchKernelGGL(lrd::mesh_mark_kernel, dim3(blocks_for(a.instance_count)), block, 0, ctx->stream, a);
        LR_HIP_CHECK(hipGetLastError());
    }
    if (auto r = rebake_and_refit(ctx); r != LRHIP_OK) { return r; }
    return timer_end(ctx, ctx->mesh_timer);
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_set_mesh_vertices(lrhip_ctx *ctx, const lrhip_mesh_update_params *p) {
    // (no count screened: a mesh's vertex count bounds it below)
    if (auto r = screen("lrhip_set_mesh_vertices", ctx, p, LRHIP_RAY_DEVICE_POINTERS | LRHIP_MESH_RECOMPUTE_NORMALS, nullptr); r != LRHIP_OK) { return r; }
    const std::string what{"lrhip_set_mesh_vertices: "};
    if (p->mesh >= ctx->meshes.size()) {
        return fail(LRHIP_ERROR_INVALID, what + "mesh " + std::to_string(p->mesh) + " out of range (" + std::to_string(ctx->meshes.size()) + " meshes)");
    }
    const auto &mesh = ctx->meshes[p->mesh];
    if (static_cast<uint64_t>(mesh.vertex_offset) + mesh.vertex_count > ctx->vertex_count ||
        static_cast<uint64_t>(mesh.triangle_offset) + mesh.triangle_count > ctx->update_counts[3]) {
        return fail(LRHIP_ERROR_INVALID, what + "mesh " + std::to_string(p->mesh) + " of the uploaded scene does not lie inside its vertex and triangle tables");
    }
    if (p->first_vertex > mesh.vertex_count || p->count > mesh.vertex_count - p->first_vertex) {
        return fail(LRHIP_ERROR_INVALID, what + "vertices " + std::to_string(p->first_vertex) + " + " + std::to_string(p->count) +
                                             " are not inside the mesh's " + std::to_string(mesh.vertex_count));
    }
    if (p->count != 0u && p->positions == nullptr) { return fail(LRHIP_ERROR_INVALID, what + "positions is NULL"); }
    const auto recompute = (p->flags & LRHIP_MESH_RECOMPUTE_NORMALS) != 0u;
    if (recompute && p->normals != nullptr) { return fail(LRHIP_ERROR_INVALID, what + "normals must be NULL with LRHIP_MESH_RECOMPUTE_NORMALS"); }
    if (ctx->mesh_light[p->mesh] != LR_INVALID_ID) {
        return fail(LRHIP_ERROR_UNSUPPORTED, what + "mesh " + std::to_string(p->mesh) + " is an emitter (instance " + std::to_string(ctx->mesh_light[p->mesh]) +
                                                 " carries a light): its area sampling tables are not rebuilt on the device");
    }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    const auto floats = static_cast<size_t>(p->count) * 3u;
    if (device_pointers && p->count != 0u) {
        if (misaligned({{p->positions, 3u}, {p->normals, 3u}})) {
            return fail(LRHIP_ERROR_INVALID, what + "device positions and normals must be 4-byte aligned");
        }
    }
    if (!device_pointers) {
        for (auto array : {static_cast<const float *>(p->positions), static_cast<const float *>(p->normals)}) {
            for (size_t i = 0u; array != nullptr && i < floats; i++) {
                if (!std::isfinite(array[i])) {
                    return fail(LRHIP_ERROR_INVALID, what + "vertex " + std::to_string(i / 3u) + " has a non-finite " +
                                                         (array == p->normals ? "normal" : "position"));
                }
            }
        }
    }
    if (p->count != 0u && ctx->level_offsets.empty()) {
        return fail(LRHIP_ERROR_UNSUPPORTED, what + "the BVH's nodes are not stored parents first; it cannot be refitted in place");
    }
    if (auto r = timer_start(ctx, ctx->mesh_timer, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    if (device_pointers) { return update_device(ctx, p, p->positions, p->normals); }
    // host pointers: positions, then normals, through the staging buffer
    const auto bytes = floats * sizeof(float);
    if (auto r = ensure(ctx->update_stage, bytes * 2u); r != LRHIP_OK) { return r; }
    const auto staged_normals = static_cast<char *>(ctx->update_stage.ptr) + bytes;
    LR_HIP_CHECK(hipMemcpyAsync(ctx->update_stage.ptr, p->positions, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (p->normals != nullptr) { LR_HIP_CHECK(hipMemcpyAsync(staged_normals, p->normals, bytes, hipMemcpyHostToDevice, ctx->stream)); }
    if (auto r = update_device(ctx, p, ctx->update_stage.ptr, p->normals != nullptr ? staged_normals : nullptr); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return timer_collect(ctx->mesh_timer, false);
}

double lrhip_last_mesh_update_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->mesh_timer, false) : 0.0; }

}// extern "C"
