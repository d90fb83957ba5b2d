// lrhip_instance_update.hip — C ABI of moving instances on the device (include/lrhip.h: lrhip_set_instance_transforms,
// lrhip_last_instance_update_ms) and the test hook that reads the moved tables back (lrhip_read_scene_table).  Holds the kernels
// of instance_update_kernels.h, and launches the re-bake and refit for lrhip_mesh_update.hip too (rebake_and_refit).  This object is held
// to unfused host code bit for bit, so it is built with flags of its own: no fp contraction, correctly rounded fp32 division (Makefile:
// lrhip_instance_update_FLAGS).
#include "lrhip_internal.h"
#include "instance_update_kernels.h"

static_assert(sizeof(lr_bvh4_node) == 128u && offsetof(lr_bvh4_node, hi_x) == 48u && offsetof(lr_bvh4_node, child) == 96u,
    "instance_refit_kernel reads a node as rows lo_x lo_y lo_z hi_x hi_y hi_z child");
static_assert(sizeof(lr_bvh_triangle) == 48u && offsetof(lr_bvh_triangle, inst) == 12u && offsetof(lr_bvh_triangle, prim) == 28u,
    "instance_triangle_kernel reads a baked triangle as (v0, inst) (e1, prim) (e2, flags)");
static_assert(sizeof(lr_vertex) == 32u && offsetof(lr_vertex, nx) == 12u, "a vertex is (px py pz nx) (ny nz u v)");
static_assert(offsetof(lrd::DInstance, c0) == 16u && offsetof(lrd::DInstance, vertex_offset) == 28u && offsetof(lrd::DInstance, triangle_offset) == 44u
    && offsetof(lrd::DInstance, t) == 64u && offsetof(lrd::DInstance, n0) == 80u, "instance_triangle_kernel reads an instance record by quads");
static_assert(offsetof(lrd::DShadeTri, n0) == 48u && offsetof(lrd::DShadeTri, uv1y) == 96u, "the first six quads of a shading record move");

namespace lrd {
// the light sample's triangle records with THIS unit's arithmetic (light_record_kernels.h; kernel_forms.h: LR_LIGHT_TRIS): what the kernels
// built without contraction and with correctly rounded division and square root compute per sample
__global__ void __launch_bounds__(kLightRecordBlock) light_triangle_record_exact_kernel(LightRecordArgs a) {
    light_triangle_record(a, blockIdx.x * kLightRecordBlock + threadIdx.x);
}
}// namespace lrd

namespace lrh {

hipError_t launch_light_triangles_exact(lrhip_ctx *ctx, const lrd::LightRecordArgs &args) {
    hipLaunchKernelGGL(lrd::light_triangle_record_exact_kernel, dim3((args.tri_count + lrd::kLightRecordBlock - 1u) / lrd::kLightRecordBlock),
                       dim3(lrd::kLightRecordBlock), 0, ctx->stream, args);
    return hipGetLastError();
}

namespace {

size_t table_bytes(const lrhip_ctx *ctx, uint32_t which, const void **base) {
    if (!ctx->scene_ready) { return 0u; }
    const auto &d = ctx->scene;
    switch (which) {
        case LRHIP_TABLE_NODES: *base = d.nodes; return static_cast<size_t>(ctx->update_counts[0]) * sizeof(lrd::DNodeQ);
        case LRHIP_TABLE_BVH_TRIANGLES: *base = d.bvh_tris; return (static_cast<size_t>(ctx->update_counts[1]) + 1u) * sizeof(lr_bvh_triangle);
        case LRHIP_TABLE_INSTANCES: *base = d.instances; return static_cast<size_t>(ctx->update_counts[2]) * sizeof(lrd::DInstance);
        case LRHIP_TABLE_SHADE_TRIANGLES: *base = d.shade_tris; return static_cast<size_t>(ctx->update_counts[1]) * sizeof(lrd::DShadeTri);
        case LRHIP_TABLE_VERTICES: *base = d.vertices; return static_cast<size_t>(ctx->vertex_count) * sizeof(lr_vertex);
        case LRHIP_TABLE_LIGHT_INSTANCES: *base = d.light_records; return static_cast<size_t>(ctx->light_record_count) * sizeof(lrd::DLightInstance);
        case LRHIP_TABLE_LIGHT_TRIANGLES: *base = d.light_tris; return static_cast<size_t>(ctx->light_tri_count) * sizeof(lrd::DLightTri);
        case LRHIP_TABLE_LIGHT_TRIANGLES_EXACT: *base = d.light_tris_exact; return static_cast<size_t>(ctx->light_tri_count) * sizeof(lrd::DLightTri);
        default: return 0u;
    }
}

unsigned blocks_for(uint64_t threads) { return static_cast<unsigned>((threads + lrd::kUpdateBlock - 1u) / lrd::kUpdateBlock); }

// the tables of the uploaded scene as the kernels take them, with the call's scratch
lrd::InstanceUpdateArgs scene_args(lrhip_ctx *ctx) {
    const auto &d = ctx->scene;
    const auto instance_count = ctx->update_counts[2];
    lrd::InstanceUpdateArgs a{};
    a.instances = const_cast<lrd::DInstance *>(d.instances), a.instance_count = instance_count;
    a.bvh_tris = const_cast<lr_bvh_triangle *>(d.bvh_tris), a.triangle_count = ctx->update_counts[1];
    a.shade_tris = const_cast<lrd::DShadeTri *>(d.shade_tris);
    a.nodes = const_cast<lrd::DNodeQ *>(d.nodes), a.node_count = ctx->update_counts[0];
    a.nodes32 = ctx->nodes32;
    a.vertices = d.vertices, a.vertex_count = static_cast<uint32_t>(std::min<uint64_t>(ctx->vertex_count, 0xffffffffull));
    a.triangles = d.triangles, a.mesh_triangle_count = ctx->update_counts[3];
    a.owner = static_cast<uint32_t *>(ctx->update_scratch.ptr);
    a.moved = update_moved_mask(ctx);
    return a;
}

// the kernels of one call over `count` matrices in device memory, between the events of the context's instance timer
int update_device(lrhip_ctx *ctx, const void *matrices, const void *ids, uint32_t count) {
    if (ctx->update_counts[2] == 0u) { return LRHIP_OK; }// (every id is out of range)
    if (auto r = clear_update_scratch(ctx); r != LRHIP_OK) { return r; }
    auto a = scene_args(ctx);
    a.matrices = static_cast<const float4 *>(matrices), a.ids = static_cast<const uint32_t *>(ids), a.count = count;
    const dim3 block(lrd::kUpdateBlock);
    if (auto r = timer_begin(ctx, ctx->instance_timer); r != LRHIP_OK) { return r; }
    hipLaunchKernelGGL(lrd::instance_claim_kernel, dim3(blocks_for(count)), block, 0, ctx->stream, a);
    LR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lrd::instance_record_kernel, dim3(blocks_for(count)), block, 0, ctx->stream, a);
    LR_HIP_CHECK(hipGetLastError());
    if (auto r = rebake_and_refit(ctx); r != LRHIP_OK) { return r; }
    return timer_end(ctx, ctx->instance_timer);
}

}// namespace

// scratch of a call: an owner word per instance, then a bit per instance; cleared per call, so that nothing leaks from the call before
int clear_update_scratch(lrhip_ctx *ctx) {
    const auto instance_count = ctx->update_counts[2];
    const auto owner_bytes = static_cast<size_t>(instance_count) * sizeof(uint32_t);
    const auto mask_bytes = (static_cast<size_t>(instance_count) + 31u) / 32u * sizeof(uint32_t);
    if (auto r = ensure(ctx->update_scratch, owner_bytes + mask_bytes); r != LRHIP_OK) { return r; }
    if (owner_bytes + mask_bytes != 0u) { LR_HIP_CHECK(hipMemsetAsync(ctx->update_scratch.ptr, 0, owner_bytes + mask_bytes, ctx->stream)); }
    return LRHIP_OK;
}

uint32_t *update_moved_mask(lrhip_ctx *ctx) { return static_cast<uint32_t *>(ctx->update_scratch.ptr) + ctx->update_counts[2]; }

int rebake_and_refit(lrhip_ctx *ctx) {
    const auto a = scene_args(ctx);
    const dim3 block(lrd::kUpdateBlock);
    if (a.triangle_count != 0u) {
        hipLaunchKernelGGL(lrd::instance_triangle_kernel, dim3(blocks_for(a.triangle_count)), block, 0, ctx->stream, a);
        LR_HIP_CHECK(hipGetLastError());
    }
    // the light sample's records of the marked instances (lrhip_tables.hip: bake_light_records); an instance without a light has none, and
    // nothing of another instance's is written
    if (auto r = bake_light_records(ctx, a.moved); r != LRHIP_OK) { return r; }
    // every node of every level, from the deepest level up (restricting the refit to the ancestors of moved triangles: not done)
    for (auto l = ctx->level_offsets.size() - 1u; l-- > 0u;) {
        const auto first = ctx->level_offsets[l], n = ctx->level_offsets[l + 1u] - first;
        if (n == 0u) { continue; }
        hipLaunchKernelGGL(lrd::instance_refit_kernel, dim3(blocks_for(static_cast<uint64_t>(n) * 4u)), block, 0, ctx->stream, a,
                           ctx->level_nodes + first, n);
        LR_HIP_CHECK(hipGetLastError());
    }
    return LRHIP_OK;
}

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_set_instance_transforms(lrhip_ctx *ctx, const lrhip_instance_update_params *p) {
    if (auto r = screen("lrhip_set_instance_transforms", ctx, p, LRHIP_RAY_DEVICE_POINTERS, "matrices"); r != LRHIP_OK) { return r; }
    const auto instance_count = ctx->update_counts[2];
    if (p->instances == nullptr && p->count > instance_count) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_set_instance_transforms: " + std::to_string(p->count) + " matrices without ids for " +
                                             std::to_string(instance_count) + " instances");
    }
    if (p->count != 0u && p->object_to_world == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_set_instance_transforms: object_to_world is NULL"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    const auto count = static_cast<uint32_t>(p->count);
    if (device_pointers && count != 0u) {
        if (misaligned({{p->object_to_world, 15u}, {p->instances, 3u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_set_instance_transforms: device matrices must be 16-byte aligned, device ids 4-byte aligned");
        }
    }
    if (!device_pointers && count != 0u) {
        const auto ids = static_cast<const uint32_t *>(p->instances);
        if (ids != nullptr) {
            std::vector<char> seen(instance_count, 0);
            for (uint32_t i = 0u; i < count; i++) {
                if (ids[i] >= instance_count) {
                    return fail(LRHIP_ERROR_INVALID, "lrhip_set_instance_transforms: instance id " + std::to_string(ids[i]) + " out of range");
                }
                if (seen[ids[i]] != 0) {
                    return fail(LRHIP_ERROR_INVALID, "lrhip_set_instance_transforms: instance id " + std::to_string(ids[i]) + " is listed twice");
                }
                seen[ids[i]] = 1;
            }
        }
        const auto m = static_cast<const float *>(p->object_to_world);
        for (size_t i = 0u; i < static_cast<size_t>(count) * 16u; i++) {
            if (!std::isfinite(m[i])) {
                return fail(LRHIP_ERROR_INVALID, "lrhip_set_instance_transforms: matrix " + std::to_string(i / 16u) + " has a non-finite element");
            }
        }
    }
    if (count != 0u && ctx->level_offsets.empty()) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_set_instance_transforms: the BVH's nodes are not stored parents first; it cannot be refitted in place");
    }
    if (auto r = timer_start(ctx, ctx->instance_timer, count != 0u); r != LRHIP_OK) { return r; }
    if (count == 0u) { return LRHIP_OK; }
    if (device_pointers) { return update_device(ctx, p->object_to_world, p->instances, count); }
    // host pointers: matrices, then ids, through the staging buffer
    const auto matrix_bytes = static_cast<size_t>(count) * 16u * sizeof(float), id_bytes = static_cast<size_t>(count) * sizeof(uint32_t);
    if (auto r = ensure(ctx->update_stage, matrix_bytes + id_bytes); r != LRHIP_OK) { return r; }
    const auto staged_ids = static_cast<char *>(ctx->update_stage.ptr) + matrix_bytes;
    LR_HIP_CHECK(hipMemcpyAsync(ctx->update_stage.ptr, p->object_to_world, matrix_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (p->instances != nullptr) { LR_HIP_CHECK(hipMemcpyAsync(staged_ids, p->instances, id_bytes, hipMemcpyHostToDevice, ctx->stream)); }
    if (auto r = update_device(ctx, ctx->update_stage.ptr, p->instances != nullptr ? staged_ids : nullptr, count); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return timer_collect(ctx->instance_timer, false);
}

double lrhip_last_instance_update_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->instance_timer, false) : 0.0; }

uint64_t lrhip_scene_table_bytes(lrhip_ctx *ctx, uint32_t which) {
    const void *base = nullptr;
    return ctx != nullptr ? table_bytes(ctx, which, &base) : 0u;
}

int lrhip_read_scene_table(lrhip_ctx *ctx, uint32_t which, uint64_t byte_offset, uint64_t bytes, void *out) {
    if (ctx == nullptr || !ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_read_scene_table: no scene uploaded"); }
    if (which > LRHIP_TABLE_SHADE_TRIANGLES && which != LRHIP_TABLE_VERTICES && which != LRHIP_TABLE_LIGHT_INSTANCES && which != LRHIP_TABLE_LIGHT_TRIANGLES &&
        which != LRHIP_TABLE_LIGHT_TRIANGLES_EXACT) { return fail(LRHIP_ERROR_INVALID, "lrhip_read_scene_table: unknown table"); }
    const void *base = nullptr;
    const auto size = table_bytes(ctx, which, &base);
    if (byte_offset > size || bytes > size - byte_offset) { return fail(LRHIP_ERROR_INVALID, "lrhip_read_scene_table: the range is not inside the table"); }
    if (bytes != 0u && out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_read_scene_table: out is NULL"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (bytes != 0u) { LR_HIP_CHECK(hipMemcpy(out, static_cast<const char *>(base) + byte_offset, bytes, hipMemcpyDeviceToHost)); }
    return LRHIP_OK;
}

}// extern "C"
