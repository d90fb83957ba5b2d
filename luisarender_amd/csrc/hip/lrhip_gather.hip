// lrhip_gather.hip — C ABI of the gather vertex query (include/lrhip.h: lrhip_query_gather_vertex, lrhip_last_gather_ms).  Holds
// the four instantiations of gather_kernel.h (hit or texel records / bare points x Independent / generic sampler) and their launches on the
// context's stream, through the queries' one host path (lrhip_query.hip).  The texture lookup and the environment's evaluate / sample are
// real calls in this translation unit, and it holds dev_shade.h's walk of nested Combined environments, as lrhip_light.hip; the object is
// built with the oracle's arithmetic, as lrhip_light.o and for its reason (Makefile: lrhip_gather_FLAGS): a query hands single answers to
// its caller, and these are held to the light and BSDF queries' bit for bit
#define LR_CALL __device__ __noinline__
#define LR_ENV_TREE_WALK 1
#define LR_EXACT_ARITHMETIC_UNIT 1// (Makefile: this unit's flags; kernel_forms.h: LR_LIGHT_TRIS)
#include "lrhip_internal.h"
#include "gather_kernel.h"

static_assert(sizeof(lrhip_gather_vertex) == 96u && sizeof(lrhip_gather_vertex) == lrd::kGatherVertexFloat4s * sizeof(float4) &&
                  offsetof(lrhip_gather_vertex, shadow) == 32u && offsetof(lrhip_gather_vertex, nee) == 64u && offsetof(lrhip_gather_vertex, light_pdf) == 76u &&
                  offsetof(lrhip_gather_vertex, beta) == 80u && offsetof(lrhip_gather_vertex, pdf) == 92u,
              "lrhip_gather_vertex = the six float4 gather_vertex_kernel stores");
static_assert(LRHIP_GATHER_FROM_POINTS == LRHIP_LIGHT_FROM_POINTS, "bare points are flagged as the light query flags them");

namespace lrd {
template __global__ void gather_vertex_kernel<false, false>(DScenePtr, GatherArgs);
template __global__ void gather_vertex_kernel<false, true>(DScenePtr, GatherArgs);
template __global__ void gather_vertex_kernel<true, false>(DScenePtr, GatherArgs);
template __global__ void gather_vertex_kernel<true, true>(DScenePtr, GatherArgs);
}

static_assert(LRHIP_GATHER_ACCUMULATE == LRHIP_RADIANCE_ACCUMULATE && LRHIP_FEAT_GATHER == lrd::kFeatGather, "lrhip.h's values are the kernels'");
static_assert(sizeof(lrd::GatherTable) == 32u, "the gather table is two pointers and four words");

using namespace lrh;

namespace {

struct GatherLaunch {
    uint32_t mask;   // the kernel
    Chunking ck;     // sample chunks of an item: a function of the CALL's record count and sample range, the same for every staged chunk
    uint32_t spp_begin, spp_end;
    float clamp;
};

// one launch over `count` records in device memory (and, with several sample chunks, the reduce of their partial planes), between the events
// of the context's gather timer: lrhip_radiance.hip's launch_device with the records in the rays' column and the gather table beside it
int launch_gather(lrhip_ctx *ctx, const GatherLaunch &q, const void *records, const void *normals, const void *streams, void *out, uint32_t count,
                  uint32_t stream_base) {
    const auto entry = find_kernel(q.mask);
    if (entry == nullptr) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_gather_irradiance: no gather kernel for feature mask " + std::to_string(q.mask) +
                                                 " was compiled into this library");
    }
    uint32_t blocks_per_cu = 0u;
    if (auto r = kernel_blocks(ctx, *entry, 0u, blocks_per_cu); r != LRHIP_OK) { return r; }
    if (auto r = resident_meshes(ctx); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->gather_table, sizeof(lrd::GatherTable)); r != LRHIP_OK) { return r; }
    lrd::GatherTable table{};
    table.normals = static_cast<const float4 *>(normals), table.meshes = static_cast<const lr_mesh *>(ctx->surface_meshes.ptr);
    table.triangle_count = ctx->update_counts[1], table.instance_count = ctx->update_counts[2];
    table.mesh_count = static_cast<uint32_t>(ctx->meshes.size());
    // (pageable host memory: hipMemcpyAsync has staged it when it returns, as upload_scene_record's)
    LR_HIP_CHECK(hipMemcpyAsync(ctx->gather_table.ptr, &table, sizeof(table), hipMemcpyHostToDevice, ctx->stream));
    const auto resident = ctx->cu_count * blocks_per_cu;
    const auto tiles = (count + 63u) / 64u;// items of 64 consecutive records
    lrd::RenderArgs args{};
    args.spp_begin = q.spp_begin, args.spp_end = q.spp_end;
    args.tile_begin = 0u, args.tile_end = tiles, args.tile_stride = 1u;
    args.tiles_x = tiles, args.tiles_y = 1u;
    args.chunk_count = q.ck.count;
    args.chunk_big_count = q.ck.big_count, args.chunk_big = q.ck.big, args.chunk_small = q.ck.small;
    args.item_count = tiles * q.ck.count;
    args.work_counter = static_cast<uint32_t *>(ctx->work_counter.ptr);
    args.spill = static_cast<uint32_t *>(ctx->spill.ptr);
    args.counters = static_cast<lrd::DCounters *>(ctx->counters.ptr);
    args.total_threads = resident * lrd::kBlockThreads;
    args.pool = static_cast<float4 *>(ctx->gather_table.ptr);// (the gather kernels read a GatherTable there: megapath_kernel.h)
    args.query_rays = static_cast<const float4 *>(records), args.query_streams = static_cast<const uint32_t *>(streams);
    args.query_out = static_cast<float4 *>(out), args.query_count = count, args.query_stream_base = stream_base;
    // THE BOUND OF THE STACK'S OVERFLOW AREA, as lrhip_trace_radiance checks it
    const auto blocks = std::min(resident, (args.item_count + 3u) / 4u);
    if (resident > ctx->grid_blocks || static_cast<size_t>(args.total_threads) * lrd::kSpillEntries * sizeof(uint32_t) > ctx->spill.bytes) {
        return fail(LRHIP_ERROR_DEVICE, "lrhip_gather_irradiance: the grid does not fit the traversal stack's overflow area");
    }
    if (q.ck.count > 1u) {
        if (auto r = ensure(ctx->partial, static_cast<size_t>(q.ck.count) * count * sizeof(float4)); r != LRHIP_OK) { return r; }
        args.partial = static_cast<float4 *>(ctx->partial.ptr);
    }
    LR_HIP_CHECK(hipMemsetAsync(ctx->work_counter.ptr, 0, 1024u, ctx->stream));
    auto record = ctx->scene;
    record.film_clamp = q.clamp, record.shutter_weight = 1.f;
    lrd::DScenePtr device_scene{};
    if (auto r = upload_scene_record(ctx, device_scene, &record); r != LRHIP_OK) { return r; }
    if (auto r = timer_begin(ctx, ctx->gather_timer); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(entry->launch(blocks, ctx->stream, (const lrd::DScene *)device_scene, &args, 0u));
    if (q.ck.count > 1u) { LR_HIP_CHECK(launch_resolve_records(ctx, args.query_out, args.partial, count, q.ck.count)); }
    return timer_end(ctx, ctx->gather_timer);
}

}// namespace

extern "C" {

int lrhip_gather_irradiance(lrhip_ctx *ctx, const lrhip_gather_params *p) {
    if (auto r = screen("lrhip_gather_irradiance", ctx, p, LRHIP_RAY_DEVICE_POINTERS | LRHIP_GATHER_ACCUMULATE | LRHIP_GATHER_FROM_POINTS, "records");
        r != LRHIP_OK) { return r; }
    const std::string what{"lrhip_gather_irradiance: "};
    if (!(p->clamp >= 0.f)) { return fail(LRHIP_ERROR_INVALID, what + "the clamp must be positive, or 0 for the scene's"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    const auto accumulate = (p->flags & LRHIP_GATHER_ACCUMULATE) != 0u;
    const auto points = (p->flags & LRHIP_GATHER_FROM_POINTS) != 0u;
    const auto normals = points ? p->normals : nullptr;// what the mode does not read is not looked at
    if (p->count != 0u) {
        if (p->records == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, what + "records / out is NULL"); }
        if (points && normals == nullptr) { return fail(LRHIP_ERROR_INVALID, what + "normals is NULL with LRHIP_GATHER_FROM_POINTS"); }
        if (device_pointers && misaligned({{p->records, 15u}, {normals, 15u}, {p->out, 15u}, {p->streams, 3u}})) {
            return fail(LRHIP_ERROR_INVALID, what + "device pointers must be 16-byte aligned (streams: 4-byte)");
        }
    }
    if ((ctx->features & (lrd::kFeatAux | lrd::kFeatVpt | lrd::kFeatAov)) != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, what + "the uploaded scene's integrator is not MegaPath");
    }
    // a scene without lights and without an environment: nothing is launched, as lrhip_trace_radiance and lrhip_render do (the light sampler
    // divides by the light count and indexes the light tables)
    const auto no_lighting = !ctx->scene.has_lights && ctx->scene.env_kind == lrd::kEnvNone;
    const auto launches = p->count != 0u && p->spp_begin < p->spp_end && !no_lighting;
    if (auto r = timer_start(ctx, ctx->gather_timer, launches); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    if (!launches) {// a record that is not accumulated into holds the sums of no sample
        const auto out_bytes = static_cast<size_t>(p->count) * sizeof(float4);
        if (!accumulate) {
            if (device_pointers) { LR_HIP_CHECK(hipMemsetAsync(p->out, 0, out_bytes, ctx->stream)); }
            else { std::memset(p->out, 0, out_bytes); }
        }
        return LRHIP_OK;
    }
    GatherLaunch q{};
    q.mask = lrd::kFeatGather | lrd::kFeatQuery | lrd::kFeatSceneMask | (ctx->features & lrd::kFeatNest) |
             (ctx->scene.sampler_kind != LR_SAMPLER_INDEPENDENT ? lrd::kFeatGeneric : 0u);
    q.ck = chunking_of(p->spp_end - p->spp_begin, static_cast<double>((p->count + 63u) / 64u), 1.25, true);
    q.spp_begin = p->spp_begin, q.spp_end = p->spp_end;
    q.clamp = p->clamp > 0.f ? p->clamp : ctx->scene.film_clamp;
    return staged_call(ctx, ctx->gather_timer, p->count, device_pointers,
                       {Column{p->out, sizeof(float4), accumulate ? kColumnInOut : kColumnClear}, column_in(p->streams, sizeof(uint32_t)),
                        column_in(p->records, points ? sizeof(float4) : sizeof(lrhip_ray_hit)), column_in(normals, sizeof(float4))},
                       [&](uint32_t n, uint64_t first, void *const *d) { return launch_gather(ctx, q, d[2], d[3], d[1], d[0], n, static_cast<uint32_t>(first)); });
}

int lrhip_query_gather_vertex(lrhip_ctx *ctx, const lrhip_gather_vertex_params *p) {
    if (auto r = screen("lrhip_query_gather_vertex", ctx, p, LRHIP_RAY_DEVICE_POINTERS | LRHIP_GATHER_FROM_POINTS, "records"); r != LRHIP_OK) { return r; }
    const std::string what{"lrhip_query_gather_vertex: "};
    const auto points = (p->flags & LRHIP_GATHER_FROM_POINTS) != 0u;
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    const auto normals = points ? p->normals : nullptr;// what the mode does not read is not looked at
    if (p->count != 0u) {
        if (p->records == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, what + "records / out is NULL"); }
        if (points && normals == nullptr) { return fail(LRHIP_ERROR_INVALID, what + "normals is NULL with LRHIP_GATHER_FROM_POINTS"); }
        if (device_pointers && misaligned({{p->records, 15u}, {normals, 15u}, {p->out, 15u}, {p->streams, 3u}})) {
            return fail(LRHIP_ERROR_INVALID, what + "device pointers must be 16-byte aligned (streams: 4-byte)");
        }
    }
    if ((ctx->features & (lrd::kFeatAux | lrd::kFeatVpt | lrd::kFeatAov)) != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, what + "the uploaded scene's integrator is not MegaPath");
    }
    if (ctx->scene.sampler_kind == LR_SAMPLER_PADDED_SOBOL && ctx->scene.sampler_spp == 0u) {
        return fail(LRHIP_ERROR_INVALID, what + "the scene's PaddedSobol sampler has a permutation of length 0 (sampler.spp)");
    }
    if (auto r = timer_start(ctx, ctx->gather_timer, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    const auto generic = ctx->scene.sampler_kind != LR_SAMPLER_INDEPENDENT;
    return staged_call(ctx, ctx->gather_timer, p->count, device_pointers,
                       {column_out(p->out, sizeof(lrhip_gather_vertex)), column_in(p->streams, sizeof(uint32_t)),
                        column_in(p->records, points ? sizeof(float4) : sizeof(lrhip_ray_hit)), column_in(normals, sizeof(float4))},
                       [&](uint32_t n, uint64_t first, void *const *d) {
        if (auto r = resident_meshes(ctx); r != LRHIP_OK) { return r; }
        lrd::GatherArgs args{};
        fill_hit_table(ctx, args, d[2], nullptr, n);
        args.out = static_cast<float4 *>(d[0]), args.streams = static_cast<const uint32_t *>(d[1]), args.normals = static_cast<const float4 *>(d[3]);
        args.stream_base = static_cast<uint32_t>(first), args.sample_index = p->sample_index;
        lrd::DScenePtr device_scene{};
        if (auto r = upload_scene_record(ctx, device_scene); r != LRHIP_OK) { return r; }
        if (auto r = timer_begin(ctx, ctx->gather_timer); r != LRHIP_OK) { return r; }
        const dim3 grid(blocks_of(n)), block(lrd::kBlockThreads);
        if (points) {
            if (generic) { hipLaunchKernelGGL((lrd::gather_vertex_kernel<true, true>), grid, block, 0, ctx->stream, device_scene, args); }
            else { hipLaunchKernelGGL((lrd::gather_vertex_kernel<true, false>), grid, block, 0, ctx->stream, device_scene, args); }
        } else {
            if (generic) { hipLaunchKernelGGL((lrd::gather_vertex_kernel<false, true>), grid, block, 0, ctx->stream, device_scene, args); }
            else { hipLaunchKernelGGL((lrd::gather_vertex_kernel<false, false>), grid, block, 0, ctx->stream, device_scene, args); }
        }
        LR_HIP_CHECK(hipGetLastError());
        return timer_end(ctx, ctx->gather_timer);
    });
}

double lrhip_last_gather_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->gather_timer) : 0.0; }

}// extern "C"
