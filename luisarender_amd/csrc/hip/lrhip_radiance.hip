// lrhip_radiance.hip — C ABI of the radiance queries (include/lrhip.h: lrhip_trace_radiance, lrhip_last_radiance_ms): MegaPath's
// estimator along caller-supplied rays.  The kernels are the kFeatQuery instantiations of megapath_kernel.h (variants.h: LR_QUERY_LIST), found in
// the kernel table by mask; this file validates the call, stages host pointers, sizes the work items and the grid as lrhip_render does for a
// frame, and launches on the context's stream.
#include "lrhip_internal.h"

namespace lrh {

namespace {

struct RadianceLaunch {
    uint32_t mask;       // the kernel
    Chunking ck;         // sample chunks of an item: a function of the CALL's ray count and sample range, the same for every staged chunk
    uint32_t spp_begin, spp_end;
    float clamp;
    bool count;
};

// one launch over `count` rays in device memory (and, with several sample chunks, the reduce of their partial planes), between the events of
// the context's radiance timer.  `stream_base`: the stream id of rays[0] when `streams` is NULL
int launch_device(lrhip_ctx *ctx, const RadianceLaunch &q, const void *rays, const void *streams, void *out, uint32_t count, uint32_t stream_base) {
    const auto entry = find_kernel(q.mask);
    if (entry == nullptr) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_trace_radiance: no query kernel for feature mask " + std::to_string(q.mask) +
                                                 " was compiled into this library");
    }
    uint32_t blocks_per_cu = 0u;
    if (auto r = kernel_blocks(ctx, *entry, 0u, blocks_per_cu); r != LRHIP_OK) { return r; }
    const auto resident = ctx->cu_count * blocks_per_cu;
    const auto tiles = (count + 63u) / 64u;// items of 64 consecutive rays
    lrd::RenderArgs args{};
    args.spp_begin = q.spp_begin, args.spp_end = q.spp_end;
    args.tile_begin = 0u, args.tile_end = tiles, args.tile_stride = 1u;
    args.tiles_x = tiles, args.tiles_y = 1u;
    args.chunk_count = q.ck.count;
    args.chunk_big_count = q.ck.big_count, args.chunk_big = q.ck.big, args.chunk_small = q.ck.small;
    args.item_count = tiles * q.ck.count;// (count < 2^31, at most kMaxChunks chunks: below 2^31)
    args.work_counter = static_cast<uint32_t *>(ctx->work_counter.ptr);
    args.spill = static_cast<uint32_t *>(ctx->spill.ptr);
    args.counters = static_cast<lrd::DCounters *>(ctx->counters.ptr);
    args.total_threads = resident * lrd::kBlockThreads;
    args.query_rays = static_cast<const float4 *>(rays), args.query_streams = static_cast<const uint32_t *>(streams);
    args.query_out = static_cast<float4 *>(out), args.query_count = count, args.query_stream_base = stream_base;
    // THE BOUND OF THE STACK'S OVERFLOW AREA (lrhip_raycast.hip: trace_device): thread gtid touches words [entry x total_threads + gtid] of it,
    // and lrhip_upload_scene sized it for ctx->grid_blocks blocks
    const auto blocks = std::min(resident, (args.item_count + 3u) / 4u);
    if (resident > ctx->grid_blocks || static_cast<size_t>(args.total_threads) * lrd::kSpillEntries * sizeof(uint32_t) > ctx->spill.bytes) {
        return fail(LRHIP_ERROR_DEVICE, "lrhip_trace_radiance: the grid does not fit the traversal stack's overflow area");
    }
    if (q.ck.count > 1u) {
        if (auto r = ensure(ctx->partial, static_cast<size_t>(q.ck.count) * count * sizeof(float4)); r != LRHIP_OK) { return r; }
        args.partial = static_cast<float4 *>(ctx->partial.ptr);
    }
    LR_HIP_CHECK(hipMemsetAsync(ctx->work_counter.ptr, 0, 1024u, ctx->stream));
    // the scene record of THIS launch: the uploaded scene as the host holds it now, with the query's clamp and a shutter weight of 1 (a copy:
    // lrhip_render's own fields of ctx->scene stay as its last call left them)
    auto record = ctx->scene;
    record.film_clamp = q.clamp, record.shutter_weight = 1.f;
    lrd::DScenePtr device_scene{};
    if (auto r = upload_scene_record(ctx, device_scene, &record); r != LRHIP_OK) { return r; }
    if (auto r = timer_begin(ctx, ctx->radiance_timer); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(entry->launch(blocks, ctx->stream, (const lrd::DScene *)device_scene, &args, 0u));
    if (q.ck.count > 1u) { LR_HIP_CHECK(launch_resolve_records(ctx, args.query_out, args.partial, count, q.ck.count)); }
    return timer_end(ctx, ctx->radiance_timer);
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_trace_radiance(lrhip_ctx *ctx, const lrhip_radiance_query_params *p) {
    if (auto r = screen("lrhip_trace_radiance", ctx, p, LRHIP_RAY_DEVICE_POINTERS | LRHIP_RADIANCE_ACCUMULATE | LRHIP_RADIANCE_COUNTERS, "rays");
        r != LRHIP_OK) { return r; }
    if (!(p->clamp >= 0.f)) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: the clamp must be positive, or 0 for the scene's"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    const auto accumulate = (p->flags & LRHIP_RADIANCE_ACCUMULATE) != 0u;
    if (p->count != 0u) {
        if (p->rays == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: rays / out is NULL"); }
        if (device_pointers && misaligned({{p->rays, 15u}, {p->out, 15u}, {p->streams, 3u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: device pointers must be 16-byte aligned (streams: 4-byte)");
        }
    }
    if ((ctx->features & (lrd::kFeatAux | lrd::kFeatVpt | lrd::kFeatAov)) != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_trace_radiance: the uploaded scene's integrator is not MegaPath");
    }
    // MegakernelPathTracingInstance::_render_one_camera (mega_path.cpp:40-47) renders nothing for a scene without lights and without an
    // environment, and lrhip_render launches nothing there: the megakernel never runs with no light to sample (its light sampler divides by
    // the light count and indexes the light tables).  The same here: such a scene's records are those of no sample
    const auto no_lighting = !ctx->scene.has_lights && ctx->scene.env_kind == lrd::kEnvNone;
    const auto launches = p->count != 0u && p->spp_begin < p->spp_end && !no_lighting;
    if (auto r = timer_start(ctx, ctx->radiance_timer, launches); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    if (!launches) {// a record that is not accumulated into holds the sums of no sample
        const auto out_bytes = static_cast<size_t>(p->count) * sizeof(float4);
        if (!accumulate) {
            if (device_pointers) { LR_HIP_CHECK(hipMemsetAsync(p->out, 0, out_bytes, ctx->stream)); }
            else { std::memset(p->out, 0, out_bytes); }
        }
        return LRHIP_OK;
    }
    RadianceLaunch q{};
    q.count = (p->flags & LRHIP_RADIANCE_COUNTERS) != 0u;
    q.mask = lrd::kFeatQuery | lrd::kFeatSceneMask | (ctx->features & lrd::kFeatNest) | (q.count ? lrd::kFeatCount : 0u) |
             (ctx->scene.sampler_kind != LR_SAMPLER_INDEPENDENT ? lrd::kFeatGeneric : 0u);
    // the work items: (64 consecutive rays, sample chunk), sized by lrhip_render's loss model for a frame of count / 64 tiles -- a function of
    // (count, sample range) only, never of the device, the pointers' kind or the staging chunk
    q.ck = chunking_of(p->spp_end - p->spp_begin, static_cast<double>((p->count + 63u) / 64u), 1.25, true);
    q.spp_begin = p->spp_begin, q.spp_end = p->spp_end;
    q.clamp = p->clamp > 0.f ? p->clamp : ctx->scene.film_clamp;
    return staged_call(ctx, ctx->radiance_timer, p->count, device_pointers,
                       {Column{p->out, sizeof(float4), accumulate ? kColumnInOut : kColumnClear}, column_in(p->rays, sizeof(lrhip_ray)),
                        column_in(p->streams, sizeof(uint32_t))},
                       [&](uint32_t n, uint64_t first, void *const *d) { return launch_device(ctx, q, d[1], d[2], d[0], n, static_cast<uint32_t>(first)); });
}

double lrhip_last_radiance_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->radiance_timer) : 0.0; }

}// extern "C"
