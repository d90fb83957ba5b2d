// lrhip_radiance.hip — C ABI of the radiance queries (include/lrhip.h: lrhip_trace_radiance, lrhip_last_radiance_ms): MegaPath's
// estimator along caller-supplied rays.  The kernels are the kFeatQuery instantiations of megapath_kernel.h (variants.h: LR_QUERY_LIST), found in
// the kernel table by mask; this file validates the call, stages host pointers, sizes the work items and the grid as lrhip_render does for a
// frame, and launches on the context's stream.
#include "lrhip_internal.h"

namespace lrh {

namespace {

// rays per chunk of a host-pointer call (lrhip_raycast.hip's cap): 32 MiB of rays, 16 MiB of records and 4 MiB of stream ids in the staging buffers
constexpr uint64_t kRadianceChunk = 1ull << 20u;

struct QueryLaunch {
    uint32_t mask;       // the kernel
    Chunking ck;         // sample chunks of an item: a function of the CALL's ray count and sample range, the same for every staged chunk
    uint32_t spp_begin, spp_end;
    float clamp;
    bool count;
};

// one launch over `count` rays in device memory (and, with several sample chunks, the reduce of their partial planes), between the context's
// radiance events.  `stream_base`: the stream id of rays[0] when `streams` is NULL
int launch_device(lrhip_ctx *ctx, const QueryLaunch &q, const void *rays, const void *streams, void *out, uint32_t count, uint32_t stream_base) {
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
    // (`record` is pageable host memory: hipMemcpyAsync has staged it when it returns, as for ctx->scene in lrhip_render -- do not pin it)
    auto record = ctx->scene;
    record.film_clamp = q.clamp, record.shutter_weight = 1.f;
    if (auto r = ensure(ctx->scene_record, sizeof(lrd::DScene)); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemcpyAsync(ctx->scene_record.ptr, &record, sizeof(lrd::DScene), hipMemcpyHostToDevice, ctx->stream));
    LR_HIP_CHECK(hipEventRecord(ctx->radiance_begin, ctx->stream));
    LR_HIP_CHECK(entry->launch(blocks, ctx->stream, static_cast<const lrd::DScene *>(ctx->scene_record.ptr), &args, 0u));
    if (q.ck.count > 1u) { LR_HIP_CHECK(launch_resolve_records(ctx, args.query_out, args.partial, count, q.ck.count)); }
    LR_HIP_CHECK(hipEventRecord(ctx->radiance_end, ctx->stream));
    ctx->radiance_pending = true;
    return LRHIP_OK;
}

// the pending launch's time joins the call's sum (synchronises with it)
int collect_time(lrhip_ctx *ctx) {
    if (!ctx->radiance_pending) { return LRHIP_OK; }
    float ms = 0.f;
    LR_HIP_CHECK(hipEventSynchronize(ctx->radiance_end));
    LR_HIP_CHECK(hipEventElapsedTime(&ms, ctx->radiance_begin, ctx->radiance_end));
    ctx->radiance_ms += static_cast<double>(ms);
    ctx->radiance_pending = false;
    return LRHIP_OK;
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_trace_radiance(lrhip_ctx *ctx, const lrhip_radiance_query_params *p) {
    if (ctx == nullptr || p == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: NULL argument"); }
    if ((p->flags & ~(LRHIP_RAY_DEVICE_POINTERS | LRHIP_RADIANCE_ACCUMULATE | LRHIP_RADIANCE_COUNTERS)) != 0u) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: unknown flags");
    }
    if (p->count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: more than 2^31 - 1 rays"); }
    if (!(p->clamp >= 0.f)) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: the clamp must be positive, or 0 for the scene's"); }
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: no scene uploaded"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    const auto accumulate = (p->flags & LRHIP_RADIANCE_ACCUMULATE) != 0u;
    if (p->count != 0u) {
        if (p->rays == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: rays / out is NULL"); }
        if (device_pointers && (((reinterpret_cast<uintptr_t>(p->rays) | reinterpret_cast<uintptr_t>(p->out)) & 15u) != 0u ||
                                (reinterpret_cast<uintptr_t>(p->streams) & 3u) != 0u)) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_trace_radiance: device pointers must be 16-byte aligned (streams: 4-byte)");
        }
    }
    if ((ctx->features & (lrd::kFeatAux | lrd::kFeatVpt | lrd::kFeatAov)) != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_trace_radiance: the uploaded scene's integrator is not MegaPath");
    }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->radiance_ms = 0.0, ctx->radiance_pending = false;
    if (p->count == 0u) { return LRHIP_OK; }
    const auto out_bytes = static_cast<size_t>(p->count) * sizeof(float4);
    // MegakernelPathTracingInstance::_render_one_camera (mega_path.cpp:40-47) renders nothing for a scene without lights and without an
    // environment, and lrhip_render launches nothing there: the megakernel never runs with no light to sample (its light sampler divides by
    // the light count and indexes the light tables).  The same here: such a scene's records are those of no sample
    const auto no_lighting = !ctx->scene.has_lights && ctx->scene.env_kind == lrd::kEnvNone;
    if (p->spp_begin >= p->spp_end || no_lighting) {// nothing is launched, and a record that is not accumulated into holds the sums of no sample
        if (!accumulate) {
            if (device_pointers) { LR_HIP_CHECK(hipMemsetAsync(p->out, 0, out_bytes, ctx->stream)); }
            else { std::memset(p->out, 0, out_bytes); }
        }
        return LRHIP_OK;
    }
    if (ctx->radiance_begin == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->radiance_begin)); }
    if (ctx->radiance_end == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->radiance_end)); }
    QueryLaunch q{};
    q.count = (p->flags & LRHIP_RADIANCE_COUNTERS) != 0u;
    q.mask = lrd::kFeatQuery | lrd::kFeatSceneMask | (ctx->features & lrd::kFeatNest) | (q.count ? lrd::kFeatCount : 0u) |
             (ctx->scene.sampler_kind != LR_SAMPLER_INDEPENDENT ? lrd::kFeatGeneric : 0u);
    // the work items: (64 consecutive rays, sample chunk), sized by lrhip_render's loss model for a frame of count / 64 tiles -- a function of
    // (count, sample range) only, never of the device, the pointers' kind or the staging chunk
    q.ck = chunking_of(p->spp_end - p->spp_begin, static_cast<double>((p->count + 63u) / 64u), 1.25, true);
    q.spp_begin = p->spp_begin, q.spp_end = p->spp_end;
    q.clamp = p->clamp > 0.f ? p->clamp : ctx->scene.film_clamp;
    if (device_pointers) {
        if (!accumulate) { LR_HIP_CHECK(hipMemsetAsync(p->out, 0, out_bytes, ctx->stream)); }
        return launch_device(ctx, q, p->rays, p->streams, p->out, static_cast<uint32_t>(p->count), 0u);
    }
    // host pointers: chunk by chunk through the staging buffers
    const auto chunk = std::min<uint64_t>(p->count, kRadianceChunk);
    if (auto r = ensure(ctx->raycast_rays, chunk * sizeof(lrhip_ray)); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->radiance_out, chunk * sizeof(float4)); r != LRHIP_OK) { return r; }
    if (p->streams != nullptr) {
        if (auto r = ensure(ctx->radiance_streams, chunk * sizeof(uint32_t)); r != LRHIP_OK) { return r; }
    }
    for (uint64_t first = 0u; first < p->count; first += chunk) {
        const auto n = std::min<uint64_t>(chunk, p->count - first);
        const auto host_out = static_cast<char *>(p->out) + first * sizeof(float4);
        LR_HIP_CHECK(hipMemcpyAsync(ctx->raycast_rays.ptr, static_cast<const lrhip_ray *>(p->rays) + first, n * sizeof(lrhip_ray),
                                    hipMemcpyHostToDevice, ctx->stream));
        if (p->streams != nullptr) {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->radiance_streams.ptr, static_cast<const uint32_t *>(p->streams) + first, n * sizeof(uint32_t),
                                        hipMemcpyHostToDevice, ctx->stream));
        }
        if (accumulate) { LR_HIP_CHECK(hipMemcpyAsync(ctx->radiance_out.ptr, host_out, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream)); }
        else { LR_HIP_CHECK(hipMemsetAsync(ctx->radiance_out.ptr, 0, n * sizeof(float4), ctx->stream)); }
        if (auto r = launch_device(ctx, q, ctx->raycast_rays.ptr, p->streams != nullptr ? ctx->radiance_streams.ptr : nullptr,
                                   ctx->radiance_out.ptr, static_cast<uint32_t>(n), static_cast<uint32_t>(first)); r != LRHIP_OK) {
            return r;
        }
        LR_HIP_CHECK(hipMemcpyAsync(host_out, ctx->radiance_out.ptr, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = collect_time(ctx); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

double lrhip_last_radiance_ms(lrhip_ctx *ctx) {
    if (ctx == nullptr) { return 0.0; }
    if (hipSetDevice(ctx->device) != hipSuccess || collect_time(ctx) != LRHIP_OK) { return -1.0; }
    return ctx->radiance_ms;
}

}// extern "C"
