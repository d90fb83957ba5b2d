// lrhip_wavefront.hip — the host loop of wavefront mode.
#include "lrhip_internal.h"

namespace lrh {

// ---- wavefront mode (dev_scene.h: WfArgs): a scene with Mix or Layered surfaces under the MegaPath integrator.  The frame is cut
// into SLICES of the sample range whose paths fit the queues (a path is parked at most once per round, so a queue never needs more
// slots than the slice has paths); per slice: the camera pass of the lean megakernel <.. | Wf> (its own work items, chunked by the
// same loss model as the plain megakernel), then up to max_depth ROUNDS of { heavy kernel -> continuation pass <.. | Wf | Cont> }.
// Nothing comes back to the host in between: the kernels read their record counts from device memory and the grids are the
// persistent ones (an empty round costs a few microseconds), so a slice is one uninterrupted stretch of the stream.
// `plan`: the camera pass, the continuation pass and the three heavy kernels (lrhip_kernels.hip: plan_kernels).
int render_wavefront(lrhip_ctx *ctx, const lrhip_render_params *p, const KernelPlan &plan, uint32_t tiles_x, uint32_t tiles_y,
                     uint32_t tiles_in_range, uint32_t tile_count) {
    // (lrhip_upload_scene packs no scene that renders in wavefront mode: its lean passes hold no 8-bit texel decode)
    if (ctx->packed_texel_words != 0u) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_render: wavefront mode with 8-bit texels on the device (lrhip_set_texture_storage)");
    }
    const auto spp = p->spp_end - p->spp_begin;
    const auto pixel_count = ctx->width * ctx->height;
    const auto sampler_words = (plan.main & lrd::kFeatGeneric) != 0u ? lrd::kWfSamplerWordsMax : 1u;
    // Slice size: every slice pays the latency of its last rounds (a handful of paths, one batch each), so slices are large -- C5 at
    // 512 spp: 356 / 404 / 442 / 472 Msamples/s with 2^25 / 2^26 / 2^27 / ~2^27.9 paths per slice.  A slice is 2^28 paths of ONE NOMINAL
    // SHARD of the frame (tile_count / balance_shards tiles, like the chunking): its length in samples is a function of the frame and
    // the caller's hint only -- never of the free memory or of the tile range of this call -- because the work items, and with
    // them the order of the film's float sums, are cut per slice: every shard of a frame, and the unsharded frame rendered with the
    // same hint, must cut them alike.  A path takes (3 queues x 15..18 words + 26..29 words) x 4 B = 284 .. 332 B: 2^28 of them are
    // 76 .. 89 GB of the 288.  What the memory does decide is how many TILES go through the queues at a time (tile groups, below):
    // a call over more tiles than fit -- the unsharded frame with a shard hint, a GPU with little memory left -- takes its tiles
    // group after group with the same slices, which regroups nothing (items are per tile; parked paths add in fixed point).
    const auto nominal_paths = ctx->wf_slice_paths != 0u ? static_cast<uint64_t>(ctx->wf_slice_paths) : (1ull << 28u);
    const auto nominal_tiles = std::max<uint64_t>(1u, static_cast<uint64_t>(static_cast<double>(tile_count) / std::max(p->balance_shards,
        1u) + 0.5));
    const auto slice_spp = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(spp, nominal_paths / (nominal_tiles * 64u))));
    const auto per_path = static_cast<uint64_t>(lrd::kWfKinds * (lrd::kWfHeavyWords + sampler_words) + lrd::kWfContWords
        + sampler_words) * sizeof(uint32_t);
    size_t free_bytes = 0u, total_bytes = 0u;
    LR_HIP_CHECK(hipMemGetInfo(&free_bytes, &total_bytes));
    const auto have = free_bytes + ctx->wf_heavy.bytes + ctx->wf_cont.bytes;// (the queues of an earlier call count as free)
    // at most half of what is free, and at most kWfQueueBudget: the 2^28-path default slice needs 86-100 GB with its hand-over margin,
    // more buys nothing
    auto fit_paths = std::min<uint64_t>(1ull << 30u,// (dev_wavefront.h: a slot's byte offset inside a queue column is 32 bits)
                                         std::max<uint64_t>(1ull << 16u, std::min<uint64_t>(have / 2u, kWfQueueBudget) / per_path));
    // (tests: the slots of eight tiles, i.e. seven at a time with the margin below)
    if (ctx->wf_mode == 2u) { fit_paths = 8ull * 64u * slice_spp; }
    // (round 6: the queues hold an eighth more than a slice's own paths -- room for what the slice before handed over, film_kernels.h:
    // wf_carry_kernel)
    const auto group_tiles = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(tiles_in_range,
        fit_paths * 8u / 9u / (64ull * slice_spp))));
    const auto slice_paths = std::min<uint64_t>(static_cast<uint64_t>(group_tiles) * 64u * slice_spp, (1ull << 30u) * 8u / 9u);
    const auto carry_margin = static_cast<uint32_t>(slice_paths / 8u);
    const auto capacity = static_cast<uint32_t>(slice_paths + carry_margin);
    const auto heavy_words = static_cast<size_t>(lrd::kWfKinds) * (lrd::kWfHeavyWords + sampler_words) * capacity;
    const auto cont_words = static_cast<size_t>(lrd::kWfContWords + sampler_words) * capacity;
    if (auto r = ensure(ctx->wf_heavy, heavy_words * sizeof(uint32_t)); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->wf_cont, cont_words * sizeof(uint32_t)); r != LRHIP_OK) { return r; }
    if (ctx->wf_counts.ptr == nullptr) {
        if (auto r = ensure(ctx->wf_counts, lrd::kWfCounterBufferWords * sizeof(uint32_t)); r != LRHIP_OK) { return r; }
    }
    if (auto r = ensure_accum(ctx, pixel_count); r != LRHIP_OK) { return r; }
    auto &scene = ctx->scene;
    scene.shutter_weight = (p->flags & LRHIP_RENDER_SHUTTER_WEIGHT) != 0u ? p->shutter_weight : 1.f;
    const auto scale_log2 = fixed_point_bits(scene.film_clamp, scene.shutter_weight, spp);// (>= kMinFixedBits: lrhip_render checked)
    const auto accum_scale = std::ldexp(1.0, scale_log2);
    scene.wf.heavy = static_cast<uint32_t *>(ctx->wf_heavy.ptr), scene.wf.cont = static_cast<uint32_t *>(ctx->wf_cont.ptr);
    scene.wf.counts = static_cast<uint32_t *>(ctx->wf_counts.ptr), scene.wf.capacity = capacity;
    scene.wf.accum = static_cast<unsigned long long *>(ctx->wf_accum.ptr), scene.wf.accum_scale = static_cast<float>(accum_scale);
    // the plan's kernels in this library, and how many blocks of each a CU holds
    const auto e_camera = find_kernel(plan.main), e_cont = find_kernel(plan.cont);
    const KernelEntry *e_heavy[lrd::kWfKinds];
    auto heavy_ok = true;
    for (auto k = 0u; k < lrd::kWfKinds; k++) { heavy_ok = (e_heavy[k] = find_kernel(plan.heavy[k], true)) != nullptr && heavy_ok; }
    if (e_camera == nullptr || e_cont == nullptr || !heavy_ok) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_render: the wavefront kernels for feature mask " + std::to_string(ctx->features) +
                                                 " were not compiled into this library");
    }
    const auto pool = (plan.main & lrd::kFeatPool) != 0u;// round 4: both lean passes under the path-pool scheduler (megapool_kernel.h)
    scene.wf.count_at_flush = pool ? 1u : 0u;
    const auto pool_film = pool;// the camera pass sums its tiles into the frame's fixed-point sums: no partial planes
    uint32_t b_camera = 0u, b_cont = 0u, b_heavy[lrd::kWfKinds] = {0u, 0u, 0u};
    if (auto r = kernel_blocks(ctx, *e_camera, 0u, b_camera); r != LRHIP_OK) { return r; }
    if (auto r = kernel_blocks(ctx, *e_cont, 0u, b_cont); r != LRHIP_OK) { return r; }
    for (auto k = 0u; k < lrd::kWfKinds; k++) {
        if (auto r = kernel_blocks(ctx, *e_heavy[k], 0u, b_heavy[k]); r != LRHIP_OK) { return r; }
    }
    // which closure kinds the scene holds at all (a Mix / Layered surface may reach a Disney child, which is shaded inside that kind's kernel)
    const bool has_kind[lrd::kWfKinds] = {(ctx->features & lrd::kFeatDisney) != 0u, (ctx->features & lrd::kFeatMix) != 0u,
        (ctx->features & lrd::kFeatLayered) != 0u};
    const auto resident = ctx->cu_count * std::max(b_camera, b_cont);
    if (auto r = ensure(ctx->spill, static_cast<size_t>(resident) * lrd::kBlockThreads * lrd::kSpillEntries * sizeof(uint32_t)); r != LRHIP_OK) {
        return r;
    }
    if (pool) {
        if (auto r = ensure_pool(ctx, resident); r != LRHIP_OK) { return r; }
    }
    if (auto r = ensure(ctx->scene_record, sizeof(lrd::DScene)); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemcpyAsync(ctx->scene_record.ptr, &scene, sizeof(lrd::DScene), hipMemcpyHostToDevice, ctx->stream));
    const auto device_scene = static_cast<const lrd::DScene *>(ctx->scene_record.ptr);
    lrd::RenderArgs args{};
    args.film = ctx->film;
    args.tile_begin = p->tile_begin, args.tile_end = p->tile_end, args.tile_stride = p->tile_stride;
    args.tiles_x = tiles_x, args.tiles_y = tiles_y;
    args.work_counter = static_cast<uint32_t *>(ctx->work_counter.ptr);
    args.spill = static_cast<uint32_t *>(ctx->spill.ptr);
    args.pool = static_cast<float4 *>(ctx->pool.ptr);
    args.counters = static_cast<lrd::DCounters *>(ctx->counters.ptr);
    const auto counts = static_cast<uint32_t *>(ctx->wf_counts.ptr);
    const auto shard_tiles = static_cast<double>(tile_count) / std::max(p->balance_shards, 1u);
    auto item_scale = 1.25;
    if (ctx->diag_item_scale != 0.) { item_scale *= std::max(0.01, std::fabs(ctx->diag_item_scale)); }
    if (!ctx->in_split) { LR_HIP_CHECK(hipEventRecord(ctx->ev_begin, ctx->stream)); }
    LR_HIP_CHECK(hipMemsetAsync(counts, 0, lrd::kWfCounterBufferWords * sizeof(uint32_t), ctx->stream));// (nothing handed over yet)
    // rounds a slice runs before it hands what is still parked over to the next one (the last slice of the call runs them all)
    const auto carry_rounds = ctx->diag_wf_carry_rounds != 0u ? ctx->diag_wf_carry_rounds : kWfCarryRounds;
    for (auto g0 = 0u; g0 < tiles_in_range; g0 += group_tiles) {// tile groups: what fits the queues at a time (see above)
    const auto group_count = std::min(group_tiles, tiles_in_range - g0);
    args.tile_begin = p->tile_begin + g0 * p->tile_stride;
    args.tile_end = std::min(p->tile_end, args.tile_begin + group_count * p->tile_stride);
    for (auto s0 = p->spp_begin; s0 < p->spp_end; s0 += slice_spp) {
        const auto s1 = std::min(p->spp_end, s0 + slice_spp);
        const auto n = s1 - s0;
        // ---- camera pass: samples [s0, s1) of every tile of the shard; heavy hits are parked
        const auto ck = chunking_of(n, shard_tiles, item_scale, ctx->diag_item_scale >= 0.);
        const auto chunk_count = ck.count;
        args.spp_begin = s0, args.spp_end = s1, args.chunk_count = chunk_count, args.item_count = group_count * chunk_count;
        args.chunk_big_count = ck.big_count, args.chunk_big = ck.big, args.chunk_small = ck.small;
        args.total_threads = ctx->cu_count * b_camera * lrd::kBlockThreads;
        if (chunk_count > 1u && !pool_film) {// (the pool kernels add every item to the frame's fixed-point sums: no partial planes)
            if (auto r = ensure(ctx->partial, static_cast<size_t>(chunk_count) * pixel_count * sizeof(float4)); r != LRHIP_OK) { return r; }
            args.partial = static_cast<float4 *>(ctx->partial.ptr);
        }
        const auto last_slice = g0 + group_tiles >= tiles_in_range && s0 + slice_spp >= p->spp_end;
        LR_HIP_CHECK(hipMemsetAsync(ctx->work_counter.ptr, 0, 1024u, ctx->stream));
        LR_HIP_CHECK(hipMemsetAsync(counts, 0, lrd::kWfCounterWords * sizeof(uint32_t), ctx->stream));
        LR_HIP_CHECK(launch_wf_carry(ctx, carry_margin, 1u));// (the paths the slice before handed over)
        LR_HIP_CHECK(e_camera->launch(std::min(ctx->cu_count * b_camera, (args.item_count + 3u) / 4u), ctx->stream, device_scene, &args, 0u));
        if (chunk_count > 1u && !pool_film) {
            LR_HIP_CHECK(launch_resolve_partial(ctx, args.partial, chunk_count, tiles_x, args.tile_begin, args.tile_end, p->tile_stride));
        }
        // ---- rounds: a path leaves a round either finished or parked again (one level deeper), so max_depth rounds empty the queues
        args.chunk_count = 1u, args.item_count = 0u;// (the continuation pass reads its item count from the device)
        args.chunk_big_count = 1u, args.chunk_big = 0u, args.chunk_small = 0u;
        for (auto round = 0u; round < std::max(scene.max_depth, 1u); round++) {
            for (auto k = 0u; k < lrd::kWfKinds; k++) {
                if (has_kind[k]) { LR_HIP_CHECK(e_heavy[k]->launch(ctx->cu_count * b_heavy[k], ctx->stream, device_scene, &args, 0u)); }
            }
            // the heavy kernels have consumed the parked paths: their counters (and work counters) restart for the continuation pass
            LR_HIP_CHECK(hipMemsetAsync(counts + lrd::kWfCountHeavy, 0, 3u * sizeof(uint32_t), ctx->stream));
            LR_HIP_CHECK(hipMemsetAsync(counts + lrd::kWfWorkHeavy, 0, 3u * sizeof(uint32_t), ctx->stream));
            args.total_threads = ctx->cu_count * b_cont * lrd::kBlockThreads;
            LR_HIP_CHECK(e_cont->launch(ctx->cu_count * b_cont, ctx->stream, device_scene, &args, 0u));
            LR_HIP_CHECK(hipMemsetAsync(counts + lrd::kWfCountCont, 0, 2u * sizeof(uint32_t), ctx->stream));// (+ its work counter, next to it)
            if (!last_slice && round + 1u >= carry_rounds && carry_rounds < 0xffffu) {
                LR_HIP_CHECK(launch_wf_carry(ctx, carry_margin, 0u));
            }
        }
    }
    }
    LR_HIP_CHECK(launch_wf_resolve(ctx, 1.0 / accum_scale));
    LR_HIP_CHECK(hipEventRecord(ctx->ev_end, ctx->stream));
    ctx->timed = true;
    // what rendered: the lean camera-pass kernel's mask + the closure bits the heavy kernel served
    ctx->last_variant = e_camera->mask | (ctx->features & (lrd::kFeatDisney | lrd::kFeatMix | lrd::kFeatLayered | lrd::kFeatNest));
    return LRHIP_OK;
}

}// namespace lrh
