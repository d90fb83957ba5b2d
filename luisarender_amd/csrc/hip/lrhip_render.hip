// lrhip_render.hip — lrhip_render: the work items of a launch, the fixed-point film, the scheduler's rule and the launch of the
// one-path-per-lane, pool and AOV kernels (wavefront mode: lrhip_wavefront.hip).  Which kernels: lrhip_kernels.hip, plan_kernels.
#include "lrhip_internal.h"

namespace lrh {

// Work items of a launch over `spp` samples per pixel of a shard with `shard_tiles` tiles (dev_scene.h: RenderArgs / item_range).
// Two losses are balanced.  The drain at the end of every item -- its last paths finish with most lanes idle -- is a share of
// ~a / S of an item of S samples per pixel; the tail of the launch -- waves out of items while the last ones finish -- is
// ~S_last * waves / (2 * spp * tiles).  With uniform items both depend on the same S and the optimum is S = sqrt(2a * spp * tiles /
// waves) (a = 0.625 from sweeps, rounds 1-2).  Round 3: the items TAPER -- the first ~90 % of the samples go out in items 2.5x that
// size, the rest in items a third of it, and all big items are handed out before the first small one: the bulk drains rarely, the
// end of the launch is made of short items.  C2 at 1024 spp, full frame / 1-of-8 shard: uniform 1213.5 / 164.5 ms, tapered 1197.5 /
// 158.0 ms (kernel-level strong-scaling efficiency at 8 shards 0.922 -> 0.947); big factor 2 / 2.5 / 3.5 / 4, small divisor 2 / 3 /
// 4 / 5 and fractions 0.75 / 0.85 / 0.9 were swept (profiles/archive/r03p_taper_sweep.txt).  The partition is a function of (spp,
// shard_tiles, scale) only -- never of the device or of the tile range of the call -- so films stay bit-identical under any sharding with
// the same balance_shards.
#ifndef LR_TAPER_BIG
#define LR_TAPER_BIG 2.5
#endif
#ifndef LR_TAPER_SMALL
#define LR_TAPER_SMALL 3.0
#endif
#ifndef LR_TAPER_FRACTION
#define LR_TAPER_FRACTION 0.9
#endif
Chunking chunking_of(uint32_t spp, double shard_tiles, double item_scale, bool taper) {
    const auto s_opt = std::max(1.0, std::sqrt(item_scale * spp * shard_tiles / kNominalWaves));
    Chunking c{};
    if (taper && spp >= 16u) {
        // (the partial planes bound the chunk count: at most half of them for the big items, the rest for the small ones)
        const auto big_min = static_cast<long>((static_cast<uint64_t>(spp) * 2u + kMaxChunks - 1u) / kMaxChunks);
        c.big = static_cast<uint32_t>(std::clamp(std::max(std::lround(LR_TAPER_BIG * s_opt), big_min), 1l, static_cast<long>(spp)));
        c.small = static_cast<uint32_t>(std::clamp(std::lround(s_opt / LR_TAPER_SMALL), 1l, static_cast<long>(c.big)));
        c.big_count = static_cast<uint32_t>(std::floor(LR_TAPER_FRACTION * spp / c.big));
        const auto rest = spp - c.big_count * c.big;
        auto small_count = (rest + c.small - 1u) / c.small;
        if (c.big_count + small_count > kMaxChunks && c.big_count < kMaxChunks) {// (few tiles and many samples: what fits the partial planes)
            c.small = (rest + (kMaxChunks - c.big_count) - 1u) / (kMaxChunks - c.big_count);
            small_count = (rest + c.small - 1u) / c.small;
        }
        c.count = c.big_count + small_count;
        if (c.big_count >= 1u && small_count >= 1u && c.count <= kMaxChunks) { return c; }
    }
    auto count = static_cast<uint32_t>(std::lround(spp / s_opt));
    count = std::max(1u, std::min({count, spp, kMaxChunks}));
    c.count = c.big_count = count, c.big = (spp + count - 1u) / count, c.small = c.big;
    return c;
}

// ---- fixed-point film sums (dev_wavefront.h: radiance_to_fixed; the pool kernels of round 4 and the parked paths of wavefront
// mode).  One sample adds at most clamp x |shutter weight| per channel and a pixel takes at most `spp` of them in one lrhip_render; the
// scale is the largest power of two that keeps that sum below 2^61, at most 2^40 (1e-12 of absolute resolution).  Returns log2 of the
// scale, or -1 when fewer than kMinFixedBits fractional bits would be left -- a clamp used to switch clamping off (1e20, inf): such a
// film cannot be held in 64-bit fixed point, and lrhip_render takes the float-accumulating kernels of rounds 1-3 instead.
constexpr int kMinFixedBits = 24;
int fixed_point_bits(float film_clamp, float shutter_weight, uint32_t spp) {
    const auto bound = std::max(1.0, static_cast<double>(film_clamp) * std::max(1.0,
        std::fabs(static_cast<double>(shutter_weight)))) * std::max(1u, spp);
    if (!std::isfinite(bound)) { return -1; }
    const auto bits = std::min(40, 61 - static_cast<int>(std::ceil(std::log2(bound))));
    return bits >= kMinFixedBits ? bits : -1;
}
// the frame's fixed-point sums [pixel][rgb], zero between renders (wf_resolve_kernel clears what it adds to the film)
int ensure_accum(lrhip_ctx *ctx, uint32_t pixel_count) {
    const auto bytes = static_cast<size_t>(pixel_count) * 3u * sizeof(unsigned long long);
    if (ctx->wf_accum.bytes < bytes) {
        if (auto r = ensure(ctx->wf_accum, bytes); r != LRHIP_OK) { return r; }
        LR_HIP_CHECK(hipMemsetAsync(ctx->wf_accum.ptr, 0, bytes, ctx->stream));
    }
    return LRHIP_OK;
}
// Which scheduler a frame of this scene runs under (lrhip_set_scheduler).  Automatic: the pool kernels, except on scenes so small that
// a ray is a handful of traversal steps -- there the pool kernel's costlier shading block (path state through global memory, the
// current context through the LDS) is not paid back by fuller traversal steps.  Measured in round 4 at the bench's scenes (kernel
// time, one path per lane / pool, profiles/r04_final_schedulers.txt): Cornell box, 32 triangles, 0.88; C2 1.5 M triangles 1.08 (1024
// spp) ... 1.12 (256 spp); C3 1.18; C4 1.06; C5 (wavefront mode) 1.10.
// A room scene swept over its triangle count (profiles/archive/r04i_scheduler_crossover.txt): 0.88 at 2-5 thousand triangles, 0.93 at 12,
// 0.96 at 30, 1.06 at 100, 1.20 at 400 thousand.
// Round 5 (tools/sched_sweep.py, profiles/r05j_scheduler_sweep.txt: the room scene over its triangle count x path depth x spp, the Cornell
// box over depth x spp): what the pool buys grows with the LENGTH of the walks (triangles) and of the paths (depth) and with the share of
// a launch that is drain (few samples per pixel); the break-even moves from ~30 thousand triangles (depth 16, 16 spp) to ~100 thousand
// (depth 16, 256 spp), ~130 (depth 4, 16 spp) and ~180 (depth 4, 256 spp).  The rule follows it with the SCENE's own numbers -- its BVH
// triangles, its integrator's depth, the spp its description asks for (not the spp of this call: every call of a frame must take the
// same kernel family, whose film sums differ in their last bits) -- and is never more than 1.4 % off the better kernel in that sweep
// (the triangle count alone: 3.8 %).
constexpr uint32_t kPoolAutoTriangles = 98304u;
uint32_t pool_auto_triangles(uint32_t max_depth, uint32_t scene_spp) {
    auto t = kPoolAutoTriangles;
    if (max_depth <= 6u) { t *= 2u; }
    if (scene_spp != 0u && scene_spp < 64u) { t /= 2u; }
    return t;
}
bool wants_pool(const lrhip_ctx *ctx) {
    return ctx->scheduler == 2u || (ctx->scheduler == 0u && ctx->update_counts[1] >= pool_auto_triangles(ctx->scene.max_depth,
        ctx->scene.sampler_spp));
}
// path state of the pool kernels: two contexts per thread, 4 (Independent sampler) | 5 float4 each and one more for the ids of a path
// whose last shadow ray rides with the next one (LR_POOL_SHADOW_RIDE), [context][quad][thread] (megapool_kernel.h); sized for 6.  Behind the
// records, every wave's stash of started paths (LR_POOL_PATH_STASH): kPoolStashEntries entries of kPoolStashQuads float4, [wave][quad][entry]
int ensure_pool(lrhip_ctx *ctx, uint32_t resident_blocks) {
    return ensure(ctx->pool, static_cast<size_t>(resident_blocks) * lrd::kWavesPerBlock
        * (lrd::kPoolSlots * lrd::kPoolRecordQuadsMax + lrd::kPoolStashEntries * lrd::kPoolStashQuads) * sizeof(float4));
}

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_render(lrhip_ctx *ctx, const lrhip_render_params *p) {
    if (ctx == nullptr || p == nullptr || !ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_render: no scene uploaded"); }
    auto tiles_x = (ctx->width + 7u) / 8u, tiles_y = (ctx->height + 7u) / 8u;
    auto tile_count = tiles_x * tiles_y;
    if (p->spp_end < p->spp_begin || p->tile_stride == 0u || p->tile_end > tile_count) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_render: invalid spp/tile range");
    }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->timed = false;
    if (p->spp_end == p->spp_begin || p->tile_begin >= p->tile_end) { return LRHIP_OK; }// (rank >= tile count: an empty shard)
    // MegakernelPathTracingInstance::_render_one_camera (mega_path.cpp:40-47): no lights -> nothing rendered
    // (the normal visualiser needs no light: normal.cpp has no such check)
    if (!ctx->scene.has_lights && ctx->scene.env_kind == lrd::kEnvNone && ctx->scene.integrator_kind != LR_INTEGRATOR_NORMAL) {
        return LRHIP_OK;
    }
    auto tiles_in_range = (p->tile_end - p->tile_begin + p->tile_stride - 1u) / p->tile_stride;
    auto spp = p->spp_end - p->spp_begin;
    const auto weight = (p->flags & LRHIP_RENDER_SHUTTER_WEIGHT) != 0u ? p->shutter_weight : 1.f;
    const auto fixed_bits = fixed_point_bits(ctx->scene.film_clamp, weight, spp);
    // which kernels (lrhip_kernels.hip: plan_kernels decides, nothing here restates a condition of it)
    PlanInputs in{};
    in.features = ctx->features, in.force_features = ctx->diag_force_features, in.sampler_kind = ctx->scene.sampler_kind;
    in.wf_mode = ctx->wf_mode, in.max_depth = ctx->scene.max_depth;
    in.count = (p->flags & LRHIP_RENDER_COUNTERS) != 0u, in.env_tree = ctx->env_tree, in.byte_texels = ctx->packed_texel_words != 0u;
    in.wants_pool = wants_pool(ctx), in.fixed_fits = fixed_bits >= 0;
    // A call whose sums do not fit the fixed-point film as a whole (clamp x spp beyond 2^37: a clamp of 1e7 at 65536 spp) is rendered in sample
    // sub-ranges that do, one resolve into the float film per range, instead of silently leaving wavefront mode and the pool kernels for the
    // all-in-one variants (the kitchen class runs at ~300 instead of ~560 Msamples/s there).  Only a clamp that does not even
    // hold ONE sample (switched off: 1e20, inf) still takes the float-accumulating kernels -- lrhip.h says so.
    // (Only where the frame WOULD be summed in fixed point if it fitted -- wavefront mode or a pool kernel: the float-accumulating kernels
    // render such a call in one launch as before, in their usual order of adds.  ADVICE r05.)
    if (fixed_bits < 0 && !ctx->in_split && fixed_point_bits(ctx->scene.film_clamp, weight, 1u) >= 0) {
        auto fitting = in;
        fitting.fixed_fits = true;
        if (plan_kernels(fitting).fixed_point) {
            auto n = spp;
            while (n > 1u && fixed_point_bits(ctx->scene.film_clamp, weight, n) < 0) { n = (n + 1u) / 2u; }
            LR_HIP_CHECK(hipEventRecord(ctx->ev_begin, ctx->stream));// (before the flag: a failure here must not leave it set)
            struct SplitGuard {
                lrhip_ctx *c;
                ~SplitGuard() { c->in_split = false; }
            } guard{ctx};
            ctx->in_split = true;
            auto rc = LRHIP_OK;
            for (auto s0 = p->spp_begin; s0 < p->spp_end && rc == LRHIP_OK; s0 += n) {
                auto sub = *p;
                sub.spp_begin = s0, sub.spp_end = std::min(p->spp_end, s0 + n);
                rc = lrhip_render(ctx, &sub);
            }
            return rc;
        }
    }
    const auto plan = plan_kernels(in);
    if (plan.family == LRHIP_FAMILY_WAVEFRONT) { return render_wavefront(ctx, p, plan, tiles_x, tiles_y, tiles_in_range, tile_count); }
    // Chunking (chunking_of above: tapered items) is a function of the frame only (tile_count, spp, balance_shards), never of the device
    // or the tile range of this call: tile_count is that of ONE shard of the frame as the caller declares it (balance_shards), so that
    // every shard of a frame -- and the unsharded frame rendered with the same hint -- uses the same chunking.  (Uniform items, rounds
    // 1-2, C2 at 1024 spp: full frame 7 / 14 / 28 chunks -> 1992 / 1987 / 1987 ms; the 1/8 shard 14 / 28 / 56 / 64 chunks -> 305 / 271 / 266 / 265 ms.)
    auto shard_tiles = static_cast<double>(tile_count) / std::max(p->balance_shards, 1u);
    auto item_scale = 1.25;
    // lrhip_set_diagnostics: sweep of the loss model's constant (< 0: uniform items)
    if (ctx->diag_item_scale != 0.) { item_scale *= std::max(0.01, std::fabs(ctx->diag_item_scale)); }
    const auto ck = chunking_of(spp, shard_tiles, item_scale, ctx->diag_item_scale >= 0.);
    const auto chunk_count = ck.count;
    lrd::RenderArgs args{};
    args.film = ctx->film;
    ctx->scene.shutter_weight = weight;
    args.spp_begin = p->spp_begin, args.spp_end = p->spp_end;
    args.tile_begin = p->tile_begin, args.tile_end = p->tile_end, args.tile_stride = p->tile_stride;
    args.tiles_x = tiles_x, args.tiles_y = tiles_y;
    args.chunk_count = chunk_count;
    args.chunk_big_count = ck.big_count, args.chunk_big = ck.big, args.chunk_small = ck.small;
    args.item_count = tiles_in_range * chunk_count;
    args.work_counter = static_cast<uint32_t *>(ctx->work_counter.ptr);
    args.spill = static_cast<uint32_t *>(ctx->spill.ptr);
    args.counters = static_cast<lrd::DCounters *>(ctx->counters.ptr);
    auto pixel_count = ctx->width * ctx->height;
    LR_HIP_CHECK(hipMemsetAsync(ctx->work_counter.ptr, 0, 1024u, ctx->stream));
    const auto aov = plan.family == LRHIP_FAMILY_AOV, pool = plan.family == LRHIP_FAMILY_POOL;
    const auto entry = plan.family != LRHIP_FAMILY_NONE ? find_kernel(plan.main) : nullptr;
    if (entry == nullptr) {
        if (aov) {
            return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_render: no AOV kernel for feature mask " + std::to_string(plan.main)
                + " was compiled into this library");
        }
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_render: no megakernel variant for feature mask " + std::to_string(ctx->features) +
                                                 " was compiled into this library");
    }
    // the AOV kernels keep the wave tiles of the enabled channels in dynamic LDS; when the launch has several chunks, the AOV partial planes are
    // resolved in chunk order like the film's -- bit-reproducible run to run and under any tile sharding with the same balance_shards.  The film
    // is not touched (aov.cpp accumulates none).
    const auto aov_channels = aov ? ctx->scene.aov_channels : 0u;
    const auto lds_bytes = static_cast<unsigned>(lrd::kWavesPerBlock * 64u * aov_channels * sizeof(float));
    uint32_t blocks_per_cu = 0u;
    if (auto r = kernel_blocks(ctx, *entry, lds_bytes, blocks_per_cu); r != LRHIP_OK) { return r; }
    auto resident = ctx->cu_count * blocks_per_cu;
    args.total_threads = resident * lrd::kBlockThreads;
    if (chunk_count > 1u && !pool) {// (the pool kernels add every item to the frame's fixed-point sums: no partial planes)
        if (auto r = ensure(ctx->partial, static_cast<size_t>(chunk_count) * pixel_count * sizeof(float4)); r != LRHIP_OK) { return r; }
        args.partial = static_cast<float4 *>(ctx->partial.ptr);
        if (aov_channels != 0u) {
            if (auto r = ensure(ctx->aov_partial, static_cast<size_t>(chunk_count) * aov_channels * pixel_count * sizeof(float));
                    r != LRHIP_OK) {
                return r;
            }
        }
    }
    if (aov) { ctx->scene.aov_partial = chunk_count > 1u && aov_channels != 0u ? static_cast<float *>(ctx->aov_partial.ptr) : nullptr; }
    auto blocks = std::min(resident, (args.item_count + 3u) / 4u);
    if (pool) {
        if (auto r = ensure_pool(ctx, resident); r != LRHIP_OK) { return r; }
        args.pool = static_cast<float4 *>(ctx->pool.ptr);
        // the frame's fixed-point sums (megapool_kernel.h: FILM)
        if (auto r = ensure_accum(ctx, pixel_count); r != LRHIP_OK) { return r; }
        ctx->scene.wf.accum = static_cast<unsigned long long *>(ctx->wf_accum.ptr);
        ctx->scene.wf.accum_scale = static_cast<float>(std::ldexp(1.0, fixed_bits));
    }
    // how this launch's kernel counts its samples, set on EVERY path (the field lives in ctx->scene and used to keep whatever the
    // last pool / wavefront call left in it): a pool kernel counts an item's samples when its wave leaves the item, the others where they finish
    ctx->scene.wf.count_at_flush = pool ? 1u : 0u;
    // the scene record of THIS launch (shutter weight, film clamp, ...) in stream order
    lrd::DScenePtr device_scene{};
    if (auto r = upload_scene_record(ctx, device_scene); r != LRHIP_OK) { return r; }
    if (!ctx->in_split) { LR_HIP_CHECK(hipEventRecord(ctx->ev_begin, ctx->stream)); }
    LR_HIP_CHECK(entry->launch(blocks, ctx->stream, (const lrd::DScene *)device_scene, &args, lds_bytes));
    ctx->last_variant = entry->mask;
    LR_HIP_CHECK(hipGetLastError());
    LR_HIP_CHECK(hipEventRecord(ctx->ev_end, ctx->stream));
    ctx->timed = true;
    if (pool) {// the frame's fixed-point sums join the film (and are cleared for the next call)
        LR_HIP_CHECK(launch_wf_resolve(ctx, std::ldexp(1.0, -fixed_bits)));
    } else if (aov) {
        if (chunk_count > 1u && aov_channels != 0u) {
            LR_HIP_CHECK(launch_resolve_aov_partial(ctx, chunk_count, tiles_x, p->tile_begin, p->tile_end, p->tile_stride));
        }
    } else if (chunk_count > 1u) {
        LR_HIP_CHECK(launch_resolve_partial(ctx, args.partial, chunk_count, tiles_x, p->tile_begin, p->tile_end, p->tile_stride));
    }
    return LRHIP_OK;
}

uint32_t lrhip_pool_auto_triangles(uint32_t max_depth, uint32_t scene_spp) { return pool_auto_triangles(max_depth, scene_spp); }

int lrhip_work_items(uint32_t width, uint32_t height, uint32_t spp, uint32_t balance_shards, uint32_t out[4]) {
    if (out == nullptr || width == 0u || height == 0u || spp == 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_work_items: invalid argument"); }
    const auto tile_count = ((width + 7u) / 8u) * ((height + 7u) / 8u);
    const auto c = chunking_of(spp, static_cast<double>(tile_count) / std::max(balance_shards, 1u), 1.25, true);
    out[0] = c.count, out[1] = c.big_count, out[2] = c.big, out[3] = c.small;
    return LRHIP_OK;
}


}// extern "C"
