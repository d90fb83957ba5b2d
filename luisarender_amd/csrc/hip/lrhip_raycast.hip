// lrhip_raycast.hip — C ABI of the ray queries (include/lrhip.h: lrhip_trace_rays, lrhip_last_trace_ms).  Holds the two
// instantiations of raycast_kernel.h (alpha test off / on) and their launches on the context's stream.
#include "lrhip_internal.h"
#include "raycast_kernel.h"

static_assert(sizeof(lrhip_ray) == 32u && sizeof(lrd::Ray) == sizeof(lrhip_ray), "a ray is two dwordx4 loads");
static_assert(offsetof(lrhip_ray, t_min) == 12u && offsetof(lrhip_ray, d) == 16u && offsetof(lrhip_ray, t_max) == 28u, "lrhip_ray = lrd::Ray");
static_assert(sizeof(lrhip_ray_hit) == 32u && offsetof(lrhip_ray_hit, inst) == 12u && offsetof(lrhip_ray_hit, reserved) == 24u,
    "a hit record is two dwordx4 stores (raycast_kernel.h: store)");

namespace lrd {
template __global__ void raycast_kernel<false>(DScenePtr, RaycastArgs);
template __global__ void raycast_kernel<true>(DScenePtr, RaycastArgs);
}

namespace lrh {

namespace {

// rays per chunk of a host-pointer call: 32 MiB of rays and at most as much of results in the staging buffers, whatever the count
constexpr uint64_t kRaycastChunk = 1ull << 20u;
#ifndef LR_RAYCAST_GRAB
#define LR_RAYCAST_GRAB 256
#endif
constexpr uint32_t kRaycastGrab = LR_RAYCAST_GRAB;// rays a wave takes from the global counter with one atomic, at most (raycast_kernel.h); a multiple of 64
static_assert(kRaycastGrab % 64u == 0u && kRaycastGrab >= 64u, "whole waves of rays");

hipError_t launch_kernel(bool alpha, unsigned blocks, hipStream_t stream, const lrd::DScene *device_scene, const lrd::RaycastArgs &args) {
    if (alpha) { hipLaunchKernelGGL(lrd::raycast_kernel<true>, dim3(blocks), dim3(lrd::kBlockThreads), 0, stream, (lrd::DScenePtr)device_scene, args); }
    else { hipLaunchKernelGGL(lrd::raycast_kernel<false>, dim3(blocks), dim3(lrd::kBlockThreads), 0, stream, (lrd::DScenePtr)device_scene, args); }
    return hipGetLastError();
}

// one launch over `count` rays in device memory, between the context's trace events
int trace_device(lrhip_ctx *ctx, const void *rays, void *out, uint32_t count, uint32_t phase, bool alpha) {
    auto &per_cu = ctx->raycast_blocks[alpha ? 1 : 0];
    if (per_cu < 0) {
        int n = 0;
        if (alpha) { LR_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lrd::raycast_kernel<true>, lrd::kBlockThreads, 0)); }
        else { LR_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, lrd::raycast_kernel<false>, lrd::kBlockThreads, 0)); }
        per_cu = std::max(1, std::min(n, static_cast<int>(kMaxBlocksPerCu)));
    }
    // persistent grid: the blocks that fill the device, or fewer for a small batch.  THE BOUND OF THE STACK'S OVERFLOW AREA: lrhip_upload_scene
    // sized ctx->spill for ctx->grid_blocks = cu_count x kMaxBlocksPerCu blocks of kBlockThreads threads (kSpillEntries words each), and
    // refused a BVH whose walk could need more entries; this grid has at most that many blocks, and thread gtid < blocks x kBlockThreads
    // touches words [entry x total_threads + gtid] of it only
    const auto resident = ctx->cu_count * static_cast<uint32_t>(per_cu);
    const auto blocks = std::min(resident, (count + lrd::kBlockThreads - 1u) / lrd::kBlockThreads);
    if (blocks > ctx->grid_blocks || static_cast<size_t>(blocks) * lrd::kBlockThreads * lrd::kSpillEntries * sizeof(uint32_t) > ctx->spill.bytes) {
        return fail(LRHIP_ERROR_DEVICE, "lrhip_trace_rays: the grid does not fit the traversal stack's overflow area");
    }
    lrd::RaycastArgs args{};
    args.rays = static_cast<const float4 *>(rays), args.out = out;
    args.count = count, args.phase = phase;
    args.next = static_cast<uint32_t *>(ctx->work_counter.ptr);
    args.spill = static_cast<uint32_t *>(ctx->spill.ptr);
    args.total_threads = blocks * lrd::kBlockThreads;
    // rays per grab: a quarter of a wave's share of the batch, so that the waves finish together, within 64 .. kRaycastGrab
    const auto share = count / (blocks * lrd::kWavesPerBlock * 4u);
    args.grab = std::min(kRaycastGrab, std::max(64u, share & ~63u));
    LR_HIP_CHECK(hipMemsetAsync(ctx->work_counter.ptr, 0, sizeof(uint32_t), ctx->stream));
    // the scene record as the host holds it now (lrhip_render writes one per launch; none exists before the first render)
    if (auto r = ensure(ctx->scene_record, sizeof(lrd::DScene)); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemcpyAsync(ctx->scene_record.ptr, &ctx->scene, sizeof(lrd::DScene), hipMemcpyHostToDevice, ctx->stream));
    LR_HIP_CHECK(hipEventRecord(ctx->raycast_begin, ctx->stream));
    LR_HIP_CHECK(launch_kernel(alpha, blocks, ctx->stream, static_cast<const lrd::DScene *>(ctx->scene_record.ptr), args));
    LR_HIP_CHECK(hipEventRecord(ctx->raycast_end, ctx->stream));
    ctx->raycast_pending = true;
    return LRHIP_OK;
}

// the pending launch's time joins the call's sum (synchronises with it)
int collect_time(lrhip_ctx *ctx) {
    if (!ctx->raycast_pending) { return LRHIP_OK; }
    float ms = 0.f;
    LR_HIP_CHECK(hipEventSynchronize(ctx->raycast_end));
    LR_HIP_CHECK(hipEventElapsedTime(&ms, ctx->raycast_begin, ctx->raycast_end));
    ctx->raycast_ms += static_cast<double>(ms);
    ctx->raycast_pending = false;
    return LRHIP_OK;
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_trace_rays(lrhip_ctx *ctx, const lrhip_ray_query_params *p) {
    if (ctx == nullptr || p == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: NULL argument"); }
    if (p->mode != LRHIP_RAY_CLOSEST && p->mode != LRHIP_RAY_ANY) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: unknown mode " + std::to_string(p->mode));
    }
    if ((p->flags & ~(LRHIP_RAY_DEVICE_POINTERS | LRHIP_RAY_ALPHA_TEST)) != 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: unknown flags"); }
    if (p->count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: more than 2^31 - 1 rays"); }
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: no scene uploaded"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->rays == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: rays / out is NULL"); }
        if (device_pointers && ((reinterpret_cast<uintptr_t>(p->rays) | reinterpret_cast<uintptr_t>(p->out)) & 15u) != 0u) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: device pointers must be 16-byte aligned");
        }
    }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->raycast_ms = 0.0, ctx->raycast_pending = false;
    if (p->count == 0u) { return LRHIP_OK; }
    if (ctx->raycast_begin == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->raycast_begin)); }
    if (ctx->raycast_end == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->raycast_end)); }
    const auto phase = p->mode == LRHIP_RAY_ANY ? lrd::kPhaseShadow : lrd::kPhaseClosest;
    // (a scene without maybe-non-opaque instances parks no candidate: the kernel without the alpha test gives the same answers)
    const auto alpha = (p->flags & LRHIP_RAY_ALPHA_TEST) != 0u && (ctx->features & lrd::kFeatAlpha) != 0u;
    if (device_pointers) { return trace_device(ctx, p->rays, p->out, static_cast<uint32_t>(p->count), phase, alpha); }
    // host pointers: chunk by chunk through the staging buffers
    const size_t out_bytes = p->mode == LRHIP_RAY_ANY ? sizeof(uint32_t) : sizeof(lrhip_ray_hit);
    const auto chunk = std::min<uint64_t>(p->count, kRaycastChunk);
    if (auto r = ensure(ctx->raycast_rays, chunk * sizeof(lrhip_ray)); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->raycast_out, chunk * out_bytes); r != LRHIP_OK) { return r; }
    for (uint64_t first = 0u; first < p->count; first += chunk) {
        const auto n = std::min<uint64_t>(chunk, p->count - first);
        LR_HIP_CHECK(hipMemcpyAsync(ctx->raycast_rays.ptr, static_cast<const lrhip_ray *>(p->rays) + first, n * sizeof(lrhip_ray),
                                    hipMemcpyHostToDevice, ctx->stream));
        if (auto r = trace_device(ctx, ctx->raycast_rays.ptr, ctx->raycast_out.ptr, static_cast<uint32_t>(n), phase, alpha); r != LRHIP_OK) { return r; }
        LR_HIP_CHECK(hipMemcpyAsync(static_cast<char *>(p->out) + first * out_bytes, ctx->raycast_out.ptr, n * out_bytes, hipMemcpyDeviceToHost,
                                    ctx->stream));
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = collect_time(ctx); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

double lrhip_last_trace_ms(lrhip_ctx *ctx) {
    if (ctx == nullptr) { return 0.0; }
    if (hipSetDevice(ctx->device) != hipSuccess || collect_time(ctx) != LRHIP_OK) { return -1.0; }
    return ctx->raycast_ms;
}

}// extern "C"
