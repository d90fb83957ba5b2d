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

#ifndef LR_RAYCAST_GRAB
#define LR_RAYCAST_GRAB 256
#endif
constexpr uint32_t kRaycastGrab = LR_RAYCAST_GRAB;// rays a wave takes from the global counter with one atomic, at most (raycast_kernel.h); a multiple of 64
static_assert(kRaycastGrab % 64u == 0u && kRaycastGrab >= 64u, "whole waves of rays");

hipError_t launch_kernel(bool alpha, unsigned blocks, hipStream_t stream, lrd::DScenePtr device_scene, const lrd::RaycastArgs &args) {
    if (alpha) { hipLaunchKernelGGL(lrd::raycast_kernel<true>, dim3(blocks), dim3(lrd::kBlockThreads), 0, stream, device_scene, args); }
    else { hipLaunchKernelGGL(lrd::raycast_kernel<false>, dim3(blocks), dim3(lrd::kBlockThreads), 0, stream, device_scene, args); }
    return hipGetLastError();
}

// one launch over `count` rays in device memory, between the events of the context's raycast timer
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
    lrd::DScenePtr device_scene{};
    if (auto r = upload_scene_record(ctx, device_scene); r != LRHIP_OK) { return r; }
    if (auto r = timer_begin(ctx, ctx->raycast_timer); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(launch_kernel(alpha, blocks, ctx->stream, device_scene, args));
    return timer_end(ctx, ctx->raycast_timer);
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_trace_rays(lrhip_ctx *ctx, const lrhip_ray_query_params *p) {
    if (auto r = screen("lrhip_trace_rays", ctx, p, LRHIP_RAY_DEVICE_POINTERS | LRHIP_RAY_ALPHA_TEST, "rays"); r != LRHIP_OK) { return r; }
    if (p->mode != LRHIP_RAY_CLOSEST && p->mode != LRHIP_RAY_ANY) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: unknown mode " + std::to_string(p->mode));
    }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->rays == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: rays / out is NULL"); }
        if (device_pointers && misaligned({{p->rays, 15u}, {p->out, 15u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_trace_rays: device pointers must be 16-byte aligned");
        }
    }
    if (auto r = timer_start(ctx, ctx->raycast_timer, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    const auto phase = p->mode == LRHIP_RAY_ANY ? lrd::kPhaseShadow : lrd::kPhaseClosest;
    // (a scene without maybe-non-opaque instances parks no candidate: the kernel without the alpha test gives the same answers)
    const auto alpha = (p->flags & LRHIP_RAY_ALPHA_TEST) != 0u && (ctx->features & lrd::kFeatAlpha) != 0u;
    return staged_call(ctx, ctx->raycast_timer, p->count, device_pointers,
                       {column_out(p->out, p->mode == LRHIP_RAY_ANY ? sizeof(uint32_t) : sizeof(lrhip_ray_hit)), column_in(p->rays, sizeof(lrhip_ray))},
                       [&](uint32_t n, uint64_t, void *const *d) { return trace_device(ctx, d[1], d[0], n, phase, alpha); });
}

double lrhip_last_trace_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->raycast_timer) : 0.0; }

}// extern "C"
