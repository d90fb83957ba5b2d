// lrhip_camera.hip — C ABI of the camera, sampler and film queries (include/lrhip.h: lrhip_query_sampler, lrhip_query_camera, lrhip_film_splat,
// lrhip_last_camera_ms).  Holds the four kernels of camera_kernel.h (the sampler's two instantiations, the camera's and the
// splat's) and their launches on the context's stream.  They make no real call: no texture, no closure and no environment is touched.  The
// object is built with the oracle's arithmetic, as lrhip_bsdf.o and lrhip_light.o (Makefile: lrhip_camera_FLAGS): a query hands single
// answers to its caller -- the Sobol sampler's pixel draw has a multiply-subtract that contraction would fuse, the camera's normalize a
// division
#include "lrhip_internal.h"
#include "camera_kernel.h"

static_assert(sizeof(lrhip_camera_sample) == 16u && offsetof(lrhip_camera_sample, film_x) == 4u && offsetof(lrhip_camera_sample, pixel) == 12u,
              "lrhip_camera_sample = the float4 camera_kernel stores");
static_assert(sizeof(lrhip_ray) == 32u && offsetof(lrhip_ray, t_min) == 12u && offsetof(lrhip_ray, d) == 16u && offsetof(lrhip_ray, t_max) == 28u,
              "a camera ray is two dwordx4 stores (camera_kernel.h)");
static_assert(LRHIP_DRAW_1D == lrd::kDraw1d && LRHIP_DRAW_2D == lrd::kDraw2d && LRHIP_DRAW_PIXEL_2D == lrd::kDrawPixel2d &&
                  LRHIP_SAMPLER_MAX_DRAWS == lrd::kSamplerMaxDraws,
              "lrhip.h's draw codes are the kernel's");
static_assert(lrd::PathSampler<true>::kSavedWords == 4u && lrd::PathSampler<false>::kSavedWords == 1u, "a sampler state is one uint4");
static_assert((LRHIP_SAMPLER_START & (LRHIP_RAY_DEVICE_POINTERS | LRHIP_RAY_ALPHA_TEST | LRHIP_RADIANCE_ACCUMULATE | LRHIP_RADIANCE_COUNTERS |
                                      LRHIP_MESH_RECOMPUTE_NORMALS | LRHIP_SURFACE_GEOMETRY_ONLY | LRHIP_LIGHT_FROM_POINTS)) == 0u,
              "the queries' flags share one word");

namespace lrd {
template __global__ void sampler_kernel<false>(DScenePtr, SamplerArgs);
template __global__ void sampler_kernel<true>(DScenePtr, SamplerArgs);
}

namespace lrh {

namespace {

// records per chunk of a host-pointer call: 16 MiB each of states, numbers and records, 32 MiB of rays, 4 MiB each of ids and 4 MiB per drawn
// float in the staging buffers, whatever the count; every host-pointer call synchronises per chunk
constexpr uint64_t kCameraChunk = 1ull << 20u;
// blocks of a launch, at most: 2^20 blocks of 256 lanes cover 2^28 records in one pass; a larger batch strides
constexpr uint32_t kCameraMaxBlocks = 1u << 20u;

uint32_t blocks_of(uint32_t count) { return std::min(kCameraMaxBlocks, (count + lrd::kBlockThreads - 1u) / lrd::kBlockThreads); }

// the scene record as the host holds it now (lrhip_render writes one per launch; none exists before the first render), then the begin event
int begin_launch(lrhip_ctx *ctx, lrd::DScenePtr &device_scene) {
    if (auto r = ensure(ctx->scene_record, sizeof(lrd::DScene)); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemcpyAsync(ctx->scene_record.ptr, &ctx->scene, sizeof(lrd::DScene), hipMemcpyHostToDevice, ctx->stream));
    device_scene = (lrd::DScenePtr) static_cast<const lrd::DScene *>(ctx->scene_record.ptr);
    LR_HIP_CHECK(hipEventRecord(ctx->camera_begin, ctx->stream));
    return LRHIP_OK;
}
int end_launch(lrhip_ctx *ctx) {
    LR_HIP_CHECK(hipGetLastError());
    LR_HIP_CHECK(hipEventRecord(ctx->camera_end, ctx->stream));
    ctx->camera_pending = true;
    return LRHIP_OK;
}

// the pending launch's time joins the call's sum (synchronises with it)
int collect_time(lrhip_ctx *ctx) {
    if (!ctx->camera_pending) { return LRHIP_OK; }
    float ms = 0.f;
    LR_HIP_CHECK(hipEventSynchronize(ctx->camera_end));
    LR_HIP_CHECK(hipEventElapsedTime(&ms, ctx->camera_begin, ctx->camera_end));
    ctx->camera_ms += static_cast<double>(ms);
    ctx->camera_pending = false;
    return LRHIP_OK;
}

// what the three calls share before their first launch: the device, the call's time, the events
int begin_call(lrhip_ctx *ctx, bool launches) {
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    ctx->camera_ms = 0.0, ctx->camera_pending = false;
    if (!launches) { return LRHIP_OK; }
    if (ctx->camera_begin == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->camera_begin)); }
    if (ctx->camera_end == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->camera_end)); }
    return LRHIP_OK;
}

bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0u; }

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

int lrhip_query_sampler(lrhip_ctx *ctx, const lrhip_sampler_query_params *p) {
    if (ctx == nullptr || p == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: NULL argument"); }
    if ((p->flags & ~(LRHIP_RAY_DEVICE_POINTERS | LRHIP_SAMPLER_START)) != 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: unknown flags"); }
    if (p->count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: more than 2^31 - 1 records"); }
    if (p->pattern_count > LRHIP_SAMPLER_MAX_DRAWS) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: more than 64 draws"); }
    if (p->pattern_count != 0u && p->pattern == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: pattern is NULL"); }
    lrd::SamplerArgs args{};
    for (uint32_t i = 0u; i < p->pattern_count; i++) {
        const auto code = p->pattern[i];
        if (code != LRHIP_DRAW_1D && code != LRHIP_DRAW_2D && code != LRHIP_DRAW_PIXEL_2D) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: unknown draw code " + std::to_string(code));
        }
        args.pattern[i >> 5u] |= static_cast<unsigned long long>(code) << ((i & 31u) * 2u);
        args.floats += code == LRHIP_DRAW_1D ? 1u : 2u;
    }
    args.draws = p->pattern_count;
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: no scene uploaded"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    const auto start = (p->flags & LRHIP_SAMPLER_START) != 0u;
    // what the call does not read is not looked at
    const auto streams = start ? p->streams : nullptr;
    const auto indices = start ? p->indices : nullptr;
    if (p->count != 0u) {
        if (p->state == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: state is NULL"); }
        if (args.floats != 0u && p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: out is NULL"); }
        if (device_pointers && (misaligned(p->state, 15u) || (args.floats != 0u && misaligned(p->out, 15u)) || misaligned(streams, 3u) ||
                                misaligned(indices, 3u))) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: device pointers must be 16-byte aligned (streams, indices: 4-byte)");
        }
    }
    if (ctx->scene.sampler_kind == LR_SAMPLER_PADDED_SOBOL && ctx->scene.sampler_spp == 0u) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: the scene's PaddedSobol sampler has a permutation of length 0 (sampler.spp)");
    }
    const auto launches = p->count != 0u && (start || args.draws != 0u);// (no draw of a restored state: the state is what it was)
    if (auto r = begin_call(ctx, launches); r != LRHIP_OK) { return r; }
    if (!launches) { return LRHIP_OK; }
    args.start = start ? 1u : 0u, args.sample_index = p->sample_index;
    const auto generic = ctx->scene.sampler_kind != LR_SAMPLER_INDEPENDENT;
    auto launch = [&](uint32_t count) {
        lrd::DScenePtr device_scene{};
        args.count = count;
        if (auto r = begin_launch(ctx, device_scene); r != LRHIP_OK) { return r; }
        if (generic) {
            hipLaunchKernelGGL((lrd::sampler_kernel<true>), dim3(blocks_of(count)), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args);
        } else {
            hipLaunchKernelGGL((lrd::sampler_kernel<false>), dim3(blocks_of(count)), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args);
        }
        return end_launch(ctx);
    };
    if (device_pointers) {
        args.state = static_cast<uint4 *>(p->state), args.streams = streams, args.indices = indices, args.out = p->out;
        return launch(static_cast<uint32_t>(p->count));
    }
    // host pointers: chunk by chunk through the staging buffers
    const auto chunk = std::min<uint64_t>(p->count, kCameraChunk);
    const auto row_bytes = static_cast<size_t>(args.floats) * sizeof(float);
    if (auto r = ensure(ctx->camera_state, chunk * sizeof(uint4)); r != LRHIP_OK) { return r; }
    if (streams != nullptr) { if (auto r = ensure(ctx->camera_streams, chunk * sizeof(uint32_t)); r != LRHIP_OK) { return r; } }
    if (indices != nullptr) { if (auto r = ensure(ctx->camera_indices, chunk * sizeof(uint32_t)); r != LRHIP_OK) { return r; } }
    if (row_bytes != 0u) { if (auto r = ensure(ctx->camera_out, chunk * row_bytes); r != LRHIP_OK) { return r; } }
    args.state = static_cast<uint4 *>(ctx->camera_state.ptr), args.out = static_cast<float *>(ctx->camera_out.ptr);
    args.streams = streams != nullptr ? static_cast<const uint32_t *>(ctx->camera_streams.ptr) : nullptr;
    args.indices = indices != nullptr ? static_cast<const uint32_t *>(ctx->camera_indices.ptr) : nullptr;
    for (uint64_t first = 0u; first < p->count; first += chunk) {
        const auto n = std::min<uint64_t>(chunk, p->count - first);
        const auto host_state = static_cast<uint4 *>(p->state) + first;
        if (!start) { LR_HIP_CHECK(hipMemcpyAsync(ctx->camera_state.ptr, host_state, n * sizeof(uint4), hipMemcpyHostToDevice, ctx->stream)); }
        if (streams != nullptr) {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->camera_streams.ptr, streams + first, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        }
        if (indices != nullptr) {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->camera_indices.ptr, indices + first, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        }
        args.stream_base = static_cast<uint32_t>(first);
        if (auto r = launch(static_cast<uint32_t>(n)); r != LRHIP_OK) { return r; }
        LR_HIP_CHECK(hipMemcpyAsync(host_state, ctx->camera_state.ptr, n * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
        if (row_bytes != 0u) {
            LR_HIP_CHECK(hipMemcpyAsync(reinterpret_cast<char *>(p->out) + first * row_bytes, ctx->camera_out.ptr, n * row_bytes, hipMemcpyDeviceToHost,
                                        ctx->stream));
        }
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = collect_time(ctx); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

int lrhip_query_camera(lrhip_ctx *ctx, const lrhip_camera_query_params *p) {
    if (ctx == nullptr || p == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: NULL argument"); }
    if ((p->flags & ~LRHIP_RAY_DEVICE_POINTERS) != 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: unknown flags"); }
    if (p->count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: more than 2^31 - 1 records"); }
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: no scene uploaded"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->u == nullptr || p->out_rays == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: u / out_rays / out is NULL"); }
        if (p->pixels == nullptr && p->count > static_cast<uint64_t>(ctx->width) * ctx->height) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: without pixels, record k is pixel k: more records than the frame has pixels");
        }
        if (device_pointers && (misaligned(p->u, 15u) || misaligned(p->out_rays, 15u) || misaligned(p->out, 15u) || misaligned(p->pixels, 3u))) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: device pointers must be 16-byte aligned (pixels: 4-byte)");
        }
    }
    if (auto r = begin_call(ctx, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    lrd::CameraArgs args{};
    auto launch = [&](uint32_t count) {
        lrd::DScenePtr device_scene{};
        args.count = count;
        if (auto r = begin_launch(ctx, device_scene); r != LRHIP_OK) { return r; }
        hipLaunchKernelGGL(lrd::camera_kernel, dim3(blocks_of(count)), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args);
        return end_launch(ctx);
    };
    if (device_pointers) {
        args.pixels = p->pixels, args.u = static_cast<const float4 *>(p->u);
        args.out_rays = static_cast<float4 *>(p->out_rays), args.out = static_cast<float4 *>(p->out);
        return launch(static_cast<uint32_t>(p->count));
    }
    // host pointers: chunk by chunk through the staging buffers (the numbers through the BSDF queries' buffer, the rays through the light queries')
    const auto chunk = std::min<uint64_t>(p->count, kCameraChunk);
    if (auto r = ensure(ctx->bsdf_dirs, chunk * sizeof(float4)); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->light_rays, chunk * sizeof(lrhip_ray)); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->camera_state, chunk * sizeof(lrhip_camera_sample)); r != LRHIP_OK) { return r; }
    if (p->pixels != nullptr) { if (auto r = ensure(ctx->camera_streams, chunk * sizeof(uint32_t)); r != LRHIP_OK) { return r; } }
    args.pixels = p->pixels != nullptr ? static_cast<const uint32_t *>(ctx->camera_streams.ptr) : nullptr;
    args.u = static_cast<const float4 *>(ctx->bsdf_dirs.ptr);
    args.out_rays = static_cast<float4 *>(ctx->light_rays.ptr), args.out = static_cast<float4 *>(ctx->camera_state.ptr);
    for (uint64_t first = 0u; first < p->count; first += chunk) {
        const auto n = std::min<uint64_t>(chunk, p->count - first);
        LR_HIP_CHECK(hipMemcpyAsync(ctx->bsdf_dirs.ptr, static_cast<const float4 *>(p->u) + first, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
        if (p->pixels != nullptr) {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->camera_streams.ptr, p->pixels + first, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        }
        args.pixel_base = static_cast<uint32_t>(first);
        if (auto r = launch(static_cast<uint32_t>(n)); r != LRHIP_OK) { return r; }
        LR_HIP_CHECK(hipMemcpyAsync(static_cast<lrhip_ray *>(p->out_rays) + first, ctx->light_rays.ptr, n * sizeof(lrhip_ray), hipMemcpyDeviceToHost,
                                    ctx->stream));
        LR_HIP_CHECK(hipMemcpyAsync(static_cast<lrhip_camera_sample *>(p->out) + first, ctx->camera_state.ptr, n * sizeof(lrhip_camera_sample),
                                    hipMemcpyDeviceToHost, ctx->stream));
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = collect_time(ctx); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

int lrhip_film_splat(lrhip_ctx *ctx, const lrhip_film_splat_params *p) {
    if (ctx == nullptr || p == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: NULL argument"); }
    if ((p->flags & ~LRHIP_RAY_DEVICE_POINTERS) != 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: unknown flags"); }
    if (p->count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: more than 2^31 - 1 records"); }
    if (!(p->clamp >= 0.f)) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: the clamp must be positive, or 0 for the scene's"); }
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: no scene uploaded"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->values == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: values is NULL"); }
        if (p->pixels == nullptr && p->count > static_cast<uint64_t>(ctx->width) * ctx->height) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: without pixels, record k goes to pixel k: more records than the frame has pixels");
        }
        if (device_pointers && (misaligned(p->values, 15u) || misaligned(p->pixels, 3u))) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: device pointers must be 16-byte aligned (pixels: 4-byte)");
        }
    }
    if (ctx->film == nullptr) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_film_splat: the context holds no film"); }
    if (auto r = begin_call(ctx, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    lrd::SplatArgs args{};
    args.film = ctx->film;
    args.clamp = p->clamp > 0.f ? p->clamp : ctx->scene.film_clamp;
    auto launch = [&](uint32_t count) {
        lrd::DScenePtr device_scene{};
        args.count = count;
        if (auto r = begin_launch(ctx, device_scene); r != LRHIP_OK) { return r; }
        hipLaunchKernelGGL(lrd::splat_kernel, dim3(blocks_of(count)), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args);
        return end_launch(ctx);
    };
    if (device_pointers) {
        args.pixels = p->pixels, args.values = static_cast<const float4 *>(p->values);
        return launch(static_cast<uint32_t>(p->count));
    }
    // host pointers: chunk by chunk through the staging buffers (the values through the BSDF queries' buffer)
    const auto chunk = std::min<uint64_t>(p->count, kCameraChunk);
    if (auto r = ensure(ctx->bsdf_dirs, chunk * sizeof(float4)); r != LRHIP_OK) { return r; }
    if (p->pixels != nullptr) { if (auto r = ensure(ctx->camera_streams, chunk * sizeof(uint32_t)); r != LRHIP_OK) { return r; } }
    args.pixels = p->pixels != nullptr ? static_cast<const uint32_t *>(ctx->camera_streams.ptr) : nullptr;
    args.values = static_cast<const float4 *>(ctx->bsdf_dirs.ptr);
    for (uint64_t first = 0u; first < p->count; first += chunk) {
        const auto n = std::min<uint64_t>(chunk, p->count - first);
        LR_HIP_CHECK(hipMemcpyAsync(ctx->bsdf_dirs.ptr, static_cast<const float4 *>(p->values) + first, n * sizeof(float4), hipMemcpyHostToDevice,
                                    ctx->stream));
        if (p->pixels != nullptr) {
            LR_HIP_CHECK(hipMemcpyAsync(ctx->camera_streams.ptr, p->pixels + first, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        }
        args.pixel_base = static_cast<uint32_t>(first);
        if (auto r = launch(static_cast<uint32_t>(n)); r != LRHIP_OK) { return r; }
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = collect_time(ctx); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

double lrhip_last_camera_ms(lrhip_ctx *ctx) {
    if (ctx == nullptr) { return 0.0; }
    if (hipSetDevice(ctx->device) != hipSuccess || collect_time(ctx) != LRHIP_OK) { return -1.0; }
    return ctx->camera_ms;
}

}// extern "C"
