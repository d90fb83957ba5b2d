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

using namespace lrh;

namespace {

// one launch of `kernel` over args.count records, between the events of the context's camera timer
template<typename Kernel, typename Args>
int launch_between_events(lrhip_ctx *ctx, Kernel kernel, const Args &args) {
    lrd::DScenePtr device_scene{};
    if (auto r = upload_scene_record(ctx, device_scene); r != LRHIP_OK) { return r; }
    if (auto r = timer_begin(ctx, ctx->camera_timer); r != LRHIP_OK) { return r; }
    hipLaunchKernelGGL(kernel, dim3(blocks_of(args.count)), dim3(lrd::kBlockThreads), 0, ctx->stream, device_scene, args);
    LR_HIP_CHECK(hipGetLastError());
    return timer_end(ctx, ctx->camera_timer);
}

}// namespace

extern "C" {

int lrhip_query_sampler(lrhip_ctx *ctx, const lrhip_sampler_query_params *p) {
    if (auto r = screen("lrhip_query_sampler", ctx, p, LRHIP_RAY_DEVICE_POINTERS | LRHIP_SAMPLER_START, "records"); r != LRHIP_OK) { return r; }
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
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    const auto start = (p->flags & LRHIP_SAMPLER_START) != 0u;
    // what the call does not read or write is not looked at
    const auto streams = start ? p->streams : nullptr;
    const auto indices = start ? p->indices : nullptr;
    const auto out = args.floats != 0u ? p->out : nullptr;
    if (p->count != 0u) {
        if (p->state == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: state is NULL"); }
        if (args.floats != 0u && p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: out is NULL"); }
        if (device_pointers && misaligned({{p->state, 15u}, {out, 15u}, {streams, 3u}, {indices, 3u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: device pointers must be 16-byte aligned (streams, indices: 4-byte)");
        }
    }
    if (ctx->scene.sampler_kind == LR_SAMPLER_PADDED_SOBOL && ctx->scene.sampler_spp == 0u) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_query_sampler: the scene's PaddedSobol sampler has a permutation of length 0 (sampler.spp)");
    }
    const auto launches = p->count != 0u && (start || args.draws != 0u);// (no draw of a restored state: the state is what it was)
    if (auto r = timer_start(ctx, ctx->camera_timer, launches); r != LRHIP_OK) { return r; }
    if (!launches) { return LRHIP_OK; }
    args.start = start ? 1u : 0u, args.sample_index = p->sample_index;
    const auto generic = ctx->scene.sampler_kind != LR_SAMPLER_INDEPENDENT;
    return staged_call(ctx, ctx->camera_timer, p->count, device_pointers,
                       {column_out(out, args.floats * sizeof(float)), Column{p->state, sizeof(uint4), start ? kColumnOut : kColumnInOut},
                        column_in(streams, sizeof(uint32_t)), column_in(indices, sizeof(uint32_t))},
                       [&](uint32_t n, uint64_t first, void *const *d) {
        args.out = static_cast<float *>(d[0]), args.state = static_cast<uint4 *>(d[1]);
        args.streams = static_cast<const uint32_t *>(d[2]), args.indices = static_cast<const uint32_t *>(d[3]);
        args.count = n, args.stream_base = static_cast<uint32_t>(first);
        return generic ? launch_between_events(ctx, lrd::sampler_kernel<true>, args) : launch_between_events(ctx, lrd::sampler_kernel<false>, args);
    });
}

int lrhip_query_camera(lrhip_ctx *ctx, const lrhip_camera_query_params *p) {
    if (auto r = screen("lrhip_query_camera", ctx, p, LRHIP_RAY_DEVICE_POINTERS, "records"); r != LRHIP_OK) { return r; }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->u == nullptr || p->out_rays == nullptr || p->out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: u / out_rays / out is NULL"); }
        if (p->pixels == nullptr && p->count > static_cast<uint64_t>(ctx->width) * ctx->height) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: without pixels, record k is pixel k: more records than the frame has pixels");
        }
        if (device_pointers && misaligned({{p->u, 15u}, {p->out_rays, 15u}, {p->out, 15u}, {p->pixels, 3u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_query_camera: device pointers must be 16-byte aligned (pixels: 4-byte)");
        }
    }
    if (auto r = timer_start(ctx, ctx->camera_timer, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    // (no column 0: the 16-byte records go where a sampler's states do, the drawn numbers alone are wide -- DESIGN §4.17)
    return staged_call(ctx, ctx->camera_timer, p->count, device_pointers,
                       {Column{}, column_out(p->out, sizeof(lrhip_camera_sample)), column_in(p->pixels, sizeof(uint32_t)), column_in(p->u, sizeof(float4)),
                        column_out(p->out_rays, sizeof(lrhip_ray))},
                       [&](uint32_t n, uint64_t first, void *const *d) {
        lrd::CameraArgs args{};
        args.out = static_cast<float4 *>(d[1]), args.pixels = static_cast<const uint32_t *>(d[2]);
        args.u = static_cast<const float4 *>(d[3]), args.out_rays = static_cast<float4 *>(d[4]);
        args.count = n, args.pixel_base = static_cast<uint32_t>(first);
        return launch_between_events(ctx, lrd::camera_kernel, args);
    });
}

int lrhip_film_splat(lrhip_ctx *ctx, const lrhip_film_splat_params *p) {
    if (auto r = screen("lrhip_film_splat", ctx, p, LRHIP_RAY_DEVICE_POINTERS, "records"); r != LRHIP_OK) { return r; }
    if (!(p->clamp >= 0.f)) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: the clamp must be positive, or 0 for the scene's"); }
    const auto device_pointers = (p->flags & LRHIP_RAY_DEVICE_POINTERS) != 0u;
    if (p->count != 0u) {
        if (p->values == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: values is NULL"); }
        if (p->pixels == nullptr && p->count > static_cast<uint64_t>(ctx->width) * ctx->height) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: without pixels, record k goes to pixel k: more records than the frame has pixels");
        }
        if (device_pointers && misaligned({{p->values, 15u}, {p->pixels, 3u}})) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_film_splat: device pointers must be 16-byte aligned (pixels: 4-byte)");
        }
    }
    if (ctx->film == nullptr) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_film_splat: the context holds no film"); }
    if (auto r = timer_start(ctx, ctx->camera_timer, p->count != 0u); r != LRHIP_OK) { return r; }
    if (p->count == 0u) { return LRHIP_OK; }
    // (columns 2 and 3, as the camera query's pixels and numbers)
    return staged_call(ctx, ctx->camera_timer, p->count, device_pointers,
                       {Column{}, Column{}, column_in(p->pixels, sizeof(uint32_t)), column_in(p->values, sizeof(float4))},
                       [&](uint32_t n, uint64_t first, void *const *d) {
        lrd::SplatArgs args{};
        args.film = ctx->film;
        args.clamp = p->clamp > 0.f ? p->clamp : ctx->scene.film_clamp;
        args.pixels = static_cast<const uint32_t *>(d[2]), args.values = static_cast<const float4 *>(d[3]);
        args.count = n, args.pixel_base = static_cast<uint32_t>(first);
        return launch_between_events(ctx, lrd::splat_kernel, args);
    });
}

double lrhip_last_camera_ms(lrhip_ctx *ctx) { return ctx != nullptr ? timer_read(ctx, ctx->camera_timer) : 0.0; }

}// extern "C"
