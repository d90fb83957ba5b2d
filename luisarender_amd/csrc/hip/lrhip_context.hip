// lrhip_context.hip — C ABI (include/lrhip.h) of the gfx950 megakernel path tracer: the context, its setters, the film's binding,
// clearing and read-back, counters.  Holds the small film kernels (film_kernels.h) and their launchers.  Device code lives in the
// dev_*.h headers and megapath_kernel.h.
#include "lrhip_internal.h"
#include "film_kernels.h"

namespace lrh {

namespace {
thread_local std::string g_last_error;
}

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

int ensure(DeviceBuffer &b, size_t bytes) {
    if (b.bytes >= bytes) { return LRHIP_OK; }
    b.release();
    LR_HIP_CHECK(hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
    return LRHIP_OK;
}

void release_scene(lrhip_ctx *ctx) {
    for (auto &b : ctx->scene_buffers) { b.release(); }
    ctx->scene_buffers.clear();
    ctx->scene_ready = false;
    ctx->nodes32 = nullptr, ctx->level_nodes = nullptr, ctx->level_offsets.clear();
    for (auto &b : ctx->mesh_adjacency) { b.release(); }
    ctx->mesh_adjacency.clear(), ctx->meshes.clear(), ctx->mesh_light.clear(), ctx->instance_handles.clear();
    ctx->surface_meshes_ready = false;
    ctx->light_tri_owner = nullptr, ctx->light_record_count = 0u, ctx->light_tri_count = 0u;
    // the queues of wavefront mode and the pool kernels' state records are sized for the scene (and the memory free at the time): a new
    // scene starts without them (76-89 GB kept until lrhip_destroy starved later allocations on the same GPU)
    ctx->wf_heavy.release(), ctx->wf_cont.release(), ctx->pool.release();
}

// ---- the film kernels (plain __global__ definitions: this is the one translation unit that holds them), launched on the context's stream
hipError_t launch_resolve_partial(lrhip_ctx *ctx, const float4 *partial, uint32_t chunk_count, uint32_t tiles_x, uint32_t tile_begin,
                                  uint32_t tile_end, uint32_t tile_stride) {
    const auto pixel_count = ctx->width * ctx->height;
    hipLaunchKernelGGL(lrd::resolve_partial_kernel, dim3((pixel_count + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->film, partial,
                       pixel_count, chunk_count, ctx->width, tiles_x, tile_begin, tile_end, tile_stride);
    return hipGetLastError();
}

hipError_t launch_resolve_aov_partial(lrhip_ctx *ctx, uint32_t chunk_count, uint32_t tiles_x, uint32_t tile_begin, uint32_t tile_end,
                                      uint32_t tile_stride) {
    const auto pixel_count = ctx->width * ctx->height;
    const auto channels = ctx->scene.aov_channels;
    const auto n = static_cast<size_t>(pixel_count) * channels;
    hipLaunchKernelGGL(lrd::resolve_aov_partial_kernel, dim3(static_cast<unsigned>((n + 255u) / 256u)), dim3(256), 0, ctx->stream,
                       ctx->scene.aov, ctx->scene.aov_partial, pixel_count, channels, chunk_count, ctx->width, tiles_x, tile_begin, tile_end,
                       tile_stride);
    return hipGetLastError();
}

// The same reduce over the records of a radiance query: one row of `count` "pixels".  The frame is declared 2^31 wide with 2^28 tile columns, so
// that record i < 2^31 is pixel (i, 0) of tile i / 8 in row 0 -- whose rotation is none -- and every tile is in the range [0, 2^32 - 1) at stride 1
hipError_t launch_resolve_records(lrhip_ctx *ctx, float4 *records, const float4 *partial, uint32_t count, uint32_t chunk_count) {
    hipLaunchKernelGGL(lrd::resolve_partial_kernel, dim3((count + 255u) / 256u), dim3(256), 0, ctx->stream, records, partial, count, chunk_count,
                       0x80000000u, 1u << 28u, 0u, 0xffffffffu, 1u);
    return hipGetLastError();
}

// the frame's fixed-point sums join the film (and are cleared for the next call)
hipError_t launch_wf_resolve(lrhip_ctx *ctx, double inv_scale) {
    const auto pixel_count = ctx->width * ctx->height;
    hipLaunchKernelGGL(lrd::wf_resolve_kernel, dim3((pixel_count + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->film,
                       static_cast<unsigned long long *>(ctx->wf_accum.ptr), pixel_count, inv_scale);
    return hipGetLastError();
}

hipError_t launch_wf_carry(lrhip_ctx *ctx, uint32_t margin, uint32_t mode) {
    hipLaunchKernelGGL(lrd::wf_carry_kernel, dim3(1), dim3(64), 0, ctx->stream, static_cast<uint32_t *>(ctx->wf_counts.ptr), margin, mode);
    return hipGetLastError();
}

}// namespace lrh

using namespace lrh;

extern "C" {

const char *lrhip_last_error(void) { return g_last_error.c_str(); }

int lrhip_create(int device_ordinal, lrhip_ctx **out) {
    if (out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_create: out is NULL"); }
    int count = 0;
    LR_HIP_CHECK(hipGetDeviceCount(&count));
    if (device_ordinal < 0 || device_ordinal >= count) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_create: device ordinal " + std::to_string(device_ordinal) +
                                             " out of range (" + std::to_string(count) + " HIP devices)");
    }
    LR_HIP_CHECK(hipSetDevice(device_ordinal));
    auto ctx = new lrhip_ctx{};
    ctx->device = device_ordinal;
    hipDeviceProp_t prop{};
    if (auto e = hipGetDeviceProperties(&prop, device_ordinal); e != hipSuccess) {
        delete ctx;
        return fail(LRHIP_ERROR_DEVICE, std::string{"hipGetDeviceProperties: "} + hipGetErrorString(e));
    }
    ctx->cu_count = static_cast<uint32_t>(prop.multiProcessorCount);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev_begin) != hipSuccess || hipEventCreate(&ctx->ev_end) != hipSuccess) {
        delete ctx;
        return fail(LRHIP_ERROR_DEVICE, "lrhip_create: failed to create stream/events");
    }
    *out = ctx;
    return LRHIP_OK;
}

void lrhip_destroy(lrhip_ctx *ctx) {
    if (ctx == nullptr) { return; }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    release_scene(ctx);
    ctx->film_own.release(), ctx->converted.release(), ctx->partial.release();
    ctx->aov.release(), ctx->aov_partial.release();
    ctx->denoise_guide.release(), ctx->denoise_colour[0].release(), ctx->denoise_colour[1].release(), ctx->denoise_inputs.release();
    if (ctx->denoise_begin) { (void)hipEventDestroy(ctx->denoise_begin); }
    if (ctx->denoise_end) { (void)hipEventDestroy(ctx->denoise_end); }
    for (auto &slot : ctx->staging) { slot.release(); }
    for (auto timer : {&ctx->raycast_timer, &ctx->radiance_timer, &ctx->surface_timer, &ctx->bsdf_timer, &ctx->light_timer, &ctx->camera_timer,
                       &ctx->instance_timer, &ctx->mesh_timer, &ctx->lightmap_timer, &ctx->gather_timer}) {
        timer_destroy(*timer);
    }
    ctx->update_stage.release(), ctx->update_scratch.release(), ctx->surface_meshes.release(), ctx->lightmap_owner.release(), ctx->gather_table.release();
    ctx->spill.release(), ctx->wf_heavy.release(), ctx->wf_cont.release(), ctx->wf_counts.release(), ctx->wf_accum.release();
    ctx->pool.release(), ctx->counters.release(), ctx->work_counter.release(), ctx->scene_record.release();
    if (ctx->ev_begin) { (void)hipEventDestroy(ctx->ev_begin); }
    if (ctx->ev_end) { (void)hipEventDestroy(ctx->ev_end); }
    if (ctx->own_stream && ctx->stream) { (void)hipStreamDestroy(ctx->stream); }
    delete ctx;
}

int lrhip_set_stream(lrhip_ctx *ctx, void *hip_stream) {
    if (ctx == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_set_stream: ctx is NULL"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) { (void)hipStreamDestroy(ctx->stream); }
    if (hip_stream == nullptr) {
        LR_HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    } else {
        ctx->stream = static_cast<hipStream_t>(hip_stream);
        ctx->own_stream = false;
    }
    return LRHIP_OK;
}

int lrhip_bind_film(lrhip_ctx *ctx, void *device_float4_film) {
    if (ctx == nullptr || !ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_bind_film: no scene uploaded"); }
    ctx->film_external = static_cast<float4 *>(device_float4_film);
    ctx->film_external_w = ctx->width, ctx->film_external_h = ctx->height;
    ctx->film = device_float4_film != nullptr ? static_cast<float4 *>(device_float4_film) : static_cast<float4 *>(ctx->film_own.ptr);
    return LRHIP_OK;
}

int lrhip_film_clear(lrhip_ctx *ctx) {
    if (ctx == nullptr || !ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_clear: no scene uploaded"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    LR_HIP_CHECK(hipMemsetAsync(ctx->film, 0, static_cast<size_t>(ctx->width) * ctx->height * sizeof(float4), ctx->stream));
    if (ctx->scene.aov_channels != 0u) {
        LR_HIP_CHECK(hipMemsetAsync(ctx->aov.ptr, 0, static_cast<size_t>(ctx->width) * ctx->height * ctx->scene.aov_channels
            * sizeof(float), ctx->stream));
    }
    return LRHIP_OK;
}

uint64_t lrhip_packed_texels(lrhip_ctx *ctx) { return ctx != nullptr ? ctx->packed_texel_words : 0u; }

int lrhip_set_texture_storage(lrhip_ctx *ctx, uint32_t mode) {
    if (ctx == nullptr || mode > 2u) { return fail(LRHIP_ERROR_INVALID, "lrhip_set_texture_storage: invalid argument"); }
    ctx->byte_textures = mode;
    return LRHIP_OK;
}

int lrhip_set_diagnostics(lrhip_ctx *ctx, uint32_t force_features, double item_scale) {
    if (ctx == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_set_diagnostics: ctx is NULL"); }
    ctx->diag_force_features = force_features, ctx->diag_item_scale = item_scale;
    return LRHIP_OK;
}

int lrhip_set_scheduler(lrhip_ctx *ctx, uint32_t mode) {
    if (ctx == nullptr || mode > 2u) { return fail(LRHIP_ERROR_INVALID, "lrhip_set_scheduler: invalid argument"); }
    ctx->scheduler = mode;
    return LRHIP_OK;
}

int lrhip_set_wavefront(lrhip_ctx *ctx, uint32_t mode, uint32_t slice_paths) {
    if (ctx == nullptr || (mode & 0xffu) > 2u || (mode >> 24u) != 0u) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_set_wavefront: invalid argument");
    }
    ctx->wf_mode = mode & 0xffu, ctx->wf_slice_paths = slice_paths;
    ctx->diag_wf_carry_rounds = mode >> 8u;// (bits 8-23: rounds before a slice hands its parked paths over; 0 = default, 65535 = never)
    return LRHIP_OK;
}

int lrhip_synchronize(lrhip_ctx *ctx) {
    if (ctx == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_synchronize: ctx is NULL"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return LRHIP_OK;
}

int lrhip_film_download(lrhip_ctx *ctx, float *rgba, int converted) {
    if (ctx == nullptr || rgba == nullptr || !ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_download: invalid argument"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    auto pixel_count = ctx->width * ctx->height;
    auto bytes = static_cast<size_t>(pixel_count) * sizeof(float4);
    const void *src = ctx->film;
    if (converted) {
        hipLaunchKernelGGL(lrd::film_convert_kernel, dim3((pixel_count + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->film,
                           static_cast<float4 *>(ctx->converted.ptr), pixel_count, ctx->film_scale[0], ctx->film_scale[1], ctx->film_scale[2]);
        LR_HIP_CHECK(hipGetLastError());
        src = ctx->converted.ptr;
    }
    LR_HIP_CHECK(hipMemcpyAsync(rgba, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return LRHIP_OK;
}

int lrhip_aov_download(lrhip_ctx *ctx, uint32_t component, float *out) {
    if (ctx == nullptr || out == nullptr || !ctx->scene_ready || component >= LR_AOV_COMPONENTS) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_aov_download: invalid argument");
    }
    const auto off = ctx->scene.aov_offset[component];
    if (off == lrd::kInvalid) { return fail(LRHIP_ERROR_INVALID, "lrhip_aov_download: the component is not enabled in the uploaded scene"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    const auto pixel_count = static_cast<size_t>(ctx->width) * ctx->height;
    const auto channels = kAovChannels[component];
    std::vector<float> planes(pixel_count * channels);
    LR_HIP_CHECK(hipMemcpyAsync(planes.data(), ctx->scene.aov + off * pixel_count, planes.size() * sizeof(float), hipMemcpyDeviceToHost,
        ctx->stream));
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < pixel_count; i++) {
        for (uint32_t c = 0u; c < channels; c++) { out[i * channels + c] = planes[c * pixel_count + i]; }
    }
    return LRHIP_OK;
}

int lrhip_get_counters(lrhip_ctx *ctx, lrhip_counters *out) {
    if (ctx == nullptr || out == nullptr || !ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_get_counters: invalid argument"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    static_assert(sizeof(lrhip_counters) == sizeof(lrd::DCounters), "counter layouts must match");
    LR_HIP_CHECK(hipMemcpy(out, ctx->counters.ptr, sizeof(lrhip_counters), hipMemcpyDeviceToHost));
    return LRHIP_OK;
}

uint32_t lrhip_last_variant(lrhip_ctx *ctx) { return ctx != nullptr ? ctx->last_variant : 0u; }

double lrhip_last_render_ms(lrhip_ctx *ctx) {
    if (ctx == nullptr || !ctx->timed) { return 0.0; }
    if (hipSetDevice(ctx->device) != hipSuccess || hipEventSynchronize(ctx->ev_end) != hipSuccess) { return -1.0; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end) != hipSuccess) { return -1.0; }
    return static_cast<double>(ms);
}

}// extern "C"
