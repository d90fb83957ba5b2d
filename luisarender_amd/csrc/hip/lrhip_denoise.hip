// lrhip_denoise.hip — C ABI of the edge-avoiding a-trous wavelet filter (include/lrhip.h: lrhip_denoise, lrhip_aov_denoise).
// Holds the three kernels of denoise_kernels.h and their launches on the context's stream.
#include "lrhip_internal.h"
#include "denoise_kernels.h"

namespace lrh {

namespace {

constexpr uint64_t kDenoiseMaxPixels = 1ull << 27u;// 32-bit element indices hold three floats per pixel

std::string check_params(const lrhip_denoise_params *p) {
    if (p->iterations < 1u || p->iterations > LRHIP_DENOISE_MAX_ITERATIONS) {
        return "iterations " + std::to_string(p->iterations) + " is outside 1 .. " + std::to_string(LRHIP_DENOISE_MAX_ITERATIONS);
    }
    for (auto sigma : {p->sigma_color, p->sigma_normal, p->sigma_depth}) {
        if (!(sigma > 0.f) || !std::isfinite(sigma)) { return "the sigmas must be positive and finite"; }
    }
    if ((p->flags & ~LRHIP_DENOISE_DEMODULATE) != 0u) { return "unknown flags"; }
    return {};
}

// prepare -> `iterations` passes -> finish, on the context's stream.  The inputs are device pointers laid out as `layout` says; the
// interleaved rgb result lands in the colour buffer the last pass did not write (16 bytes per pixel hold its 12) and is copied to `out`.
int run_filter(lrhip_ctx *ctx, const lrhip_denoise_params *p, uint32_t width, uint32_t height, const float *color, const float *albedo,
               const float *normal, const float *depth, lrd::DenoiseLayout layout, float scale, float *out) {
    const auto pixel_count = width * height;
    const auto record_bytes = static_cast<size_t>(pixel_count) * sizeof(float4);
    if (auto rc = ensure(ctx->denoise_guide, record_bytes); rc != LRHIP_OK) { return rc; }
    for (auto &b : ctx->denoise_colour) {
        if (auto rc = ensure(b, record_bytes); rc != LRHIP_OK) { return rc; }
    }
    if (ctx->denoise_begin == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->denoise_begin)); }
    if (ctx->denoise_end == nullptr) { LR_HIP_CHECK(hipEventCreate(&ctx->denoise_end)); }
    const auto guide = static_cast<float4 *>(ctx->denoise_guide.ptr);
    float4 *colour[2] = {static_cast<float4 *>(ctx->denoise_colour[0].ptr), static_cast<float4 *>(ctx->denoise_colour[1].ptr)};
    const auto demodulate = p->flags & LRHIP_DENOISE_DEMODULATE;
    const dim3 linear_grid((pixel_count + 255u) / 256u), linear_block(256);
    ctx->denoise_timed = false;
    LR_HIP_CHECK(hipEventRecord(ctx->denoise_begin, ctx->stream));
    hipLaunchKernelGGL(lrd::denoise_prepare_kernel, linear_grid, linear_block, 0, ctx->stream, colour[0], guide, color, albedo, normal, depth,
                       layout, pixel_count, scale, demodulate);
    LR_HIP_CHECK(hipGetLastError());
    const dim3 tile_grid((width + lrd::kDenoiseTile - 1u) / lrd::kDenoiseTile, (height + lrd::kDenoiseTile - 1u) / lrd::kDenoiseTile);
    const dim3 tile_block(lrd::kDenoiseTile, lrd::kDenoiseTile);
    const auto sigma_normal = std::max(p->sigma_normal, lrd::kDenoiseScaleMin);
    auto src = 0u;
    for (auto i = 0u; i < p->iterations; i++, src ^= 1u) {
        hipLaunchKernelGGL(lrd::denoise_pass_kernel, tile_grid, tile_block, 0, ctx->stream, colour[src ^ 1u], colour[src], guide,
                           static_cast<int>(width), static_cast<int>(height), 1 << i, std::ldexp(p->sigma_color, -static_cast<int>(i)),
                           1.f / (sigma_normal * sigma_normal), p->sigma_depth);
        LR_HIP_CHECK(hipGetLastError());
    }
    const auto rgb = reinterpret_cast<float *>(colour[src ^ 1u]);
    hipLaunchKernelGGL(lrd::denoise_finish_kernel, linear_grid, linear_block, 0, ctx->stream, rgb, colour[src], albedo, layout, pixel_count,
                       scale, demodulate);
    LR_HIP_CHECK(hipGetLastError());
    LR_HIP_CHECK(hipEventRecord(ctx->denoise_end, ctx->stream));
    ctx->denoise_timed = true;
    LR_HIP_CHECK(hipMemcpyAsync(out, rgb, static_cast<size_t>(pixel_count) * 3u * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return LRHIP_OK;
}

}// namespace

}// namespace lrh

using namespace lrh;

extern "C" {

void lrhip_denoise_default_params(lrhip_denoise_params *params) {
    if (params == nullptr) { return; }
    *params = lrhip_denoise_params{0u, 0u, LRHIP_DENOISE_DEFAULT_ITERATIONS, LRHIP_DENOISE_DEMODULATE, LRHIP_DENOISE_DEFAULT_SIGMA_COLOR,
                                   LRHIP_DENOISE_DEFAULT_SIGMA_NORMAL, LRHIP_DENOISE_DEFAULT_SIGMA_DEPTH};
}

int lrhip_denoise(lrhip_ctx *ctx, const lrhip_denoise_params *params, const float *color, const float *albedo, const float *normal,
                  const float *depth, float *out) {
    if (ctx == nullptr || params == nullptr || color == nullptr || albedo == nullptr || normal == nullptr || depth == nullptr || out == nullptr) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_denoise: NULL argument");
    }
    if (params->width == 0u || params->height == 0u || static_cast<uint64_t>(params->width) * params->height > kDenoiseMaxPixels) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_denoise: width x height must be 1 .. 2^27 pixels");
    }
    if (auto error = check_params(params); !error.empty()) { return fail(LRHIP_ERROR_INVALID, "lrhip_denoise: " + error); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    // the host arrays, one behind the other: color, albedo, normal (3 floats per pixel each), depth (1)
    const auto n = static_cast<size_t>(params->width) * params->height;
    if (auto rc = ensure(ctx->denoise_inputs, n * 10u * sizeof(float)); rc != LRHIP_OK) { return rc; }
    const auto inputs = static_cast<float *>(ctx->denoise_inputs.ptr);
    const float *host[4] = {color, albedo, normal, depth};
    for (auto k = 0u; k < 4u; k++) {
        LR_HIP_CHECK(hipMemcpyAsync(inputs + n * 3u * k, host[k], n * (k < 3u ? 3u : 1u) * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    return run_filter(ctx, params, params->width, params->height, inputs, inputs + n * 3u, inputs + n * 6u, inputs + n * 9u,
                      lrd::DenoiseLayout{3u, 1u}, 1.f, out);
}

int lrhip_aov_denoise(lrhip_ctx *ctx, const lrhip_denoise_params *params, uint32_t component, uint32_t samples, float *out) {
    if (ctx == nullptr || params == nullptr || out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_aov_denoise: NULL argument"); }
    if (!ctx->scene_ready || ctx->scene.aov_channels == 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_aov_denoise: no AOV scene uploaded"); }
    if (component != LR_AOV_SAMPLE && component != LR_AOV_DIFFUSE && component != LR_AOV_SPECULAR) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_aov_denoise: the component must be sample, diffuse or specular");
    }
    if (samples == 0u) { return fail(LRHIP_ERROR_INVALID, "lrhip_aov_denoise: samples is 0"); }
    if ((params->width != 0u && params->width != ctx->width) || (params->height != 0u && params->height != ctx->height)) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_aov_denoise: width / height differ from the uploaded scene's");
    }
    if (static_cast<uint64_t>(ctx->width) * ctx->height > kDenoiseMaxPixels) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_aov_denoise: more than 2^27 pixels");
    }
    if (auto error = check_params(params); !error.empty()) { return fail(LRHIP_ERROR_INVALID, "lrhip_aov_denoise: " + error); }
    static const char *const kNames[LR_AOV_COMPONENTS] = {"sample", "diffuse", "specular", "normal", "albedo", "depth", "roughness", "ndc", "mask"};
    const auto pixel_count = static_cast<size_t>(ctx->width) * ctx->height;
    const float *planes[4]{};
    const uint32_t needed[4] = {component, LR_AOV_ALBEDO, LR_AOV_NORMAL, LR_AOV_DEPTH};
    for (auto k = 0u; k < 4u; k++) {
        const auto off = ctx->scene.aov_offset[needed[k]];
        if (off == lrd::kInvalid) {
            return fail(LRHIP_ERROR_INVALID, std::string{"lrhip_aov_denoise: the component '"} + kNames[needed[k]] + "' is not enabled in the uploaded scene");
        }
        planes[k] = ctx->scene.aov + off * pixel_count;
    }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    return run_filter(ctx, params, ctx->width, ctx->height, planes[0], planes[1], planes[2], planes[3],
                      lrd::DenoiseLayout{1u, static_cast<uint32_t>(pixel_count)}, static_cast<float>(1.0 / static_cast<double>(samples)), out);
}

double lrhip_last_denoise_ms(lrhip_ctx *ctx) {
    if (ctx == nullptr || !ctx->denoise_timed) { return 0.0; }
    if (hipSetDevice(ctx->device) != hipSuccess || hipEventSynchronize(ctx->denoise_end) != hipSuccess) { return -1.0; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->denoise_begin, ctx->denoise_end) != hipSuccess) { return -1.0; }
    return static_cast<double>(ms);
}

}// extern "C"
