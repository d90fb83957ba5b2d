// denoise_kernels.h — the edge-avoiding a-trous wavelet filter over the AOV integrator's buffers (Dammertz et al. 2010; the definition:
// include/lrhip.h).  Included by lrhip_denoise.hip only.  Three kernels: prepare (demodulate, pack into 16-byte records),
// pass (one launch per iteration over two ping-pong colour buffers), finish (re-modulate, interleaved rgb).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lrd {

constexpr uint32_t kDenoiseTile = 16u;    // a block of the pass kernel: 16 x 16 pixels, four waves of 16 x 4
constexpr float kDenoiseAlbedoMin = 1e-3f;// a channel's albedo at or below it is not divided out
constexpr float kDenoiseEps = 1e-4f;      // added to the colour's and the depth's scale
constexpr float kDenoiseScaleMin = 1e-18f;// floor of sigma x scale: its square stays a normal float

// Where the inputs lie: value (pixel i, channel ch) at [i * pixel_stride + ch * channel_stride] -- interleaved host arrays (3, 1) or the
// planar sums of the AOV integrator (1, pixel count).  Depth is one float per pixel either way.
struct DenoiseLayout {
    uint32_t pixel_stride, channel_stride;
};

__device__ inline float denoise_albedo(const float *albedo, DenoiseLayout l, uint32_t i, uint32_t ch, float scale, uint32_t demodulate) {
    if (demodulate == 0u) { return 1.f; }
    const auto a = albedo[i * l.pixel_stride + ch * l.channel_stride] * scale;
    return a > kDenoiseAlbedoMin ? a : 1.f;
}

// colour[i] = { u_0.rgb, 0 }, guide[i] = { N.xyz, z }: every input times `scale` (1 / samples for sums, 1 for means), then u_0 = c / a'
__global__ void denoise_prepare_kernel(float4 *__restrict__ colour, float4 *__restrict__ guide, const float *__restrict__ c,
                                       const float *__restrict__ albedo, const float *__restrict__ normal, const float *__restrict__ depth,
                                       DenoiseLayout l, uint32_t pixel_count, float scale, uint32_t demodulate) {
    const auto i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixel_count) { return; }
    float u[3], n[3];
    for (auto ch = 0u; ch < 3u; ch++) {
        u[ch] = c[i * l.pixel_stride + ch * l.channel_stride] * scale / denoise_albedo(albedo, l, i, ch, scale, demodulate);
        n[ch] = normal[i * l.pixel_stride + ch * l.channel_stride] * scale;
    }
    colour[i] = make_float4(u[0], u[1], u[2], 0.f);
    guide[i] = make_float4(n[0], n[1], n[2], depth[i] * scale);
}

// One pass: out(p) = sum_q w(p, q) in(q) / sum_q w(p, q) over the 5 x 5 taps q = p + step (dx, dy) inside the image, in row-major order
// of (dy, dx).  One lane per pixel; every tap but the centre is two 16-byte loads (L2 / Infinity Cache: 32 bytes per pixel are read 25
// times) and one hardware exponential.  The centre tap has d = 0 by definition and comes from the registers.
#ifdef LR_DENOISE_WAVES// A/B builds (make hip-variant DEFS=-DLR_DENOISE_WAVES=4): waves per SIMD the register allocation aims at
__attribute__((amdgpu_waves_per_eu(LR_DENOISE_WAVES, LR_DENOISE_WAVES)))
#endif
__global__ void __launch_bounds__(kDenoiseTile *kDenoiseTile)
    denoise_pass_kernel(float4 *__restrict__ out, const float4 *__restrict__ in, const float4 *__restrict__ guide, int width, int height,
                        int step, float sigma_color, float inv_sigma_normal2, float sigma_depth) {
    const auto x = static_cast<int>(blockIdx.x * kDenoiseTile + threadIdx.x), y = static_cast<int>(blockIdx.y * kDenoiseTile + threadIdx.y);
    if (x >= width || y >= height) { return; }
    const auto p = static_cast<uint32_t>(y) * static_cast<uint32_t>(width) + static_cast<uint32_t>(x);
    const auto up = in[p], gp = guide[p];
    // (the floor keeps 1 / scale^2 finite under any sigma > 0, so that an equal pair never meets 0 x inf)
    const auto sc = fmaxf(sigma_color * ((up.x + up.y + up.z) / 3.f + kDenoiseEps), kDenoiseScaleMin);
    const auto sz = fmaxf(sigma_depth * (fabsf(gp.w) + kDenoiseEps), kDenoiseScaleMin);
    const auto inv_c2 = 1.f / (sc * sc), inv_z2 = 1.f / (sz * sz);
    constexpr float k[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
#pragma unroll
    for (auto dy = -2; dy <= 2; dy++) {
        const auto qy = y + dy * step;
#pragma unroll
        for (auto dx = -2; dx <= 2; dx++) {
            const auto qx = x + dx * step;
            const auto h = k[dx + 2] * k[dy + 2];
            if (dx == 0 && dy == 0) {
                sr += h * up.x, sg += h * up.y, sb += h * up.z, sw += h;
                continue;
            }
            // a tap outside the image is skipped: it reads the centre instead and weighs 0, so that no load waits for a branch
            const auto inside = qx >= 0 && qx < width && qy >= 0 && qy < height;
            const auto q = inside ? static_cast<uint32_t>(qy) * static_cast<uint32_t>(width) + static_cast<uint32_t>(qx) : p;
            const auto uq = in[q], gq = guide[q];
            const auto cr = up.x - uq.x, cg = up.y - uq.y, cb = up.z - uq.z;
            const auto nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z, dz = gp.w - gq.w;
            const auto d = (cr * cr + cg * cg + cb * cb) * inv_c2 + (nx * nx + ny * ny + nz * nz) * inv_sigma_normal2 + dz * dz * inv_z2;
            const auto w = (inside ? h : 0.f) * __expf(-d);// exp(-d) is in [0, 1] (NaN only from NaN inputs)
            sr += w * uq.x, sg += w * uq.y, sb += w * uq.z, sw += w;
        }
    }
    const auto inv = 1.f / sw;// sw >= 9 / 64: the centre tap
    out[p] = make_float4(sr * inv, sg * inv, sb * inv, 0.f);
}

// rgb[i] = u_K(i) a'(i), three interleaved floats per pixel
__global__ void denoise_finish_kernel(float *__restrict__ rgb, const float4 *__restrict__ colour, const float *__restrict__ albedo,
                                      DenoiseLayout l, uint32_t pixel_count, float scale, uint32_t demodulate) {
    const auto i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixel_count) { return; }
    const auto u = colour[i];
    rgb[i * 3u] = u.x * denoise_albedo(albedo, l, i, 0u, scale, demodulate);
    rgb[i * 3u + 1u] = u.y * denoise_albedo(albedo, l, i, 1u, scale, demodulate);
    rgb[i * 3u + 2u] = u.z * denoise_albedo(albedo, l, i, 2u, scale, demodulate);
}

}// namespace lrd
