// camera_kernel.h — camera, sampler and film queries (include/lrhip.h: lrhip_query_sampler, lrhip_query_camera, lrhip_film_splat):
// the three ends of a render that the megakernels keep to themselves -- the scene's sampler streams with their state made explicit, the
// camera ray of a pixel for the random numbers the caller gives, and the film's accumulate rule for the caller's values -- so that a whole
// lrhip_render can be written as a loop over queries.
//
// One lane per record, no LDS, no queue, as light_kernel.h: the lane loads its 16-byte record(s) as dwordx4, checks every index BEFORE it
// is used, and then makes exactly the calls the renderers make (megapath_kernel.h: PathSampler<>::start / next_pixel_2d / next_2d /
// next_1d with save / restore around them; camera_ray; film_accumulate on the pixel in the film).  This file holds no sampling, camera or
// accumulate arithmetic of its own.  What it adds is screening: a state the caller damaged is brought back into the range the draws can
// index (sampler_screen), a pixel id beyond the frame or a non-finite number gives the invalid record or is skipped.
#pragma once
#include "dev_wavefront.h"
#include "raycast_kernel.h"

namespace lrd {

enum : uint32_t { kDraw1d = 0u, kDraw2d = 1u, kDrawPixel2d = 2u };// lrhip.h: LRHIP_DRAW_*
constexpr uint32_t kSamplerMaxDraws = 64u;                        // lrhip.h: LRHIP_SAMPLER_MAX_DRAWS

struct SamplerArgs {
    uint4 *state;           // [count]: the words PathSampler<>::save writes; read unless `start`, always written
    const uint32_t *streams;// start: stream id of each record, or nullptr: record k has stream stream_base + k
    const uint32_t *indices;// start: sample index of each record, or nullptr: sample_index
    float *out;             // [count][floats], row-major; not touched when floats == 0
    uint32_t count;
    uint32_t stream_base;   // (a host-pointer call goes through the staging buffers chunk by chunk: the chunk's first record)
    uint32_t sample_index;
    uint32_t start;         // LRHIP_SAMPLER_START
    uint32_t draws;         // <= kSamplerMaxDraws
    uint32_t floats;        // per record: the draws' 1 or 2 each
    // the pattern by value, wave-uniform: draw i is the two bits (i & 31) * 2 of word i >> 5
    unsigned long long pattern[2];
};

// A state word the draws would index a table with, brought into the table's range: a state that save() wrote passes unchanged.
//   Sobol        the dimension w2 indexes sobol_bytes [LR_SOBOL_DIMENSIONS]; next_1d wraps at >= and next_2d at + 1 >=, so any value beyond
//                is the same as LR_SOBOL_DIMENSIONS itself.  The sequence index has LR_SOBOL_MATRIX_SIZE bits: its high word's table walk
//                stays inside the dimension's rows
//   PaddedSobol  permutation_element's cycle walk ends for an index below the length; with a length that is no power of two an index at
//                or beyond it need not, so it is folded back (a power of two masks the index itself: padded_sobol.cpp:59-91)
LR_D void sampler_screen(const DScene &scene, PathSampler<true> &s) {
    if (scene.sampler_kind == LR_SAMPLER_SOBOL) {
        s.w2 = min(s.w2, static_cast<uint32_t>(LR_SOBOL_DIMENSIONS));
        s.hi &= (1u << (static_cast<uint32_t>(LR_SOBOL_MATRIX_SIZE) - 32u)) - 1u;
    } else if (scene.sampler_kind == LR_SAMPLER_PADDED_SOBOL) {
        const auto l = scene.sampler_spp;
        if ((l & (l - 1u)) != 0u && s.lo >= l) { s.lo %= l; }
    }
}
LR_D void sampler_screen(const DScene &, PathSampler<false> &) {}

// GENERIC = false: the Independent sampler (one state word; the other three are written 0); true: PCG32 / Sobol / PaddedSobol at run time
// -- the split the renderers make (megapath_kernel.h: PCG)
template<bool GENERIC>
__global__ __launch_bounds__(kBlockThreads) void sampler_kernel(DScenePtr scene_ptr, SamplerArgs args) {
    const DScene &scene = *(const DScene *)scene_ptr;
    const auto stride = gridDim.x * kBlockThreads;
    for (auto k = blockIdx.x * kBlockThreads + threadIdx.x; k < args.count; k += stride) {
        PathSampler<GENERIC> sampler{};
        if (args.start != 0u) {// as Li starts the stream of pixel (j mod W, (j div W) mod H) at sample s (megapath_kernel.h)
            const auto j = args.streams != nullptr ? args.streams[k] : args.stream_base + k;
            const auto s = args.indices != nullptr ? args.indices[k] : args.sample_index;
            sampler.start(scene, j % scene.camera.width, (j / scene.camera.width) % scene.camera.height, s);
        } else {
            const auto w = args.state[k];
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
            sampler.restore(scene, words);
        }
        sampler_screen(scene, sampler);
        auto row = args.out + static_cast<size_t>(k) * args.floats;
        for (auto i = 0u; i < args.draws; i++) {// wave-uniform
            const auto code = static_cast<uint32_t>(args.pattern[i >> 5u] >> ((i & 31u) * 2u)) & 3u;
            if (code == kDraw1d) {
                *row++ = sampler.next_1d();
            } else {
                const auto u = code == kDraw2d ? sampler.next_2d() : sampler.next_pixel_2d();
                row[0] = u.x, row[1] = u.y;
                row += 2;
            }
        }
        uint32_t words[4] = {0u, 0u, 0u, 0u};
        (void)sampler.save(words);
        args.state[k] = make_uint4(words[0], words[1], words[2], words[3]);
    }
}

struct CameraArgs {
    const uint32_t *pixels;// pixel id py * W + px of each record, or nullptr: record k is pixel pixel_base + k
    const float4 *u;       // [count]: (u_filter.x, u_filter.y, u_lens.x, u_lens.y)
    float4 *out_rays;      // lrhip_ray[count], two float4 each
    float4 *out;           // lrhip_camera_sample[count]: (weight, film_x, film_y, pixel)
    uint32_t count;
    uint32_t pixel_base;
};

__global__ __launch_bounds__(kBlockThreads) void camera_kernel(DScenePtr scene_ptr, CameraArgs args) {
    const DScene &scene = *(const DScene *)scene_ptr;
    const auto stride = gridDim.x * kBlockThreads;
    const auto width = scene.camera.width, pixel_count = width * scene.camera.height;// (at most 65535 x 65535: lrhip_upload_scene)
    const auto thin_lens = scene.camera.kind == LR_CAMERA_THIN_LENS;
    const auto zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (auto k = blockIdx.x * kBlockThreads + threadIdx.x; k < args.count; k += stride) {
        const auto id = args.pixels != nullptr ? args.pixels[k] : args.pixel_base + k;
        const auto q = args.u[k];
        const auto rays = args.out_rays + static_cast<size_t>(k) * 2u;
        // the lens pair is read by the thin lens only: another camera does not look at it
        const auto valid = id < pixel_count && raycast_finite(q.x) && raycast_finite(q.y) && (!thin_lens || (raycast_finite(q.z) && raycast_finite(q.w)));
        if (!valid) {// the invalid record: a zero ray, weight 0, pixel LR_INVALID_ID
            rays[0] = zero, rays[1] = zero;
            args.out[k] = make_float4(0.f, 0.f, 0.f, __uint_as_float(kInvalid));
            continue;
        }
        const auto py = id / width, px = id - py * width;
        const f2 u_filter{q.x, q.y};
        Ray ray{};
        float weight;
        camera_ray(scene, scene.filter, px, py, u_filter, thin_lens ? f2{q.z, q.w} : f2{.5f, .5f}, ray, weight);
        // camera_sample.pixel: the filter's offset once more, same arithmetic (as the AOV kernel takes it, megapath_kernel.h)
        f2 off;
        float fw;
        filter_sample(scene.filter, u_filter, off, fw);
        rays[0] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.t_min);
        rays[1] = make_float4(ray.d.x, ray.d.y, ray.d.z, ray.t_max);
        args.out[k] = make_float4(weight, static_cast<float>(px) + .5f + off.x, static_cast<float>(py) + .5f + off.y, __uint_as_float(id));
    }
}

struct SplatArgs {
    const uint32_t *pixels;// as CameraArgs
    const float4 *values;  // [count]: (r, g, b, ignored)
    float4 *film;          // the film the context accumulates into
    uint32_t count;
    uint32_t pixel_base;
    float clamp;
};

__global__ __launch_bounds__(kBlockThreads) void splat_kernel(DScenePtr scene_ptr, SplatArgs args) {
    const DScene &scene = *(const DScene *)scene_ptr;
    const auto stride = gridDim.x * kBlockThreads;
    const auto pixel_count = scene.camera.width * scene.camera.height;
    for (auto k = blockIdx.x * kBlockThreads + threadIdx.x; k < args.count; k += stride) {
        const auto id = args.pixels != nullptr ? args.pixels[k] : args.pixel_base + k;
        const auto v = args.values[k];
        if (id < pixel_count) { film_accumulate(args.film + id, mk3(v.x, v.y, v.z), args.clamp); }// color.cpp:107-130
    }
}

}// namespace lrd
