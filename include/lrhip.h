/* lrhip.h — thin C ABI of the MI355X (gfx950) megakernel path tracer (liblrhip.so).
 *
 * This is the drop-in boundary of the hot path.  The reference has no such C interface: its
 * MegaPath integrator is a C++ plugin (`create`/`destroy`, src/base/scene_node.h:58-67) whose
 * Instance::render JIT-compiles and launches a LuisaCompute kernel.  Each entry point below
 * replaces one step of that path; the reference-side binding a maintainer would add lives in
 * INTEGRATION.md and luisarender_amd/csrc/host/plugin_megapath.cpp.
 *
 *   lrhip_create / lrhip_destroy   Context::create_device + Stream       src/apps/cli.cpp:166-172,181
 *   lrhip_upload_scene             Pipeline::create uploads               src/base/pipeline.cpp:44-99,
 *                                  Geometry::build                        src/base/geometry.cpp:12-27
 *   lrhip_update_scene             Pipeline::update / Geometry::update    src/base/pipeline.cpp:101-113, geometry.cpp:194-216
 *   lrhip_film_clear               ColorFilmInstance::prepare/clear       src/films/color.cpp:132-144
 *   lrhip_render                   _render_one_camera's spp loop of       src/base/integrator.cpp:86-107
 *                                  render(sample_id, time, weight).dispatch(resolution), i.e.
 *                                  Li() + film accumulate                 src/integrators/mega_path.cpp:49-156
 *   lrhip_film_download            ColorFilmInstance::download            src/films/color.cpp:99-105
 *   lrhip_film_reduce              (no reference equivalent: the one collective of the multi-GPU path)
 *   lrhip_trace_rays               (no reference entry point: Geometry::trace_closest / trace_any for the caller's rays)
 *   lrhip_trace_radiance           (no reference entry point: MegakernelPathTracingInstance::Li for the caller's rays)
 *   lrhip_query_surface            (no reference entry point: Geometry::shading_point, the closure's albedo / roughness and the light's emission
 *                                  at the caller's hits)
 *   lrhip_query_bsdf               (no reference entry point: Surface::Closure::evaluate / sample at the caller's hits)
 *   lrhip_query_light              (no reference entry point: LightSampler::Instance::sample / evaluate_hit / evaluate_miss at the caller's hits,
 *                                  DESIGN §4.15)
 *   lrhip_query_sampler            (no reference entry point: Sampler::Instance::start / generate_1d / generate_2d / generate_pixel_2d with the
 *                                  state in the caller's hands)
 *   lrhip_query_camera             (no reference entry point: Camera::Instance::generate_ray for the caller's pixels and numbers)
 *   lrhip_film_splat               (no reference entry point: ColorFilmInstance::_accumulate for the caller's values)
 *   lrhip_set_instance_transforms  (Geometry::update for matrices the caller holds, computed on the device)
 *   lrhip_set_mesh_vertices        (no reference equivalent: new vertex positions for one mesh, re-baked and refitted on the device)
 *   lrhip_get_counters             (no reference equivalent; roofline accounting)
 *
 * Conventions: 0 = OK, negative = error (text via lrhip_last_error, thread-local); nothing
 * throws or aborts across the boundary.  One context per GPU; a context is not thread-safe;
 * different contexts may be driven from different host threads / processes.  All buffers are
 * POD, little-endian, laid out as in lr_scene.h.  The library copies what it needs during
 * lrhip_upload_scene; the caller keeps ownership of the scene tables.
 */
#ifndef LRHIP_H
#define LRHIP_H

#include "lr_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrhip_ctx lrhip_ctx;

#define LRHIP_OK 0
#define LRHIP_ERROR_INVALID (-1)  /* bad argument / state        */
#define LRHIP_ERROR_DEVICE (-2)   /* HIP runtime failure         */
#define LRHIP_ERROR_UNSUPPORTED (-3)

/* Work of one lrhip_render call: samples [spp_begin, spp_end) of every pixel of the screen tiles
 * {tile_begin + k * tile_stride : tile_begin + k * tile_stride < tile_end}.  Tiles are 8x8 pixels; tile number
 * t = ty * tiles_x + j names the tile in row ty whose column is (j + ty) mod tiles_x (tiles_x = ceil(W/8)): every row is
 * rotated by its index, so that a strided shard (rank, tile_count, world) is a set of DIAGONALS of the frame, never a set
 * of columns (tiles_x is a multiple of the world size for every power-of-two frame).  Every tile has exactly one number,
 * so any partition of [0, tile_count) partitions the frame.  (0, tile_count, 1) renders the whole frame; (rank, tile_count,
 * world) is the interleaved screen-tile shard of one GPU; tile_begin >= tile_end is an empty shard (no error). */
typedef struct lrhip_render_params {
    uint32_t spp_begin, spp_end;
    uint32_t tile_begin, tile_end, tile_stride;
    uint32_t flags;          /* LRHIP_RENDER_* */
    /* Work-item sizing hint: the number of shards the frame is split into (0 = 1).  A frame is cut into
     * (tile, sample-chunk) items whose size balances the drain at the end of every item against the tail of the
     * launch; a 1/W shard has W times fewer tiles per GPU and wants smaller items (item size ~ sqrt(tiles per shard)).  The chunking —
     * and with it the fp32 summation order of the film — is a function of (resolution, spp, balance_shards) ONLY:
     * renders that pass the same value are bit-identical under any tile sharding and on any device.            */
    uint32_t balance_shards;
    /* Camera::ShutterSample weight of these samples (src/base/integrator.cpp:74,91-95: film()->accumulate(pixel,
     * shutter_weight * L)); read only when flags has LRHIP_RENDER_SHUTTER_WEIGHT, otherwise 1 */
    float shutter_weight;
} lrhip_render_params;

#define LRHIP_RENDER_COUNTERS 1u /* gather per-ray node/triangle counters (slower kernel variant) */
#define LRHIP_RENDER_SHUTTER_WEIGHT 2u /* lrhip_render_params.shutter_weight is valid */

typedef struct lrhip_counters {
    uint64_t paths, closest_rays, shadow_rays;
    uint64_t nodes_visited;  /* quantised BVH4 packets fetched (64 B each)   */
    uint64_t tris_tested;    /* triangle tests (48 B each)                   */
    uint64_t surface_hits, nee_samples, path_length_sum;
    /* SIMD-occupancy diagnostics: lane-iterations of the traversal loop (all lanes of every wave) and the
     * ones in which the lane had a ray in flight; shading blocks executed per lane / with a hit to shade */
    uint64_t trace_steps, trace_steps_busy, shade_calls, shade_busy;
    uint64_t trace_steps_starved; /* lane-steps idle because the lane had no sample left to start */
    /* wave-cycle diagnostics (s_memtime, summed over waves): inside the shading block (A), inside the traversal
     * loop (B), and from a wave's first to its last instruction */
    uint64_t shade_cycles, trace_cycles, wave_cycles;
    uint64_t nodes_empty;    /* node visits in which no child was hit (popped after the ray had already shortened, or plain misses) */
    /* wave cycles of three sections of the shading block: hit reconstruction + emission + light sample, closure evaluate + sample +
     * Russian roulette, path regeneration (camera rays); the remainder of shade_cycles is queue bookkeeping and ray launch */
    uint64_t shade_light_cycles, shade_closure_cycles, shade_regen_cycles;
    /* round 6: section cycles of the traversal loop and the shading block from the stall-probe build of the counting kernels
     * (make hip-variant DEFS=-DLR_STALL_PROBE, tools/stall_probe.py; slot names there); zero in the shipped library */
    uint64_t probe[16];
} lrhip_counters;

int lrhip_create(int device_ordinal, lrhip_ctx **out);
void lrhip_destroy(lrhip_ctx *ctx);

/* optional: launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL = own stream */
int lrhip_set_stream(lrhip_ctx *ctx, void *hip_stream);

/* scene->accel must be built (lrhost_scene_build_accel) */
int lrhip_upload_scene(lrhip_ctx *ctx, const lr_scene *scene);

/* Pipeline::update (src/base/pipeline.cpp:101-113) for the next shutter sample of a motion-blurred frame: `scene` must be the
 * uploaded scene moved to another time (lrhost_scene_set_time).  Only what moves is copied again, over the same device buffers
 * and in stream order — instance matrices, the re-baked triangles and their shading records, the refitted BVH packets, camera and
 * environment transforms — while textures, environment tables, materials, the film, its binding and the counters stay.  Table
 * sizes and BVH topology are checked against the upload; anything else that differs is the caller's error.                      */
int lrhip_update_scene(lrhip_ctx *ctx, const lr_scene *scene);

/* optional: accumulate into a caller-owned device buffer float4[W*H] (e.g. a torch tensor that
 * RCCL reduces afterwards); NULL = library-owned film (default) */
int lrhip_bind_film(lrhip_ctx *ctx, void *device_float4_film);
int lrhip_film_clear(lrhip_ctx *ctx);

/* asynchronous on the context's stream */
int lrhip_render(lrhip_ctx *ctx, const lrhip_render_params *params);
int lrhip_synchronize(lrhip_ctx *ctx);

/* converted != 0: (sum.rgb / max(sum.w, 1)) * 2^exposure, alpha 1 (color.cpp:87-93);
 * converted == 0: the raw (sum r, sum g, sum b, n) film.  Synchronises.              */
int lrhip_film_download(lrhip_ctx *ctx, float *rgba, int converted);

/* The AOV integrator (LR_INTEGRATOR_AOV, src/integrators/aov.cpp): the raw per-pixel sums of one component (LR_AOV_*, lr_scene.h),
 * W x H x channels floats, row 0 at the top, channels interleaved (3 for every component but depth and mask; roughness is (rx, ry, 0)).
 * Divide by the sample count for the reference's images.  The buffers of the enabled components are allocated by lrhip_upload_scene
 * and cleared with the film by lrhip_film_clear; an AOV scene leaves the film itself untouched.  Synchronises.               */
int lrhip_aov_download(lrhip_ctx *ctx, uint32_t component, float *out);

/* The edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; DESIGN §4.8 holds the definition) over per-pixel MEANS of colour c,
 * albedo a, normal N and depth z.  With LRHIP_DENOISE_DEMODULATE, per channel a' = a where a > 1e-3 and 1 elsewhere (without it a' = 1),
 * u_0 = c / a'; pass i = 0 .. iterations-1 has step s = 2^i and sigma_color * 2^-i, taps q = p + s (dx, dy), dx, dy in -2 .. 2, those
 * outside the image skipped, weights k[dx+2] k[dy+2] exp(-d), k = (1/16, 1/4, 3/8, 1/4, 1/16),
 *   d = |u(p)-u(q)|^2 / (sigma_color_i r(p))^2 + |N(p)-N(q)|^2 / sigma_normal^2 + (z(p)-z(q))^2 / (sigma_depth (|z(p)| + 1e-4))^2,
 *   r(p) = mean of u(p)'s channels + 1e-4;  u_{i+1}(p) = sum w u_i(q) / sum w;  the output is u_iterations a'.
 * Pixels that see only the environment (N = 0, z = 0, a = 0) mix among themselves.  The reference has no denoiser of its own (it leaves
 * denoising to a LuisaCompute extension).  The working buffers (48 bytes per pixel) belong to the context and grow on demand. */
typedef struct lrhip_denoise_params {
    uint32_t width, height; /* lrhip_aov_denoise: 0 = the uploaded scene's; anything else must match it */
    uint32_t iterations;    /* 1 .. LRHIP_DENOISE_MAX_ITERATIONS */
    uint32_t flags;         /* LRHIP_DENOISE_* */
    float sigma_color, sigma_normal, sigma_depth; /* each > 0 */
} lrhip_denoise_params;
#define LRHIP_DENOISE_DEMODULATE 1u
#define LRHIP_DENOISE_MAX_ITERATIONS 8u
#define LRHIP_DENOISE_DEFAULT_ITERATIONS 5u
#define LRHIP_DENOISE_DEFAULT_SIGMA_COLOR 0.9f
#define LRHIP_DENOISE_DEFAULT_SIGMA_NORMAL 0.35f
#define LRHIP_DENOISE_DEFAULT_SIGMA_DEPTH 0.1f
/* width = height = 0, the defaults above, LRHIP_DENOISE_DEMODULATE set */
void lrhip_denoise_default_params(lrhip_denoise_params *params);
/* Host arrays, interleaved as lrhip_aov_download gives them (color, albedo, normal, out: W x H x 3; depth: W x H), already divided by
 * their sample counts.  Needs no uploaded scene: a MegaPath film is denoised with the guides of a short AOV run this way.  Synchronises. */
int lrhip_denoise(lrhip_ctx *ctx, const lrhip_denoise_params *params, const float *color, const float *albedo, const float *normal,
                  const float *depth, float *out);
/* The same kernels on the device-resident sums of the uploaded AOV scene, without a trip through the host: `component` (LR_AOV_SAMPLE,
 * LR_AOV_DIFFUSE or LR_AOV_SPECULAR) filtered under the scene's albedo, normal and depth, every sum times 1.0f / samples (the float
 * product MegaPathRenderer.download_aov forms); out: W x H x 3.  LRHIP_ERROR_INVALID when one of the four components is not enabled.
 * For whole frames: a context that rendered a tile shard holds the sums of its tiles only.  Synchronises. */
int lrhip_aov_denoise(lrhip_ctx *ctx, const lrhip_denoise_params *params, uint32_t component, uint32_t samples, float *out);
/* HIP-event time of the kernels (prepare, the passes, finish) of the last lrhip_denoise / lrhip_aov_denoise call, in ms */
double lrhip_last_denoise_ms(lrhip_ctx *ctx);

/* Ray queries: closest hit or occlusion for caller-supplied rays against the scene of the last lrhip_upload_scene /
 * lrhip_update_scene, on the renderers' own traversal loop.  The reference has no such entry point (its Geometry::trace_closest /
 * trace_any are only reachable from inside a kernel, src/base/geometry.cpp:218-279).  Camera, integrator and sampler play no part;
 * LRHIP_ERROR_INVALID before any scene has been uploaded.
 *   What can be hit   the baked BVH triangles of VISIBLE instances (lr_instance.visible, baked flag bit 0), exactly as in the renderer.
 *   A hit             has max(t_min, +0) < t < t_max, both strict; t_max = +inf is allowed.  The search never reaches behind the origin:
 *                     t_min = -0.0 or a negative t_min searches from +0, and a ray whose t_max is not above +0 finds nothing.
 *                     Directions need not be normalised: t, t_min and t_max are in units of |d|, for every finite non-zero d, denormal
 *                     components and lengths up to 2^126 included (a direction whose squared length is within 4e-7 of 1 is traced bit for
 *                     bit as given; any other is normalised first and t scaled back).  A hit whose t does not fit float32 in the caller's
 *                     units reports t = +inf (or a denormal) with valid ids: inst tells a hit from a miss.  u, v: the weights of the
 *                     triangle's second and third vertex; inst, prim: the instance and primitive ids of the renderer's hit record
 *                     (lr_scene.instances, the primitive within its mesh); tri indexes lr_scene.accel.triangles; reserved is written 0.
 *   A miss            t = +inf, u = v = 0, inst = prim = tri = LR_INVALID_ID.
 *   LRHIP_RAY_ANY     stops at the first accepted triangle: out[i] = 1 (occluded) or 0.
 *   Screened rays     a ray with a non-finite component (t_max = +inf is the one exception), a zero direction, or for which
 *                     t_max > t_min is false is a miss / not occluded; it never enters the traversal loop.
 *   Alpha test        without LRHIP_RAY_ALPHA_TEST every visible triangle is opaque.  With it, candidates on maybe-non-opaque instances
 *                     pass through the scene's stochastic alpha test exactly as in the renderer (Geometry::_alpha_skip: a hash of instance,
 *                     primitive and the barycentric bits against the surface's opacity there).  Ignored for scenes with any_non_opaque == 0.
 *   Pointers          with LRHIP_RAY_DEVICE_POINTERS both are device memory, 16-byte aligned (else LRHIP_ERROR_INVALID), and the call is
 *                     asynchronous on the context's stream.  Without it both are host memory: the library stages them through context-owned
 *                     buffers (they grow on demand up to 32 MiB each and are released with the context; a larger batch goes through them
 *                     chunk by chunk) and the call synchronises.
 *   Determinism       a ray's result is a function of the ray and the scene only: bit-identical from run to run and wherever the ray
 *                     stands in the batch.                                                                                          */
typedef struct lrhip_ray { float o[3], t_min, d[3], t_max; } lrhip_ray;                                       /* 32 bytes */
typedef struct lrhip_ray_hit { float t, u, v; uint32_t inst, prim, tri, reserved[2]; } lrhip_ray_hit;         /* 32 bytes */
typedef struct lrhip_ray_query_params {
    const void *rays;  /* lrhip_ray[count] */
    void *out;         /* LRHIP_RAY_CLOSEST: lrhip_ray_hit[count]; LRHIP_RAY_ANY: uint32_t[count] (1 occluded, 0 not) */
    uint64_t count;    /* 0 is legal and launches nothing; at most 2^31 - 1 */
    uint32_t mode;     /* LRHIP_RAY_CLOSEST or LRHIP_RAY_ANY */
    uint32_t flags;    /* LRHIP_RAY_DEVICE_POINTERS, LRHIP_RAY_ALPHA_TEST */
} lrhip_ray_query_params;
#define LRHIP_RAY_CLOSEST 0u
#define LRHIP_RAY_ANY 1u
#define LRHIP_RAY_DEVICE_POINTERS 1u
#define LRHIP_RAY_ALPHA_TEST 2u
#define LRHIP_RAY_MAX_COUNT 0x7fffffffull
int lrhip_trace_rays(lrhip_ctx *ctx, const lrhip_ray_query_params *params);
/* HIP-event time of the kernel(s) of the last lrhip_trace_rays call (a host-pointer call: summed over its chunks), in ms; synchronises */
double lrhip_last_trace_ms(lrhip_ctx *ctx);

/* Radiance queries: the radiance that arrives along caller-supplied rays, by the MegaPath estimator of the scene of the last
 * lrhip_upload_scene / lrhip_update_scene (at the time it was moved to) -- lightmap and probe baking, cameras the scene format does not have,
 * radiance for a batch of rays, a re-render of a few pixels.  The reference's Li is only reachable through a scene's camera and film.
 *   Estimator      sample s of ray k is MegakernelPathTracingInstance::Li (src/integrators/mega_path.cpp:49-156) with the caller's ray in place
 *                  of camera.generate_ray, and nothing else changed: the throughput starts at 1 and pdf_bsdf at 1e16 (emission and environment
 *                  seen directly are unweighted); depth, rr_depth and rr_threshold are the uploaded scene's integrator's; the shutter weight is 1.
 *                  t_min and t_max bound the first segment only.  Directions need not be normalised: shading takes wo = -d / |d|, so the
 *                  kernel divides |d| out of the direction and multiplies t_min and t_max by it -- the segment is the caller's; a direction
 *                  whose squared length is within 4e-7 of 1 (what a float normalisation returns) is taken bit for bit.  Any finite non-zero
 *                  direction will do, denormal or near FLT_MAX: an end of the segment whose distance in units of the unit vector is beyond
 *                  the float range becomes +inf, one below it 0.
 *   Sampler        ray k has the stream id j = streams ? streams[k] : k.  Its sampler is started exactly as Li starts it for pixel
 *                  (j mod W, (j div W) mod H) of the scene's camera frame W x H at sample index s, then draws and discards what Li draws before
 *                  its first bounce: generate_pixel_2d, and generate_2d for the lens iff the scene's camera is a thin lens.  So a ray that IS
 *                  camera ray (px, py, s), queried with stream py W + px at sample s, walks the path the film's sample walks.  Two rays with
 *                  the same j at the same s share their random numbers; for j >= W H the stream wraps (no error).
 *   Accumulation   per sample ColorFilmInstance::_accumulate (src/films/color.cpp:107-130) into the ray's record (sum r, sum g, sum b, n), the
 *                  film's layout: a sample with a NaN or infinite component is rejected, the others are clamped to `clamp` and n += 1.  Without
 *                  LRHIP_RADIANCE_ACCUMULATE the library zeroes `out` first; with it the sums are added to what `out` holds (progressive
 *                  refinement over calls with disjoint sample ranges).
 *   Screened rays  a ray lrhip_trace_rays would screen (a non-finite component other than t_max = +inf, a zero direction, t_max > t_min false)
 *                  starts no path: its record is (0, 0, 0, 0), or untouched under LRHIP_RADIANCE_ACCUMULATE.  n = 0 tells.
 *   No lighting    a scene with neither lights nor an environment renders nothing in the reference (mega_path.cpp:40-47: "no lights in scene",
 *                  the film stays black with n = 0) and in lrhip_render.  Here too: nothing is launched, every record is (0, 0, 0, 0), or
 *                  untouched under LRHIP_RADIANCE_ACCUMULATE, and the call returns LRHIP_OK.
 *   Pointers       as for lrhip_trace_rays.  With LRHIP_RAY_DEVICE_POINTERS rays and out are 16-byte aligned device memory, streams 4-byte
 *                  aligned (else LRHIP_ERROR_INVALID), and the call is asynchronous on the context's stream.  Without it all three are host
 *                  memory, staged through context-owned buffers 2^20 rays at a time, and the call synchronises.
 *   Determinism    the same call gives the same bits from run to run.  With ONE sample per call a ray's record is a function of (ray, stream id,
 *                  s, scene) only, wherever the ray stands in the batch.  With several samples per call the adds of one ray happen in the order
 *                  its paths finish, which depends on the 63 rays of its work item, and the sample range is cut into chunks by a rule of (count,
 *                  sample range) only: across batch layouts the result is the same up to the order of float additions, no more.
 *   Scope          scenes whose integrator is MegaPath, nested Mix / Layered surfaces included; LRHIP_ERROR_UNSUPPORTED for AOV, Direct, Normal
 *                  and MegaVPTNaive scenes, LRHIP_ERROR_INVALID before any upload, for NULL rays / out with count > 0 and for misaligned device
 *                  pointers.  One kernel serves every MegaPath scene -- the all-closures one-path-per-lane kernel -- so a scene without Mix /
 *                  Layered surfaces is queried more slowly than lrhip_render renders it.  lrhip_last_variant keeps reporting the last lrhip_render.
 *   Counters       LRHIP_RADIANCE_COUNTERS runs the counting twin and adds to lrhip_get_counters; `paths` counts the valid rays x samples. */
typedef struct lrhip_radiance_query_params {
    const void *rays;      /* lrhip_ray[count], as for lrhip_trace_rays */
    const void *streams;   /* uint32_t[count] or NULL (= 0, 1, 2, ...): the sampler stream of each ray */
    void *out;             /* float4[count]: (sum r, sum g, sum b, n) per ray */
    uint64_t count;        /* 0 is legal and launches nothing; at most LRHIP_RAY_MAX_COUNT */
    uint32_t spp_begin, spp_end;  /* sample indices [begin, end) of every ray; begin >= end launches nothing */
    uint32_t flags;        /* LRHIP_RAY_DEVICE_POINTERS, LRHIP_RADIANCE_ACCUMULATE, LRHIP_RADIANCE_COUNTERS */
    float clamp;           /* per-sample radiance clamp; 0 = the uploaded scene's film clamp */
} lrhip_radiance_query_params;
#define LRHIP_RADIANCE_ACCUMULATE 4u
#define LRHIP_RADIANCE_COUNTERS 8u
int lrhip_trace_radiance(lrhip_ctx *ctx, const lrhip_radiance_query_params *params);
/* HIP-event time of the kernel(s) of the last lrhip_trace_radiance call (a host-pointer call: summed over its chunks), in ms; synchronises */
double lrhip_last_radiance_ms(lrhip_ctx *ctx);

/* Surface queries: what is AT a hit -- world position, normals, uv, material and emission -- for hit records the caller
 * supplies: what lrhip_trace_rays wrote, or records made from a texel's (inst, prim, u, v).  Picking, the start points and guides of a
 * lightmap bake, normal and albedo baking.  The reference computes these inside its kernels only (Geometry::shading_point,
 * src/base/geometry.cpp:345-389; Surface::Closure::albedo / roughness; Light::Closure::evaluate); the AOV integrator sums them per pixel of
 * the scene's camera.  Camera, integrator and sampler play no part here.
 *   Which triangle    hit.tri < the BVH's triangle count: the renderer's path.  inst and prim are read from the triangle's record, the caller's
 *                     copies are ignored, and the point is the one a render shades at this hit, from the baked shading record, bit for bit.
 *                     hit.tri == LR_INVALID_ID with inst < instance_count and prim inside that instance's mesh: the same quantities from the
 *                     instance, its triangle and three vertices, with weights (1 - u - v, u, v) -- for callers who hold a texel's
 *                     (inst, prim, u, v) and no ray.  The two paths differ in the last bits only (world-space against object-space arithmetic).
 *                     Any other record -- a miss, an id out of range, a non-finite u or v -- gives the INVALID RECORD: 128 zero bytes except
 *                     inst = prim = surface = light = closure_kind = LR_INVALID_ID.  Every index is checked before it is used: a malformed
 *                     record never faults.  u and v are not confined to the triangle: a point outside it is extrapolated.
 *   Viewing direction with rays: wo = -d / |d| (the normalisation rule of lrhip_trace_radiance: a direction whose squared length is within 4e-7
 *                     of 1 is taken bit for bit), and the emission is the light's towards o.  A ray lrhip_trace_rays would screen makes
 *                     its record invalid.  With rays == NULL: wo = ng, the surface seen from its front, from p + ng.
 *                     LRHIP_SURFACE_BACK_FACING = dot(wo, ng) < 0.
 *   Geometry          p, area (world space), ng (unit, the orientation of cross(e1, e2), never flipped), ns (the interaction's shading normal,
 *                     face-forwarded to ng: what the AOV `normal` buffer sums), tangent (the shading frame's s: dpdu, or the fallback frame's
 *                     where the uv determinant is 0), uv.
 *   Material          where the instance has a surface, the closure is resolved exactly as the shading block resolves it (textures and normal
 *                     map at uv): n_closure is the normal of its frame, closure_kind its LR_SURFACE_* kind, albedo and roughness
 *                     Surface::Closure::albedo / roughness as the AOV integrator reports them.  Without a surface: albedo = roughness = 0,
 *                     n_closure = ns, closure_kind = LR_INVALID_ID.  emission: the light's L towards the ray's origin where the scene has
 *                     lights and the instance carries LR_SHAPE_HAS_LIGHT (0 from behind a one-sided light), else 0.  surface: the closure
 *                     index ((tags >> 12) & 4095) or LR_INVALID_ID; light: the light index (tags & 4095) or LR_INVALID_ID.
 *   LRHIP_SURFACE_GEOMETRY_ONLY  skips material and emission: those fields are written as for "no surface, no light"; surface, light and
 *                     the flag bits are still reported.  A kernel of its own that holds no texture or closure code.
 *   Scope             the full query is refused with LRHIP_ERROR_UNSUPPORTED for scenes with Mix / Layered surfaces nested in each other
 *                     (the AOV integrator refuses them for the same reason); it serves MegaPath, AOV, Direct, Normal and MegaVPTNaive scenes
 *                     alike.  The geometry-only query serves every uploaded scene.
 *   Pointers          as for lrhip_trace_rays.  With LRHIP_RAY_DEVICE_POINTERS hits, rays and out are device memory, 16-byte aligned (else
 *                     LRHIP_ERROR_INVALID), and the call is asynchronous on the context's stream: a trace followed by a surface query needs no
 *                     host round trip.  Without it they are host memory, staged 2^20 records at a time through context-owned buffers released
 *                     with the context, and the call synchronises.
 *   Errors            LRHIP_ERROR_INVALID before any upload, for NULL hits or out with count > 0, unknown flags, misaligned device pointers
 *                     and count > LRHIP_RAY_MAX_COUNT.
 *   Determinism       a record's result is a function of (record, ray, scene) only: bit-identical from run to run and wherever the record
 *                     stands in the batch.  The tables are read as lrhip_update_scene, lrhip_set_instance_transforms and
 *                     lrhip_set_mesh_vertices left them.  lrhip_last_variant, film, AOV buffers and counters are untouched.                 */
typedef struct lrhip_surface_point {          /* 128 bytes, eight dwordx4 stores */
    float p[3];         float area;           /* world position; world-space area of the triangle */
    float ng[3];        uint32_t flags;       /* unit geometric normal, orientation of cross(e1, e2), never flipped; LRHIP_SURFACE_* bits */
    float ns[3];        uint32_t inst;        /* the interaction's shading normal (face-forwarded to ng): what the AOV `normal` buffer sums */
    float tangent[3];   uint32_t prim;        /* shading frame's s (dpdu, or the fallback frame's where the uv determinant is 0) */
    float n_closure[3]; uint32_t closure_kind;/* normal of the closure's frame (normal map applied); = ns and LR_INVALID_ID without a surface */
    float uv[2];        float roughness[2];
    float albedo[3];    uint32_t surface;     /* closure index ((tags >> 12) & 4095) or LR_INVALID_ID */
    float emission[3];  uint32_t light;       /* the light's L towards the ray's origin; light index (tags & 4095) or LR_INVALID_ID */
} lrhip_surface_point;
#define LRHIP_SURFACE_VALID 1u
#define LRHIP_SURFACE_BACK_FACING 2u
#define LRHIP_SURFACE_HAS_SURFACE 4u
#define LRHIP_SURFACE_HAS_LIGHT 8u
typedef struct lrhip_surface_query_params {
    const void *hits;   /* lrhip_ray_hit[count]: what lrhip_trace_rays wrote, or records the caller made */
    const void *rays;   /* lrhip_ray[count] or NULL */
    void *out;          /* lrhip_surface_point[count] */
    uint64_t count;     /* 0 is legal and launches nothing; at most LRHIP_RAY_MAX_COUNT */
    uint32_t flags;     /* LRHIP_RAY_DEVICE_POINTERS, LRHIP_SURFACE_GEOMETRY_ONLY */
} lrhip_surface_query_params;
#define LRHIP_SURFACE_GEOMETRY_ONLY 32u
int lrhip_query_surface(lrhip_ctx *ctx, const lrhip_surface_query_params *params);
/* HIP-event time of the kernel(s) of the last lrhip_query_surface call (a host-pointer call: summed over its chunks), in ms; synchronises */
double lrhip_last_surface_ms(lrhip_ctx *ctx);

/* BSDF queries: the closure's answer at a hit the caller names -- Surface::Closure::evaluate for a direction the caller gives,
 * or Surface::Closure::sample for three random numbers the caller gives (src/base/surface.cpp:35-68) -- the missing piece between
 * lrhip_query_surface (what is at a hit) and lrhip_trace_radiance (the whole estimator): a direct-lighting estimator of the caller's own, path
 * guiding, an integrator written as tensor operations over batches of rays, a material preview.  Camera, integrator and sampler play no part:
 * the query is a pure function of its inputs.
 *   Which triangle    exactly as for lrhip_query_surface: hit.tri < the BVH's triangle count is the baked path, hit.tri == LR_INVALID_ID with
 *                     valid (inst, prim) the instance path; every index is checked before it is used, a non-finite u or v gives the invalid record.
 *   Viewing direction exactly as for lrhip_query_surface: wo = -d / |d| of the record's ray (a direction whose squared length is within 4e-7 of 1
 *                     is taken bit for bit); a ray lrhip_trace_rays would screen makes its record invalid; rays == NULL: wo = ng.
 *   dirs              one float4 per record.  LRHIP_BSDF_EVALUATE: (wi.x, wi.y, wi.z, ignored) -- wi in world space, pointing AWAY from the
 *                     surface, of any length: it is normalised by wo's rule; a zero or non-finite wi gives the invalid record.
 *                     LRHIP_BSDF_SAMPLE: (u_lobe, u_x, u_y, ignored) -- the three numbers Surface::Closure::sample draws, in the order the
 *                     path tracer draws them; a non-finite one gives the invalid record.  No sampler is touched.
 *   What is computed  the closure is resolved as the shading block resolves it (textures and normal map at uv), then evaluated or sampled by
 *                     the calls the MegaPath shading block makes, for radiance transport, from outside (eta_i = 1).  f INCLUDES |cos theta_i|
 *                     (Surface::Evaluation::f as the path tracer consumes it: throughput *= f / pdf).  Layered surfaces estimate f by a random
 *                     walk seeded from the bits of p and the directions: deterministic, but a different draw at another point.
 *   Result            evaluate: (f, pdf, the unit wi that was used, event = 0).  sample: (f, pdf, the sampled world-space wi, event =
 *                     LRHIP_BSDF_EVENT_*).  pdf = 0 is a failed sample: its f and wi are what the closure left there and may be non-finite (a
 *                     total internal reflection), as in the reference, whose path tracer tests pdf > 0 first.  THE INVALID RECORD -- an invalid hit record, ray or dirs, or a
 *                     valid hit on an instance without a surface -- is 32 zero bytes except event = LR_INVALID_ID.  A malformed record never faults.
 *   Scope             scenes of every integrator with basic closures, Disney, Mix (trees of basic and Disney leaves included) and Layered;
 *                     LRHIP_ERROR_UNSUPPORTED for scenes with Mix / Layered surfaces nested in each other, as the full surface query.
 *   Pointers          as for lrhip_query_surface.  With LRHIP_RAY_DEVICE_POINTERS hits, rays, dirs and out are device memory, 16-byte aligned
 *                     (else LRHIP_ERROR_INVALID), and the call is asynchronous on the context's stream: trace, then sample, needs no host round
 *                     trip.  Without it they are host memory, staged 2^20 records at a time through context-owned buffers released with the
 *                     context, and the call synchronises.
 *   Errors            LRHIP_ERROR_INVALID before any upload, for NULL hits, dirs or out with count > 0, unknown flags, an unknown mode,
 *                     misaligned device pointers and count > LRHIP_RAY_MAX_COUNT.
 *   Determinism       a record's result is a function of (record, ray, dirs, scene) only: bit-identical from run to run and wherever the record
 *                     stands in the batch.  lrhip_last_variant, film, AOV buffers and counters are untouched.
 *   Not done          nested Mix / Layered, importance transport, the closure's eta (Russian roulette), opacity.                             */
typedef struct lrhip_bsdf_result {            /* 32 bytes, two dwordx4 stores */
    float f[3];         float pdf;            /* value * |cos theta_i|; solid-angle density of wi */
    float wi[3];        uint32_t event;       /* unit world-space direction; LRHIP_BSDF_EVENT_* (evaluate: 0), LR_INVALID_ID in the invalid record */
} lrhip_bsdf_result;
#define LRHIP_BSDF_EVALUATE 0u
#define LRHIP_BSDF_SAMPLE 1u
#define LRHIP_BSDF_EVENT_REFLECT 0u           /* Surface::event_reflect / _enter / _exit / _through (src/base/surface.h:46-50) */
#define LRHIP_BSDF_EVENT_ENTER 1u
#define LRHIP_BSDF_EVENT_EXIT 2u
#define LRHIP_BSDF_EVENT_THROUGH 4u
typedef struct lrhip_bsdf_query_params {
    const void *hits;   /* lrhip_ray_hit[count]: what lrhip_trace_rays wrote, or records the caller made */
    const void *rays;   /* lrhip_ray[count] or NULL */
    const void *dirs;   /* float[4][count]: (wi, -) or (u_lobe, u_x, u_y, -) */
    void *out;          /* lrhip_bsdf_result[count] */
    uint64_t count;     /* 0 is legal and launches nothing; at most LRHIP_RAY_MAX_COUNT */
    uint32_t mode;      /* LRHIP_BSDF_EVALUATE or LRHIP_BSDF_SAMPLE */
    uint32_t flags;     /* LRHIP_RAY_DEVICE_POINTERS */
} lrhip_bsdf_query_params;
int lrhip_query_bsdf(lrhip_ctx *ctx, const lrhip_bsdf_query_params *params);
/* HIP-event time of the kernel(s) of the last lrhip_query_bsdf call (a host-pointer call: summed over its chunks), in ms; synchronises */
double lrhip_last_bsdf_ms(lrhip_ctx *ctx);

/* Light queries: the scene's emitters as seen from points the caller names -- LightSampler::Instance::sample for three random
 * numbers the caller gives (src/base/light_sampler.cpp:57-63, src/lightsamplers/uniform.cpp:78-137), or what a BSDF-sampled ray found at its
 * end, LightSampler::Instance::evaluate_hit / evaluate_miss (uniform.cpp:50-76) -- the last piece of a next-event estimator of the caller's own:
 * with lrhip_trace_rays, lrhip_query_surface and lrhip_query_bsdf, MegaPath's Li can be written as a loop over five queries.  Camera, integrator
 * and sampler play no part: the query is a pure function of its inputs.
 *   LRHIP_LIGHT_SAMPLE    one light, or the environment, sampled from each hit.
 *     hits            resolved exactly as for lrhip_query_bsdf: hit.tri < the BVH's triangle count is the baked path, hit.tri == LR_INVALID_ID
 *                     with valid (inst, prim) the instance path; every index is checked before it is used; a non-finite u or v gives the invalid
 *                     record.  The hit need not carry a surface: the light sampler never asks for one.  No viewing ray is needed (rays is not
 *                     read): the sampler reads the point, its normals and its offset bits, never wo.
 *     dirs            one float4 per record: (u_light_selection, u_surface_x, u_surface_y, ignored) -- the three numbers the path tracer draws
 *                     for its light sample, in its order; a non-finite one gives the invalid record.  No sampler is touched.
 *     out_rays        lrhip_ray[count]: the shadow ray exactly as the shading block launches it -- the origin is the point moved off its surface
 *                     towards the light (Interaction::p_robust), d the unit direction, t_min = 0, t_max = 0.9999 x the distance for an area
 *                     light and FLT_MAX for the environment.  An array of its own, so that it goes into lrhip_trace_rays(LRHIP_RAY_ANY) as it
 *                     stands.
 *     out             L: the radiance towards the point.  pdf: the solid-angle density at the point TIMES the selection probability -- the
 *                     shading block's light_pdf, so that balance(pdf, bsdf_pdf) / pdf is the reference's weight.  kind: LRHIP_LIGHT_KIND_AREA
 *                     or LRHIP_LIGHT_KIND_ENVIRONMENT.  reserved is written 0.
 *     A failed sample has pdf = 0 (the back of a one-sided light, a light seen at a grazing angle) and L = 0; its ray is whatever the sampler
 *                     left there and may be non-finite: lrhip_trace_rays screens such rays.  Test pdf > 0 first, as the path tracer does.
 *     LRHIP_LIGHT_FROM_POINTS (sample mode only): hits is float[4][count] = (p, ignored), a bare world-space point -- the reference's
 *                     Interaction{p} of a medium point: no offset, the shadow ray starts at p itself.  Irradiance probes, volumes.  A non-finite
 *                     p gives the invalid record.
 *   LRHIP_LIGHT_EVALUATE  what a ray found.  rays (required) are the rays, hits the records lrhip_trace_rays wrote for them; dirs and out_rays are
 *                     not read or written and may be NULL.
 *     an emitter      a hit (resolved as above, back-facing by wo = -d / |d| under lrhip_query_surface's normalisation rule) on an instance with
 *                     LR_SHAPE_HAS_LIGHT in a scene with lights: the light's L towards the ray's origin, pdf = its solid-angle density there x
 *                     (1 - env_prob) / light_count, kind = LRHIP_LIGHT_KIND_AREA (src/integrators/mega_path.cpp:79-86).  From behind a one-sided
 *                     light: L = 0, pdf = 0, still LRHIP_LIGHT_KIND_AREA.
 *     a miss          exactly what lrhip_trace_rays writes, inst == tri == LR_INVALID_ID, in a scene with an environment: the environment's L
 *                     along d / |d|, pdf x env_prob, kind = LRHIP_LIGHT_KIND_ENVIRONMENT (mega_path.cpp:70-76).
 *     anything else   a hit on a non-emitter, a miss in a scene without an environment: L = 0, pdf = 0, kind = LRHIP_LIGHT_KIND_NONE -- a valid answer.
 *   THE INVALID RECORD    an all-zero ray (sample mode; the ray queries screen a zero direction) and an all-zero result except kind =
 *                     LR_INVALID_ID: in sample mode a miss, an id out of range, a non-finite u, v, dirs or point; in evaluate mode a ray
 *                     lrhip_trace_rays would screen, a non-finite u or v, an id out of range that is not the miss pattern.  A malformed record
 *                     never faults.
 *   No lighting       a scene with neither lights nor an environment is no error: every record, whatever it holds, is answered L = 0, pdf = 0,
 *                     kind = LRHIP_LIGHT_KIND_NONE, with a zero ray in sample mode, and no light table is read.
 *   Scope             scenes of every integrator and every closure set, Mix / Layered surfaces nested in each other included: no closure is
 *                     touched.  Spherical (constant or image), Directional and Combined environments, Combined nodes nested in each other included.
 *   Pointers          as for lrhip_query_bsdf.  With LRHIP_RAY_DEVICE_POINTERS every array is device memory, 16-byte aligned (else
 *                     LRHIP_ERROR_INVALID), and the call is asynchronous on the context's stream: trace, sample, trace the shadow rays needs no
 *                     host round trip.  Without it they are host memory, staged 2^20 records at a time through context-owned buffers released
 *                     with the context, and the call synchronises.
 *   Errors            LRHIP_ERROR_INVALID before any upload, with count > 0 for NULL hits or out, NULL dirs or out_rays in sample mode and NULL
 *                     rays in evaluate mode, for unknown flags, an unknown mode, LRHIP_LIGHT_FROM_POINTS in evaluate mode, misaligned device
 *                     pointers and count > LRHIP_RAY_MAX_COUNT.
 *   Determinism       a record's result is a function of (record, ray, dirs, scene) only: bit-identical from run to run and wherever the record
 *                     stands in the batch.  The tables are read as lrhip_update_scene, lrhip_set_instance_transforms and
 *                     lrhip_set_mesh_vertices left them.  lrhip_last_variant, film, AOV buffers and counters are untouched.
 *   Not done          which light or triangle a sample picked, beyond kind; power- or BVH-based light selection; emitter sampling for media
 *                     transmittance.                                                                                                        */
typedef struct lrhip_light_result {           /* 32 bytes, two dwordx4 stores */
    float L[3];         float pdf;            /* radiance towards the point; solid-angle density x selection probability */
    uint32_t kind;      uint32_t reserved[3]; /* LRHIP_LIGHT_KIND_*, LR_INVALID_ID in the invalid record; 0 */
} lrhip_light_result;
#define LRHIP_LIGHT_SAMPLE 0u
#define LRHIP_LIGHT_EVALUATE 1u
#define LRHIP_LIGHT_KIND_AREA 0u
#define LRHIP_LIGHT_KIND_ENVIRONMENT 1u
#define LRHIP_LIGHT_KIND_NONE 2u
#define LRHIP_LIGHT_FROM_POINTS 64u
typedef struct lrhip_light_query_params {
    const void *hits;   /* lrhip_ray_hit[count]; with LRHIP_LIGHT_FROM_POINTS float[4][count] = (p, -) */
    const void *rays;   /* LRHIP_LIGHT_EVALUATE: lrhip_ray[count]; LRHIP_LIGHT_SAMPLE: not read */
    const void *dirs;   /* LRHIP_LIGHT_SAMPLE: float[4][count] = (u_light_selection, u_surface_x, u_surface_y, -); LRHIP_LIGHT_EVALUATE: not read */
    void *out_rays;     /* LRHIP_LIGHT_SAMPLE: lrhip_ray[count], the shadow rays; LRHIP_LIGHT_EVALUATE: not written */
    void *out;          /* lrhip_light_result[count] */
    uint64_t count;     /* 0 is legal and launches nothing; at most LRHIP_RAY_MAX_COUNT */
    uint32_t mode;      /* LRHIP_LIGHT_SAMPLE or LRHIP_LIGHT_EVALUATE */
    uint32_t flags;     /* LRHIP_RAY_DEVICE_POINTERS, LRHIP_LIGHT_FROM_POINTS */
} lrhip_light_query_params;
int lrhip_query_light(lrhip_ctx *ctx, const lrhip_light_query_params *params);
/* HIP-event time of the kernel(s) of the last lrhip_query_light call (a host-pointer call: summed over its chunks), in ms; synchronises */
double lrhip_last_light_ms(lrhip_ctx *ctx);

/* Camera, sampler and film queries: the three ends of a render -- where its random numbers come from, where its paths start
 * and where its samples go -- as queries in the style of the ones above, so that a whole lrhip_render can be written as a loop over queries on
 * the device: start the streams, draw, make camera rays, trace / shade with lrhip_trace_rays, lrhip_query_surface, lrhip_query_bsdf and
 * lrhip_query_light, draw again per vertex, and splat weight x Li into the film that lrhip_film_download, lrhip_film_reduce and the denoiser read.
 * The kernels make the renderers' own calls (PathSampler<>::start / next_*, camera_ray, film_accumulate) and are built with the oracle's
 * arithmetic (no contraction, correctly rounded division and square root): numbers, rays and weights are those of the reference, bit for bit.
 *
 * lrhip_query_sampler: Sampler::Instance with its state made explicit, so that a caller draws a path's numbers bounce by bounce.
 *   state           uint32_t[4] per record, read (unless LRHIP_SAMPLER_START) and written: the stream's position.  Opaque, and valid only for
 *                   the scene upload that made it (it names the scene's sampler kind, seed, tables).  The Independent sampler uses word 0 and
 *                   writes the other words 0.  A state the caller damaged never faults: what would index a table is brought into its range.
 *   LRHIP_SAMPLER_START  before drawing, the state is initialised as Li initialises it for stream id j at sample index s:
 *                   j = streams ? streams[k] : k, the stream of pixel (j mod W, (j div W) mod H), as for lrhip_trace_radiance; the TileShared
 *                   wrapper and its jitter are applied by the start itself.  s = indices ? indices[k] : sample_index.  Without the flag,
 *                   streams and indices are not read.
 *   pattern         host memory always: pattern_count <= LRHIP_SAMPLER_MAX_DRAWS codes, drawn in order for every record.  The three kinds are
 *                   NOT interchangeable: LRHIP_DRAW_2D is generate_2d -- PaddedSobol shares one permutation between its two dimensions, so
 *                   it is not two 1-D draws, and Sobol wraps its dimension counter one early for a pair -- and LRHIP_DRAW_PIXEL_2D is
 *                   generate_pixel_2d: for Sobol dimensions 0 / 1 against the pixel, for the others a 2-D draw.  An empty pattern with
 *                   LRHIP_SAMPLER_START only makes states; without the flag it does nothing.
 *   out             float[count][D], row-major, D = the pattern's number of floats (1 per 1-D draw, 2 per other; at most 128).  May be NULL
 *                   when D = 0.
 *   Draw order of MegaPath's Li (megapath_kernel.h): per sample LRHIP_DRAW_PIXEL_2D; then LRHIP_DRAW_2D for the lens iff the camera is a thin
 *                   lens.  Then per vertex that is shaded: 1-D light selection and 2-D light surface (both only where the scene has lights or an
 *                   environment), 1-D lobe, 2-D BSDF, and from depth + 1 >= rr_depth on a 1-D Russian-roulette number.  A vertex that is a miss
 *                   or carries no surface draws nothing.
 *   PaddedSobol     the permutation's length is the scene's sampler.spp, so sample indices at or beyond it repeat earlier streams: index s takes
 *                   the permutation slot of s mod spp (under the scramble of its own hash) and adds no new stratum.  A length that is no power
 *                   of two: the index itself is taken modulo it, where the reference's cycle walk need not end.
 *   Kernels         an Independent scene runs the PathSampler<false> instantiation, every other the run-time generic one -- the renderers' split.
 *
 * lrhip_query_camera: Camera::Instance::generate_ray with the filter's importance sampling, a pure function -- no sampler is touched.
 *   pixels          uint32_t[count] pixel ids py * W + px, or NULL: record k is pixel k (then count <= W * H).
 *   u               float[4][count] = (u_filter.x, u_filter.y, u_lens.x, u_lens.y): what LRHIP_DRAW_PIXEL_2D and, for a thin lens, the following
 *                   LRHIP_DRAW_2D gave.  u_lens is not looked at by the other cameras.
 *   out_rays        lrhip_ray[count], exactly the ray the renderers start: origin and unit direction in world space through the uploaded
 *                   camera_to_world, at the time the scene was moved to; t_min, t_max = the clip planes over the cosine to the axis.  An array of
 *                   its own, so that it goes into lrhip_trace_rays as it stands.
 *   out             lrhip_camera_sample[count].  weight: the filter's f / pdf -- exactly 1 for Box, negative in the lobes of Mitchell / Lanczos;
 *                   a path's throughput starts as it.  film_x, film_y: the continuous film position pixel + 0.5 + offset.  pixel: the id.
 *   THE INVALID RECORD  a pixel id >= W * H or a non-finite u that is looked at: a zero ray (the ray queries screen it), weight 0, film position
 *                   0 and pixel = LR_INVALID_ID.
 *
 * lrhip_film_splat: samples into the film.
 *   pixels          as above (NULL: record k goes to pixel k, count <= W * H).  A pixel id >= W * H is skipped.
 *   values          float[4][count] = (r, g, b, ignored): the caller has already multiplied the camera weight and the shutter weight in.
 *   clamp           0 = the scene's film clamp.
 *   Rule            ColorFilmInstance::_accumulate (src/films/color.cpp:107-130, effective spp 1): a record with a NaN or infinite component is
 *                   rejected and n is not incremented; otherwise the value is scaled down so that its largest component's magnitude is at most
 *                   the clamp, and (r, g, b, 1) is added to the pixel's float4 of the film the context accumulates into -- its own, or
 *                   lrhip_bind_film's.
 *   Ordering        on the context's stream: behind earlier renders, before later ones and downloads.
 *   Determinism     when the pixels of one call are distinct (pixels == NULL always is) each pixel receives one add and the film is
 *                   bit-determined.  Several records of one pixel in one call are added by float atomics in no fixed order: the result is the
 *                   same up to the order of float additions (n, a small integer, is exact).
 *   Scope           every scene whose context holds a film -- in this library every context does, an AOV scene's included (its auxiliary buffers
 *                   are not written).  LRHIP_ERROR_UNSUPPORTED if the context holds none.
 *
 *   Pointers        as for lrhip_query_light.  With LRHIP_RAY_DEVICE_POINTERS every array but pattern is device memory -- state, u, values,
 *                   out_rays, out 16-byte aligned, streams, indices, pixels 4-byte aligned, else LRHIP_ERROR_INVALID -- and the call is
 *                   asynchronous on the context's stream.  Without it they are host memory, staged 2^20 records at a time through context-owned
 *                   buffers released with the context, and the call synchronises.
 *   Errors          LRHIP_ERROR_INVALID before any upload, with count > 0 for a NULL required array, for unknown flags, an unknown draw code,
 *                   more than LRHIP_SAMPLER_MAX_DRAWS draws, a negative or NaN clamp, misaligned device pointers, count > LRHIP_RAY_MAX_COUNT,
 *                   and count > W * H without pixels.  count == 0 launches nothing.
 *   Determinism     a record's result is a function of (record, scene) only: bit-identical from run to run and wherever the record stands in
 *                   the batch.  Film (but for the splat), AOV buffers, counters and lrhip_last_variant are untouched.
 *   Not done        the closure's eta for Russian roulette (lrhip_query_bsdf does not report it); filtered splatting across pixels (the
 *                   reference's film takes one pixel per sample); AOV buffers; a fixed order for several splats of one pixel in one call; a
 *                   fused start-to-splat kernel.                                                                                          */
#define LRHIP_DRAW_1D 0u
#define LRHIP_DRAW_2D 1u
#define LRHIP_DRAW_PIXEL_2D 2u
#define LRHIP_SAMPLER_MAX_DRAWS 64u
#define LRHIP_SAMPLER_START 128u
typedef struct lrhip_sampler_query_params {
    void *state;              /* uint32_t[4][count] */
    const uint32_t *streams;  /* LRHIP_SAMPLER_START: uint32_t[count] or NULL (stream k) */
    const uint32_t *indices;  /* LRHIP_SAMPLER_START: uint32_t[count] or NULL (sample_index) */
    const uint32_t *pattern;  /* HOST memory: LRHIP_DRAW_*[pattern_count] */
    float *out;               /* float[count][D]; may be NULL when D = 0 */
    uint64_t count;           /* 0 is legal and launches nothing; at most LRHIP_RAY_MAX_COUNT */
    uint32_t pattern_count;   /* at most LRHIP_SAMPLER_MAX_DRAWS */
    uint32_t sample_index;
    uint32_t flags;           /* LRHIP_RAY_DEVICE_POINTERS, LRHIP_SAMPLER_START */
    uint32_t reserved;        /* 0 */
} lrhip_sampler_query_params;
int lrhip_query_sampler(lrhip_ctx *ctx, const lrhip_sampler_query_params *params);
typedef struct lrhip_camera_sample {          /* 16 bytes, one dwordx4 store */
    float weight;       float film_x, film_y; /* filter f / pdf; continuous film position */
    uint32_t pixel;                           /* py * W + px; LR_INVALID_ID in the invalid record */
} lrhip_camera_sample;
typedef struct lrhip_camera_query_params {
    const uint32_t *pixels;   /* uint32_t[count] or NULL (pixel k) */
    const void *u;            /* float[4][count] = (u_filter.x, u_filter.y, u_lens.x, u_lens.y) */
    void *out_rays;           /* lrhip_ray[count] */
    void *out;                /* lrhip_camera_sample[count] */
    uint64_t count;
    uint32_t flags;           /* LRHIP_RAY_DEVICE_POINTERS */
    uint32_t reserved;        /* 0 */
} lrhip_camera_query_params;
int lrhip_query_camera(lrhip_ctx *ctx, const lrhip_camera_query_params *params);
typedef struct lrhip_film_splat_params {
    const uint32_t *pixels;   /* uint32_t[count] or NULL (pixel k) */
    const void *values;       /* float[4][count] = (r, g, b, -) */
    uint64_t count;
    uint32_t flags;           /* LRHIP_RAY_DEVICE_POINTERS */
    float clamp;              /* 0 = the scene's film clamp */
} lrhip_film_splat_params;
int lrhip_film_splat(lrhip_ctx *ctx, const lrhip_film_splat_params *params);
/* HIP-event time of the kernel(s) of the last of these three calls (a host-pointer call: summed over its chunks), in ms; synchronises */
double lrhip_last_camera_ms(lrhip_ctx *ctx);

/* Moving instances on the device: Geometry::update (src/base/geometry.cpp:194-216) for object-to-world matrices the caller holds --
 * an animation frame, a physics step whose matrices are a tensor on the GPU, a drag in an editor -- between two renders or queries, without a
 * trip of the tables through the host.
 *   What it rewrites  the four device tables lrhip_update_scene rewrites for moved geometry: the instance records (matrix and normal matrix), the
 *                     baked BVH triangles of the listed instances, their shading records, and every BVH packet, refitted over the same topology
 *                     and quantised again.  Afterwards they hold, bit for bit, what lrhip_update_scene would have written for the uploaded scene
 *                     with exactly these matrices in lr_instance.object_to_world, re-baked and refitted by the host (lrhost_scene_set_instance_transforms).
 *                     Film, AOV buffers, counters, camera, environment, textures, lights and the selected kernels stay as they are.  The call is
 *                     ordered on the context's stream behind earlier renders and queries and before later ones.
 *   Matrices          float[count][16], column-major: element [4 c + r] is row r of column c, the layout of lr_instance.object_to_world; the
 *                     fourth row is not read.  instances: the id of each matrix's instance (an index into lr_scene.instances), or NULL for ids
 *                     0 .. count-1 (then count <= instance_count).  Instances that are not listed keep their matrices.
 *   Pointers          without LRHIP_RAY_DEVICE_POINTERS both arrays are host memory: ids are checked to be in range and distinct, every matrix
 *                     element to be finite (else LRHIP_ERROR_INVALID, nothing changed), they are staged through a context-owned buffer, and the
 *                     call synchronises.  With it both are device memory, the matrices 16-byte and the ids 4-byte aligned (else
 *                     LRHIP_ERROR_INVALID), and the call is asynchronous on the context's stream: an id out of range is skipped, of several
 *                     entries with one id the last one wins, and a non-finite matrix gives non-finite tables -- the caller's error, but no fault.
 *   The host scene    the caller's lr_scene is not read and does not change.  A later lrhip_update_scene or lrhip_upload_scene overwrites what
 *                     this call wrote: the host's tables win again.  A caller who keeps both in step moves the host scene by
 *                     lrhost_scene_set_instance_transforms.
 *   Errors            LRHIP_ERROR_INVALID before any upload, for NULL matrices with count > 0, unknown flags and count > 2^31 - 1;
 *                     LRHIP_ERROR_UNSUPPORTED for a BVH whose nodes are not stored parents first (lrhost_scene_build_accel's are).             */
typedef struct lrhip_instance_update_params {
    const void *object_to_world; /* float[count][16], column-major, the layout of lr_instance.object_to_world */
    const void *instances;       /* uint32_t[count] instance ids, or NULL: ids 0 .. count-1 */
    uint64_t count;              /* 0 is legal and launches nothing; with instances == NULL at most instance_count */
    uint32_t flags;              /* LRHIP_RAY_DEVICE_POINTERS */
} lrhip_instance_update_params;
int lrhip_set_instance_transforms(lrhip_ctx *ctx, const lrhip_instance_update_params *params);
/* HIP-event time of the kernels of the last lrhip_set_instance_transforms call, in ms; synchronises */
double lrhip_last_instance_update_ms(lrhip_ctx *ctx);

/* Deforming a mesh on the device (no reference equivalent: the reference's meshes are fixed after Geometry::build): new object-space
 * vertex positions for one mesh of the uploaded scene -- a skinned character, cloth, a morph target, the output of an optimiser or a physics
 * step that is a tensor on the GPU -- between two renders or queries, without parsing and uploading the scene again.
 *   What it rewrites  vertices [first_vertex, first_vertex + count) of mesh `mesh` in the device vertex table get new px py pz, with `normals`
 *                     also new nx ny nz; u v stay.  Then the baked BVH triangles and shading records of EVERY instance of that mesh (a mesh
 *                     that several instances share, the Sphere shapes of one subdivision level for example, moves in all of them) and every
 *                     BVH packet, refitted over the same topology and quantised again.  Afterwards the four tables lrhip_update_scene
 *                     rewrites hold, byte for byte, what lrhip_update_scene would have written for the uploaded scene with these vertices
 *                     in lr_scene.vertices, re-baked and refitted by the host (lrhost_scene_set_mesh_vertices), and the device vertex table
 *                     holds the host's bytes.  Instance records, film, AOV buffers, counters, camera, environment, textures and the selected
 *                     kernels stay.  The call is ordered on the context's stream behind earlier renders and queries and before later ones.
 *   Normals           normals != NULL: written as given, not normalised.  normals == NULL without LRHIP_MESH_RECOMPUTE_NORMALS: kept -- the
 *                     caller's choice for small deformations.  LRHIP_MESH_RECOMPUTE_NORMALS (normals must be NULL): the normals of ALL
 *                     vertices of the mesh are recomputed from the new positions, area-weighted and deterministic.  For vertex v: s = (0,0,0);
 *                     for every triangle t of the mesh in ascending t, and within it every corner in ascending order that names v,
 *                     s += c_t = cross(p[i1] - p[i0], p[i2] - p[i0]) (components a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x);
 *                     l2 = (s.x s.x + s.y s.y) + s.z s.z; if l2 > 0 && l2 <= FLT_MAX then n = s / sqrtf(l2) per component, otherwise the
 *                     normal stays.  All of it fp32, unfused, with correctly rounded divide and sqrt.  Normals are written whether or not the
 *                     mesh's instances carry LR_SHAPE_HAS_VERTEX_NORMAL; shading reads them only where the flag is set.  The first
 *                     recomputing call on a mesh builds the mesh's corner lists from a read-back of its index range and SYNCHRONISES; the
 *                     lists (12 B per mesh triangle + 4 B per vertex) stay with the context until the scene is released.
 *   Emitters          a mesh of which any instance carries LR_SHAPE_HAS_LIGHT is refused with LRHIP_ERROR_UNSUPPORTED, nothing changed: the
 *                     mesh's area alias table (tri_alias, tri_pdf) and the copy of tri_pdf in the shading records are functions of the
 *                     object-space areas, and rebuilding them to the host's fp64-summed bits is a separate piece of work.
 *   Pointers          without LRHIP_RAY_DEVICE_POINTERS both arrays are host memory: mesh < mesh_count, the range inside the mesh and every
 *                     element finite are checked (else LRHIP_ERROR_INVALID, nothing changed), the arrays are staged through a context-owned
 *                     buffer, and the call synchronises.  With it both are device memory, 4-byte aligned (else LRHIP_ERROR_INVALID), read in
 *                     place, and the call is asynchronous on the context's stream; mesh and range are checked all the same (they are
 *                     scalars), and non-finite values give non-finite tables -- the caller's error, but no fault and no endless loop.
 *   The host scene    the caller's lr_scene is not read and does not change.  A later lrhip_update_scene (which copies lr_scene.vertices too)
 *                     or lrhip_upload_scene overwrites what this call wrote: the host's tables win again.
 *   Errors            LRHIP_ERROR_INVALID before any upload, for NULL positions with count > 0, normals together with
 *                     LRHIP_MESH_RECOMPUTE_NORMALS, and unknown flags; LRHIP_ERROR_UNSUPPORTED for an emitter and for a BVH whose nodes are
 *                     not stored parents first (as lrhip_set_instance_transforms).
 *   Not done          emissive meshes; changing vertex or triangle counts or the topology; a BVH rebuild when a deformation degrades the
 *                     tree (the refit keeps the build's topology); several meshes in one call; changing u v.                              */
typedef struct lrhip_mesh_update_params {
    const void *positions;   /* float[count][3], packed, object space */
    const void *normals;     /* float[count][3], packed, or NULL */
    uint32_t mesh;           /* index into lr_scene.meshes (lr_instance.handle.x >> 10) */
    uint32_t first_vertex;   /* within the mesh */
    uint64_t count;          /* 0 is legal and launches nothing */
    uint32_t flags;          /* LRHIP_RAY_DEVICE_POINTERS, LRHIP_MESH_RECOMPUTE_NORMALS */
} lrhip_mesh_update_params;
#define LRHIP_MESH_RECOMPUTE_NORMALS 16u
int lrhip_set_mesh_vertices(lrhip_ctx *ctx, const lrhip_mesh_update_params *params);
/* HIP-event time of the kernels of the last lrhip_set_mesh_vertices call, in ms; synchronises */
double lrhip_last_mesh_update_ms(lrhip_ctx *ctx);

/* Lightmap texels (no reference equivalent): the UV rasteriser of a bake.  Which point of ONE instance's mesh each texel of a
 * width x height lightmap over the mesh's UV chart stands for, as the record the surface, BSDF and light queries take for "a texel's point
 * without a ray": out[j * width + i] = lrhip_ray_hit { t = 0, u, v, inst = instance, prim, tri = 0xffffffff, reserved = { flags, 0 } }.
 *   Texels            texel (i, j) has its centre at uv = ((i + 1/2) / width, (j + 1/2) / height); row 0 is at v = 0.  Nothing wraps: a chart
 *                     outside [0, 1]^2 is not covered there.
 *   Coverage          a texel is CENTRE-COVERED by a triangle when the three edge functions of the triangle's UVs at its centre are >= 0, with
 *                     the orientation normalised (a mirrored chart works as well); a triangle without area in UV space, with a non-finite UV
 *                     or with a vertex index outside its mesh owns nothing.  With LRHIP_LIGHTMAP_CONSERVATIVE a texel is also TOUCHED by a
 *                     triangle when the texel's closed square meets it.  Centre coverage beats touching, and the lowest prim wins within each
 *                     class: overlapping charts are the caller's business, and the result is a function of the chart alone, bit-identical
 *                     from run to run.  All decisions are made in float64 from the fp32 UVs of the device vertex table.
 *   u, v              the barycentrics of the centre in the owner triangle, p = (1 - u - v) p0 + u p1 + v p2; for a touched texel those of the
 *                     triangle's point nearest to the centre (UV distance).  Rounded to fp32 last and kept at u, v >= 0, u + v <= 1.
 *   flags             reserved[0]: LRHIP_LIGHTMAP_TEXEL_CENTRE or LRHIP_LIGHTMAP_TEXEL_TOUCHED.  A texel nobody owns gets the miss record
 *                     inst = prim = tri = 0xffffffff with flags 0, which every query answers with its invalid record.
 *   What it reads     the instance's mesh in the device's vertex and triangle tables, as lrhip_update_scene and lrhip_set_mesh_vertices left
 *                     them; positions do not matter, only u v and the indices.  The instance's mesh and property flags come from
 *                     the host's copy of its handle as the uploads wrote it: nothing is read back.
 *   Pointers          out: width * height records.  With LRHIP_RAY_DEVICE_POINTERS device memory, 16-byte aligned (else LRHIP_ERROR_INVALID),
 *                     written asynchronously on the context's stream; without it host memory, staged 2^20 records at a time, and the call
 *                     synchronises.
 *   Errors            LRHIP_ERROR_INVALID before any upload, for an instance out of range, NULL out with width * height > 0, unknown flags and
 *                     width * height > LRHIP_RAY_MAX_COUNT; LRHIP_ERROR_UNSUPPORTED for an instance whose mesh has no vertex UVs
 *                     (LR_SHAPE_HAS_VERTEX_UV).  width or height 0 is legal and launches nothing.
 *   Not done          unwrapping, seam dilation, filtered or supersampled texels, several instances in one map.                               */
#define LRHIP_LIGHTMAP_CONSERVATIVE 256u
#define LRHIP_LIGHTMAP_TEXEL_CENTRE 1u
#define LRHIP_LIGHTMAP_TEXEL_TOUCHED 2u
int lrhip_lightmap_texels(lrhip_ctx *ctx, uint32_t instance, uint32_t width, uint32_t height, uint32_t flags, void *out);
/* HIP-event time of the kernels of the last lrhip_lightmap_texels call (a host-pointer call: summed over its chunks), in ms; synchronises */
double lrhip_last_lightmap_ms(lrhip_ctx *ctx);

/* The gather vertex: the plan of ONE irradiance sample at points the caller names -- a path that starts AT a surface point
 * instead of along a camera ray.  For each record, MegaPath's shading vertex for a virtual white Lambert surface at the point (a Matte closure
 * with Kd = 1, sigma = 0 on the record's shading frame, seen from its front): one light sample and one cosine-distributed continuation
 * direction, with the throughput started at pi so that the path's radiance IS the irradiance sample, E = pi L_o.  The caller continues it:
 *     sample = (shadow ray unoccluded ? nee : 0) + beta x (what `ray` finds, each emitter or environment weighted by balance(pdf, its light pdf))
 * with lrhip_trace_rays, lrhip_query_light in evaluate mode and, for deeper paths, the other queries or lrhip_trace_radiance.
 *   Records           lrhip_ray_hit[count], everything the surface, BSDF and light queries take: a hit of lrhip_trace_rays or a texel's
 *                     (inst, prim, u, v) with tri = 0xffffffff (lrhip_lightmap_texels).  With LRHIP_GATHER_FROM_POINTS float[4][count] bare
 *                     positions and, in `normals`, float[4][count] normals of any length but 0 (ng = ns = normalize(n)); both rays then start
 *                     at the point itself, as lrhip_query_light's bare points do.
 *   Random numbers    stream `streams[k]` (NULL: k) at sample index `sample_index`, exactly as lrhip_trace_radiance starts it: stream j is pixel
 *                     (j mod W, (j div W) mod H)'s, the pixel draw and, for a thin lens, the lens draw are drawn and discarded, then the
 *                     vertex's draws follow in MegaPath's order: light selection, light surface (2), lobe (not used), direction (2).  A map
 *                     with more texels than the camera has pixels repeats streams: pass `streams` to decorrelate.
 *   Result            lrhip_gather_vertex: ray = (robust origin, wi, 0, FLT_MAX) and pdf, the cosine density of wi; shadow, nee and light_pdf
 *                     of the light sample (light_pdf = 0: it failed, nee = 0, the shadow ray may be non-finite); beta = pi f / pdf.  The
 *                     point's own emission is not part of it.  The invalid record -- a non-finite u, v, point or normal, a zero normal, ids
 *                     out of range, a miss -- is all zeros, and so is every record of a scene with neither lights nor an environment.
 *   Scope, pointers   MegaPath scenes (else LRHIP_ERROR_UNSUPPORTED); pointers, alignment and errors as for lrhip_query_light.               */
typedef struct lrhip_gather_vertex {
    lrhip_ray ray;            /* the continuation ray */
    lrhip_ray shadow;         /* the light sample's shadow ray */
    float nee[3], light_pdf;
    float beta[3], pdf;
} lrhip_gather_vertex;        /* 96 bytes */
typedef struct lrhip_gather_vertex_params {
    const void *records;      /* lrhip_ray_hit[count]; LRHIP_GATHER_FROM_POINTS: float[4][count] = (p, -) */
    const void *normals;      /* LRHIP_GATHER_FROM_POINTS: float[4][count] = (n, -); else not read */
    const uint32_t *streams;  /* uint32_t[count] or NULL (stream k) */
    void *out;                /* lrhip_gather_vertex[count] */
    uint64_t count;           /* 0 is legal and launches nothing; at most LRHIP_RAY_MAX_COUNT */
    uint32_t sample_index;
    uint32_t flags;           /* LRHIP_RAY_DEVICE_POINTERS, LRHIP_GATHER_FROM_POINTS */
} lrhip_gather_vertex_params;
#define LRHIP_GATHER_FROM_POINTS 64u
int lrhip_query_gather_vertex(lrhip_ctx *ctx, const lrhip_gather_vertex_params *params);

/* Irradiance gathers: the hemisphere integral at points the caller names, on the device -- the second end of a lightmap or
 * probe bake.  For every record, samples [spp_begin, spp_end) of MegaPath's estimator for paths that START at the record's point with the
 * gather vertex above (next-event estimation at the point itself, MIS for what the continuation ray finds, then the scene's own path
 * tracing to its max_depth with its Russian roulette), summed into out[k] = (sum E_r, sum E_g, sum E_b, n): the irradiance is sum / n.
 * The kernels are the radiance query's (lrhip_trace_radiance) with another prologue, so everything of that call holds here:
 *   Records, streams  as lrhip_query_gather_vertex: lrhip_ray_hit records (hits or texels), or with LRHIP_GATHER_FROM_POINTS positions and
 *                     normals; stream streams[k] (NULL: k) is pixel (j mod W, (j div W) mod H)'s, so a map with more texels than the camera
 *                     has pixels repeats streams -- correlated noise, an unbiased mean; pass `streams` to decorrelate.
 *   Samples           the texel is the path's camera end: the continuation ray has depth 0.  A scene with max_depth 0 starts no ray: every
 *                     valid record counts its samples with E = 0.  The point's own emission is not part of E.  Each sample goes through the
 *                     film's accumulate rule (NaN / Inf rejected, clamp -- 0: the scene's film clamp) before it is summed.
 *   Invalid records   (as lrhip_query_gather_vertex) give no sample: n stays 0.  A scene with neither lights nor an environment launches
 *                     nothing and returns the sums of no sample, as lrhip_trace_radiance does; so does spp_begin >= spp_end.
 *   LRHIP_GATHER_ACCUMULATE   out holds earlier sums and is added to (refinement); without it out is cleared first.
 *   Determinism, pointers, scope, errors   as lrhip_trace_radiance: with one sample per call a record's result is a function of (record,
 *                     stream, sample index) alone, wherever it stands in the batch; device pointers 16-byte aligned (streams 4-byte).          */
typedef struct lrhip_gather_params {
    const void *records;      /* lrhip_ray_hit[count]; LRHIP_GATHER_FROM_POINTS: float[4][count] = (p, -) */
    const void *normals;      /* LRHIP_GATHER_FROM_POINTS: float[4][count] = (n, -); else not read */
    const uint32_t *streams;  /* uint32_t[count] or NULL (stream k) */
    void *out;                /* float[4][count]: (sum E_r, sum E_g, sum E_b, n) */
    uint64_t count;           /* 0 is legal and launches nothing; at most LRHIP_RAY_MAX_COUNT */
    uint32_t spp_begin, spp_end;
    uint32_t flags;           /* LRHIP_RAY_DEVICE_POINTERS, LRHIP_GATHER_ACCUMULATE, LRHIP_GATHER_FROM_POINTS */
    float clamp;              /* 0 = the scene's film clamp */
} lrhip_gather_params;
#define LRHIP_GATHER_ACCUMULATE 4u
#define LRHIP_FEAT_GATHER 131072u /* the gather kernels (with LRHIP_FEAT_QUERY; never reported by lrhip_last_variant) */
int lrhip_gather_irradiance(lrhip_ctx *ctx, const lrhip_gather_params *params);
/* HIP-event time of the kernel(s) of the last lrhip_gather_irradiance or lrhip_query_gather_vertex call (a host-pointer call: summed over its
 * chunks), in ms; synchronises */
double lrhip_last_gather_ms(lrhip_ctx *ctx);

/* The path's only collective: sum-reduce of the per-rank films to rank `root` over RCCL / xGMI, in place on the film
 * this context accumulates into, in stream order behind the renders.  `nccl_comm` is the caller's ncclComm_t (one per process /
 * GPU, created by the caller: ncclCommInitRank); librccl.so is loaded on first use, so the library has no link-time dependency
 * on it.  Every pixel is owned by exactly one rank under tile sharding and the others hold exact zeros there, so the reduced
 * film is bit-identical to the 1-GPU film.  The reference has no multi-device path (src/apps/cli.cpp:172,181).              */
int lrhip_film_reduce(lrhip_ctx *ctx, void *nccl_comm, int root);
/* the same for several contexts driven by ONE host thread (one process, one context + communicator per GPU): a single RCCL group */
int lrhip_film_reduce_group(int count, lrhip_ctx *const *ctxs, void *const *comms, int root);

/* Communicators for lrhip_film_reduce, so that a host needs no RCCL headers of its own (librccl.so is loaded on first use):
 *   one process per GPU:  rank 0 calls lrhip_comm_unique_id, ships the 128 bytes to the other ranks by its own means (MPI, a
 *                         file, torch.distributed), every rank calls lrhip_comm_init_rank on its context         (ncclCommInitRank)
 *   one process, N GPUs:  lrhip_comm_init_all(N, device ordinals, comms)                                        (ncclCommInitAll)
 * lrhip_comm_destroy releases one communicator.  lrhip_device_count = hipGetDeviceCount.                                      */
#define LRHIP_COMM_ID_BYTES 128
int lrhip_device_count(int *count);
int lrhip_comm_unique_id(unsigned char id[LRHIP_COMM_ID_BYTES]);
int lrhip_comm_init_rank(lrhip_ctx *ctx, int world, int rank, const unsigned char id[LRHIP_COMM_ID_BYTES], void **comm);
int lrhip_comm_init_all(int count, const int *devices, void **comms);
int lrhip_comm_destroy(void *comm);
/* what a communicator actually spans: out = { ranks (ncclCommCount), this rank (ncclCommUserRank), its HIP device (ncclCommCuDevice) } --
 * so that a host (bench.py's multi_gpu block) can say from its own output whether RCCL saw the N ranks it was launched with */
int lrhip_comm_info(void *comm, int out[3]);

int lrhip_get_counters(lrhip_ctx *ctx, lrhip_counters *out); /* summed since upload; synchronises */
/* HIP-event time of the megakernel launches of the last lrhip_render call, in ms; synchronises */
double lrhip_last_render_ms(lrhip_ctx *ctx);
/* Feature mask of the precompiled megakernel variant the last lrhip_render launched (the reference JIT-compiles one
 * kernel per scene, src/base/integrator.cpp:56-77; here the smallest precompiled superset of the scene's needs is
 * picked): bit 0 counters, 1 generic sampler, 2 image/directional environment, 3 alpha-tested traversal, 4 Disney,
 * 5 Mix, 6 Layered.  The kernel's symbol is lrd::megapath_kernel<mask>.                                          */
#define LRHIP_FEAT_COUNT 1u
#define LRHIP_FEAT_GENERIC_SAMPLER 2u
#define LRHIP_FEAT_ENVIRONMENT 4u
#define LRHIP_FEAT_ALPHA 8u
#define LRHIP_FEAT_DISNEY 16u
#define LRHIP_FEAT_BYTE_TEXELS 8192u /* a lean kernel that decodes 8-bit texels (lrhip_set_texture_storage) */
#define LRHIP_FEAT_PADDED_SOBOL 16384u /* (with LRHIP_FEAT_GENERIC_SAMPLER | LRHIP_FEAT_POOL) a pool kernel compiled for the PaddedSobol sampler */
#define LRHIP_FEAT_MIX 32u
#define LRHIP_FEAT_LAYERED 64u
#define LRHIP_FEAT_AUX_INTEGRATORS 128u
#define LRHIP_FEAT_VOLUMETRIC 256u
#define LRHIP_FEAT_NESTED 512u /* Mix trees with Layered leaves / Layered surfaces with Mix interfaces */
#define LRHIP_FEAT_AOV 32768u  /* the AOV integrator's kernels (lrhip_last_variant: with the all-closures scene bits) */
#define LRHIP_FEAT_QUERY 65536u /* the radiance-query kernels (lrhip_trace_radiance; never reported by lrhip_last_variant) */
uint32_t lrhip_last_variant(lrhip_ctx *ctx);

/* Diagnostics of ONE context, for tests and tools (the product path never calls it; the library reads no environment variable):
 *   force_features  scene-feature bits (LRHIP_FEAT_ENVIRONMENT .. LRHIP_FEAT_LAYERED) OR-ed into what the uploaded scene needs, so
 *                   that a larger precompiled variant renders a scene that does not need it (A/B of variants, twin tests); 0 = none
 *   item_scale      factor on the loss model's constant behind the work-item size of lrhip_render (sweeps); 0 or 1 = default; a
 *                   negative value = its magnitude with UNIFORM work items (rounds 1-2) instead of the tapered ones of round 3.
 *                   A value other than the default changes the order of a pixel's float adds, i.e. the film's last bits.        */
int lrhip_set_diagnostics(lrhip_ctx *ctx, uint32_t force_features, double item_scale);

/* The work-item partition lrhip_render uses for `spp` samples per pixel of a frame cut into `balance_shards` shards (no device
 * needed): out = { chunks per tile, how many of them are big, samples per pixel of a big chunk, of a small chunk }.  Chunk k of a
 * tile covers samples [k * big, ..) for k < big count and [big count * big + (k - big count) * small, ..) after that, clipped to spp;
 * all big items of a launch are handed out before the first small one (items taper towards the end of the launch).              */
int lrhip_work_items(uint32_t width, uint32_t height, uint32_t spp, uint32_t balance_shards, uint32_t out[4]);

/* Wavefront mode (round 3): a scene with Mix or Layered surfaces under the MegaPath integrator is rendered by a lean megakernel that
 * parks the paths reaching a Disney / Mix / Layered surface in HBM queues, a heavy-closure kernel that shades those vertices in full
 * waves of one closure kind, and a continuation pass of the megakernel -- alternating until the queues are empty.  The sample range
 * is cut into slices of `slice_paths` paths of one nominal shard of the frame (tile_count / balance_shards tiles): a function of the
 * frame and the caller's hint only, like the work items, so that films stay bit-identical under sharding and whatever memory is
 * free; a call over more tiles than the queues can hold takes them group after group, which changes no bit.
 *   mode         0 = automatic (default), 1 = never: the all-in-one megakernel variants (A/B, tests),
 *                2 = automatic with queues of seven tiles (the slots of eight, less the hand-over margin of an eighth of a slice's paths;
 *                tests: the tile groups a GPU short of memory would use)
 *                Round 6: a slice runs ONE round and HANDS the paths still parked OVER to the next slice's first round (they are
 *                independent of their slice and add to the frame's order-independent fixed-point sums; the call's last slice runs all its
 *                rounds) -- its remaining rounds moved a few thousand paths each at one batch's latency, 6 % of a kitchen-class frame.
 *                mode | rounds << 8 overrides the one (tests, A/B); mode | 65535 << 8: never, every slice runs all its rounds.
 *   slice_paths  paths per slice (0 = default 2^28: 86 .. 100 GB of queues when a whole slice is in flight, the hand-over margin included)
 * lrhip_last_variant reports LRHIP_FEAT_WAVEFRONT | the lean kernel's bits | the closure bits the heavy kernel served.          */
#define LRHIP_FEAT_WAVEFRONT 1024u
int lrhip_set_wavefront(lrhip_ctx *ctx, uint32_t mode, uint32_t slice_paths);

/* Scheduling of the lean megakernels (round 4).  The path-pool kernels (csrc/hip/megapool_kernel.h) give every lane TWO path contexts:
 * while one context's rays are traced the other waits -- for the shading block with its hit, or for the lane with the rays of its
 * next job -- so that a lane whose job ends goes on with its other context inside the traversal loop (rays and hits in registers,
 * the 64 bytes of path state in a per-thread record, the ray in flight parked in the LDS while the lane shades).  Work items overlap
 * inside a wave and the film is summed in 64-bit fixed point: bit-reproducible under ANY sharding, grid size and work-item
 * partition.  Measured on MI355X (profiles/r04_final_*): lane utilisation of the traversal loop 0.56 -> 0.91, of the shading block
 * 0.47 -> 0.63, films equal to the one-path-per-lane kernels' to 8e-8, and 5 .. 18 % faster on every scene but the smallest ones
 * (a Cornell box: 13 % slower -- a ray is a handful of steps there and the pool's costlier shading block is not paid back).  They
 * serve every scene the lean kernels serve (basic closures and Disney inline, the wavefront-mode passes).
 * The fixed-point film -- the pool kernels' and wavefront mode's alike -- holds film clamp x spp up to 2^37 per call: a call beyond that
 * (a clamp of 1e7 at 65536 spp) is rendered in sample sub-ranges that fit, one after the other (round 5; the film is the same film: a
 * sub-range is what a progressive caller would have passed).  Only a clamp that cannot hold ONE sample (clamping switched off: 1e20,
 * inf) takes the float-accumulating kernels of rounds 1-3 instead -- one path per lane, Mix / Layered scenes on the all-in-one
 * variants (about half the speed of wavefront mode on the kitchen class) -- as do paths deeper than 65535 and the variants with
 * out-of-line closures / sibling integrators / media.  lrhip_last_variant tells which family rendered (LRHIP_FEAT_POOL, LRHIP_FEAT_WAVEFRONT).
 *   mode  0 = automatic: the pool kernels where they are the faster ones -- from 98304 BVH triangles up, from twice that for paths of
 *             depth <= 6, from half of it for scenes of fewer than 64 spp (tools/sched_sweep.py: triangles x depth x spp; the choice is
 *             never more than 1.4 % off the better kernel there) -- one path per lane below;
 *         1 = one path per lane; 2 = the pool kernels wherever one exists for the scene
 * lrhip_last_variant reports LRHIP_FEAT_POOL when the pool kernels rendered.                                                         */
#define LRHIP_FEAT_POOL 4096u
int lrhip_set_scheduler(lrhip_ctx *ctx, uint32_t mode);
/* Texel storage of the NEXT lrhip_upload_scene (round 5).  The host hands every image over as float RGBA texels (lr_scene.texels: what the
 * reference's textures hold).  An image whose every texel is an 8-bit code's float -- decoded from a PNG / JPEG / BMP / TGA file -- can stay
 * 8 bits per channel on the device: a quarter of the footprint in HBM and in the caches, decoded per lookup to exactly the floats the host
 * made (both of the host readers' conversions, b * (1 / 255.f) and b / 255.f, bit for bit: tests/test_gpu_parity.py).
 *   mode  1 = automatic (default): where the scene's image texels exceed 192 MB as floats (below that the caches hold them and the
 *             decode's few instructions per texel are not paid back: kitchen class -1.5 %, camera class +4 %);
 *         0 = never; 2 = every image that qualifies (A/B, tests).
 * Round 6: the decode is compiled into the kernels that need it only (lean kernels of the LRHIP_FEAT_BYTE_TEXELS bit -- the Disney feature
 * sets of both schedulers -- and every variant that makes real calls); a MegaPath scene with alpha-tested, Mix or Layered surfaces or
 * nested Combined environments renders on kernels without it and keeps float texels under mode 1; mode 2 on such a scene is
 * LRHIP_ERROR_UNSUPPORTED at upload.  The float texels of a packed image are not uploaded as well.                                    */
int lrhip_set_texture_storage(lrhip_ctx *ctx, uint32_t mode);
uint64_t lrhip_packed_texels(lrhip_ctx *ctx); /* texels of the uploaded scene held as 8-bit codes (4 bytes each instead of 16) */

/* The automatic rule's threshold (no device needed): the number of BVH triangles from which a scene whose integrator allows paths of
 * `max_depth` vertices and whose description asks for `scene_spp` samples per pixel (0 = unknown) renders on the pool kernels.       */
uint32_t lrhip_pool_auto_triangles(uint32_t max_depth, uint32_t scene_spp);

/* TEST HOOK (no device needed, the product path never calls it): the selection rule of lrhip_render -- which kernels a call of a scene
 * runs on -- for one point of its input space.
 *   features        what the uploaded scene needs: LRHIP_FEAT_ENVIRONMENT .. LRHIP_FEAT_LAYERED, LRHIP_FEAT_NESTED, and the integrator class
 *                   (none: MegaPath; LRHIP_FEAT_AUX_INTEGRATORS / LRHIP_FEAT_VOLUMETRIC / LRHIP_FEAT_AOV, each as lrhip_upload_scene sets it)
 *   force_features  lrhip_set_diagnostics
 *   flags           LRHIP_PLAN_FLAG_*: the call gathers counters; Combined environments nested in each other; the scene holds packed 8-bit texels;
 *                   the scheduler wants the pool kernels (lrhip_set_scheduler, lrhip_pool_auto_triangles); the fixed-point film can hold the call
 *   sampler_kind    LR_SAMPLER_*;  wf_mode: lrhip_set_wavefront;  max_depth: the integrator's
 * out = { family LRHIP_FAMILY_*, mask of the main kernel (wavefront mode: of the camera pass), of the continuation pass, of the heavy kernels
 * of Disney / Mix / Layered (their own numbering: bit 0 counters, 1 generic sampler, 4 Mix, 8 Layered, 512 nested), whether the film is
 * summed in fixed point, whether lrhip_upload_scene packs such a scene's texels at all }; masks that do not apply are 0xffffffff.
 * LRHIP_ERROR_UNSUPPORTED (out still filled) when a kernel of the plan is not compiled into this library.                              */
#define LRHIP_FAMILY_NONE 0u      /* no compiled feature set covers the scene */
#define LRHIP_FAMILY_LANE 1u      /* one path per lane, float film */
#define LRHIP_FAMILY_POOL 2u
#define LRHIP_FAMILY_WAVEFRONT 3u
#define LRHIP_FAMILY_AOV 4u
#define LRHIP_PLAN_FLAG_COUNTERS 1u
#define LRHIP_PLAN_FLAG_ENV_TREE 2u
#define LRHIP_PLAN_FLAG_PACKED_TEXELS 4u
#define LRHIP_PLAN_FLAG_WANTS_POOL 8u
#define LRHIP_PLAN_FLAG_FIXED_FITS 16u
#define LRHIP_PLAN_WORDS 8
int lrhip_plan_kernels(uint32_t features, uint32_t force_features, uint32_t flags, uint32_t sampler_kind, uint32_t wf_mode, uint32_t max_depth,
                       uint32_t out[LRHIP_PLAN_WORDS]);

/* TEST HOOK (the product path never calls it): `bytes` bytes from `byte_offset` of one of the four device tables that move with the geometry,
 * as lrhip_upload_scene / lrhip_update_scene / lrhip_set_instance_transforms / lrhip_set_mesh_vertices left them, copied to `out`.
 * Synchronises.  The tables: the 64-byte BVH packets; the 48-byte baked triangles and, behind the last one, the all-zero sentinel the empty
 * node slots name; the 128-byte instance records; the 128-byte shading records; and, as table 8, the object-space vertex table of 32-byte
 * lr_vertex records that lrhip_set_mesh_vertices writes (ids 4 to 7 name no table).  Tables 16 and 17 are the light sample's records, built
 * on the device: 96 bytes per light instance (its instance id, the base and length of its alias table, its first triangle record; the shape's
 * property flags, tags and offset bits; the four columns of object_to_world, a quad each) and 80 bytes per (light instance, primitive)
 * (object-space p0 p1 p2 with the world-space geometric normal in the quads' fourth words; uv0 uv1; uv2, world-space area, pdf table entry).
 * Table 18 is table 17 once more, as the units without fp contraction bake it (the volumetric and gather kernels, the light and gather queries).
 * LRHIP_ERROR_INVALID before any upload, for an unknown table and for a range that is not inside the table.                              */
#define LRHIP_TABLE_NODES 0u
#define LRHIP_TABLE_BVH_TRIANGLES 1u
#define LRHIP_TABLE_INSTANCES 2u
#define LRHIP_TABLE_SHADE_TRIANGLES 3u
#define LRHIP_TABLE_VERTICES 8u
#define LRHIP_TABLE_LIGHT_INSTANCES 16u
#define LRHIP_TABLE_LIGHT_TRIANGLES 17u
#define LRHIP_TABLE_LIGHT_TRIANGLES_EXACT 18u
int lrhip_read_scene_table(lrhip_ctx *ctx, uint32_t which, uint64_t byte_offset, uint64_t bytes, void *out);
/* size in bytes of that table in the uploaded scene (0: none, or an unknown table) */
uint64_t lrhip_scene_table_bytes(lrhip_ctx *ctx, uint32_t which);

const char *lrhip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* LRHIP_H */
