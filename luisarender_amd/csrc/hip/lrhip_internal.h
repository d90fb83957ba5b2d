// lrhip_internal.h — what the host sources of liblrhip.so share behind include/lrhip.h: the context, device buffers, error reporting, the
// nominal-grid constants, the kernel table and the selection rule's declarations.  The sources, by responsibility:
//   lrhip_context.hip    context, setters, film binding / download, counters; the small film kernels (film_kernels.h) and their launchers
//   lrhip_tables.hip     host-side checks and tables of an upload: index validation, 8-bit texel packing, the time-dependent tables; the light sample's records
//   lrhip_upload.hip     lrhip_upload_scene (in named steps) / lrhip_update_scene
//   lrhip_kernels.hip    the table of compiled kernels (variants.h), the selection rule (plan_kernels), occupancy
//   lrhip_render.hip     work items, fixed-point film, lrhip_render (one path per lane, pool, AOV)
//   lrhip_wavefront.hip  the host loop of wavefront mode
//   lrhip_comm.hip       the RCCL collectives
//   lrhip_denoise.hip    the edge-avoiding wavelet filter over the AOV buffers (denoise_kernels.h)
//   lrhip_query.hip      what the queries and the device updates share on the host: screening, timers, the scene record, staging
//   lrhip_raycast.hip    ray queries: closest hit / occlusion for caller-supplied rays (raycast_kernel.h)
//   lrhip_radiance.hip   radiance queries: MegaPath's estimator along caller-supplied rays (the kFeatQuery kernels of megapath_kernel.h)
//   lrhip_surface.hip    surface queries: position, normals, uv, material and emission at caller-supplied hits (surface_kernel.h)
//   lrhip_bsdf.hip       BSDF queries: the closure evaluated or sampled at caller-supplied hits (bsdf_kernel.h)
//   lrhip_light.hip      light queries: the emitters sampled from, or evaluated at, caller-supplied hits (light_kernel.h)
//   lrhip_camera.hip     camera, sampler and film queries: sampler streams, camera rays, splats into the film (camera_kernel.h)
//   lrhip_gather.hip     the gather vertex query: the plan of one irradiance sample at caller-supplied points (gather_vertex.h, gather_kernel.h)
//   lrhip_lightmap.hip   the UV rasteriser of lightmap baking: texel records of one instance's UV chart (lightmap_kernels.h)
//   lrhip_instance_update.hip  moving instances on the device: re-bake, refit and re-quantise (instance_update_kernels.h); the table test hook
//   lrhip_mesh_update.hip      deforming a mesh on the device: vertex write, normal recompute, marking (mesh_update_kernels.h), then the re-bake and refit
// Written for gfx950 only; no host fallback exists -- without a HIP device every entry point fails with LRHIP_ERROR_DEVICE.
#pragma once
#include "../../../include/lrhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "megapath_kernel.h"
#include "megapool_kernel.h"
#include "light_record_kernels.h"
#include "query_columns.h"
#include "variants.h"

namespace lrh {

int fail(int code, const std::string &msg);// sets the thread's lrhip_last_error text (lrhip_context.hip), returns `code`

#define LR_HIP_CHECK(expr)                                                                                   \
    do {                                                                                                     \
        auto err_ = (expr);                                                                                  \
        if (err_ != hipSuccess) {                                                                            \
            return lrh::fail(LRHIP_ERROR_DEVICE, std::string{#expr} + ": " + hipGetErrorString(err_));       \
        }                                                                                                    \
    } while (0)

struct DeviceBuffer {
    void *ptr{nullptr};
    size_t bytes{0};
    void release() {
        if (ptr != nullptr) { (void)hipFree(ptr); }
        ptr = nullptr, bytes = 0;
    }
};
int ensure(DeviceBuffer &b, size_t bytes);// grows, never shrinks; the contents are lost when it grows

// the kernel time of a family's last call (lrhip_query.hip): events around the last launch, made on first use; the time of the call's
// finished launches; whether a launch is still to be read
struct Timer {
    hipEvent_t begin{nullptr}, end{nullptr};
    double ms{0.};
    bool pending{false};
};
// staging slots of a host-pointer call, one per column of the widest call (staged_call)
constexpr uint32_t kQuerySlots = 5u;

// persistent-grid sizing inputs that must not depend on the device actually present, so that the
// chunking (and therefore the fp32 summation order of the film) is identical on every GPU
constexpr double kNominalWaves = 4096.0;// 256 CUs x 4 SIMDs x 4 waves
constexpr uint32_t kMaxChunks = 64u;     // partial planes: chunk_count x 16 B per pixel
// wavefront mode: rounds of a slice before its parked paths wait for the next slice (film_kernels.h: wf_carry_kernel)
constexpr uint32_t kWfCarryRounds = 1u;
// bytes the queues of wavefront mode may take (of 288 GB; round 6: 104 GB -- the default slice with its hand-over margin takes 86 - 100)
constexpr uint64_t kWfQueueBudget = 104ull << 30u;
#ifndef LR_MAX_BLOCKS_PER_CU
#define LR_MAX_BLOCKS_PER_CU 8
#endif
constexpr uint32_t kMaxBlocksPerCu = LR_MAX_BLOCKS_PER_CU; // resident 256-thread blocks per CU the persistent grid may use (-D: A/B builds)
// channels per pixel of each AOV component (lr_scene.h: LR_AOV_*)
constexpr uint32_t kAovChannels[LR_AOV_COMPONENTS] = {3u, 3u, 3u, 3u, 3u, 1u, 3u, 3u, 1u};

// ---- the compiled kernels (lrhip_kernels.hip): one entry per mask of variants.h, megakernels (LR_MEGAKERNEL_LIST) first, then the
// heavy-closure kernels of wavefront mode (LR_HEAVY_LIST, whose masks are a numbering of their own: `heavy`).  The entry points are weak,
// so that experimental builds may leave kernels out (make hip-variant VARIANT_MASKS=...): a missing one is reported, never silently
// replaced.
struct KernelEntry {
    uint32_t mask;
    bool heavy;
    hipError_t (*launch)(unsigned blocks, hipStream_t, const lrd::DScene *device_scene, const lrd::RenderArgs *, unsigned lds_bytes);
    hipError_t (*occupancy)(int *blocks_per_cu, unsigned lds_bytes);
};
#define LR_COUNT_ONE(mask) +1u
constexpr size_t kKernelCount = 0u LR_MEGAKERNEL_LIST(LR_COUNT_ONE) LR_HEAVY_LIST(LR_COUNT_ONE);
#undef LR_COUNT_ONE
extern const KernelEntry kKernels[kKernelCount];
// the entry of a mask whose entry points are in the loaded library; nullptr: not compiled into it
const KernelEntry *find_kernel(uint32_t mask, bool heavy = false);

// ---- the selection rule (lrhip_kernels.hip: plan_kernels), the one place that decides which kernels a call runs on
struct PlanInputs {
    // lrhip_ctx::features: the scene's lrd::kFeat* bits, with the integrator class (kFeatAux / kFeatVpt / kFeatAov) and kFeatNest
    uint32_t features;
    uint32_t force_features;// lrhip_set_diagnostics
    uint32_t sampler_kind;  // LR_SAMPLER_*
    uint32_t wf_mode;       // lrhip_set_wavefront
    uint32_t max_depth;
    bool count;             // LRHIP_RENDER_COUNTERS
    bool env_tree;          // Combined environments nested in each other
    bool byte_texels;       // the uploaded scene holds packed 8-bit texels
    bool wants_pool;        // the scheduler's choice (lrhip_render.hip: wants_pool)
    bool fixed_fits;        // the fixed-point film can hold this call (fixed_point_bits)
};
constexpr uint32_t kNoKernel = ~0u;
struct KernelPlan {
    uint32_t family;// LRHIP_FAMILY_*
    uint32_t main;  // mask of the kernel that renders; wavefront mode: of the camera pass
    uint32_t cont;  // wavefront mode: the continuation pass
    uint32_t heavy[lrd::kWfKinds];// wavefront mode: the heavy kernel of each closure kind (LR_HEAVY_LIST numbering)
    bool fixed_point;// the film is summed in 64-bit fixed point
};
KernelPlan plan_kernels(const PlanInputs &in);
bool scene_kernels_decode_byte_texels(bool alpha_tested, bool mix_or_layered, bool env_tree, bool megapath);

}// namespace lrh

struct lrhip_ctx {
    int device{0};
    hipStream_t stream{nullptr};
    bool own_stream{true};
    hipEvent_t ev_begin{nullptr}, ev_end{nullptr};
    bool timed{false};
    // 8-bit images as 8-bit texels on the device (lrhip_upload_scene): lrhip_set_texture_storage: 0 never, 1 = where the scene's float
    // texels exceed kByteTextureFloatBytes, 2 always
    uint32_t byte_textures{1u};
    uint64_t packed_texel_words{0u};// texels of the uploaded scene held as 8-bit codes (lrhip_packed_texels)
    uint64_t texel_bytes{0u};       // bytes of the texel table on the device (float texels of the images that stay float + the packed words)
    bool in_split{false};        // lrhip_render is rendering a call in sample sub-ranges: the first sub-range's begin event stands for the call
    std::vector<lrh::DeviceBuffer> scene_buffers;
    lrd::DScene scene{};
    bool scene_ready{false};
    uint32_t width{0}, height{0};
    float film_scale[3]{1.f, 1.f, 1.f};
    lrh::DeviceBuffer film_own, converted, partial, spill, counters, work_counter;
    lrh::DeviceBuffer scene_record;// lrd::DScene in device memory: the kernels read it through scalar loads (dev_scene.h: DScenePtr)
    float4 *film{nullptr};// bound film (own or external)
    float4 *film_external{nullptr};// lrhip_bind_film's buffer; kept across uploads of the same resolution
    uint32_t film_external_w{0}, film_external_h{0};
    uint32_t grid_blocks{0};
    uint32_t cu_count{0};
    uint32_t bvh_depth{0};
    uint32_t update_counts[7]{};// table sizes of the uploaded scene: what lrhip_update_scene checks its argument against
    uint32_t last_variant{0u};// feature mask of the kernel the last lrhip_render launched
    uint32_t features{0u};// lrd::kFeat* bits the uploaded scene needs (environment, alpha test, Disney / Mix / Layered)
    bool env_tree{false};// Combined environments nested in each other: only the call-making variants walk them (dev_shade.h)
    // resident blocks per CU of each kernel of kKernels, same index (-1: not asked yet; kernel_blocks).  lrhip_upload_scene resets it: the
    // AOV kernels' LDS size depends on the uploaded scene
    int kernel_blocks[lrh::kKernelCount];
    uint32_t diag_force_features{0u};// lrhip_set_diagnostics (tests / tools)
    double diag_item_scale{0.};
    // wavefront mode (dev_scene.h: WfArgs): queues, counters and the fixed-point radiance sums; sized on first use
    lrh::DeviceBuffer wf_heavy, wf_cont, wf_counts, wf_accum;
    // lrhip_set_wavefront: 0 = automatic (scenes with Mix / Layered surfaces), 1 = never, 2 = automatic with tiny tile groups (tests)
    uint32_t wf_mode{0u};
    uint32_t wf_slice_paths{0u}; // paths per slice (queue capacity); 0 = default
    // lrhip_set_diagnostics: rounds before a slice hands its parked paths over (0 = kWfCarryRounds; 65535 = never: every slice drains)
    uint32_t diag_wf_carry_rounds{0u};
    // round 4: the path-pool scheduler (megapool_kernel.h): slot records of every resident wave; lrhip_set_scheduler
    lrh::DeviceBuffer pool;
    // lrhip_set_scheduler: 0 = automatic (wants_pool), 1 = one path per lane, 2 = the pool kernels where one exists for the scene
    uint32_t scheduler{0u};
    // the AOV integrator: planar sums [channel][pixel] of the enabled components (lrd::DScene::aov) and the chunks' partial planes
    lrh::DeviceBuffer aov, aov_partial;
    // the denoiser (lrhip_denoise.hip): the guide { N, z } and two ping-pong colours, float4 per pixel each, and lrhip_denoise's copy of
    // its host arrays; they grow on demand and outlive the scene
    lrh::DeviceBuffer denoise_guide, denoise_colour[2], denoise_inputs;
    hipEvent_t denoise_begin{nullptr}, denoise_end{nullptr};// around the kernels of the last call (lrhip_last_denoise_ms); made on first use
    bool denoise_timed{false};
    // The queries and the device updates (lrhip_query.hip).  `staging`: the slots of a host-pointer call, column i of the call in slot i
    // (staged_call); they grow on demand and outlive the scene.  NOTHING STAGED OUTLIVES A CALL: every host-pointer call synchronises per
    // chunk, so a slot is free for whichever call comes next.  The calls list their columns in one order -- 0 the result, 1 rays or sampler
    // states, 2 hit records or ids, 3 numbers or sample indices, 4 rays written -- which is what bounds the slots' sizes.
    // One timer per family (lrhip_last_*_ms)
    lrh::DeviceBuffer staging[lrh::kQuerySlots];
    lrh::Timer raycast_timer, radiance_timer, surface_timer, bsdf_timer, light_timer, camera_timer, instance_timer, mesh_timer;
    int raycast_blocks[2]{-1, -1};// ray queries: resident blocks per CU of the two kernels (alpha test off / on; -1: not asked yet)
    // moving instances (lrhip_instance_update.hip).  Of the uploaded scene (in scene_buffers): the fp32 boxes of the BVH the packets are
    // quantised from, refitted in place, and the node indices sorted by level of the tree -- level l is level_nodes[level_offsets[l] ..
    // level_offsets[l + 1]); empty level_offsets: the node order does not allow a refit (a child before its parent).  Of the context: the
    // staging buffer of a host-pointer call (matrices, then ids) and the call's scratch (owner word per instance, then the moved-instance
    // bits)
    lr_bvh4_node *nodes32{nullptr};
    const uint32_t *level_nodes{nullptr};
    std::vector<uint32_t> level_offsets;
    uint64_t vertex_count{0u};
    lrh::DeviceBuffer update_stage, update_scratch;
    // deforming a mesh (lrhip_mesh_update.hip).  Of the uploaded scene: a host copy of the lr_mesh table, per mesh the first instance that
    // carries a light (LR_INVALID_ID: none -- an emitter's vertices are not moved), and per mesh the corner lists of the normal recompute in
    // device memory, built on first use and released with the scene.  Staging buffer and scratch are the instance call's
    std::vector<lr_mesh> meshes;
    std::vector<uint32_t> mesh_light;
    std::vector<lrh::DeviceBuffer> mesh_adjacency;
    // surface, BSDF and light queries.  Of the uploaded scene: the lr_mesh table in device memory (what bounds `prim` of a record that names
    // an instance), copied on the first such query after an upload (resident_meshes; release_scene clears the flag), and the kFeatDisney /
    // kFeatMix / kFeatLayered bits of its surfaces THEMSELVES, whatever the integrator (`features` above is what the renderer's kernel must
    // hold: the sibling integrators set every closure bit in it and the volumetric one clears them) -- what picks the BSDF query's kernel
    lrh::DeviceBuffer surface_meshes;
    bool surface_meshes_ready{false};
    uint32_t closure_features{0u};
    // the UV rasteriser (lrhip_lightmap.hip): the owner word per texel of the last call's map; grows on demand and outlives the scene
    lrh::DeviceBuffer lightmap_owner;
    // lrd::GatherTable of the gather launch in flight (lrhip_gather.hip), written on the context's stream ahead of every launch
    lrh::DeviceBuffer gather_table;
    // handle[0] of every instance record as lrhip_upload_scene / lrhip_update_scene wrote it (the mesh index and the shape's property flags;
    // no device update changes it): the rasteriser needs no read-back
    std::vector<uint32_t> instance_handles;
    // the light sample's records (dev_scene.h: DLightInstance, DLightTri; lrhip_tables.hip: bake_light_records).  Of the uploaded scene (in
    // scene_buffers): the light instance that owns each triangle record, and the two tables' sizes
    const uint32_t *light_tri_owner{nullptr};
    uint32_t light_record_count{0u}, light_tri_count{0u};
    lrh::Timer lightmap_timer, gather_timer;// (gather_timer: the gather vertex query's, lrhip_gather.hip)
};

namespace lrh {

// resident blocks per CU of `entry` (asked once per upload, at most kMaxBlocksPerCu); `lds_bytes`: the launch's dynamic LDS
int kernel_blocks(lrhip_ctx *ctx, const KernelEntry &entry, unsigned lds_bytes, uint32_t &blocks_per_cu);

// ---- lrhip_query.hip: the one host path of the queries and the device updates
// A call's timer.  timer_start: the device, a call's time of zero, and the events if the call will launch.  timer_begin / timer_end: around a
// launch on the context's stream.  timer_collect: the pending launch's time joins the call's (synchronises with it); `sum`: the call adds
// its launches up (the queries), or keeps the last one (the updates).  timer_read: the whole body of a lrhip_last_*_ms
int timer_start(lrhip_ctx *ctx, Timer &t, bool launches);
int timer_begin(lrhip_ctx *ctx, Timer &t);
int timer_end(lrhip_ctx *ctx, Timer &t);
int timer_collect(Timer &t, bool sum = true);
double timer_read(lrhip_ctx *ctx, Timer &t, bool sum = true);
void timer_destroy(Timer &t);
// What every call checks first, in this order: NULL context or parameters, flags outside `allowed_flags`, more than LRHIP_RAY_MAX_COUNT
// `noun` (nullptr: the call bounds its count itself), no scene uploaded
int screen_call(const char *name, const lrhip_ctx *ctx, const void *params, uint32_t flags, uint32_t allowed_flags, uint64_t count, const char *noun);
template<typename Params>
int screen(const char *name, const lrhip_ctx *ctx, const Params *p, uint32_t allowed_flags, const char *noun) {
    return screen_call(name, ctx, p, p != nullptr ? p->flags : 0u, allowed_flags, p != nullptr ? p->count : 0u, noun);
}
struct PointerMask {
    const void *pointer;
    uintptr_t mask;// 15: 16-byte aligned, 3: 4-byte
};
bool misaligned(std::initializer_list<PointerMask> pointers);// (NULL is aligned)
// ctx->scene, or the caller's modified copy of it, into ctx->scene_record on the context's stream
int upload_scene_record(lrhip_ctx *ctx, lrd::DScenePtr &device_scene, const lrd::DScene *record = nullptr);
int resident_meshes(lrhip_ctx *ctx);// the lr_mesh table of the uploaded scene in ctx->surface_meshes: copied once per upload
// what the surface, BSDF and light kernels' arguments share: the hit records, the rays, the tables that bound a record's ids
template<typename Args>
void fill_hit_table(const lrhip_ctx *ctx, Args &args, const void *hits, const void *rays, uint32_t count) {
    args.hits = static_cast<const float4 *>(hits), args.rays = static_cast<const float4 *>(rays);
    args.meshes = static_cast<const lr_mesh *>(ctx->surface_meshes.ptr);
    args.count = count;
    args.triangle_count = ctx->update_counts[1], args.instance_count = ctx->update_counts[2];
    args.mesh_count = static_cast<uint32_t>(ctx->meshes.size());
}
// blocks of a one-lane-per-record launch: 2^20 blocks of 256 lanes cover 2^28 records in one pass; a larger batch strides
constexpr uint32_t kQueryMaxBlocks = 1u << 20u;
inline uint32_t blocks_of(uint32_t count) { return std::min(kQueryMaxBlocks, (count + lrd::kBlockThreads - 1u) / lrd::kBlockThreads); }
// One call over `count` records, column i of `columns` through ctx->staging[i].  launch(n, first, pointers): one launch over records
// [first, first + n) whose column i is at device address pointers[i] (nullptr: absent), between timer_begin and timer_end of `timer`.
// Device pointers: one launch over the caller's arrays.  Host pointers: per chunk of kQueryChunk records the copies in, the launch, the
// copies out, a synchronise and timer_collect
using QueryLaunch = std::function<int(uint32_t n, uint64_t first, void *const *pointers)>;
int staged_call(lrhip_ctx *ctx, Timer &timer, uint64_t count, bool device_pointers, std::initializer_list<Column> columns, const QueryLaunch &launch);

void release_scene(lrhip_ctx *ctx);// frees the uploaded scene's buffers and what is sized for it (queues, pool records)

// lrhip_tables.hip: host-side checks and tables of an upload (empty string / empty error: fine)
std::string validate_indices(const lr_scene *s);
constexpr uint64_t kByteTextureFloatBytes = 192ull << 20u;// float texels of a scene's images from which lrhip_set_texture_storage mode 1 packs
std::vector<uint32_t> pack_byte_textures(const lr_scene *s, std::vector<lr_texture> &textures);
uint32_t bvh_depth(const lr_accel &accel);
std::vector<lrd::DNodeQ> build_packed_nodes(const lr_scene *s);
std::vector<uint8_t> build_padded_triangles(const lr_scene *s);
std::vector<lrd::DInstance> build_instances(const lr_scene *s);
std::vector<lrd::DShadeTri> build_shade_tris(const lr_scene *s, const std::vector<lrd::DInstance> &instances, std::string &error);
void set_camera(lrd::DScene &d, const lr_scene *s);
// The light sample's records.  upload_light_records: allocates the two tables of the scene being uploaded (their buffers join scene_buffers),
// writes what the host knows -- per light instance its ids and bases, per triangle record its owner -- and bakes every record.
// bake_light_records: the kernels of light_record_kernels.h on the context's stream, over the light instances whose instance has its bit set
// in `moved` (a bit per instance in device memory), or over all of them (nullptr); nothing is launched for a scene without lights
int upload_light_records(lrhip_ctx *ctx, const lr_scene *s);
int bake_light_records(lrhip_ctx *ctx, const uint32_t *moved);
// (lrhip_instance_update.hip: light_triangle_record over `args` with that unit's arithmetic, for DScene::light_tris_exact)
hipError_t launch_light_triangles_exact(lrhip_ctx *ctx, const lrd::LightRecordArgs &args);

// lrhip_render.hip
struct Chunking {
    uint32_t count, big_count, big, small;
};
Chunking chunking_of(uint32_t spp, double shard_tiles, double item_scale, bool taper);
int fixed_point_bits(float film_clamp, float shutter_weight, uint32_t spp);
int ensure_accum(lrhip_ctx *ctx, uint32_t pixel_count);
int ensure_pool(lrhip_ctx *ctx, uint32_t resident_blocks);
// lrhip_wavefront.hip
int render_wavefront(lrhip_ctx *ctx, const lrhip_render_params *p, const KernelPlan &plan, uint32_t tiles_x, uint32_t tiles_y,
                     uint32_t tiles_in_range, uint32_t tile_count);

// launchers of the film kernels (film_kernels.h, compiled into lrhip_context.hip), on the context's stream
hipError_t launch_resolve_partial(lrhip_ctx *ctx, const float4 *partial, uint32_t chunk_count, uint32_t tiles_x, uint32_t tile_begin,
                                  uint32_t tile_end, uint32_t tile_stride);
hipError_t launch_resolve_aov_partial(lrhip_ctx *ctx, uint32_t chunk_count, uint32_t tiles_x, uint32_t tile_begin, uint32_t tile_end,
                                      uint32_t tile_stride);
hipError_t launch_wf_resolve(lrhip_ctx *ctx, double inv_scale);
// resolve_partial_kernel over a "frame" of `count` records instead of the film's pixels (radiance queries): records[i] += sum of partial[c][i]
hipError_t launch_resolve_records(lrhip_ctx *ctx, float4 *records, const float4 *partial, uint32_t count, uint32_t chunk_count);
hipError_t launch_wf_carry(lrhip_ctx *ctx, uint32_t margin, uint32_t mode);

// lrhip_instance_update.hip, for the calls that move geometry on the device (the __global__ functions of instance_update_kernels.h live in
// that object).  The call's scratch is an owner word per instance, then a bit per instance.  clear_update_scratch: sizes it for the uploaded
// scene and clears it on the context's stream.  update_moved_mask: its bit per instance, valid after clear_update_scratch.
// rebake_and_refit: instance_triangle_kernel over the instances whose bit is set, the light sample's records of those instances
// (bake_light_records), then instance_refit_kernel level by level from the deepest up, on the context's stream
int clear_update_scratch(lrhip_ctx *ctx);
uint32_t *update_moved_mask(lrhip_ctx *ctx);
int rebake_and_refit(lrhip_ctx *ctx);

}// namespace lrh
