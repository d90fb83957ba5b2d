// lrhip_upload.hip — scene upload into HBM (lrhip_upload_scene) and the per-shutter-sample update (lrhip_update_scene).
#include "lrhip_internal.h"

#include <array>
#include <functional>
#include <map>
#include <set>

using namespace lrh;

namespace {

template<typename T>
int upload(lrhip_ctx *ctx, const T *host, size_t count, const T **device) {
    DeviceBuffer b;
    b.bytes = std::max<size_t>(count * sizeof(T), 16u);
    LR_HIP_CHECK(hipMalloc(&b.ptr, b.bytes));
    ctx->scene_buffers.emplace_back(b);
    if (count != 0u) { LR_HIP_CHECK(hipMemcpy(b.ptr, host, count * sizeof(T), hipMemcpyHostToDevice)); }
    *device = static_cast<const T *>(b.ptr);
    return LRHIP_OK;
}

// a failed step returns its code; lrhip_upload_scene releases what was uploaded so far
#define LR_UP(call)                                                    \
    if (auto rc_ = (call); rc_ != LRHIP_OK) { return rc_; }

// textures: 8-bit images are uploaded as 8-bit texels (lrhip_tables.hip: pack_byte_textures; dev_shade.h: texel_at), behind the float texels
int upload_textures(lrhip_ctx *ctx, const lr_scene *s) {
    auto &d = ctx->scene;
    std::vector<lr_texture> textures(s->textures, s->textures + s->texture_count);
    // ... where the float texels are more than the caches hold: the decode costs a few instructions per texel, which a scene whose
    // images sit in the L2 / Infinity Cache anyway does not get back (kitchen class, 36 MB of float texels: -1.5 % packed; camera
    // class, 512 MB: +4 %; the same frame at 128 MB of float texels: +-0 -- profiles/r05zd_byte_textures.txt,
    // r05zc_byte_textures_always.txt, r05zb_c4_texture_size.txt)
    auto image_texels = static_cast<uint64_t>(0u);
    for (auto &t : textures) { if (t.kind == LR_TEX_IMAGE) { image_texels += static_cast<uint64_t>(t.width) * t.height; } }
    // ... and where the kernels the scene renders on decode them (scene_kernels_decode_byte_texels)
    auto mix_or_layered = false, nested_env = false;
    for (uint32_t i = 0; i < s->surface_count; i++) {
        mix_or_layered = mix_or_layered || s->surfaces[i].kind == LR_SURFACE_MIX || s->surfaces[i].kind == LR_SURFACE_LAYERED;
    }
    if (s->environment.kind == LR_ENV_COMBINED) {
        for (uint32_t i = 0; i < s->environment_child_count; i++) {
            nested_env = nested_env || s->environment_children[i].kind == LR_ENV_COMBINED;
        }
    }
    // (the rule lives beside the selection rule it must agree with: lrhip_kernels.hip, plan_kernels)
    const auto decodes = scene_kernels_decode_byte_texels(s->any_non_opaque != 0u, mix_or_layered, nested_env,
                                                          s->integrator.kind == LR_INTEGRATOR_MEGAPATH);
    if (ctx->byte_textures == 2u && !decodes) {
        return fail(LRHIP_ERROR_UNSUPPORTED,
            "lrhip_upload_scene: texture storage mode 2 (always 8-bit texels) on a scene whose kernels do not decode them "
                                             "(alpha-tested, Mix or Layered surfaces, nested Combined environments under MegaPath)");
    }
    const auto pack = decodes && (ctx->byte_textures == 2u || (ctx->byte_textures == 1u && image_texels * 16u > kByteTextureFloatBytes));
    for (auto &t : textures) { t.pad = 0u; }
    const auto packed = pack ? pack_byte_textures(s, textures) : std::vector<uint32_t>{};
    // The float texels of an image that is held packed do NOT go to the device as well (the camera class kept 512 MB of dead
    // floats beside its 128 MB of codes): what is uploaded is the union of the texel ranges the float-kept images name, closed up, with
    // their offsets rebased (ranges that overlap -- two records over one image -- stay one range).
    std::vector<std::pair<uint64_t, uint64_t>> ranges;// [begin, end) in texels, of the images that stay float
    for (auto &t : textures) {
        const auto count = static_cast<uint64_t>(t.width) * t.height;
        if (t.kind == LR_TEX_IMAGE && t.pad == 0u && count != 0u && t.texel_offset + count <= s->texel_count) {
            ranges.emplace_back(t.texel_offset, t.texel_offset + count);
        }
    }
    std::sort(ranges.begin(), ranges.end());
    std::vector<std::array<uint64_t, 3>> kept;// merged ranges: begin, end, where it starts on the device
    uint64_t kept_texels = 0u;
    for (auto &r : ranges) {
        if (!kept.empty() && r.first <= kept.back()[1]) {
            if (r.second > kept.back()[1]) { kept_texels += r.second - kept.back()[1], kept.back()[1] = r.second; }
        } else {
            kept.push_back({r.first, r.second, kept_texels}), kept_texels += r.second - r.first;
        }
    }
    // (nothing packed: the table as the host made it)
    if (packed.empty()) { kept.assign(1u, {0u, s->texel_count, 0u}), kept_texels = s->texel_count; }
    for (auto &t : textures) {
        if (t.kind != LR_TEX_IMAGE) { continue; }
        if (t.pad != 0u) { t.texel_offset += kept_texels * 4u; continue; }// packed: 32-bit words from the same base, behind the floats
        for (auto &k : kept) {
            if (t.texel_offset >= k[0] && t.texel_offset < k[1]) { t.texel_offset = t.texel_offset - k[0] + k[2]; break; }
        }
    }
    LR_UP(upload(ctx, textures.data(), textures.size(), &d.textures));
    DeviceBuffer b;
    const auto float_bytes = static_cast<size_t>(kept_texels) * 4u * sizeof(float);
    b.bytes = std::max<size_t>(float_bytes + packed.size() * sizeof(uint32_t), 16u);
    LR_HIP_CHECK(hipMalloc(&b.ptr, b.bytes));
    ctx->scene_buffers.emplace_back(b);
    for (auto &k : kept) {
        if (k[1] > k[0]) {
            LR_HIP_CHECK(hipMemcpy(static_cast<char *>(b.ptr) + k[2] * 16u, s->texels + k[0] * 4u, (k[1] - k[0]) * 16u, hipMemcpyHostToDevice));
        }
    }
    if (!packed.empty()) {
        LR_HIP_CHECK(hipMemcpy(static_cast<char *>(b.ptr) + float_bytes, packed.data(), packed.size() * sizeof(uint32_t),
            hipMemcpyHostToDevice));
    }
    d.texels = static_cast<const float *>(b.ptr);
    ctx->packed_texel_words = packed.size();
    ctx->texel_bytes = b.bytes;
    return LRHIP_OK;
}

// surfaces and their closures; the scene's closure feature bits (ctx->features)
int upload_surfaces(lrhip_ctx *ctx, const lr_scene *s) {
    auto &d = ctx->scene;
    // closures: fold constant textures on the host (same arithmetic as the per-hit device path)
    auto is_constant = [&](int32_t id) { return id < 0 || s->textures[id].kind == LR_TEX_CONSTANT; };
    std::vector<lrd::DClosure> closures(s->surface_count);
    // the surfaces as the device reads them for dynamic closures: the host's record + every texture slot's value where its texture is
    // constant + which slots need a lookup per hit (dev_scene.h: DSurface)
    std::vector<lrd::DSurface> surfaces(s->surface_count);
    for (uint32_t i = 0; i < s->surface_count; i++) {
        auto &rec = surfaces[i];
        std::memset(&rec, 0, sizeof(rec));
        rec.raw = s->surfaces[i];
        for (auto slot = 0u; slot < lrd::kSurfaceSlots; slot++) {
            const auto id = rec.raw.tex[slot];
            if (id < 0) { continue; }
            auto &t = s->textures[id];
            if (t.kind == LR_TEX_CONSTANT) { std::memcpy(rec.value[slot], t.v, sizeof(t.v)); }
            else { rec.dynamic_mask |= 1u << slot; }
            rec.channels[slot >> 3u] |= (t.channels & 15u) << ((slot & 7u) * 4u);
        }
        rec.first_lookup = rec.raw.normal_tex >= 0 ? rec.raw.normal_tex : (rec.dynamic_mask != 0u
            ? rec.raw.tex[__builtin_ctz(rec.dynamic_mask)] : -1);
    }
    LR_UP(upload(ctx, surfaces.data(), surfaces.size(), &d.surfaces));
    for (uint32_t i = 0; i < s->surface_count; i++) {
        auto &surf = s->surfaces[i];
        if (surf.kind == LR_SURFACE_DISNEY) { ctx->features |= lrd::kFeatDisney; }
        if (surf.kind == LR_SURFACE_MIX) { ctx->features |= lrd::kFeatMix; }
        if (surf.kind == LR_SURFACE_LAYERED) { ctx->features |= lrd::kFeatLayered | lrd::kFeatDisney; }
        // composition of the two (validate_indices checked the child indices)
        if (surf.kind == LR_SURFACE_MIX || surf.kind == LR_SURFACE_LAYERED) {
            // The interpreters of dev_heavy.h assume what the C++ loader enforces (scene.cpp: depth_of, surface_layered_levels); a
            // C-ABI caller gets the same answer here instead of silently wrong shading: at most LR_LAYERED_MAX_LEVELS Layered surfaces on
            // a path through the interfaces, Mix trees at most kMixMaxDepth levels deep with u[2] = that depth, no cycles.
            std::string bad;
            // (memoised per (surface, Layered levels above it): subtrees shared between parents -- a DAG from a C-ABI caller -- are walked
            // once, not once per path to them; a surface met again while it is still being walked is a cycle)
            std::map<std::pair<uint32_t, uint32_t>, int> memo;
            std::set<std::pair<uint32_t, uint32_t>> walking;
            std::function<int(uint32_t, uint32_t, uint32_t)> depth_of_inner;
            std::function<int(uint32_t, uint32_t, uint32_t)> depth_of = [&](uint32_t tag, uint32_t budget, uint32_t layered_above) -> int {
                const auto key = std::make_pair(tag, layered_above);
                if (auto it = memo.find(key); it != memo.end()) { return it->second; }
                if (!walking.insert(key).second) {
                    bad = "a Mix / Layered tree that is cyclic or deeper than the interpreter reaches"; return 0;
                }
                const auto d = depth_of_inner(tag, budget, layered_above);
                walking.erase(key);
                if (bad.empty()) { memo.emplace(key, d); }
                return d;
            };
            depth_of_inner = [&](uint32_t tag, uint32_t budget, uint32_t layered_above) -> int {
                auto &c = s->surfaces[tag];
                if (budget == 0u) { bad = "a Mix / Layered tree that is cyclic or deeper than the interpreter reaches"; return 0; }
                if (c.kind == LR_SURFACE_LAYERED) {
                    if (layered_above >= static_cast<uint32_t>(LR_LAYERED_MAX_LEVELS)) {
                        bad = "Layered surfaces nested more than " + std::to_string(LR_LAYERED_MAX_LEVELS) + " levels deep are not supported";
                        return 0;
                    }
                    depth_of(c.u[0], budget - 1u, layered_above + 1u), depth_of(c.u[1], budget - 1u, layered_above + 1u);
                    return 1;// a leaf of the tree that holds it (its own interfaces count from zero)
                }
                if (c.kind != LR_SURFACE_MIX) { return 0; }
                auto depth = std::max(depth_of(c.u[0], budget - 1u, layered_above), depth_of(c.u[1], budget - 1u, layered_above));
                if (bad.empty() && static_cast<int>(c.u[2]) != depth) { bad = "a Mix surface whose u[2] is not the depth of its tree"; }
                if (bad.empty() && depth > lrd::kMixMaxDepth) {
                    bad = "Mix surfaces nested more than " + std::to_string(lrd::kMixMaxDepth) + " levels deep are not supported";
                }
                return 1 + depth;
            };
            depth_of(i, (static_cast<uint32_t>(lrd::kMixMaxDepth) + 2u) * (static_cast<uint32_t>(LR_LAYERED_MAX_LEVELS) + 1u) + 2u, 0u);
            if (!bad.empty()) {
                return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_upload_scene: surface " + std::to_string(i) + ": " + bad);
            }
            for (auto k = 0u; k < 2u; k++) {
                auto child = s->surfaces[surf.u[k]].kind;
                if ((surf.kind == LR_SURFACE_MIX && child == LR_SURFACE_LAYERED) || (surf.kind == LR_SURFACE_LAYERED
                        && (child == LR_SURFACE_MIX || child == LR_SURFACE_LAYERED))) {
                    ctx->features |= lrd::kFeatNest;
                }
            }
        }
        auto dynamic = surf.normal_tex >= 0;
        for (auto t : surf.tex) { dynamic = dynamic || !is_constant(t); }
        lrd::DClosure c{};
        if (!dynamic) {
            c = lrd::resolve_closure(
                surf,
                [&](int slot) {
                    auto &t = s->textures[surf.tex[slot]];
                    return make_float4(t.v[0], t.v[1], t.v[2], t.v[3]);
                },
                [&](int slot) { return s->textures[surf.tex[slot]].channels; }, 1.f);
        } else {
            c.kind = surf.kind;
            c.x[0] = surf.u[0], c.x[1] = surf.u[1], c.x[2] = surf.u[2], c.x[3] = surf.u[3];// children / masks are needed before resolution
        }
        c.dynamic = dynamic ? 1u : 0u;
        closures[i] = c;
    }
    LR_UP(upload(ctx, closures.data(), closures.size(), &d.closures));
    return LRHIP_OK;
}

int upload_lights(lrhip_ctx *ctx, const lr_scene *s) {
    auto &d = ctx->scene;
    std::vector<lrd::DLight> lights(s->light_count);
    for (uint32_t i = 0; i < s->light_count; i++) {
        auto &src = s->lights[i];
        lrd::DLight l{};
        l.emission_tex = src.emission_tex, l.scale = src.scale, l.two_sided = src.two_sided;
        auto &t = s->textures[src.emission_tex];
        l.dynamic = t.kind == LR_TEX_CONSTANT ? 0u : 1u;
        if (!l.dynamic) {// evaluate_illuminant_spectrum of a static texture, texture.cpp:49-53,77-79
            auto rgb = lrd::extend_rgb(make_float4(t.v[0], t.v[1], t.v[2], t.v[3]), t.channels);
            auto sv = lrd::max0(rgb) * src.scale;
            l.L[0] = sv.x, l.L[1] = sv.y, l.L[2] = sv.z;
        }
        lights[i] = l;
    }
    LR_UP(upload(ctx, lights.data(), lights.size(), &d.lights));
    return LRHIP_OK;
}

// the environment's records; kFeatEnv and ctx->env_tree
int upload_environment(lrhip_ctx *ctx, const lr_scene *s) {
    auto &d = ctx->scene;
    d.env_kind = lrd::kEnvNone;
    d.env = nullptr;
    if (s->environment.kind != LR_ENV_NONE) {
        auto &e = s->environment;
        if (e.kind != LR_ENV_COMBINED && (e.emission_tex < 0 || static_cast<uint32_t>(e.emission_tex) >= s->texture_count)) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: environment without an emission texture");
        }
        auto &t = s->textures[e.kind == LR_ENV_COMBINED ? 0 : e.emission_tex];
        if (e.kind == LR_ENV_SPHERICAL && t.kind == LR_TEX_CONSTANT) {
            d.env_kind = lrd::kEnvConstant;
            auto sv = lrd::max0(lrd::extend_rgb(make_float4(t.v[0], t.v[1], t.v[2], t.v[3]), t.channels)) * e.scale;
            d.env_L[0] = sv.x, d.env_L[1] = sv.y, d.env_L[2] = sv.z;
            std::memcpy(d.env_to_world, e.env_to_world, sizeof(d.env_to_world));
        } else {
            // one DEnvironment per record; a Combined root points at its two children
            auto make_record = [&](const lr_environment &r, lrd::DEnvironment &de) -> int {
                auto &rt = s->textures[r.emission_tex];
                de = lrd::DEnvironment{};
                std::memcpy(de.world_to_env, r.world_to_env, sizeof(de.world_to_env));
                std::memcpy(de.env_to_world, r.env_to_world, sizeof(de.env_to_world));
                de.emission_tex = r.emission_tex, de.scale = r.scale;
                de.constant_emission = rt.kind == LR_TEX_CONSTANT ? 1u : 0u;
                std::memcpy(de.direction, r.direction, sizeof(de.direction));
                de.cos_half_angle = r.cos_half_angle, de.visible = r.visible;
                if (r.kind == LR_ENV_DIRECTIONAL) { de.kind = lrd::kEnvDirectional; return LRHIP_OK; }
                if (r.kind != LR_ENV_SPHERICAL) { return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: invalid environment record"); }
                if (rt.kind == LR_TEX_CONSTANT) { de.kind = lrd::kEnvConstant; return LRHIP_OK; }
                if (r.alias == nullptr || r.pdf == nullptr || r.map_width == 0u || r.map_height == 0u) {
                    return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: image-based Spherical environment without importance tables");
                }
                de.kind = lrd::kEnvImage;
                de.map_width = r.map_width, de.map_height = r.map_height;
                auto texels = static_cast<size_t>(r.map_width) * r.map_height;
                if (auto rc2 = upload(ctx, r.alias, texels + r.map_height, &de.alias); rc2 != LRHIP_OK) { return rc2; }
                return upload(ctx, r.pdf, texels, &de.pdf);
            };
            ctx->features |= lrd::kFeatEnv;
            // a Combined node points at its two children (uploaded before it: lr_scene.h orders children before parents)
            std::vector<const lrd::DEnvironment *> uploaded(e.kind == LR_ENV_COMBINED ? s->environment_child_count : 0u, nullptr);
            auto make_node = [&](const lr_environment &r, lrd::DEnvironment &de) -> int {
                if (r.kind != LR_ENV_COMBINED) { return make_record(r, de); }
                de = lrd::DEnvironment{};
                std::memcpy(de.world_to_env, r.world_to_env, sizeof(de.world_to_env));
                std::memcpy(de.env_to_world, r.env_to_world, sizeof(de.env_to_world));
                de.kind = lrd::kEnvCombined;
                for (auto k = 0; k < 2; k++) {
                    de.child_scale[k] = r.child_scale[k], de.child[k] = uploaded[r.child[k]];
                    if (s->environment_children[r.child[k]].kind == LR_ENV_COMBINED) { de.tree = 1u; }
                }
                return LRHIP_OK;
            };
            lrd::DEnvironment root{};
            int rc2 = LRHIP_OK;
            for (uint32_t i = 0; i < uploaded.size() && rc2 == LRHIP_OK; i++) {
                lrd::DEnvironment child{};
                if ((rc2 = make_node(s->environment_children[i], child)) == LRHIP_OK) { rc2 = upload(ctx, &child, 1u, &uploaded[i]); }
            }
            if (rc2 == LRHIP_OK) { rc2 = make_node(e, root); }
            // a root over nested Combined nodes is walked by out-of-line code that only the call-making variants hold (dev_shade.h:
            // env_evaluate_tree); lrhip_render picks one of those
            ctx->env_tree = root.tree != 0u;
            if (rc2 == LRHIP_OK) { rc2 = upload(ctx, &root, 1u, &d.env); }
            if (rc2 != LRHIP_OK) {
                return rc2;
            }
            d.env_kind = root.kind;
        }
    }
    return LRHIP_OK;
}

// the Sobol samplers' matrices and the bytewise tables built from them
int upload_sampler_tables(lrhip_ctx *ctx, const lr_scene *s) {
    auto &d = ctx->scene;
    if (s->sampler.sobol_matrices == nullptr || (d.sampler_kind == LR_SAMPLER_SOBOL && d.sobol_scale > 1u
            && (s->sampler.vdc_sobol == nullptr || s->sampler.vdc_sobol_inv == nullptr))) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: Sobol sampler without its tables");
    }
    int rc2;
    if ((rc2 = upload(ctx, s->sampler.sobol_matrices, static_cast<size_t>(LR_SOBOL_DIMENSIONS) * LR_SOBOL_MATRIX_SIZE,
        &d.sobol_matrices)) != LRHIP_OK ||
        (s->sampler.vdc_sobol != nullptr &&
         ((rc2 = upload(ctx, s->sampler.vdc_sobol, static_cast<size_t>(LR_SOBOL_MATRIX_SIZE), &d.vdc_sobol)) != LRHIP_OK ||
          (rc2 = upload(ctx, s->sampler.vdc_sobol_inv, static_cast<size_t>(LR_SOBOL_MATRIX_SIZE), &d.vdc_sobol_inv)) != LRHIP_OK))) {
        return rc2;
    }
    if (d.sampler_kind == LR_SAMPLER_SOBOL) {
        // the global Sobol sampler multiplies a 52-bit index with the generator matrix of the draw's dimension (sobol.cpp:52-60: one
        // table word per set bit).  The product is linear over GF(2), so it is the XOR of one precomputed word per index BYTE:
        // [dimension][byte][256] words, 7.3 MB, built here from the same matrices (bit-identical results; dev_shade.h: sobol_bits)
        constexpr size_t kBytes = (LR_SOBOL_MATRIX_SIZE + 7) / 8;
        std::vector<uint32_t> table(static_cast<size_t>(LR_SOBOL_DIMENSIONS) * kBytes * 256u, 0u);
        for (size_t dim = 0; dim < LR_SOBOL_DIMENSIONS; dim++) {
            auto m = s->sampler.sobol_matrices + dim * LR_SOBOL_MATRIX_SIZE;
            for (size_t k = 0; k < kBytes; k++) {
                auto t = table.data() + (dim * kBytes + k) * 256u;
                for (uint32_t b = 1u; b < 256u; b++) {
                    auto bit = 8u * static_cast<uint32_t>(k) + static_cast<uint32_t>(__builtin_ctz(b));
                    t[b] = t[b & (b - 1u)] ^ (bit < static_cast<uint32_t>(LR_SOBOL_MATRIX_SIZE) ? m[bit] : 0u);
                }
            }
        }
        if ((rc2 = upload(ctx, table.data(), table.size(), &d.sobol_bytes)) != LRHIP_OK) {
            return rc2;
        }
        // the same for the two 64-bit products that turn (pixel, sample number) into the sample's index in the global sequence
        // (_sobol_interval_to_index, sobol.cpp:67-96): [byte][256] each
        d.vdc_bytes = nullptr, d.vdc_inv_bytes = nullptr;
        if (s->sampler.vdc_sobol != nullptr) {
            auto bytewise = [&](const uint64_t *rows) {
                std::vector<uint64_t> t(kBytes * 256u, 0ull);
                for (size_t k = 0; k < kBytes; k++) {
                    for (uint32_t b = 1u; b < 256u; b++) {
                        auto bit = 8u * static_cast<uint32_t>(k) + static_cast<uint32_t>(__builtin_ctz(b));
                        t[k * 256u + b] = t[k * 256u + (b & (b - 1u))] ^ (bit < static_cast<uint32_t>(LR_SOBOL_MATRIX_SIZE) ? rows[bit] : 0ull);
                    }
                }
                return t;
            };
            auto vdc = bytewise(s->sampler.vdc_sobol), inv = bytewise(s->sampler.vdc_sobol_inv);
            if ((rc2 = upload(ctx, vdc.data(), vdc.size(), &d.vdc_bytes)) != LRHIP_OK || (rc2 = upload(ctx, inv.data(), inv.size(),
                    &d.vdc_inv_bytes)) != LRHIP_OK) {
                return rc2;
            }
        }
    }
    return LRHIP_OK;
}

// what lrhip_set_instance_transforms refits the tree from (lrhip_instance_update.hip): the fp32 boxes and the nodes by level.  refit_accel
// (csrc/host/accel.cpp) walks the nodes from the last to the first because children have larger indices than their parents; the same property
// gives every node a level in one ascending pass.  A tree without it is rendered like any other, but cannot be refitted on the device
int upload_refit_tables(lrhip_ctx *ctx, const lr_scene *s) {
    const lr_bvh4_node *nodes32 = nullptr;
    LR_UP(upload(ctx, s->accel.nodes, s->accel.node_count, &nodes32));
    ctx->nodes32 = const_cast<lr_bvh4_node *>(nodes32);
    ctx->vertex_count = s->vertex_count;
    // what lrhip_set_mesh_vertices checks its argument against (lrhip_mesh_update.hip): the mesh table, and which meshes emit
    ctx->meshes.assign(s->meshes, s->meshes + s->mesh_count);
    ctx->mesh_light.assign(s->mesh_count, LR_INVALID_ID);
    ctx->mesh_adjacency.assign(s->mesh_count, DeviceBuffer{});
    for (uint32_t i = 0u; i < s->instance_count; i++) {
        const auto handle = s->instances[i].handle.x;
        if ((handle & LR_SHAPE_HAS_LIGHT) != 0u && (handle >> 10u) < s->mesh_count && ctx->mesh_light[handle >> 10u] == LR_INVALID_ID) {
            ctx->mesh_light[handle >> 10u] = i;
        }
    }
    const auto n = s->accel.node_count;
    std::vector<uint32_t> level(n, 0u);
    auto depth = 0u;
    auto ordered = true;
    for (uint32_t i = 0u; i < n && ordered; i++) {
        for (auto c : s->accel.nodes[i].child) {
            if (c == LR_INVALID_ID || (c & 0x80000000u) != 0u) { continue; }
            if (c <= i || c >= n) { ordered = false; break; }
            level[c] = std::max(level[c], level[i] + 1u);
        }
        depth = std::max(depth, level[i]);
    }
    ctx->level_offsets.clear();
    if (!ordered) { return LRHIP_OK; }
    std::vector<uint32_t> offsets(depth + 2u, 0u), sorted(n);
    for (uint32_t i = 0u; i < n; i++) { offsets[level[i] + 1u]++; }
    for (size_t l = 1u; l < offsets.size(); l++) { offsets[l] += offsets[l - 1u]; }
    auto next = offsets;
    for (uint32_t i = 0u; i < n; i++) { sorted[next[level[i]]++] = i; }
    LR_UP(upload(ctx, sorted.data(), sorted.size(), &ctx->level_nodes));
    ctx->level_offsets = std::move(offsets);
    return LRHIP_OK;
}

// everything lrhip_upload_scene puts on the device and into ctx->scene, step by step
int upload_scene_tables(lrhip_ctx *ctx, const lr_scene *s) {
    auto &d = ctx->scene;
    d = lrd::DScene{};
    {
        auto packed = build_packed_nodes(s);
        LR_UP(upload(ctx, packed.data(), packed.size(), &d.nodes));
    }
    LR_UP(upload_refit_tables(ctx, s));
    {
        auto padded = build_padded_triangles(s);
        const uint8_t *dev = nullptr;
        LR_UP(upload(ctx, padded.data(), padded.size(), &dev));
        d.bvh_tris = reinterpret_cast<const lr_bvh_triangle *>(dev);
    }
    LR_UP(upload(ctx, s->vertices, s->vertex_count, &d.vertices));
    LR_UP(upload(ctx, s->triangles, s->triangle_count, &d.triangles));
    LR_UP(upload(ctx, s->tri_alias, s->triangle_count, &d.tri_alias));
    LR_UP(upload(ctx, s->tri_pdf, s->triangle_count, &d.tri_pdf));
    LR_UP(upload(ctx, s->light_instances, s->light_instance_count, &d.light_instances));
    LR_UP(upload_textures(ctx, s));
    LR_UP(upload(ctx, &s->filter, 1u, &d.filter));
    auto instances = build_instances(s);
    LR_UP(upload(ctx, instances.data(), instances.size(), &d.instances));
    // (what lrhip_lightmap_texels reads an instance's mesh and property flags from: the device record's first word, kept on the host)
    ctx->instance_handles.resize(instances.size());
    for (size_t i = 0u; i < instances.size(); i++) { ctx->instance_handles[i] = instances[i].handle[0]; }
    {
        std::string error;
        auto shade = build_shade_tris(s, instances, error);
        if (!error.empty()) { return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: " + error); }
        LR_UP(upload(ctx, shade.data(), shade.size(), &d.shade_tris));
    }
    LR_UP(upload_light_records(ctx, s));// (reads the instance, vertex, triangle and pdf tables above on the device)
    LR_UP(upload_surfaces(ctx, s));
    // the surfaces' own closure bits, before the integrator's class rewrites ctx->features below: what picks a BSDF query's kernel
    ctx->closure_features = ctx->features & (lrd::kFeatDisney | lrd::kFeatMix | lrd::kFeatLayered);
    LR_UP(upload_lights(ctx, s));
    set_camera(d, s);
    LR_UP(upload_environment(ctx, s));
    d.max_depth = s->integrator.max_depth, d.rr_depth = s->integrator.rr_depth;
    d.integrator_kind = s->integrator.kind, d.integrator_flags = s->integrator.flags;
    if (s->integrator.kind > LR_INTEGRATOR_AOV) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_upload_scene: unknown integrator kind"); }
    d.env_medium_tag = s->integrator.environment_medium_tag;
    const auto nested = (ctx->features & lrd::kFeatNest) != 0u;
    if (s->integrator.kind == LR_INTEGRATOR_VPT_NAIVE) {// the volumetric megakernel is one kernel with everything in it
        for (uint32_t i = 0; i < s->instance_count; i++) {
            if ((s->instances[i].handle.x & LR_SHAPE_HAS_MEDIUM) && (s->instances[i].handle.y >> 24u) >= s->medium_count) {
                return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: an instance references a medium that is not in scene->media");
            }
        }
        if (d.env_medium_tag != LR_INVALID_ID && d.env_medium_tag >= s->medium_count) {
            return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: invalid environment medium tag");
        }
        if (auto r = upload(ctx, s->media, s->medium_count, &d.media); r != LRHIP_OK) { return r; }
        ctx->features = lrd::kFeatVpt;
        if (nested) {
            return fail(LRHIP_ERROR_UNSUPPORTED,
                "lrhip_upload_scene: Mix / Layered surfaces nested in each other are supported by the MegaPath integrator only");
        }
    } else if (s->integrator.kind == LR_INTEGRATOR_AOV) {// the AOV integrator has kernels of its own on top of the all-closures mask
        if (nested) {
            return fail(LRHIP_ERROR_UNSUPPORTED,
                "lrhip_upload_scene: Mix / Layered surfaces nested in each other are supported by the MegaPath integrator only");
        }
        ctx->features |= lrd::kFeatSceneMask | lrd::kFeatAov;
    } else if (s->integrator.kind != LR_INTEGRATOR_MEGAPATH) {
        if (nested) {
            return fail(LRHIP_ERROR_UNSUPPORTED,
                "lrhip_upload_scene: Mix / Layered surfaces nested in each other are supported by the MegaPath integrator only");
        }
        // the sibling integrators (Direct / Normal) live in the all-features variant only
        ctx->features |= lrd::kFeatSceneMask | lrd::kFeatAux;
    }
    d.rr_threshold = s->integrator.rr_threshold, d.env_prob = s->integrator.env_prob;
    d.light_count = s->integrator.light_count;
    d.has_lights = s->light_count != 0u ? 1u : 0u;
    d.sampler_kind = s->sampler.kind, d.seed = s->sampler.seed;
    d.sampler_spp = s->sampler.spp, d.sobol_scale = s->sampler.scale;
    if (s->sampler.tile_size[0] > 0xffffu || s->sampler.tile_size[1] > 0xffffu
            || (s->sampler.tile_size[0] != 0u) != (s->sampler.tile_size[1] != 0u)) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: invalid sampler tile size");
    }
    d.sampler_tile = s->sampler.tile_size[0] | (s->sampler.tile_size[1] << 16u), d.sampler_tile_jitter = s->sampler.tile_jitter;
    // (the generic samplers keep a pixel as x | y << 16)
    if (s->camera.width == 0u || s->camera.height == 0u || s->camera.width > 0xffffu || s->camera.height > 0xffffu) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: the film must be 1 .. 65535 pixels wide and high");
    }
    if (d.sampler_kind == LR_SAMPLER_SOBOL || d.sampler_kind == LR_SAMPLER_PADDED_SOBOL) { LR_UP(upload_sampler_tables(ctx, s)); }
    d.film_clamp = s->film.clamp;
    for (auto i = 0; i < 3; i++) { ctx->film_scale[i] = s->film.scale[i]; }
    ctx->width = s->camera.width, ctx->height = s->camera.height;
    auto film_bytes = static_cast<size_t>(ctx->width) * ctx->height * sizeof(float4);
    if (auto r = ensure(ctx->film_own, film_bytes); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->converted, film_bytes); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->counters, sizeof(lrd::DCounters)); r != LRHIP_OK) { return r; }
    if (auto r = ensure(ctx->work_counter, 1024u); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemset(ctx->counters.ptr, 0, sizeof(lrd::DCounters)));
    // a caller-owned film (lrhip_bind_film) stays bound across uploads of the same resolution (MegaPathRenderer.render_frame
    // uploads per shutter sample); a resolution change unbinds it -- its size is no longer the frame's
    if (ctx->film_external != nullptr && ctx->film_external_w == ctx->width && ctx->film_external_h == ctx->height) {
        ctx->film = ctx->film_external;
    } else {
        ctx->film_external = nullptr;
        ctx->film = static_cast<float4 *>(ctx->film_own.ptr);
    }
    LR_HIP_CHECK(hipMemset(ctx->film, 0, film_bytes));
    // the AOV buffers of the enabled components (lr_integrator.flags), in LR_AOV_* order
    d.aov = nullptr, d.aov_partial = nullptr, d.aov_channels = 0u;
    for (uint32_t k = 0u; k < LR_AOV_COMPONENTS; k++) {
        const auto on = s->integrator.kind == LR_INTEGRATOR_AOV && (s->integrator.flags & LR_AOV_BIT(k)) != 0u;
        d.aov_offset[k] = on ? d.aov_channels : lrd::kInvalid;
        if (on) { d.aov_channels += kAovChannels[k]; }
    }
    if (d.aov_channels != 0u) {
        const auto aov_bytes = static_cast<size_t>(ctx->width) * ctx->height * d.aov_channels * sizeof(float);
        if (auto r = ensure(ctx->aov, aov_bytes); r != LRHIP_OK) { return r; }
        LR_HIP_CHECK(hipMemset(ctx->aov.ptr, 0, aov_bytes));
        d.aov = static_cast<float *>(ctx->aov.ptr);
    }
    // persistent grid: as many blocks as are resident, asked per kernel at its first launch (kernel_blocks; the AOV kernels' answer depends
    // on this scene's channels); the traversal-stack overflow area is sized for the densest variant
    for (auto &b : ctx->kernel_blocks) { b = -1; }
    ctx->grid_blocks = ctx->cu_count * kMaxBlocksPerCu;
    auto total_threads = static_cast<size_t>(ctx->grid_blocks) * lrd::kBlockThreads;
    if (auto r = ensure(ctx->spill, total_threads * lrd::kSpillEntries * sizeof(uint32_t)); r != LRHIP_OK) { return r; }
    ctx->update_counts[0] = s->accel.node_count, ctx->update_counts[1] = s->accel.triangle_count, ctx->update_counts[2] = s->instance_count;
    ctx->update_counts[3] = static_cast<uint32_t>(s->triangle_count), ctx->update_counts[4] = s->texture_count;
    ctx->update_counts[5] = s->surface_count;
    ctx->update_counts[6] = s->environment.kind;
    ctx->scene_ready = true;
    return LRHIP_OK;
}
#undef LR_UP

}// namespace

extern "C" {

int lrhip_update_scene(lrhip_ctx *ctx, const lr_scene *s) {
    if (ctx == nullptr || !ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_update_scene: no scene uploaded"); }
    if (s == nullptr || s->camera.width != ctx->width || s->camera.height != ctx->height) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_update_scene: the film resolution must not change");
    }
    // Only what Pipeline::update / Geometry::update move is copied again (instance matrices, the baked triangles and their
    // shading records, the refitted BVH packets, camera and environment transforms), over the SAME device buffers: a frame with
    // 256 shutter samples must not push its textures and environment tables through PCIe 256 times.  Everything else must be
    // the scene that was uploaded; the table sizes are the part of that contract that can be checked.
    if (s->accel.nodes == nullptr || s->accel.node_count != ctx->update_counts[0] || s->accel.triangle_count != ctx->update_counts[1] ||
        s->instance_count != ctx->update_counts[2] || s->triangle_count != ctx->update_counts[3] || s->vertex_count != ctx->vertex_count ||
        s->texture_count != ctx->update_counts[4] || s->surface_count != ctx->update_counts[5] || s->environment.kind != ctx->update_counts[6]) {
        return fail(LRHIP_ERROR_INVALID,
            "lrhip_update_scene: not the uploaded scene at another time (table sizes differ); use lrhip_upload_scene");
    }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    if (bvh_depth(s->accel) != ctx->bvh_depth) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_update_scene: the BVH topology changed; use lrhip_upload_scene");
    }
    auto &d = ctx->scene;
    auto copy = [&](const void *device, const void *host, size_t bytes) {// stream-ordered behind the renders that still read the old tables
        return bytes == 0u ? hipSuccess : hipMemcpyAsync(const_cast<void *>(device), host, bytes, hipMemcpyHostToDevice, ctx->stream);
    };
    auto packed = build_packed_nodes(s);
    auto instances = build_instances(s);
    std::string error;
    auto shade = build_shade_tris(s, instances, error);
    if (!error.empty()) { return fail(LRHIP_ERROR_INVALID, "lrhip_update_scene: " + error); }
    LR_HIP_CHECK(copy(d.nodes, packed.data(), packed.size() * sizeof(packed[0])));
    auto padded = build_padded_triangles(s);
    LR_HIP_CHECK(copy(d.bvh_tris, padded.data(), padded.size()));
    LR_HIP_CHECK(copy(d.instances, instances.data(), instances.size() * sizeof(instances[0])));
    ctx->instance_handles.resize(instances.size());
    for (size_t i = 0u; i < instances.size(); i++) { ctx->instance_handles[i] = instances[i].handle[0]; }
    LR_HIP_CHECK(copy(d.shade_tris, shade.data(), shade.size() * sizeof(shade[0])));
    // the fp32 boxes a later lrhip_set_instance_transforms refits from: the host's tables win again
    LR_HIP_CHECK(copy(ctx->nodes32, s->accel.nodes, static_cast<size_t>(s->accel.node_count) * sizeof(lr_bvh4_node)));
    // ... and the object-space vertices it, and lrhip_set_mesh_vertices, re-bake from: either side may have deformed a mesh since
    LR_HIP_CHECK(copy(d.vertices, s->vertices, static_cast<size_t>(s->vertex_count) * sizeof(lr_vertex)));
    // the light sample's records follow the instances and vertices just copied (an animated emitter: re-baked per shutter sample)
    if (auto r = bake_light_records(ctx, nullptr); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));// the host vectors above go out of scope
    set_camera(d, s);
    if (d.env_kind == lrd::kEnvConstant) {
        std::memcpy(d.env_to_world, s->environment.env_to_world, sizeof(d.env_to_world));
    } else if (d.env != nullptr && s->environment.kind != LR_ENV_COMBINED) {// (animated Combined environments are rejected by the host loader)
        // the record's two matrices lead the struct: overwrite them in place
        float m[18];
        std::memcpy(m, s->environment.world_to_env, sizeof(float) * 9u);
        std::memcpy(m + 9, s->environment.env_to_world, sizeof(float) * 9u);
        static_assert(offsetof(lrd::DEnvironment, world_to_env) == 0u && offsetof(lrd::DEnvironment, env_to_world) == sizeof(float) * 9u,
            "DEnvironment layout");
        LR_HIP_CHECK(hipMemcpy(const_cast<lrd::DEnvironment *>(d.env), m, sizeof(m), hipMemcpyHostToDevice));
    }
    return LRHIP_OK;
}

int lrhip_upload_scene(lrhip_ctx *ctx, const lr_scene *s) {
    if (ctx == nullptr || s == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: NULL argument"); }
    if (s->accel.nodes == nullptr || s->accel.node_count == 0u) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: scene->accel is not built (lrhost_scene_build_accel)");
    }
    if (s->environment.kind > LR_ENV_COMBINED || (s->environment.kind == LR_ENV_COMBINED && (s->environment_child_count < 2u
            || s->environment_children == nullptr))) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_upload_scene: environment kind not supported");
    }
    if (auto bad = validate_indices(s); !bad.empty()) { return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: " + bad); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    release_scene(ctx);
    ctx->bvh_depth = bvh_depth(s->accel);
    if (ctx->bvh_depth == 0u) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_upload_scene: the BVH must have one-triangle leaves (lrhost_scene_build_accel builds them)");
    }
    ctx->features = s->any_non_opaque != 0u ? lrd::kFeatAlpha : 0u;
    ctx->closure_features = 0u;
    ctx->env_tree = false;
    // a leaf names its triangle in 27 bits (the sentinel of the empty slots is one more); the traversal loop addresses packets and leaf
    // triangles by 32-bit byte offsets from their table bases (64 B x 2^26 packets, 48 B x 89 478 484 triangles = 4 GiB)
    constexpr uint32_t kMaxBvhTriangles = static_cast<uint32_t>((1ull << 32u) / sizeof(lr_bvh_triangle)) - 2u;
    static_assert(sizeof(lr_bvh_triangle) == 48u && kMaxBvhTriangles < lrd::kLeafIndexMask,
        "dev_trace.h: trav_leaf_fetch multiplies the leaf's triangle index by 48 in 32 bits");
    if (s->accel.triangle_count >= kMaxBvhTriangles || s->accel.node_count >= (1u << 26u)) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_upload_scene: more than 89 478 482 BVH triangles or 2^26 - 1 BVH packets");
    }
    // a walk pushes at most three entries per level; a pool kernel parks five more words on top of a lane's stack across the shading block
    // (megapool_kernel.h).  From the constants of THIS build: the `make shallow` library keeps 4 entries in LDS, not 16
    if (ctx->bvh_depth * 3u + lrd::kPoolParkedWords > lrd::kStackLds + lrd::kSpillEntries) {
        return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_upload_scene: BVH depth " + std::to_string(ctx->bvh_depth) +
                                                 " exceeds the traversal stack capacity");
    }
    const auto rc = upload_scene_tables(ctx, s);
    if (rc != LRHIP_OK) { release_scene(ctx); }
    return rc;
}

}// extern "C"
