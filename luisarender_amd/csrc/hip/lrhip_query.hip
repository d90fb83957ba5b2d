// lrhip_query.hip — the one host path of the queries (lrhip_raycast / radiance / surface / bsdf / light / camera.hip) and of the device
// updates (lrhip_instance_update / mesh_update.hip): what a call checks first, the timer of a family's last call, the scene record of a
// launch, the lr_mesh table, and a host-pointer call's way through the staging slots.  Host code only: no kernel lives here.
#include "lrhip_internal.h"

namespace lrh {

int timer_start(lrhip_ctx *ctx, Timer &t, bool launches) {
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    t.ms = 0.0, t.pending = false;
    if (!launches) { return LRHIP_OK; }
    if (t.begin == nullptr) { LR_HIP_CHECK(hipEventCreate(&t.begin)); }
    if (t.end == nullptr) { LR_HIP_CHECK(hipEventCreate(&t.end)); }
    return LRHIP_OK;
}

int timer_begin(lrhip_ctx *ctx, Timer &t) {
    LR_HIP_CHECK(hipEventRecord(t.begin, ctx->stream));
    return LRHIP_OK;
}

int timer_end(lrhip_ctx *ctx, Timer &t) {
    LR_HIP_CHECK(hipEventRecord(t.end, ctx->stream));
    t.pending = true;
    return LRHIP_OK;
}

int timer_collect(Timer &t, bool sum) {
    if (!t.pending) { return LRHIP_OK; }
    float ms = 0.f;
    LR_HIP_CHECK(hipEventSynchronize(t.end));
    LR_HIP_CHECK(hipEventElapsedTime(&ms, t.begin, t.end));
    t.ms = (sum ? t.ms : 0.0) + static_cast<double>(ms);
    t.pending = false;
    return LRHIP_OK;
}

double timer_read(lrhip_ctx *ctx, Timer &t, bool sum) {
    if (hipSetDevice(ctx->device) != hipSuccess || timer_collect(t, sum) != LRHIP_OK) { return -1.0; }
    return t.ms;
}

void timer_destroy(Timer &t) {
    if (t.begin != nullptr) { (void)hipEventDestroy(t.begin); }
    if (t.end != nullptr) { (void)hipEventDestroy(t.end); }
    t = Timer{};
}

int screen_call(const char *name, const lrhip_ctx *ctx, const void *params, uint32_t flags, uint32_t allowed_flags, uint64_t count, const char *noun) {
    const auto what = std::string{name} + ": ";
    if (ctx == nullptr || params == nullptr) { return fail(LRHIP_ERROR_INVALID, what + "NULL argument"); }
    if ((flags & ~allowed_flags) != 0u) { return fail(LRHIP_ERROR_INVALID, what + "unknown flags"); }
    if (noun != nullptr && count > LRHIP_RAY_MAX_COUNT) { return fail(LRHIP_ERROR_INVALID, what + "more than 2^31 - 1 " + noun); }
    if (!ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, what + "no scene uploaded"); }
    return LRHIP_OK;
}

bool misaligned(std::initializer_list<PointerMask> pointers) {
    for (auto &p : pointers) {
        if ((reinterpret_cast<uintptr_t>(p.pointer) & p.mask) != 0u) { return true; }
    }
    return false;
}

// The scene record of a launch: the uploaded scene as the host holds it now (lrhip_render writes one per launch; none exists before the first
// render), or the caller's copy of it with the fields of its own call.  `record` is pageable host memory: hipMemcpyAsync has staged it when
// it returns, so a copy on the caller's stack may go out of scope -- do not pin it
int upload_scene_record(lrhip_ctx *ctx, lrd::DScenePtr &device_scene, const lrd::DScene *record) {
    if (auto r = ensure(ctx->scene_record, sizeof(lrd::DScene)); r != LRHIP_OK) { return r; }
    LR_HIP_CHECK(hipMemcpyAsync(ctx->scene_record.ptr, record != nullptr ? record : &ctx->scene, sizeof(lrd::DScene), hipMemcpyHostToDevice,
                                ctx->stream));
    device_scene = (lrd::DScenePtr) static_cast<const lrd::DScene *>(ctx->scene_record.ptr);
    return LRHIP_OK;
}

// (the host copy of the table is lrhip_set_mesh_vertices')
int resident_meshes(lrhip_ctx *ctx) {
    if (ctx->surface_meshes_ready) { return LRHIP_OK; }
    const auto bytes = ctx->meshes.size() * sizeof(lr_mesh);
    if (auto r = ensure(ctx->surface_meshes, std::max<size_t>(bytes, 16u)); r != LRHIP_OK) { return r; }
    if (bytes != 0u) { LR_HIP_CHECK(hipMemcpyAsync(ctx->surface_meshes.ptr, ctx->meshes.data(), bytes, hipMemcpyHostToDevice, ctx->stream)); }
    ctx->surface_meshes_ready = true;
    return LRHIP_OK;
}

int staged_call(lrhip_ctx *ctx, Timer &timer, uint64_t count, bool device_pointers, std::initializer_list<Column> columns, const QueryLaunch &launch) {
    if (columns.size() > kQuerySlots) { return fail(LRHIP_ERROR_INVALID, "staged_call: more columns than staging slots"); }
    const auto cols = columns.begin();
    const auto n_cols = static_cast<uint32_t>(columns.size());
    void *pointers[kQuerySlots]{};
    if (device_pointers) {
        for (uint32_t c = 0u; c < n_cols; c++) {
            pointers[c] = cols[c].host;
            if (cols[c].use == kColumnClear && cols[c].host != nullptr) {
                LR_HIP_CHECK(hipMemsetAsync(cols[c].host, 0, static_cast<size_t>(count) * cols[c].bytes, ctx->stream));
            }
        }
        return launch(static_cast<uint32_t>(count), 0u, pointers);
    }
    for (uint32_t c = 0u; c < n_cols; c++) {
        const auto bytes = slot_bytes(cols[c], count);
        if (bytes == 0u) { continue; }
        if (auto r = ensure(ctx->staging[c], bytes); r != LRHIP_OK) { return r; }
        pointers[c] = ctx->staging[c].ptr;
    }
    for (uint64_t i = 0u; i < chunk_count(count); i++) {
        const auto span = chunk_span(count, i);
        for (uint32_t c = 0u; c < n_cols; c++) {
            const auto s = column_span(cols[c], span);
            if (pointers[c] == nullptr) { continue; }
            if ((cols[c].use & kColumnIn) != 0u) { LR_HIP_CHECK(hipMemcpyAsync(pointers[c], s.host, s.bytes, hipMemcpyHostToDevice, ctx->stream)); }
            if (cols[c].use == kColumnClear) { LR_HIP_CHECK(hipMemsetAsync(pointers[c], 0, s.bytes, ctx->stream)); }
        }
        if (auto r = launch(static_cast<uint32_t>(span.n), span.first, pointers); r != LRHIP_OK) { return r; }
        for (uint32_t c = 0u; c < n_cols; c++) {
            const auto s = column_span(cols[c], span);
            if (pointers[c] != nullptr && (cols[c].use & kColumnOut) != 0u) {
                LR_HIP_CHECK(hipMemcpyAsync(s.host, pointers[c], s.bytes, hipMemcpyDeviceToHost, ctx->stream));
            }
        }
        LR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (auto r = timer_collect(timer); r != LRHIP_OK) { return r; }
    }
    return LRHIP_OK;
}

}// namespace lrh
