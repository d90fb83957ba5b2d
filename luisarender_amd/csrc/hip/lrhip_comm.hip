// lrhip_comm.hip — the multi-GPU path's collectives over RCCL (lrhip_comm_*, lrhip_film_reduce*).
#include "lrhip_internal.h"

#include <dlfcn.h>

using namespace lrh;

namespace {
// librccl.so is loaded on first use (no link-time dependency): the handful of entry points the multi-GPU path needs
struct Rccl {
    using unique_id = struct { char internal[128]; };
    int (*get_unique_id)(unique_id *){nullptr};
    int (*comm_init_rank)(void **, int, unique_id, int){nullptr};
    int (*comm_init_all)(void **, int, const int *){nullptr};
    int (*comm_destroy)(void *){nullptr};
    int (*reduce)(const void *, void *, size_t, int, int, int, void *, hipStream_t){nullptr};
    int (*group_start)(){nullptr};
    int (*group_end)(){nullptr};
    int (*comm_count)(void *, int *){nullptr};// (optional: lrhip_comm_info)
    int (*comm_user_rank)(void *, int *){nullptr};
    int (*comm_device)(void *, int *){nullptr};
    bool ok{false};
    Rccl() {
        auto lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (lib == nullptr) { lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL); }
        if (lib == nullptr) { return; }
        get_unique_id = reinterpret_cast<decltype(get_unique_id)>(dlsym(lib, "ncclGetUniqueId"));
        comm_init_rank = reinterpret_cast<decltype(comm_init_rank)>(dlsym(lib, "ncclCommInitRank"));
        comm_init_all = reinterpret_cast<decltype(comm_init_all)>(dlsym(lib, "ncclCommInitAll"));
        comm_destroy = reinterpret_cast<decltype(comm_destroy)>(dlsym(lib, "ncclCommDestroy"));
        reduce = reinterpret_cast<decltype(reduce)>(dlsym(lib, "ncclReduce"));
        group_start = reinterpret_cast<decltype(group_start)>(dlsym(lib, "ncclGroupStart"));
        group_end = reinterpret_cast<decltype(group_end)>(dlsym(lib, "ncclGroupEnd"));
        comm_count = reinterpret_cast<decltype(comm_count)>(dlsym(lib, "ncclCommCount"));
        comm_user_rank = reinterpret_cast<decltype(comm_user_rank)>(dlsym(lib, "ncclCommUserRank"));
        comm_device = reinterpret_cast<decltype(comm_device)>(dlsym(lib, "ncclCommCuDevice"));
        ok = get_unique_id && comm_init_rank && comm_init_all && comm_destroy && reduce && group_start && group_end;
    }
};
extern "C++" const Rccl &rccl() {
    static Rccl r;
    return r;
}
}// namespace

extern "C" {

int lrhip_device_count(int *count) {
    if (count == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_device_count: NULL argument"); }
    LR_HIP_CHECK(hipGetDeviceCount(count));
    return LRHIP_OK;
}

int lrhip_comm_unique_id(unsigned char id[LRHIP_COMM_ID_BYTES]) {
    if (id == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_comm_unique_id: NULL argument"); }
    if (!rccl().ok) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_comm_unique_id: librccl.so could not be loaded"); }
    Rccl::unique_id u{};
    static_assert(sizeof(u) == LRHIP_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    if (auto rc = rccl().get_unique_id(&u); rc != 0) {
        return fail(LRHIP_ERROR_DEVICE, "ncclGetUniqueId failed with code " + std::to_string(rc));
    }
    std::memcpy(id, &u, sizeof(u));
    return LRHIP_OK;
}

int lrhip_comm_init_rank(lrhip_ctx *ctx, int world, int rank, const unsigned char id[LRHIP_COMM_ID_BYTES], void **comm) {
    if (ctx == nullptr || id == nullptr || comm == nullptr || world < 1 || rank < 0 || rank >= world) {
        return fail(LRHIP_ERROR_INVALID, "lrhip_comm_init_rank: invalid argument");
    }
    if (!rccl().ok) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_comm_init_rank: librccl.so could not be loaded"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    Rccl::unique_id u{};
    std::memcpy(&u, id, sizeof(u));
    if (auto rc = rccl().comm_init_rank(comm, world, u, rank); rc != 0) {
        return fail(LRHIP_ERROR_DEVICE, "ncclCommInitRank failed with code " + std::to_string(rc));
    }
    return LRHIP_OK;
}

int lrhip_comm_init_all(int count, const int *devices, void **comms) {
    if (count < 1 || devices == nullptr || comms == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_comm_init_all: invalid argument"); }
    if (!rccl().ok) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_comm_init_all: librccl.so could not be loaded"); }
    if (auto rc = rccl().comm_init_all(comms, count, devices); rc != 0) {
        return fail(LRHIP_ERROR_DEVICE, "ncclCommInitAll failed with code " + std::to_string(rc));
    }
    return LRHIP_OK;
}

int lrhip_comm_destroy(void *comm) {
    if (comm == nullptr) { return LRHIP_OK; }
    if (!rccl().ok) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_comm_destroy: librccl.so could not be loaded"); }
    if (auto rc = rccl().comm_destroy(comm); rc != 0) {
        return fail(LRHIP_ERROR_DEVICE, "ncclCommDestroy failed with code " + std::to_string(rc));
    }
    return LRHIP_OK;
}

int lrhip_comm_info(void *comm, int out[3]) {
    if (comm == nullptr || out == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_comm_info: NULL argument"); }
    if (!rccl().ok || !rccl().comm_count || !rccl().comm_user_rank || !rccl().comm_device) {
        return fail(LRHIP_ERROR_UNSUPPORTED,
            "lrhip_comm_info: librccl.so (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) could not be loaded");
    }
    if (auto rc = rccl().comm_count(comm, out + 0); rc != 0) {
        return fail(LRHIP_ERROR_DEVICE, "ncclCommCount failed with code " + std::to_string(rc));
    }
    if (auto rc = rccl().comm_user_rank(comm, out + 1); rc != 0) {
        return fail(LRHIP_ERROR_DEVICE, "ncclCommUserRank failed with code " + std::to_string(rc));
    }
    if (auto rc = rccl().comm_device(comm, out + 2); rc != 0) {
        return fail(LRHIP_ERROR_DEVICE, "ncclCommCuDevice failed with code " + std::to_string(rc));
    }
    return LRHIP_OK;
}

int lrhip_film_reduce(lrhip_ctx *ctx, void *nccl_comm, int root) {
    if (ctx == nullptr || !ctx->scene_ready) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_reduce: no scene uploaded"); }
    if (nccl_comm == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_reduce: communicator is NULL"); }
    if (!rccl().ok) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_film_reduce: librccl.so (ncclReduce) could not be loaded"); }
    LR_HIP_CHECK(hipSetDevice(ctx->device));
    auto count = static_cast<size_t>(ctx->width) * ctx->height * 4u;
    // ncclReduce(sendbuff, recvbuff, count, ncclFloat32 = 7, ncclSum = 0, root, comm, stream), rccl.h
    if (auto rc = rccl().reduce(ctx->film, ctx->film, count, 7, 0, root, nccl_comm, ctx->stream); rc != 0) {
        return fail(LRHIP_ERROR_DEVICE, "lrhip_film_reduce: ncclReduce failed with code " + std::to_string(rc));
    }
    return LRHIP_OK;
}

// One host thread drives several contexts of one process (the C++ host's multi-GPU path): the reduces of all of them go out as
// ONE group, as RCCL requires of a single thread that owns several communicators.
int lrhip_film_reduce_group(int count, lrhip_ctx *const *ctxs, void *const *comms, int root) {
    if (count < 1 || ctxs == nullptr || comms == nullptr) { return fail(LRHIP_ERROR_INVALID, "lrhip_film_reduce_group: invalid argument"); }
    if (!rccl().ok) { return fail(LRHIP_ERROR_UNSUPPORTED, "lrhip_film_reduce_group: librccl.so could not be loaded"); }
    if (auto rc = rccl().group_start(); rc != 0) { return fail(LRHIP_ERROR_DEVICE, "ncclGroupStart failed with code " + std::to_string(rc)); }
    auto status = LRHIP_OK;
    for (auto i = 0; i < count && status == LRHIP_OK; i++) { status = lrhip_film_reduce(ctxs[i], comms[i], root); }
    if (auto rc = rccl().group_end(); rc != 0 && status == LRHIP_OK) {
        return fail(LRHIP_ERROR_DEVICE, "ncclGroupEnd failed with code " + std::to_string(rc));
    }
    return status;
}

}// extern "C"
