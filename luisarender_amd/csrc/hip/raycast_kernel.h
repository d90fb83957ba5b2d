// raycast_kernel.h — ray queries (include/lrhip.h: lrhip_trace_rays): closest-hit and occlusion for caller-supplied rays.
//
// Persistent waves over ONE global ray counter, on the renderers' traversal loop (dev_trace.h: trace_steps; with the alpha test,
// dev_shade.h: trace_until_refill) -- this file holds no traversal of its own.  A lane without a ray takes the next index from a
// wave-level grab: one atomic per wave for all its idle lanes -- and for its next few refills, RaycastArgs::grab rays at a time: every
// wave of the device adds to the same word, and at one atomic per 64 rays that word's throughput was what bounded the first form of
// this kernel.  The lane loads its 32-byte ray as two dwordx4 and -- unless the ray is screened out below -- calls
// trav_begin; the wave traces with has_next = false; a lane whose ray ended stores its 32-byte record (closest hit) or its occlusion
// word (any hit) and is idle again.  A lane's walk does not depend on its neighbours, so a ray's result is a function
// of the ray and the scene only: bit-identical from run to run and wherever the ray stands in the batch.
//
// LR_RAYCAST_REFILL: the wave leaves the traversal loop for stores and new rays once that many of the lanes that entered with a ray
// are idle -- the sample queue of megapath_kernel.h (LR_REFILL).  64 = a wave drains all its rays before it takes the next 64: form (A)
// of DESIGN §4.9, the baseline of its A/B (make hip-variant NAME=r64 RAYCAST_DEFS=-DLR_RAYCAST_REFILL=64 VARIANT_MASKS=0 HEAVY_MASKS=).
// 16 is the fastest of the measured forms on incoherent rays: 9394 Mrays/s against 8703 (32), 6887 (48) and 4539 (64) for closest hits of
// random rays in the C2 room (profiles/raycast_ab.txt).
#pragma once
#include "dev_shade.h"

#ifndef LR_RAYCAST_REFILL
#define LR_RAYCAST_REFILL 16
#endif
#ifndef LR_RAYCAST_WAVES
#define LR_RAYCAST_WAVES 4// waves per SIMD asked of the register allocator: what the LDS of a block (stack + staging area) allows anyway
#endif

namespace lrd {

struct RaycastArgs {
    const float4 *rays;    // lrhip_ray[count]: (o, t_min), (d, t_max)
    void *out;             // closest hit: lrhip_ray_hit[count] as two float4 each; any hit: uint32_t[count]
    uint32_t count;        // < 2^31: the counter ends below count + grab per resident wave, which does not wrap
    uint32_t phase;        // kPhaseClosest / kPhaseShadow, wave-uniform
    uint32_t *next;        // the global ray counter, zero at launch
    uint32_t grab;         // rays a wave takes from the counter at a time (a multiple of 64)
    uint32_t *spill;       // traversal stack overflow area [kSpillEntries][total_threads]
    uint32_t total_threads;// gridDim.x * kBlockThreads
};

// SCREENING (lrhip.h): a ray with a non-finite component (t_max = +inf excepted), a zero direction or an empty interval is a miss /
// "not occluded" and never enters the traversal loop -- its lane does not call trav_begin.  Tested on the bits: whatever the build's
// floating-point flags make of comparisons with NaN, an exponent of all ones is not finite.
LR_D bool raycast_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
LR_D bool raycast_ray_valid(const float4 &a, const float4 &b) {
    const auto finite = raycast_finite(a.x) && raycast_finite(a.y) && raycast_finite(a.z) && raycast_finite(a.w) && raycast_finite(b.x) &&
                        raycast_finite(b.y) && raycast_finite(b.z) && (raycast_finite(b.w) || __float_as_uint(b.w) == 0x7f800000u);
    const auto moves = ((__float_as_uint(b.x) | __float_as_uint(b.y) | __float_as_uint(b.z)) & 0x7fffffffu) != 0u;
    return finite && moves && b.w > a.w;// (both finite or t_max = +inf here: an ordinary compare)
}

template<bool ALPHA>
__global__ __launch_bounds__(kBlockThreads, LR_RAYCAST_WAVES) void raycast_kernel(DScenePtr scene_ptr, RaycastArgs args) {
    const DScene &scene = *(const DScene *)scene_ptr;
    __shared__ uint32_t s_stack[kStackLds * kBlockThreads];
    __shared__ float4 s_stage[kWavesPerBlock * kStageWave];// 4 KiB of node packets per wave
    const auto tid = threadIdx.x;
    const auto lane = tid & 63u;
    const auto gtid = blockIdx.x * kBlockThreads + tid;// < args.total_threads: the overflow area holds kSpillEntries rows of that many words
    TraversalStack stack{s_stack + tid, args.spill + gtid, args.total_threads, s_stage + __builtin_amdgcn_readfirstlane(tid >> 6u) * kStageWave};
    const auto shadow = args.phase == kPhaseShadow;
    const auto hits = static_cast<float4 *>(args.out);
    const auto words = static_cast<uint32_t *>(args.out);
    const auto store = [&](uint32_t k, const TravState &tr) {
        if (shadow) {
            words[k] = tr.occluded ? 1u : 0u;
        } else {
            const auto hit = tr.hit.inst != kInvalid;
            const auto record = hits + static_cast<size_t>(k) * 2u;
            record[0] = make_float4(hit ? tr.t_max : __uint_as_float(0x7f800000u), tr.hit.u, tr.hit.v, __uint_as_float(tr.hit.inst));
            record[1] = make_float4(__uint_as_float(tr.hit.prim), __uint_as_float(tr.hit.tri), 0.f, 0.f);
        }
    };
    TravState tr{};
    tr.phase = kPhaseIdle;
    auto index = kInvalid; // the ray this lane traces
    auto w_next = 0u, w_end = 0u;// wave-uniform: the rays [w_next, w_end) are this wave's to hand to its lanes
    auto exhausted = false;      // wave-uniform: the counter has passed the last ray
    const Ray none{};
    for (;;) {
        // ---- lanes whose ray ended: store the result
        if (tr.phase == kPhaseIdle && index != kInvalid) {
            store(index, tr);
            index = kInvalid;
        }
        // ---- idle lanes take the next rays of the wave's own range; an empty range is refilled with ONE atomic for the whole wave
        const auto idle = tr.phase == kPhaseIdle;
        const auto mask = lr_ballot(idle);
        if (!exhausted && mask != 0ull) {
            if (w_next == w_end) {
                auto base = 0u;
                if (lane == 0u) { base = atomicAdd(args.next, args.grab); }
                base = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base)));
                w_next = min(base, args.count), w_end = min(base + args.grab, args.count);// (base <= count + grab per resident wave < 2^32: no wrap)
                exhausted = w_next == w_end;
            }
            // (the lanes the range does not reach wait for the next one: once per args.grab rays)
            const auto rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32u), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
            const auto mine = idle && rank < w_end - w_next;
            const auto k = w_next + rank;
            w_next += min(static_cast<uint32_t>(__popcll(mask)), w_end - w_next);
            if (mine) {
                const auto rp = args.rays + static_cast<size_t>(k) * 2u;
                const auto a = rp[0], b = rp[1];
                tr.hit.inst = kInvalid, tr.hit.prim = kInvalid, tr.hit.tri = kInvalid, tr.hit.u = 0.f, tr.hit.v = 0.f;
                tr.occluded = false;
                if (raycast_ray_valid(a, b)) {
                    index = k;
                    trav_begin(tr, Ray{mk3(a.x, a.y, a.z), a.w, mk3(b.x, b.y, b.z), b.w}, args.phase);
                } else {
                    store(k, tr);// screened: a miss, and the lane stays idle
                }
            }
        }
        if (!lr_any(tr.phase != kPhaseIdle)) {
            if (exhausted) { break; }
            continue;// (a wave of screened rays)
        }
        // ---- all 64 lanes walk until LR_RAYCAST_REFILL of the rays in flight have ended (or all of them)
        TraceStats ts{};
        if constexpr (ALPHA) { trace_until_refill<false, true>(scene, stack, tr, false, none, LR_RAYCAST_REFILL, ts); }
        else { trace_steps<false, false>(scene, stack, tr, false, none, LR_RAYCAST_REFILL, ts, tr.phase == kPhaseIdle); }
    }
}

}// namespace lrd
