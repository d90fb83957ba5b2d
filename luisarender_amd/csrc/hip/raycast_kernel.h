// raycast_kernel.h — ray queries (include/lrhip.h: lrhip_trace_rays): closest-hit and occlusion for caller-supplied rays.
//
// Persistent waves over ONE global ray counter, on the renderers' traversal loop (dev_trace.h: trace_steps; with the alpha test,
// dev_shade.h: trace_until_refill) -- this file holds no traversal of its own.  A lane without a ray takes the next index from a
// wave-level grab: one atomic per wave for all its idle lanes -- and for its next few refills, RaycastArgs::grab rays at a time: every
// wave of the device adds to the same word, and at one atomic per 64 rays that word's throughput was what bounded the first form of
// this kernel.  The lane loads its 32-byte ray as two dwordx4 and -- unless the ray is screened out below -- calls
// trav_begin with the ray in the loop's units (raycast_ray below); the wave traces with has_next = false; a lane whose ray ended stores its 32-byte record (closest hit) or its occlusion
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
#ifndef LR_RAYCAST_CALLER_UNITS
#define LR_RAYCAST_CALLER_UNITS 1// 0: the ray goes to the loop as the caller gave it -- right for unit directions and t_min > 0 only; the baseline of raycast_ray's A/B
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

// THE CALLER'S UNITS (lrhip.h: "directions need not be normalised: t is in units of |d|", "the search starts at max(t_min, +0)").  The traversal
// loop is the renderers', whose rays have unit directions and t_min >= 0, and it relies on both: safe_inverse caps |1 / d| at 1e30 per component,
// so the slab tests of a direction shorter than 2^-100 walk along (+-1, +-1, +-1) while the triangle test uses d; the triangle test's products
// underflow or overflow with |d|; and a child whose entry distance max(planes, t_min) is negative or -0.0 has a key with the sign bit set, which
// is how the loop marks a child it missed.  So the prologue hands the loop what it was built for, by the rule of the radiance queries
// (megapath_kernel.h, the kFeatQuery prologue) and surface_unit_direction:
//   * t_min = max(t_min, +0) (a select, so that -0.0 becomes +0 whatever v_max makes of signed zeros);
//   * a direction whose squared length is within 4e-7 of 1 is taken bit for bit -- a normalised ray's result has the bits it always had;
//   * any other finite non-zero d: a power of two first brings its largest component into 2^-60 .. 2^60 (exact; neither the squares nor v_sqrt_f32
//     and v_rcp_f32, 1 ulp each on normal numbers, meet a denormal or overflow), d becomes dp * (1 / len), and the interval's ends take |d| in two
//     factors, len and 2^-k, so that no product is 0 x inf (raycast_scale: in the order that keeps the intermediate in range);
//   * a hit's t goes back to the caller's units at the store, by the factors 1 / len and 2^k: it overflows to +inf or underflows only where the
//     caller's units make it (inst tells a hit from a miss).
// tests/raycast_judge.py derives its error bands from exactly these operations.
struct RaycastUnits {
    float inv_len, pre;// t of the caller = raycast_scale(t of the loop, inv_len, pre); 1, 1 for a direction taken bit for bit
};
// t * f * 2^k, k in (-100, 0, 100) and f within 2^-61 .. 2^61: the power of two goes first where it brings t TOWARDS 1 (|t| >= 1 and k < 0, |t| < 1
// and k > 0) and last otherwise, so that the intermediate leaves float32's range only if the result does.  (t * f) * 2^k alone turns t_max = 2^70
// under |d| = 2^-41 into +inf, where the product is 2^29.  The power of two is exact: one rounding either way.
LR_D float raycast_scale(float t, float f, float pow2) {
    return ((fabsf(t) >= 1.f) == (pow2 < 1.f)) ? (t * pow2) * f : (t * f) * pow2;
}
LR_D Ray raycast_ray(const float4 &a, const float4 &b, RaycastUnits &units) {
    auto d = mk3(b.x, b.y, b.z);
    units.inv_len = 1.f, units.pre = 1.f;
    if (!LR_RAYCAST_CALLER_UNITS) { return Ray{mk3(a.x, a.y, a.z), a.w, d, b.w}; }
    auto t_min = a.w > 0.f ? a.w : 0.f, t_max = b.w;
    if (!(fabsf(dot(d, d) - 1.f) <= 4e-7f)) {
        const auto m = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z));
        const auto pre = m < 0x1p-40f ? 0x1p100f : (m > 0x1p40f ? 0x1p-100f : 1.f);
        const auto unpre = m < 0x1p-40f ? 0x1p-100f : (m > 0x1p40f ? 0x1p100f : 1.f);
        const auto dp = d * pre;
        const auto len = __builtin_amdgcn_sqrtf(dot(dp, dp));
        const auto inv_len = __builtin_amdgcn_rcpf(len);
        d = dp * inv_len;
        t_min = raycast_scale(t_min, len, unpre), t_max = raycast_scale(t_max, len, unpre);
        units.inv_len = inv_len, units.pre = pre;
    }
    return Ray{mk3(a.x, a.y, a.z), t_min, d, t_max};
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
    const auto store = [&](uint32_t k, const TravState &tr, const RaycastUnits &units) {
        if (shadow) {
            words[k] = tr.occluded ? 1u : 0u;
        } else {
            const auto hit = tr.hit.inst != kInvalid;
            const auto record = hits + static_cast<size_t>(k) * 2u;
            record[0] = make_float4(hit ? raycast_scale(tr.t_max, units.inv_len, units.pre) : __uint_as_float(0x7f800000u), tr.hit.u, tr.hit.v, __uint_as_float(tr.hit.inst));
            record[1] = make_float4(__uint_as_float(tr.hit.prim), __uint_as_float(tr.hit.tri), 0.f, 0.f);
        }
    };
    TravState tr{};
    tr.phase = kPhaseIdle;
    auto index = kInvalid; // the ray this lane traces
    RaycastUnits units{1.f, 1.f};// ... and what takes its t back to the caller's units
    auto w_next = 0u, w_end = 0u;// wave-uniform: the rays [w_next, w_end) are this wave's to hand to its lanes
    auto exhausted = false;      // wave-uniform: the counter has passed the last ray
    const Ray none{};
    for (;;) {
        // ---- lanes whose ray ended: store the result
        if (tr.phase == kPhaseIdle && index != kInvalid) {
            store(index, tr, units);
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
                    trav_begin(tr, raycast_ray(a, b, units), args.phase);
                } else {
                    store(k, tr, units);// screened: a miss, and the lane stays idle
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
