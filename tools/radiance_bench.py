#!/usr/bin/env python3
"""Msamples/s of lrhip_trace_radiance from lrhip_last_radiance_ms -- HIP events around the kernel -- on the bench's C2 room,
next to lrhip_render of the same frame forced onto the kernel the query is an instantiation of: the all-closures one-path-per-lane kernel
(set_diagnostics(force_features=124), set_scheduler(pool=False); lrhip_last_render_ms).  The query's rays are the room camera's rays through
the pixel centres of the RES x RES frame, ray py * RES + px with that pixel's sampler stream, SPP samples each in one call, in device
memory.  Two warm-up rounds, then RUNS rounds that alternate the two; the medians, their ratio, and the counting twins (one run of the render, two of
the query: lane utilisations, wave cycles per path of each section, and the counting kernels' own times -- they are other binaries than
the timed ones).  One JSON line per result.

    python tools/radiance_bench.py [--res 512] [--spp 64] [--runs 7] [--triangles 600000]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from luisarender_amd import Scene  # noqa: E402
from luisarender_amd.render import MegaPathRenderer  # noqa: E402
from luisarender_amd.scenes import generate_room_scene  # noqa: E402
from raycast_bench import primary_rays  # noqa: E402

ALL_CLOSURES = 124  # LRHIP_FEAT_ENVIRONMENT | ALPHA | DISNEY | MIX | LAYERED


def utilisation(c):
    """what the counting twins say about where a launch's cycles go"""
    return {"trace_lane_utilisation": round(c["trace_steps_busy"] / max(c["trace_steps"], 1), 4),
            "shade_share_of_wave_cycles": round(c["shade_cycles"] / max(c["wave_cycles"], 1), 4),
            "regen_share_of_shade_cycles": round(c["shade_regen_cycles"] / max(c["shade_cycles"], 1), 4),
            "regen_cycles_per_path": round(c["shade_regen_cycles"] / max(c["paths"], 1), 2),
            # wave cycles per path of the launch and of its sections (summed over waves: 64 lanes share a wave's cycle)
            "wave_cycles_per_path": round(c["wave_cycles"] / max(c["paths"], 1), 1),
            "shade_cycles_per_path": round(c["shade_cycles"] / max(c["paths"], 1), 1),
            "trace_cycles_per_path": round(c["trace_cycles"] / max(c["paths"], 1), 1),
            "light_cycles_per_path": round(c["shade_light_cycles"] / max(c["paths"], 1), 1),
            "closure_cycles_per_path": round(c["shade_closure_cycles"] / max(c["paths"], 1), 1),
            "shade_rounds": c["shade_calls"] // 64, "shade_lane_utilisation": round(c["shade_busy"] / max(c["shade_calls"], 1), 4),
            "paths": c["paths"], "closest_rays": c["closest_rays"], "shadow_rays": c["shadow_rays"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--triangles", type=int, default=600_000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("radiance_bench: no GPU -- a rate is a measurement on the device, there is no fallback")
    device = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(prefix="radiance_bench_") as out_dir:
        scene = Scene.load(generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(args.res, args.res), spp=args.spp,
                                               inline_meshes=True))
    renderer = MegaPathRenderer(0)
    renderer.upload(scene)
    renderer.set_diagnostics(force_features=ALL_CLOSURES)
    renderer.set_scheduler(pool=False)
    rays = primary_rays(torch, device, args.res)
    rays[:, 3] = 0.0
    torch.cuda.synchronize()
    samples = args.res * args.res * args.spp
    render_ms, query_ms = [], []
    for k in range(2 + args.runs):
        renderer.clear()
        renderer.render(0, args.spp, sync=True)
        r_ms = renderer.last_render_ms()
        renderer.radiance(rays, spp=args.spp, raw=True)
        q_ms = renderer.last_radiance_ms()
        if not (r_ms > 0.0 and q_ms > 0.0):
            raise RuntimeError(f"event times {r_ms}, {q_ms}")
        if k >= 2:
            render_ms.append(r_ms), query_ms.append(q_ms)
    variant = renderer.last_variant()
    r_med, q_med = statistics.median(render_ms), statistics.median(query_ms)
    base = {"res": args.res, "spp": args.spp, "triangles": int(scene.view().accel.triangle_count), "runs": args.runs}
    print(json.dumps({**base, "what": "lrhip_render", "variant": variant, "ms": round(r_med, 3), "msamples_per_s": round(samples / r_med * 1e-3, 1),
                      "min_ms": round(min(render_ms), 3), "max_ms": round(max(render_ms), 3)}), flush=True)
    print(json.dumps({**base, "what": "lrhip_trace_radiance", "ms": round(q_med, 3), "msamples_per_s": round(samples / q_med * 1e-3, 1),
                      "min_ms": round(min(query_ms), 3), "max_ms": round(max(query_ms), 3)}), flush=True)
    print(json.dumps({**base, "what": "ratio", "query_over_render": round(r_med / q_med, 4)}), flush=True)
    # the counting twins, one run each (the counters are summed since the upload: differences)
    c0 = renderer.counters()
    renderer.clear()
    renderer.render(0, args.spp, counters=True, sync=True)
    count_render_ms = renderer.last_render_ms()
    c1 = renderer.counters()
    renderer.radiance(rays, spp=args.spp, raw=True, counters=True)
    count_query_ms = renderer.last_radiance_ms()
    c2 = renderer.counters()
    renderer.radiance(rays, spp=args.spp, raw=True, counters=True)  # once more: what two counting runs of the same call differ by
    c3 = renderer.counters()
    diff = lambda a, b: {k: b[k] - a[k] for k in a if k != "probe"}
    print(json.dumps({**base, "what": "lrhip_render counters", **utilisation(diff(c0, c1))}), flush=True)
    print(json.dumps({**base, "what": "lrhip_trace_radiance counters", **utilisation(diff(c1, c2))}), flush=True)
    print(json.dumps({**base, "what": "lrhip_trace_radiance counters, again", **utilisation(diff(c2, c3))}), flush=True)
    print(json.dumps({**base, "what": "counting kernels, ms", "lrhip_render": round(count_render_ms, 3), "lrhip_trace_radiance": round(count_query_ms, 3)}),
          flush=True)
    renderer.close()


if __name__ == "__main__":
    main()
