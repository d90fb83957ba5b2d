#!/usr/bin/env python3
"""Msamples/s and Mevaluations/s of lrhip_query_light from lrhip_last_light_ms -- HIP events around the kernel -- on the bench's C2
room: the hit records of the pinhole camera's rays over a 1024 x 1024 grid with SUB x SUB positions per pixel (2^24 at the default), in device
memory; u uniform in [0, 1)^3.  Sample mode from the hit records and from the hits' bare positions; evaluate mode for the sampled directions
traced to their closest hits (what a BSDF-sampled ray would have found).  Next to lrhip_trace_rays' closest-hit rate for the camera rays and
its any-hit rate for the shadow rays.  Device pointers, two warm-up calls, then the median of RUNS calls.  One JSON line per measurement.

    python tools/light_bench.py [--runs 10] [--sub 4] [--triangles 600000]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from luisarender_amd import Scene  # noqa: E402
from luisarender_amd.render import MegaPathRenderer  # noqa: E402
from luisarender_amd.scenes import generate_room_scene  # noqa: E402
from raycast_bench import primary_rays  # noqa: E402
from surface_bench import median_rate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sub", type=int, default=4, help="positions per pixel and axis of the 1024 x 1024 grid: 4 gives 2^24 records per call")
    ap.add_argument("--triangles", type=int, default=600_000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("light_bench: no GPU -- a rate is a measurement on the device, there is no fallback")
    device = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(prefix="light_bench_") as out_dir:
        scene = Scene.load(generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(1024, 1024), spp=1, inline_meshes=True))
    renderer = MegaPathRenderer(0)
    renderer.upload(scene)
    rays = primary_rays(torch, device, 1024 * args.sub)
    n = len(rays)
    g = torch.Generator(device=device).manual_seed(3)
    u = torch.rand((n, 4), generator=g, device=device).clamp_(max=1.0 - 2.0 ** -24)
    hits = renderer.trace(rays)
    torch.cuda.synchronize()
    sampled = renderer.light_sample(hits, u)
    points = renderer.surface(hits, geometry_only=True).buffer[:, 0:4].contiguous()  # (p, area): the fourth column is ignored
    torch.cuda.synchronize()
    towards = sampled.rays.clone()
    towards[:, 7] = float("inf")
    found = renderer.trace(towards)
    evaluated = renderer.light_evaluate(found, towards)
    view = scene.view()
    common = {"count": n, "triangles": int(view.accel.triangle_count), "lights": int(view.integrator.light_count),
              "env_prob": round(float(view.integrator.env_prob), 3), "hit_share": round(float(hits.hit.float().mean()), 4),
              "valid_share": round(float(sampled.valid.float().mean()), 4)}
    rate = median_rate(lambda: renderer.trace(rays), renderer.last_trace_ms, n, args.runs)
    print(json.dumps({"call": "trace", "mode": "closest", **common, "mrays_per_s": round(rate, 1)}), flush=True)
    rate = median_rate(lambda: renderer.trace(sampled.rays, any_hit=True), renderer.last_trace_ms, n, args.runs)
    print(json.dumps({"call": "trace", "mode": "any, the shadow rays", **common, "mrays_per_s": round(rate, 1)}), flush=True)
    share = {"pdf_positive_share": round(float((sampled.pdf > 0).float().mean()), 4),
             "environment_share": round(float((sampled.kind == 1).float().mean()), 4)}
    rate = median_rate(lambda: renderer.light_sample(hits, u), renderer.last_light_ms, n, args.runs)
    print(json.dumps({"call": "light", "mode": "sample", **common, **share, "msamples_per_s": round(rate, 1)}), flush=True)
    rate = median_rate(lambda: renderer.light_sample(points=points, u=u), renderer.last_light_ms, n, args.runs)
    print(json.dumps({"call": "light", "mode": "sample from points", **common, "msamples_per_s": round(rate, 1)}), flush=True)
    share = {"area_share": round(float((evaluated.kind == 0).float().mean()), 4), "environment_share": round(float((evaluated.kind == 1).float().mean()), 4)}
    rate = median_rate(lambda: renderer.light_evaluate(found, towards), renderer.last_light_ms, n, args.runs)
    print(json.dumps({"call": "light", "mode": "evaluate", **common, **share, "mevaluations_per_s": round(rate, 1)}), flush=True)
    renderer.close()


if __name__ == "__main__":
    main()
