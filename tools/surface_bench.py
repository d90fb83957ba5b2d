#!/usr/bin/env python3
"""Mpoints/s of lrhip_query_surface from lrhip_last_surface_ms -- HIP events around the kernel -- on the bench's C2 room: the hit
records of the pinhole camera's rays over a 1024 x 1024 grid with SUB x SUB positions per pixel (2^24 at the default), in device memory,
for the geometry-only and the full query, with and without the rays, next to lrhip_trace_rays' closest-hit rate for the same rays.
Device pointers, two warm-up calls, then the median of RUNS calls.  One JSON line per measurement.

    python tools/surface_bench.py [--runs 10] [--sub 4] [--triangles 600000]
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


def median_rate(call, last_ms, count, runs, warmup=2):
    rates = []
    for k in range(warmup + runs):
        call()
        ms = last_ms()
        if not ms > 0.0:
            raise RuntimeError(f"the kernel time of the last call is {ms}")
        if k >= warmup:
            rates.append(count / ms * 1e-3)
    return statistics.median(rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sub", type=int, default=4, help="positions per pixel and axis of the 1024 x 1024 grid: 4 gives 2^24 records per call")
    ap.add_argument("--triangles", type=int, default=600_000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("surface_bench: no GPU -- a rate is a measurement on the device, there is no fallback")
    device = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(prefix="surface_bench_") as out_dir:
        scene = Scene.load(generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(1024, 1024), spp=1, inline_meshes=True))
    renderer = MegaPathRenderer(0)
    renderer.upload(scene)
    rays = primary_rays(torch, device, 1024 * args.sub)
    hits = renderer.trace(rays)
    torch.cuda.synchronize()
    n = len(rays)
    common = {"count": n, "triangles": int(scene.view().accel.triangle_count), "hit_share": round(float(hits.hit.float().mean()), 4)}
    rate = median_rate(lambda: renderer.trace(rays), renderer.last_trace_ms, n, args.runs)
    print(json.dumps({"call": "trace", "mode": "closest", **common, "mrays_per_s": round(rate, 1)}), flush=True)
    for geometry_only in (True, False):
        for with_rays in (True, False):
            rate = median_rate(lambda: renderer.surface(hits, rays if with_rays else None, geometry_only=geometry_only), renderer.last_surface_ms,
                               n, args.runs)
            print(json.dumps({"call": "surface", "mode": "geometry_only" if geometry_only else "full", "rays": with_rays, **common,
                              "mpoints_per_s": round(rate, 1), "gb_per_s_of_records": round(rate * 1e-3 * (160 + (32 if with_rays else 0)), 1)}),
                  flush=True)
    renderer.close()


if __name__ == "__main__":
    main()
