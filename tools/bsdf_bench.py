#!/usr/bin/env python3
"""Mevaluations/s and Msamples/s of lrhip_query_bsdf from lrhip_last_bsdf_ms -- HIP events around the kernel -- on the bench's C2
room: the hit records of the pinhole camera's rays over a 1024 x 1024 grid with SUB x SUB positions per pixel (2^24 at the default), in device
memory, with the rays as viewing directions; wi uniform on the sphere, u uniform in [0, 1)^3.  Next to lrhip_trace_rays' closest-hit rate and
the full surface query's rate for the same records.  Device pointers, two warm-up calls, then the median of RUNS calls.  One JSON line per
measurement.

    python tools/bsdf_bench.py [--runs 10] [--sub 4] [--triangles 600000]
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
        sys.exit("bsdf_bench: no GPU -- a rate is a measurement on the device, there is no fallback")
    device = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(prefix="bsdf_bench_") as out_dir:
        scene = Scene.load(generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(1024, 1024), spp=1, inline_meshes=True))
    renderer = MegaPathRenderer(0)
    renderer.upload(scene)
    rays = primary_rays(torch, device, 1024 * args.sub)
    n = len(rays)
    g = torch.Generator(device=device).manual_seed(3)
    wi = torch.zeros((n, 4), dtype=torch.float32, device=device)
    wi[:, 0:3] = torch.randn((n, 3), generator=g, device=device)
    wi[:, 0:3] /= wi[:, 0:3].norm(dim=1, keepdim=True)
    u = torch.rand((n, 4), generator=g, device=device).clamp_(max=1.0 - 2.0 ** -24)
    hits = renderer.trace(rays)
    torch.cuda.synchronize()
    answered = renderer.bsdf_evaluate(hits, wi, rays)
    sampled = renderer.bsdf_sample(hits, u, rays)
    common = {"count": n, "triangles": int(scene.view().accel.triangle_count), "hit_share": round(float(hits.hit.float().mean()), 4),
              "valid_share": round(float(answered.valid.float().mean()), 4)}
    rate = median_rate(lambda: renderer.trace(rays), renderer.last_trace_ms, n, args.runs)
    print(json.dumps({"call": "trace", "mode": "closest", **common, "mrays_per_s": round(rate, 1)}), flush=True)
    rate = median_rate(lambda: renderer.surface(hits, rays), renderer.last_surface_ms, n, args.runs)
    print(json.dumps({"call": "surface", "mode": "full", **common, "mpoints_per_s": round(rate, 1)}), flush=True)
    rate = median_rate(lambda: renderer.bsdf_evaluate(hits, wi, rays), renderer.last_bsdf_ms, n, args.runs)
    print(json.dumps({"call": "bsdf", "mode": "evaluate", **common, "pdf_positive_share": round(float((answered.pdf > 0).float().mean()), 4),
                      "mevaluations_per_s": round(rate, 1)}), flush=True)
    rate = median_rate(lambda: renderer.bsdf_sample(hits, u, rays), renderer.last_bsdf_ms, n, args.runs)
    print(json.dumps({"call": "bsdf", "mode": "sample", **common, "pdf_positive_share": round(float((sampled.pdf > 0).float().mean()), 4),
                      "msamples_per_s": round(rate, 1)}), flush=True)
    renderer.close()


if __name__ == "__main__":
    main()
