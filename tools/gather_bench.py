#!/usr/bin/env python3
"""The rates of lightmap baking on the bench's C2 room, median of RUNS calls after two warm-up calls, one JSON line each:

  irradiance        Msamples/s of lrhip_gather_irradiance from lrhip_last_gather_ms -- HIP events around the kernel -- over 2^20 records in
                    device memory (the hit records of the room camera's rays over a 1024 x 1024 grid), SPP samples each in one call
  radiance route    what a caller had before: per sample index, SPP times, cosine-distributed rays about each record's normal built on the
                    HOST in numpy (32 bytes a ray), copied to the device and passed to radiance(); Msamples/s with the host's time (build +
                    copy + kernel, wall clock) and without it (the kernels' event time alone).  No next-event estimation at the texel,
                    and the mean is left to the caller
  lightmap_texels   Mtexels/s of lrhip_lightmap_texels for a 1024 x 1024 map of the room's first instance that has vertex UVs

    python tools/gather_bench.py [--runs 10] [--spp 16] [--triangles 600000]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from luisarender_amd import Scene  # noqa: E402
from luisarender_amd.render import DeviceError, MegaPathRenderer  # noqa: E402
from luisarender_amd.scenes import generate_room_scene  # noqa: E402
from raycast_bench import primary_rays  # noqa: E402
from surface_bench import median_rate  # noqa: E402


def cosine_rays(rng, p, n):
    """[N, 8] float32 rays from p + 1e-3 n, cosine-distributed about n: the host's share of the old route"""
    u = rng.random((len(p), 2), dtype=np.float32)
    r, phi = np.sqrt(u[:, 0]), np.float32(2 * np.pi) * u[:, 1]
    local = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(np.float32(0), 1 - u[:, 0]))], 1)
    a = np.where(np.abs(n[:, 0:1]) > 0.9, np.float32([0, 1, 0]), np.float32([1, 0, 0]))
    t = np.cross(n, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    rays = np.empty((len(p), 8), np.float32)
    rays[:, 0:3] = p + np.float32(1e-3) * n
    rays[:, 3] = 0
    rays[:, 4:7] = local[:, 0:1] * t + local[:, 1:2] * b + local[:, 2:3] * n
    rays[:, 7] = np.inf
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--triangles", type=int, default=600_000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gather_bench: no GPU -- a rate is a measurement on the device, there is no fallback")
    device = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(prefix="gather_bench_") as out_dir:
        scene = Scene.load(generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(1024, 1024), spp=1, inline_meshes=True))
    renderer = MegaPathRenderer(0)
    renderer.upload(scene)
    rays = primary_rays(torch, device, 1024)
    n = len(rays)
    hits = renderer.trace(rays)
    torch.cuda.synchronize()
    view = scene.view()
    common = {"records": n, "spp": args.spp, "triangles": int(view.accel.triangle_count), "depth": int(view.integrator.max_depth),
              "hit_share": round(float(hits.hit.float().mean()), 4)}
    raw = renderer.irradiance(hits, spp=args.spp, raw=True)
    samples = float(raw[:, 3].sum())
    rate = median_rate(lambda: renderer.irradiance(hits, spp=args.spp, raw=True), renderer.last_gather_ms, samples, args.runs)
    print(json.dumps({"call": "irradiance", **common, "samples": int(samples), "ms": round(samples / rate * 1e-3, 3), "msamples_per_s": round(rate, 1)}), flush=True)
    # ---- the old route: cosine rays from the host, one radiance() call per sample index
    points = renderer.surface(hits, geometry_only=True)
    valid = points.valid.cpu().numpy()
    p, ng = points.p.cpu().numpy()[valid], points.ng.cpu().numpy()[valid]
    rng = np.random.default_rng(7)
    walls, kernels = [], []
    for k in range(2 + args.runs):
        t0 = time.perf_counter()
        kernel_ms = 0.0
        total = torch.zeros((len(p), 4), device=device)
        for s in range(args.spp):
            r = torch.from_numpy(cosine_rays(rng, p, ng)).to(device)
            total += renderer.radiance(r, spp=1, spp_begin=s, raw=True)
            kernel_ms += renderer.last_radiance_ms()
        torch.cuda.synchronize()
        if k >= 2:
            walls.append(time.perf_counter() - t0), kernels.append(kernel_ms)
    count = float(len(p)) * args.spp
    print(json.dumps({"call": "radiance over host-built cosine rays", **common, "samples": int(count),
                      "ray_bytes_built": int(count) * 32, "ms_with_host": round(statistics.median(walls) * 1e3, 1),
                      "msamples_per_s_with_host": round(count / statistics.median(walls) * 1e-6, 1),
                      "ms_kernels": round(statistics.median(kernels), 3),
                      "msamples_per_s_kernels": round(count / statistics.median(kernels) * 1e-3, 1)}), flush=True)
    # ---- the rasteriser
    for instance in range(int(view.instance_count)):
        try:
            texels = renderer.lightmap_texels(instance, 1024, 1024, on_device=True)
        except DeviceError:
            continue  # no vertex UVs
        rate = median_rate(lambda: renderer.lightmap_texels(instance, 1024, 1024, on_device=True), renderer.last_lightmap_ms, 1 << 20, args.runs)
        print(json.dumps({"call": "lightmap_texels", "instance": instance, "mesh_triangles": len(scene.mesh_triangles(scene.instance_mesh(instance))),
                          "texels": 1 << 20, "covered_share": round(float(texels.covered.float().mean()), 4),
                          "ms": round((1 << 20) / rate * 1e-3, 4), "mtexels_per_s": round(rate, 1)}), flush=True)
        break
    renderer.close()


if __name__ == "__main__":
    main()
