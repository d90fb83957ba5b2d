#!/usr/bin/env python3
"""Mrays/s of lrhip_trace_rays from lrhip_last_trace_ms -- HIP events around the kernel -- on the bench's C2 room, closest hit
and any hit, for three ray sets in device memory:
    primary  the pinhole camera's rays over a 1024 x 1024 grid with SUB x SUB positions per pixel (row-major over the fine grid)
    random   origins uniform in the scene's bounds, directions uniform on the sphere: incoherent
    ao       a cosine-weighted hemisphere direction from every primary hit, length AO_RADIUS: the ambient-occlusion pattern
Device pointers, two warm-up calls, then the median of RUNS calls of at least 2^24 rays.  Several builds of the library (--libs: names under
lib/variants/, "base" = the shipped one) are measured ALTERNATING, --repeats times each, in one process; a summary line per build, ray set and
mode gives the mean of the medians and their spread.  One JSON line per measurement.

    python tools/raycast_bench.py [--libs base,drain] [--repeats 3] [--runs 10] [--sub 4] [--triangles 600000] [--sets primary,random,ao]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from luisarender_amd import Scene  # noqa: E402
from luisarender_amd.render import MegaPathRenderer  # noqa: E402
from luisarender_amd.scenes import generate_room_scene  # noqa: E402

AO_RADIUS = 1.0
T_MIN = 1e-4
# the room's camera (scenes/bathroom.py): a pinhole at `position` looking along `front`, vertical field of view 55 degrees
CAMERA = {"position": (2.0, 1.6, 3.85), "front": (0.0, -0.15, -1.0), "up": (0.0, 1.0, 0.0), "fov": 55.0}


def primary_rays(torch, device, grid):
    """the pinhole rays through the centres of a grid x grid raster"""
    f = torch.tensor(CAMERA["front"], dtype=torch.float64)
    f = f / f.norm()
    r = torch.linalg.cross(f, torch.tensor(CAMERA["up"], dtype=torch.float64))
    r = r / r.norm()
    u = torch.linalg.cross(r, f)
    tan = float(np.tan(np.radians(CAMERA["fov"]) / 2.0))
    c = ((torch.arange(grid, dtype=torch.float64) + 0.5) / grid * 2.0 - 1.0) * tan
    d = f[None, None, :] + c[None, :, None] * r[None, None, :] - c[:, None, None] * u[None, None, :]
    d = (d / d.norm(dim=2, keepdim=True)).reshape(-1, 3)
    rays = torch.empty((grid * grid, 8), dtype=torch.float32)
    rays[:, 0:3] = torch.tensor(CAMERA["position"], dtype=torch.float32)
    rays[:, 3], rays[:, 4:7], rays[:, 7] = T_MIN, d.float(), float("inf")
    return rays.to(device)


def random_rays(torch, device, n, lo, hi, seed=1):
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    rays = torch.empty((n, 8), dtype=torch.float32)
    rays[:, 0:3] = lo + (hi - lo) * torch.rand((n, 3), generator=g)
    d = torch.randn((n, 3), generator=g)
    rays[:, 3], rays[:, 4:7], rays[:, 7] = T_MIN, d / d.norm(dim=1, keepdim=True), float("inf")
    return rays.to(device)


def ao_rays(torch, primary, hits, triangles, seed=2):
    """one cosine-weighted direction about the geometric normal (turned towards the viewer) from every primary hit"""
    hit = hits.hit
    rays, t, tri = primary[hit], hits.t[hit], hits.tri[hit].long()
    e1, e2 = triangles["e1"][tri], triangles["e2"][tri]
    n = torch.linalg.cross(e1, e2)
    n = n / n.norm(dim=1, keepdim=True)
    n = torch.where((n * rays[:, 4:7]).sum(dim=1, keepdim=True) > 0, -n, n)
    p = rays[:, 0:3] + t[:, None] * rays[:, 4:7]
    g = torch.Generator(device=primary.device).manual_seed(seed)
    xi = torch.rand((len(p), 2), generator=g, device=primary.device)
    radius, phi = xi[:, 0].sqrt(), 2.0 * np.pi * xi[:, 1]
    helper = torch.where(n[:, 0:1].abs() < 0.9, torch.tensor([1.0, 0.0, 0.0], device=p.device), torch.tensor([0.0, 1.0, 0.0], device=p.device))
    s = torch.linalg.cross(n, helper.expand_as(n))
    s = s / s.norm(dim=1, keepdim=True)
    b = torch.linalg.cross(n, s)
    d = radius[:, None] * (phi.cos()[:, None] * s + phi.sin()[:, None] * b) + (1.0 - xi[:, 0]).clamp_min(0.0).sqrt()[:, None] * n
    out = torch.empty((len(p), 8), dtype=torch.float32, device=p.device)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = p + 1e-3 * n, T_MIN, d, AO_RADIUS
    return out.contiguous()


def median_mrays(renderer, rays, any_hit, runs, warmup=2):
    rates = []
    for k in range(warmup + runs):
        renderer.trace(rays, any_hit=any_hit)
        ms = renderer.last_trace_ms()
        if not ms > 0.0:
            raise RuntimeError(f"lrhip_last_trace_ms returned {ms}")
        if k >= warmup:
            rates.append(len(rays) / ms * 1e-3)
    return statistics.median(rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="base")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sub", type=int, default=4, help="positions per pixel and axis of the 1024 x 1024 grid: 4 gives 2^24 rays per call")
    ap.add_argument("--triangles", type=int, default=600_000)
    ap.add_argument("--sets", default="primary,random,ao")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("raycast_bench: no GPU -- a rate is a measurement on the device, there is no fallback")
    device = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(prefix="raycast_bench_") as out_dir:
        scene = Scene.load(generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(1024, 1024), spp=1, inline_meshes=True))
    accel = scene.view().accel
    lo, hi = list(accel.world_min), list(accel.world_max)
    names = args.libs.split(",")
    renderers = {}
    for name in names:
        path = None if name == "base" else os.path.join(ROOT, "luisarender_amd", "lib", "variants", f"liblrhip_{name}.so")
        renderers[name] = MegaPathRenderer(0, lib_path=path)
        renderers[name].upload(scene)
    first = renderers[names[0]]
    sets = {}
    wanted = args.sets.split(",")
    primary = primary_rays(torch, device, 1024 * args.sub)
    if "primary" in wanted:
        sets["primary"] = primary
    if "random" in wanted:
        sets["random"] = random_rays(torch, device, len(primary), lo, hi)
    if "ao" in wanted:
        raw = np.ctypeslib.as_array(accel.triangles, shape=(accel.triangle_count,))
        words = torch.from_numpy(np.frombuffer(raw.tobytes(), dtype=np.float32).reshape(-1, 12).copy()).to(device)
        sets["ao"] = ao_rays(torch, primary, first.trace(primary), {"e1": words[:, 4:7], "e2": words[:, 8:11]})
    torch.cuda.synchronize()
    results = {}
    for repeat in range(args.repeats):
        for name in names:
            for set_name, rays in sets.items():
                for mode in ("closest", "any"):
                    rate = median_mrays(renderers[name], rays, mode == "any", args.runs)
                    results.setdefault((name, set_name, mode), []).append(rate)
                    print(json.dumps({"repeat": repeat, "lib": name, "rays": set_name, "mode": mode, "count": len(rays),
                                      "triangles": int(accel.triangle_count), "mrays_per_s": round(rate, 1)}), flush=True)
    for (name, set_name, mode), rates in results.items():
        print(json.dumps({"summary": True, "lib": name, "rays": set_name, "mode": mode, "mean_mrays_per_s": round(statistics.mean(rates), 1),
                          "min": round(min(rates), 1), "max": round(max(rates), 1), "repeats": len(rates)}), flush=True)
    for r in renderers.values():
        r.close()


if __name__ == "__main__":
    main()
