#!/usr/bin/env python3
"""Gstates/s, Gdraws/s, Grays/s and Gsplats/s of lrhip_query_sampler, lrhip_query_camera and lrhip_film_splat from
lrhip_last_camera_ms -- HIP events around the kernel -- on the bench's C2 room at 1024 x 1024: 2^24 records in device memory (SUB x SUB per
pixel at the default; record k is stream / pixel k mod W H, so a splat call names every pixel SUB x SUB times).  The states of sample index 0;
the per-vertex pattern "1212" drawn from them (four draws, six floats per record); the camera rays for the numbers of "p2"; the splat of uniform
values.  Device pointers, two warm-up calls, then the median of RUNS calls.  One JSON line per measurement, with the bytes the kernel moves per
record.

    python tools/camera_bench.py [--runs 10] [--sub 4] [--triangles 600000]
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
from surface_bench import median_rate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sub", type=int, default=4, help="records per pixel and axis of the 1024 x 1024 frame: 4 gives 2^24 records per call")
    ap.add_argument("--triangles", type=int, default=600_000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("camera_bench: no GPU -- a rate is a measurement on the device, there is no fallback")
    device = torch.device("cuda:0")
    with tempfile.TemporaryDirectory(prefix="camera_bench_") as out_dir:
        scene = Scene.load(generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(1024, 1024), spp=1, inline_meshes=True))
    view = scene.view()
    renderer = MegaPathRenderer(0)
    renderer.upload(scene)
    pixels = renderer.width * renderer.height
    n = pixels * args.sub * args.sub
    ids = (torch.arange(n, dtype=torch.int64, device=device) % pixels).to(torch.int32)
    g = torch.Generator(device=device).manual_seed(3)
    values = torch.rand((n, 4), generator=g, device=device) * 4.0
    state = renderer.sampler_start(count=n, sample=0, on_device=True)
    u = renderer.sampler_draw(state.clone(), "p2")
    torch.cuda.synchronize()
    common = {"count": n, "sampler_kind": int(view.sampler.kind), "camera_kind": int(view.camera.kind), "filter_radius": float(view.filter.radius)}
    rate = median_rate(lambda: renderer.sampler_start(count=n, sample=0, on_device=True), renderer.last_camera_ms, n, args.runs)
    print(json.dumps({"call": "sampler", "mode": "start", **common, "bytes_per_record": 16, "gstates_per_s": round(rate * 1e-3, 2)}), flush=True)
    work = state.clone()
    rate = median_rate(lambda: renderer.sampler_draw(work, "1212"), renderer.last_camera_ms, n, args.runs)
    print(json.dumps({"call": "sampler", "mode": "draw 1212", **common, "bytes_per_record": 16 + 16 + 24, "grecords_per_s": round(rate * 1e-3, 2),
                      "gdraws_per_s": round(4 * rate * 1e-3, 2)}), flush=True)
    rate = median_rate(lambda: renderer.camera_rays(u, ids), renderer.last_camera_ms, n, args.runs)
    print(json.dumps({"call": "camera", **common, "bytes_per_record": 4 + 16 + 32 + 16, "grays_per_s": round(rate * 1e-3, 2)}), flush=True)
    rate = median_rate(lambda: renderer.film_splat(values, ids), renderer.last_camera_ms, n, args.runs)
    print(json.dumps({"call": "splat", "mode": f"{args.sub * args.sub} records per pixel", **common, "bytes_per_record": 4 + 16 + 32,
                      "gsplats_per_s": round(rate * 1e-3, 2)}), flush=True)
    renderer.clear()
    rate = median_rate(lambda: renderer.film_splat(values[:pixels]), renderer.last_camera_ms, pixels, args.runs)
    print(json.dumps({"call": "splat", "mode": "one record per pixel", **{**common, "count": pixels}, "bytes_per_record": 16 + 32,
                      "gsplats_per_s": round(rate * 1e-3, 2)}), flush=True)
    renderer.close()


if __name__ == "__main__":
    main()
