#!/usr/bin/env python3
"""Mtexels/s of lrhip_lightmap_texels from lrhip_last_lightmap_ms -- HIP events around the owner pass and the record pass -- for
a SIZE x SIZE lightmap (1024: 2^20 texel records) written to device memory, over the two extremes of a chart: an inline quad of two
triangles that fill the map (every wave of the owner pass is a slice of a triangle's texels) and an icosphere of 20 x 4^LEVEL triangles
(a few texels per triangle), each with centre coverage alone and with the conservative mode.  Device pointers, two warm-up calls, then the
median of RUNS calls.  One JSON line per measurement.

    python tools/lightmap_bench.py [--runs 10] [--size 1024] [--level 6]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from luisarender_amd import Scene  # noqa: E402
from luisarender_amd.render import MegaPathRenderer  # noqa: E402
from surface_bench import median_rate  # noqa: E402

SCENE = """
Shape quad : InlineMesh { positions { 0,0,0, 1,0,0, 1,1,0, 0,1,0 } indices { 0,1,2, 0,2,3 } uvs { 0.031,0.043, 0.961,0.043, 0.961,0.933, 0.031,0.933 } surface : Matte { } }
Shape ball : Sphere { subdivision { LEVEL } surface : Matte { } transform : SRT { translate { 0, 0, -3 } } }
Shape lamp : InlineMesh { positions { 0,0,4, 1,0,4, 0,1,4 } indices { 0,2,1 } light : Diffuse { emission : Constant { v { 5 } } } }
Camera cam : Pinhole { spp { 1 } film : Color { resolution { 8, 8 } } position { 0.5, 0.5, 3 } look_at { 0.5, 0.5, 0 } fov { 40 } }
render { cameras { @cam } shapes { @quad, @ball, @lamp } integrator : MegaPath { depth { 2 } sampler : Independent { } } }
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("lightmap_bench: no GPU -- a rate is a measurement on the device, there is no fallback")
    scene = Scene.from_string(SCENE.replace("LEVEL", str(args.level)))
    renderer = MegaPathRenderer(0)
    renderer.upload(scene)
    n = args.size * args.size
    for instance, name in ((0, "quad"), (1, "ball")):
        triangles = len(scene.mesh_triangles(scene.instance_mesh(instance)))
        for conservative in (False, True):
            texels = renderer.lightmap_texels(instance, args.size, args.size, conservative=conservative, on_device=True)
            rate = median_rate(lambda: renderer.lightmap_texels(instance, args.size, args.size, conservative=conservative, on_device=True),
                               renderer.last_lightmap_ms, n, args.runs)
            print(json.dumps({"call": "lightmap_texels", "chart": name, "triangles": triangles, "texels": n, "conservative": conservative,
                              "covered_share": round(float(texels.covered.float().mean()), 4),
                              "touched_share": round(float(texels.touched.float().mean()), 4),
                              "ms": round(n / rate * 1e-3, 4), "mtexels_per_s": round(rate, 1)}), flush=True)
    renderer.close()


if __name__ == "__main__":
    main()
