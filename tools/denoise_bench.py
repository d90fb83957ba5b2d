#!/usr/bin/env python3
"""HIP-event time of lrhip_aov_denoise on the Cornell box under the AOV integrator, beside the time of one 8-spp AOV frame
of the same size measured in the same run.  A warm-up, then the median of RUNS calls; the time per pass is the difference between
K and K - 1 iterations.  One JSON line per size.

    python tools/denoise_bench.py [--sizes 1024x1024,3840x2160] [--iterations 5] [--runs 10] [--lib name under lib/variants/]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from luisarender_amd import Scene  # noqa: E402
from luisarender_amd.render import MegaPathRenderer  # noqa: E402
from luisarender_amd.scenes import cornell_box  # noqa: E402

FRAME_SPP = 8


def median_ms(call, read, runs, warmup=2):
    times = []
    for k in range(warmup + runs):
        call()
        if k >= warmup:
            times.append(read())
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024x1024,3840x2160")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    lib = args.lib and os.path.join(ROOT, "luisarender_amd", "lib", "variants", f"liblrhip_{args.lib}.so")
    renderer = MegaPathRenderer(0, lib_path=lib)
    for size in args.sizes.split(","):
        width, height = (int(v) for v in size.split("x"))
        text = cornell_box(resolution=(width, height), spp=FRAME_SPP, depth=5, rr_depth=100)
        text = text.replace("integrator : MegaPath {", f"integrator : AOV {{ noisy_count {{ {FRAME_SPP} }} ")
        renderer.upload(Scene.from_string(text))

        def frame():
            renderer.clear()
            renderer.render(0, FRAME_SPP, sync=True)

        frame_ms = median_ms(frame, renderer.last_render_ms, max(args.runs // 2, 3), warmup=1)
        by_iterations = [0.0] + [median_ms(lambda: renderer.denoise_aov("sample", iterations=k), renderer.last_denoise_ms, args.runs)
                                 for k in range(1, args.iterations + 1)]
        total = by_iterations[-1]
        print(json.dumps({"size": size, "iterations": args.iterations, "lib": args.lib or "base", "denoise_ms": round(total, 4),
                          "pass_ms": [round(b - a, 4) for a, b in zip(by_iterations[1:-1], by_iterations[2:])],
                          "prepare_first_pass_finish_ms": round(by_iterations[1], 4), f"aov_frame_{FRAME_SPP}spp_ms": round(frame_ms, 4),
                          "denoise_over_frame": round(total / frame_ms, 4)}), flush=True)
    renderer.close()


if __name__ == "__main__":
    main()
