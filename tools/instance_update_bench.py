#!/usr/bin/env python3
"""What moving an instance costs on the bench's C2 room, in ms per move: lrhip_set_instance_transforms with one matrix through
host pointers (the call synchronises), the same with device pointers (a host clock around call + synchronise, and the HIP-event time of its
kernels, lrhip_last_instance_update_ms), the full matrix table both ways, and the route the library had before -- Scene.set_time on a copy
of the scene whose first fixture carries a Lerp transform, then upload(keep_film=True), i.e. lrhost_scene_set_time + lrhip_update_scene: the
host re-bakes and refits, rebuilds every dependent table and copies each one whole.  Every route makes the same move per round (the fixture
slides along x; round k puts it at time k / rounds), two warm-up rounds, then RUNS rounds that alternate the routes.  The last round's device
tables of the two contexts are compared byte for byte.  One JSON line per result, with the hash of the sources that were timed.

    python tools/instance_update_bench.py [--runs 9] [--triangles 600000]
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from luisarender_amd import Scene, _ffi  # noqa: E402
from luisarender_amd.render import MegaPathRenderer  # noqa: E402
from luisarender_amd.scenes import generate_room_scene  # noqa: E402

SOURCES = ("luisarender_amd/csrc/hip/instance_update_kernels.h", "luisarender_amd/csrc/hip/lrhip_instance_update.hip",
           "luisarender_amd/csrc/hip/lrhip_upload.hip", "luisarender_amd/csrc/hip/lrhip_tables.hip", "luisarender_amd/csrc/host/accel.cpp", "Makefile")


def source_hash() -> str:
    h = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(ROOT, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:12]


def animate_first_fixture(text: str) -> str:
    """the scene with obj0 on a Lerp between its own transform and the same one 0.5 further along x"""
    m = re.search(r"(Shape obj0 : Instance \{.*?transform : )(SRT \{ (.*?)translate \{ ([-0-9.]+), ([-0-9.]+), ([-0-9.]+) \} \})", text)
    if m is None:
        raise RuntimeError("instance_update_bench: the room's first fixture was not found")
    x = float(m.group(4))
    there = f"SRT {{ {m.group(3)}translate {{ {x + 0.5:.4f}, {m.group(5)}, {m.group(6)} }} }}"
    return text[:m.start(2)] + f"Lerp {{ time_points {{ 0, 1 }} transforms {{ {m.group(2)}, {there} }} }}" + text[m.end(2):]


def matrices_of(scene: Scene) -> np.ndarray:
    v = scene.view()
    return np.array([v.instances[i].object_to_world[:] for i in range(v.instance_count)], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--triangles", type=int, default=600_000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("instance_update_bench: no GPU -- a time is a measurement on the device, there is no fallback")
    with tempfile.TemporaryDirectory(prefix="instance_update_bench_") as out_dir:
        path = generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(64, 64), spp=1, inline_meshes=True)
        with open(path) as f:
            text = animate_first_fixture(f.read())
        animated = Scene.from_string(text, virtual_path=path)   # the host route's scene ...
        matrix_source = Scene.from_string(text, virtual_path=path, build_accel=False)  # ... and where the other routes' matrices come from
    still = matrices_of(animated)
    matrix_source.set_time(0.5)
    moved = [i for i in range(len(still)) if not np.array_equal(still[i], matrices_of(matrix_source)[i])]
    if len(moved) != 1:
        raise RuntimeError(f"instance_update_bench: {len(moved)} instances moved, expected one")
    ids = np.array(moved, np.uint32)
    device_route, host_route = MegaPathRenderer(0), MegaPathRenderer(0)
    device_route.upload(animated)
    host_route.upload(animated)
    view = animated.view()
    base = {"triangles": int(view.accel.triangle_count), "nodes": int(view.accel.node_count), "instances": int(view.instance_count),
            "runs": args.runs, "sources": source_hash()}
    table_bytes = sum(int(device_route._lib.lrhip_scene_table_bytes(device_route._ctx, k)) for k in range(4))
    times = {name: [] for name in ("one_host_pointers", "one_device_pointers", "one_device_kernels", "all_host_pointers", "all_device_pointers",
                                   "all_device_kernels", "host_route", "host_route_set_time", "host_route_update_scene")}
    rounds = 2 + args.runs
    for k in range(rounds):
        t = (k + 1) / rounds
        matrix_source.set_time(t)
        full = matrices_of(matrix_source)
        one = np.ascontiguousarray(full[moved])
        device_full, device_one = torch.from_numpy(full).to("cuda:0"), torch.from_numpy(one).to("cuda:0")
        device_ids = torch.from_numpy(ids.astype(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        got = {}

        def timed(name, call, sync=None):
            begin = time.perf_counter()
            call()
            if sync is not None:
                sync()
            got[name] = (time.perf_counter() - begin) * 1e3

        timed("one_host_pointers", lambda: device_route.set_instance_transforms(one, ids))
        timed("one_device_pointers", lambda: device_route.set_instance_transforms(device_one, device_ids, sync=False), device_route.synchronize)
        got["one_device_kernels"] = device_route.last_instance_update_ms()
        timed("all_host_pointers", lambda: device_route.set_instance_transforms(full))
        timed("all_device_pointers", lambda: device_route.set_instance_transforms(device_full, sync=False), device_route.synchronize)
        got["all_device_kernels"] = device_route.last_instance_update_ms()
        timed("host_route_set_time", lambda: animated.set_time(t))
        timed("host_route_update_scene", lambda: host_route.upload(animated, keep_film=True))
        got["host_route"] = got["host_route_set_time"] + got["host_route_update_scene"]
        if k >= 2:
            for name, ms in got.items():
                times[name].append(ms)
    same = all(np.array_equal(device_route.scene_table(k), host_route.scene_table(k)) for k in range(4))
    for name, ms in times.items():
        print(json.dumps({**base, "what": name, "ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}), flush=True)
    print(json.dumps({**base, "what": "summary", "table_bytes": table_bytes, "tables_equal_after_last_round": bool(same),
                      "host_route_over_one_device_pointers": round(statistics.median(times["host_route"]) / statistics.median(times["one_device_pointers"]), 2)}),
          flush=True)
    device_route.close()
    host_route.close()
    if not same:
        sys.exit("instance_update_bench: the device tables of the two routes differ")


if __name__ == "__main__":
    main()
