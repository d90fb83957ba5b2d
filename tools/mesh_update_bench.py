#!/usr/bin/env python3
"""What deforming a mesh costs on the bench's C2 room, in ms per deformation of the mesh of the room's first fixture:
lrhip_set_mesh_vertices through host pointers (the call synchronises) and through device pointers (a host clock around call + synchronise,
and the HIP-event time of its kernels, lrhip_last_mesh_update_ms), each with kept and with recomputed normals, and the host route --
Scene.set_mesh_vertices, then upload(keep_film=True), i.e. lrhost_scene_set_mesh_vertices + lrhip_update_scene: the host re-bakes and
refits, rebuilds every dependent table and copies each one whole.  Every route makes the same deformation per round (round k scales the
mesh by 1 + 0.1 sin(3 y + k)), two warm-up rounds, then RUNS rounds that alternate the routes; every round ends with recomputed normals on
both contexts, and the last round's device tables of the two, the vertex table included, are compared byte for byte.  One JSON line per
result, with the hash of the sources that were timed.

    python tools/mesh_update_bench.py [--runs 9] [--triangles 600000]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from instance_update_bench import animate_first_fixture, matrices_of  # noqa: E402
from luisarender_amd import Scene, _ffi  # noqa: E402
from luisarender_amd.render import MegaPathRenderer  # noqa: E402
from luisarender_amd.scenes import generate_room_scene  # noqa: E402

SOURCES = ("luisarender_amd/csrc/hip/mesh_update_kernels.h", "luisarender_amd/csrc/hip/lrhip_mesh_update.hip",
           "luisarender_amd/csrc/hip/instance_update_kernels.h", "luisarender_amd/csrc/hip/lrhip_instance_update.hip",
           "luisarender_amd/csrc/hip/lrhip_upload.hip", "luisarender_amd/csrc/hip/lrhip_tables.hip", "luisarender_amd/csrc/host/accel.cpp",
           "luisarender_amd/csrc/host/scene.cpp", "Makefile")
TABLES = (_ffi.TABLE_NODES, _ffi.TABLE_BVH_TRIANGLES, _ffi.TABLE_INSTANCES, _ffi.TABLE_SHADE_TRIANGLES, _ffi.TABLE_VERTICES)


def source_hash() -> str:
    h = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(ROOT, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--triangles", type=int, default=600_000)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mesh_update_bench: no GPU -- a time is a measurement on the device, there is no fallback")
    with tempfile.TemporaryDirectory(prefix="mesh_update_bench_") as out_dir:
        path = generate_room_scene(out_dir, target_triangles=args.triangles, resolution=(64, 64), spp=1, inline_meshes=True)
        with open(path) as f:
            text = f.read()
        scene = Scene.from_string(text, virtual_path=path)
        # the first fixture is the instance that moves when it alone is put on a Lerp transform
        probe = Scene.from_string(animate_first_fixture(text), virtual_path=path, build_accel=False)
    still = matrices_of(probe)
    probe.set_time(0.5)
    moved = [i for i in range(len(still)) if not np.array_equal(still[i], matrices_of(probe)[i])]
    probe.close()
    if len(moved) != 1:
        raise RuntimeError(f"mesh_update_bench: {len(moved)} instances moved, expected one")
    mesh = scene.instance_mesh(moved[0])
    rest, _ = scene.mesh_vertices(mesh)
    view = scene.view()
    sharing = sum(1 for i in range(view.instance_count) if scene.instance_mesh(i) == mesh)
    device_route, host_route = MegaPathRenderer(0), MegaPathRenderer(0)
    device_route.upload(scene)
    host_route.upload(scene)
    base = {"triangles": int(view.accel.triangle_count), "nodes": int(view.accel.node_count), "instances": int(view.instance_count),
            "mesh": mesh, "mesh_vertices": int(view.meshes[mesh].vertex_count), "mesh_triangles": int(view.meshes[mesh].triangle_count),
            "instances_of_mesh": sharing, "runs": args.runs, "sources": source_hash()}
    table_bytes = sum(int(device_route._lib.lrhip_scene_table_bytes(device_route._ctx, k)) for k in TABLES)
    names = ("host_pointers_kept", "device_pointers_kept", "device_kernels_kept", "host_pointers_recomputed", "device_pointers_recomputed",
             "device_kernels_recomputed", "host_route_kept", "host_route_kept_set_mesh_vertices", "host_route_kept_update_scene",
             "host_route_recomputed", "host_route_recomputed_set_mesh_vertices", "host_route_recomputed_update_scene")
    times = {name: [] for name in names}
    for k in range(2 + args.runs):
        positions = np.ascontiguousarray((rest.astype(np.float64) * (1.0 + 0.1 * np.sin(3.0 * rest[:, 1:2] + k))).astype(np.float32))
        device_positions = torch.from_numpy(positions).to("cuda:0")
        torch.cuda.synchronize()
        got = {}

        def timed(name, call, sync=None):
            begin = time.perf_counter()
            call()
            if sync is not None:
                sync()
            got[name] = (time.perf_counter() - begin) * 1e3

        for what, recompute in (("kept", False), ("recomputed", True)):
            timed(f"host_pointers_{what}", lambda: device_route.set_mesh_vertices(mesh, positions, recompute_normals=recompute))
            timed(f"device_pointers_{what}", lambda: device_route.set_mesh_vertices(mesh, device_positions, recompute_normals=recompute, sync=False),
                  device_route.synchronize)
            got[f"device_kernels_{what}"] = device_route.last_mesh_update_ms()
            timed(f"host_route_{what}_set_mesh_vertices", lambda: scene.set_mesh_vertices(mesh, positions, recompute_normals=recompute))
            timed(f"host_route_{what}_update_scene", lambda: host_route.upload(scene, keep_film=True))
            got[f"host_route_{what}"] = got[f"host_route_{what}_set_mesh_vertices"] + got[f"host_route_{what}_update_scene"]
        if k >= 2:
            for name, ms in got.items():
                times[name].append(ms)
    same = all(np.array_equal(device_route.scene_table(k), host_route.scene_table(k)) for k in TABLES)
    for name, ms in times.items():
        print(json.dumps({**base, "what": name, "ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}), flush=True)
    print(json.dumps({**base, "what": "summary", "table_bytes": table_bytes, "tables_equal_after_last_round": bool(same),
                      "host_route_over_device_pointers_kept": round(statistics.median(times["host_route_kept"]) / statistics.median(times["device_pointers_kept"]), 2)}),
          flush=True)
    device_route.close()
    host_route.close()
    if not same:
        sys.exit("mesh_update_bench: the device tables of the two routes differ")


if __name__ == "__main__":
    main()
