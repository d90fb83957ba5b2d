"""tools/ that the design decisions lean on must keep building: tools/bvh_sim.cpp is the CPU model of the kernel's BVH walk
 that the host builder's choices were compared with."""
import os
import re
import shutil
import subprocess

import pytest

from luisarender_amd import _ffi
from luisarender_amd.scenes import cornell_box


def test_bvh_sim_builds_and_counts(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    _ffi.host_lib()
    exe = tmp_path / "bvh_sim"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(_ffi.REPO_ROOT, "include"), os.path.join(_ffi.REPO_ROOT, "tools", "bvh_sim.cpp"),
                           "-L", _ffi.LIB_DIR, "-llrhost", f"-Wl,-rpath,{_ffi.LIB_DIR}", "-o", str(exe)])
    scene = tmp_path / "c.luisa"
    scene.write_text(cornell_box(resolution=64, spp=1))
    out = {}
    for knobs in ({}, {"LR_BVH_SWEEP": "0", "LR_BVH_COLLAPSE": "0", "LR_BVH_REINSERT": "0"}):
        r = subprocess.run([str(exe), str(scene), "48", "4"], capture_output=True, text=True, timeout=120, env={**os.environ, **knobs})
        assert r.returncode == 0, r.stderr
        m = re.search(r"nodes (\d+), tris (\d+) \| closest: rays (\d+) nodes/ray ([\d.]+) tris/ray ([\d.]+)", r.stdout)
        assert m, r.stdout
        out[bool(knobs)] = (int(m.group(1)), int(m.group(2)), float(m.group(4)))
    # 32 triangles, every ray of the closed box hits something; the default builder is never worse than the round-1b one here
    assert out[False][1] == 32 and out[True][1] == 32 and out[False][2] <= out[True][2] * 1.05


def test_default_builder_beats_the_round1b_builder_on_a_room(tmp_path):
    """regression guard for DESIGN.md §4.6: on a (small) bathroom-class room the default builder (exact sweep + reinsertion +
    optimal collapse) visits clearly fewer nodes per ray than 16-bin SAH + greedy collapse"""
    from luisarender_amd.scenes import generate_room_scene
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    _ffi.host_lib()
    exe = tmp_path / "bvh_sim"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(_ffi.REPO_ROOT, "include"), os.path.join(_ffi.REPO_ROOT, "tools", "bvh_sim.cpp"),
                           "-L", _ffi.LIB_DIR, "-llrhost", f"-Wl,-rpath,{_ffi.LIB_DIR}", "-o", str(exe)])
    scene = generate_room_scene(str(tmp_path), target_triangles=40_000, resolution=(64, 64), spp=1)
    steps = {}
    for name, knobs in (("default", {}), ("round1b", {"LR_BVH_SWEEP": "0", "LR_BVH_COLLAPSE": "0", "LR_BVH_REINSERT": "0"})):
        r = subprocess.run([str(exe), scene, "64", "5"], capture_output=True, text=True, timeout=300, env={**os.environ, **knobs})
        assert r.returncode == 0, r.stderr
        steps[name] = float(re.search(r"total steps/ray ([\d.]+)", r.stdout).group(1))
    assert steps["default"] < 0.92 * steps["round1b"], steps


def test_query_column_arithmetic_under_the_sanitizers(tmp_path):
    """tools/query_columns_check.cpp: the staged-call routine's column arithmetic (csrc/hip/query_columns.h: which bytes of which host
    column are chunk i, what a slot must hold) as a stand-alone program under AddressSanitizer and UBSan, for 0, 1, 2^20, 2^20 + 65 and
    2^31 - 1 records"""
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "query_columns_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(_ffi.REPO_ROOT, "tools", "query_columns_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "query columns: ok" in r.stdout, r.stdout + r.stderr
