"""The float64 reference of the ray queries (tests/raycast_reference.py) on hand-computed cases, the cap on the share of rays it leaves
out as ambiguous for every scene and ray set tests/test_gpu_raycast.py uses, and MegaPathRenderer.trace's input checker.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import raycast_reference as R
from luisarender_amd import _ffi
from luisarender_amd.render import RayHits, check_rays


def _triangles(rows):
    """rows of (v0, e1, e2, inst, prim, flags)"""
    tris = np.zeros(len(rows), R._TRIANGLE)
    for k, (v0, e1, e2, inst, prim, flags) in enumerate(rows):
        tris[k] = (v0, inst, e1, prim, e2, flags)
    return tris


def _ray(o, d, t_min=1e-4, t_max=np.inf):
    return np.array([[*o, t_min, *d, t_max]], np.float32)


# the triangle (0,0,0) (1,0,0) (0,1,0) in the plane z = 0, seen from z = 2 looking down
ONE = _triangles([((0, 0, 0), (1, 0, 0), (0, 1, 0), 5, 9, 3)])


def test_centre_hit():
    ref = R.reference(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -1)))
    assert ref["hit"][0] and ref["occluded"][0] and not ref["ambiguous_closest"][0] and not ref["ambiguous_any"][0]
    assert ref["t"][0] == pytest.approx(2.0, abs=1e-12)
    assert ref["u"][0] == pytest.approx(0.25, abs=1e-12) and ref["v"][0] == pytest.approx(0.5, abs=1e-12)  # weights of vertex 1 and vertex 2
    assert (ref["inst"][0], ref["prim"][0], ref["tri"][0]) == (5, 9, 0)
    # t is in units of |d|
    ref = R.reference(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -4)))
    assert ref["t"][0] == pytest.approx(0.5, abs=1e-12)


@pytest.mark.parametrize("x, y", [(-0.01, 0.5), (0.5, -0.01), (0.51, 0.51)])
def test_miss_beside_each_edge(x, y):
    ref = R.reference(ONE, _ray((x, y, 2.0), (0, 0, -1)))
    assert not ref["hit"][0] and not ref["occluded"][0] and np.isinf(ref["t"][0])
    assert (ref["u"][0], ref["v"][0]) == (0.0, 0.0)
    assert ref["inst"][0] == ref["prim"][0] == ref["tri"][0] == R.INVALID
    assert not ref["ambiguous_closest"][0]  # 0.01 from the edge: far outside the 1e-4 band


def test_behind_the_origin_and_beyond_t_max():
    assert not R.reference(ONE, _ray((0.25, 0.5, 2.0), (0, 0, 1)))["hit"][0]
    assert not R.reference(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -1), t_max=1.5))["hit"][0]
    assert R.reference(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -1), t_max=2.5))["hit"][0]
    assert not R.reference(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -1), t_min=2.0))["hit"][0]  # both bounds are strict
    assert not R.reference(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -1), t_max=2.0))["hit"][0]


def test_closest_of_two_and_invisible_triangles():
    two = _triangles([((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, 0, 3), ((0, 0, 1), (1, 0, 0), (0, 1, 0), 1, 0, 3)])
    ref = R.reference(two, _ray((0.25, 0.5, 2.0), (0, 0, -1)))
    assert ref["tri"][0] == 1 and ref["t"][0] == pytest.approx(1.0, abs=1e-12)
    two["flags"][1] = 2  # bit 0 clear: an invisible instance's triangle is never hit
    ref = R.reference(two, _ray((0.25, 0.5, 2.0), (0, 0, -1)))
    assert ref["tri"][0] == 0 and ref["t"][0] == pytest.approx(2.0, abs=1e-12)


def test_what_counts_as_ambiguous():
    grazing = R.reference(ONE, _ray((0.25, 0.00005, 2.0), (0, 0, -1)))
    assert grazing["ambiguous_closest"][0] and grazing["ambiguous_any"][0]
    at_t_max = R.reference(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -1), t_max=2.000001))
    assert at_t_max["ambiguous_closest"][0] and at_t_max["ambiguous_any"][0]
    tie = _triangles([((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, 0, 3), ((0, 0, 1e-6), (1, 0, 0), (0, 1, 0), 1, 0, 3)])
    ref = R.reference(tie, _ray((0.25, 0.5, 2.0), (0, 0, -1)))
    assert ref["ambiguous_closest"][0] and not ref["ambiguous_any"][0]
    # a grazing triangle far BEHIND the closest hit does not matter to the closest hit, but to "some triangle in range"
    behind = _triangles([((0, 0, 1), (1, 0, 0), (0, 1, 0), 0, 0, 3), ((0.25, 0.49995, 0), (1, 0, 0), (0, 1, 0), 1, 0, 3)])
    ref = R.reference(behind, _ray((0.25, 0.5, 2.0), (0, 0, -1)))
    assert not ref["ambiguous_closest"][0] and ref["ambiguous_any"][0]


@pytest.mark.parametrize("name", R.SCENES)
def test_ambiguous_share_is_capped(name):
    """at most 1 % of a scene's rays may be left out of a comparison, for closest hit and any hit"""
    scene, rays, ref = R.case(name)
    assert rays.shape == (R.RAY_COUNT, 8) and R.RAY_COUNT % 64 != 0
    tris = R.baked_triangles(scene)
    assert len(tris) <= 8000
    for mode in ("ambiguous_closest", "ambiguous_any"):
        share = ref[mode].mean()
        print(f"[raycast] {name}: {len(tris)} triangles, {int(ref['hit'].sum())} hits, {mode} {int(ref[mode].sum())} of {len(rays)}")
        assert share <= R.AMBIGUOUS_CAP, (name, mode, share)
    assert 0.2 < ref["hit"].mean() < 0.95  # the ray set exercises hits and misses
    eighth = R.RAY_COUNT // 8
    assert ((rays[:eighth, 4:7] == 0).sum(axis=1) == 2).all()  # axis-parallel
    assert np.isfinite(rays[eighth:2 * eighth, 7]).all() and np.isinf(rays[2 * eighth:, 7]).all()  # segments, then unbounded rays


def test_the_room_has_instanced_meshes():
    scene, _, _ = R.case("room")
    view = scene.view()
    assert view.mesh_count < view.instance_count  # fixtures share meshes under SRT transforms


def test_check_rays():
    good = np.zeros((5, 8), np.float32)
    assert check_rays(good) == "numpy" and check_rays(np.zeros((0, 8), np.float32)) == "numpy"
    for bad in (np.zeros((5, 8), np.float64), np.zeros((5, 7), np.float32), np.zeros(8, np.float32), np.zeros((2, 5, 8), np.float32),
                np.zeros((8, 5), np.float32).T, np.zeros((5, 16), np.float32)[:, ::2], [[0.0] * 8], None):
        with pytest.raises(ValueError):
            check_rays(bad)


def test_check_rays_refuses_host_tensors():
    torch = pytest.importorskip("torch")
    for bad in (torch.zeros((5, 8)), torch.zeros((5, 8), dtype=torch.float64)):  # on the CPU: numpy is the host path
        with pytest.raises(ValueError):
            check_rays(bad)


def test_ray_hits_are_views_of_one_buffer():
    buffer = np.zeros((3, 8), np.float32)
    hits = RayHits(buffer)
    words = buffer.view(np.uint32)
    words[:, 3:6] = R.INVALID
    buffer[:, 0] = np.inf
    words[1, 3:6] = (4, 7, 11)
    buffer[1, 0:3] = (2.5, 0.25, 0.5)
    for field in (hits.t, hits.u, hits.v, hits.inst, hits.prim, hits.tri):
        assert np.shares_memory(field, buffer)
    assert list(hits.hit) == [False, True, False] and len(hits) == 3
    assert (hits.t[1], hits.u[1], hits.v[1], hits.inst[1], hits.prim[1], hits.tri[1]) == (2.5, 0.25, 0.5, 4, 7, 11)


def test_abi_structs():
    """32-byte rays and hit records (two dwordx4 each), laid out as the numpy rows are"""
    assert C.sizeof(_ffi.Ray) == C.sizeof(_ffi.RayHit) == 32 and C.sizeof(_ffi.RayQueryParams) == 32
    assert _ffi.Ray.t_min.offset == 12 and _ffi.Ray.d.offset == 16 and _ffi.Ray.t_max.offset == 28
    assert _ffi.RayHit.inst.offset == 12 and _ffi.RayHit.tri.offset == 20
    for name in ("lrhip_ray", "lrhip_ray_hit", "lrhip_ray_query_params"):
        assert name in _ffi.STRUCTS
