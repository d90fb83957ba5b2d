"""Reference of the ray queries (include/lrhip.h: lrhip_trace_rays): a float64 Moeller-Trumbore over THE BAKED fp32 RECORDS
THE KERNEL READS -- Scene.view().accel.triangles (v0, e1, e2, inst, prim, flags) widened to float64 -- by brute force, with the accept rule of
trav_leaf_test (dev_trace.h): min(u, v) >= 0, u + v <= 1, t_min < t < t_max, flags & 1.  No BVH, no float32: what it disagrees with the
device about is the device's traversal or its arithmetic.

A ray is AMBIGUOUS when float32 may legitimately decide otherwise, and is left out of the comparisons:
  * some visible triangle with t in range and t <= t_best (1 + 1e-4) has |min(u, v, 1 - u - v)| < 1e-4 (any-hit: any triangle in range);
  * a visible triangle with (u, v) inside has |t - t_min| < 1e-5 or |t - t_max| < 1e-5 max(1, t_max) (on either side of the bound: a
    superset of "an accepted triangle", since float32 may also accept what float64 just rejects);
  * two accepted triangles lie within 1e-5 relative of t_best (closest hit only).
The share left out may not exceed AMBIGUOUS_CAP per scene and mode (tests/test_raycast_reference.py asserts it for every case)."""
import functools
import tempfile

import numpy as np

from luisarender_amd import Scene
from luisarender_amd.scenes import cornell_box
from luisarender_amd.scenes.bathroom import generate_room_scene, inline_mesh

INVALID = 0xFFFFFFFF
EDGE_EPS = 1e-4       # barycentric distance from an edge, and the relative depth window in which an edge-grazing triangle matters
BOUND_EPS = 1e-5      # distance of t from t_min / t_max (the latter relative to max(1, t_max))
TIE_EPS = 1e-5        # relative distance of two accepted triangles
AMBIGUOUS_CAP = 0.01
RAY_COUNT = 4133      # not a multiple of 64
RAY_SEED = 11
T_MIN = 1e-4

# The largest errors of the device's closest hits on unambiguous rays over the three scenes below, measured on the MI355X
# (tests/test_gpu_raycast.py prints them): |t - t_ref| / max(1, t_ref) and max(|u - u_ref|, |v - v_ref|).  The device's triangle test
# uses v_rcp_f32 (1 ulp) and written-out fmas.  The bars are 4 x the recorded values -- the project's margin for a float32-against-float64
# bar -- and the test asserts that they stay below the ambiguity thresholds above (a looser bar could pass a neighbouring triangle's result).
MEASURED_T_ERROR = 2.7e-6   # soup 4.2e-7, cornell 2.7e-6, room 1.9e-7
MEASURED_UV_ERROR = 1.1e-5  # soup 2.5e-6, cornell 2.4e-7, room 1.1e-5
BAR_T = 4.0 * MEASURED_T_ERROR
BAR_UV = 4.0 * MEASURED_UV_ERROR

_TRIANGLE = np.dtype([("v0", np.float32, 3), ("inst", np.uint32), ("e1", np.float32, 3), ("prim", np.uint32), ("e2", np.float32, 3),
                      ("flags", np.uint32)])
_HEAD = """Camera cam : Pinhole { fov { 40 } spp { 1 } film : Color { resolution { 8, 8 } } position { 0, 0, 5 } look_at { 0, 0, 0 } }
"""


def baked_triangles(scene):
    """lr_scene.accel.triangles of the scene AS IT STANDS (after set_time: the re-baked ones), a structured copy"""
    accel = scene.view().accel
    assert _TRIANGLE.itemsize == 48
    raw = np.ctypeslib.as_array(accel.triangles, shape=(accel.triangle_count,))
    return np.frombuffer(raw.tobytes(), dtype=_TRIANGLE).copy()


def scene_bounds(scene):
    accel = scene.view().accel
    return np.array(accel.world_min[:], np.float64), np.array(accel.world_max[:], np.float64)


def soup_text(n=2000, seed=7):
    """an InlineMesh of n triangles: centres uniform in [-1, 1]^3, edge vectors N(0, 0.12^2) per component"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1.0, 1.0, (n, 3))
    e1, e2 = rng.normal(0.0, 0.12, (n, 3)), rng.normal(0.0, 0.12, (n, 3))
    v = np.stack([centre, centre + e1, centre + e2], axis=1).reshape(-1, 3)
    mesh = inline_mesh("soup", v, np.arange(3 * n))[:-2] + "  surface : Matte { Kd : Constant { v { 0.5 } } }\n}\n"
    return mesh + _HEAD + "render { cameras { @cam } shapes { @soup } integrator : MegaPath { } }\n"


@functools.lru_cache(maxsize=None)
def scene_of(name):
    if name == "soup":
        return Scene.from_string(soup_text())
    if name == "soup64":
        return Scene.from_string(soup_text(64))
    if name == "cornell":
        return Scene.from_string(cornell_box(resolution=16, spp=1))
    if name == "room":  # instanced meshes under SRT transforms and a deeper tree; the smallest fixtures the generator's arguments give
        with tempfile.TemporaryDirectory(prefix="raycast_room_") as out_dir:  # (inline meshes: the one file holds the scene)
            return Scene.load(generate_room_scene(out_dir, target_triangles=6000, resolution=(16, 16), spp=1, inline_meshes=True,
                                                  mesh_levels=(2, 3), torus_res=(24, 12), box_n=4))
    raise KeyError(name)


SCENES = ("soup", "cornell", "room")


def make_rays(scene, n=RAY_COUNT, seed=RAY_SEED):
    """[n, 8] float32 (o, t_min, d, t_max): origins uniform in the scene bounds grown by 10 % (5 % on each side), directions uniform on the sphere; the first
    eighth axis-parallel (two zero components: the safe_inverse path), the second eighth segments with t_max uniform in 5 .. 80 % of the
    scene's diagonal, every other ray unbounded; t_min = 1e-4"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(scene)
    grow = 0.05 * (hi - lo)
    origin = rng.uniform(lo - grow, hi + grow, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    eighth = n // 8
    axis, sign = rng.integers(0, 3, eighth), rng.choice([-1.0, 1.0], eighth)
    d[:eighth] = 0.0
    d[np.arange(eighth), axis] = sign
    t_max = np.full(n, np.inf)
    t_max[eighth:2 * eighth] = rng.uniform(0.05, 0.8, eighth) * np.linalg.norm(hi - lo)
    rays = np.empty((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origin, T_MIN, d, t_max
    return rays


def reference(tris, rays, chunk=64):
    """-> dict of per-ray arrays: hit, t, u, v, inst, prim, tri of the closest accepted triangle (a miss: t = inf, u = v = 0, ids INVALID),
    occluded (some accepted triangle), ambiguous_closest, ambiguous_any"""
    n = len(rays)
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    visible = (tris["flags"] & 1) != 0
    out = {"hit": np.zeros(n, bool), "t": np.full(n, np.inf), "u": np.zeros(n), "v": np.zeros(n),
           "inst": np.full(n, INVALID, np.uint32), "prim": np.full(n, INVALID, np.uint32), "tri": np.full(n, INVALID, np.uint32),
           "occluded": np.zeros(n, bool), "ambiguous_closest": np.zeros(n, bool), "ambiguous_any": np.zeros(n, bool)}
    if len(tris) == 0 or n == 0:
        return out
    r64 = rays.astype(np.float64)

    def cross(a, b):
        return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    E1, E2 = [e1[None, :, k] for k in range(3)], [e2[None, :, k] for k in range(3)]
    for first in range(0, n, chunk):
        r = r64[first:first + chunk]
        sl = slice(first, first + len(r))
        o, d = [r[:, k, None] for k in range(3)], [r[:, 4 + k, None] for k in range(3)]
        t_min, t_max = r[:, 3, None], r[:, 7, None]
        with np.errstate(all="ignore"):
            pvec = cross(d, E2)
            inv_det = 1.0 / dot(E1, pvec)
            tvec = [o[k] - v0[None, :, k] for k in range(3)]
            u = dot(tvec, pvec) * inv_det
            qvec = cross(tvec, E1)
            v = dot(d, qvec) * inv_det
            t = dot(E2, qvec) * inv_det
            inside = (np.minimum(u, v) >= 0.0) & (u + v <= 1.0) & visible[None, :]
            in_range = (t > t_min) & (t < t_max)
            accepted = inside & in_range
            t_acc = np.where(accepted, t, np.inf)
            best = np.argmin(t_acc, axis=1)
            rows = np.arange(len(r))
            t_best = t_acc[rows, best]
            hit = np.isfinite(t_best)
            edge = np.abs(np.minimum(np.minimum(u, v), 1.0 - u - v)) < EDGE_EPS
            grazing = edge & in_range & visible[None, :]
            near_front = t <= (t_best + EDGE_EPS * np.abs(t_best))[:, None]  # (t_best = inf: every triangle in range)
            at_bound = inside & ((np.abs(t - t_min) < BOUND_EPS) | (np.abs(t - t_max) < BOUND_EPS * np.maximum(1.0, t_max)))
            ties = (accepted & (t <= (t_best * (1.0 + TIE_EPS))[:, None])).sum(axis=1) >= 2
        out["hit"][sl], out["occluded"][sl] = hit, hit
        out["t"][sl] = t_best
        out["u"][sl], out["v"][sl] = np.where(hit, u[rows, best], 0.0), np.where(hit, v[rows, best], 0.0)
        for key in ("inst", "prim"):
            out[key][sl] = np.where(hit, tris[key][best], INVALID)
        out["tri"][sl] = np.where(hit, best, INVALID)
        out["ambiguous_any"][sl] = grazing.any(axis=1) | at_bound.any(axis=1)
        out["ambiguous_closest"][sl] = (grazing & near_front).any(axis=1) | at_bound.any(axis=1) | ties
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, rays, reference over its baked triangles), computed once per process and shared: do not modify"""
    scene = scene_of(name)
    rays = make_rays(scene)
    ref = reference(baked_triangles(scene), rays)
    rays.setflags(write=False)
    for a in ref.values():
        a.setflags(write=False)
    return scene, rays, ref
