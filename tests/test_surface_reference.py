"""tests/surface_reference.py held to the oracle on the CPU: for the oracle's own camera rays and closest hits on the plane-and-ball scene of
tests/test_gpu_aov.py (restated here), the float64 restatement of Geometry::shading_point puts p on the ray at the oracle's t, the floor's
shading normal is the plane's, and the ball's interpolated normal is the analytic sphere's at the tessellation's accuracy -- the bars of
test_first_hit_buffers.  The GPU tests compare the device with this reference; this file is what the reference itself rests on."""
import functools

import numpy as np

import surface_reference as R
from instance_scene import host_tables
from luisarender_amd import Scene
from oracle.check import Oracle

# tests/test_gpu_aov.py: PLANE_BALL
PLANE_BALL = """
Surface w : Matte { Kd : Constant { v { 0.5 } } }
Shape floor : InlineMesh { positions { -50,0,-50, 50,0,-50, 50,0,50, -50,0,50 } indices { 0,2,1, 0,3,2 } surface { @w } }
Shape ball : Sphere { subdivision { 4 } surface { @w } transform : SRT { scale { 1.5, 1.5, 1.5 } translate { 0, 1.5, -6 } } }
Camera cam : Pinhole { fov { 50 } spp { 4 } film : Color { resolution { 40, 30 } } filter : Gaussian { radius { 1.5 } }
  position { 0, 3, 2 } look_at { 0, 1, -6 } }
render { cameras { @cam } shapes { @floor, @ball } environment : Spherical { emission : Constant { v { 1 } } }
  integrator : AOV { components { "mask", "depth", "ndc", "normal" } } }
"""
BALL_CENTRE = np.array([0.0, 1.5, -6.0])


def camera_rays(scene, sample):
    """[H * W, 8] float32 rays (o, 0, d, inf) of the oracle's camera for sample `sample` of every pixel, row by row"""
    o = Oracle(scene, bake_instances=True)
    rays = np.zeros((o.height * o.width, 8), np.float32)
    for py in range(o.height):
        for px in range(o.width):
            r = o.camera_ray(px, py, sample)
            rays[py * o.width + px, 0:3], rays[py * o.width + px, 4:7] = r[0:3], r[3:6]
    rays[:, 7] = np.inf
    o.close()
    return rays


@functools.lru_cache(maxsize=None)
def plane_ball_hits():
    """(scene, rays of sample 0, the oracle's closest hits as columns inst, prim, u, v, t) -- computed once, shared: do not modify"""
    scene = Scene.from_string(PLANE_BALL)
    rays = camera_rays(scene, 0)
    o = Oracle(scene, bake_instances=True)
    hits = np.array([o.trace_closest(r[0:3], r[4:7]) for r in rays], np.float64)
    o.close()
    rays.setflags(write=False)
    hits.setflags(write=False)
    return scene, rays, hits


def test_points_lie_on_the_oracles_rays():
    scene, rays, hits = plane_ball_hits()
    hit = hits[:, 0] != R.INVALID
    assert hit.mean() > 0.5 and (~hit).any()  # sky above the horizon
    inst, prim, u, v, t = (hits[hit][:, k] for k in range(5))
    ref = R.shading_points(scene, inst.astype(np.int64), prim.astype(np.int64), u, v)
    r = rays[hit].astype(np.float64)
    want = r[:, 0:3] + t[:, None] * r[:, 4:7]
    err = np.linalg.norm(ref["p"] - want, axis=1) / np.maximum(1.0, t)  # the depth bar of test_first_hit_buffers: |p - o| against t
    assert err.max() <= 1e-5, err.max()
    assert (ref["area"] > 0).all() and np.allclose(np.linalg.norm(ref["ng"], axis=1), 1.0, atol=1e-12)


def test_normals_of_floor_and_ball():
    scene, _, hits = plane_ball_hits()
    hit = hits[:, 0] != R.INVALID
    inst, prim, u, v, _ = (hits[hit][:, k] for k in range(5))
    ref = R.shading_points(scene, inst.astype(np.int64), prim.astype(np.int64), u, v)
    floor, ball = inst == 0, inst == 1
    assert floor.sum() > 100 and ball.sum() > 50
    assert np.array_equal(ref["ns"][floor], np.broadcast_to([0.0, 1.0, 0.0], (int(floor.sum()), 3)))
    assert np.array_equal(ref["ng"][floor], ref["ns"][floor])
    analytic = ref["p"][ball] - BALL_CENTRE
    analytic /= np.linalg.norm(analytic, axis=1, keepdims=True)
    assert np.abs(ref["ns"][ball] - analytic).max() <= 5e-3
    # the frame: unit tangents orthogonal to ns wherever the uv determinant is not zero (the ball), and the floor's uv are its (u, v)
    assert (ref["det"][ball] != 0).all() and (ref["det"][floor] == 0).all()
    s = ref["tangent"][ball]
    assert np.allclose(np.linalg.norm(s, axis=1), 1.0, atol=1e-12) and np.abs(np.einsum("nk,nk->n", s, ref["ns"][ball])).max() < 1e-12
    assert np.array_equal(ref["uv"][floor], np.stack([u[floor], v[floor]], axis=1))


def test_tables_and_records():
    scene, _, _ = plane_ball_hits()
    t = host_tables(scene)
    assert len(t["instances"]) == 2 and (t["instances"][:, 0] & R.HAS_SURFACE).all() and not (t["instances"][:, 0] & R.HAS_LIGHT).any()
    rec = R.hit_records([1, 0], [5, 1], [0.25, 0.5], [0.5, 0.125])
    assert rec.shape == (2, 8) and rec.dtype == np.float32 and rec.view(np.uint32)[:, 3:6].tolist() == [[1, 5, R.INVALID], [0, 1, R.INVALID]]
    assert R.invalid_record().view(np.float32)[[0, 4, 8, 20, 24, 28]].tolist() == [0.0] * 6 and int((R.invalid_record() == R.INVALID).sum()) == 5
    for name in ("P", "NG", "NS", "UV", "TANGENT", "AREA", "AOV_BALL_NORMAL"):  # every bar is 4 x its recorded value, and no value is a bug's
        measured, bar = getattr(R, f"MEASURED_{name}_ERROR"), getattr(R, f"BAR_{name}")
        assert bar == 4.0 * measured and (measured <= R.LARGEST_SOUND_ERROR or name == "AOV_BALL_NORMAL")
