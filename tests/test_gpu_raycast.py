"""Ray queries on the device (include/lrhip.h: lrhip_trace_rays) against the float64 brute-force reference of
tests/raycast_reference.py, ray by ray, and the properties the header promises: order independence, screened rays, visibility, the
alpha test, moving geometry, the torch path, the error returns."""
import ctypes as C

import numpy as np
import pytest

import raycast_reference as R
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import DeviceError, MegaPathRenderer

pytestmark = pytest.mark.gpu

LRHIP_ERROR_INVALID = -1
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def _is_miss(hits, rows=slice(None)):
    return (np.isposinf(hits.t[rows]) & (hits.u[rows] == 0) & (hits.v[rows] == 0) & (hits.inst[rows] == R.INVALID) & (hits.prim[rows] == R.INVALID)
            & (hits.tri[rows] == R.INVALID) & (hits.buffer.view(np.uint32)[rows, 6:8] == 0).all(axis=1))


@pytest.mark.parametrize("name", R.SCENES)
def test_closest_hit_against_the_reference(renderer, capsys, name):
    """Measured on the MI355X over the three scenes (raycast_reference.py: MEASURED_T_ERROR, MEASURED_UV_ERROR); the bars are 4 x the
    recorded values and may not exceed the ambiguity thresholds 1e-4 (t) and 1e-3 (u, v)."""
    scene, rays, ref = R.case(name)
    renderer.upload(scene)
    hits = renderer.trace(rays)
    ok = ~ref["ambiguous_closest"]
    hit = np.asarray(hits.hit)
    both = ok & ref["hit"] & hit
    err_t = float((np.abs(hits.t[both].astype(np.float64) - ref["t"][both]) / np.maximum(1.0, ref["t"][both])).max())
    err_uv = float(max(np.abs(hits.u[both] - ref["u"][both]).max(), np.abs(hits.v[both] - ref["v"][both]).max()))
    with capsys.disabled():
        print(f"\n[raycast] {name}: {int(ok.sum())} unambiguous rays, {int(both.sum())} hits, hit/miss differs on {int((hit != ref['hit'])[ok].sum())}, "
              f"t error {err_t:.3e} (recorded {R.MEASURED_T_ERROR:.1e}, bar {R.BAR_T:.1e}), uv error {err_uv:.3e} "
              f"(recorded {R.MEASURED_UV_ERROR:.1e}, bar {R.BAR_UV:.1e}), {renderer.last_trace_ms():.3f} ms")
    assert hits.buffer.shape == (len(rays), 8) and hits.buffer.dtype == np.float32
    assert np.array_equal(hit[ok], ref["hit"][ok])
    for key in ("inst", "prim", "tri"):
        assert np.array_equal(getattr(hits, key)[ok], ref[key][ok]), key
    assert _is_miss(hits, ~hit).all()  # every miss, ambiguous rays included, is the one miss record
    assert (hits.buffer.view(np.uint32)[:, 6:8] == 0).all()
    assert err_t <= R.BAR_T <= 1e-4
    assert err_uv <= R.BAR_UV <= 1e-3


@pytest.mark.parametrize("name", R.SCENES)
def test_any_hit_against_the_reference(renderer, name):
    scene, rays, ref = R.case(name)
    renderer.upload(scene)
    occluded = renderer.trace(rays, any_hit=True)
    ok = ~ref["ambiguous_any"]
    assert occluded.shape == (len(rays),) and occluded.dtype == bool
    assert np.array_equal(occluded[ok], ref["occluded"][ok])
    assert 0.2 < occluded.mean() < 0.95


def test_order_and_grouping(renderer):
    """a ray's result is a function of the ray and the scene only"""
    scene, rays, _ = R.case("soup")
    renderer.upload(scene)
    full = renderer.trace(rays).buffer.view(np.uint32)
    full_any = renderer.trace(rays, any_hit=True)
    assert np.array_equal(renderer.trace(rays).buffer.view(np.uint32), full)  # twice: the same bits
    assert np.array_equal(renderer.trace(rays, any_hit=True), full_any)
    perm = np.random.default_rng(3).permutation(len(rays))
    shuffled = np.ascontiguousarray(rays[perm])
    assert np.array_equal(renderer.trace(shuffled).buffer.view(np.uint32), full[perm])
    assert np.array_equal(renderer.trace(shuffled, any_hit=True), full_any[perm])
    for count in (1, 63, 64, 65, len(rays)):
        head = np.ascontiguousarray(rays[:count])
        assert np.array_equal(renderer.trace(head).buffer.view(np.uint32), full[:count]), count
        assert np.array_equal(renderer.trace(head, any_hit=True), full_any[:count]), count
    # the alpha-test flag is ignored for a scene without non-opaque surfaces
    assert scene.view().any_non_opaque == 0
    assert np.array_equal(renderer.trace(rays, alpha_test=True).buffer.view(np.uint32), full)
    # count = 0 is legal, launches nothing and leaves `out` alone
    empty = renderer.trace(np.zeros((0, 8), np.float32))
    assert len(empty) == 0 and renderer.trace(np.zeros((0, 8), np.float32), any_hit=True).shape == (0,)
    sentinel = np.full((4, 8), 0xDEADBEEF, np.uint32)
    p = _ffi.RayQueryParams(rays.ctypes.data, sentinel.ctypes.data, 0, _ffi.RAY_CLOSEST, 0)
    assert renderer._lib.lrhip_trace_rays(renderer._ctx, C.byref(p)) == 0
    renderer.synchronize()
    assert (sentinel == 0xDEADBEEF).all() and renderer.last_trace_ms() == 0.0


def test_a_host_batch_larger_than_one_staging_chunk(renderer):
    """host pointers are staged 2^20 rays at a time: a batch that needs two chunks gives every ray the bits it has in a small batch"""
    scene, rays, _ = R.case("soup")
    renderer.upload(scene)
    full = renderer.trace(rays).buffer.view(np.uint32)
    full_any = renderer.trace(rays, any_hit=True)
    copies = (1 << 20) // len(rays) + 1
    big = np.tile(rays, (copies, 1))
    assert (1 << 20) < len(big) < (1 << 21) and len(big) % 64 != 0
    assert np.array_equal(renderer.trace(big).buffer.view(np.uint32), np.tile(full, (copies, 1)))
    assert renderer.last_trace_ms() > 0.0
    assert np.array_equal(renderer.trace(big, any_hit=True), np.tile(full_any, copies))


def test_screened_rays(renderer):
    """rays that never enter the traversal loop: misses / not occluded, and their neighbours' results unchanged"""
    scene, rays, _ = R.case("soup")
    renderer.upload(scene)
    batch = rays[:200].copy()
    clean = renderer.trace(batch).buffer.view(np.uint32).copy()
    clean_any = renderer.trace(batch, any_hit=True)
    nan = np.float32(np.nan)
    bad = {3: (0, nan), 64: (4, INF), 65: (slice(4, 7), 0.0), 100: (7, np.float32(1e-4)), 101: (7, np.float32(-1.0)), 130: (3, nan),
           131: (5, -INF), 199: (7, nan), 198: (1, INF)}
    for row, (column, value) in bad.items():
        batch[row, column] = value  # NaN origin, Inf direction, zero direction, t_max = t_min, t_max < t_min, NaN t_min, ...
    hits = renderer.trace(batch)
    occluded = renderer.trace(batch, any_hit=True)
    rows = np.array(sorted(bad))
    others = np.setdiff1d(np.arange(len(batch)), rows)
    assert _is_miss(hits, rows).all() and not occluded[rows].any()
    assert np.array_equal(hits.buffer.view(np.uint32)[others], clean[others]) and np.array_equal(occluded[others], clean_any[others])
    assert clean_any[rows].any()  # (some of the replaced rays did hit something before)
    # a batch of nothing but screened rays
    assert _is_miss(renderer.trace(np.ascontiguousarray(batch[rows]))).all()


def test_direction_length_and_negative_t_min_beside_their_neighbours(renderer):
    """what the header promises of the caller's units, among ordinary rays: a direction scaled by a power of two finds the same triangle with t scaled
    the other way and the same u, v, to within the bars of the reference comparison (the normalisation rounds); directions of 2^-140, whose components
    are denormal and rounded, are judged in test_gpu_raycast_edges.py; t_min =
    -0.0 or negative searches from +0 -- the result of t_min = +0; and the neighbours keep their bits"""
    scene, rays, _ = R.case("soup")
    renderer.upload(scene)
    batch = rays[:200].copy()
    batch[:, 3] = 0.0
    clean = renderer.trace(batch)
    clean_bits = clean.buffer.view(np.uint32).copy()
    clean_any = renderer.trace(batch, any_hit=True)
    hit_rows = np.nonzero(np.asarray(clean.hit))[0]
    assert len(hit_rows) >= 40
    scaled = {int(row): k for row, k in zip(hit_rows[0:16], (-120, -100, -30, -10, 10, 30, 100, 126) * 2)}
    negative = {int(row): value for row, value in zip(hit_rows[16:24], (-0.0, -1.0, -1e30, -1e-40) * 2)}
    changed = batch.copy()
    for row, k in scaled.items():
        changed[row, 4:7] = (batch[row, 4:7].astype(np.float64) * 2.0 ** k).astype(np.float32)
        assert (changed[row, 4:7].astype(np.float64) == batch[row, 4:7].astype(np.float64) * 2.0 ** k).all()  # exact: no component turns denormal
    for row, value in negative.items():
        changed[row, 3] = value
    hits = renderer.trace(changed)
    occluded = renderer.trace(changed, any_hit=True)
    others = np.setdiff1d(np.arange(len(batch)), list(scaled) + list(negative))
    assert np.array_equal(hits.buffer.view(np.uint32)[others], clean_bits[others]) and np.array_equal(occluded[others], clean_any[others])
    rows = np.array(sorted(negative))
    assert np.array_equal(hits.buffer.view(np.uint32)[rows], clean_bits[rows]) and occluded[rows].all()  # the bits of t_min = +0
    for row, k in scaled.items():
        assert occluded[row] and hits.tri[row] == clean.tri[row] and hits.inst[row] == clean.inst[row] and hits.prim[row] == clean.prim[row], (row, k)
        want = float(clean.t[row]) * 2.0 ** -k
        if want > np.finfo(np.float32).max:
            assert np.isposinf(hits.t[row]), (row, k)
        else:
            assert abs(float(hits.t[row]) - want) <= max(R.BAR_T * want, 2.0 ** -149), (row, k)
        assert abs(hits.u[row] - clean.u[row]) <= R.BAR_UV and abs(hits.v[row] - clean.v[row]) <= R.BAR_UV, (row, k)


QUADS = """
Texture holes : Checkerboard { on : Constant { v { 1 } } off : Constant { v { 0 } } scale { 1 } }
Surface cutout : Matte { Kd : Constant { v { 0.7 } } alpha { @holes } }
Surface plain : Matte { Kd : Constant { v { 0.3 } } }
Shape front : InlineMesh { positions { -1,-1,1, 1,-1,1, 1,1,1, -1,1,1 } indices { 0,1,2, 0,2,3 }
  uvs { 0,0.5, 2,0.5, 2,0.5, 0,0.5 } surface { @FRONT_SURFACE } FRONT_EXTRA }
Shape back : InlineMesh { positions { -2,-2,0, 2,-2,0, 2,2,0, -2,2,0 } indices { 0,1,2, 0,2,3 } surface { @plain } }
Camera cam : Pinhole { fov { 40 } spp { 1 } film : Color { resolution { 8, 8 } } position { 0, 0, 5 } look_at { 0, 0, 0 } }
render { cameras { @cam } shapes { @front, @back } integrator : MegaPath { } }
"""


def _down_rays(xy, z=3.0, t_max=np.inf):
    rays = np.zeros((len(xy), 8), np.float32)
    rays[:, 0:2], rays[:, 2], rays[:, 3], rays[:, 6], rays[:, 7] = xy, z, 1e-4, -1.0, t_max
    return rays


def _instances_by_height(scene):
    tris = R.baked_triangles(scene)
    return {float(z): int(tris["inst"][tris["v0"][:, 2] == z][0]) for z in np.unique(tris["v0"][:, 2])}


def test_alpha_tested_quad(renderer):
    """the front quad's opacity is 1 where x < 0 (checkerboard cell u in [0, 1)) and 0 where x > 0: the stochastic test is deterministic"""
    scene = Scene.from_string(QUADS.replace("FRONT_SURFACE", "cutout").replace("FRONT_EXTRA", ""))
    assert scene.view().any_non_opaque == 1
    renderer.upload(scene)
    inst = _instances_by_height(scene)
    rng = np.random.default_rng(5)
    xy = np.stack([rng.uniform(0.1, 0.9, 96) * np.where(np.arange(96) % 2 == 0, -1.0, 1.0), rng.uniform(-0.9, 0.9, 96)], axis=1)
    xy = xy[np.abs(np.abs(xy[:, 0]) - np.abs(xy[:, 1])) > 0.02]  # off the quads' diagonals
    rays = _down_rays(xy)
    opaque_side = xy[:, 0] < 0
    tested = renderer.trace(rays, alpha_test=True)
    assert np.array_equal(tested.inst, np.where(opaque_side, inst[1.0], inst[0.0]).astype(np.uint32))
    assert np.allclose(tested.t, np.where(opaque_side, 2.0, 3.0), atol=1e-5)
    untested = renderer.trace(rays)
    assert (untested.inst == inst[1.0]).all() and np.allclose(untested.t, 2.0, atol=1e-5)
    # occlusion of the segment that ends between the quads: the cut-out half lets it through
    segment = _down_rays(xy, t_max=2.5)
    assert np.array_equal(renderer.trace(segment, any_hit=True, alpha_test=True), opaque_side)
    assert renderer.trace(segment, any_hit=True).all()
    assert renderer.trace(rays, any_hit=True, alpha_test=True).all()  # the back quad stops every unbounded ray


def test_invisible_instance_is_never_hit(renderer):
    scene = Scene.from_string(QUADS.replace("FRONT_SURFACE", "plain").replace("FRONT_EXTRA", "visible { false }"))
    tris = R.baked_triangles(scene)
    assert ((tris["flags"] & 1) == 0).sum() == 2  # the front quad's two triangles
    renderer.upload(scene)
    inst = _instances_by_height(scene)
    xy = np.random.default_rng(6).uniform(-0.9, 0.9, (64, 2))
    xy = xy[np.abs(np.abs(xy[:, 0]) - np.abs(xy[:, 1])) > 0.02]
    rays = _down_rays(xy)
    hits = renderer.trace(rays)
    assert (hits.inst == inst[0.0]).all() and np.allclose(hits.t, 3.0, atol=1e-5)
    assert not renderer.trace(_down_rays(xy, t_max=2.5), any_hit=True).any()
    ref = R.reference(tris, rays)
    assert np.array_equal(hits.tri, ref["tri"]) and np.array_equal(hits.inst, ref["inst"])


MOVING = """
Shape lift : InlineMesh { positions { -1,-1,0, 1,-1,0, 1,1,0, -1,1,0 } indices { 0,1,2, 0,2,3 } surface : Matte { Kd : Constant { v { 0.5 } } }
  transform : Lerp { time_points { 0, 1 } transforms { SRT { translate { 0, 0, 0 } }, SRT { translate { 0, 0, 2 } } } } }
Camera cam : Pinhole { fov { 40 } spp { 1 } film : Color { resolution { 8, 8 } } position { 0, 0, 5 } look_at { 0, 0, 0 } }
render { cameras { @cam } shapes { @lift } integrator : MegaPath { } }
"""


def test_moving_geometry(renderer):
    """lrhip_update_scene re-bakes the triangles: the same ray's t follows the quad"""
    scene = Scene.from_string(MOVING)
    rays = _down_rays(np.array([[0.3, 0.1], [-0.4, 0.7], [0.5, -0.2]]), z=3.0)
    renderer.upload(scene)
    seen = []
    for k, time in enumerate((0.0, 0.25, 0.75)):
        if k > 0:
            assert scene.set_time(time)
            renderer.upload(scene, keep_film=True)
        ref = R.reference(R.baked_triangles(scene), rays)
        hits = renderer.trace(rays)
        assert ref["hit"].all() and not ref["ambiguous_closest"].any()
        assert np.array_equal(hits.tri, ref["tri"])
        assert (np.abs(hits.t - ref["t"]) / np.maximum(1.0, ref["t"])).max() <= R.BAR_T and np.allclose(ref["t"], 3.0 - 2.0 * time, atol=1e-5)
        seen.append(float(hits.t[0]))
    assert seen[0] > seen[1] > seen[2]


def test_torch_path(renderer):
    """device tensors in and out, no copy through the host: the numpy path's bits"""
    torch = pytest.importorskip("torch")
    scene, rays, _ = R.case("soup")
    renderer.upload(scene)
    want = renderer.trace(rays).buffer.view(np.uint32)
    want_any = renderer.trace(rays, any_hit=True)
    device_rays = torch.from_numpy(np.array(rays)).to("cuda:0")
    hits = renderer.trace(device_rays)
    assert isinstance(hits.buffer, torch.Tensor) and hits.buffer.device == device_rays.device and hits.buffer.shape == (len(rays), 8)
    assert np.array_equal(hits.buffer.cpu().numpy().view(np.uint32), want)
    assert hits.t.data_ptr() == hits.buffer.data_ptr() and hits.inst.data_ptr() == hits.buffer.data_ptr() + 12  # views, not copies
    assert np.array_equal(hits.hit.cpu().numpy(), want[:, 3] != R.INVALID)
    occluded = renderer.trace(device_rays, any_hit=True)
    assert occluded.dtype == torch.bool and np.array_equal(occluded.cpu().numpy(), want_any)
    assert renderer.last_trace_ms() > 0.0
    for bad in (device_rays.cpu(), device_rays.double(), device_rays[:, :7], device_rays.t()):
        with pytest.raises(ValueError):
            renderer.trace(bad)


def test_errors(renderer):
    scene, rays, _ = R.case("soup")
    lib = renderer._lib
    out = np.zeros((len(rays), 8), np.float32)

    def call(ctx, rays_ptr, out_ptr, count, mode, flags):
        p = _ffi.RayQueryParams(rays_ptr, out_ptr, count, mode, flags)
        rc = lib.lrhip_trace_rays(ctx, C.byref(p))
        return rc, lib.lrhip_last_error().decode()

    fresh = MegaPathRenderer(0)
    try:  # a query before any upload
        rc, message = call(fresh._ctx, rays.ctypes.data, out.ctypes.data, len(rays), _ffi.RAY_CLOSEST, 0)
        assert rc == LRHIP_ERROR_INVALID and "no scene" in message
        with pytest.raises(DeviceError):
            fresh.trace(rays)
    finally:
        fresh.close()
    renderer.upload(scene)
    rc, message = call(renderer._ctx, rays.ctypes.data, out.ctypes.data, len(rays), 7, 0)
    assert rc == LRHIP_ERROR_INVALID and "mode" in message
    rc, message = call(renderer._ctx, rays.ctypes.data, out.ctypes.data, len(rays), _ffi.RAY_ANY, 64)
    assert rc == LRHIP_ERROR_INVALID and "flags" in message
    rc, message = call(renderer._ctx, rays.ctypes.data, out.ctypes.data, 1 << 31, _ffi.RAY_CLOSEST, 0)
    assert rc == LRHIP_ERROR_INVALID and "2^31" in message
    torch = pytest.importorskip("torch")
    device_rays = torch.from_numpy(np.array(rays)).to("cuda:0")
    device_out = torch.empty((len(rays), 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for rays_ptr, out_ptr in ((device_rays.data_ptr() + 4, device_out.data_ptr()), (device_rays.data_ptr(), device_out.data_ptr() + 8)):
        rc, message = call(renderer._ctx, rays_ptr, out_ptr, 16, _ffi.RAY_CLOSEST, _ffi.RAY_DEVICE_POINTERS)
        assert rc == LRHIP_ERROR_INVALID and "aligned" in message
    # the context is as good as before
    assert np.array_equal(renderer.trace(rays, any_hit=True), renderer.trace(device_rays, any_hit=True).cpu().numpy())
