"""Deforming a mesh on the device (lrhip_set_mesh_vertices).  The yardstick is the host: context A takes the new call, context B
takes Scene.set_mesh_vertices (vertex write, normal recompute, re-bake and refit on the CPU, tests/test_mesh_vertices.py) +
upload(keep_film=True), i.e. lrhip_update_scene -- and the four device tables that move with the geometry must come out EQUAL BYTE FOR BYTE,
A's vertex table must hold the host view's bytes, and everything rendered or queried from the tables must be equal bit for bit."""
import ctypes as C

import numpy as np
import pytest

import instance_scene as S
import mesh_deform_scene as M
from luisarender_amd import _ffi
from luisarender_amd.render import DeviceError, MegaPathRenderer

pytestmark = pytest.mark.gpu

LRHIP_ERROR_INVALID, LRHIP_ERROR_UNSUPPORTED = -1, -3
TABLES = {"nodes": _ffi.TABLE_NODES, "bvh_triangles": _ffi.TABLE_BVH_TRIANGLES, "instances": _ffi.TABLE_INSTANCES, "shade_triangles": _ffi.TABLE_SHADE_TRIANGLES}
GEOMETRY = [name for name in TABLES if name != "instances"]  # what a deformation changes; the instance records stay


def tables(renderer) -> dict:
    return {name: renderer.scene_table(which) for name, which in TABLES.items()}


def vertex_table(renderer) -> np.ndarray:
    return renderer.scene_table(_ffi.TABLE_VERTICES).view(np.uint32)


def assert_equal_tables(a: dict, b: dict, what="") -> None:
    for name in TABLES:
        assert a[name].shape == b[name].shape, (what, name)
        rows = np.nonzero((a[name] != b[name]).any(axis=1))[0]
        assert rows.size == 0, (what, name, rows.size, rows[:8], a[name][rows[:1]].view(np.uint32), b[name][rows[:1]].view(np.uint32))


def differ(a: dict, b: dict) -> list:
    return [name for name in TABLES if not np.array_equal(a[name], b[name])]


def assert_both_routes_agree(ra, scene_b, rb, what) -> dict:
    """the four tables of A and B equal byte for byte, and the vertex tables of both the host view's bytes -> A's tables"""
    a = tables(ra)
    assert_equal_tables(a, tables(rb), what)
    host = S.host_tables(scene_b)["vertices"]
    for r in (ra, rb):
        got = vertex_table(r)
        rows = np.nonzero((got != host).any(axis=1))[0]
        assert got.shape == host.shape and rows.size == 0, (what, "vertices", rows.size, rows[:8], got[rows[:1]], host[rows[:1]])
    return a


@pytest.fixture
def pair():
    """(ids, scene A, context A, scene B, context B): two uploads of the fixture scene, checked on the CPU first"""
    scene_a, scene_b = M.room(), M.room()
    ids = M.check_room(scene_a)
    ra, rb = MegaPathRenderer(0), MegaPathRenderer(0)
    ra.upload(scene_a)
    rb.upload(scene_b)
    yield ids, scene_a, ra, scene_b, rb
    ra.close()
    rb.close()


def deform_both(ra, scene_b, rb, mesh, positions, normals=None, first=0, recompute_normals=False):
    ra.set_mesh_vertices(mesh, positions, normals, first=first, recompute_normals=recompute_normals)
    scene_b.set_mesh_vertices(mesh, positions, normals, first=first, recompute_normals=recompute_normals)
    rb.upload(scene_b, keep_film=True)


def first_move(scene):
    """the first deformation of the balls' mesh with normals of the caller's (not unit length: they are written as given)"""
    p, n = scene.mesh_vertices(1)
    return M.first_deformation(p), np.ascontiguousarray(n[:, [1, 2, 0]] * np.float32(1.5))


def random_rays(count, seed):
    rng = np.random.default_rng(seed)
    rays = np.empty((count, 8), np.float32)
    rays[:, 0:3] = rng.uniform((-2.5, 0.25, -2.5), (2.5, 4.5, 2.5), (count, 3))
    d = rng.normal(size=(count, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3], rays[:, 7] = 1e-4, np.inf
    return rays


def test_basic_moves_equal_the_host_route(pair):
    _, scene_a, ra, scene_b, rb = pair
    start = assert_both_routes_agree(ra, scene_b, rb, "upload")
    assert len(start["bvh_triangles"]) == 2575 and not start["bvh_triangles"][-1].any()  # the sentinel behind the last triangle
    moved, normals = first_move(scene_a)
    deform_both(ra, scene_b, rb, 1, moved, normals)
    a = assert_both_routes_agree(ra, scene_b, rb, "full deformation, supplied normals")
    assert differ(a, start) == GEOMETRY and not a["bvh_triangles"][-1].any()
    assert ra.last_mesh_update_ms() > 0.0
    # a second, different deformation on the same contexts: no scratch leaks between calls
    again = M.second_deformation(moved)
    deform_both(ra, scene_b, rb, 1, again, np.ascontiguousarray(normals[::-1]))
    b = assert_both_routes_agree(ra, scene_b, rb, "second deformation")
    assert differ(b, a) == GEOMETRY
    # a partial range with kept normals
    lo, hi = M.PARTIAL
    part = np.ascontiguousarray(M.first_deformation(again)[lo:hi])
    deform_both(ra, scene_b, rb, 1, part, first=lo)
    c = assert_both_routes_agree(ra, scene_b, rb, "partial range, kept normals")
    assert differ(c, b) == GEOMETRY
    # recomputed normals, over a full range and then over the partial one (the normals of ALL vertices follow)
    deform_both(ra, scene_b, rb, 1, moved, recompute_normals=True)
    d = assert_both_routes_agree(ra, scene_b, rb, "recomputed normals")
    assert differ(d, c) == GEOMETRY
    want, _ = M.numpy_normals(moved, M.mesh_triangles(S.host_tables(scene_b), 1), normals)
    offset = int(S.host_tables(scene_b)["meshes"][1][0])
    assert np.array_equal(vertex_table(ra)[offset:offset + 642, 3:6], want.view(np.uint32))
    deform_both(ra, scene_b, rb, 1, part, first=lo, recompute_normals=True)
    e = assert_both_routes_agree(ra, scene_b, rb, "partial range, recomputed normals")
    assert differ(e, d) == GEOMETRY
    assert ra.last_mesh_update_ms() > 0.0


def test_the_card_quad_bent_and_moved_in_its_plane(pair):
    ids, scene_a, ra, scene_b, rb = pair
    mesh = ids["card_mesh"]

    def flat_packets(t):  # packets without extent on an axis: scale 0 there
        return int((t["nodes"].view(np.uint32)[:, [3, 10, 11]].view(np.float32) == 0.0).any(axis=1).sum())

    start = tables(ra)
    p, _ = scene_a.mesh_vertices(mesh)
    assert p.shape == (4, 3) and (p[:, 1] == 0).all()
    # in its plane: the packet of scale 0 survives and is among the bytes compared
    slid = np.ascontiguousarray(p * np.float32([1.5, 1.0, 0.75]) + np.float32([0.25, 0.0, -0.5]))
    deform_both(ra, scene_b, rb, mesh, slid)
    a = assert_both_routes_agree(ra, scene_b, rb, "in plane")
    assert differ(a, start) == GEOMETRY and flat_packets(a) == flat_packets(start) > 0
    # out of plane, with recomputed normals (a mesh of four vertices, valences 1 and 2): the node of the two triangles gains extent
    bent = slid.copy()
    bent[2, 1], bent[0, 1] = 0.375, -0.125
    deform_both(ra, scene_b, rb, mesh, bent, recompute_normals=True)
    b = assert_both_routes_agree(ra, scene_b, rb, "bent")
    assert differ(b, a) == GEOMETRY and flat_packets(b) == flat_packets(start) - 1
    # and flat again
    deform_both(ra, scene_b, rb, mesh, p, recompute_normals=True)
    c = assert_both_routes_agree(ra, scene_b, rb, "flat again")
    assert flat_packets(c) == flat_packets(start)
    for name in ("nodes", "bvh_triangles"):
        assert np.array_equal(c[name], start[name]), name


def test_device_pointers_equal_host_pointers(pair):
    torch = pytest.importorskip("torch")
    _, scene_a, ra, scene_b, rb = pair
    moved, normals = first_move(scene_a)
    rays = random_rays(1024, 2)
    before = ra.trace(rays).buffer.view(np.uint32).copy()
    rc = MegaPathRenderer(0)  # a third context: the same calls through host pointers
    try:
        rc.upload(scene_a)
        device_positions, device_normals = torch.from_numpy(moved).to("cuda:0"), torch.from_numpy(normals).to("cuda:0")
        ra.set_mesh_vertices(1, device_positions, device_normals)  # asynchronous: nothing waits for the kernels here ...
        after = ra.trace(rays).buffer.view(np.uint32)  # ... and the next query on the stream sees the deformation
        scene_b.set_mesh_vertices(1, moved, normals)
        rb.upload(scene_b, keep_film=True)
        assert np.array_equal(after, rb.trace(rays).buffer.view(np.uint32)) and not np.array_equal(after, before)
        assert_both_routes_agree(ra, scene_b, rb, "device pointers")
        assert ra.last_mesh_update_ms() > 0.0
        rc.set_mesh_vertices(1, moved, normals)
        assert_equal_tables(tables(ra), tables(rc), "device pointers against host pointers")
        assert np.array_equal(vertex_table(ra), vertex_table(rc))
        # a partial range and the recompute through device pointers (the tensor stays referenced until the stream has passed the call)
        lo, hi = M.PARTIAL
        part = np.ascontiguousarray(M.second_deformation(moved)[lo:hi])
        device_part = torch.from_numpy(part).to("cuda:0")
        ra.set_mesh_vertices(1, device_part, first=lo, recompute_normals=True)
        scene_b.set_mesh_vertices(1, part, first=lo, recompute_normals=True)
        rb.upload(scene_b, keep_film=True)
        assert_both_routes_agree(ra, scene_b, rb, "device pointers, partial range, recomputed normals")
        rc.set_mesh_vertices(1, part, first=lo, recompute_normals=True)
        assert_equal_tables(tables(ra), tables(rc), "device pointers against host pointers, partial range, recomputed normals")
        assert np.array_equal(vertex_table(ra), vertex_table(rc))
    finally:
        rc.close()
    for bad in ((device_positions.cpu(), None), (device_positions.double(), None), (device_positions, device_normals.cpu()),
                (device_positions, device_normals.double()), (device_positions[:, :2], None), (device_positions.reshape(-1), None),
                (device_positions, device_normals[:10]), (device_positions, normals), (device_positions.t()[:, :3], None)):
        with pytest.raises(ValueError):
            ra.set_mesh_vertices(1, *bad)
    assert_both_routes_agree(ra, scene_b, rb, "refused tensors change nothing")


def test_renders_and_queries_see_the_deformation(pair):
    """bit for bit against the host route, and different from before: the MegaPath film on both schedulers, ray queries, radiance queries,
    AOV buffers"""
    ids, scene_a, ra, scene_b, rb = pair
    moved, _ = first_move(scene_a)
    rays = random_rays(4096, 3)
    before = {"closest": ra.trace(rays).buffer.view(np.uint32).copy(), "any": ra.trace(rays, any_hit=True).copy(),
              "radiance": ra.radiance(rays[:1024], spp=1, raw=True).copy()}
    for pool in (False, True):  # the undeformed film of each scheduler
        ra.set_scheduler(pool=pool)
        ra.clear()
        ra.render(0, 4, sync=True)
        assert bool(ra.last_variant() & 4096) == pool
        before[pool] = ra.download(converted=False)
    start_tables = tables(ra)
    deform_both(ra, scene_b, rb, 1, moved, recompute_normals=True)
    assert differ(assert_both_routes_agree(ra, scene_b, rb, "MegaPath scene"), start_tables) == GEOMETRY
    for pool in (False, True):
        films = []
        for r in (ra, rb):
            r.set_scheduler(pool=pool)
            r.clear()
            r.render(0, 4, sync=True)
            films.append(r.download(converted=False))
            assert bool(r.last_variant() & 4096) == pool
        assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32)), pool
        assert (films[0][..., 3] == 4).all() and films[0][..., :3].sum() > 0
        assert not np.array_equal(films[0], before[pool]), pool
    closest = ra.trace(rays)
    assert np.array_equal(closest.buffer.view(np.uint32), rb.trace(rays).buffer.view(np.uint32))
    assert not np.array_equal(closest.buffer.view(np.uint32), before["closest"])
    any_hit = ra.trace(rays, any_hit=True)
    assert np.array_equal(any_hit, rb.trace(rays, any_hit=True)) and not np.array_equal(any_hit, before["any"])
    assert np.isin(closest.inst, [ids["ball_a"], ids["ball_b"]]).sum() > 100  # the deformed instances are among what the rays see
    radiance = [r.radiance(rays[:1024], spp=1, raw=True) for r in (ra, rb)]
    assert np.array_equal(radiance[0].view(np.uint32), radiance[1].view(np.uint32)) and radiance[0][:, :3].sum() > 0
    assert not np.array_equal(radiance[0], before["radiance"])
    # the AOV variant of the scene: the normal and depth buffers
    aov_a, aov_b = M.room(aov=True), M.room(aov=True)
    ra.upload(aov_a)
    ra.render(0, 8, sync=True)
    start = {c: ra.download_aov(c, normalized=False) for c in ("normal", "depth")}
    ra.upload(aov_a)
    rb.upload(aov_b)
    start_tables = assert_both_routes_agree(ra, aov_b, rb, "AOV scene, upload")
    deform_both(ra, aov_b, rb, 1, moved, recompute_normals=True)
    assert differ(assert_both_routes_agree(ra, aov_b, rb, "AOV scene"), start_tables) == GEOMETRY
    for r in (ra, rb):
        r.render(0, 8, sync=True)
    for c in ("normal", "depth"):
        got = ra.download_aov(c, normalized=False)
        assert np.array_equal(got.view(np.uint32), rb.download_aov(c, normalized=False).view(np.uint32)), c
        assert np.abs(start[c]).sum() > 0 and not np.array_equal(got, start[c])


@pytest.mark.parametrize("deform_first", [True, False])
def test_with_instance_transforms_in_both_orders(pair, deform_first):
    ids, scene_a, ra, scene_b, rb = pair
    moved, normals = first_move(scene_a)
    which = np.array([ids["ball_b"]])
    matrix = S.srt(scale=(0.75, 0.4, 0.6), axis=(0, 1, 1), degrees=-110.0, translate=(1.0, 0.75, 1.25))[None]

    def deform():
        deform_both(ra, scene_b, rb, 1, moved, normals)

    def move():
        ra.set_instance_transforms(matrix, which)
        scene_b.set_instance_transforms(matrix, which)
        rb.upload(scene_b, keep_film=True)

    start = tables(ra)
    for step in ((deform, move) if deform_first else (move, deform)):
        step()
        assert_both_routes_agree(ra, scene_b, rb, (deform_first, step.__name__))
    assert differ(tables(ra), start) == list(TABLES)


def test_film_and_counters_carry_on(pair):
    _, scene_a, ra, scene_b, rb = pair
    for r in (ra, rb):
        r.render(0, 3, counters=True, sync=True)
    paths = ra.counters()["paths"]
    assert paths == 32 * 32 * 3
    start_tables = tables(ra)
    deform_both(ra, scene_b, rb, 1, first_move(scene_a)[0], recompute_normals=True)
    assert differ(assert_both_routes_agree(ra, scene_b, rb, "between the two ranges"), start_tables) == GEOMETRY
    assert ra.counters()["paths"] == paths  # the deformation resets no counter ...
    for r in (ra, rb):
        r.render(3, 8, counters=True, sync=True)
    film = ra.download(converted=False)
    assert (film[..., 3] == 8).all()  # ... and the film accumulates over both ranges
    assert np.array_equal(film.view(np.uint32), rb.download(converted=False).view(np.uint32))
    ca, cb = ra.counters(), rb.counters()
    assert ca["paths"] == 32 * 32 * 8 and all(ca[k] == cb[k] for k in ("paths", "closest_rays", "shadow_rays", "nodes_visited", "tris_tested", "surface_hits"))


def test_update_scene_restores_the_host_tables_vertices_included(pair):
    ids, scene_a, ra, scene_b, rb = pair
    start, start_vertices = tables(ra), vertex_table(ra)
    assert np.array_equal(start_vertices, S.host_tables(scene_a)["vertices"])
    ra.set_mesh_vertices(1, first_move(scene_a)[0], recompute_normals=True)
    assert differ(tables(ra), start) == GEOMETRY and not np.array_equal(vertex_table(ra), start_vertices)
    ra.upload(scene_a, keep_film=True)  # lrhip_update_scene: the host's tables win again, the fp32 boxes and the vertices included
    assert_equal_tables(tables(ra), start, "restored")
    assert np.array_equal(vertex_table(ra), start_vertices)
    # a device move of an instance of the mesh re-bakes from the restored vertices: it equals the host route over the undeformed mesh
    which = np.array([ids["ball_a"]])
    matrix = S.srt(scale=(0.5, 1.0, 0.75), axis=(1, 2, 3), degrees=40.0, translate=(-0.5, 1.5, 0.5))[None]
    ra.set_instance_transforms(matrix, which)
    scene_b.set_instance_transforms(matrix, which)
    rb.upload(scene_b, keep_film=True)
    assert_both_routes_agree(ra, scene_b, rb, "an instance move after the restore")


def test_errors(pair):
    torch = pytest.importorskip("torch")
    ids, scene_a, ra, scene_b, rb = pair
    lib = ra._lib
    moved, normals = first_move(scene_a)

    def call(ctx, mesh, first, count, positions=None, normal_ptr=None, flags=0):
        p = _ffi.MeshUpdateParams(positions, normal_ptr, mesh, first, count, flags)
        rc = lib.lrhip_set_mesh_vertices(ctx, C.byref(p))
        return rc, lib.lrhip_last_error().decode()

    fresh = MegaPathRenderer(0)
    try:  # before any upload
        rc, message = call(fresh._ctx, 1, 0, 642, moved.ctypes.data)
        assert rc == LRHIP_ERROR_INVALID and "no scene" in message
        with pytest.raises(DeviceError):
            fresh.set_mesh_vertices(1, moved)
        assert lib.lrhip_read_scene_table(fresh._ctx, _ffi.TABLE_VERTICES, 0, 0, None) == LRHIP_ERROR_INVALID
        assert fresh.last_mesh_update_ms() == 0.0
    finally:
        fresh.close()
    start, start_vertices = tables(ra), vertex_table(ra)
    quad, _ = scene_a.mesh_vertices(ids["lamp_mesh"])
    rc, message = call(ra._ctx, ids["lamp_mesh"], 0, 4, quad.ctypes.data)
    assert rc == LRHIP_ERROR_UNSUPPORTED and "light" in message and "emitter" in message  # the emitter: its alias table is not rebuilt
    with pytest.raises(DeviceError, match="emitter"):
        ra.set_mesh_vertices(ids["lamp_mesh"], quad)
    nan = moved.copy()
    nan[641, 2] = np.nan
    for args, text in (((1, 1, 642, moved.ctypes.data), "not inside"), ((1, 643, 0, moved.ctypes.data), "not inside"),
                       ((int(scene_a.view().mesh_count), 0, 1, moved.ctypes.data), "out of range"),
                       ((1, 0, 642, nan.ctypes.data), "non-finite"), ((1, 0, 642, moved.ctypes.data, nan.ctypes.data), "non-finite"),
                       ((1, 0, 642, None), "NULL"), ((1, 0, 642, moved.ctypes.data, None, 64), "unknown flags"),
                       ((1, 0, 642, moved.ctypes.data, None, 4), "unknown flags"),
                       ((1, 0, 642, moved.ctypes.data, normals.ctypes.data, _ffi.MESH_RECOMPUTE_NORMALS), "NULL with")):
        rc, message = call(ra._ctx, *args)
        assert rc == LRHIP_ERROR_INVALID and text in message, (args[:3], rc, message)
    device_positions = torch.from_numpy(np.concatenate([moved, moved[:1]])).to("cuda:0")
    torch.cuda.synchronize()
    for position_ptr, normal_ptr in ((device_positions.data_ptr() + 2, None), (device_positions.data_ptr(), device_positions.data_ptr() + 1)):
        rc, message = call(ra._ctx, 1, 0, 642, position_ptr, normal_ptr, _ffi.RAY_DEVICE_POINTERS)
        assert rc == LRHIP_ERROR_INVALID and "aligned" in message
    rc, message = call(ra._ctx, 1, 600, 43, device_positions.data_ptr(), None, _ffi.RAY_DEVICE_POINTERS)  # scalars are checked on the host
    assert rc == LRHIP_ERROR_INVALID and "not inside" in message
    # nothing to do is legal and launches nothing
    assert call(ra._ctx, 1, 0, 0)[0] == 0 and call(ra._ctx, 1, 642, 0, None, None, _ffi.MESH_RECOMPUTE_NORMALS | _ffi.RAY_DEVICE_POINTERS)[0] == 0
    assert ra.last_mesh_update_ms() == 0.0
    # the vertex table through the test hook: 32-byte records; a range past the end and the ids between the tables are invalid
    size = int(lib.lrhip_scene_table_bytes(ra._ctx, _ffi.TABLE_VERTICES))
    assert size == int(scene_a.view().vertex_count) * 32
    assert lib.lrhip_read_scene_table(ra._ctx, _ffi.TABLE_VERTICES, size - 16, 32, (C.c_uint8 * 32)()) == LRHIP_ERROR_INVALID
    assert lib.lrhip_read_scene_table(ra._ctx, _ffi.TABLE_VERTICES, size - 32, 32, (C.c_uint8 * 32)()) == 0
    for which in (4, 5, 6, 7, 9):
        assert lib.lrhip_read_scene_table(ra._ctx, which, 0, 0, None) == LRHIP_ERROR_INVALID and lib.lrhip_scene_table_bytes(ra._ctx, which) == 0
    assert_equal_tables(tables(ra), start, "refused calls change nothing")
    assert np.array_equal(vertex_table(ra), start_vertices)
    # a device-pointer call whose positions hold a NaN: non-finite tables, but no fault and no endless loop -- the context goes on working
    poisoned = torch.from_numpy(nan).to("cuda:0")
    ra.set_mesh_vertices(1, poisoned, recompute_normals=True)
    assert not np.isfinite(ra.scene_table(_ffi.TABLE_BVH_TRIANGLES).view(np.float32)[:-1, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).all()
    deform_both(ra, scene_b, rb, 1, moved, normals)
    assert_both_routes_agree(ra, scene_b, rb, "a deformation after the non-finite one")
