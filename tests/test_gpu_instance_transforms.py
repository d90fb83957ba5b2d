"""Moving instances on the device (lrhip_set_instance_transforms).  The yardstick is the host: context A takes the new call, context
B takes Scene.set_instance_transforms (re-bake and refit on the CPU, tests/test_instance_transforms.py) + upload(keep_film=True), i.e. the
unchanged lrhip_update_scene -- and the four device tables that move with the geometry must come out EQUAL BYTE FOR BYTE, as must everything
rendered or queried from them."""
import ctypes as C

import numpy as np
import pytest

import instance_scene as S
from luisarender_amd import _ffi
from luisarender_amd.render import DeviceError, MegaPathRenderer

pytestmark = pytest.mark.gpu

LRHIP_ERROR_INVALID = -1
TABLES = {"nodes": _ffi.TABLE_NODES, "bvh_triangles": _ffi.TABLE_BVH_TRIANGLES, "instances": _ffi.TABLE_INSTANCES, "shade_triangles": _ffi.TABLE_SHADE_TRIANGLES}


def tables(renderer) -> dict:
    return {name: renderer.scene_table(which) for name, which in TABLES.items()}


def assert_equal_tables(a: dict, b: dict, what="") -> None:
    for name in TABLES:
        assert a[name].shape == b[name].shape, (what, name)
        rows = np.nonzero((a[name] != b[name]).any(axis=1))[0]
        assert rows.size == 0, (what, name, rows[:8], a[name][rows[:1]].view(np.uint32), b[name][rows[:1]].view(np.uint32))


def differ(a: dict, b: dict) -> list:
    return [name for name in TABLES if not np.array_equal(a[name], b[name])]


@pytest.fixture
def pair():
    """(ids, scene A, context A, scene B, context B): two uploads of the fixture scene, checked on the CPU first"""
    scene_a, scene_b = S.room(), S.room()
    ids = S.check_room(scene_a)
    ra, rb = MegaPathRenderer(0), MegaPathRenderer(0)
    ra.upload(scene_a)
    rb.upload(scene_b)
    yield ids, scene_a, ra, scene_b, rb
    ra.close()
    rb.close()


def first_move(ids):
    """a mesh instance by rotation x non-uniform scale x translation, the emitter and the flat quad by translations"""
    return (np.array([ids["ball_a"], ids["lamp"], ids["card"]]),
            np.stack([S.srt(scale=(0.5, 1.0, 0.75), axis=(1, 2, 3), degrees=40.0, translate=(-0.5, 1.5, 0.5)),
                      S.srt(translate=(0.5, -0.25, 0.25)), S.srt(translate=(-0.75, 0.5, 1.5))]))


def second_move(ids):
    return (np.array([ids["card"], ids["ball_b"]]),
            np.stack([S.srt(translate=(1.0, 2.5, 0.0)), S.srt(scale=(0.75, 0.4, 0.6), axis=(0, 1, 1), degrees=-110.0, translate=(1.0, 0.75, 1.25))]))


def move_both(ra, scene_b, rb, which, matrices):
    ra.set_instance_transforms(matrices, which)
    scene_b.set_instance_transforms(matrices, which)
    rb.upload(scene_b, keep_film=True)


def test_the_four_tables_equal_the_host_route(pair):
    ids, _, ra, scene_b, rb = pair
    start = tables(ra)
    assert_equal_tables(start, tables(rb), "upload")
    assert len(start["bvh_triangles"]) == 655 and not start["bvh_triangles"][-1].any()  # the sentinel behind the last triangle
    move_both(ra, scene_b, rb, *first_move(ids))
    a = tables(ra)
    assert_equal_tables(a, tables(rb), "first move")
    assert differ(a, start) == list(TABLES) and not a["bvh_triangles"][-1].any()
    assert ra.last_instance_update_ms() > 0.0
    # packets of zero extent on an axis (scale 0) are among what was compared: the moved flat quad keeps one
    nodes = a["nodes"].view(np.uint32)
    assert (nodes[:, [3, 10, 11]].view(np.float32) == 0.0).any()
    # a second, different move on the same contexts: no state leaks between calls
    move_both(ra, scene_b, rb, *second_move(ids))
    again = tables(ra)
    assert_equal_tables(again, tables(rb), "second move")
    assert differ(again, a) == list(TABLES)


def test_identity_write_back_of_the_full_table(pair):
    _, scene_a, ra, _, rb = pair
    ra.set_instance_transforms(S.instance_matrices(scene_a))
    assert_equal_tables(tables(ra), tables(rb), "identity")


def test_a_list_of_ids_equals_the_full_table(pair):
    ids, scene_a, ra, _, rb = pair
    which, matrices = first_move(ids)
    full = S.instance_matrices(scene_a)
    full[which] = matrices
    ra.set_instance_transforms(matrices, which)
    rb.set_instance_transforms(full)
    want = tables(rb)
    assert_equal_tables(tables(ra), want, "ids against the full table")
    # a permuted list, over tables that already moved once
    rc = MegaPathRenderer(0)
    try:
        rc.upload(scene_a)
        rc.set_instance_transforms(np.ascontiguousarray(matrices[[2, 0, 1]]), which[[2, 0, 1]])
        assert_equal_tables(tables(rc), want, "permuted ids")
    finally:
        rc.close()


def random_rays(count, seed):
    rng = np.random.default_rng(seed)
    rays = np.empty((count, 8), np.float32)
    rays[:, 0:3] = rng.uniform((-2.5, 0.25, -2.5), (2.5, 4.5, 2.5), (count, 3))
    d = rng.normal(size=(count, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3], rays[:, 7] = 1e-4, np.inf
    return rays


def test_device_pointers_equal_host_pointers(pair):
    torch = pytest.importorskip("torch")
    ids, _, ra, _, rb = pair
    which, matrices = first_move(ids)
    rays = random_rays(1024, 2)
    before = ra.trace(rays).buffer.view(np.uint32).copy()
    device_matrices = torch.from_numpy(matrices).to("cuda:0")
    device_ids = torch.from_numpy(which.astype(np.int32)).to("cuda:0")
    ra.set_instance_transforms(device_matrices, device_ids)  # asynchronous: nothing waits for the kernels here ...
    moved = ra.trace(rays).buffer.view(np.uint32)  # ... and the next query on the stream sees the move
    rb.set_instance_transforms(matrices, which)
    assert np.array_equal(moved, rb.trace(rays).buffer.view(np.uint32)) and not np.array_equal(moved, before)
    assert_equal_tables(tables(ra), tables(rb), "device pointers")
    assert ra.last_instance_update_ms() > 0.0
    for bad in ((device_matrices.cpu(), device_ids), (device_matrices.double(), device_ids), (device_matrices, device_ids.long()),
                (device_matrices, device_ids.cpu()), (device_matrices[:, :3], device_ids), (device_matrices, which)):
        with pytest.raises(ValueError):
            ra.set_instance_transforms(*bad)


def test_renders_and_queries_see_the_move(pair):
    """bit for bit against the host route: the MegaPath film on both schedulers, ray queries, radiance queries, AOV buffers"""
    ids, _, ra, scene_b, rb = pair
    move_both(ra, scene_b, rb, *first_move(ids))
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
    rays = random_rays(4096, 3)
    assert np.array_equal(ra.trace(rays).buffer.view(np.uint32), rb.trace(rays).buffer.view(np.uint32))
    assert np.array_equal(ra.trace(rays, any_hit=True), rb.trace(rays, any_hit=True))
    hit_moved = np.isin(ra.trace(rays).inst, [ids["ball_a"], ids["card"], ids["lamp"]])
    assert hit_moved.sum() > 100  # the moved instances are among what the rays see
    radiance = [r.radiance(rays[:1024], spp=1, raw=True) for r in (ra, rb)]
    assert np.array_equal(radiance[0].view(np.uint32), radiance[1].view(np.uint32)) and radiance[0][:, :3].sum() > 0
    # one AOV scene: the normal and depth buffers
    aov_a, aov_b = S.room(aov=True), S.room(aov=True)
    ra.upload(aov_a)
    rb.upload(aov_b)
    start = {c: ra.download_aov(c, normalized=False) for c in ("normal", "depth")}
    move_both(ra, aov_b, rb, *first_move(ids))
    for r in (ra, rb):
        r.render(0, 8, sync=True)
    for c in ("normal", "depth"):
        got = ra.download_aov(c, normalized=False)
        assert np.array_equal(got.view(np.uint32), rb.download_aov(c, normalized=False).view(np.uint32)), c
        assert not np.array_equal(got, start[c])


def test_lerp_scene_follows_the_host_at_two_times():
    """the matrices the host view shows after set_time(t), applied by the new call to a context uploaded at the shutter's opening, against a
    context that took lrhip_update_scene at t"""
    scene_a, scene_b = S.room(lerp=True), S.room(lerp=True)
    ids = S.check_room(scene_a)
    ra, rb = MegaPathRenderer(0), MegaPathRenderer(0)
    try:
        ra.upload(scene_a)
        rb.upload(scene_b)
        for k, time in enumerate((0.375, 1.0)):
            assert scene_b.set_time(time)
            rb.upload(scene_b, keep_film=True)
            ra.set_instance_transforms(S.instance_matrices(scene_b)[[ids["ball_a"]]], np.array([ids["ball_a"]]))
            assert_equal_tables(tables(ra), tables(rb), time)
            for r in (ra, rb):
                r.render(4 * k, 4 * k + 4, sync=True)
            assert np.array_equal(ra.download(converted=False).view(np.uint32), rb.download(converted=False).view(np.uint32)), time
    finally:
        ra.close()
        rb.close()


def test_film_and_counters_carry_on(pair):
    ids, _, ra, scene_b, rb = pair
    for r in (ra, rb):
        r.render(0, 3, counters=True, sync=True)
    paths = ra.counters()["paths"]
    assert paths == 32 * 32 * 3
    move_both(ra, scene_b, rb, *first_move(ids))
    assert ra.counters()["paths"] == paths  # the move resets no counter ...
    for r in (ra, rb):
        r.render(3, 8, counters=True, sync=True)
    film = ra.download(converted=False)
    assert (film[..., 3] == 8).all()  # ... and the film accumulates over both ranges
    assert np.array_equal(film.view(np.uint32), rb.download(converted=False).view(np.uint32))
    ca, cb = ra.counters(), rb.counters()
    assert ca["paths"] == 32 * 32 * 8 and all(ca[k] == cb[k] for k in ("paths", "closest_rays", "shadow_rays", "nodes_visited", "tris_tested", "surface_hits"))


def test_update_scene_restores_the_host_tables_and_a_move_works_again(pair):
    ids, scene_a, ra, scene_b, rb = pair
    start = tables(ra)
    ra.set_instance_transforms(*first_move(ids)[::-1])
    assert differ(tables(ra), start) == list(TABLES)
    ra.upload(scene_a, keep_film=True)  # lrhip_update_scene: the host's tables win again, the fp32 boxes included
    assert_equal_tables(tables(ra), start, "restored")
    move_both(ra, scene_b, rb, *second_move(ids))
    assert_equal_tables(tables(ra), tables(rb), "a move after the restore")


def test_errors(pair):
    torch = pytest.importorskip("torch")
    ids, scene_a, ra, _, rb = pair
    lib = ra._lib
    which, matrices = first_move(ids)
    which = which.astype(np.uint32)

    def call(ctx, matrix_ptr, id_ptr, count, flags=0):
        p = _ffi.InstanceUpdateParams(matrix_ptr, id_ptr, count, flags)
        rc = lib.lrhip_set_instance_transforms(ctx, C.byref(p))
        return rc, lib.lrhip_last_error().decode()

    fresh = MegaPathRenderer(0)
    try:  # before any upload
        rc, message = call(fresh._ctx, matrices.ctypes.data, which.ctypes.data, 3)
        assert rc == LRHIP_ERROR_INVALID and "no scene" in message
        with pytest.raises(DeviceError):
            fresh.set_instance_transforms(matrices, which)
        assert lib.lrhip_read_scene_table(fresh._ctx, 0, 0, 0, None) == LRHIP_ERROR_INVALID
    finally:
        fresh.close()
    start = tables(ra)
    out_of_range, twice, nan = which.copy(), which.copy(), matrices.copy()
    out_of_range[1], twice[2], nan[1, 3, 2] = 5, twice[0], np.nan
    for (m, i, count), text in (((matrices, out_of_range, 3), "out of range"), ((matrices, twice, 3), "twice"), ((nan, which, 3), "non-finite"),
                                ((S.instance_matrices(scene_a), None, 6), "without ids")):
        rc, message = call(ra._ctx, m.ctypes.data, i.ctypes.data if i is not None else None, count)
        assert rc == LRHIP_ERROR_INVALID and text in message, (rc, message)
    assert call(ra._ctx, None, None, 1)[0] == LRHIP_ERROR_INVALID and call(ra._ctx, matrices.ctypes.data, None, 1, 64)[0] == LRHIP_ERROR_INVALID
    assert call(ra._ctx, None, None, 0)[0] == 0  # nothing to do is legal
    device_matrices = torch.from_numpy(np.concatenate([matrices, matrices[:1]])).to("cuda:0")
    device_ids = torch.tensor([int(which[0]), 9999, int(which[1]), int(which[2])], dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for matrix_ptr, id_ptr in ((device_matrices.data_ptr() + 4, device_ids.data_ptr()), (device_matrices.data_ptr(), device_ids.data_ptr() + 2)):
        rc, message = call(ra._ctx, matrix_ptr, id_ptr, 2, _ffi.RAY_DEVICE_POINTERS)
        assert rc == LRHIP_ERROR_INVALID and "aligned" in message
    size = int(lib.lrhip_scene_table_bytes(ra._ctx, _ffi.TABLE_INSTANCES))
    assert size == 5 * 128 and lib.lrhip_read_scene_table(ra._ctx, _ffi.TABLE_INSTANCES, size - 64, 128, (C.c_uint8 * 128)()) == LRHIP_ERROR_INVALID
    assert lib.lrhip_read_scene_table(ra._ctx, 4, 0, 0, None) == LRHIP_ERROR_INVALID
    unknown = max(_ffi.TABLE_RECORD_BYTES) + 1  # the first number behind the last table (18: the exact-arithmetic light triangles)
    assert unknown == 19 and lib.lrhip_read_scene_table(ra._ctx, unknown, 0, 0, None) == LRHIP_ERROR_INVALID and lib.lrhip_scene_table_bytes(ra._ctx, unknown) == 0
    assert_equal_tables(tables(ra), start, "refused calls change nothing")
    # a device-pointer list with one id out of range: that entry is left out, the others are applied
    skipped = torch.from_numpy(np.stack([matrices[0], S.srt(translate=(9, 9, 9)), matrices[1], matrices[2]])).to("cuda:0")
    ra.set_instance_transforms(skipped, device_ids)
    rb.set_instance_transforms(matrices, which)
    assert_equal_tables(tables(ra), tables(rb), "an id out of range is skipped")
