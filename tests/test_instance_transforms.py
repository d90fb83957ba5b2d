"""Moving instances by matrices the caller holds, the part that needs no device: the host mirror lrhost_scene_set_instance_transforms
(the yardstick of tests/test_gpu_instance_transforms.py) against a bake in numpy float32, its agreement with the build-time bake and with
set_time, the argument rules, and the new symbols of liblrhip.so."""
import ctypes as C
import os

import numpy as np
import pytest

import instance_scene as S
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import check_instance_transforms


def test_host_bake_matches_numpy_and_the_tree_holds_it():
    sc = Scene.from_string(S.TWO_BALLS)
    before = S.host_tables(sc)
    balls = S.instances_of_mesh(before, 80)
    assert len(balls) == 2 and len(before["instances"]) == 4 and len(before["meshes"]) == 3  # two instances of ONE mesh
    a, b = balls
    move = S.srt(scale=(1.5, 0.5, 0.75), axis=(1, 2, 3), degrees=40.0, translate=(0.25, 1.5, -0.5))
    sc.set_instance_transforms(move[None], np.array([a]))
    after = S.host_tables(sc)
    # the matrix is in the instance record, and nothing else of the records moved
    want = before["instances"].copy()
    want[a, 4:20] = move.reshape(16).view(np.uint32)
    assert np.array_equal(after["instances"], want)
    # every triangle of the moved instance is the numpy bake, bit for bit; the others did not change
    inst = after["bvh_triangles"][:, 3]
    bake = S.numpy_bake(after, S.instance_matrices(sc))
    assert (inst == a).sum() == 80
    assert np.array_equal(S.baked(after)[inst == a].view(np.uint32), bake[inst == a].view(np.uint32))
    assert np.array_equal(after["bvh_triangles"][inst != a], before["bvh_triangles"][inst != a])
    assert not np.array_equal(after["bvh_triangles"][inst == a], before["bvh_triangles"][inst == a])
    assert np.array_equal(after["bvh_triangles"][:, [3, 7, 11]], before["bvh_triangles"][:, [3, 7, 11]])  # inst, prim, flags
    assert np.array_equal(after["bvh_nodes"][:, 24:], before["bvh_nodes"][:, 24:])  # the topology is the build's
    S.check_tree(after)
    # a second move, both balls at once in a permuted order: no state of the first call is left
    moves = np.stack([S.srt(scale=(0.5, 0.5, 2.0), axis=(0, 1, 0), degrees=-75.0, translate=(1.0, 0.75, 1.0)),
                      S.srt(scale=(1.25, 1.0, 0.5), axis=(1, 0, 0), degrees=15.0, translate=(-2.0, 1.0, 0.5))])
    sc.set_instance_transforms(moves.reshape(2, 16), np.array([b, a], np.int64))
    again = S.host_tables(sc)
    inst = again["bvh_triangles"][:, 3]
    moved = (inst == a) | (inst == b)
    assert np.array_equal(S.instance_matrices(sc)[[b, a]], moves)
    assert np.array_equal(S.baked(again).view(np.uint32)[moved], S.numpy_bake(again, S.instance_matrices(sc)).view(np.uint32)[moved])
    assert np.array_equal(again["bvh_triangles"][~moved], before["bvh_triangles"][~moved])
    S.check_tree(again)


@pytest.mark.parametrize("source", [S.TWO_BALLS, S.LERP_BALLS])
def test_identity_write_back_changes_no_byte(source):
    """the build-time bake and tree and the refit agree: writing back the matrices the scene holds is a no-op on every table"""
    sc = Scene.from_string(source)
    before = S.host_tables(sc)
    sc.set_instance_transforms(S.instance_matrices(sc))
    after = S.host_tables(sc)
    for name in ("instances", "bvh_triangles", "bvh_nodes"):
        assert np.array_equal(before[name], after[name]), name
    ids = np.arange(len(before["instances"]))[::-1].copy()
    sc.set_instance_transforms(S.instance_matrices(sc)[ids], ids)
    after = S.host_tables(sc)
    for name in ("instances", "bvh_triangles", "bvh_nodes"):
        assert np.array_equal(before[name], after[name]), name


@pytest.mark.parametrize("time", [0.25, 1.0])
def test_agrees_with_set_time(time):
    """the matrices set_time produces, applied through set_instance_transforms to the same description, give the same tables"""
    timed = Scene.from_string(S.LERP_BALLS)
    assert timed.set_time(time)
    want = S.host_tables(timed)
    sc = Scene.from_string(S.LERP_BALLS)
    start = S.host_tables(sc)
    assert not np.array_equal(start["bvh_triangles"], want["bvh_triangles"])
    changed = [i for i in range(len(start["instances"])) if not np.array_equal(start["instances"][i], want["instances"][i])]
    assert len(changed) == 1
    sc.set_instance_transforms(S.instance_matrices(timed)[changed], np.array(changed))
    got = S.host_tables(sc)
    for name in ("instances", "bvh_triangles", "bvh_nodes"):
        assert np.array_equal(got[name], want[name]), name
    # set_time keeps its behaviour afterwards: the animated instance goes back to its transform's value
    sc.set_time(0.0)
    assert np.array_equal(S.host_tables(sc)["bvh_triangles"], start["bvh_triangles"])


def test_argument_checks():
    sc = Scene.from_string(S.TWO_BALLS)
    before = S.host_tables(sc)
    good = S.instance_matrices(sc)
    n = len(good)
    assert check_instance_transforms(good, None, n) == "numpy" and check_instance_transforms(good.reshape(n, 16), np.arange(n), n) == "numpy"
    assert check_instance_transforms(good[:0], None, n) == "numpy" and check_instance_transforms(good[:2], np.array([3, 1], np.uint32), n) == "numpy"
    nan, inf = good.copy(), good.copy()
    nan[1, 2, 1] = np.nan
    inf[0, 3, 0] = np.inf
    bad = [(good.astype(np.float64), None), (good.reshape(n, 2, 8), None), (good.reshape(-1), None), (good[:, :3], None), (good[:, :, ::-1], None),
           (good.tolist(), None), (nan, None), (inf, None),
           (good, np.arange(n - 1)), (good, np.arange(n, dtype=np.float32)), (good, list(range(n))), (good[:2], np.array([0, n])),
           (good[:2], np.array([-1, 0])), (good[:2], np.array([1, 1])), (good[:2], np.array([[0, 1]])),
           (np.concatenate([good, good[:1]]), None)]
    for matrices, ids in bad:
        with pytest.raises(ValueError):
            check_instance_transforms(matrices, ids, n)
        with pytest.raises(ValueError):
            sc.set_instance_transforms(matrices, ids)
    # the host call itself validates like the device call, and a refused call changes nothing
    lib = _ffi.host_lib()
    ids = (C.c_uint32 * 2)
    for count, id_list, matrices in ((2, ids(0, n), good), (2, ids(2, 2), good), (1, None, nan[1:]), (1, ids(1, 0), inf), (n + 1, None, np.concatenate([good, good[:1]])),
                                     (1, None, None)):
        rc = lib.lrhost_scene_set_instance_transforms(sc._handle, count, id_list, matrices.ctypes.data if matrices is not None else None)
        assert rc != 0 and lib.lrhost_last_error(), (count, id_list)
    assert lib.lrhost_scene_set_instance_transforms(sc._handle, 0, None, None) == 0  # nothing to do is legal
    sc._views.clear()
    after = S.host_tables(sc)
    for name in ("instances", "bvh_triangles", "bvh_nodes"):
        assert np.array_equal(before[name], after[name]), name


def test_new_symbols_exist_and_refuse_a_null_context():
    """needs no device: the entry points are in liblrhip.so and bound in _ffi, and a NULL context is LRHIP_ERROR_INVALID"""
    path = os.path.join(_ffi.LIB_DIR, "liblrhip.so")
    raw = C.CDLL(path)
    for name in ("lrhip_set_instance_transforms", "lrhip_last_instance_update_ms", "lrhip_read_scene_table", "lrhip_scene_table_bytes"):
        assert hasattr(raw, name), name
    lib = _ffi.hip_lib()
    p = _ffi.InstanceUpdateParams()
    assert C.sizeof(p) == 32 == _ffi.host_lib().lrhost_sizeof(b"lrhip_instance_update_params")
    assert lib.lrhip_set_instance_transforms(None, C.byref(p)) == -1 and b"NULL" in lib.lrhip_last_error()
    assert lib.lrhip_last_instance_update_ms(None) == 0.0
    out = (C.c_uint8 * 16)()
    assert lib.lrhip_read_scene_table(None, _ffi.TABLE_NODES, 0, 16, out) == -1
    assert lib.lrhip_scene_table_bytes(None, _ffi.TABLE_INSTANCES) == 0
    assert hasattr(_ffi.host_lib(), "lrhost_scene_set_instance_transforms")
