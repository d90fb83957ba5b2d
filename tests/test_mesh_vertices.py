"""Deforming a mesh, the part that needs no device: the host mirror lrhost_scene_set_mesh_vertices (the yardstick of
tests/test_gpu_mesh_vertices.py) against numpy float32 -- the vertex table, the re-bake of every instance of the mesh, the normal recompute
by its definition --, its agreement with the build-time tables and with set_time, the refusals, the argument rules, the ctypes mirror
against a C translation unit of the header, and the new symbols of liblrhip.so."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import instance_scene as S
import mesh_deform_scene as M
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import check_mesh_vertices
from luisarender_amd.scene import HostError

LRHIP_ERROR_INVALID = -1
MOVING = ("vertices", "bvh_triangles", "bvh_nodes")
FIELDS = ("positions", "normals", "mesh", "first_vertex", "count", "flags")


def assert_same(a: dict, b: dict, names=("vertices", "triangles", "meshes", "instances", "bvh_triangles", "bvh_nodes")) -> None:
    for name in names:
        assert np.array_equal(a[name], b[name]), name


def test_fixture_is_what_it_is_for():
    ids = M.check_room(M.room())
    assert ids["ball_mesh"] == 1 and len({ids["ball_mesh"], ids["card_mesh"], ids["lamp_mesh"]}) == 3
    lerp = M.room(lerp=True)
    assert M.check_room(lerp)["ball_a"] == ids["ball_a"]
    assert lerp.instance_mesh(ids["ball_a"]) == lerp.instance_mesh(ids["ball_b"]) == 1 and lerp.instance_mesh(ids["card"]) == ids["card_mesh"]
    with pytest.raises(ValueError):
        lerp.instance_mesh(5)


def test_vertices_and_the_bake_of_both_instances_match_numpy():
    sc = M.room()
    ids = M.check_room(sc)
    before = S.host_tables(sc)
    p, n = sc.mesh_vertices(1)
    assert p.shape == n.shape == (642, 3) and p.dtype == n.dtype == np.float32
    assert np.array_equal(np.concatenate([p, n], axis=1).view(np.uint32), M.vertex_words(sc, 1)[:, 0:6])
    moved, normals = M.first_deformation(p), np.ascontiguousarray(n[:, [1, 2, 0]] * np.float32(1.5))  # written as given: not unit length
    assert not np.array_equal(moved, p)
    sc.set_mesh_vertices(1, moved, normals)
    after = S.host_tables(sc)
    # the vertex table holds the inputs; u v and every other mesh's vertices stay
    want = before["vertices"].copy()
    offset = int(before["meshes"][1][0])
    want[offset:offset + 642, 0:3], want[offset:offset + 642, 3:6] = moved.view(np.uint32), normals.view(np.uint32)
    assert np.array_equal(after["vertices"], want)
    got_p, got_n = sc.mesh_vertices(1)
    assert np.array_equal(got_p.view(np.uint32), moved.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), normals.view(np.uint32))
    # every triangle of BOTH instances is the numpy bake over the new vertices, bit for bit; the others did not change
    inst = after["bvh_triangles"][:, 3]
    of_mesh = np.isin(inst, [ids["ball_a"], ids["ball_b"]])
    assert of_mesh.sum() == 2560
    bake = S.numpy_bake(after, S.instance_matrices(sc))
    assert np.array_equal(S.baked(after)[of_mesh].view(np.uint32), bake[of_mesh].view(np.uint32))
    assert np.array_equal(after["bvh_triangles"][~of_mesh], before["bvh_triangles"][~of_mesh])
    for i in (ids["ball_a"], ids["ball_b"]):
        assert not np.array_equal(after["bvh_triangles"][inst == i], before["bvh_triangles"][inst == i])
    assert np.array_equal(after["bvh_triangles"][:, [3, 7, 11]], before["bvh_triangles"][:, [3, 7, 11]])  # inst, prim, flags
    assert np.array_equal(after["bvh_nodes"][:, 24:], before["bvh_nodes"][:, 24:])  # the topology is the build's
    assert_same(after, before, ("instances", "triangles", "meshes"))
    S.check_tree(after)
    # a partial range with kept normals on top: only those positions change
    lo, hi = M.PARTIAL
    again = M.second_deformation(moved)
    sc.set_mesh_vertices(1, np.ascontiguousarray(again[lo:hi]), first=lo)
    want[offset + lo:offset + hi, 0:3] = again[lo:hi].view(np.uint32)
    last = S.host_tables(sc)
    assert np.array_equal(last["vertices"], want)
    assert np.array_equal(S.baked(last)[of_mesh].view(np.uint32), S.numpy_bake(last, S.instance_matrices(sc))[of_mesh].view(np.uint32))
    S.check_tree(last)


def test_recomputed_normals_match_the_definition_in_numpy():
    sc = M.room()
    before = S.host_tables(sc)
    p, n = sc.mesh_vertices(1)
    triangles = M.mesh_triangles(before, 1)
    # the undeformed icosphere: recomputed normals are distinguishable from the stored ones
    still, _ = M.numpy_normals(p, triangles, n)
    assert 1e-3 < np.abs(still - n).max() < 0.1
    moved = M.first_deformation(p)
    want, l2 = M.numpy_normals(moved, triangles, n)
    assert l2.min() > 1e-3  # no vertex takes the "normal stays" branch here
    sc.set_mesh_vertices(1, moved, recompute_normals=True)
    got_p, got_n = sc.mesh_vertices(1)
    assert np.array_equal(got_p.view(np.uint32), moved.view(np.uint32))
    assert np.array_equal(got_n.view(np.uint32), want.view(np.uint32))
    assert np.abs(np.linalg.norm(got_n.astype(np.float64), axis=1) - 1).max() < 1e-6
    # a partial range: the normals of ALL vertices of the mesh follow
    lo, hi = M.PARTIAL
    again = moved.copy()
    again[lo:hi] = M.second_deformation(moved)[lo:hi]
    sc.set_mesh_vertices(1, np.ascontiguousarray(again[lo:hi]), first=lo, recompute_normals=True)
    want_again, _ = M.numpy_normals(again, triangles, want)
    got_p, got_n = sc.mesh_vertices(1)
    assert np.array_equal(got_p.view(np.uint32), again.view(np.uint32)) and np.array_equal(got_n.view(np.uint32), want_again.view(np.uint32))
    changed = (want_again != want).any(axis=1)
    assert changed[:lo].any() or changed[hi:].any()  # neighbours outside the range
    S.check_tree(S.host_tables(sc))


COLLAPSED = """
Shape flake : InlineMesh { positions { 0,1,0, 1,1,0, 1,2,0, 0,2,0 } indices { 0,1,2, 0,2,3 } surface : Matte { } }
Shape floor : InlineMesh { positions { -4,0,-4, 4,0,-4, 4,0,4, -4,0,4 } indices { 0,2,1, 0,3,2 } surface : Matte { } }
Shape lamp : InlineMesh { positions { -1,4,-1, 1,4,-1, 1,4,1, -1,4,1 } indices { 0,1,2, 0,2,3 } light : Diffuse { emission : Constant { v { 9 } } } }
Camera cam : Pinhole { spp { 1 } film : Color { resolution { 8, 8 } } position { 0, 2, 7 } look_at { 0, 1, 0 } fov { 40 } }
render { cameras { @cam } shapes { @flake, @floor, @lamp } integrator : MegaPath { depth { 2 } } }
"""


def test_a_collapsed_mesh_keeps_its_normals():
    """two triangles collapsed to a point: every sum is zero, the recompute leaves the normals as they are (and divides by nothing)"""
    sc = Scene.from_string(COLLAPSED)
    mesh = sc.instance_mesh(0)
    p, n = sc.mesh_vertices(mesh)
    assert p.shape == (4, 3)
    given = np.ascontiguousarray(np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (4, 1)))
    sc.set_mesh_vertices(mesh, p, given)
    point = np.ascontiguousarray(np.tile(np.array([[0.5, 1.5, 0.25]], np.float32), (4, 1)))
    sc.set_mesh_vertices(mesh, point, recompute_normals=True)
    got_p, got_n = sc.mesh_vertices(mesh)
    assert np.array_equal(got_p, point) and np.array_equal(got_n.view(np.uint32), given.view(np.uint32))
    S.check_tree(S.host_tables(sc))
    # one live triangle (0, 1, 2): vertex 3 is named by the collapsed one alone and keeps its normal, the others get the live one's
    live = point.copy()
    live[1], live[2] = (1.5, 1.5, 0.25), (1.5, 2.5, 0.25)
    live[3] = live[0]
    sc.set_mesh_vertices(mesh, live, recompute_normals=True)
    _, got_n = sc.mesh_vertices(mesh)
    assert np.array_equal(got_n[:3], np.tile(np.array([[0, 0, 1]], np.float32), (3, 1))) and np.array_equal(got_n[3], given[3])


def test_supplied_kept_and_recomputed_normals_differ():
    vertices = []
    for mode in ("supplied", "kept", "recomputed"):
        sc = M.room()
        p, n = sc.mesh_vertices(1)
        moved = M.first_deformation(p)
        if mode == "supplied":
            sc.set_mesh_vertices(1, moved, np.ascontiguousarray(n[::-1]))
        else:
            sc.set_mesh_vertices(1, moved, recompute_normals=mode == "recomputed")
        vertices.append(M.vertex_words(sc, 1))
    assert np.array_equal(vertices[1][:, 3:6], M.vertex_words(M.room(), 1)[:, 3:6])  # kept
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert np.array_equal(vertices[a][:, 0:3], vertices[b][:, 0:3]) and not np.array_equal(vertices[a][:, 3:6], vertices[b][:, 3:6])


@pytest.mark.parametrize("lerp", [False, True])
def test_writing_back_a_meshs_own_vertices_changes_no_byte(lerp):
    """the build-time bake and tree and the re-bake agree"""
    sc = M.room(lerp=lerp)
    before = S.host_tables(sc)
    for mesh in (1, M.check_room(sc)["card_mesh"]):
        p, n = sc.mesh_vertices(mesh)
        sc.set_mesh_vertices(mesh, p, n)
        assert_same(S.host_tables(sc), before)
        sc.set_mesh_vertices(mesh, p)
        assert_same(S.host_tables(sc), before)


def test_set_time_bakes_the_new_vertices():
    sc, timed = M.room(lerp=True), M.room(lerp=True)
    ids = M.check_room(sc)
    p, _ = sc.mesh_vertices(1)
    moved = M.first_deformation(p)
    sc.set_mesh_vertices(1, moved, recompute_normals=True)
    assert sc.set_time(0.625)
    after = S.host_tables(sc)
    inst = after["bvh_triangles"][:, 3]
    of_mesh = np.isin(inst, [ids["ball_a"], ids["ball_b"]])
    assert np.array_equal(S.baked(after)[of_mesh].view(np.uint32), S.numpy_bake(after, S.instance_matrices(sc))[of_mesh].view(np.uint32))
    S.check_tree(after)
    # the other order gives the same tables: set_time first, then the deformation
    assert timed.set_time(0.625)
    timed.set_mesh_vertices(1, moved, recompute_normals=True)
    assert_same(S.host_tables(timed), after)
    assert not np.array_equal(after["bvh_triangles"], S.host_tables(M.room(lerp=True))["bvh_triangles"])


def test_refusals_change_nothing():
    sc = M.room()
    ids = M.check_room(sc)
    before = S.host_tables(sc)
    p, n = sc.mesh_vertices(1)
    lib = _ffi.host_lib()

    def call(mesh, first, count, positions, normals=None, flags=0):
        rc = lib.lrhost_scene_set_mesh_vertices(sc._handle, mesh, first, count, positions.ctypes.data if positions is not None else None,
                                                normals.ctypes.data if normals is not None else None, flags)
        return rc, lib.lrhost_last_error().decode()

    quad, _ = sc.mesh_vertices(ids["lamp_mesh"])
    rc, message = call(ids["lamp_mesh"], 0, 4, quad)
    assert rc != 0 and "light" in message and str(ids["lamp"]) in message  # the emitter: its alias table is not rebuilt
    with pytest.raises(HostError, match="light"):
        sc.set_mesh_vertices(ids["lamp_mesh"], quad)
    nan = p.copy()
    nan[300, 1] = np.nan
    bad_normal = n.copy()
    bad_normal[641, 2] = np.inf
    for args, text in (((1, 1, 642, p), "not inside"), ((1, 643, 0, p), "not inside"), ((len(before["meshes"]), 0, 1, p), "out of range"),
                       ((1, 0, 642, nan), "non-finite"), ((1, 0, 642, p, bad_normal), "non-finite"),
                       ((1, 0, 642, p, n, _ffi.MESH_RECOMPUTE_NORMALS), "NULL with"), ((1, 0, 642, None), "NULL"), ((1, 0, 642, p, None, 1), "flags")):
        rc, message = call(*args)
        assert rc != 0 and text in message, (args[:3], message)
    assert call(1, 642, 0, None)[0] == 0 and call(1, 0, 0, None, None, _ffi.MESH_RECOMPUTE_NORMALS)[0] == 0  # nothing to do is legal
    sc._views.clear()
    assert_same(S.host_tables(sc), before)
    for args in ((1, p[:, :2]), (1, p, n[:10]), (1, p, None, 1), (1, nan), (5, p), (1, p.astype(np.float64))):
        with pytest.raises(ValueError):
            sc.set_mesh_vertices(*args)
    with pytest.raises(ValueError):
        sc.set_mesh_vertices(1, p, n, recompute_normals=True)
    with pytest.raises(ValueError):
        sc.mesh_vertices(5)
    assert_same(S.host_tables(sc), before)


def test_argument_checks():
    p = np.zeros((6, 3), np.float32)
    n = np.ones((6, 3), np.float32)
    counts = [8, 6, 4]
    assert check_mesh_vertices(p) == "numpy" and check_mesh_vertices(p, n, 1, 0, counts) == "numpy"
    assert check_mesh_vertices(p[:2], n[:2], 0, 6, counts) == "numpy" and check_mesh_vertices(p[:0], None, 2, 4, counts) == "numpy"
    nan, inf = p.copy(), n.copy()
    nan[5, 2] = np.nan
    inf[0, 0] = -np.inf
    bad = [dict(positions=p.astype(np.float64)), dict(positions=p.reshape(3, 6)), dict(positions=p.reshape(-1)), dict(positions=p[:, ::-1]),
           dict(positions=np.zeros((6, 4), np.float32)[:, :3]), dict(positions=p.tolist()), dict(positions=nan), dict(positions=p, normals=inf),
           dict(positions=p, normals=n[:5]), dict(positions=p, normals=n.astype(np.float64)), dict(positions=p, normals=n.tolist()),
           dict(positions=p, mesh=3), dict(positions=p, mesh=-1), dict(positions=p, mesh=1.0), dict(positions=p, mesh=1, first=1),
           dict(positions=p, mesh=2), dict(positions=p, mesh=0, first=-1), dict(positions=p, mesh=0, first=3)]
    for kwargs in bad:
        with pytest.raises(ValueError):
            check_mesh_vertices(**{"meshes": counts, **kwargs})
    torch = pytest.importorskip("torch")
    for tensor in (torch.zeros(6, 3), torch.zeros(6, 3, dtype=torch.float64)):  # a CPU tensor is neither kind
        with pytest.raises(ValueError):
            check_mesh_vertices(tensor)
    with pytest.raises(ValueError):
        check_mesh_vertices(p, torch.zeros(6, 3))


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of _ffi.MeshUpdateParams, the flag and the table id against what the host compiler makes of lrhip.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(lrhip_mesh_update_params));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_mesh_update_params, {f}));' for f in FIELDS]
    lines += ['    printf("%u %u %u\\n", LRHIP_MESH_RECOMPUTE_NORMALS, LRHIP_RAY_DEVICE_POINTERS, LRHIP_TABLE_VERTICES);', "    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    st = _ffi.MeshUpdateParams
    assert [name for name, _ in st._fields_] == list(FIELDS)
    assert C.sizeof(st) == int(out[0]) == _ffi.host_lib().lrhost_sizeof(b"lrhip_mesh_update_params")
    for f, line in zip(FIELDS, out[1:]):
        assert getattr(st, f).offset == int(line), f
    assert [int(v) for v in out[1 + len(FIELDS)].split()] == [_ffi.MESH_RECOMPUTE_NORMALS, _ffi.RAY_DEVICE_POINTERS, _ffi.TABLE_VERTICES]
    assert _ffi.STRUCTS["lrhip_mesh_update_params"] is st and _ffi.TABLE_RECORD_BYTES[_ffi.TABLE_VERTICES] == 32
    assert _ffi.MESH_RECOMPUTE_NORMALS & (_ffi.RAY_DEVICE_POINTERS | _ffi.RAY_ALPHA_TEST | _ffi.RADIANCE_ACCUMULATE | _ffi.RADIANCE_COUNTERS) == 0


def test_new_symbols_exist_and_refuse_a_null_context():
    """needs no device: the entry points are in liblrhip.so and bound in _ffi, and a NULL context is LRHIP_ERROR_INVALID"""
    raw = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))
    for name in ("lrhip_set_mesh_vertices", "lrhip_last_mesh_update_ms"):
        assert hasattr(raw, name), name
    lib = _ffi.hip_lib()
    p = _ffi.MeshUpdateParams()
    assert lib.lrhip_set_mesh_vertices(None, C.byref(p)) == LRHIP_ERROR_INVALID and b"NULL" in lib.lrhip_last_error()
    assert lib.lrhip_set_mesh_vertices(None, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_last_mesh_update_ms(None) == 0.0
    assert lib.lrhip_scene_table_bytes(None, _ffi.TABLE_VERTICES) == 0
    assert lib.lrhip_read_scene_table(None, _ffi.TABLE_VERTICES, 0, 16, (C.c_uint8 * 16)()) == LRHIP_ERROR_INVALID
    assert hasattr(_ffi.host_lib(), "lrhost_scene_set_mesh_vertices")
