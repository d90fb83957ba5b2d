"""GPU test of the light sample's THREE tables (csrc/hip/dev_scene.h: DLightInstance, DLightTri; light_tris and light_tris_exact) against a yardstick
that is not the device: tests/light_record_reference.py restates the records in float64 from the host scene view (its module text: what is
compared as words, the band of 2 area ng, the counted roundings, the excluded triangles without area).  tests/test_gpu_light_records.py holds
the tables to a fresh upload made by the same kernels, which a wrong column, a wrong vertex offset or a transposed uv pair passes.

Judged: every scene of test_gpu_light_records.py at upload, and `crowd` (tests/light_record_scenes.py: 326 instances in 11 words of the `moved`
bit mask, 313 light instances -- a second block of light_instance_record_kernel -- a mirrored emitter, an emitter and a plain instance of one
mesh, a four-triangle emitter with a triangle without area behind larger meshes) at upload, after lrhip_set_instance_transforms of ids
{31, 32, 63, 64, 255, 256, last} in one call, after a second call on another set, after a move of instances without a light only, after
lrhip_update_scene, and after lrhip_set_mesh_vertices of a mesh whose instances sit at ids 41, 151 and 325.  At each moment the three light
tables are judged against the float64 restatement and compared byte for byte with a fresh upload of the moved scene, and the four geometry
tables are held byte for byte to the host route (as tests/test_gpu_instance_transforms.py does on 5 instances: here the update kernels see a
second mask word, and the scratch behind 32 instances, for the first time)."""
import numpy as np
import pytest

import instance_scene as I
import light_record_reference as L
import light_record_scenes as S
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import MegaPathRenderer
from test_gpu_light_records import SCENES

pytestmark = pytest.mark.gpu

LIGHT = {"light_instances": _ffi.TABLE_LIGHT_INSTANCES, "light_tris": _ffi.TABLE_LIGHT_TRIANGLES, "light_tris_exact": _ffi.TABLE_LIGHT_TRIANGLES_EXACT}
GEOMETRY = {"nodes": _ffi.TABLE_NODES, "bvh_triangles": _ffi.TABLE_BVH_TRIANGLES, "instances": _ffi.TABLE_INSTANCES, "shade_triangles": _ffi.TABLE_SHADE_TRIANGLES}
worst = {"light_tris": 0.0, "light_tris_exact": 0.0}  # the largest error / band of this run (light_record_reference.py: MEASURED_DEVICE_ERROR)


def _tables(r, which) -> dict:
    return {name: r.scene_table(t) for name, t in which.items()}


def _judge(light: dict, host: dict, matrices, degenerate: int, what: str) -> None:
    """the three light tables against the float64 restatement of the host view under `matrices`"""
    e = L.expected(host, matrices)
    L.judge_instances(light["light_instances"], e, what)
    for name in ("light_tris", "light_tris_exact"):
        ratio = L.judge_triangles(light[name], e, degenerate, f"{what}: {name}")
        worst[name] = max(worst[name], ratio)
        assert L.MEASURED_DEVICE_ERROR[name] is None or L.MEASURED_DEVICE_ERROR[name] <= 1.0  # a record of a run beside the bound, never the bound
        print(f"{what}: {name}: {len(e['copies'])} records, {degenerate} without area, largest error / band {ratio:.4f} (this run so far {worst[name]:.4f})")


def _assert_equal(a: dict, b: dict, what: str) -> None:
    for name in a:
        assert a[name].shape == b[name].shape, (what, name, a[name].shape, b[name].shape)
        rows = np.nonzero((a[name] != b[name]).any(axis=1))[0]
        assert rows.size == 0, (what, name, rows[:8], a[name][rows[:1]].view(np.uint32), b[name][rows[:1]].view(np.uint32))


@pytest.mark.parametrize("case", list(SCENES))
def test_the_tables_of_the_existing_scenes_against_float64(case):
    text, _ = SCENES[case]()
    scene = Scene.from_string(text)
    host = L.host_tables(scene)
    r = MegaPathRenderer(0)
    try:
        r.upload(scene)
        light = _tables(r, LIGHT)
    finally:
        r.close()
    assert len(light["light_instances"]) == len(host["light_instances"]) and (len(light["light_tris"]) > 0) == (case != "no_light")
    _judge(light, host, None, 0, case)
    for name in ("light_tris", "light_tris_exact"):  # no triangle without area in these scenes: every area is positive (as test_gpu_light_records.py asserts)
        assert (light[name].view(np.float32)[:, L.TRI_AREA_WORD] > 0).all()


def _srt(k: int) -> np.ndarray:
    """a matrix of its own for the k-th moved instance: rotation x non-uniform scale x translation, every third one mirrored"""
    scale = (0.1 + 0.03 * (k % 5), 1.0 + 0.1 * (k % 3), 0.15 + 0.02 * (k % 7))
    if k % 3 == 2:
        scale = (-scale[0], scale[1], scale[2])
    return I.srt(scale=scale, axis=(1 + k % 2, 2, 0.5 * (k % 4)), degrees=23.0 * k + 10.0, translate=(-2.0 + 0.37 * (k % 11), 2.0 + 0.21 * (k % 9), -1.5 + 0.3 * (k % 8)))


def _move(ra, scene_b, rb, ids, first=0):
    ids = np.asarray(ids)
    matrices = np.stack([_srt(first + k) for k in range(len(ids))])
    ra.set_instance_transforms(matrices, ids)
    scene_b.set_instance_transforms(matrices, ids)
    rb.upload(scene_b, keep_film=True)  # the host route: lrhip_update_scene


def _moment(ra, scene_b, rb, what: str, moved_from=None):
    """context A (the device route) at one moment: its light tables against float64 from scene B's host view (the moved scene), against context B
    (which took the host route) and against a fresh upload of scene B; its geometry tables against context B -> A's light tables"""
    host = L.host_tables(scene_b)
    light = _tables(ra, LIGHT)
    _judge(light, host, None, 1, what)
    if moved_from is not None:  # the restatement from the UNMOVED host view and the matrices alone, as the issue of a device move sees it
        _judge(light, moved_from, I.instance_matrices(scene_b), 1, what + " (from the matrices)")
    _assert_equal(light, _tables(rb, LIGHT), what + ": against the host route")
    _assert_equal(_tables(ra, GEOMETRY), _tables(rb, GEOMETRY), what + ": against the host route")
    fresh = MegaPathRenderer(0)
    try:
        fresh.upload(scene_b)
        _assert_equal(light, _tables(fresh, LIGHT), what + ": against a fresh upload")
    finally:
        fresh.close()
    return light


def _differs(a: dict, b: dict) -> list:
    return [name for name in a if not np.array_equal(a[name], b[name])]


def test_the_crowd_at_upload_after_moves_and_after_an_update():
    scene_a, scene_b = S.crowd(), S.crowd()
    ids = S.check_crowd(scene_a)
    unmoved = ids["tables"]
    lit, last = set(ids["lit"]), ids["last"]
    ra, rb = MegaPathRenderer(0), MegaPathRenderer(0)
    try:
        ra.upload(scene_a)
        rb.upload(scene_b)
        start = _moment(ra, scene_b, rb, "crowd at upload")
        heads = start["light_instances"].view(np.uint32)
        assert len(heads) == 313 > 256 and len(start["light_tris"]) == 310 * 2 + 2 * 320 + 4
        flat = start["light_tris"].view(np.float32)[heads[ids["lit"].index(ids["fan"]), 3] + S.FAN_FLAT]
        print(f"the triangle without area: ng {flat[L.TRI_NG_WORDS]}, area {flat[L.TRI_AREA_WORD]}, pdf {flat[L.TRI_PDF_WORD]}")
        # first move: mask words 0, 1, 2, 7, 8 and 10 in one call, emitters and others on both sides of three word boundaries
        first = [31, 32, 63, 64, 255, 256, last]
        assert {i >> 5 for i in first} == {0, 1, 2, 7, 8, 10} and 0 < len(lit & set(first)) < len(first)
        _move(ra, scene_b, rb, first)
        a = _moment(ra, scene_b, rb, "crowd after the first move", unmoved)
        assert _differs(a, start) == list(LIGHT)
        # second move, another set: the mirrored and the unmirrored icosphere swap roles, the four-triangle emitter, quads in words 0, 3 and 9
        second = [ids["glow"][0], ids["glow"][1], ids["fan"], 1, 33, 100, 290, 64]
        assert all(i in lit for i in second[:7])
        _move(ra, scene_b, rb, second, first=7)
        b = _moment(ra, scene_b, rb, "crowd after the second move", unmoved)
        assert _differs(b, a) == list(LIGHT)
        # a move of instances without a light only -- among them the plain instance of the emitters' mesh, and quads that share the emissive quads'
        # mesh in words 0, 1, 2, 8 -- leaves all three light tables as they are; the geometry follows the host route as before
        plain = [i for i in ids["plain"] if i != ids["room"]]
        assert ids["ball"] in plain and {i >> 5 for i in plain} >= {0, 1, 2, 8, 10}
        _move(ra, scene_b, rb, plain, first=15)
        c = _moment(ra, scene_b, rb, "crowd after a move of instances without a light", unmoved)
        assert _differs(c, b) == []
        # lrhip_update_scene over the device-moved context: scene A's own (unmoved) tables win again, every record re-baked
        ra.upload(scene_a, keep_film=True)
        _assert_equal(_tables(ra, LIGHT), start, "restored by lrhip_update_scene")
        _judge(_tables(ra, LIGHT), unmoved, None, 1, "crowd after lrhip_update_scene")
        # ... and a move works again
        scene_c = S.crowd()
        _move(ra, scene_c, rb, first)
        _moment(ra, scene_c, rb, "crowd, a move after the restore", unmoved)
    finally:
        ra.close()
        rb.close()


def test_a_deformation_behind_the_first_mask_word_equals_the_host_route():
    """lrhip_set_mesh_vertices of the slab mesh, whose instances are 41, 151 and 325 (mask words 1, 4 and 10): mesh_mark_kernel marks them, the
    update kernels re-bake, refit and re-quantise what they cover -- the four geometry tables against the host route -- and no light record moves"""
    scene_a, scene_b = S.crowd(), S.crowd()
    ids = S.check_crowd(scene_a)
    slabs = ids["slabs"]
    assert min(slabs) >= 32 and len({i >> 5 for i in slabs}) == 3
    mesh = scene_a.instance_mesh(slabs[0])
    assert all(scene_a.instance_mesh(i) == mesh for i in slabs)
    positions, _ = scene_a.mesh_vertices(mesh)
    assert positions.shape == (S.SLAB_VERTICES, 3)
    moved = (positions * [1.5, 1.0, 0.75] + [0.1, 0.2, -0.2]).astype(np.float32)
    moved[:, 1] += 0.1 * np.arange(S.SLAB_VERTICES, dtype=np.float32)  # out of its plane: the boxes grow on every axis
    ra, rb = MegaPathRenderer(0), MegaPathRenderer(0)
    try:
        ra.upload(scene_a)
        rb.upload(scene_b)
        start_light, start_geometry = _tables(ra, LIGHT), _tables(ra, GEOMETRY)
        ra.set_mesh_vertices(mesh, moved, recompute_normals=True)
        scene_b.set_mesh_vertices(mesh, moved, recompute_normals=True)
        rb.upload(scene_b, keep_film=True)
        geometry = _tables(ra, GEOMETRY)
        _assert_equal(geometry, _tables(rb, GEOMETRY), "deformed: against the host route")
        changed = _differs(geometry, start_geometry)
        assert "bvh_triangles" in changed and "shade_triangles" in changed and "nodes" in changed, changed
        # every baked triangle of the three instances moved, and no other
        inst = geometry["bvh_triangles"].view(np.uint32)[:-1, 3]
        rows = (geometry["bvh_triangles"][:-1] != start_geometry["bvh_triangles"][:-1]).any(axis=1)
        assert set(inst[rows]) == set(slabs) and rows.sum() == 3 * S.SLAB_TRIANGLES
        light = _tables(ra, LIGHT)
        assert _differs(light, start_light) == []
        _judge(light, L.host_tables(scene_b), None, 1, "crowd after a deformation")
        # then a device move of two of them and an emitter on top of the deformed vertices
        _move(ra, scene_b, rb, [slabs[2], 31, slabs[0]], first=3)
        _moment(ra, scene_b, rb, "crowd, a move after the deformation")
    finally:
        ra.close()
        rb.close()
