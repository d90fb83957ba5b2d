"""GPU test of the light sample's records (csrc/hip/dev_shade.h: LR_LIGHT_RECORDS; dev_scene.h: DLightInstance, DLightTri).

A light sample used to walk light instance -> instance -> alias entry -> triangle indices -> three vertices and to compute the emissive
triangle's world-space normal and area per sample.  The shipped kernels read one record per light instance and one per (light instance,
primitive), built on the device by the function that computed those constants per sample (dev_shade.h: triangle_constants), at upload and
again for whatever a scene update moves.  No random number, ray or branch of a path changes.  `make nolightrec` builds the kernels with the
chain of gathers (LR_LIGHT_RECORDS=0); this test holds the shipped library to it, on the pool kernel <4096> and on the one-path kernel <2>
(the scenes under the PaddedSobol sampler: <0>, which they take under the Independent one, spills one more register on the records and keeps
the chain, kernel_forms.h):

  * films bit-identical, from the shipped binaries (no counters) and from their counting twins;
  * the twins' path, ray, vertex, node, triangle and nee counters equal;
  * the light queries' answers bit-identical;
  * after lrhip_set_instance_transforms / lrhip_update_scene the film and the two tables equal a fresh upload of the moved scene, bit for
    bit, and a moved instance WITHOUT a light leaves both tables as they were.

The scenes, at 16 x 16 or 24 x 24 pixels, 2 to 8 spp, depth <= 4: the Cornell box's quad lamp; an emissive icosphere of 1280 triangles with
vertex uvs and a checkerboard (per-sample, `dynamic`) emission; a quad under a non-uniform scale and a rotation, one-sided and two-sided; two
instances of one emissive mesh; emitters under a constant environment with 0 < env_prob < 1; no light at all (empty tables, nothing read).
lrhip_set_mesh_vertices refuses a mesh with an emissive instance (its alias table is not rebuilt on the device), so no record can go stale
through it: the test holds that refusal and that the records stay."""
import os

import numpy as np
import pytest

from luisarender_amd import Scene, _ffi
from luisarender_amd.scenes import cornell_box
from luisarender_amd.scenes.bathroom import icosphere, inline_mesh

pytestmark = pytest.mark.gpu
POOL = 4096  # LRHIP_FEAT_POOL
GENERIC = 2  # LRHIP_FEAT_GENERIC: the run-time generic sampler
EQUAL_COUNTERS = ("paths", "closest_rays", "shadow_rays", "surface_hits", "nee_samples", "path_length_sum", "nodes_visited", "tris_tested", "nodes_empty",
                  "shade_busy")

_HEAD = """
Shape room : InlineMesh { positions { -3,0,-3, 3,0,-3, 3,0,3, -3,0,3, -3,5,-3, 3,5,-3, 3,5,3, -3,5,3 }
  indices { 0,2,1, 0,3,2, 4,5,6, 4,6,7, 0,1,5, 0,5,4, 0,4,7, 0,7,3, 1,2,6, 1,6,5 } surface : Matte { Kd : Constant { v { 0.6, 0.6, 0.55 } } } }
Shape ball : Sphere { subdivision { 1 } surface : Matte { Kd : Constant { v { 0.7, 0.3, 0.2 } } } transform : SRT { scale { 0.8, 0.8, 0.8 } translate { -1.25, 0.8, 0 } } }
"""
_TAIL = """
Camera cam : Pinhole { spp { SPP } film : Color { resolution { RES, RES } } position { 0, 2.5, 8.5 } look_at { 0, 2, 0 } fov { 40 } }
render { cameras { @cam } shapes { @room, @ball, SHAPES } ENVIRONMENT integrator : MegaPath { depth { DEPTH } sampler : Independent { seed { 11 } } } }
"""
_QUAD = "InlineMesh { positions { -0.75,0,-0.75, 0.75,0,-0.75, 0.75,0,0.75, -0.75,0,0.75 } indices { 0,1,2, 0,2,3 }"
_ENV = "environment : Spherical { emission : Constant { v { 0.3, 0.5, 0.8 } } scale { 1.5 } transform : SRT { rotate { 0.3, 1, 0.2, 70 } } }"


def _room(shapes: dict, resolution=16, spp=4, depth=4, environment="") -> str:
    tail = _TAIL.replace("SPP", str(spp)).replace("RES", str(resolution)).replace("DEPTH", str(depth)).replace("ENVIRONMENT", environment)
    return _HEAD + "".join(f"Shape {name} : {text}\n" for name, text in shapes.items()) + tail.replace("SHAPES", ", ".join("@" + n for n in shapes))


def _scaled_quad(two_sided: bool) -> str:
    return _room({"lamp": _QUAD + " light : Diffuse { emission : Constant { v { 12, 11, 9 } } two_sided { %s } } "
                          "transform : SRT { scale { 1.5, 1, 0.4 } rotate { 1, 0.3, 0.2, 25 } translate { 0.4, 3.6, 0.2 } } }" % ("true" if two_sided else "false")})


def _textured_icosphere() -> str:
    v, f, n = icosphere(3)
    assert len(f) == 1280
    uv = np.stack([np.arctan2(v[:, 2], v[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(v[:, 1], -1, 1)) / np.pi], -1)
    mesh = inline_mesh("glow", v * 0.6, f, n, uv)
    assert mesh.endswith("}\n")
    light = ("  light : Diffuse { emission : Checkerboard { on : Constant { v { 9, 6, 2 } } off : Constant { v { 1, 3, 8 } } scale { 6 } } }\n"
             "  transform : SRT { scale { 1, 0.7, 1.2 } rotate { 0, 1, 1, 30 } translate { 0.5, 3.4, 0.3 } }\n}\n")
    text = _room({"glow": "PLACEHOLDER"}, resolution=24, spp=2, depth=3)
    return text.replace("Shape glow : PLACEHOLDER\n", mesh[:-2] + light)


def _two_instances() -> str:
    lamp = "Sphere { subdivision { 2 } light : Diffuse { emission : Constant { v { %s } } two_sided { true } } transform : SRT { %s } }"
    return _room({"lamp_a": lamp % ("9, 2, 1", "scale { 0.4, 0.4, 0.4 } translate { -1.5, 3.8, 0.5 }"),
                  "lamp_b": lamp % ("1, 3, 9", "scale { 0.3, 0.6, 0.3 } rotate { 1, 0, 0, 50 } translate { 1.6, 3.2, -0.5 }")}, resolution=24, spp=2)


def _with_environment() -> str:
    return _room({"lamp": _QUAD + " light : Diffuse { emission : Constant { v { 12, 11, 9 } } } transform : SRT { translate { 0, 4.2, 0 } } }",
                  "hole": _QUAD + " surface : Matte { } transform : SRT { translate { 0, 5.5, 0 } } }"}, environment=_ENV).replace(
        "4,5,6, 4,6,7, ", "")  # (the room without its ceiling: the environment lights it)


def _no_light() -> str:
    return _room({"card": _QUAD + " surface : Matte { } transform : SRT { translate { 0, 1.5, 1 } } }"}, environment=_ENV).replace("4,5,6, 4,6,7, ", "")


SCENES = {
    "cornell_quad": lambda: (cornell_box(resolution=16, spp=8, depth=4), 8),
    "textured_icosphere": lambda: (_textured_icosphere(), 2),
    "scaled_one_sided": lambda: (_scaled_quad(False), 4),
    "scaled_two_sided": lambda: (_scaled_quad(True), 4),
    "two_instances": lambda: (_two_instances(), 2),
    "environment": lambda: (_with_environment(), 4),
    "no_light": lambda: (_no_light(), 4),
}


def _twin():
    lib = os.path.join(_ffi.LIB_DIR, "variants", "liblrhip_nolightrec.so")
    if not os.path.exists(lib):  # (a failure, not a skip: without the library nothing is checked)
        pytest.fail("luisarender_amd/lib/variants/liblrhip_nolightrec.so is missing: make nolightrec (python __graft_entry__.py builds it)")
    return lib


def _renderer(lib_path, pool):
    from luisarender_amd.render import MegaPathRenderer
    r = MegaPathRenderer(0, lib_path=lib_path) if lib_path else MegaPathRenderer(0)
    r.set_scheduler(pool)
    return r


def _scene(case, pool):
    """the case's scene and spp; for the one-path kernels under the PaddedSobol sampler, which takes <2> (the run-time generic sampler)"""
    text, spp = SCENES[case]()
    if pool is False:
        assert text.count("sampler : Independent") == 1
        text = text.replace("sampler : Independent", "sampler : PaddedSobol")
    return Scene.from_string(text), spp


def _frames(r, spp):
    """film without counters, film and counters of the counting twin, the variants that ran"""
    r.clear()
    r.render(0, spp, sync=True)
    shipped, v_shipped = r.download(False), r.last_variant()
    r.clear()
    start = r.counters()  # (a context's counters run on from render to render)
    r.render(0, spp, counters=True, sync=True)
    counters = {k: v - start[k] for k, v in r.counters().items() if not isinstance(v, list)}
    return shipped, v_shipped, r.download(False), r.last_variant(), counters


def _assert_same(a, b, spp, pool, what):
    film_a, va, twin_a, vta, ca = a
    film_b, vb, twin_b, vtb, cb = b
    assert va == vb == (POOL if pool else GENERIC) and vta == vtb == (va | 1), (what, va, vb, vta, vtb)
    assert np.isfinite(film_a).all() and (film_a[..., 3] == spp).all(), what
    assert np.array_equal(film_a.view(np.uint32), film_b.view(np.uint32)), f"{what}: shipped binaries: the films differ"
    assert np.array_equal(twin_a.view(np.uint32), twin_b.view(np.uint32)), f"{what}: counting twins: the films differ"
    for k in EQUAL_COUNTERS:
        assert ca[k] == cb[k], (what, k, ca[k], cb[k])


@pytest.mark.parametrize("pool", [True, False], ids=["pool", "one_path"])
@pytest.mark.parametrize("case", list(SCENES))
def test_records_render_the_frames_of_the_chain_of_gathers(case, pool):
    lib = _twin()
    scene, spp = _scene(case, pool)
    view = scene.view()
    results, tables = [], None
    for path in (None, lib):
        r = _renderer(path, pool)
        try:
            r.upload(scene)
            results.append(_frames(r, spp))
            if path is None:
                tables = r.scene_table(_ffi.TABLE_LIGHT_INSTANCES), r.scene_table(_ffi.TABLE_LIGHT_TRIANGLES)
        finally:
            r.close()
    ca = results[0][4]
    print(f"{case} ({'pool' if pool else 'one path'}): <{results[0][1]}>, light instances {len(tables[0])}, triangle records {len(tables[1])}, "
          f"nee samples {ca['nee_samples']}, shadow rays {ca['shadow_rays']}, vertices {ca['shade_busy']}")
    _assert_same(results[0], results[1], spp, pool, case)
    assert len(tables[0]) == int(view.light_instance_count)
    if case == "no_light":
        assert len(tables[0]) == 0 and len(tables[1]) == 0
    else:
        assert ca["nee_samples"] > 0 and ca["shadow_rays"] > 0 and results[0][0][..., :3].sum() > 0
        head = tables[0].view(np.uint32)
        assert len(tables[1]) == int(head[:, 2].sum())  # one record per (light instance, primitive): per instance, not per mesh
        assert np.array_equal(head[:, 3], np.concatenate([[0], np.cumsum(head[:, 2])[:-1]]))
        tris = tables[1].view(np.float32)
        assert np.isfinite(tris).all() and (tris[:, 18] > 0).all()  # world-space area
        assert np.allclose(np.linalg.norm(tris[:, [3, 7, 11]], axis=1), 1.0, atol=1e-5)  # world-space geometric normal
    if case == "two_instances":
        head = tables[0].view(np.uint32)
        assert len(head) == 2 and head[0, 1] == head[1, 1] and head[0, 0] != head[1, 0]  # one mesh (one alias table), two instances
        tris = tables[1].view(np.float32)
        half = len(tris) // 2
        assert np.array_equal(tris[:half, 0:3], tris[half:, 0:3]) and not np.array_equal(tris[:half, 18], tris[half:, 18])  # same vertices, other areas
    if case == "environment":
        assert 0.0 < float(view.integrator.env_prob) < 1.0


def _light_query(r, scene_points, u):
    s = r.light_sample(points=scene_points, u=u)
    return [np.asarray(x) for x in (s.rays, s.L, s.pdf)]


@pytest.mark.parametrize("case", ["textured_icosphere", "scaled_one_sided", "environment"])
def test_light_queries_answer_alike(case):
    lib = _twin()
    text, _ = SCENES[case]()
    scene = Scene.from_string(text)
    rng = np.random.default_rng(7)
    n = 1000  # (no multiple of the block)
    points = (rng.random((n, 3)) * [5.0, 2.5, 5.0] + [-2.5, 0.2, -2.5]).astype(np.float32)
    u = rng.random((n, 3)).astype(np.float32)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 7] = [0.0, 1.0, 2.0], 1e-3, 1e30
    d = rng.normal(size=(n, 3))
    d[:, 1] = np.abs(d[:, 1])
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    answers = []
    for path in (None, lib):
        r = _renderer(path, None)
        try:
            r.upload(scene)
            sampled = _light_query(r, points, u)
            found = r.light_evaluate(r.trace(rays), rays)
            answers.append(sampled + [np.asarray(found.L), np.asarray(found.pdf), np.asarray(found.kind)])
        finally:
            r.close()
    for a, b in zip(*answers):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), case
    area = answers[0][2] > 0
    print(f"{case}: {int(area.sum())} of {n} samples with a pdf, {int((answers[0][5] == _ffi.LIGHT_KIND_AREA).sum())} rays found an emitter")
    assert area.sum() > n // 10


def _ids(scene):
    """instance ids by what they are: the emitter and a mesh instance without a light"""
    v = scene.view()
    handles = np.array([v.instances[i].handle.x for i in range(v.instance_count)])
    lights = [i for i in range(len(handles)) if handles[i] & 8]  # LR_SHAPE_HAS_LIGHT
    balls = [i for i in range(len(handles)) if not handles[i] & 8 and v.meshes[handles[i] >> 10].triangle_count == 80]
    assert len(lights) == 1 and len(balls) == 1
    return lights[0], balls[0]


def _srt(scale, axis, degrees, translate):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.deg2rad(degrees)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = (np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)) @ np.diag(np.asarray(scale, np.float64))
    m[:3, 3] = translate
    return np.ascontiguousarray(m.T.astype(np.float32))  # column-major storage


@pytest.mark.parametrize("pool", [True, False], ids=["pool", "one_path"])
@pytest.mark.parametrize("which", ["emitter", "other"])
def test_a_move_on_the_device_equals_a_fresh_upload(which, pool):
    """lrhip_set_instance_transforms, then the host route lrhip_update_scene, against a fresh upload of the moved scene"""
    (scene_a, spp), (scene_b, _) = _scene("scaled_one_sided", pool), _scene("scaled_one_sided", pool)
    lamp, ball = _ids(scene_a)
    target = np.array([lamp if which == "emitter" else ball])
    matrix = _srt((0.8, 1.0, 1.7), (0.2, 1, 0.4), 200.0, (-0.6, 3.1, 0.5))[None]
    ra, rb = _renderer(None, pool), _renderer(None, pool)
    try:
        ra.upload(scene_a)
        before = ra.scene_table(_ffi.TABLE_LIGHT_INSTANCES), ra.scene_table(_ffi.TABLE_LIGHT_TRIANGLES)
        film_before = _frames(ra, spp)[0]
        ra.set_instance_transforms(matrix, target)
        scene_b.set_instance_transforms(matrix, target)
        rb.upload(scene_b)
        after = ra.scene_table(_ffi.TABLE_LIGHT_INSTANCES), ra.scene_table(_ffi.TABLE_LIGHT_TRIANGLES)
        fresh = rb.scene_table(_ffi.TABLE_LIGHT_INSTANCES), rb.scene_table(_ffi.TABLE_LIGHT_TRIANGLES)
        for t in range(2):
            assert np.array_equal(after[t], fresh[t]), (which, t)
            assert np.array_equal(after[t], before[t]) == (which == "other"), (which, t)  # another instance's move leaves the records alone
        a, b = _frames(ra, spp), _frames(rb, spp)
        _assert_same(a, b, spp, pool, which)
        assert not np.array_equal(a[0], film_before)
        # the host route over the same context: lrhip_update_scene re-bakes every record
        ra.upload(scene_b, keep_film=True)
        for t, table in enumerate((_ffi.TABLE_LIGHT_INSTANCES, _ffi.TABLE_LIGHT_TRIANGLES)):
            assert np.array_equal(ra.scene_table(table), fresh[t]), (which, t)
        _assert_same(_frames(ra, spp), b, spp, pool, which + ", lrhip_update_scene")
    finally:
        ra.close()
        rb.close()


def test_an_emissive_mesh_is_not_deformed_and_its_records_stay():
    from luisarender_amd.render import DeviceError
    text, _ = SCENES["scaled_one_sided"]()
    scene = Scene.from_string(text)
    lamp, ball = _ids(scene)
    r = _renderer(None, None)
    try:
        r.upload(scene)
        before = r.scene_table(_ffi.TABLE_LIGHT_INSTANCES), r.scene_table(_ffi.TABLE_LIGHT_TRIANGLES)
        with pytest.raises(DeviceError, match="emitter"):
            r.set_mesh_vertices(scene.instance_mesh(lamp), np.zeros((4, 3), np.float32))
        # deforming a mesh without a light marks its instances, and only those: the records are not written
        r.set_mesh_vertices(scene.instance_mesh(ball), np.full((1, 3), 0.25, np.float32))
        assert np.array_equal(r.scene_table(_ffi.TABLE_LIGHT_INSTANCES), before[0])
        assert np.array_equal(r.scene_table(_ffi.TABLE_LIGHT_TRIANGLES), before[1])
    finally:
        r.close()
