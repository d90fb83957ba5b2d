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
through it: the test holds that refusal and that the records stay.

Further down, one record-reading kernel of every other family against the same twin (FAMILIES, the two query families), each asserted NOT to be
one of the kernels that keep the chain in the shipped library (csrc/hip/kernel_forms.h: LR_MASK_KEEPS_LIGHT_GATHERS, read off the header), on a scene
whose three emitters have 320, 2 and 80 triangles; and a four-triangle emitter with a triangle without area, end to end.  The tables' CONTENT is
judged against float64 in tests/test_gpu_light_record_tables.py."""
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


# ---- every family of kernels that reads the records, against the chain of gathers ----------------------------------------------------------------
# The cases above reach <4096>, <2> and the light query unit.  `make nolightrec` also holds one record-reading kernel of every other family
# (Makefile: NOLIGHTREC_MASKS); each case below renders or queries one scene on the shipped library and on the twin and holds the answers to
# each other bit for bit.  The scenes' emitters tell records apart: three light instances of 320, 2 and 80 triangles -- a wrong tri_base, alias_base
# or table shows -- the first of them an icosphere with vertex uvs under a checkerboard emission.
ENV, ALPHA, DISNEY, MIX, LAYERED, AUX, VPT, NEST, WF, CONT, PADDED, AOV, QUERY, GATHER = 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 16384, 32768, 65536, 131072
_CUTOUT = "Surface NAME : Matte { Kd : Constant { v { 0.7, 0.6, 0.2 } } alpha : Checkerboard { on : Constant { v { 1 } } off : Constant { v { 0.2 } } scale { 3 } } }"
_MATTE = "Surface NAME : Matte { Kd : Constant { v { 0.7, 0.3, 0.2 } } }"


def _keep_list() -> set:
    """the masks of LR_MASK_KEEPS_LIGHT_GATHERS, read off csrc/hip/kernel_forms.h (each stands for itself and its counting twin)"""
    import re
    text = open(os.path.join(_ffi.REPO_ROOT, "luisarender_amd", "csrc", "hip", "kernel_forms.h")).read()
    body = re.search(r"#define LR_MASK_KEEPS_LIGHT_GATHERS\(M\)((?:.*\\\n)*.*\n)", text).group(1)
    masks = {int(m) for m in re.findall(r"LR_MASK_OR_TWIN\(M, (\d+)\)", body)}
    assert len(masks) == 25 and 0 in masks and 4116 in masks, masks
    return masks


def _reads_records(mask: int) -> bool:
    return (mask & ~1) not in _keep_list()


def _surface(name: str, material: str) -> str:
    from helpers import MATERIALS
    text = {"matte": _MATTE, "cutout": _CUTOUT}.get(material) or MATERIALS[material].replace("Surface m ", "Surface NAME ")
    return text.replace("NAME", name) + "\n"


_SUN = "environment : Directional { emission : Constant { v { 3, 2.5, 2 } } angle { 40 } direction { 0.1, -1, 0.2 } }"  # (a constant one needs no kernel of the environment bit)


def _family_scene(surfaces=("matte", "matte", "matte"), environment="", integrator="MegaPath {", sampler="Independent", extra="") -> str:
    """a room (open to the environment, if there is one) with two balls and a card under three emitters"""
    v, f, n = icosphere(2)
    assert len(f) == 320
    uv = np.stack([np.arctan2(v[:, 2], v[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(v[:, 1], -1, 1)) / np.pi], -1)
    glow = inline_mesh("glow", v * 0.5, f, n, uv)
    assert glow.endswith("}\n")
    glow = glow[:-2] + ("  light : Diffuse { emission : Checkerboard { on : Constant { v { 9, 6, 2 } } off : Constant { v { 1, 3, 8 } } scale { 6 } } }\n"
                        "  transform : SRT { scale { 1, 0.7, 1.2 } rotate { 0, 1, 1, 30 } translate { 0.5, 3.4, 0.3 } }\n}\n")
    room = _HEAD.split("Shape ball")[0]
    if environment:
        room = room.replace("4,5,6, 4,6,7, ", "")
    text = "".join(_surface(f"s{k}", m) for k, m in enumerate(surfaces)) + extra + room + glow + f"""
Shape ball : Sphere {{ subdivision {{ 1 }} surface {{ @s0 }} transform : SRT {{ scale {{ 0.8, 0.8, 0.8 }} translate {{ -1.25, 0.8, 0 }} }} }}
Shape ball2 : Sphere {{ subdivision {{ 1 }} surface {{ @s1 }} transform : SRT {{ scale {{ 0.6, 0.6, 0.6 }} translate {{ 1.3, 0.6, 0.6 }} }} }}
Shape card : {_QUAD} surface {{ @s2 }} transform : SRT {{ scale {{ 2, 1, 2 }} rotate {{ 1, 0, 0, 20 }} translate {{ 0, 0.4, 1.2 }} }} }}
Shape lamp : {_QUAD} light : Diffuse {{ emission : Constant {{ v {{ 12, 11, 9 }} }} two_sided {{ true }} }}
  transform : SRT {{ scale {{ 1.5, 1, 0.4 }} rotate {{ 1, 0.3, 0.2, 25 }} translate {{ -1.2, 3.6, -0.8 }} }} }}
Shape bulb : Sphere {{ subdivision {{ 1 }} light : Diffuse {{ emission : Constant {{ v {{ 2, 8, 3 }} }} two_sided {{ true }} }}
  transform : SRT {{ scale {{ 0.25, 0.4, 0.25 }} translate {{ 1.8, 2.6, -1.2 }} }} }}
Camera cam : Pinhole {{ spp {{ 2 }} film : Color {{ resolution {{ 24, 24 }} }} position {{ 0, 2.5, 8.5 }} look_at {{ 0, 2, 0 }} fov {{ 40 }} }}
render {{ cameras {{ @cam }} shapes {{ @room, @glow, @ball, @ball2, @card, @lamp, @bulb }} {environment}
  integrator : {integrator} depth {{ 3 }} sampler : {sampler} {{ seed {{ 11 }} }} }} }}
"""
    return text


# family: (scene arguments, what runs: pool scheduler / wavefront mode, the kernel it lands on, whether the twin holds its counting twin,
# whether the case is run once more after a device move of an emitter)
FAMILIES = {
    "alpha": (dict(surfaces=("cutout", "matte", "matte")), dict(pool=False), ALPHA, True, False),
    "disney": (dict(surfaces=("disney", "matte", "disney_thin")), dict(pool=False), DISNEY, True, False),
    "env_disney": (dict(surfaces=("disney", "matte", "matte"), environment=_SUN), dict(pool=False), ENV | DISNEY, True, False),
    "mix": (dict(surfaces=("mix", "cutout", "disney"), environment=_ENV), dict(pool=False, wavefront=False), 60, True, False),
    "layered": (dict(surfaces=("layered", "mix", "disney")), dict(pool=False, wavefront=False), 124, True, True),
    "nested": (dict(surfaces=("mix_layered", "layered_mix", "matte")), dict(pool=False, wavefront=False), 636, False, False),
    "direct": (dict(surfaces=("glass", "matte", "matte"), integrator='Direct { importance_sampling { "both" }'), dict(pool=False), 252, False, False),
    "aov": (dict(surfaces=("disney", "matte", "matte"), integrator='AOV { components { "sample", "diffuse", "specular" }'), dict(pool=False), 32892, False, False),
    "volumetric": (dict(surfaces=("glass", "matte", "matte"), integrator="MegaVPTNaive {"), dict(pool=False), VPT, False, True),
    "wavefront": (dict(surfaces=("mix", "layered", "disney")), dict(pool=False, wavefront=True), WF, True, True),
    "pool_wavefront": (dict(surfaces=("mix", "layered", "disney")), dict(pool=True, wavefront=True), POOL | WF, False, False),
    "padded_pool": (dict(sampler="PaddedSobol"), dict(pool=True), PADDED | POOL | GENERIC, True, False),
}


def _emitter(scene) -> int:
    """the instance of the textured icosphere: the emitter with 320 triangles"""
    v = scene.view()
    ids = [i for i in range(v.instance_count) if v.instances[i].handle.x & 8 and v.meshes[v.instances[i].handle.x >> 10].triangle_count == 320]
    assert len(ids) == 1
    return ids[0]


def _plan(features, pool, sampler_kind, wf_mode, depth):
    """lrhip_plan_kernels: (family, camera or main mask, continuation mask, heavy masks of Disney / Mix / Layered)"""
    import ctypes as C
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))
    lib.lrhip_plan_kernels.argtypes = [C.c_uint32] * 6 + [C.POINTER(C.c_uint32 * 8)]
    out = (C.c_uint32 * 8)()
    assert lib.lrhip_plan_kernels(features, 0, (8 if pool else 0) | 16, sampler_kind, wf_mode, depth, C.byref(out)) == 0
    return list(out)[:6]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_reader_family_renders_the_frames_of_the_chain_of_gathers(family):
    lib = _twin()
    scene_args, run, mask, counting, moves = FAMILIES[family]
    scene = Scene.from_string(_family_scene(**scene_args))
    view = scene.view()
    assert int(view.light_instance_count) == 3
    spp = 2
    matrix = _srt((0.8, 1.0, 1.4), (0.2, 1, 0.4), 200.0, (-0.3, 3.0, 0.6))[None]
    target = np.array([_emitter(scene)])
    answers = []
    for path in (None, lib):
        r = _renderer(path, run["pool"])
        try:
            if "wavefront" in run:
                r.set_wavefront(run["wavefront"])
            r.upload(scene)
            rounds = []
            for moved in ((False, True) if moves else (False,)):
                if moved:  # the shipped library re-bakes the emitter's records; the twin reads `instances` itself: a stale record is a film difference
                    r.set_instance_transforms(matrix, target)
                r.clear()
                r.render(0, spp, sync=True)
                if family == "aov":  # (its film is the `sample` buffer)
                    got = {c: r.download_aov(c, normalized=False) for c in ("sample", "diffuse", "specular")}
                    got["film"], got["variant"] = got["sample"], r.last_variant()
                else:
                    got = {"film": r.download(False), "variant": r.last_variant()}
                if counting:
                    r.clear()
                    start = r.counters()
                    r.render(0, spp, counters=True, sync=True)
                    got["counting film"], got["counting variant"] = r.download(False), r.last_variant()
                    got["counters"] = {k: v - start[k] for k, v in r.counters().items() if not isinstance(v, list)}
                rounds.append(got)
            answers.append(rounds)
        finally:
            r.close()
    for k, (a, b) in enumerate(zip(*answers)):
        what = f"{family}{', after a device move of the emitter' if k else ''}"
        variant = a["variant"]
        if run.get("wavefront"):
            closures = variant & (DISNEY | MIX | LAYERED | NEST)
            camera = variant & ~closures
            plan = _plan(closures, run["pool"], int(view.sampler.kind), 0, 3)
            assert plan[0] == 3 and plan[1] == camera == mask and plan[2] == (camera | CONT) and closures == (DISNEY | MIX | LAYERED), (what, variant, plan)
            kernels = [camera, camera | CONT]  # (the heavy kernels have no form that keeps the chain in the shipped library: kernel_forms.h)
            print(f"{what}: camera pass <{camera}>, continuation pass <{camera | CONT}>, heavy kernels {plan[3:6]}")
        else:
            assert variant == mask, (what, variant, mask)
            kernels = [variant]
            print(f"{what}: <{variant}>")
        for m in kernels:
            assert _reads_records(m), (what, m, "keeps the chain of gathers in the shipped library: the case would compare the chain with itself")
        assert b["variant"] == variant, (what, variant, b["variant"])
        film = a["film"]
        if family != "aov":
            assert np.isfinite(film).all() and (film[..., 3] == spp).all() and film[..., :3].sum() > 0, what
        assert np.array_equal(film.view(np.uint32), b["film"].view(np.uint32)), f"{what}: the films differ"
        if family == "aov":
            for c in ("sample", "diffuse", "specular"):
                assert np.array_equal(a[c].view(np.uint32), b[c].view(np.uint32)), f"{what}: the {c} buffers differ"
            assert np.isfinite(a["sample"]).all() and a["sample"].sum() > 0
        if counting:
            assert a["counting variant"] == b["counting variant"] and a["counting variant"] & 1, what
            assert np.array_equal(a["counting film"].view(np.uint32), b["counting film"].view(np.uint32)), f"{what}: counting twins: the films differ"
            for c in EQUAL_COUNTERS:
                assert a["counters"][c] == b["counters"][c], (what, c, a["counters"][c], b["counters"][c])
            assert a["counters"]["nee_samples"] > 0 and a["counters"]["shadow_rays"] > 0
    if moves:
        assert not np.array_equal(answers[0][0]["film"], answers[0][1]["film"])


@pytest.mark.parametrize("family", ["gather", "radiance"])
def test_query_families_answer_as_the_chain_of_gathers(family):
    """lrhip_gather_irradiance on <196734> (the exact-arithmetic table) and lrhip_trace_radiance on <65660>: raw sums over 1000 records, explicit streams;
    the gather once more after a device move of the emitter.  Neither call reports its kernel: the mask is the rule of lrhip_gather.hip /
    lrhip_radiance.hip -- the all-closures mask, | 2 for a sampler other than Independent -- and the twin holds no other kernel of either kind, where
    a missing kernel is an error."""
    lib = _twin()
    sampler = "PaddedSobol" if family == "gather" else "Independent"  # (<196732>, the gather kernel of the Independent sampler, keeps the chain)
    scene = Scene.from_string(_family_scene(surfaces=("disney", "mix", "matte"), sampler=sampler))
    generic = GENERIC if int(scene.view().sampler.kind) != 0 else 0
    mask = (GATHER | QUERY | 124 | generic) if family == "gather" else (QUERY | 124 | generic)
    assert mask == (196734 if family == "gather" else 65660) and _reads_records(mask)
    print(f"{family}: <{mask}>")
    rng = np.random.default_rng(5)
    n = 1000  # (no multiple of the block)
    streams = rng.permutation(4096)[:n].astype(np.uint32)
    points = (rng.random((n, 3)) * [5.0, 2.5, 5.0] + [-2.5, 0.2, -2.5]).astype(np.float32)
    normals = rng.normal(size=(n, 3))
    normals[:, 1] = np.abs(normals[:, 1])
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 7] = points, 1e-3, 1e30
    rays[:, 4:7] = normals
    matrix = _srt((0.8, 1.0, 1.4), (0.2, 1, 0.4), 200.0, (-0.3, 3.0, 0.6))[None]
    target = np.array([_emitter(scene)])
    answers = []
    for path in (None, lib):
        r = _renderer(path, None)
        try:
            r.upload(scene)
            ask = (lambda: r.irradiance(points=points, normals=normals, spp=4, streams=streams, raw=True)) if family == "gather" else \
                  (lambda: r.radiance(rays, spp=4, streams=streams, raw=True))
            got = [np.array(ask())]
            if family == "gather":
                r.set_instance_transforms(matrix, target)
                got.append(np.array(ask()))
            answers.append(got)
        finally:
            r.close()
    for k, (a, b) in enumerate(zip(*answers)):
        assert a.shape == (n, 4) and np.isfinite(a).all() and (a[:, 3] == 4).all() and a[:, :3].sum() > 0, (family, k)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{family}{', after a device move of the emitter' if k else ''}: the sums differ"
    if family == "gather":
        assert not np.array_equal(answers[0][0], answers[0][1])


# ---- a triangle without area inside an emitter, end to end ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [True, False], ids=["pool", "one_path"])
def test_a_triangle_without_area_is_never_sampled(pool):
    """tests/light_record_scenes.py: the four-triangle emitter whose primitive 2 has two equal corners.  Its record holds area 0 and a normal that is
    not a number (tests/test_gpu_light_record_tables.py prints it); the host gives it the probability 0 and no alias entry names it, so no sample may
    go through it: the film is finite with every sample counted, shipped equals twin bit for bit, and no light sample carries a non-finite number."""
    import light_record_reference as L
    import light_record_scenes as S
    lib = _twin()
    spp = 4
    scene = Scene.from_string(S.fan_text(spp=spp, resolution=24, sampler="Independent" if pool else "PaddedSobol"))
    t = L.host_tables(scene)
    (fan,) = [i for i in range(len(t["instances"])) if t["instances"][i, 0] & 8]
    _, _, tri_offset, tri_count = (int(x) for x in t["meshes"][t["instances"][fan, 0] >> 10])
    assert tri_count == S.FAN_TRIANGLES and L.expected(t)["degenerate"].tolist() == [k == S.FAN_FLAT for k in range(tri_count)]
    import ctypes as C
    alias = np.frombuffer(C.string_at(scene.view().tri_alias, (tri_offset + tri_count) * 8), np.uint32).reshape(-1, 2)[tri_offset:]
    assert alias[S.FAN_FLAT, 0:1].view(np.float32)[0] == 0.0 and t["tri_pdf"][tri_offset + S.FAN_FLAT] == 0  # never kept when its slot is drawn ...
    assert all(int(alias[k, 1]) != S.FAN_FLAT for k in range(tri_count) if alias[k, 0:1].view(np.float32)[0] < 1.0)  # ... and nobody's alias
    rng = np.random.default_rng(3)
    n = 4096
    points = (rng.random((n, 3)) * [5.0, 3.0, 5.0] + [-2.5, 0.2, -2.5]).astype(np.float32)
    u = rng.random((n, 3)).astype(np.float32)
    results = []
    for path in (None, lib):
        r = _renderer(path, pool)
        try:
            r.upload(scene)
            frames = _frames(r, spp)
            results.append((frames, _light_query(r, points, u), r.scene_table(_ffi.TABLE_LIGHT_TRIANGLES)))
        finally:
            r.close()
    _assert_same(results[0][0], results[1][0], spp, pool, "fan")  # finite, spp samples in every pixel, films and counters equal
    assert results[0][0][0][..., :3].sum() > 0 and results[0][0][4]["nee_samples"] > 0
    for a, b in zip(results[0][1], results[1][1]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    rays, radiance, pdf = results[0][1]
    assert np.isfinite(pdf).all() and np.isfinite(radiance).all() and (pdf >= 0).all()
    hit = pdf > 0
    assert hit.sum() > n // 2 and np.isfinite(rays[hit]).all()
    # the samples whose random number draws the flat triangle's slot of the alias table must come out on its alias: their points spread over an area,
    # where the flat triangle is a segment
    tris = results[0][2].view(np.float32)
    assert tris[S.FAN_FLAT, 18] == 0.0 and tris[S.FAN_FLAT, 19] == 0.0 and (np.delete(tris[:, 18], S.FAN_FLAT) > 0).all()
    slot = hit & (np.floor(u[:, 1] * tri_count) == S.FAN_FLAT)  # (dev_shade.h: alias_slot of u_light_surface.x)
    assert slot.sum() > 100
    p = (rays[slot, 0:3] + rays[slot, 4:7] * rays[slot, 7:8]).astype(np.float64)
    spread = np.linalg.svd(p - p.mean(axis=0), compute_uv=False)
    print(f"fan ({'pool' if pool else 'one path'}): {int(hit.sum())} of {n} samples with a pdf, {int(slot.sum())} drew the flat triangle's slot; singular values of their points {spread}")
    assert spread[1] > 0.05 * spread[0]  # an area (the alias triangle), where a segment has one direction only
