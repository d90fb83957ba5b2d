"""Scenes shared by tests/test_gpu_light_record_tables.py and tests/test_gpu_light_records.py: `crowd`, the fixture in which the light sample's
records (csrc/hip/dev_scene.h: DLightInstance, DLightTri) and the `moved` bit masks of the device updates can go wrong where the suite's other
scenes cannot, and `fan`, its four-triangle emitter with a triangle without area in a small room of its own.  check_crowd asserts on the host
view that the scene has the properties it exists for."""
import numpy as np

from luisarender_amd import Scene

import light_record_reference as L

_ROOM = """
Shape room : InlineMesh { positions { -3,0,-3, 3,0,-3, 3,0,3, -3,0,3, -3,5,-3, 3,5,-3, 3,5,3, -3,5,3 }
  indices { 0,2,1, 0,3,2, 4,5,6, 4,6,7, 0,1,5, 0,5,4, 0,4,7, 0,7,3, 1,2,6, 1,6,5 } surface : Matte { Kd : Constant { v { 0.6, 0.6, 0.55 } } } }
"""
_TAIL = """
Camera cam : Pinhole { spp { SPP } film : Color { resolution { RES, RES } } position { 0, 2.5, 8.5 } look_at { 0, 2, 0 } fov { 40 } }
render { cameras { @cam } shapes { SHAPES } integrator : MegaPath { depth { 3 } sampler : Independent { seed { 11 } } } }
"""
_QUAD = "InlineMesh { positions { -0.5,0,-0.5, 0.5,0,-0.5, 0.5,0,0.5, -0.5,0,0.5 } indices { 0,1,2, 0,2,3 }"
# four triangles over five vertices; vertices 1 and 4 are EQUAL, so triangle 2 = (1, 4, 3) has two equal corners and no area
FAN = ("InlineMesh { positions { 0,0,0, 0.5,0,0, 0.5,0,0.6, 0,0,0.5, 0.5,0,0 } uvs { 0,0, 1,0, 1,1, 0,1, 1,0 } indices { 0,1,2, 0,2,3, 1,4,3, 4,2,3 }\n"
       "  light : Diffuse { emission : Constant { v { 7, 9, 11 } } two_sided { true } } transform : SRT { TRANSFORM } }")
FAN_TRIANGLES, FAN_FLAT = 4, 2  # triangles of the mesh; the primitive without area
# a mesh that no emitter shares (equal InlineMeshes share one mesh, so the plain quads share the emissive quads'): what lrhip_set_mesh_vertices may deform
_SLAB = "InlineMesh { positions { -0.5,0,-0.5, 0.5,0,-0.5, 0.6,0,0.2, 0,0,0.6, -0.6,0,0.2 } indices { 0,1,2, 0,2,3, 0,3,4 } surface : Matte { }"
SLAB_TRIANGLES, SLAB_VERTICES = 3, 5

QUADS = 320  # quad instances in the crowd, of them PLAIN without a light
# the quads without a light, by their position among the quads (the room is shape 0, so quad k is instance k + 1 where instance ids follow the
# order of the shapes: check_crowd asserts what matters, not this)
PLAIN = (4, 31, 40, 41, 63, 90, 150, 200, 255, 300)
SLABS = (40, 150)  # of them, instances of the slab mesh; a third one is the scene's last instance


def _shapes(shapes: list, spp: int, resolution: int) -> str:
    body = "".join(f"Shape {name} : {text}\n" for name, text in shapes)
    tail = _TAIL.replace("SPP", str(spp)).replace("RES", str(resolution)).replace("SHAPES", ", ".join(["@room"] + ["@" + n for n, _ in shapes]))
    return _ROOM + body + tail


def crowd_text(spp: int = 2, resolution: int = 16) -> str:
    shapes = []
    for k in range(QUADS):  # a 20 x 16 grid of small quads under the ceiling, every one under a matrix of its own
        x, z = -2.6 + 0.27 * (k % 20), -2.4 + 0.3 * (k // 20)
        srt = (f"transform : SRT {{ scale {{ {0.08 + 0.01 * (k % 7)}, 1, {0.1 + 0.015 * (k % 5)} }} rotate {{ {0.1 * (k % 3)}, 1, {0.05 * (k % 4)}, {7 * k % 360} }} "
               f"translate {{ {x:.3f}, {4.2 + 0.002 * k:.3f}, {z:.3f} }} }}")
        if k in SLABS:
            shapes.append((f"q{k}", f"{_SLAB} {srt} }}"))
        elif k in PLAIN:
            shapes.append((f"q{k}", f"{_QUAD} surface : Matte {{ Kd : Constant {{ v {{ 0.2, 0.6, 0.3 }} }} }} {srt} }}"))
        else:
            shapes.append((f"q{k}", f"{_QUAD} light : Diffuse {{ emission : Constant {{ v {{ {1 + k % 3}, {1 + k % 4}, {1 + k % 5} }} }} two_sided {{ true }} }} {srt} }}"))
    glow = "Sphere { subdivision { 2 } light : Diffuse { emission : Constant { v { 3, 2, 1 } } two_sided { true } } transform : SRT { %s } }"
    shapes.append(("glow_a", glow % "scale { 0.4, 0.3, 0.5 } rotate { 1, 1, 0, 35 } translate { -1.4, 2.2, 0.4 }"))
    shapes.append(("glow_m", glow % "scale { -1, 1, 1 } translate { 1.5, 1.2, -0.6 }"))  # mirrored: a negative determinant
    shapes.append(("ball", "Sphere { subdivision { 2 } surface : Matte { Kd : Constant { v { 0.7, 0.3, 0.2 } } } transform : SRT { scale { 0.5, 0.5, 0.5 } translate { 0.2, 0.5, 0.8 } } }"))
    shapes.append(("fan", FAN.replace("TRANSFORM", "scale { 1.5, 1, 2 } rotate { 1, 0, 0.3, 160 } translate { -0.4, 3.1, -0.2 }")))
    shapes.append(("card", f"{_SLAB} transform : SRT {{ translate {{ 0.25, 1.75, 1.0 }} }} }}"))
    return _shapes(shapes, spp, resolution)


def crowd(**kw) -> Scene:
    return Scene.from_string(crowd_text(**kw))


def fan_text(spp: int = 4, resolution: int = 24, sampler: str = "Independent") -> str:
    text = _shapes([("fan", FAN.replace("TRANSFORM", "scale { 3, 1, 3 } rotate { 1, 0, 0.2, 170 } translate { -0.8, 4.2, 0.6 }")),
                    ("card", f"{_QUAD} surface : Matte {{ }} transform : SRT {{ translate {{ 0.25, 1.0, 1.0 }} }} }}")], spp, resolution)
    return text.replace("sampler : Independent", f"sampler : {sampler}")


def check_crowd(scene: Scene) -> dict:
    """the properties the fixture is there for, on the host view -> {"lit": ids of the emitters, "plain": ids of the instances without a light,
    "quads_lit", "quads_plain", "slabs", "glow": the two emissive icosphere instances (unmirrored, mirrored), "ball", "fan", "room", "last", "tables"}"""
    t = L.host_tables(scene)
    inst = t["instances"]
    n = len(inst)
    lit = (inst[:, 0] & L.LR_SHAPE_HAS_LIGHT) != 0
    mesh = inst[:, 0] >> 10
    tri_count = t["meshes"][mesh, 3]
    assert 320 <= n <= 340, n
    for i in (31, 32, 63, 64, 255, 256):
        assert i < n
    assert lit[31] != lit[32] and lit[63] != lit[64]  # emitters and others on both sides of the first two boundaries between mask words
    assert lit[255] != lit[256]
    words = lambda ids: {int(i) >> 5 for i in ids}
    lights = t["light_instances"]
    assert len(lights) > 256 and sorted(lights[:, 0]) == list(np.nonzero(lit)[0])  # the light instance kernel's second block
    quads = tri_count == 2
    assert (quads & lit).sum() >= 300 and (quads & ~lit).sum() >= 8 and len(set(mesh[quads])) == 1
    assert words(np.nonzero(quads & ~lit)[0]) >= {0, 1, 2, 8}  # instances without a light that share the emitters' mesh, in many mask words
    slabs = np.nonzero(tri_count == SLAB_TRIANGLES)[0]
    assert len(slabs) == 3 and len(set(mesh[slabs])) == 1 and not lit[mesh == mesh[slabs[0]]].any() and slabs.min() >= 32  # a mesh without an emitter
    assert len(words(slabs)) == 3 and t["meshes"][mesh[slabs[0]], 1] == SLAB_VERTICES  # ... whose instances sit in three mask words behind the first
    balls = np.nonzero(tri_count == 320)[0]
    assert len(balls) == 3 and len(set(mesh[balls])) == 1 and lit[balls].sum() == 2  # one mesh: two emitters and a plain instance
    dets = [np.linalg.det(inst[i, 4:20].copy().view(np.float32).reshape(4, 4)[:3, :3].astype(np.float64)) for i in balls]
    glow = [int(i) for i, d in zip(balls, dets) if lit[i] and d > 0], [int(i) for i, d in zip(balls, dets) if lit[i] and d < 0]
    assert len(glow[0]) == 1 and len(glow[1]) == 1  # the mirrored emitter
    (fan,) = np.nonzero(tri_count == FAN_TRIANGLES)[0]
    fan_mesh = t["meshes"][mesh[fan]]
    assert lit[fan] and fan_mesh[0] > 0 and fan_mesh[2] > 0 and fan >= 32  # behind larger meshes: offsets that are not zero
    idx = t["triangles"][fan_mesh[2] + FAN_FLAT] + fan_mesh[0]
    corners = t["vertices"][idx, 0:3]
    assert (corners[0] == corners[1]).all() and float(t["tri_pdf"][fan_mesh[2] + FAN_FLAT:][:1].view(np.float32)[0]) == 0.0  # two equal corners, never chosen
    (room,) = np.nonzero(tri_count == 10)[0]
    assert not lit[n - 1] and (n - 1) >> 5 == 10
    return {"lit": [int(i) for i in np.nonzero(lit)[0]], "plain": [int(i) for i in np.nonzero(~lit)[0]], "quads_lit": [int(i) for i in np.nonzero(quads & lit)[0]],
            "quads_plain": [int(i) for i in np.nonzero(quads & ~lit)[0]], "glow": (glow[0][0], glow[1][0]), "ball": int(balls[~lit[balls]][0]), "fan": int(fan),
            "room": int(room), "slabs": [int(i) for i in slabs], "last": n - 1, "tables": t}
