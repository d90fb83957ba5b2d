"""Shared by tests/test_instance_transforms.py and tests/test_gpu_instance_transforms.py: scenes whose instances the tests move, numpy copies of
the host tables that move with them, and the bake / containment checks in numpy float32 (which is unfused, like the host library)."""
import ctypes as C

import numpy as np

from luisarender_amd import Scene

INVALID = 0xFFFFFFFF
LEAF = 0x80000000

# two instances of one icosphere mesh (Sphere shapes of one subdivision level share their mesh) and a static floor
TWO_BALLS = """
Shape ball_a : Sphere { subdivision { 1 } surface : Matte { Kd : Constant { v { 0.7, 0.3, 0.2 } } } transform : SRT { translate { -1.25, 1, 0 } } }
Shape ball_b : Sphere { subdivision { 1 } surface : Matte { Kd : Constant { v { 0.2, 0.3, 0.7 } } } transform : SRT { scale { 0.5, 0.5, 0.5 } translate { 1.5, 0.5, 0.25 } } }
Shape floor : InlineMesh { positions { -4,0,-4, 4,0,-4, 4,0,4, -4,0,4 } indices { 0,2,1, 0,3,2 } surface : Matte { } }
Shape lamp : InlineMesh { positions { -1,4,-1, 1,4,-1, 1,4,1, -1,4,1 } indices { 0,1,2, 0,2,3 }
  light : Diffuse { emission : Constant { v { 9 } } two_sided { true } } }
Camera cam : Pinhole { spp { 4 } film : Color { resolution { 16, 16 } } position { 0, 2, 7 } look_at { 0, 1, 0 } fov { 40 } }
render { cameras { @cam } shapes { @ball_a, @ball_b, @floor, @lamp } integrator : MegaPath { depth { 3 } sampler : Independent { seed { 5 } } } }
"""

# a ball on a Lerp transform (rotation, scale and translation all move) beside a static one
LERP_BALLS = TWO_BALLS.replace(
    "transform : SRT { translate { -1.25, 1, 0 } }",
    "transform : Lerp { time_points { 0, 1 } transforms { SRT { scale { 1, 1.5, 0.75 } rotate { 0, 0, 1, 10 } translate { -1.25, 1, 0 } }, "
    "SRT { scale { 0.5, 1, 1.25 } rotate { 0, 1, 0, 80 } translate { 0.5, 1.5, -1 } } } }").replace(
    "fov { 40 }", "fov { 40 } shutter_span { 0, 1 } shutter_samples { 2 }")


def srt(scale=(1, 1, 1), axis=(0, 0, 1), degrees=0.0, translate=(0, 0, 0)) -> np.ndarray:
    """translation x rotation x non-uniform scale as a float32 matrix in COLUMN-MAJOR storage [4, 4] ([c, r]: what set_instance_transforms takes)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = (np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)) @ np.diag(np.asarray(scale, np.float64))
    m[:3, 3] = translate
    return np.ascontiguousarray(m.T.astype(np.float32))


def _words(ptr, count, record_bytes) -> np.ndarray:
    if count == 0:
        return np.zeros((0, record_bytes // 4), np.uint32)
    return np.frombuffer(C.string_at(ptr, count * record_bytes), np.uint32).reshape(count, record_bytes // 4).copy()


def host_tables(scene: Scene) -> dict:
    """copies of the host tables as 32-bit words: instances [n, 24] (handle 0:4, object_to_world 4:20), bvh_triangles [n, 12] (v0 0:3, inst 3,
    e1 4:7, prim 7, e2 8:11, flags 11), bvh_nodes [n, 32] (lo_x 0:4 lo_y lo_z hi_x hi_y hi_z 20:24, child 24:28), meshes, triangles, vertices"""
    v = scene.view()
    return {"instances": _words(v.instances, v.instance_count, 96), "bvh_triangles": _words(v.accel.triangles, v.accel.triangle_count, 48),
            "bvh_nodes": _words(v.accel.nodes, v.accel.node_count, 128), "meshes": _words(v.meshes, v.mesh_count, 16),
            "triangles": _words(v.triangles, v.triangle_count, 12), "vertices": _words(v.vertices, v.vertex_count, 32)}


def instance_matrices(scene: Scene) -> np.ndarray:
    """the scene's object_to_world matrices as set_instance_transforms takes them: float32 [n, 4, 4], column-major"""
    return np.ascontiguousarray(host_tables(scene)["instances"][:, 4:20].view(np.float32).reshape(-1, 4, 4))


def instances_of_mesh(tables: dict, triangle_count: int) -> list:
    """ids of the instances whose mesh has `triangle_count` triangles"""
    mesh = tables["instances"][:, 0] >> 10
    return [int(i) for i in range(len(mesh)) if tables["meshes"][mesh[i], 3] == triangle_count]


def numpy_bake(tables: dict, matrices: np.ndarray) -> np.ndarray:
    """the baked triangles [n, 9] (v0, e1, e2) of every BVH triangle under `matrices` [instances, 4, 4] (column-major), in the order the host
    writes: p = ((c0 x + c1 y) + c2 z) + c3 (lr_math.h: operator*(float4x4, float4)), e1 = p1 - p0, e2 = p2 - p0; numpy float32 is unfused"""
    bt = tables["bvh_triangles"]
    inst, prim = bt[:, 3], bt[:, 7]
    mesh = tables["meshes"][tables["instances"][inst, 0] >> 10]
    tri = tables["triangles"][mesh[:, 2] + prim]
    m = matrices[inst].astype(np.float32)  # [n, c, r]
    p = []
    for k in range(3):
        v = tables["vertices"][mesh[:, 0] + tri[:, k]].view(np.float32)
        x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
        p.append(((m[:, 0, :3] * x + m[:, 1, :3] * y) + m[:, 2, :3] * z) + m[:, 3, :3])
    return np.concatenate([p[0], p[1] - p[0], p[2] - p[0]], axis=1)


def baked(tables: dict) -> np.ndarray:
    """[n, 9] float32 (v0, e1, e2) of the host's or the device's 48-byte triangle records as 32-bit words"""
    bt = tables["bvh_triangles"] if isinstance(tables, dict) else tables
    return bt[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].view(np.float32)


def check_tree(tables: dict) -> None:
    """every child box holds the three corners (p0, p0 + e1, p0 + e2: the refit's own) of every triangle below it, exactly; the walk from the
    root reaches every triangle once and every node once"""
    nodes, bt = tables["bvh_nodes"], tables["bvh_triangles"]
    f = bt.view(np.float32)
    p0 = f[:, 0:3]
    corners = np.stack([p0, p0 + f[:, 4:7], p0 + f[:, 8:11]], axis=1)  # [n, 3, 3]
    seen_tri = np.zeros(len(bt), np.int64)
    seen_node = np.zeros(len(nodes), np.int64)

    def walk(ni):
        seen_node[ni] += 1
        below = []
        boxes = nodes[ni, 0:24].view(np.float32).reshape(6, 4)
        for k in range(4):
            c = int(nodes[ni, 24 + k])
            if c == INVALID:
                continue
            if c & LEAF:
                assert (c >> 27) & 15 == 0
                tris = [c & 0x7FFFFFF]
                seen_tri[tris[0]] += 1
            else:
                tris = walk(c)
            pts = corners[tris].reshape(-1, 3)
            assert (pts >= boxes[0:3, k]).all() and (pts <= boxes[3:6, k]).all(), (ni, k)
            below += tris
        return below

    walk(0)
    assert (seen_tri == 1).all() and (seen_node == 1).all()


# ---- the fixture of the GPU tests, the smallest scene in which each stage of the device path can go wrong: a box room; two instances of one
# 320-triangle mesh (654 BVH triangles in all: no multiple of 64, a tree of 9 levels); an emissive quad as an instance of its own; an
# axis-aligned flat quad whose two triangles share a node of zero extent in y (the scale-0 branch of the quantiser; the room's back wall
# gives one in z); nodes with empty slots.  check_room asserts all of that on the host tables.
ROOM = """
Shape room : InlineMesh { positions { -3,0,-3, 3,0,-3, 3,0,3, -3,0,3, -3,5,-3, 3,5,-3, 3,5,3, -3,5,3 }
  indices { 0,2,1, 0,3,2, 4,5,6, 4,6,7, 0,1,5, 0,5,4, 0,4,7, 0,7,3, 1,2,6, 1,6,5 } surface : Matte { Kd : Constant { v { 0.6, 0.6, 0.55 } } } }
Shape ball_a : Sphere { subdivision { 2 } surface : Matte { Kd : Constant { v { 0.7, 0.3, 0.2 } } } transform : BALL_A }
Shape ball_b : Sphere { subdivision { 2 } surface : Mirror { } transform : SRT { scale { 0.5, 0.5, 0.5 } translate { 1.5, 0.5, 0.25 } } }
Shape lamp : InlineMesh { positions { -0.75,4.9,-0.75, 0.75,4.9,-0.75, 0.75,4.9,0.75, -0.75,4.9,0.75 } indices { 0,1,2, 0,2,3 }
  light : Diffuse { emission : Constant { v { 12, 11, 9 } } } }
Shape card : InlineMesh { positions { -0.5,0,-0.5, 0.5,0,-0.5, 0.5,0,0.5, -0.5,0,0.5 } indices { 0,2,1, 0,3,2 }
  surface : Matte { Kd : Constant { v { 0.2, 0.6, 0.3 } } } transform : SRT { translate { 0.25, 1.75, 1.0 } } }
Camera cam : Pinhole { spp { 8 } film : Color { resolution { 32, 32 } } position { 0, 2.5, 8.5 } look_at { 0, 2, 0 } fov { 40 } SHUTTER }
render { cameras { @cam } shapes { @room, @ball_a, @ball_b, @lamp, @card } integrator : INTEGRATOR }
"""
_BALL_A = "SRT { scale { 0.8, 0.8, 0.8 } translate { -1.25, 0.8, 0 } }"
_BALL_A_LERP = ("Lerp { time_points { 0, 1 } transforms { SRT { scale { 0.8, 0.8, 0.8 } translate { -1.25, 0.8, 0 } }, "
                "SRT { scale { 0.5, 1, 0.75 } rotate { 1, 1, 0, 70 } translate { 0.5, 1.5, -1 } } } }")
_MEGAPATH = "MegaPath { depth { 4 } sampler : Independent { seed { 11 } } }"


def room(lerp: bool = False, aov: bool = False) -> Scene:
    text = ROOM.replace("BALL_A", _BALL_A_LERP if lerp else _BALL_A).replace("SHUTTER", "shutter_span { 0, 1 } shutter_samples { 2 }" if lerp else "")
    return Scene.from_string(text.replace("INTEGRATOR", 'AOV { depth { 4 } components { "normal", "depth" } }' if aov else _MEGAPATH))


def check_room(scene: Scene) -> dict:
    """the properties the fixture is there for, on the host tables -> {"ball_a", "ball_b", "lamp", "card", "room"}: instance ids"""
    t = host_tables(scene)
    nodes = t["bvh_nodes"]
    child = nodes[:, 24:28]
    valid = child != INVALID
    assert len(t["bvh_triangles"]) == 654 and len(t["bvh_triangles"]) % 64 != 0
    assert (~valid).any(axis=1).sum() > 0  # nodes with an empty slot
    boxes = nodes[:, 0:24].view(np.float32).reshape(-1, 6, 4)
    flat = [(i, ax) for i in range(len(nodes)) for ax in range(3) if boxes[i, ax][valid[i]].min() == boxes[i, 3 + ax][valid[i]].max()]
    assert flat  # a node without extent on an axis: its packet has scale 0 there
    level = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        for c in child[i][valid[i]]:
            if not c & LEAF:
                assert c > i  # children behind their parents: what the refit's order rests on
                level[c] = level[i] + 1
    assert level.max() + 1 >= 3
    check_tree(t)
    balls = instances_of_mesh(t, 320)
    quads = instances_of_mesh(t, 2)
    assert len(balls) == 2 and len(quads) == 2 and len(t["instances"]) == 5
    lamp = [i for i in quads if t["instances"][i, 0] & 8]  # LR_SHAPE_HAS_LIGHT
    card = [i for i in quads if not t["instances"][i, 0] & 8]
    assert len(lamp) == 1 and len(card) == 1
    (rest,) = set(range(5)) - set(balls) - set(quads)
    return {"ball_a": balls[0], "ball_b": balls[1], "lamp": lamp[0], "card": card[0], "room": rest}
