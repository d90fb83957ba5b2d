"""Shared by tests/test_mesh_vertices.py and tests/test_gpu_mesh_vertices.py: the room of instance_scene.py with finer balls, the deformations the
tests apply to their mesh, and the normal recompute of lrhip_set_mesh_vertices in numpy float32 (which is unfused, like the host library)."""
import numpy as np

import instance_scene as S
from luisarender_amd import Scene

FLT_MAX = np.float32(3.402823466e+38)

# ---- the fixture: instance_scene.ROOM with both balls at subdivision 3.  The balls' mesh has 642 welded vertices, so a kernel with one
# thread per vertex runs two full blocks of 256 and a partial one of 130 (the 162-vertex ball of instance_scene never leaves one block);
# 2574 BVH triangles are no multiple of 64; the flat `card` quad keeps the scale-0 branch of the quantiser in play.  check_room asserts
# all of that on the host tables.
ROOM = S.ROOM.replace("subdivision { 2 }", "subdivision { 3 }")
assert ROOM.count("subdivision { 3 }") == 2
BALL_MESH = 1  # the room's box is mesh 0; the two balls share mesh 1
PARTIAL = (200, 500)  # vertices 200 .. 499: across vertices 256 and 512 of the mesh, 300 of them (one full block of threads and a partial one)


def room(lerp: bool = False, aov: bool = False) -> Scene:
    text = ROOM.replace("BALL_A", S._BALL_A_LERP if lerp else S._BALL_A).replace("SHUTTER", "shutter_span { 0, 1 } shutter_samples { 2 }" if lerp else "")
    return Scene.from_string(text.replace("INTEGRATOR", 'AOV { depth { 4 } components { "normal", "depth" } }' if aov else S._MEGAPATH))


def mesh_triangles(tables: dict, mesh: int) -> np.ndarray:
    """the index triples [T, 3] of a mesh, relative to the mesh's first vertex"""
    _, _, offset, count = (int(x) for x in tables["meshes"][mesh])
    return tables["triangles"][offset:offset + count].astype(np.int64)


def check_room(scene: Scene) -> dict:
    """the properties the fixture is there for, on the host tables -> instance ids {"ball_a", "ball_b", "lamp", "card", "room"} and mesh ids
    {"ball_mesh", "card_mesh", "lamp_mesh"}"""
    t = S.host_tables(scene)
    assert [int(x) for x in t["meshes"][BALL_MESH][[1, 3]]] == [642, 1280]
    mesh_of = t["instances"][:, 0] >> 10
    balls = [int(i) for i in np.nonzero(mesh_of == BALL_MESH)[0]]
    assert len(balls) == 2 and balls == S.instances_of_mesh(t, 1280)  # two instances share mesh 1
    assert all(int(t["instances"][i, 0]) & 1023 == 7 for i in balls)  # vertex normals, uvs, a surface; no light
    assert len(t["bvh_triangles"]) == 2574 and len(t["bvh_triangles"]) % 64 != 0
    nodes = t["bvh_nodes"]
    child = nodes[:, 24:28]
    level = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        for c in child[i][child[i] != S.INVALID]:
            if not c & S.LEAF:
                assert c > i
                level[c] = level[i] + 1
    assert len(nodes) == 1046 and level.max() + 1 == 10
    valence = np.bincount(mesh_triangles(t, BALL_MESH).reshape(-1), minlength=642)
    assert set(valence.tolist()) == {5, 6}
    S.check_tree(t)
    quads = S.instances_of_mesh(t, 2)
    lamp = [i for i in quads if t["instances"][i, 0] & 8]  # LR_SHAPE_HAS_LIGHT
    card = [i for i in quads if not t["instances"][i, 0] & 8]
    assert len(lamp) == 1 and len(card) == 1 and len(t["instances"]) == 5
    (rest,) = set(range(5)) - set(balls) - set(quads)
    return {"ball_a": balls[0], "ball_b": balls[1], "lamp": lamp[0], "card": card[0], "room": rest,
            "ball_mesh": BALL_MESH, "card_mesh": int(mesh_of[card[0]]), "lamp_mesh": int(mesh_of[lamp[0]])}


def first_deformation(p: np.ndarray) -> np.ndarray:
    """p' = float32(p (1 + 0.25 sin(3 p.y))): with it the smallest squared length the normal recompute divides by is 1.2e-3"""
    p = p.astype(np.float64)
    return np.ascontiguousarray((p * (1.0 + 0.25 * np.sin(3.0 * p[:, 1:2]))).astype(np.float32))


def second_deformation(p: np.ndarray) -> np.ndarray:
    """p' = float32(p + 0.1 sin(5 p.zxy))"""
    p = p.astype(np.float64)
    return np.ascontiguousarray((p + 0.1 * np.sin(5.0 * p[:, [2, 0, 1]])).astype(np.float32))


def numpy_normals(positions: np.ndarray, triangles: np.ndarray, normals: np.ndarray) -> tuple:
    """the definition of LRHIP_MESH_RECOMPUTE_NORMALS as a float32 loop: s[v] = s[v] + cross(p1 - p0, p2 - p0) over the triangles in ascending
    order and their corners in ascending order, l2 = (sx sx + sy sy) + sz sz, n = s / sqrt(l2) where 0 < l2 <= FLT_MAX, else the normal
    stays -> (normals [V, 3], l2 [V])"""
    p = positions.astype(np.float32)
    s = np.zeros_like(p)
    for tri in triangles:
        a, b = p[tri[1]] - p[tri[0]], p[tri[2]] - p[tri[0]]
        c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float32)
        for v in tri:
            s[v] = s[v] + c
    l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    assert l2.dtype == np.float32
    ok = (l2 > 0) & (l2 <= FLT_MAX)
    out = normals.astype(np.float32).copy()
    out[ok] = s[ok] / np.sqrt(l2[ok])[:, None]
    return out, l2


def vertex_words(scene: Scene, mesh: int) -> np.ndarray:
    """the mesh's lr_vertex records in the host view, as 32-bit words [V, 8]"""
    t = S.host_tables(scene)
    offset, count = int(t["meshes"][mesh][0]), int(t["meshes"][mesh][1])
    return t["vertices"][offset:offset + count]
