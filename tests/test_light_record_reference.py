"""The float64 restatement of the light sample's records (tests/light_record_reference.py) tested on its own: closed forms, the layout rules,
the band arithmetic on a hand-made sliver, and that the judge can fail -- it accepts a float32 restatement of dev_shade.h: triangle_constants
and rejects a wrong column, a wrong vertex offset, a transposed uv pair, a wrong tri_base and a normal that is off by a few bands.  No GPU."""
import numpy as np
import pytest

import light_record_reference as L

F = np.float32
HAS_LIGHT, HAS_SURFACE = 8, 4


def _u(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _scene(meshes, instances, lights):
    """meshes: [(positions [n, 3], uvs [n, 2], triangles [m, 3])]; instances: [(mesh, flags, matrix [4, 4] column-major)]; lights: instance ids"""
    vertices, triangles, table, pdf = [], [], [], []
    for positions, uvs, tris in meshes:
        table.append((sum(len(v) for v in vertices), len(positions), sum(len(t) for t in triangles), len(tris)))
        v = np.zeros((len(positions), 8), np.float32)
        v[:, 0:3], v[:, 3:6], v[:, 6:8] = positions, (0, 1, 0), uvs
        vertices.append(v)
        triangles.append(np.asarray(tris, np.uint32))
        corners = np.asarray(positions, np.float64)[np.asarray(tris)]
        area = np.linalg.norm(np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]), axis=1)
        pdf.append((area / area.sum()).astype(np.float32))  # a triangle without area is never chosen
    inst = np.zeros((len(instances), 24), np.uint32)
    for i, (mesh, flags, matrix) in enumerate(instances):
        inst[i, 0:4] = (mesh << 10) | flags, 0x123000 + i, table[mesh][3], 0x40 + i
        inst[i, 4:20] = _u(matrix).reshape(16)
    return {"instances": inst, "meshes": np.array(table, np.uint32), "triangles": np.concatenate(triangles), "vertices": _u(np.concatenate(vertices)),
            "tri_pdf": _u(np.concatenate(pdf)), "light_instances": np.array([(i, 7) for i in lights], np.uint32).reshape(-1, 2)}


def _matrix(m3=np.eye(3), t=(0, 0, 0)):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = m3, t
    return np.ascontiguousarray(m.T.astype(np.float32))


def _rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


QUAD = (np.array([(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)], F), np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F), [(0, 2, 1), (0, 3, 2)])
BIG = (np.arange(30, dtype=F).reshape(10, 3) ** 2 % 7, np.arange(20, dtype=F).reshape(10, 2) / 20, [(0, 1, 2), (3, 4, 5), (6, 7, 8), (1, 5, 9), (2, 4, 6)])
FAN = (np.array([(0, 0, 0), (1, 0, 0), (0.5, 0, 1), (1, 0, 0), (2, 1, 0.25)], F), np.array([(0.1, 0.2), (0.3, 0.4), (0.5, 0.6), (0.7, 0.8), (0.9, 1.0)], F),
       [(0, 2, 1), (1, 3, 4), (1, 2, 4)])  # vertices 1 and 3 coincide: the second triangle has no area


def _device(tables, matrices=None):
    """dev_shade.h: triangle_constants and the two record kernels restated in numpy float32 (unfused): (instance words, triangle words)"""
    e = L.expected(tables, matrices)
    inst = tables["instances"]
    if matrices is None:
        matrices = inst[:, 4:20].copy().view(F).reshape(-1, 4, 4)
    tris = np.zeros((len(e["copies"]), L.TRI_WORDS), np.uint32)
    tris[:, L.TRI_COPY_WORDS] = e["copies"]
    f = tris.view(F)
    for t in range(len(tris)):
        m = matrices[e["instances"][e["owner"][t], 0]]
        p0, p1, p2 = f[t, 0:3], f[t, 4:7], f[t, 8:11]
        mul = lambda v: (m[0, :3] * v[0] + m[1, :3] * v[1]) + m[2, :3] * v[2]
        a, b = mul(p1 - p0), mul(p2 - p0)
        c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)
        dot = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            f[t, L.TRI_NG_WORDS] = c * (F(1) / np.sqrt(dot))
        f[t, L.TRI_AREA_WORD] = np.sqrt(dot) * F(0.5)
    return e["instances"].copy(), tris, e


def test_the_count_is_the_sum_of_the_counted_lines():
    factor = 1 + 3
    cross = 2 * factor + 1 + 1
    length, half, normalize, product = 3 + 2, 1, 3 + 2 + 2 + 1, 1
    assert L.ROUNDINGS == cross + length + half + normalize + product == 25 and L.UNIT == 2.0 ** -24 and L.NG_LENGTH_ULPS == 4


@pytest.mark.parametrize("a, b", [(2.0, 3.0), (0.25, 7.0), (1.5, 0.4)])
def test_a_scaled_unit_quad(a, b):
    """scale(a, 1, b) of the unit quad in the xz plane: both triangles have area a b / 2 and ng = +y for (0, 2, 1) / (0, 3, 2)"""
    e = L.expected(_scene([QUAD], [(0, HAS_LIGHT, _matrix(np.diag([a, 1.0, b])))], [0]))
    assert np.allclose(e["cross"], [[0, a * b, 0]] * 2, rtol=1e-7, atol=0) and not e["degenerate"].any()
    area = np.linalg.norm(e["cross"], axis=1) / 2
    assert np.allclose(area, F(a) * np.float64(F(b)) / 2, rtol=1e-15)
    # a mirrored matrix flips the normal and keeps the area; a rotation keeps the area and turns the normal with it
    mirrored = L.expected(_scene([QUAD], [(0, HAS_LIGHT, _matrix(np.diag([-a, 1.0, b])))], [0]))
    assert np.array_equal(mirrored["cross"], -e["cross"])
    r = _rotation((1, 2, 3), 40.0)
    turned = L.expected(_scene([QUAD], [(0, HAS_LIGHT, _matrix(r @ np.diag([a, 1.0, b])))], [0]))
    assert np.allclose(np.linalg.norm(turned["cross"], axis=1) / 2, area, rtol=1e-6)
    assert np.allclose(turned["cross"] / np.linalg.norm(turned["cross"], axis=1, keepdims=True), [r[:, 1]] * 2, atol=1e-6)
    # the translation column does not enter
    moved = L.expected(_scene([QUAD], [(0, HAS_LIGHT, _matrix(np.diag([a, 1.0, b]), (5, -3, 9)))], [0]))
    assert np.array_equal(moved["cross"], e["cross"]) and np.array_equal(moved["band"], e["band"])


def _layout_scene():
    return _scene([BIG, QUAD, FAN], [(0, HAS_SURFACE, _matrix()), (2, HAS_LIGHT | HAS_SURFACE, _matrix(_rotation((0, 1, 1), 20), (1, 2, 3))),
                                     (1, HAS_SURFACE, _matrix()), (1, HAS_LIGHT, _matrix(np.diag([2.0, 1, 3]))), (2, HAS_LIGHT, _matrix(np.diag([-1.0, 1, 1])))],
                  [3, 1, 4])


def test_the_layout_rules():
    t = _layout_scene()
    e = L.expected(t)
    r = e["instances"]
    assert r.shape == (3, 24) and list(r[:, 0]) == [3, 1, 4]  # the light instance list's order, not the instances'
    assert list(r[:, 1]) == [5, 7, 7] and list(r[:, 2]) == [2, 3, 3]  # the mesh's triangle offset and count
    assert list(r[:, 3]) == [0, 2, 5] and len(e["copies"]) == 8 and list(e["owner"]) == [0, 0, 1, 1, 1, 2, 2, 2]  # tri_base: the running sum
    assert list(r[:, 4]) == [HAS_LIGHT, HAS_LIGHT | HAS_SURFACE, HAS_LIGHT] and list(r[:, 5]) == [0x123003, 0x123001, 0x123004]
    assert list(r[:, 6]) == [0x43, 0x41, 0x44] and not r[:, [7, 11, 15, 19, 23]].any()
    assert np.array_equal(r[1, 20:23].view(F), F([1, 2, 3])) and np.array_equal(r[0, 8:11].view(F), F([2, 0, 0]))
    # the FAN mesh sits behind 14 vertices and 7 triangles: record 2 is its first triangle (0, 2, 1) read THROUGH those offsets
    assert np.array_equal(e["copies"][2, 0:9].view(F), F([0, 0, 0, 0.5, 0, 1, 1, 0, 0]))
    assert np.array_equal(e["copies"][2, 9:15].view(F), F([0.1, 0.2, 0.5, 0.6, 0.3, 0.4]))
    assert e["copies"][2, 15] == t["tri_pdf"][7] and e["copies"][0, 15] == t["tri_pdf"][5]
    # one mesh under two instances: the same copies, other cross products; the coincident vertices give one flat triangle per instance
    assert np.array_equal(e["copies"][2:5], e["copies"][5:8]) and not np.array_equal(e["cross"][2:5], e["cross"][5:8])
    assert list(np.nonzero(e["degenerate"])[0]) == [3, 6]
    # other matrices: only the columns and the computed values follow
    m = t["instances"][:, 4:20].copy().view(F).reshape(-1, 4, 4)
    m[3] = _matrix(np.diag([1.0, 1, 1]), (9, 9, 9))
    e2 = L.expected(t, m)
    assert np.array_equal(e2["copies"], e["copies"]) and np.array_equal(e2["instances"][1:], e["instances"][1:])
    assert np.array_equal(e2["instances"][0, 20:23].view(F), F([9, 9, 9])) and np.array_equal(e2["cross"][0], [0, 1, 0])
    with pytest.raises(AssertionError):  # a light instance list that names an instance without a light
        L.expected(dict(t, light_instances=np.array([(0, 7)], np.uint32)))
    empty = L.expected(dict(t, light_instances=np.zeros((0, 2), np.uint32)))
    assert empty["instances"].shape == (0, 24) and empty["copies"].shape == (0, 16) and empty["cross"].shape == (0, 3)


def test_the_band_on_a_sliver():
    """p0 = (1, 0, 1), p1 = (3, 0, 1), p2 = (2, 0, 1 + 2^-20) under scale(1, 1, 1): A = (2, 0, 0), B = (1, 0, 2^-20); c = (0, -2^-19, 0); the expanded
    terms of c.y = A.z B.x - A.x B.z: |A|.z = 1 + 1 = 2, |B|.x = 2 + 1 = 3, |A|.x = 3 + 1 = 4, |B|.z = (1 + 2^-20) + 1 -> 6 + 4 (2 + 2^-20)"""
    tiny = 2.0 ** -20
    sliver = (np.array([(1, 0, 1), (3, 0, 1), (2, 0, 1 + tiny)], F), np.zeros((3, 2), F), [(0, 1, 2)])
    e = L.expected(_scene([sliver], [(0, HAS_LIGHT, _matrix())], [0]))
    assert np.array_equal(e["cross"], [[0.0, -2 * tiny, 0.0]])
    want = 6 + 4 * (2 + tiny)
    assert np.array_equal(e["band"], L.ROUNDINGS * L.UNIT * np.array([[0.0, want, 0.0]]))
    # the band is wider than the cross product itself (25 x 2^-24 x 14 against 2^-19: eleven times): what makes ng of a sliver ill-conditioned,
    # and why ng is not compared
    assert 10 < e["band"][0, 1] / (2 * tiny) < 12
    # the judge holds x and z, whose terms all vanish, to exactly zero
    inst, tris, _ = _device(_scene([sliver], [(0, HAS_LIGHT, _matrix())], [0]))
    assert L.judge_triangles(tris, e, 0) <= 1.0
    tilted = tris.copy()
    tilted.view(F)[0, 3] = 1e-3
    with pytest.raises(AssertionError, match="2 area ng"):
        L.judge_triangles(tilted, e, 0)


def test_the_judge_accepts_the_float32_restatement_and_rejects_wrong_ones():
    t = _layout_scene()
    inst, tris, e = _device(t)
    L.judge_instances(inst, e)
    ratio = L.judge_triangles(tris, e, 2)
    assert 0.0 <= ratio < 0.5  # unfused fp32 with correctly rounded operations stays far inside a band that counts every rounding as its worst
    L.judge_triangles(tris.view(np.uint8).reshape(len(tris), 80), e, 2)  # the bytes as lrhip_read_scene_table hands them out
    with pytest.raises(AssertionError):  # a degenerate record nobody declared
        L.judge_triangles(tris, e, 0)

    def wrong(words, value=None, table="tris"):
        bad = (tris if table == "tris" else inst).copy()
        for k, (row, word) in enumerate(words):
            bad[row, word] = value[k] if value is not None else bad[row, word] ^ 1
        return bad

    with pytest.raises(AssertionError, match="copied words"):  # a transposed uv pair
        L.judge_triangles(wrong([(2, 12), (2, 13)], [tris[2, 13], tris[2, 12]]), e, 2)
    with pytest.raises(AssertionError, match="copied words"):  # the vertex of another mesh: offset 0 instead of the mesh's own
        L.judge_triangles(wrong([(5, 4), (5, 5), (5, 6)], t["vertices"][2, 0:3]), e, 2)
    with pytest.raises(AssertionError, match="copied words"):  # one bit of tri_pdf
        L.judge_triangles(wrong([(7, 19)]), e, 2)
    with pytest.raises(AssertionError, match="without area"):  # an area on the flat triangle
        L.judge_triangles(wrong([(3, 18)], [np.uint32(0x3F800000)]), e, 2)
    flipped = tris.copy()
    flipped[5:8, 3] ^= 0x80000000  # ng.x of the mirrored instance with the sign of the unmirrored one
    with pytest.raises(AssertionError, match="2 area ng"):
        L.judge_triangles(flipped, e, 2)
    scaled = tris.copy()
    scaled.view(F)[0, 18] *= F(1 + 2.0 ** -17)  # an area off by 64 ulp: |c| 2 (1 + ...) against terms of the same size and 25 units of 2^-24
    with pytest.raises(AssertionError, match="2 area ng"):
        L.judge_triangles(scaled, e, 2)
    long = tris.copy()
    long.view(F)[0, 7] = np.nextafter(long.view(F)[0, 7], F(2), dtype=F)  # inside the band, outside the length rule?  no: 1 ulp of 1.0 is allowed
    L.judge_triangles(long, e, 2)
    with pytest.raises(AssertionError, match="light instance records"):  # tri_base
        L.judge_instances(wrong([(1, 3)], table="inst"), e)
    with pytest.raises(AssertionError, match="light instance records"):  # a column's row
        L.judge_instances(wrong([(2, 9)], table="inst"), e)
    with pytest.raises(AssertionError, match="light instance records"):  # a pad word that is not zero
        L.judge_instances(wrong([(0, 23)], table="inst"), e)
    with pytest.raises(AssertionError):  # a record too few
        L.judge_triangles(tris[:-1], e, 2)


def test_records_under_other_matrices_follow_the_restatement():
    t = _layout_scene()
    m = t["instances"][:, 4:20].copy().view(F).reshape(-1, 4, 4)
    m[1] = _matrix(_rotation((3, 1, 2), 200.0) @ np.diag([0.3, 2.0, 1.1]), (-1, 0.5, 2))
    inst, tris, e = _device(t, m)
    L.judge_instances(inst, e)
    assert L.judge_triangles(tris, e, 2) < 0.5
    stale, _, _ = _device(t)  # the records of the matrices before the move
    with pytest.raises(AssertionError, match="light instance records"):
        L.judge_instances(stale, e)
    with pytest.raises(AssertionError, match="2 area ng"):
        L.judge_triangles(_device(t)[1], e, 2)
