"""A float64 restatement of the light sample's records (csrc/hip/dev_scene.h: DLightInstance, DLightTri), for tests/test_light_record_reference.py
(which tests this module on the CPU) and tests/test_gpu_light_record_tables.py (which judges the device's three tables with it).

It works from the HOST scene view alone -- the instances' handles and object-to-world columns, the meshes' offsets, lr_vertex, lr_triangle,
tri_pdf, the light instance list -- and, for a given set of matrices, states what the two tables must hold:

  * the LAYOUT: one DLightInstance per entry of the light instance list, in its order; one DLightTri per (light instance, primitive of its
    mesh), instance after instance; tri_base = the running sum of the counts in front;
  * the COPIES, compared as 32-bit words, exactly: the whole 96-byte instance record (instance id, alias_base = the mesh's triangle offset,
    alias_count = handle.z, tri_base; handle.x & 1023, handle.y, handle.w, 0; the four columns with a zero fourth word each), and of a
    triangle record p0 p1 p2 in object space, the three uv pairs and tri_pdf (17 of its 20 words);
  * the two COMPUTED values, ng and area.  ng is ill-conditioned for slivers, so what is compared is the cross product a record implies,
    c_dev = 2 area ng, per component, with c = cross(M (p1 - p0), M (p2 - p0)) evaluated in float64 on the same fp32 inputs, inside an
    absolute band stated BEFORE any device run (below); and | |ng| - 1 | <= 4 ulp wherever |c| > 0.

No record is left out.  A triangle whose float64 cross product is exactly zero has no normal: such records are counted (the caller says how
many its scene was built with), and are held to area == 0 and tri_pdf == 0; their ng is not specified.

THE BAND.  Per component, ROUNDINGS x 2^-24 x the sum of the absolute values of the fully expanded terms of that component -- every product
m_i[r] p_k[i] m_j[s] p_l[j] that c[x] = A[y] B[z] - A[z] B[y] expands into with A = M (p1 - p0), B = M (p2 - p0) -- the form of
tests/raycast_judge.py's bands.  ROUNDINGS is counted from the source (dev_shade.h: triangle_constants; dev_math.h: cross, length, normalize),
one unit = one correctly rounded fp32 operation = a relative 2^-24, along the LONGEST path from an input to the value:

    dp = p1 - p0                                       1
    mul(dp)[r] = (m0[r] dp.x + m1[r] dp.y) + m2[r] dp.z   a product and two sums: 3       -> a factor A[r] or B[s]: 4
    cross: A[y] B[z] - A[z] B[y]                       4 + 4 (the factors), the product 1, the difference 1    -> 10
    length(c): dot = (c.x c.x + c.y c.y) + c.z c.z     3 (the component's own error is in the 10; first order, and the root halves these)
               sqrtf                                   2 (*)
    * .5f                                              1 (exact in the normal range; counted)
    normalize(c): dot 3, sqrtf 2 (*), 1.0f / x 2 (*), a * s 1                                                  -> 8
    the test's own 2 area ng (float64 here; counted as one fp32 rounding)                                      1
                                                                                                        sum:  25

(*) the library's own flags (HIPFLAGS: -fno-hip-fp32-correctly-rounded-divide-sqrt -fapprox-func) turn sqrtf and the division into
v_sqrt_f32 / v_rcp_f32 / v_rsq_f32, which the ISA documents to 1 ulp = two units; the exact-arithmetic unit rounds them correctly (one unit).
Contraction (HIPFLAGS allows it, the exact unit does not) only REMOVES roundings.  So one count serves both tables, and it is the larger one.
The errors of length and normalize are relative to |c| and to the component; both are below the component's sum of absolute terms.  Neither
the count nor the band is fitted to a device.  Values near the denormal range are outside this model: `expected` refuses inputs whose
non-zero sums of absolute terms fall below 2^-60.

MEASURED_DEVICE_ERROR records the largest |c_dev - c| / band seen per table; it is a record of a run, not a bound: the bound is 1.0."""
import numpy as np

ROUNDINGS = 25  # counted above, line by line
UNIT = 2.0 ** -24
NG_LENGTH_ULPS = 4  # | |ng| - 1 | in ulps of 1.0f (2^-23)
# largest error / band per table over every scene and moment of tests/test_gpu_light_record_tables.py, which prints them: one run of that
# file on an MI355X (gfx950, ROCm 7.2) with the change that added it (light_tris: `crowd`; light_tris_exact: `two_instances`).
MEASURED_DEVICE_ERROR = {"light_tris": 0.0477, "light_tris_exact": 0.0483}

INSTANCE_WORDS, TRI_WORDS = 24, 20
TRI_COPY_WORDS = [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 15, 16, 17, 19]  # p0 p1 p2, uv0 uv1 uv2, tri_pdf
TRI_NG_WORDS, TRI_AREA_WORD, TRI_PDF_WORD = [3, 7, 11], 18, 19
LR_SHAPE_HAS_LIGHT = 8


def host_tables(scene) -> dict:
    """copies of the host view's tables as 32-bit words: instances [n, 24] (handle 0:4, object_to_world 4:20, column-major), meshes [n, 4]
    (vertex offset, count, triangle offset, count), triangles [n, 3], vertices [n, 8] (p 0:3, n 3:6, uv 6:8), tri_pdf [n], light_instances [n, 2]"""
    import ctypes as C
    v = scene.view()

    def words(ptr, count, record_bytes):
        if count == 0:
            return np.zeros((0, record_bytes // 4), np.uint32)
        return np.frombuffer(C.string_at(ptr, count * record_bytes), np.uint32).reshape(count, record_bytes // 4).copy()

    return {"instances": words(v.instances, v.instance_count, 96), "meshes": words(v.meshes, v.mesh_count, 16),
            "triangles": words(v.triangles, v.triangle_count, 12), "vertices": words(v.vertices, v.vertex_count, 32),
            "tri_pdf": words(v.tri_pdf, v.triangle_count, 4)[:, 0], "light_instances": words(v.light_instances, v.light_instance_count, 8)}


def expected(tables: dict, matrices=None) -> dict:
    """what the tables must hold under `matrices` (float32 [instances, 4, 4], column-major; None: the host view's own) ->
    instances [l, 24] uint32; copies [t, 16] uint32 (the words TRI_COPY_WORDS of every triangle record); owner [t]; cross [t, 3] float64;
    band [t, 3] float64; degenerate [t] bool (float64 cross product exactly zero)"""
    inst = np.asarray(tables["instances"], np.uint32)
    if matrices is None:
        matrices = inst[:, 4:20].copy().view(np.float32).reshape(-1, 4, 4)
    matrices = np.ascontiguousarray(matrices, np.float32)
    assert matrices.shape == (len(inst), 4, 4)
    meshes, tris, vertices = tables["meshes"], tables["triangles"], np.asarray(tables["vertices"], np.uint32)
    lights = np.asarray(tables["light_instances"], np.uint32).reshape(-1, 2)
    records = np.zeros((len(lights), INSTANCE_WORDS), np.uint32)
    copies, owner, cross, band = [], [], [], []
    base = 0
    for i, (iid, _tag) in enumerate(lights):
        handle = inst[iid, 0:4]
        assert handle[0] & LR_SHAPE_HAS_LIGHT, (i, iid)
        vertex_offset, _vertex_count, tri_offset, tri_count = (int(x) for x in meshes[handle[0] >> 10])
        assert int(handle[2]) == tri_count, (i, iid)  # the alias table of a mesh has one entry per triangle
        records[i, 0:4] = iid, tri_offset, handle[2], base
        records[i, 4:8] = handle[0] & 1023, handle[1], handle[3], 0
        m_words = matrices[iid].view(np.uint32)  # [column, row]
        for c in range(4):
            records[i, 8 + 4 * c:11 + 4 * c] = m_words[c, 0:3]
        idx = tris[tri_offset:tri_offset + tri_count].astype(np.int64) + vertex_offset  # [n, 3]
        v = vertices[idx]  # [n, 3 corners, 8 words]
        out = np.zeros((tri_count, len(TRI_COPY_WORDS)), np.uint32)
        out[:, 0:3], out[:, 3:6], out[:, 6:9] = v[:, 0, 0:3], v[:, 1, 0:3], v[:, 2, 0:3]
        out[:, 9:11], out[:, 11:13], out[:, 13:15] = v[:, 0, 6:8], v[:, 1, 6:8], v[:, 2, 6:8]
        out[:, 15] = np.asarray(tables["tri_pdf"], np.uint32)[tri_offset:tri_offset + tri_count]
        copies.append(out)
        owner.append(np.full(tri_count, i, np.int64))
        p = v[:, :, 0:3].copy().view(np.float32).astype(np.float64)  # [n, corner, xyz]
        m = matrices[iid, 0:3, 0:3].astype(np.float64).T  # [row, column]: M x = m @ x
        c, s = _cross_and_terms(m, p)
        cross.append(c)
        band.append(ROUNDINGS * UNIT * s)
        base += tri_count
    cat = lambda parts, shape, dtype: np.concatenate(parts) if parts else np.zeros(shape, dtype)
    e = {"instances": records, "copies": cat(copies, (0, len(TRI_COPY_WORDS)), np.uint32), "owner": cat(owner, (0,), np.int64),
         "cross": cat(cross, (0, 3), np.float64), "band": cat(band, (0, 3), np.float64)}
    e["degenerate"] = (e["cross"] == 0.0).all(axis=1)
    nonzero = e["band"][e["band"] > 0.0]
    assert nonzero.size == 0 or nonzero.min() > ROUNDINGS * UNIT * 2.0 ** -60, "inputs near the denormal range: outside the band's model"
    return e


def _cross_and_terms(m: np.ndarray, p: np.ndarray):
    """float64 c = cross(M (p1 - p0), M (p2 - p0)) [n, 3] and, per component, the sum of the absolute values of its fully expanded terms"""
    a, b = (p[:, 1] - p[:, 0]) @ m.T, (p[:, 2] - p[:, 0]) @ m.T  # (differences and products of fp32 values: float64 holds the inputs exactly)
    am = (np.abs(p[:, 1]) + np.abs(p[:, 0])) @ np.abs(m).T  # sum_i |m[r, i]| (|p1[i]| + |p0[i]|)
    bm = (np.abs(p[:, 2]) + np.abs(p[:, 0])) @ np.abs(m).T
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    s = np.stack([am[:, 1] * bm[:, 2] + am[:, 2] * bm[:, 1], am[:, 2] * bm[:, 0] + am[:, 0] * bm[:, 2], am[:, 0] * bm[:, 1] + am[:, 1] * bm[:, 0]], axis=1)
    return c, s


def judge_instances(device: np.ndarray, e: dict, what="") -> None:
    """the device's instance table (bytes or words, [l, 96 B]) against the expected words, all 24 of every record"""
    got = np.ascontiguousarray(device).view(np.uint32).reshape(-1, INSTANCE_WORDS)
    assert got.shape == e["instances"].shape, (what, got.shape, e["instances"].shape)
    rows = np.nonzero((got != e["instances"]).any(axis=1))[0]
    assert rows.size == 0, (what, "light instance records", rows[:8], got[rows[:1]], e["instances"][rows[:1]])


def judge_triangles(device: np.ndarray, e: dict, degenerate_count: int, what="") -> float:
    """the device's triangle table ([t, 80 B]) against the expected copies, cross products and bands -> the largest error / band.
    Every record is judged; `degenerate_count` is the number of zero-area emissive triangle records the scene was built with."""
    got = np.ascontiguousarray(device).view(np.uint32).reshape(-1, TRI_WORDS)
    assert len(got) == len(e["copies"]), (what, len(got), len(e["copies"]))
    rows = np.nonzero((got[:, TRI_COPY_WORDS] != e["copies"]).any(axis=1))[0]
    assert rows.size == 0, (what, "copied words", rows[:8], got[rows[:1]][:, TRI_COPY_WORDS], e["copies"][rows[:1]])
    f = got.view(np.float32).astype(np.float64)
    ng, area = f[:, TRI_NG_WORDS], f[:, TRI_AREA_WORD]
    flat = e["degenerate"]
    assert int(flat.sum()) == degenerate_count, (what, int(flat.sum()), degenerate_count)
    assert (area[flat] == 0.0).all() and (f[flat, TRI_PDF_WORD] == 0.0).all(), (what, "a triangle without area", area[flat], f[flat, TRI_PDF_WORD])
    live = ~flat
    if not live.any():
        return 0.0
    assert np.isfinite(ng[live]).all() and np.isfinite(area[live]).all() and (area[live] > 0.0).all(), what
    error = np.abs(2.0 * area[live, None] * ng[live] - e["cross"][live])
    band = e["band"][live]
    ratio = np.where(band > 0.0, error / np.where(band > 0.0, band, 1.0), np.where(error == 0.0, 0.0, np.inf))
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[worst] <= 1.0, (what, "2 area ng", np.nonzero(live)[0][worst[0]], worst[1], error[worst], band[worst])
    length = np.sqrt((ng[live] ** 2).sum(axis=1))
    assert (np.abs(length - 1.0) <= NG_LENGTH_ULPS * 2.0 ** -23).all(), (what, "|ng|", np.abs(length - 1.0).max() / 2.0 ** -23)
    return float(ratio[worst])
