"""Reference of the surface queries (include/lrhip.h: lrhip_query_surface): Geometry::shading_point (src/base/geometry.cpp:345-389)
restated in float64 numpy from the HOST tables -- Scene.view() through tests/instance_scene.host_tables -- for given (inst, prim, u, v):
world position, triangle area, geometric and shading normal, uv, tangent, and the uv determinant, which tells where the tangent is dpdu and
where it is the fallback frame's (det == 0: the device takes frame_from_normal(ng).s, whose sign conventions are not restated here).

Everything is widened to float64 FIRST: the instance's float32 matrix, the float32 vertices, the float32 (u, v) the device reported.  The
normal matrix is transpose(inverse(M)) of the widened matrix, where the device reads the float32 one the host stored.  What the device
disagrees with this about is its float32 arithmetic (or its code)."""
import numpy as np

from instance_scene import host_tables

INVALID = 0xFFFFFFFF
HAS_VERTEX_NORMAL, HAS_VERTEX_UV, HAS_SURFACE, HAS_LIGHT = 1, 2, 4, 8  # lr_scene.h: LR_SHAPE_*
VALID, BACK_FACING, SURFACE, LIGHT = 1, 2, 4, 8                        # lrhip.h: LRHIP_SURFACE_*

# The largest errors of the device against this reference, measured on the MI355X over the instanced room and the Cornell box, both paths
# (baked record / instance + vertices), at the device's own (inst, prim, u, v) for tests/raycast_reference.make_rays' 4133 rays
# (tests/test_gpu_surface.py prints them): |p - p_ref| / max(1, |p_ref|), the largest componentwise error of ng, ns, uv and tangent, the
# relative error of area.  The bars are 4 x the recorded values, the project's margin for a float32-against-float64 bar;
# a measured error above 1e-4 would be a bug to find, not a bar to set.
MEASURED_P_ERROR = 1.8e-7
MEASURED_NG_ERROR = 5.0e-7
MEASURED_NS_ERROR = 9.5e-8
MEASURED_UV_ERROR = 8.2e-8
MEASURED_TANGENT_ERROR = 3.5e-7
MEASURED_AREA_ERROR = 6.3e-7
# the ball's ns against the AOV kernel's `normal` buffer of the same sample (test 4: the oracle's camera rays against the device's own)
MEASURED_AOV_BALL_NORMAL_ERROR = 2.2e-6
BAR_P, BAR_NG, BAR_NS = 4.0 * MEASURED_P_ERROR, 4.0 * MEASURED_NG_ERROR, 4.0 * MEASURED_NS_ERROR
BAR_UV, BAR_TANGENT, BAR_AREA = 4.0 * MEASURED_UV_ERROR, 4.0 * MEASURED_TANGENT_ERROR, 4.0 * MEASURED_AREA_ERROR
BAR_AOV_BALL_NORMAL = 4.0 * MEASURED_AOV_BALL_NORMAL_ERROR
LARGEST_SOUND_ERROR = 1e-4


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def shading_points(scene_or_tables, inst, prim, u, v) -> dict:
    """-> dict of float64 arrays over the N records: p [N, 3], area [N], ng, ns, tangent [N, 3], uv [N, 2], det [N] (the uv determinant in the
    float32 arithmetic of the reference, so that det == 0 means what it means there), flags, tags [N] (handle.x & 1023, handle.y).
    scene_or_tables: a Scene, or host_tables(scene) (the caller may hold moved copies)."""
    t = scene_or_tables if isinstance(scene_or_tables, dict) else host_tables(scene_or_tables)
    inst, prim = np.asarray(inst, np.int64), np.asarray(prim, np.int64)
    u, v = np.asarray(u, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    w = 1.0 - u - v
    rec = t["instances"][inst]
    flags, tags = rec[:, 0] & 1023, rec[:, 1]
    mesh = t["meshes"][rec[:, 0] >> 10]
    assert (prim < mesh[:, 3]).all()
    tri = t["triangles"][mesh[:, 2] + prim].astype(np.int64)
    vert32 = [t["vertices"][mesh[:, 0] + tri[:, k]].view(np.float32) for k in range(3)]
    vert = [x.astype(np.float64) for x in vert32]
    o2w = rec[:, 4:20].view(np.float32).astype(np.float64).reshape(-1, 4, 4)  # [n, c, r]
    m = np.transpose(o2w[:, :3, :3], (0, 2, 1))  # [n, r, c]
    mul = lambda x: np.einsum("nrc,nc->nr", m, x)
    p0, p1, p2 = (x[:, 0:3] for x in vert)
    dp0, dp1 = p1 - p0, p2 - p0
    p = mul(w[:, None] * p0 + u[:, None] * p1 + v[:, None] * p2) + o2w[:, 3, :3]
    c = np.cross(mul(dp0), mul(dp1))
    area = 0.5 * np.linalg.norm(c, axis=1)
    ng = _unit(c)
    has_uv, has_normal = (flags & HAS_VERTEX_UV) != 0, (flags & HAS_VERTEX_NORMAL) != 0
    uv0, uv1, uv2 = (x[:, 6:8] for x in vert)
    uv = np.where(has_uv[:, None], w[:, None] * uv0 + u[:, None] * uv1 + v[:, None] * uv2, np.stack([u, v], axis=1))
    # the determinant as the reference forms it, in float32 (numpy float32 is unfused): its zero test is the branch
    a32, b32, c32 = (x[:, 6:8] for x in vert32)
    d0, d1 = b32 - a32, c32 - a32
    det32 = d0[:, 0] * d1[:, 1] - d0[:, 1] * d1[:, 0]
    duv0, duv1 = uv1 - uv0, uv2 - uv0
    det = duv0[:, 0] * duv1[:, 1] - duv0[:, 1] * duv1[:, 0]
    with np.errstate(all="ignore"):
        dpdu = mul((dp0 * duv1[:, 1:2] - dp1 * duv0[:, 1:2]) / det[:, None])
    mn = np.transpose(np.linalg.inv(m), (0, 2, 1))
    n_local = w[:, None] * vert[0][:, 3:6] + u[:, None] * vert[1][:, 3:6] + v[:, None] * vert[2][:, 3:6]
    with np.errstate(all="ignore"):
        ns = np.where(has_normal[:, None], _unit(np.einsum("nrc,nc->nr", mn, n_local)), ng)
        ns = np.where((np.einsum("nk,nk->n", ns, ng) < 0.0)[:, None], -ns, ns)  # face_forward(ns, ng)
        s = _unit(dpdu - ns * np.einsum("nk,nk->n", ns, dpdu)[:, None])  # Frame::make(n, s), src/util/frame.cpp:31-35
    return {"p": p, "area": area, "ng": ng, "ns": ns, "tangent": s, "uv": uv, "det": det32.astype(np.float64), "flags": flags, "tags": tags}


def geometry_errors(points, ref) -> dict:
    """the largest errors of a SurfacePoints (numpy) against shading_points' answer for the same records, every record valid:
    p (relative to max(1, |p_ref|)), ng, ns, uv, tangent (componentwise, the tangent where det != 0 only), area (relative)"""
    assert np.asarray(points.valid).all()
    p = points.p.astype(np.float64)
    dpdu = ref["det"] != 0.0
    return {
        "p": float((np.linalg.norm(p - ref["p"], axis=1) / np.maximum(1.0, np.linalg.norm(ref["p"], axis=1))).max()),
        "ng": float(np.abs(points.ng - ref["ng"]).max()),
        "ns": float(np.abs(points.ns - ref["ns"]).max()),
        "uv": float(np.abs(points.uv - ref["uv"]).max()),
        "tangent": float(np.abs(points.tangent[dpdu] - ref["tangent"][dpdu]).max()) if dpdu.any() else 0.0,
        "area": float((np.abs(points.area - ref["area"]) / ref["area"]).max()),
    }


def hit_records(inst, prim, u, v, tri=None) -> np.ndarray:
    """[N, 8] float32 lrhip_ray_hit records a caller makes for (inst, prim, u, v): t = 0, tri = LR_INVALID_ID unless given"""
    n = len(inst)
    rec = np.zeros((n, 8), np.float32)
    ids = rec.view(np.uint32)
    rec[:, 1], rec[:, 2] = u, v
    ids[:, 3], ids[:, 4] = inst, prim
    ids[:, 5] = INVALID if tri is None else tri
    return rec


def invalid_record() -> np.ndarray:
    """the invalid record as 32 words: zeros, except inst = prim = surface = light = closure_kind = LR_INVALID_ID"""
    r = np.zeros(32, np.uint32)
    r[[11, 15, 19, 27, 31]] = INVALID
    return r
