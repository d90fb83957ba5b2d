"""Shared by tests/test_gather_reference.py and tests/test_gpu_gather.py: the UV rasteriser of lrhip_lightmap_texels (include/lrhip.h) in numpy
float64 -- the definition the device kernels (csrc/hip/lightmap_kernels.h) restate expression by expression -- the charts the tests
rasterise, and the measures the tests judge with: every texel's distance to the nearest triangle edge (the band in which the two sides may
disagree) and to the nearest triangle."""
import numpy as np

NO_OWNER = 0xFFFFFFFF
TOUCHED = 0x80000000
FLAG_CENTRE, FLAG_TOUCHED = 1, 2
EPSILON = 2.0 ** -20  # UV units: a texel centre nearer than this to a triangle edge may go to either side

# ---- the hand-made charts: (uvs [V, 2], triangles [T, 3]).  Vertices are kept off the lines of texel centres: scaled by 0.93, offset by 0.031
# (v: by 0.89 and 0.043, so that a square's diagonal does not run through the centres of a square map either)
_S, _O = (0.93, 0.89), (0.031, 0.043)


def _chart(uvs, triangles, scale=_S, offset=_O):
    return ((np.asarray(uvs, np.float64) * np.asarray(scale) + np.asarray(offset)).astype(np.float32), np.asarray(triangles, np.uint32).reshape(-1, 3))


ONE_TRIANGLE = _chart([(0, 0), (1, 0.1), (0.3, 1)], [(0, 1, 2)])
QUAD = _chart([(0, 0), (1, 0), (1, 1), (0, 1)], [(0, 1, 2), (0, 2, 3)])  # two triangles that share the diagonal
# the same quad, wound the other way in UV space (a mirrored chart)
FLIPPED = _chart([(0, 0), (1, 0), (1, 1), (0, 1)], [(0, 2, 1), (0, 3, 2)])
# a triangle without area (three points on a line), one with two equal vertices, and a sound one behind them: prims 0 and 1 own nothing
# (binary fractions, unscaled: the three points stay on one line in float32)
DEGENERATE = _chart([(0.0625, 0.0625), (0.5, 0.5), (0.9375, 0.9375), (0.9375, 0.0625), (0.2, 0.9)], [(0, 1, 2), (3, 3, 4), (0, 3, 2)], 1.0, 0.0)
# a chart that leaves [0, 1]^2 on three sides
OUTSIDE = _chart([(-0.4, 0.2), (0.7, -0.5), (1.6, 1.3), (0.1, 0.8)], [(0, 1, 2), (0, 2, 3)])
# exactly on the unit square: the shared diagonal passes through texel centres of a square map, so ties are decided by the lower prim
UNIT_QUAD = _chart([(0, 0), (1, 0), (1, 1), (0, 1)], [(0, 1, 2), (0, 2, 3)], 1.0, 0.0)
# the GPU tests' third mesh: a fan of seven triangles with a mirrored one, a degenerate one and parts outside the map
FAN = _chart([(0.5, 0.5), (1.1, 0.4), (0.9, 0.95), (0.45, 1.2), (0.02, 0.8), (-0.2, 0.3), (0.3, 0.05), (0.8, -0.1)],
             [(0, 1, 2), (0, 2, 3), (0, 4, 3), (0, 4, 5), (0, 5, 6), (0, 6, 7), (0, 7, 1), (1, 1, 2)])


def edge(ax, ay, bx, by, px, py):
    """(b - a) x (p - a): positive where p lies to the left of a -> b"""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _nearest(px, py, qx, qy, cx, cy):
    """parameter of the point of segment p -> q nearest to c, and its squared distance"""
    ex, ey = qx - px, qy - py
    l2 = ex * ex + ey * ey
    s = ((cx - px) * ex + (cy - py) * ey) / l2 if l2 > 0.0 else np.zeros_like(cx)
    s = np.minimum(np.maximum(s, 0.0), 1.0)
    dx, dy = cx - (px + s * ex), cy - (py + s * ey)
    return s, dx * dx + dy * dy


class Texels:
    """owner [H * W]: the owner words, ((centre covered ? 0 : 1) << 31) | prim, NO_OWNER where nobody owns the texel; prim, flags, u, v: the
    record's fields (prim NO_OWNER for a miss); edge_distance: the centre's distance to the nearest edge of any triangle near it (inf: none);
    triangle_distance: to the nearest triangle, 0 inside one"""

    def __init__(self, n):
        self.owner = np.full(n, NO_OWNER, np.uint32)
        self.prim = np.full(n, NO_OWNER, np.uint32)
        self.flags = np.zeros(n, np.uint32)
        self.u, self.v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.edge_distance = np.full(n, np.inf)
        self.triangle_distance = np.full(n, np.inf)
        self.on_edge = np.zeros(n, bool)

    @property
    def band(self):
        """the texels that may go either way: centres within EPSILON of an edge -- but not those EXACTLY on one (on_edge: an edge function
        that is 0.0 in float64, the icosphere's meridian u = 1/2 through the centre column of a 33-texel-wide map for one).  There the
        products are exact, nothing is left to rounding, and the rule (>= 0 covers, the lowest prim wins) decides: they are judged like
        every texel outside the band"""
        return (self.edge_distance <= EPSILON) & ~self.on_edge


def sound_triangles(uvs, triangles):
    """[(prim, a, b, c, area)] of the triangles that can own a texel: indices inside the mesh, finite UVs, an area in UV space"""
    uv = np.asarray(uvs, np.float32).astype(np.float64)
    out = []
    for prim, tri in enumerate(np.asarray(triangles)):
        if max(int(i) for i in tri) >= len(uv):
            continue
        a, b, c = (uv[int(i)] for i in tri)
        if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()):
            continue
        area = edge(a[0], a[1], b[0], b[1], c[0], c[1])
        if area != 0.0:
            out.append((prim, a, b, c, area))
    return out


def rasterise(uvs, triangles, width, height, conservative=False) -> Texels:
    """lrhip_lightmap_texels over the chart (uvs [V, 2] float32, triangles [T, 3]) in float64"""
    w, h = float(width), float(height)
    out = Texels(width * height)
    tris = sound_triangles(uvs, triangles)
    for prim, a, b, c, area in tris:
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        i_lo, j_lo = int(min(max(np.floor(lo[0] * w) - 1.0, 0.0), w)), int(min(max(np.floor(lo[1] * h) - 1.0, 0.0), h))
        i_end, j_end = int(min(max(np.floor(hi[0] * w) + 2.0, 0.0), w)), int(min(max(np.floor(hi[1] * h) + 2.0, 0.0), h))
        if i_lo >= i_end or j_lo >= j_end:
            continue
        jj, ii = np.meshgrid(np.arange(j_lo, j_end), np.arange(i_lo, i_end), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        texel = jj * width + ii
        cx, cy = (ii + 0.5) / w, (jj + 0.5) / h
        s = 1.0 if area > 0.0 else -1.0
        sides = ((b, c), (c, a), (a, b))
        covered, zero = np.ones(len(ii), bool), np.zeros(len(ii), bool)
        for p, q in sides:
            e = s * edge(p[0], p[1], q[0], q[1], cx, cy)
            covered &= e >= 0.0
            zero |= e == 0.0
        out.on_edge[texel[covered & zero]] = True
        word = np.where(covered, np.uint32(prim), np.uint32(NO_OWNER))
        d2 = np.minimum.reduce([_nearest(p[0], p[1], q[0], q[1], cx, cy)[1] for p, q in ((a, b), (b, c), (c, a))])
        if conservative:
            x0, y0, x1, y1 = ii / w, jj / h, (ii + 1.0) / w, (jj + 1.0) / h
            touched = (x0 <= hi[0]) & (x1 >= lo[0]) & (y0 <= hi[1]) & (y1 >= lo[1])
            for p, q in sides:
                e = np.maximum(np.maximum(edge(p[0], p[1], q[0], q[1], x0, y0) * s, edge(p[0], p[1], q[0], q[1], x1, y0) * s),
                               np.maximum(edge(p[0], p[1], q[0], q[1], x0, y1) * s, edge(p[0], p[1], q[0], q[1], x1, y1) * s))
                touched &= e >= 0.0
            word = np.where(covered, word, np.where(touched, np.uint32(TOUCHED | prim), np.uint32(NO_OWNER)))
        out.owner[texel] = np.minimum(out.owner[texel], word)
        out.edge_distance[texel] = np.minimum(out.edge_distance[texel], np.sqrt(d2))
        out.triangle_distance[texel] = np.minimum(out.triangle_distance[texel], np.where(covered, 0.0, np.sqrt(d2)))
    # ---- the records
    by_prim = {prim: (a, b, c, area) for prim, a, b, c, area in tris}
    owned = np.nonzero(out.owner != NO_OWNER)[0]
    for prim in np.unique(out.owner[owned] & ~np.uint32(TOUCHED)):
        a, b, c, area = by_prim[int(prim)]
        for touched_only in (False, True):
            t = owned[out.owner[owned] == (np.uint32(prim) | (np.uint32(TOUCHED) if touched_only else np.uint32(0)))]
            if len(t) == 0:
                continue
            cx, cy = (t % width + 0.5) / w, (t // width + 0.5) / h
            if not touched_only:
                u = edge(c[0], c[1], a[0], a[1], cx, cy) / area
                v = edge(a[0], a[1], b[0], b[1], cx, cy) / area
            else:
                (s_ab, d_ab), (s_bc, d_bc), (s_ca, d_ca) = (_nearest(p[0], p[1], q[0], q[1], cx, cy) for p, q in ((a, b), (b, c), (c, a)))
                u, v, d = s_ab.copy(), np.zeros_like(s_ab), d_ab.copy()
                m = d_bc < d
                u[m], v[m], d[m] = 1.0 - s_bc[m], s_bc[m], d_bc[m]
                m = d_ca < d
                u[m], v[m] = 0.0, 1.0 - s_ca[m]
            uf, vf = np.maximum(u.astype(np.float32), np.float32(0)), np.maximum(v.astype(np.float32), np.float32(0))
            uf = np.minimum(uf, np.float32(1))
            vf = np.where(uf + vf > np.float32(1), np.float32(1) - uf, vf)
            out.u[t], out.v[t], out.prim[t] = uf, vf, prim
            out.flags[t] = FLAG_TOUCHED if touched_only else FLAG_CENTRE
    return out


def chart_point(uvs, triangles, prim, u, v):
    """the UV-space points (1 - u - v) a + u b + v c of records (prim, u, v), float64 [N, 2]"""
    uv = np.asarray(uvs, np.float32).astype(np.float64)
    tri = np.asarray(triangles)[np.asarray(prim, np.int64)]
    a, b, c = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
    u, v = np.asarray(u, np.float64)[:, None], np.asarray(v, np.float64)[:, None]
    return (1.0 - u - v) * a + u * b + v * c


def distance_to_triangle(uvs, triangles, prim, points):
    """UV distance of points [N, 2] to the triangles `prim` [N] (0 inside)"""
    uv = np.asarray(uvs, np.float32).astype(np.float64)
    tri = np.asarray(triangles)[np.asarray(prim, np.int64)]
    a, b, c = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
    px, py = points[:, 0], points[:, 1]
    area = edge(a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1])
    s = np.where(area > 0.0, 1.0, -1.0)
    inside = np.ones(len(px), bool)
    d2 = np.full(len(px), np.inf)
    for p, q in ((a, b), (b, c), (c, a)):
        inside &= s * edge(p[:, 0], p[:, 1], q[:, 0], q[:, 1], px, py) >= 0.0
        ex, ey = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1]
        l2 = ex * ex + ey * ey
        t = np.clip(((px - p[:, 0]) * ex + (py - p[:, 1]) * ey) / np.where(l2 > 0.0, l2, 1.0), 0.0, 1.0)
        d2 = np.minimum(d2, (px - (p[:, 0] + t * ex)) ** 2 + (py - (p[:, 1] + t * ey)) ** 2)
    return np.where(inside, 0.0, np.sqrt(d2))


def inline_mesh(name, chart, surface="surface : Matte { }") -> str:
    """the scene text of a flat InlineMesh in the plane z = 0 whose positions are its UVs (x = u, y = v) and whose uvs are the chart's"""
    uvs, triangles = chart
    positions = ", ".join(f"{float(u)!r}, {float(v)!r}, 0" for u, v in uvs)
    uv_text = ", ".join(f"{float(u)!r}, {float(v)!r}" for u, v in uvs)
    indices = ", ".join(str(int(i)) for i in triangles.reshape(-1))
    return f"Shape {name} : InlineMesh {{ positions {{ {positions} }} indices {{ {indices} }} uvs {{ {uv_text} }} {surface} }}"
