"""A judge of the ray queries (include/lrhip.h: lrhip_trace_rays) that leaves no ray out: every ray of every family below gets
a verdict, at box corners, shared edges, grazing angles and segment ends too.  tests/raycast_reference.py excludes what float32 may decide
either way by fixed thresholds; here each (ray, triangle) pair carries ERROR BANDS derived from the device's own evaluation order.

THE BANDS.  trav_leaf_test (dev_trace.h), eps = 2^-24 (half an ulp, one rounding), every quantity below in float64 over the baked fp32 records
(raycast_reference.baked_triangles), |x| meaning "the same formula with the absolute value of every product":
    pvec = d x e2          fma(a, b, -(c * d)): the product and the fma round                              2
    det  = e1 . pvec       x first, then two fmas                                                          3   C_DET = 2 + 3 + 1 (d, below) = 6
    tvec = o - v0          one subtraction                                                                 1
    qvec = tvec x e1       as pvec                                                                         2
    u_n = tvec . pvec      3 + tvec 1 + pvec 2 + d 1 = 7;  v_n = d . qvec: 3 + qvec (2 + 1) + d 1 = 7;  t_n = e2 . qvec: 3 + 3 = 6   C_NUM = 7
    x = x_n * rcp(det)     v_rcp_f32 counted as 1 ulp = 2 eps, the product rounds once                          C_DIV = 3
"d 1": the query prologue (raycast_kernel.h) hands the loop d / |d|, whose last multiplication rounds each COMPONENT once (the common factor
1 / |d| only scales t); a direction taken bit for bit has no such rounding and the band is one count wide of the mark, on the safe side.
First order,  |dx| <= eps (C_NUM |x_n| / |det| + |x| (C_DET |det|_abs / |det| + C_DIV)),  divided by 1 - r with r = eps (C_DET |det|_abs / |det| +
C_DIV) for the reciprocal's higher orders; where r >= 1/2 float32 does not know the determinant's sign and the band is infinite.  The longest
chain has C = C_NUM + C_DET + C_DIV = 16 roundings.  u + v rounds once more.  t is reported in the caller's units: (t * (1 / len)) * 2^k, with len =
sqrt(dp . dp): C_SCALE = 8 more on t (the dot product 3, halved by the root, the root and the division 1 ulp each, two products).  The interval's
ends enter the loop as t_end * len * 2^-k (raycast_scale: the exact power of two first or last, whichever keeps the intermediate in range): C_END = 6
on each end.  Underflow: the relative model above fails where an intermediate is denormal; there an operation errs by at most FLT_MIN = 2^-126 absolutely,
flushed to zero or not.  A numerator or determinant is the end of at most 7 such operations whose later factors are of order 1 in the loop's normalised
units, so UNDERFLOW = 8 x 2^-126 = 2^-123 is added to its band: a bound for scene coordinates of order 1, a safety margin beyond that, and far below
eps times any product that matters.  Nothing here is tuned against the device: the bar on an observed
error is 1.0 band, and test_gpu_raycast_edges.py records the observed shares for information.

A weight whose numerator exceeds the determinant's largest possible magnitude, |x_n| - its band > 1.001 (|det| + its band), is above 1 in magnitude on
the device (the device's |x| is at least (|x_n| - band) / (|det| + band) x (1 - 3 eps) for the reciprocal and the product; 1.001 stands for that
1 + 3 eps = 1 + 1.8e-7 with a safety margin, on the side that rejects less) whatever sign its determinant takes there: below 0 it fails min(u, v) >= 0, above 1 either the other weight is negative or u + v > 1.  Such
a triangle is rejected for sure (rays parallel to a wall at a distance, whose determinant is nothing but a product's rounding error).
A triangle whose |det|_abs is exactly 0 (all six products of its determinant vanish: a zero edge, a ray and a wall in one axis plane) has det = 0 on
the device too, 1 / det = inf and u, v infinite or NaN: it is never accepted and belongs to neither set below.

SURE / MAYBE.  With lo = max(t_min, +0) (the contract: the search interval starts at +0 at the earliest), a visible triangle is SURE if
u > du, v > dv, u + v < 1 - dsum, lo + dlo + dt < t < t_max - dhi - dt, and MAYBE if the same holds relaxed by the bands.  Verdicts: verdicts().

THE FAMILIES (FAMILIES; each at most raycast_reference.RAY_COUNT rays, seeded) and the values pulled back so that the undecided share keeps
raycast_reference.AMBIGUOUS_CAP on the CPU (tests/test_raycast_judge.py: test_caps_and_a_correct_restatement asserts the cap,
test_pulled_back_parameters that the next step of a pulled-back distance breaks it): PULLED_BACK."""
import functools

import numpy as np

import raycast_reference as R
from luisarender_amd import Scene
from luisarender_amd.scenes.bathroom import inline_mesh

EPS = 2.0 ** -24
C_NUM, C_DET, C_DIV, C_SCALE, C_END = 7, 6, 3, 8, 6
C = C_NUM + C_DET + C_DIV  # 16: the roundings on the longest chain of u, v or t
UNDERFLOW = 2.0 ** -123
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = 2.0 ** -126
DENORMAL = 2.0 ** -149  # the spacing of float32 below FLT_MIN: what a result or an interval end in the caller's units may lose there
N = R.RAY_COUNT

# What was pulled back from the issue's starting values to keep the undecided cap, found on the CPU.
PULLED_BACK = {
    # far origins, in scene diagonals from the target.  The shell is convex and is seen from outside along directions within 60 degrees of the
    # target's normal: nothing else is in front at any distance.  In the room other fixtures stand in the way of a far origin, and a random
    # entry point 10^3 diagonals out is undecided more often than the cap allows (closest hit: a MAYBE triangle in front of the nearest SURE one).
    # At 10^4 diagonals the shell's own bands (7 eps |o - v0| / |e1| = 0.13 of a weight) exceed the targets' margin of 0.1: a third is undecided.
    # The last value of each is the most extreme that keeps the cap, searched in steps of 10^3 (shell) and 10^2 (room): with NEXT_STEP in its
    # place the family breaks it -- shell 6 x 10^3: 1.3 - 1.5 % undecided closest hits in the four shell families; room 10^3: 1.2 % -- which
    # test_raycast_judge.py::test_pulled_back_parameters asserts.
    "far_shell_diagonals": (1.0, 1e1, 1e2, 1e3, 5e3),
    "far_room_diagonals": (1.0, 1e1, 1e2, 8e2),
    # rays that are undecided by construction (in a wall's plane, through a corner that is a vertex): at most this many of the planes family
    "planes_in_plane_rays": 24,
    # rays aimed at the needle and the zero-area triangle of the degenerate family
    "degenerate_aimed_rays": 24,
    # secondary rays (origin = a hit point rounded to fp32) with t_min = 0: the surface they start on lies at t = 0 +- the origin's rounding, inside
    # its band.  The other secondary rays, and the rays that start on a vertex or a box plane, take t_min = 1e-4 x max(1, the scene's diagonal):
    # with coordinates of hundreds (the Cornell box) the band of t at the origin is 1e-4 .. 3e-4 itself.
    "secondary_rays_with_zero_t_min": 32,
}
NEXT_STEP = {"far_shell_diagonals": 6e3, "far_room_diagonals": 1e3}
# The far family of the ROOM comes as built only.  The shell is one inline mesh, which this module writes itself at any scale and under any instance
# transform; the room is a generated scene of instanced fixtures, each under an SRT transform of its own, and its generator has no argument that
# re-bases or rescales the whole: the moved, 10^-3 and 10^3 variants would need a second scene writer here.  What they test -- |o - v0| against the
# triangles' size at coordinates of 10^3 diagonals, of 10^-3 and of 10^3 -- is a property of the baked world-space records, which the shell covers.
# edge-aimed family: misses ("leaks") of the 4133 rays from the shell's centre at its edges and vertices, on the MI355X (test_gpu_raycast_edges.py
# prints them next to the count of the float32 restatement below)
MEASURED_LEAKS = {"device": 601, "restatement": 590}  # the baked records hold v0, e1, e2: two triangles do not share an edge's line bit for bit


# ---------------------------------------------------------------------------------------------------------------- scenes
def _icosphere(levels=3):
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v), np.array(f)


SHELL_CENTRE = np.array([0.11, -0.23, 0.31])
SHELL_RADIUS = 0.9


def _mesh_scene(name, v, f, extra=""):
    mesh = inline_mesh(name, v, f)[:-2] + "  surface : Matte { Kd : Constant { v { 0.5 } } }\n" + extra + "}\n"
    return mesh + R._HEAD + "render { cameras { @cam } shapes { @" + name + " } integrator : MegaPath { } }\n"


def shell_text(scale=1.0, offset=(0.0, 0.0, 0.0), translate=None):
    """the closed shell: an icosahedron subdivided three times (1280 triangles, shared vertices), vertices at `scale` x the unit shell + offset;
    translate: an instance transform on top"""
    v, f = _icosphere()
    v = (v * SHELL_RADIUS + SHELL_CENTRE) * scale + np.asarray(offset)
    extra = "" if translate is None else "  transform : SRT { translate { %.9g, %.9g, %.9g } }\n" % tuple(translate)
    return _mesh_scene("shell", v, f.reshape(-1), extra)


SHELL_DIAGONAL = 2.0 * SHELL_RADIUS * 3.0 ** 0.5
MOVED = np.array([1.0, -0.5, 0.25]) / np.linalg.norm([1.0, -0.5, 0.25]) * 1e3 * SHELL_DIAGONAL  # 10^3 diagonals from the world origin

DEGENERATE_EXTRA = """
Shape hidden : InlineMesh { positions { -2,-2,0.05, 2,-2,0.05, 2,2,0.05, -2,2,0.05 } indices { 0,1,2, 0,2,3 } visible { false }
  surface : Matte { Kd : Constant { v { 0.5 } } } }
"""


def degenerate_text():
    """soup64 plus a zero-area triangle (two vertices coincide), a needle of aspect 10^6, one triangle 10^4 times the size of the others, and an
    invisible quad through the middle (the visibility flag)"""
    rng = np.random.default_rng(7)
    n = 64
    centre = rng.uniform(-1.0, 1.0, (n, 3))
    e1, e2 = rng.normal(0.0, 0.12, (n, 3)), rng.normal(0.0, 0.12, (n, 3))
    v = np.stack([centre, centre + e1, centre + e2], axis=1).reshape(-1, 3)
    more = np.array([[0.3, 0.2, 0.1], [0.3, 0.2, 0.1], [0.5, 0.3, 0.2],                     # zero area: e1 = 0
                     [-0.5, -0.5, 0.4], [0.5, -0.5, 0.4], [0.0, -0.5 + 1e-6, 0.4],          # needle: base 1, height 1e-6
                     [-600.0, -1.7, -600.0], [600.0, -1.7, -600.0], [0.0, -1.7, 1200.0]])   # 10^4 x 0.12
    v = np.concatenate([v, more])
    text = _mesh_scene("soup", v, np.arange(len(v)))
    return text.replace("render { cameras { @cam } shapes { @soup }", DEGENERATE_EXTRA + "render { cameras { @cam } shapes { @soup, @hidden }")


ALPHA_SURFACE = ("Texture ones : Checkerboard { on : Constant { v { 1 } } off : Constant { v { 1 } } scale { 1 } }\n"
                 "Surface veil : Matte { Kd : Constant { v { 0.5 } } alpha { @ones } }\n")


def alpha_text():
    """soup64 under a surface whose opacity texture is 1 everywhere but is no constant the loader folds: every candidate is parked and committed"""
    text = R.soup_text(64)
    return ALPHA_SURFACE + text.replace("surface : Matte { Kd : Constant { v { 0.5 } } }", "surface { @veil }")


@functools.lru_cache(maxsize=None)
def scene_of(name):
    if name in ("soup", "soup64", "cornell", "room"):
        return R.scene_of(name)
    if name == "shell":
        return Scene.from_string(shell_text())
    if name == "shell_moved":
        return Scene.from_string(shell_text(translate=MOVED))
    if name == "shell_small":
        return Scene.from_string(shell_text(scale=1e-3))
    if name == "shell_large":
        return Scene.from_string(shell_text(scale=1e3))
    if name == "degenerate":
        return Scene.from_string(degenerate_text())
    if name == "alpha":
        return Scene.from_string(alpha_text())
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- the candidate table
class Table:
    """every (ray, triangle) pair that is MAYBE, sorted by ray then triangle: ray, tri, t, u, v, dt, du, dv (float64; t in the caller's units),
    sure; n rays, T triangles"""

    def __init__(self, n, T, **columns):
        self.n, self.T = n, T
        self.__dict__.update(columns)
        self.key = self.ray.astype(np.int64) * T + self.tri
        self.n_sure = np.bincount(self.ray[self.sure], minlength=n)
        self.n_maybe = np.bincount(self.ray, minlength=n)
        self.front_sure = np.full(n, np.inf)       # depth of the nearest SURE triangle
        np.minimum.at(self.front_sure, self.ray[self.sure], self.t[self.sure])
        self.front_sure_far = np.full(n, np.inf)   # ... its far band end, the least over SURE triangles
        np.minimum.at(self.front_sure_far, self.ray[self.sure], (self.t + self.dt)[self.sure])
        before = ~self.sure & (self.t < self.front_sure[self.ray])
        self.undecided_any = (self.n_sure == 0) & (self.n_maybe > 0)
        self.undecided_closest = self.undecided_any | (np.bincount(self.ray[before], minlength=n) > 0)

    def nearest_sure(self):
        """per ray: row of the table of the nearest SURE triangle, -1 if there is none"""
        row = np.full(self.n, -1)
        order = np.argsort(-self.t, kind="stable")  # the last write wins: nearest last
        order = order[self.sure[order]]
        row[self.ray[order]] = order
        return row


def table(tris, rays, cells=400_000):
    n, T = len(rays), len(tris)
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    visible = (tris["flags"] & 1) != 0
    r64 = rays.astype(np.float64)
    columns = {k: [] for k in ("ray", "tri", "t", "u", "v", "dt", "du", "dv", "sure")}
    chunk = max(1, cells // max(T, 1))

    def cross(a, b):
        return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])

    def across(a, b):
        return (a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0])

    def dot(a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    E1, E2 = [e1[None, :, k] for k in range(3)], [e2[None, :, k] for k in range(3)]
    A1, A2 = [np.abs(x) for x in E1], [np.abs(x) for x in E2]
    for first in range(0, n, chunk):
        r = r64[first:first + chunk]
        o, d = [r[:, k, None] for k in range(3)], [r[:, 4 + k, None] for k in range(3)]
        ad = [np.abs(x) for x in d]
        L = np.sqrt(dot(d, d))  # |d|: the loop's units are the caller's times L
        lo, hi = np.maximum(r[:, 3, None], 0.0), r[:, 7, None]
        with np.errstate(all="ignore"):
            pvec, pabs = cross(d, E2), across(ad, A2)
            det, adet = dot(E1, pvec), dot(A1, pabs) + 0.0 * L
            tvec = [o[k] - v0[None, :, k] for k in range(3)]
            at = [np.abs(x) for x in tvec]
            qvec, qabs = cross(tvec, E1), across(at, A1)
            den = np.abs(det)
            rel = EPS * (C_DET * adet + UNDERFLOW * L / EPS) / den + EPS * C_DIV
            known = (rel < 0.5) & (adet > 0.0)
            grow = 1.0 / (1.0 - np.where(known, rel, 0.0))
            out, outside = {}, False
            for name, num, anum, unit in (("u", dot(tvec, pvec), dot(at, pabs), L), ("v", dot(d, qvec), dot(ad, qabs), L),
                                          ("t", dot(E2, qvec), dot(A2, qabs), 1.0 + 0.0 * L)):
                x = num / det
                dx = (EPS * C_NUM * anum + UNDERFLOW * unit) / den + np.abs(x) * rel
                out[name] = np.where(known, x, 0.0), np.where(known, dx * grow, np.inf)
                if name != "t":  # |u| or |v| surely above 1, whatever the determinant's sign: rejected (see the module's text)
                    outside = outside | (np.abs(num) - (EPS * C_NUM * anum + UNDERFLOW * unit) > 1.001 * (den + EPS * C_DET * adet + UNDERFLOW * L))
            (u, du), (v, dv), (t, dt) = out["u"], out["v"], out["t"]
            dt = dt + EPS * C_SCALE * np.abs(t) + DENORMAL
            dsum = du + dv + EPS * np.abs(u + v)
            dlo = EPS * C_END * lo + DENORMAL * (1.0 + 1.0 / L)
            dhi = np.where(np.isfinite(hi), EPS * C_END * hi + DENORMAL * (1.0 + 1.0 / L), 0.0)
            live = visible[None, :] & (adet > 0.0) & ~outside
            sure = live & (u > du) & (v > dv) & (u + v < 1.0 - dsum) & (t > lo + dlo + dt) & (t < hi - dhi - dt)
            maybe = live & (u >= -du) & (v >= -dv) & (u + v <= 1.0 + dsum) & (t >= lo - dlo - dt) & (t <= hi + dhi + dt)
        rows, cols = np.nonzero(maybe)
        columns["ray"].append(rows + first), columns["tri"].append(cols)
        for name, a in (("t", t), ("u", u), ("v", v), ("dt", dt), ("du", du), ("dv", dv), ("sure", sure)):
            columns[name].append(a[rows, cols])
    return Table(n, T, **{k: np.concatenate(a) if a else np.zeros(0) for k, a in columns.items()})


# ---------------------------------------------------------------------------------------------------------------- verdicts
def verdicts(tab, tris, mode, answer):
    """mode "closest": answer is the [n, 8] float32 buffer of lrhip_ray_hit records; "any": the occlusion words / booleans.
    -> (violations: {rule: rows}, only the non-empty ones; share: the largest observed error of a reported hit as a share of its band)
         closest, a miss:  legal only if SURE is empty                                             rule "miss"
         closest, a hit:   names a MAYBE triangle                                                  "not_maybe"
                           t, u, v within that triangle's bands of its float64 values              "values"
                           no SURE triangle nearer than the reported one by more than both bands   "depth"
                           inst / prim are that triangle's, the reserved words 0                   "ids"
         any hit:          occluded only if MAYBE is non-empty, not occluded only if SURE is empty "occluded", "not_occluded" """
    bad, share = {}, 0.0
    if mode == "any":
        occluded = np.asarray(answer).astype(bool)
        bad["occluded"] = np.nonzero(occluded & (tab.n_maybe == 0))[0]
        bad["not_occluded"] = np.nonzero(~occluded & (tab.n_sure > 0))[0]
    else:
        words = np.ascontiguousarray(answer).view(np.uint32)
        t, u, v = (np.asarray(answer[:, k], np.float64) for k in range(3))
        inst, prim, tri = words[:, 3], words[:, 4], words[:, 5]
        hit = inst != R.INVALID
        record = np.isposinf(t) & (u == 0) & (v == 0) & (prim == R.INVALID) & (tri == R.INVALID)
        bad["miss"] = np.nonzero(~hit & ((tab.n_sure > 0) | ~record))[0]
        rows = np.nonzero(hit)[0]
        key = rows.astype(np.int64) * tab.T + tri[rows]
        at = np.searchsorted(tab.key, key)
        found = (tri[rows] < tab.T) & (at < len(tab.key))
        found[found] = tab.key[at[found]] == key[found]
        bad["not_maybe"] = rows[~found]
        rows, at = rows[found], at[found]
        with np.errstate(all="ignore"):
            shares = np.stack([np.abs(t[rows] - tab.t[at]) / tab.dt[at], np.abs(u[rows] - tab.u[at]) / tab.du[at], np.abs(v[rows] - tab.v[at]) / tab.dv[at]])
            shares = np.where(np.isnan(shares), 0.0, shares)  # (inf - inf: both beyond float32; 0 / 0 cannot happen, bands are positive)
            overflow = np.isposinf(t[rows]) & (tab.t[at] + tab.dt[at] >= FLT_MAX)  # the caller's t does not fit float32
            shares[0] = np.where(overflow, 0.0, shares[0])
        worst = shares.max(axis=0) if len(rows) else np.zeros(0)
        bad["values"] = rows[worst > 1.0]
        share = float(worst[np.isfinite(worst)].max()) if np.isfinite(worst).any() else 0.0
        bad["depth"] = rows[tab.front_sure_far[rows] < tab.t[at] - tab.dt[at]]
        k = tab.tri[at]
        bad["ids"] = rows[(inst[rows] != tris["inst"][k]) | (prim[rows] != tris["prim"][k]) | (words[rows, 6] != 0) | (words[rows, 7] != 0)]
    return {rule: r for rule, r in bad.items() if len(r)}, share


# ---------------------------------------------------------------------------------------------------------------- the float32 restatement
def _f(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)  # one float32 rounding of a float64-held value


def _fma(a, b, c):
    return _f(a * b + c)  # (a, b hold float32 values: the product is exact in float64)


def safe_inverse32(d):
    with np.errstate(all="ignore"):
        r = _f(1.0 / d)
    return np.where(np.abs(r) < 1e30, r, np.copysign(_f(1e30), d))


def restatement(tris, rays, wrong=None, cells=400_000):
    """trav_leaf_test and the query prologue in numpy float32 (values held in float64, rounded after every operation), brute force, exact division.
    -> ([n, 8] float32 records, occluded).  wrong: one of WRONG, a restatement the judge has to reject."""
    n, T = len(rays), len(tris)
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    visible = ((tris["flags"] & 1) != 0) | (wrong == "visibility_ignored")
    out = np.zeros((n, 8), np.float32)
    words = out.view(np.uint32)
    out[:, 0], words[:, 3:6] = np.inf, R.INVALID
    occluded = np.zeros(n, bool)
    r64 = rays.astype(np.float64)
    finite = np.isfinite(r64[:, :7]).all(axis=1) & ~np.isnan(r64[:, 7]) & ~np.isneginf(r64[:, 7])
    valid = finite & (r64[:, 4:7] != 0).any(axis=1) & (r64[:, 7] > r64[:, 3])
    chunk = max(1, cells // max(T, 1))
    E1, E2, V0 = [e1[None, :, k] for k in range(3)], [e2[None, :, k] for k in range(3)], [v0[None, :, k] for k in range(3)]
    b_lo, b_hi = (v0.min(axis=0), v0.max(axis=0)) if T else (np.zeros(3), np.zeros(3))
    for a in (v0 + e1, v0 + e2):
        if T:
            b_lo, b_hi = np.minimum(b_lo, a.min(axis=0)), np.maximum(b_hi, a.max(axis=0))
    b_lo, b_hi = _f(b_lo - 1e-3 * (b_hi - b_lo)), _f(b_hi + 1e-3 * (b_hi - b_lo))

    def crossf(p, q):
        return (_fma(p[1], q[2], -_f(p[2] * q[1])), _fma(p[2], q[0], -_f(p[0] * q[2])), _fma(p[0], q[1], -_f(p[1] * q[0])))

    def dotf(p, q):
        return _fma(p[2], q[2], _fma(p[1], q[1], _f(p[0] * q[0])))

    for first in range(0, n, chunk):
        r = r64[first:first + chunk]
        m = len(r)
        with np.errstate(all="ignore"):
            o, d = [r[:, k, None] for k in range(3)], [r[:, 4 + k, None] for k in range(3)]
            t_min, t_max = r[:, 3, None], r[:, 7, None]
            raw_d, raw_t_min = d, t_min
            # ---- the prologue (raycast_kernel.h): search from max(t_min, +0); a direction that is not unit length to within rounding is normalised
            t_min = np.where(t_min > 0.0, t_min, 0.0)
            if wrong == "t_min_ignored":
                t_min = np.full_like(t_min, -np.inf)
            unit = np.abs(dotf(d, d) - 1.0) <= _f(4e-7)
            big = np.maximum(np.maximum(np.abs(d[0]), np.abs(d[1])), np.abs(d[2]))
            pre = np.where(big < 2.0 ** -40, 2.0 ** 100, np.where(big > 2.0 ** 40, 2.0 ** -100, 1.0))
            dp = [_f(x * pre) for x in d]
            length = _f(np.sqrt(dotf(dp, dp)))
            inv_len = _f(1.0 / length)
            d = [np.where(unit, x, _f(y * inv_len)) for x, y in zip(d, dp)]
            t_min = np.where(unit, t_min, _f(_f(t_min * length) / pre))
            t_max = np.where(unit, t_max, _f(_f(t_max * length) / pre))
            # ---- trav_leaf_test
            pvec = crossf(d, E2)
            det = dotf(E1, pvec)
            inv_det = _f(1.0 / det)
            tvec = [_f(o[k] - V0[k]) for k in range(3)]
            u = _f(dotf(tvec, pvec) * inv_det)
            qvec = crossf(tvec, E1)
            v = _f(dotf(d, qvec) * inv_det)
            t = _f(dotf(E2, qvec) * inv_det)
            if wrong == "uv_swapped":
                u, v = v, u
            limit = 1.0 - 1.0 / 64.0 if wrong == "uv_sum_short" else 1.0
            ok = (np.minimum(u, v) >= 0.0) & (_f(u + v) <= limit) & (t > t_min) & (t < t_max) & visible[None, :] & valid[first:first + m, None]
            if wrong in ("inverse_capped", "signed_keys_dropped"):
                # a slab pre-test of the scene's bounds as trav_slab_sort_q makes it, WITHOUT the prologue: on the caller's direction, and
                # ("signed_keys_dropped") on the caller's t_min, a negative or -0.0 entry distance counting as "missed"
                inv = [safe_inverse32(x) for x in raw_d]
                tn = raw_t_min if wrong == "signed_keys_dropped" else np.where(raw_t_min > 0.0, raw_t_min, 0.0)
                tf = r[:, 7, None]
                for k in range(3):
                    a, b = _f(_f(b_lo[k] - o[k]) * inv[k]), _f(_f(b_hi[k] - o[k]) * inv[k])
                    tn, tf = np.maximum(tn, np.minimum(a, b)), np.minimum(tf, np.maximum(a, b))
                enter = tn <= _f(tf * _f(1.0000004))
                if wrong == "signed_keys_dropped":
                    enter = enter & ~np.signbit(tn)
                ok = ok & enter
            t_acc = np.where(ok, t, np.inf)
            best = np.argmin(t_acc, axis=1)
            if wrong == "farthest_on_97th":
                far = np.argmax(np.where(ok, t, -np.inf), axis=1)
                best = np.where((np.arange(first, first + m) % 97) == 0, far, best)
            rows = np.arange(m)
            hit = ok[rows, best]
            # ---- t in the caller's units
            t_out = np.where(unit[:, 0], t[rows, best], _f(_f(t[rows, best] * inv_len[:, 0]) * pre[:, 0]))
        sl = slice(first, first + m)
        occluded[sl] = hit
        out[sl, 0] = np.where(hit, t_out, np.inf)
        out[sl, 1], out[sl, 2] = np.where(hit, u[rows, best], 0.0), np.where(hit, v[rows, best], 0.0)
        words[sl, 3] = np.where(hit, tris["inst"][best], R.INVALID)
        words[sl, 4] = np.where(hit, tris["prim"][best], R.INVALID)
        words[sl, 5] = np.where(hit, best, R.INVALID)
    return out, occluded


WRONG = ("uv_sum_short", "uv_swapped", "farthest_on_97th", "t_min_ignored", "visibility_ignored", "inverse_capped", "signed_keys_dropped")


# ---------------------------------------------------------------------------------------------------------------- ray families
def _rays(o, d, t_min=R.T_MIN, t_max=np.inf):
    n = len(o)
    rays = np.empty((n, 8), np.float32)
    with np.errstate(over="ignore"):
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, t_min, d, t_max
    return rays


def _sphere(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _t_min_of(scene):
    return 1e-4 * max(1.0, _diagonal(scene))


def _diagonal(scene):
    lo, hi = R.scene_bounds(scene)
    return float(np.linalg.norm(hi - lo))


def _targets(rng, tris, n, least=0.1):
    """points drawn in float64 inside triangles, every barycentric weight >= least; -> (points, unit normals, triangle indices)"""
    k = rng.integers(0, len(tris), n)
    w = least + (1.0 - 3.0 * least) * rng.dirichlet((1.0, 1.0, 1.0), n)
    v0, e1, e2 = (tris[key][k].astype(np.float64) for key in ("v0", "e1", "e2"))
    normal = np.cross(e1, e2)
    return v0 + w[:, 1:2] * e1 + w[:, 2:3] * e2, normal / np.linalg.norm(normal, axis=1, keepdims=True), k


def _far(scene_name, diagonals, seed, outward_from=None):
    scene = scene_of(scene_name)
    tris = R.baked_triangles(scene)
    tris = tris[(tris["flags"] & 1) != 0]
    rng = np.random.default_rng(seed)
    per = N // len(diagonals)
    diag = _diagonal(scene)
    blocks = []
    for k in diagonals:
        p, normal, _ = _targets(rng, tris, per)
        if outward_from is not None:  # a convex shell: from outside, within 60 degrees of the outward normal
            centre = np.asarray(outward_from, np.float64)
            normal = np.where((np.sum(normal * (p - centre), axis=1) < 0)[:, None], -normal, normal)
            w = _sphere(rng, per)
            w = normal + w * np.sin(np.pi / 3.0) * rng.uniform(0.0, 1.0, (per, 1))
        else:
            w = _sphere(rng, per)
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        blocks.append(_rays(p + w * (k * diag), -w))
    return scene_name, np.concatenate(blocks)


def _base(name):
    return name, np.array(R.case(name)[1])


DIRECTION_EXPONENTS = (-140, -100, -30, -10, 10, 30, 100, 126)


def _direction_length(name):
    """base rays with d scaled by 2^k (exact), t_min and t_max scaled the other way where they stay in float32's range (else 0 and +inf)"""
    base = np.array(R.case(name)[1])
    per = N // len(DIRECTION_EXPONENTS)
    blocks = []
    for j, k in enumerate(DIRECTION_EXPONENTS):
        rows = np.arange(j, len(base), len(DIRECTION_EXPONENTS))[:per]  # every eighth ray: axis-parallel rays and segments in each block
        r = base[rows].astype(np.float64)
        d = r[:, 4:7] * 2.0 ** k
        t_min, t_max = r[:, 3] * 2.0 ** -k, r[:, 7] * 2.0 ** -k
        t_min = np.where(t_min < FLT_MIN, 0.0, t_min)
        t_max = np.where((t_max > FLT_MAX) | (t_max < 2.0 ** -120), np.inf, t_max)
        blocks.append(_rays(r[:, 0:3], d, t_min, t_max))
    rays = np.concatenate(blocks)
    assert np.isfinite(rays[:, 4:7]).all() and (np.abs(rays[:, 4:7]).max(axis=1) > 0).all()
    return name, rays


def _direction_components(name="soup64"):
    """unit directions with one or two components replaced by -0.0, 1e-20 and a denormal"""
    scene = scene_of(name)
    rng = np.random.default_rng(23)
    lo, hi = R.scene_bounds(scene)
    tris = R.baked_triangles(scene)
    p, _, _ = _targets(rng, tris, N)
    d = _sphere(rng, N)
    values = np.array([-0.0, 1e-20, 1e-40, -1e-20, -1e-40])
    first, second = rng.integers(0, 3, N), rng.integers(0, 3, N)
    d[np.arange(N), first] = values[rng.integers(0, 5, N)]
    two = rng.random(N) < 0.5
    d[np.arange(N)[two], second[two]] = values[rng.integers(0, 5, int(two.sum()))]
    left = (d != 0).any(axis=1) & (np.abs(d).max(axis=1) > 1e-3)
    d[~left] = (0.0, -0.0, 1.0)
    big = np.abs(d) > 1e-3
    d = np.where(big, d / np.linalg.norm(np.where(big, d, 0.0), axis=1, keepdims=True), d)
    return name, _rays(p - d * rng.uniform(0.3, 1.5, (N, 1)) * np.linalg.norm(hi - lo), d)


def _interval(name):
    """rays with a SURE hit at t*: t_max and t_min 4 bands on either side of t*, t_max = FLT_MAX, t_min in (0, -0, -1) from inside and outside the
    bounds, and secondary rays: origins that are a float64 hit point rounded to fp32, t_min 0 and 1e-4"""
    scene, base, _ = R.case(name)
    tris = R.baked_triangles(scene)
    rng = np.random.default_rng(29)
    base = np.array(base)
    base[:, 7] = np.inf
    tab = table(tris, base)
    row = tab.nearest_sure()
    has = np.nonzero(row >= 0)[0]
    t_star, band = tab.t[row[has]], tab.dt[row[has]] + EPS * C_END * tab.t[row[has]] + DENORMAL
    per = N // 9
    blocks = []

    def take(j):
        pick = has[(np.arange(per) * 7 + j) % len(has)]
        at = (np.arange(per) * 7 + j) % len(has)
        return base[pick].copy(), t_star[at], band[at]

    for j, side in enumerate((-4.0, 4.0)):
        r, ts, b = take(j)
        r[:, 7] = ts + side * b
        blocks.append(r)
        r, ts, b = take(j + 2)
        r[:, 3] = ts + side * b
        blocks.append(r)
    r, _, _ = take(4)
    r[:, 7] = FLT_MAX
    blocks.append(r)
    lo, hi = R.scene_bounds(scene)
    for j, t_min in enumerate((0.0, -0.0, -1.0)):
        r = base[(np.arange(per) * 5 + j) % len(base)].copy()  # origins inside the bounds grown by 5 %: inside and near them
        outside = np.arange(per) % 3 == 0
        r[outside, 0:3] = (r[outside, 0:3].astype(np.float64) - 2.0 * np.linalg.norm(hi - lo) * r[outside, 4:7]).astype(np.float32)
        r[:, 3] = t_min
        blocks.append(r)
    r, ts, _ = take(5)
    p = (r[:, 0:3].astype(np.float64) + ts[:, None] * r[:, 4:7]).astype(np.float32)
    d = _sphere(rng, per)
    blocks.append(_rays(p, d, np.where(np.arange(per) < PULLED_BACK["secondary_rays_with_zero_t_min"], 0.0, _t_min_of(scene))))
    return name, np.concatenate(blocks)


def _planes():
    """the Cornell box: origins that are a vertex exactly, or share one or two coordinates with one (the nodes' box planes are vertex coordinates);
    rays from outside through points next to the corners of the bounds; and PULLED_BACK["planes_in_plane_rays"] rays lying in a wall's plane along an
    axis or exactly through a corner of the bounds, which is a vertex of three walls"""
    scene = scene_of("cornell")
    tris = R.baked_triangles(scene)
    rng = np.random.default_rng(31)
    lo, hi = R.scene_bounds(scene)
    diag = np.linalg.norm(hi - lo)
    verts = np.concatenate([tris["v0"], tris["v0"] + tris["e1"], tris["v0"] + tris["e2"]]).astype(np.float64)
    few = PULLED_BACK["planes_in_plane_rays"]
    n_vertex = (N - few) // 3
    blocks = []
    # origin = a vertex (fp32 exactly): the triangles around it are at t = 0, outside (t_min, ...)
    p = verts[rng.integers(0, len(verts), n_vertex)]
    blocks.append(_rays(p, _sphere(rng, n_vertex), _t_min_of(scene)))
    # origin inside, one or two coordinates equal to a vertex's (box planes of the nodes are vertex coordinates): axis-parallel and random directions
    inside = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (n_vertex, 3))
    q = verts[rng.integers(0, len(verts), n_vertex)]
    same = rng.random((n_vertex, 3)) < 0.5
    same[np.arange(n_vertex), rng.integers(0, 3, n_vertex)] = True
    same[np.arange(n_vertex), rng.integers(0, 3, n_vertex)] = False
    p = np.where(same, q, inside)
    d = _sphere(rng, n_vertex)
    axis = same.sum(axis=1) == 1  # axis-parallel along the shared coordinate's axis: out of that plane, not in it
    d[axis] = same[axis] * rng.choice([-1.0, 1.0], (int(axis.sum()), 1))
    blocks.append(_rays(p, d, _t_min_of(scene)))
    # from outside through points next to the bounds' corners (a corner itself is a vertex of three walls: among the few below)
    n_corner = N - few - 2 * n_vertex
    corner = np.where(rng.random((n_corner, 3)) < 0.5, lo, hi)
    away = np.sign(corner - 0.5 * (lo + hi)) * rng.uniform(0.2, 1.0, (n_corner, 3))
    through = corner - np.sign(away) * rng.uniform(0.01, 0.2, (n_corner, 3)) * (hi - lo)
    origin = corner + away * diag
    blocks.append(_rays(origin, through - origin))  # (not normalised: lengths of a few diagonals)
    # the few: in a wall's plane along an axis, and exactly through corners
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    normal = np.cross(e1, e2)
    flat = np.nonzero((normal != 0).sum(axis=1) == 1)[0]
    rows = []
    for j in range(few - 8):
        k = flat[j % len(flat)]
        axis_n = int(np.nonzero(normal[k])[0][0])
        along = (axis_n + 1 + j % 2) % 3
        start = v0[k] + 0.3 * e1[k] + 0.3 * e2[k]
        step = np.zeros(3)
        step[along] = 1.0 if (j // 2) % 2 == 0 else -1.0
        rows.append(np.concatenate([start - 0.1 * step * (j % 3), [R.T_MIN], step, [np.inf]]))
    for j in range(8):
        c = np.where([(j >> b) & 1 for b in range(3)], hi, lo)
        out = np.sign(c - 0.5 * (lo + hi))
        rows.append(np.concatenate([c + out * (hi - lo), [R.T_MIN], -out * (hi - lo), [np.inf]]))
    blocks.append(np.array(rows, np.float32))
    return "cornell", np.concatenate(blocks)


def _edge_aimed():
    """from the shell's centre at points on its shared edges (float64 points between the baked endpoints) and at its vertices"""
    scene = scene_of("shell")
    tris = R.baked_triangles(scene)
    rng = np.random.default_rng(37)
    v0, e1, e2 = (tris[k].astype(np.float64) for k in ("v0", "e1", "e2"))
    k = rng.integers(0, len(tris), N)
    which = rng.integers(0, 3, N)
    a = np.where((which == 0)[:, None], v0[k], np.where((which == 1)[:, None], v0[k] + e1[k], v0[k] + e2[k]))
    b = np.where((which == 0)[:, None], v0[k] + e1[k], np.where((which == 1)[:, None], v0[k] + e2[k], v0[k]))
    s = rng.uniform(0.0, 1.0, (N, 1))
    s[: N // 4] = 0.0  # a quarter at vertices
    p = a + s * (b - a)
    centre = np.broadcast_to(SHELL_CENTRE.astype(np.float32).astype(np.float64), (N, 3))
    d = p - centre
    return "shell", _rays(centre, d / np.linalg.norm(d, axis=1, keepdims=True), 0.0)


def _degenerate():
    rng = np.random.default_rng(41)
    rays = R.make_rays(scene_of("soup64"), N, 43)
    # a few aimed at the needle and at the zero-area triangle's line (the needle's bands are a fifth of its width: undecided by construction)
    k = PULLED_BACK["degenerate_aimed_rays"]
    a, b = np.array([0.3, 0.2, 0.1]), np.array([0.5, 0.3, 0.2])
    p = np.where((np.arange(k) % 2 == 0)[:, None], a + rng.uniform(0, 1, (k, 1)) * (b - a),
                 np.array([-0.5, -0.5, 0.4]) + rng.uniform(0, 1, (k, 1)) * np.array([1.0, 0.0, 0.0]) + np.array([0.0, 5e-7, 0.0]))
    d = _sphere(rng, k)
    rays[:k] = _rays(p - d * rng.uniform(0.5, 3.0, (k, 1)), d)
    return "degenerate", rays


FAMILIES = {
    "base_soup": lambda: _base("soup"),
    "base_cornell": lambda: _base("cornell"),
    "base_room": lambda: _base("room"),
    "far_shell": lambda: _far("shell", PULLED_BACK["far_shell_diagonals"], 13, SHELL_CENTRE),
    "far_shell_moved": lambda: _far("shell_moved", PULLED_BACK["far_shell_diagonals"], 14, SHELL_CENTRE + MOVED),
    "far_shell_small": lambda: _far("shell_small", PULLED_BACK["far_shell_diagonals"], 15, SHELL_CENTRE * 1e-3),
    "far_shell_large": lambda: _far("shell_large", PULLED_BACK["far_shell_diagonals"], 16, SHELL_CENTRE * 1e3),
    "far_room": lambda: _far("room", PULLED_BACK["far_room_diagonals"], 17),
    "direction_length_soup64": lambda: _direction_length("soup64"),
    "direction_length_cornell": lambda: _direction_length("cornell"),
    "direction_components": _direction_components,
    "interval_soup": lambda: _interval("soup"),
    "interval_cornell": lambda: _interval("cornell"),
    "planes": _planes,
    "edge_aimed": _edge_aimed,
    "degenerate": _degenerate,
}
UNCAPPED = ("edge_aimed",)  # undecided by design: the judge's rules apply, the cap does not


@functools.lru_cache(maxsize=None)
def case(family):
    """(scene, its baked triangles, rays [n, 8] float32, the candidate table), computed once per process and shared: do not modify"""
    scene_name, rays = FAMILIES[family]()
    scene = scene_of(scene_name)
    tris = R.baked_triangles(scene)
    rays = np.ascontiguousarray(rays, np.float32)
    assert len(rays) <= N and rays.shape[1] == 8
    rays.setflags(write=False)
    return scene, tris, rays, table(tris, rays)


def leaks(answer):
    """misses among closest-hit records"""
    return int((np.ascontiguousarray(answer).view(np.uint32)[:, 3] == R.INVALID).sum())
