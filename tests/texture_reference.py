"""A judge of the texture lookup (dev_shade.h: texture_eval_tables, texel_wrap, texel_at) that gives every lookup a verdict,
texel by texel.  Three pieces, none of which needs a GPU:

THE REFERENCE.  Texture::Instance::evaluate of Constant / Image / Checkerboard (texture.cpp:21-79, image.cpp:132-168 with the sampler's
address modes of image.cpp:50-63, checkerboard.cpp) restated in float64 numpy over the HOST's tables (Scene.view(): the lr_texture records and
the float texels, whatever file they came from and however the device stores them), wrapping in Python integers; then the consumer's rule:
albedo saturate(extend_rgb(.)), emission max0(xyz) * light.scale, roughness with and without the remap.

THE JUDGE.  Input: the texture and the float32 uv AT the lookup.  The texel coordinate is taken in float64 and carries a band delta counted off
the device's evaluation order, eps = 2^-24 (half an ulp, one rounding), every |.| in float64:
    U = u * s + o          the product and the sum round: eps (|u s| + |U|);  contracted to one fma: eps |U|, which is smaller
    X = U * w              one rounding: delta_X = w delta_U + eps |X|
    F = X - 0.5            (bilinear) one more: delta_F = delta_X + eps |F|;  contracted with the product: w delta_U + eps |F|, smaller
The uncontracted count bounds both forms (the objects of the project are built either way) and is the band; x (1 + 2^-20) for the higher orders.
A uv that is not the lookup's own bit for bit (taken from another kernel's reconstruction of the same hit) widens delta_U by |s| x `uv_ulps` ulp (or by |s| x an absolute distance: a point found again by tracing a ray to it).
    point filter       |X - round(X)| <= delta on an axis: the record is MAYBE and the texel on either side of that integer is accepted; else SURE.
                       A linear float texel of a SURE record must come back as the float32 product scale * texel, and so on through the consumer.
                       (A band of more than a texel -- a traced uv under a uv_scale of millions -- leaves the texel open: MAYBE, any finite value.)
    bilinear           continuous across cells under every address mode, so no record is left out and none is MAYBE: the bar is
                       (delta_x + delta_y) D + C_MIX eps M, D the largest difference between adjacent texels (both axes) in the 4 x 4 texels around
                       the footprint (3 x 3 cells: where a coordinate off by delta < 1 may land), M the largest magnitude there.  C_MIX = 6: the
                       roundings on the longest chain of (a (1 - tx) + b tx) (1 - ty) + (c (1 - tx) + d tx) ty -- 1 - tx, the product, the inner sum,
                       1 - ty, the outer product, the outer sum -- each acting on a partial sum that M bounds (the weights are non-negative and sum
                       to 1 up to those very roundings).  tx = F - floor(F) is exact.  delta >= 1 (texel coordinates beyond ~2^22 under a free uv):
                       float32 no longer says which cell; the bar is then the range of the image, which any convex combination keeps.
    decode             scale * c rounds once more.  sRGB and gamma go through v_log_f32 / v_exp_f32, whose error is not derivable: the largest
                       relative difference to this reference is MEASURED on the MI355X (below) and MARGIN x it is asserted.
    checkerboard       floor(u * scale) + floor(v * scale): one rounding each, eps |u scale|; within that of an integer the parity is MAYBE and
                       either child is accepted.
The share of MAYBE records of a family is a function of inputs and reference only: at most MAYBE_CAP, 0 for the `exact` family.

THE FAMILIES (family(); each at most N = 4099 records: more than one 256-lane block, no multiple of 64; images at most 16 texels a side), as
caller-made hit records (tri = LR_INVALID_ID; inst, prim, u, v) on quads of two triangles, one quad per texture: exact, seams, generic, decode, bytes,
checker and alpha as the builders below describe them, and inside -- coordinates of the exact kind around 0 and +-2^20, a quarter of a texel inside
each texel, so that the channels which TRACE their rays judge both paths of texel_wrap on SURE records.

Also here: device_lookup(), a float32 numpy restatement of the device's lookup with its mistakes on request (tests/test_texture_reference.py
shows that the judge accepts the restatement and rejects each of the ten mistakes), and what tests/test_gpu_texture.py measured."""
import functools
import math

import numpy as np

from instance_scene import host_tables
from luisarender_amd import Scene
from luisarender_amd.scenes.configs import write_pfm, write_png

EPS = 2.0 ** -24
HIGHER_ORDERS = 1.0 + 2.0 ** -20
C_MIX = 6
N = 4099
MAYBE_CAP = 0.01
MARGIN = 4.0  # the project's margin of a float32-against-float64 bar over a measured error (light_reference.py)
INVALID = 0xFFFFFFFF
REPEAT, EDGE, MIRROR, ZERO = 0, 1, 2, 3  # lr_scene.h: LR_TEX_ADDR_*
ADDRESSES = {"repeat": REPEAT, "edge": EDGE, "mirror": MIRROR, "zero": ZERO}
CONSTANT, IMAGE, CHECKERBOARD = 0, 1, 2
POINT, BILINEAR = 0, 1
LINEAR, SRGB, GAMMA = 0, 1, 2
KNEE = float(np.float32(0.04045))  # the device and the reference compare the float32 texel with this float32 constant

# The largest relative difference |device - reference| / |reference| of a decoded texel over the `decode` family (point filter, SURE records, every
# channel of tests/test_gpu_texture.py), measured on the MI355X; the bars are MARGIN x these.  (None: not measured yet -- the GPU test then fails
# after printing its figures.)  dev_shade.h said "~3e-7 relative" of x^2.4 = x^2 * exp2(0.4 log2 x); 4.4e-7 is what the albedo, emission, radiance
# and film channels show (texels in [0, 2.5]), and the comment there now says so.  The gamma branch is exp2(g log2 x) as it stands: the logarithm's
# ulp is scaled by g |log2 x|, which is 30 for g = 3 and a texel of 1e-3 -- no error of the hardware beyond its ulp, but no 3e-7 either.
MEASURED_SRGB = 4.42e-7   # surface query, emission
MEASURED_GAMMA = 2.23e-6  # surface query, albedo (gamma 2.2, 2 and 3 over texels in [0, 1])
# roughness: alpha = max(r^2, 1e-4) (the remap) or r, reported as sqrt(max(alpha, 1e-4)) (dev_heavy.h: closure_albedo_roughness): the square rounds
# once (halved by the root), the root is the hardware's to 1 ulp = 2 eps, so 2.5 eps relative; the bar allows 4 eps.
ROUGHNESS_EPS = 4.0


# ---------------------------------------------------------------------------------------------------------------- the host's tables
class Tables:
    """what the lookup reads of a Scene: textures (list of dicts), texels float32 [n, 4], per instance its surface and light tags, the surfaces' texture
    slots, flags and alpha texture, the lights' emission texture and scale"""

    def __init__(self, scene: Scene):
        v = scene.view()
        n = int(v.texel_count)  # float4 units
        self.texels = np.ctypeslib.as_array(v.texels, shape=(n * 4,)).reshape(n, 4).copy() if n else np.zeros((0, 4), np.float32)
        self.textures = []
        for i in range(v.texture_count):
            t = v.textures[i]
            self.textures.append({"kind": int(t.kind), "channels": int(t.channels), "v": np.float32(list(t.v)), "width": int(t.width),
                                  "height": int(t.height), "offset": int(t.texel_offset), "address": int(t.address), "filter": int(t.filter),
                                  "encoding": int(t.encoding), "gamma": np.float32(list(t.gamma)), "uv_scale": np.float32(list(t.uv_scale)),
                                  "uv_offset": np.float32(list(t.uv_offset)), "scale": np.float32(list(t.scale)),
                                  "child": [int(c) for c in t.child], "checker_scale": np.float32(t.checker_scale)})
        inst = host_tables(scene)["instances"]
        self.light_tag, self.surface_tag = (inst[:, 1] & 4095).astype(np.int64), ((inst[:, 1] >> 12) & 4095).astype(np.int64)
        self.flags = (inst[:, 0] & 1023).astype(np.int64)
        self.surfaces = [{"kind": int(s.kind), "flags": int(s.flags), "tex": [int(x) for x in s.tex], "alpha_tex": int(s.alpha_tex)}
                         for s in (v.surfaces[i] for i in range(v.surface_count))]
        self.lights = [{"emission_tex": int(l.emission_tex), "scale": np.float32(l.scale), "two_sided": int(l.two_sided)}
                       for l in (v.lights[i] for i in range(v.light_count))]

    @classmethod
    def of_images(cls, specs: list) -> "Tables":
        """tables made by hand, without a scene: one image texture per spec (a dict of lr_texture fields over `pixels` float32 [h, w, 3 or 4])"""
        self = cls.__new__(cls)
        self.textures, chunks, offset = [], [], 0
        for spec in specs:
            px = np.asarray(spec["pixels"], np.float32)
            h, w = px.shape[:2]
            rgba = np.ones((h, w, 4), np.float32)
            rgba[..., :px.shape[2]] = px
            g = np.float32(spec.get("gamma", 1.0))
            self.textures.append({"kind": IMAGE, "channels": px.shape[2], "v": np.zeros(4, np.float32), "width": w, "height": h, "offset": offset,
                                  "address": spec.get("address", REPEAT), "filter": spec.get("filter", POINT), "encoding": spec.get("encoding", LINEAR),
                                  "gamma": np.float32([g, g, g]), "uv_scale": np.float32(spec.get("uv_scale", (1, 1))),
                                  "uv_offset": np.float32(spec.get("uv_offset", (0, 0))), "scale": np.full(4, spec.get("scale", 1.0), np.float32),
                                  "child": [-1, -1], "checker_scale": np.float32(1)})
            chunks.append(rgba.reshape(-1, 4))
            offset += w * h
        self.texels = np.concatenate(chunks)
        return self

    def image(self, t) -> np.ndarray:
        """the texels of an image texture, float32 [height, width, 4]"""
        return self.texels[t["offset"]:t["offset"] + t["width"] * t["height"]].reshape(t["height"], t["width"], 4)

    def texture_of(self, inst, role: str) -> np.ndarray:
        """the texture id each instance's `role` reads: albedo (slot 0 of its surface), roughness (slot 1: Mirror), alpha, emission"""
        inst = np.asarray(inst, np.int64)
        if role == "emission":
            return np.array([self.lights[k]["emission_tex"] for k in self.light_tag[inst]], np.int64)
        s = [self.surfaces[k] for k in self.surface_tag[inst]]
        if role == "alpha":
            return np.array([x["alpha_tex"] for x in s], np.int64)
        return np.array([x["tex"][{"albedo": 0, "roughness": 1}[role]] for x in s], np.int64)


# ---------------------------------------------------------------------------------------------------------------- the reference
def wrap(address: int, v: int, n: int):
    """the sampler's address mode on ONE Python integer -> the texel index, or None for ZERO outside the image (image.cpp:50-63)"""
    v = int(v)
    if address == EDGE:
        return min(max(v, 0), n - 1)
    if address == ZERO:
        return v if 0 <= v < n else None
    if address == MIRROR:
        m = v % (2 * n)
        return m if m < n else 2 * n - 1 - m
    return v % n


def _fetch(img, t, xs, ys) -> np.ndarray:
    """texels [len, 4] float64 at integer coordinates (any integers), zeros where ZERO says so"""
    out = np.zeros((len(xs), 4))
    for i, (x, y) in enumerate(zip(xs, ys)):
        xx, yy = wrap(t["address"], x, t["width"]), wrap(t["address"], y, t["height"])
        if xx is not None and yy is not None:
            out[i] = img[yy, xx]
    return out


def _pow(c, g):
    with np.errstate(all="ignore"):
        return np.power(c, g)  # IEEE pow: 0^g = 0 (g > 0), (-x)^g = +-x^g for an integer g, NaN for a fractional one


def _decode(t, c) -> np.ndarray:
    """image.cpp:138-153 on float64 [.., 4] (the texel widened, or the bilinear mix): the encoding, not yet the scale"""
    if t["encoding"] == SRGB:
        return np.where(c <= KNEE, c * float(np.float32(1.0 / 12.92)), _pow((c + float(np.float32(0.055))) * float(np.float32(1.0 / 1.055)), 2.4))
    if t["encoding"] == GAMMA:
        g = t["gamma"].astype(np.float64)
        return _pow(c, np.array([g[0], g[1], g[2], g[2]]))
    return c


def _relative_term(t):
    measured = {LINEAR: 0.0, SRGB: MEASURED_SRGB, GAMMA: MEASURED_GAMMA}[t["encoding"]]
    return np.inf if measured is None else MARGIN * measured


def _uv_band(uv, slack):
    """how far the lookup's own uv may lie from the float32 uv the judge is given: `slack` ulp of each component, or (ulp, absolute)"""
    ulps, absolute = slack if isinstance(slack, tuple) else (slack, 0.0)
    return ulps * np.spacing(np.abs(uv)).astype(np.float64) + absolute


def _coordinates(t, uv, uv_ulps):
    """texel coordinates X [n, 2] in float64 of the float32 uv, the bilinear F = X - 0.5 and their bands (uv_ulps None: no band at all -- the caller
    has shown that float32 makes no rounding on the way, exact_precondition)"""
    u = uv.astype(np.float64)
    s, o = t["uv_scale"].astype(np.float64), t["uv_offset"].astype(np.float64)
    size = np.array([t["width"], t["height"]], np.float64)
    us = u * s
    big_u = us + o
    if uv_ulps is None:
        return big_u * size, np.zeros(u.shape), big_u * size - 0.5, np.zeros(u.shape)
    d_u = EPS * (np.abs(us) + np.abs(big_u)) + np.abs(s) * _uv_band(uv, uv_ulps)
    x = big_u * size
    d_x = size * d_u + EPS * np.abs(x)
    f = x - 0.5
    d_f = d_x + EPS * np.abs(f)
    return x, d_x * HIGHER_ORDERS, f, d_f * HIGHER_ORDERS


def image_candidates(tables: Tables, t, uv, uv_ulps=0.0, decode_relative=None) -> dict:
    """the judge's answer for ONE image texture at the float32 uv [n, 2]: ref [n, K, 4] float64 (K = 4 candidates: the texel on either side in x
    and in y for a point lookup within its band of a border, all the same otherwise), bar [n, K, 4] (absolute, on ref), exact [n, K, 4] float32 (the
    float32 product scale * texel of a linear point lookup, NaN otherwise), bitwise [n] (exact is what must come back), maybe [n], delta [n, 2]"""
    img = tables.image(t).astype(np.float64)
    n = len(uv)
    x, d_x, f, d_f = _coordinates(t, uv, uv_ulps)
    scale = t["scale"].astype(np.float64)
    relative = _relative_term(t) if (decode_relative is None or t["encoding"] == LINEAR) else decode_relative  # (decode_relative: the bar of another float32 implementation, e.g. the oracle with libm)
    ref, bar = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    exact = np.full((n, 4, 4), np.nan, np.float32)
    if t["filter"] == POINT:
        lo, hi = np.floor(x - d_x), np.floor(x + d_x)
        maybe = (lo != hi).any(axis=1)
        wild = (hi - lo > 1).any(axis=1)  # the band spans more than two texels: float32 does not know the texel, and any finite value is accepted
        for k, (cx, cy) in enumerate(((lo, lo), (hi, lo), (lo, hi), (hi, hi))):
            c = _fetch(img, t, cx[:, 0], cy[:, 1])
            v = scale * _decode(t, c)
            ref[:, k] = v
            with np.errstate(invalid="ignore"):
                bar[:, k] = np.where(np.isfinite(v), np.abs(v) * (relative + (EPS if t["encoding"] != LINEAR else 0.0)), 0.0)
            if t["encoding"] == LINEAR:
                exact[:, k] = t["scale"] * c.astype(np.float32)
        bar[wild] = np.inf
        return {"ref": ref, "bar": bar, "exact": exact, "bitwise": np.full(n, t["encoding"] == LINEAR) & ~wild, "maybe": maybe, "delta": d_x}
    ix = np.floor(f)
    tx = f - ix
    # the 4 x 4 texels around the footprint: columns ix - 1 .. ix + 2, rows iy - 1 .. iy + 2
    block = np.zeros((n, 4, 4, 4))  # [record, row, column, channel]
    for r in range(4):
        for c in range(4):
            block[:, r, c] = _fetch(img, t, ix[:, 0] + (c - 1), ix[:, 1] + (r - 1))
    a, b, c, d = block[:, 1, 1], block[:, 1, 2], block[:, 2, 1], block[:, 2, 2]
    wx, wy = tx[:, 0:1], tx[:, 1:2]
    mix = (a * (1.0 - wx) + b * wx) * (1.0 - wy) + (c * (1.0 - wx) + d * wx) * wy
    step = np.maximum(np.abs(np.diff(block, axis=1)).max(axis=(1, 2)), np.abs(np.diff(block, axis=2)).max(axis=(1, 2)))  # [n, channel]
    largest = np.abs(block).max(axis=(1, 2))
    bar_mix = (d_f[:, 0:1] + d_f[:, 1:2]) * step * HIGHER_ORDERS + C_MIX * EPS * largest * HIGHER_ORDERS
    whole = np.abs(img).reshape(-1, 4).max(axis=0) * 2.0  # any two convex combinations of the image's texels (and zero) are this close
    bar_mix = np.where((d_f >= 1.0).any(axis=1)[:, None], whole[None, :], bar_mix)
    v = scale * _decode(t, mix)
    if t["encoding"] == LINEAR:
        bar_v = np.abs(scale) * bar_mix + EPS * np.abs(v)
    else:  # the encodings are monotone where they are continuous: the band's ends bound what lies between
        ends = np.maximum(np.abs(scale * _decode(t, mix - bar_mix) - v), np.abs(scale * _decode(t, mix + bar_mix) - v))
        with np.errstate(invalid="ignore"):
            bar_v = np.where(np.isfinite(ends), ends, np.inf) + np.abs(v) * (relative + EPS)
    for k in range(4):
        ref[:, k], bar[:, k] = v, bar_v
    return {"ref": ref, "bar": bar, "exact": exact, "bitwise": np.zeros(n, bool), "maybe": np.zeros(n, bool), "delta": d_f}


def candidates(tables: Tables, tex, uv, uv_ulps=0.0, decode_relative=None) -> dict:
    """image_candidates for any texture ids tex [N] (Constant / Image / Checkerboard over Constant or Image children) at uv [N, 2] float32;
    K = 8: a checkerboard within its band of a cell border accepts either child"""
    tex, uv = np.asarray(tex, np.int64), np.ascontiguousarray(uv, np.float32)
    n = len(tex)
    out = {"ref": np.zeros((n, 8, 4)), "bar": np.zeros((n, 8, 4)), "exact": np.full((n, 8, 4), np.nan, np.float32), "bitwise": np.zeros(n, bool),
           "maybe": np.zeros(n, bool), "delta": np.zeros((n, 2))}

    def plain(ids, rows, slots):
        """Constant / Image textures `ids` of the records `rows` into the candidate slots `slots` (4 of the 8)"""
        for i in np.unique(ids):
            m = rows[ids == i]
            t = tables.textures[int(i)]
            if t["kind"] == CONSTANT:
                for k in slots:
                    out["ref"][m, k], out["exact"][m, k] = t["v"].astype(np.float64), t["v"]
                got = {"bitwise": True, "maybe": False}
            else:
                assert t["kind"] == IMAGE
                got = image_candidates(tables, t, uv[m], uv_ulps, decode_relative)
                for j, k in enumerate(slots):
                    out["ref"][m, k], out["bar"][m, k], out["exact"][m, k] = got["ref"][:, j], got["bar"][:, j], got["exact"][:, j]
                out["delta"][m] = got["delta"]
            yield m, got

    rows = np.arange(n)
    kinds = np.array([tables.textures[int(i)]["kind"] for i in tex])
    direct = kinds != CHECKERBOARD
    for m, got in plain(tex[direct], rows[direct], range(4)):
        out["bitwise"][m], out["maybe"][m] = got["bitwise"], got["maybe"]
        out["ref"][m, 4:], out["bar"][m, 4:], out["exact"][m, 4:] = out["ref"][m, :4], out["bar"][m, :4], out["exact"][m, :4]
    for i in np.unique(tex[~direct]):
        m = rows[tex == i]
        t = tables.textures[int(i)]
        cs = float(t["checker_scale"])
        c = uv[m].astype(np.float64) * cs
        d_c = (EPS * np.abs(c) + abs(cs) * _uv_band(uv[m], uv_ulps or 0.0)) * HIGHER_ORDERS
        lo, hi = np.floor(c - d_c), np.floor(c + d_c)
        border = (lo != hi).any(axis=1)
        parity = (np.floor(c).sum(axis=1).astype(np.int64)) & 1  # floor is an integer of either sign: & 1 is its parity in two's complement too
        for which, slots in ((parity, range(4)), (np.where(border, 1 - parity, parity), range(4, 8))):
            child = np.array([t["child"][int(p)] for p in which], np.int64)
            default = child < 0  # checkerboard.cpp: no child -> white (on) / black (off)
            for k in slots:
                value = np.where(which[default, None] == 1, np.float32([0, 0, 0, 1]), np.float32([1, 1, 1, 1]))
                out["ref"][m[default], k], out["exact"][m[default], k] = value, value
            both = np.ones(len(m), bool)
            for mm, got in plain(child[~default], m[~default], slots):
                at = np.searchsorted(m, mm)
                both[at] = got["bitwise"]
                out["maybe"][mm] |= got["maybe"]
            if slots[0] == 0:
                out["bitwise"][m] = both
            else:
                out["bitwise"][m] &= both
        out["maybe"][m] |= border
    return out


# the consumers' rules (float64 on ref and bar, float32 on exact).  NaN: fmaxf / fminf return the other operand, as np.fmax / np.fmin do.
def _extend(v, channels):
    """extend_rgb, texture.cpp:14-18, on [.., 4] -> [.., 3] for per-record channel counts"""
    ch = np.asarray(channels).reshape((-1,) + (1,) * (v.ndim - 2))
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    one = np.ones_like(x)
    return np.stack([x, np.where(ch == 1, x, y), np.where(ch == 1, x, np.where(ch == 2, one, z))], axis=-1)


def consume(c: dict, role: str, channels=None, light_scale=None, remap=None) -> dict:
    """the consumer's rule over candidates() -> ref, bar [N, K, 3 (roughness: 2)], exact float32, bitwise, maybe"""
    ref, bar, exact = c["ref"], c["bar"], c["exact"]
    if role == "albedo":  # resolve_closure: saturate(extend_rgb(tex, channels)); clamping moves nothing further apart
        sat = lambda a: np.fmin(np.fmax(a, a.dtype.type(0)), a.dtype.type(1))  # noqa: E731
        return {**c, "ref": sat(_extend(ref, channels)), "bar": _extend(bar, channels), "exact": sat(_extend(exact, channels))}
    if role == "emission":  # light_evaluate_with: max0(xyz) * light.scale: one more rounding
        ls = np.asarray(light_scale, np.float32).reshape(-1, 1, 1)
        r = np.fmax(ref[..., :3], 0.0) * ls.astype(np.float64)
        return {**c, "ref": r, "bar": bar[..., :3] * ls.astype(np.float64) + EPS * np.abs(r), "exact": np.fmax(exact[..., :3], np.float32(0)) * ls}
    if role == "raw":
        return {**c, "ref": ref[..., :3], "bar": bar[..., :3], "exact": exact[..., :3]}
    assert role == "roughness"  # resolve_closure's alpha of a Mirror, then closure_albedo_roughness
    ch = np.asarray(channels).reshape(-1, 1, 1)
    r = np.stack([ref[..., 0], np.where(ch[..., 0] == 1, ref[..., 0], ref[..., 1])], axis=-1)
    b = np.stack([bar[..., 0], np.where(ch[..., 0] == 1, bar[..., 0], bar[..., 1])], axis=-1)
    floor = float(np.float32(1e-4))

    def rule(x):
        alpha = np.fmax(x * x, floor) if remap else x
        return np.sqrt(np.fmax(alpha, floor))
    out = rule(r)
    spread = np.maximum(np.abs(rule(r - b) - out), np.abs(rule(r + b) - out))  # monotone in |x| on either side of 0
    return {**c, "ref": out, "bar": spread + ROUGHNESS_EPS * EPS * np.abs(out), "exact": np.full(out.shape, np.nan, np.float32),
            "bitwise": np.zeros(len(out), bool)}


def verdicts(c: dict, got) -> dict:
    """got [N, 3 or 2] float32 against the consumed candidates -> ok [N] (some candidate accepts the record: equal to its float32 value where the
    record is bitwise -- -0 and +0 are the same value here --, within its bar otherwise, NaN only where NaN is the answer), excess [N] = the
    error over the bar of the best candidate (0 for an exact match; inf for a miss of a bitwise record)"""
    got64 = np.asarray(got, np.float64)[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        same = (got64 == c["exact"].astype(np.float64)) | (np.isnan(got64) & np.isnan(c["exact"].astype(np.float64)))
        err = np.abs(got64 - c["ref"])
        both_nan = np.isnan(got64) & np.isnan(c["ref"])
        ratio = np.where(both_nan | (err == 0.0), 0.0, np.where(np.isnan(err), np.inf, err / c["bar"]))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    per_candidate = np.where(c["bitwise"][:, None], np.where(same.all(axis=2), 0.0, np.inf), ratio.max(axis=2))
    excess = per_candidate.min(axis=1)
    return {"ok": excess <= 1.0, "excess": excess}


def relative_error(c: dict, got) -> float:
    """the largest |got - ref| / |ref| over the SURE records' finite non-zero references (what MEASURED_* record)"""
    sure = ~c["maybe"]
    ref, got = c["ref"][sure, 0], np.asarray(got, np.float64)[sure]
    use = np.isfinite(ref) & (ref != 0.0)
    return float((np.abs(got[use] - ref[use]) / np.abs(ref[use])).max()) if use.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------- the float32 restatement
def _f32(x):
    return np.asarray(x, np.float32)


def texel_wrap32(address, v, n, drop_correction=False, one_step_only=False, mirror_off_by_one=False, first_step_by_n=False):
    """dev_shade.h: texel_wrap, literally, on int32 arrays -> (index int32, zero bool).  The mistakes: the corrective step left out, the 2^20 switch
    left out, MIRROR folded with period - m"""
    v = np.asarray(v, np.int32)
    if address == EDGE:
        return np.clip(v, 0, n - 1).astype(np.int32), np.zeros(v.shape, bool)
    if address == ZERO:
        out = (v < 0) | (v >= n)
        return np.where(out, 0, v).astype(np.int32), out
    period = np.int32(2 * n if address == MIRROR else n)
    inv_period = np.float32(1.0) / np.float32(period)
    m = v.copy()
    far = ~((v > -(1 << 20)) & (v < (1 << 20)))
    if not one_step_only and far.any():
        q = np.floor(v.astype(np.float32) * inv_period).astype(np.int32)
        with np.errstate(over="ignore"):
            stepped = (v.astype(np.uint32) - q.astype(np.uint32) * np.uint32(n if first_step_by_n else period)).astype(np.int32)  # the products wrap around consistently
        m = np.where(far, stepped, m)
    q = np.floor(m.astype(np.float32) * inv_period).astype(np.int32)
    with np.errstate(over="ignore"):
        m = (m.astype(np.uint32) - q.astype(np.uint32) * np.uint32(period)).astype(np.int32)  # (int arithmetic of the device: two's complement)
    if not drop_correction:
        m = m + np.where(m < 0, period, 0).astype(np.int32)
        m = m - np.where(m >= period, period, 0).astype(np.int32)
    if address == MIRROR:
        m = np.where(m >= n, period - (0 if mirror_off_by_one else 1) - m, m)
    return m.astype(np.int32), np.zeros(v.shape, bool)


def pack_bytes(img):
    """lrhip_tables.hip: pack_byte_textures for ONE image float32 [h, w, 4] -> None (stays float) or (words uint32 [h, w], form 1 | 2, constant
    channel mask, the constant channels' values float32 [4])"""
    px = img.reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        inside = (px >= 0) & (px <= 1)
        code = np.where(inside, np.floor(px * np.float32(255.0) + np.float32(0.5)), np.float32(-1.0)).astype(np.float32)
    k = np.float32(1.0) / np.float32(255.0)
    same = (px == px[0]).all(axis=0)
    product = ((code >= 0) & (code * k == px)).all(axis=0)
    quotient = ((code >= 0) & (code / np.float32(255.0) == px)).all(axis=0)
    for form, coded in ((1, product), (2, quotient)):
        constant = ~coded & same
        if (coded | same).all() and not constant.all():
            codes = np.where(constant[None, :], 0, np.maximum(code, 0)).astype(np.uint32) & 255
            words = codes[:, 0] | (codes[:, 1] << 8) | (codes[:, 2] << 16) | (codes[:, 3] << 24)
            mask = int(sum(1 << c for c in range(4) if constant[c]))
            return words.reshape(img.shape[:2]), form, mask, px[0].copy()
    return None


def _texel_at32(tables, t, xx, yy, storage, form_2_as_1=False, constant_from_word=False):
    """dev_shade.h: texel_at -> float32 [n, 3] (x, y, z; the device reads no fourth channel)"""
    img = tables.image(t)
    outside = (xx < 0) | (xx >= t["width"]) | (yy < 0) | (yy >= t["height"])
    if outside.any():  # only a mistaken wrap gets here, and the device would read out of bounds: NaN stands for whatever lies there
        inside = _texel_at32(tables, t, np.clip(xx, 0, t["width"] - 1), np.clip(yy, 0, t["height"] - 1), storage, form_2_as_1, constant_from_word)
        return np.where(outside[:, None], np.float32(np.nan), inside)
    packed = pack_bytes(img) if storage == 2 else None
    if packed is None:
        return img[yy, xx, :3]
    words, form, mask, values = packed
    p = words[yy, xx]
    k = np.float32(0.0) if (form == 1 or form_2_as_1) else np.float32(1.0) / np.float32(255.0)
    out = np.zeros((len(p), 3), np.float32)
    for c in range(3):
        f = ((p >> np.uint32(8 * c)) & np.uint32(255)).astype(np.float32)
        q = f * (np.float32(1.0) / np.float32(255.0))
        r = (f.astype(np.float64) - q.astype(np.float64) * 255.0).astype(np.float32)        # fmaf(-q, 255, f): one rounding (the sum is exact in float64)
        v = (r.astype(np.float64) * float(k) + q.astype(np.float64)).astype(np.float32)     # fmaf(r, k, q)
        out[:, c] = v if (constant_from_word or not (mask >> c) & 1) else values[c]
    return out


def device_lookup(tables: Tables, tex, uv, storage=0, contract=False, mistake=None) -> np.ndarray:
    """dev_shade.h: texture_eval_tables in float32 numpy -> [N, 3] (x, y, z).  contract: u * s + o and U * w - 0.5 as one fma each, as a build
    with contraction makes them.  mistake: one of MISTAKES"""
    tex, uv = np.asarray(tex, np.int64), np.ascontiguousarray(uv, np.float32)
    out = np.zeros((len(tex), 3), np.float32)
    rows = np.arange(len(tex))
    pending = [(tex, rows)]
    while pending:
        ids, at = pending.pop()
        for i in np.unique(ids):
            m = at[ids == i]
            t = tables.textures[int(i)]
            if t["kind"] == CONSTANT:
                out[m] = t["v"][:3]
            elif t["kind"] == CHECKERBOARD:
                c = np.floor(uv[m] * t["checker_scale"]).astype(np.int32)
                parity = (c[:, 0] + c[:, 1]) & 1
                child = np.array([t["child"][int(p)] for p in parity], np.int64)
                none = child < 0
                out[m[none]] = np.where(parity[none, None] == 1, np.float32(0), np.float32(1))
                pending.append((child[~none], m[~none]))
            else:
                out[m] = _image32(tables, t, uv[m], storage, contract, mistake)
    return out


MISTAKES = ("no corrective step", "no 2^20 switch", "mirror period - m", "no half texel", "tx and ty swapped", "a zero flag ignored",
            "byte form 2 as form 1", "constant channel from the word", "sRGB knee at 0.0031308", "first step by n under MIRROR")
# ("no 2^20 switch" is no mistake AT 2^20: one step is exact while |v / period| < 2^20 and good for a while beyond; the `exact` family's coordinates
# of 2^23 and more reject it.  "first step by n under MIRROR" -- the first of the two steps takes q * n off instead of q * period -- is wrong wherever
# the two-step path runs: the families around +-2^20 reject it, which shows that they exercise that path)


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(np.float32)  # (exact product; the sum rounds at 53 bits first)


def _image32(tables, t, uv, storage, contract, mistake):
    assert mistake is None or mistake in MISTAKES
    s, o = t["uv_scale"], t["uv_offset"]
    big_u = _fma32(uv, s[None, :], o[None, :]) if contract else uv * s[None, :] + o[None, :]
    w, h = t["width"], t["height"]
    size = np.float32([w, h])
    wraps = {"drop_correction": mistake == "no corrective step", "one_step_only": mistake == "no 2^20 switch",
             "mirror_off_by_one": mistake == "mirror period - m", "first_step_by_n": mistake == "first step by n under MIRROR"}
    texel = functools.partial(_texel_at32, tables, t, storage=storage, form_2_as_1=mistake == "byte form 2 as form 1",
                              constant_from_word=mistake == "constant channel from the word")
    if t["filter"] == POINT:
        xy = np.floor(big_u * size).astype(np.int32)
        xx, zx = texel_wrap32(t["address"], xy[:, 0], w, **wraps)
        yy, zy = texel_wrap32(t["address"], xy[:, 1], h, **wraps)
        v = np.where((zx | zy)[:, None], np.float32(0), texel(xx, yy))
    else:
        half = np.float32(0.0 if mistake == "no half texel" else 0.5)
        f = _fma32(big_u, size, -half) if contract else big_u * size - half
        f0 = np.floor(f)
        tt = f - f0
        tx, ty = (tt[:, 1:2], tt[:, 0:1]) if mistake == "tx and ty swapped" else (tt[:, 0:1], tt[:, 1:2])
        i0 = f0.astype(np.int32)
        with np.errstate(over="ignore"):
            i1 = (i0 + np.int32(1)).astype(np.int32)
        xa, zx0 = texel_wrap32(t["address"], i0[:, 0], w, **wraps)
        xb, zx1 = texel_wrap32(t["address"], i1[:, 0], w, **wraps)
        ya, zy0 = texel_wrap32(t["address"], i0[:, 1], h, **wraps)
        yb, zy1 = texel_wrap32(t["address"], i1[:, 1], h, **wraps)
        none = np.float32(0)
        c00 = np.where((zx0 | zy0)[:, None], none, texel(xa, ya))
        c10 = np.where((zx1 | zy0)[:, None], none, texel(xb, ya))
        c01 = np.where((zx0 | zy1)[:, None], none, texel(xa, yb))
        c11 = np.where(((zx1 & (mistake != "a zero flag ignored")) | zy1)[:, None], none, texel(xb, yb))
        one = np.float32(1.0)
        v = (c00 * (one - tx) + c10 * tx) * (one - ty) + (c01 * (one - tx) + c11 * tx) * ty
    v = v.astype(np.float32)
    if t["encoding"] == SRGB:
        knee = np.float32(0.0031308 if mistake == "sRGB knee at 0.0031308" else 0.04045)
        x = (v + np.float32(0.055)) * np.float32(1.0 / 1.055)
        with np.errstate(all="ignore"):
            v = np.where(v <= knee, v * np.float32(1.0 / 12.92), x * x * np.exp2(np.float32(0.4) * np.log2(x))).astype(np.float32)
    elif t["encoding"] == GAMMA:
        v = _pow(v.astype(np.float64), t["gamma"].astype(np.float64)[None, :]).astype(np.float32)  # (pow_nonpositive's cases are IEEE pow's)
    return (t["scale"][None, :3] * v).astype(np.float32)


def consume32(v, role, channels=None, light_scale=None, remap=None):
    """the consumer's rule in float32 on device_lookup's [N, 3]"""
    v = _f32(v)
    if role == "raw":
        return v
    if role == "emission":
        return np.fmax(v, np.float32(0)) * _f32(light_scale).reshape(-1, 1)
    v4 = np.concatenate([v, np.ones((len(v), 1), np.float32)], axis=1)
    if role == "albedo":
        return np.fmin(np.fmax(_extend(v4, channels), np.float32(0)), np.float32(1)).astype(np.float32)
    ch = np.asarray(channels)
    r = np.stack([v[:, 0], np.where(ch == 1, v[:, 0], v[:, 1])], axis=1)
    alpha = np.fmax(r * r, np.float32(1e-4)) if remap else r
    return np.sqrt(np.fmax(alpha, np.float32(1e-4))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- quads, records, scenes
UNIT = ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0))  # a quad's vertex uvs; its triangles are (0, 1, 2) and (0, 2, 3)
QUAD_PITCH = 2.0  # quad q covers [2 q, 2 q + 1] x [0, 1] in the plane z = 0, its front towards +z


def square(lo, hi):
    return ((lo, lo), (hi, lo), (hi, hi), (lo, hi))


def interpolate_uv(quad_uvs, prim, u, v) -> np.ndarray:
    """reconstruct<true>'s uv in float32: bary.x uv0 + bary.y uv1 + bary.z uv2 with bary = (1 - u - v, u, v), per record; quad_uvs [N, 4, 2]"""
    quad_uvs, u, v = _f32(quad_uvs), _f32(u), _f32(v)
    corner = np.where(np.asarray(prim)[:, None] == 0, [0, 1, 2], [0, 2, 3])
    uv0, uv1, uv2 = (quad_uvs[np.arange(len(u)), corner[:, k]] for k in range(3))
    w = np.float32(1.0) - u - v
    return (w[:, None] * uv0 + u[:, None] * uv1 + v[:, None] * uv2).astype(np.float32)


def records_for_unit_uv(x, y):
    """(prim, u, v) of the point with uv = (x, y) on a UNIT quad: triangle 0 holds x >= y with uv = (u + v, v), triangle 1 uv = (u, u + v)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    first = x >= y
    return np.where(first, 0, 1).astype(np.uint32), np.where(first, x - y, x).astype(np.float32), np.where(first, y, y - x).astype(np.float32)


def hit_records(quad, prim, u, v) -> np.ndarray:
    """lrhip_ray_hit records as a caller makes them: (t, u, v, inst), (prim, tri = LR_INVALID_ID, -, -)"""
    rec = np.zeros((len(quad), 8), np.float32)
    ids = rec.view(np.uint32)
    rec[:, 1], rec[:, 2] = u, v
    ids[:, 3], ids[:, 4], ids[:, 5] = quad, prim, INVALID
    return rec


def _number(x) -> str:
    x = float(x)
    return "-0.0" if (x == 0.0 and math.copysign(1.0, x) < 0) else repr(x)


def texture_sdl(spec: dict) -> str:
    if spec["kind"] == "constant":
        return "Constant { v { " + ", ".join(_number(x) for x in spec["v"]) + " } }"
    if spec["kind"] == "checker":
        children = "".join(f"{name} : {texture_sdl(spec[name])} " for name in ("on", "off") if spec.get(name) is not None)
        return f"Checkerboard {{ {children}scale {{ {_number(spec['scale'])} }} }}"
    gamma = f" gamma {{ {_number(spec['gamma'])} }}" if spec.get("encoding", "linear") == "gamma" else ""
    sx, sy = spec.get("uv_scale", (1.0, 1.0))
    ox, oy = spec.get("uv_offset", (0.0, 0.0))
    return (f'Image {{ file {{ "{spec["file"]}" }} encoding {{ "{spec.get("encoding", "linear")}" }}{gamma} filter {{ "{spec.get("filter", "point")}" }} '
            f'address {{ "{spec.get("address", "repeat")}" }} uv_scale {{ {_number(sx)}, {_number(sy)} }} uv_offset {{ {_number(ox)}, {_number(oy)} }} '
            f'scale {{ {_number(spec.get("scale", 1.0))} }} }}')


LIGHT_SCALE = 1.5
ROLES = ("albedo", "roughness", "emission", "alpha")


def scene_text(quads: list, role: str, remap: bool = True, extra_shapes: str = "", camera: str = "", integrator: str = "MegaPath { depth { 2 } }") -> str:
    """one quad per entry of `quads` (dicts: uvs, texture), its texture in the `role`: a Matte's Kd, a Mirror's roughness, the emission of a one-sided
    Diffuse light WITHOUT a surface, a Matte's alpha"""
    shapes, names = [], []
    for q, quad in enumerate(quads):
        x0 = QUAD_PITCH * q
        tex = texture_sdl(quad["texture"])
        what = {"albedo": f"surface : Matte {{ Kd : {tex} }}",
                "roughness": f"surface : Mirror {{ color : Constant {{ v {{ 1 }} }} roughness : {tex} remap_roughness {{ {'true' if remap else 'false'} }} }}",
                "emission": f"light : Diffuse {{ emission : {tex} scale {{ {LIGHT_SCALE} }} }}",
                "alpha": f"surface : Matte {{ Kd : Constant {{ v {{ 0.5 }} }} alpha : {tex} }}"}[role]
        uvs = ", ".join(f"{_number(a)},{_number(b)}" for a, b in quad["uvs"])
        shapes.append(f"Shape q{q} : InlineMesh {{ positions {{ {x0},0,0, {x0 + 1},0,0, {x0 + 1},1,0, {x0},1,0 }} uvs {{ {uvs} }} indices {{ 0,1,2, 0,2,3 }} {what} }}")
        names.append(f"@q{q}")
    camera = camera or "Camera cam : Pinhole { fov { 30 } spp { 1 } film : Color { resolution { 8, 8 } } position { 0.5, 0.5, 3 } look_at { 0.5, 0.5, 0 } }"
    extra_names = "".join(", @" + line.split()[1] for line in extra_shapes.splitlines() if line.startswith("Shape "))
    return "\n".join(shapes) + "\n" + extra_shapes + camera + "\nrender { cameras { @cam } shapes { " + ", ".join(names) + extra_names + " } integrator : " + integrator + " }\n"


class Family:
    """quads (uvs, texture spec), images {file: float32 [h, w, 3] for a .pfm, uint8 [h, w, 3] for a .png}, and the records (quad, prim, u, v) [n]"""

    def __init__(self, name, quads, images, quad, prim, u, v):
        self.name, self.quads, self.images = name, quads, images
        self.quad, self.prim, self.u, self.v = np.asarray(quad, np.uint32), np.asarray(prim, np.uint32), _f32(u), _f32(v)
        assert len(self.quad) <= N and len(self.quad) % 64 != 0 and len(self.quad) > 256, (name, len(self.quad))
        for a in (self.quad, self.prim, self.u, self.v):
            a.setflags(write=False)

    def __len__(self):
        return len(self.quad)

    def write_images(self, folder) -> None:
        for name, pixels in self.images.items():
            (write_png if name.endswith(".png") else write_pfm)(str(folder / name), pixels)

    def scene(self, folder, role: str, **kwargs) -> Scene:
        self.write_images(folder)
        path = folder / f"{self.name}_{role}.luisa"
        path.write_text(scene_text(self.quads, role, **kwargs))
        return Scene.load(str(path))

    def hits(self) -> np.ndarray:
        return hit_records(self.quad, self.prim, self.u, self.v)

    def uv(self) -> np.ndarray:
        """the uv of every record as reconstruct<true> makes it, in float32"""
        return interpolate_uv(np.float32([q["uvs"] for q in self.quads])[self.quad], self.prim, self.u, self.v)

    def rays(self, height=1.0) -> np.ndarray:
        """rays straight down -z onto the records' points, for the channels that trace"""
        corner = np.where(self.prim[:, None] == 0, [0, 1, 2], [0, 2, 3])
        px, py = np.float64([0, 1, 1, 0]), np.float64([0, 0, 1, 1])
        b = np.stack([1.0 - self.u.astype(np.float64) - self.v, self.u, self.v], axis=1)
        rays = np.zeros((len(self), 8), np.float32)
        rays[:, 0] = QUAD_PITCH * self.quad + (b * px[corner]).sum(axis=1)
        rays[:, 1], rays[:, 2], rays[:, 6], rays[:, 7] = (b * py[corner]).sum(axis=1), height, -1.0, np.inf
        return rays


def _picture(rng, w, h, wide):
    """distinct texels: a wrong texel never looks right.  wide: values an emission may hold (negative, above 1); else inside [0, 1]"""
    return (rng.uniform(-0.5, 3.0, (h, w, 3)) if wide else rng.uniform(0.05, 0.95, (h, w, 3))).astype(np.float32)


def _random_barycentrics(rng, n):
    a, b = rng.random(n), rng.random(n)
    flip = a + b > 1.0
    return np.where(flip, 1.0 - a, a).astype(np.float32), np.where(flip, 1.0 - b, b).astype(np.float32)


# ---- exact
SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (13, 7), (16, 16))  # (width, height): the periods that are no power of two are where 1 / period is inexact
GRID = 4096  # a UNIT quad's uv are k / GRID: twelve bits


def _windows(n: int, point: bool, wrapping: bool) -> list:
    """(e, k0) per window: the axis' uv transform is U = (k + k0) 2^e for uv = k / GRID, so the texel coordinate X = n (k + k0) 2^e is a float32
    bit for bit under either contraction (exact_precondition checks it).  Fine windows -- eighths of U (quarters for bilinear: F's fraction is 0, 1/4,
    1/2 or 3/4), sixteenths where n > 8, so that n 2^e <= 1 and EVERY integer is some floor(X) although the period is no power of two -- around 0;
    eighths around +-2^20, where the device switches paths (a coordinate of 21 bits has three left for its fraction); whole multiples of n (e = 0)
    around +-2^23 (+-2^22 bilinear), where odd multiples fold under MIRROR; multiples of n 2^e up to +-2^30 for the point filter (beyond 2^24
    float(v) has rounded: only such coordinates exist in float32)"""
    fine = min(-3 if point else -2, -math.ceil(math.log2(n)))
    near = max(fine, -3)
    at = lambda centre, e: int(round(centre / (n * 2.0 ** e))) - GRID // 2  # noqa: E731
    top = float(2 ** 23 if point else 2 ** 22) - (GRID // 2) * n
    e_max = 19 - math.ceil(math.log2(n))  # n 2^e_max 2048 <= 2^30
    if wrapping:
        w = [(fine, -GRID // 2), (near, at(2.0 ** 20, near)), (near, at(-2.0 ** 20, near)), (0, at(top, 0)), (0, at(-top, 0))]
        return w + [(6, -GRID // 2), (12, -GRID // 2), (e_max, -GRID // 2)] if point else w
    return [(fine, -GRID // 2), (near, at(2.0 ** 20, near)), (0, at(top, 0)), (e_max, -GRID // 2)] if point else [(fine, -GRID // 2), (near, at(-2.0 ** 20, near)), (0, at(top, 0))]


def _special_steps(n, address, point, e, k0):
    """k in [0, GRID) split into (must, special): the texel coordinate's floor is +-2^20 or next to it / a multiple of the period or of twice the
    period or next to one, or beyond 2^24"""
    k = np.arange(GRID)
    x = n * (k + k0) * 2.0 ** e
    t = np.floor(x if point else x - 0.5).astype(np.int64)
    p = 2 * n if address == MIRROR else n
    wanted = [s * m + d for s in (-1, 1) for m in (2 ** 20, p, 2 * p) for d in (-1, 0, 1)]  # ONE step for each of these floors, where the window has one
    first = [int(np.argmax(t == value)) for value in dict.fromkeys(wanted) if (t == value).any()]
    must = np.zeros(GRID, bool)
    must[first] = True
    special = np.isin(t % p, (0, 1, p - 1)) | np.isin(t % (2 * p), (0, 1, 2 * p - 1)) | (np.abs(t) >= 2 ** 24)
    return k[must], k[special & ~must]


def _exact(wide: bool) -> Family:
    rng = np.random.default_rng(20)
    images = {f"exact_{w}x{h}.pfm": _picture(rng, w, h, wide) for w, h in SIZES}
    quads, plans = [], []
    for w, h in SIZES:
        for name, address in ADDRESSES.items():
            for point in (True, False):
                wx, wy = _windows(w, point, address in (REPEAT, MIRROR)), _windows(h, point, address in (REPEAT, MIRROR))
                slots = range(len(wx)) if (w, h) != (1, 1) else (0, len(wx) - 1)
                for j in slots:
                    (ex, kx), (ey, ky) = wx[j], wy[(j + 2) % len(wy)]
                    quads.append({"uvs": UNIT, "texture": {
                        "kind": "image", "file": f"exact_{w}x{h}.pfm", "filter": "point" if point else "bilinear", "address": name,
                        "uv_scale": (GRID * 2.0 ** ex, GRID * 2.0 ** ey), "uv_offset": (kx * 2.0 ** ex, ky * 2.0 ** ey), "scale": 1.0 if j % 2 == 0 else 0.75}})
                    plans.append((_special_steps(w, address, point, ex, kx), _special_steps(h, address, point, ey, ky)))
    per_quad = N // len(quads)
    extra = N - per_quad * len(quads)
    quad, x, y = [], [], []
    for q, plan in enumerate(plans):
        count = per_quad + (1 if q < extra else 0)
        steps = []
        for must, special in plan:
            rest = count - min(len(must), count)
            picked = np.concatenate([must[:count], rng.choice(special, rest // 2) if len(special) else np.zeros(0, np.int64), rng.integers(0, GRID, rest)])[:count]
            steps.append(rng.permutation(picked.astype(np.int64)))
        quad += [q] * count
        x.append(steps[0])
        y.append(steps[1])
    prim, u, v = records_for_unit_uv(np.concatenate(x) / GRID, np.concatenate(y) / GRID)
    return Family("exact", quads, images, quad, prim, u, v)


def exact_records(tables: Tables, tex, prim, u, v) -> np.ndarray:
    """which records (prim, u, v) on UNIT quads reach their texel coordinate without a single rounding in float32 -- barycentrics, uv, u * s + o, * w
    and, under the bilinear filter, - 0.5 -- so that every build of the lookup, contracted or not, holds the very same coordinate: bool [N].  (For
    barycentrics a TRACE returned: rays straight down onto dyadic points of quads at dyadic places are intersected without rounding too.)"""
    u32, v32 = _f32(u), _f32(v)
    u64, v64 = u32.astype(np.float64), v32.astype(np.float64)
    uv = interpolate_uv(np.tile(_f32(UNIT), (len(u32), 1, 1)), np.asarray(prim), u32, v32)
    first = np.asarray(prim) == 0
    want = np.stack([np.where(first, u64 + v64, u64), np.where(first, v64, u64 + v64)], axis=1)
    ok = ((np.float32(1.0) - u32 - v32).astype(np.float64) == 1.0 - u64 - v64) & (uv.astype(np.float64) == want).all(axis=1)
    for i in np.unique(tex):
        m = np.asarray(tex) == i
        t = tables.textures[int(i)]
        if t["kind"] != IMAGE:
            ok[m] = False
            continue
        s, o, size = t["uv_scale"], t["uv_offset"], np.float32([t["width"], t["height"]])
        us = uv[m].astype(np.float64) * s.astype(np.float64)
        x = (us + o.astype(np.float64)) * size.astype(np.float64)
        same = ((uv[m] * s).astype(np.float64) == us) & ((uv[m] * s + o).astype(np.float64) == us + o.astype(np.float64)) & \
               (((uv[m] * s + o) * size).astype(np.float64) == x) & (np.abs(x) <= 2.0 ** 30)
        if t["filter"] == BILINEAR:
            same &= ((uv[m] * s + o) * size - np.float32(0.5)).astype(np.float64) == x - 0.5
        ok[m] &= same.all(axis=1)
    return ok


def exact_precondition(family: Family, tables: Tables, tex) -> np.ndarray:
    """asserts what makes the `exact` family exact: every float32 operation from the barycentrics to the texel coordinate (and to F = X - 0.5 under the
    bilinear filter) is exact, contracted or not, so that float32 equals float64 and the band is 0.  Returns the texel coordinates [N, 2] float64"""
    uv = family.uv()
    u64, v64 = family.u.astype(np.float64), family.v.astype(np.float64)
    assert np.array_equal((1.0 - u64 - v64).astype(np.float32).astype(np.float64), 1.0 - u64 - v64)
    first = family.prim == 0
    want = np.stack([np.where(first, u64 + v64, u64), np.where(first, v64, u64 + v64)], axis=1)
    assert np.array_equal(uv.astype(np.float64), want)
    out = np.zeros((len(family), 2))
    for i in np.unique(tex):
        m = tex == i
        t = tables.textures[int(i)]
        s, o, size = t["uv_scale"], t["uv_offset"], np.float32([t["width"], t["height"]])
        us = uv[m].astype(np.float64) * s.astype(np.float64)
        big_u = us + o.astype(np.float64)
        x = big_u * size.astype(np.float64)
        f = x - 0.5
        assert np.array_equal((uv[m] * s).astype(np.float64), us) and np.array_equal((uv[m] * s + o).astype(np.float64), big_u)
        assert np.array_equal(((uv[m] * s + o) * size).astype(np.float64), x) and (np.abs(x) <= 2.0 ** 30).all()
        if t["filter"] == BILINEAR:
            assert np.array_equal(((uv[m] * s + o) * size - np.float32(0.5)).astype(np.float64), f)
            frac = f - np.floor(f)
            assert np.array_equal(frac * 16.0, np.floor(frac * 16.0))  # dyadic weights: 0, 1/4, 1/2, 3/4 and, for the finer windows, sixteenths
        out[m] = x
    return out


# ---- seams
ADDRESS_SCALE, ADDRESS_OFFSET = (2.5, -3.0), (-0.7, 1.9)  # test_oracle_vs_ref.py: ADDRESS_SCENE


def _seams(wide: bool) -> Family:
    """bilinear footprints that straddle the image's border in x, in y and at its corners, under every address mode (ZERO: two or three of the four
    texels are zero), with the identity transform (u, v exactly 0.0 and 1.0 among them) and ADDRESS_SCENE's; two quads whose u (v) is -0.0 everywhere"""
    rng = np.random.default_rng(21)
    sizes = ((2, 2), (3, 5), (13, 7), (16, 16))
    images = {f"seams_{w}x{h}.pfm": _picture(rng, w, h, wide) for w, h in sizes}
    quads, kinds = [], []
    for w, h in sizes:
        for name in ADDRESSES:
            for s, o in (((1.0, 1.0), (0.0, 0.0)), (ADDRESS_SCALE, ADDRESS_OFFSET)):
                quads.append({"uvs": square(-1.0, 3.0), "texture": {"kind": "image", "file": f"seams_{w}x{h}.pfm", "filter": "bilinear", "address": name,
                                                                  "uv_scale": s, "uv_offset": o, "scale": 1.0}})
                kinds.append("square")
    for name in ("repeat", "zero"):
        for axis in (0, 1):
            uvs = tuple((-0.0, b) if axis == 0 else (b, -0.0) for b in (-1.0, -1.0, 3.0, 3.0))
            quads.append({"uvs": uvs, "texture": {"kind": "image", "file": "seams_13x7.pfm", "filter": "bilinear", "address": name, "scale": 1.0}})
            kinds.append(axis)
    per_quad = N // len(quads)
    quad, prim, u, v = [], [], [], []
    grid = 1024  # barycentrics are multiples of 1 / 1024: uv = -1 + 4 (.) is exact
    for q, (spec, kind) in enumerate(zip(quads, kinds)):
        t = spec["texture"]
        w, h = (int(x) for x in t["file"][6:-4].split("x"))
        count = per_quad + (1 if q < N - per_quad * len(quads) else 0)
        if kind != "square":  # uv.x (or .y) is -0.0; the other runs over [-1, 3] along the edge from vertex 1 to vertex 2: triangle 0, u + v = 1
            step = rng.integers(0, grid + 1, count)
            quad += [q] * count
            prim += [0] * count
            u += list((grid - step) / grid)
            v += list(step / grid)
            continue
        s, o = t.get("uv_scale", (1.0, 1.0)), t.get("uv_offset", (0.0, 0.0))

        def axis_values(n, k, near):
            """uv on the 1 / 256 grid of [-1, 3] whose U = uv s + o lies within a texel of a border (0 or 1) -- or anywhere"""
            target = rng.integers(0, 2, count) + rng.uniform(-1.0, 1.0, count) / n
            target[:4] = (0.0, 1.0, 0.0, 1.0)  # the border itself
            free = rng.uniform(-1.0, 3.0, count) * s[k] + o[k]
            uv = (np.where(near, target, free) - o[k]) / s[k]
            return np.clip(np.round(uv * 256.0) / 256.0, -1.0, 3.0)
        which = np.arange(count) % 3  # 0: the border in x, 1: in y, 2: a corner
        x, y = axis_values(w, 0, which != 1), axis_values(h, 1, which != 0)
        # on the square (-1, 3): triangle 0 holds x >= y with uv = -1 + 4 (u + v, v), triangle 1 uv = -1 + 4 (u, u + v)
        p, uu, vv = records_for_unit_uv((x + 1.0) / 4.0, (y + 1.0) / 4.0)
        quad += [q] * count
        prim += list(p)
        u += list(uu)
        v += list(vv)
    return Family("seams", quads, images, quad, prim, u, v)


# ---- generic
HUGE_SCALE = (170001.25, -290000.5)  # test_gpu_parity.py: texel coordinates beyond 2^20 under a free uv: the bands are a good part of a texel there
HUGE_POINT_RECORDS = 40                # ... so that a point lookup there is MAYBE more often than not: few of them, for the cap


def _generic(wide: bool) -> Family:
    """random uv over [-3, 4)^2 under ADDRESS_SCENE's transform, every address mode and both filters, judged with bands; and the same under
    HUGE_SCALE (the integer path of texel_wrap under a uv that is no dyadic number)"""
    rng = np.random.default_rng(22)
    sizes = ((13, 7), (16, 16), (3, 5))
    images = {f"generic_{w}x{h}.pfm": _picture(rng, w, h, wide) for w, h in sizes}
    quads, share = [], []
    for scale, these in ((ADDRESS_SCALE, sizes), (HUGE_SCALE, sizes[:1])):
        for w, h in these:
            for name in ADDRESSES:
                for filter_mode in ("point", "bilinear"):
                    uvs = square(-3.0, 4.0) if scale is ADDRESS_SCALE else UNIT
                    quads.append({"uvs": uvs, "texture": {"kind": "image", "file": f"generic_{w}x{h}.pfm", "filter": filter_mode, "address": name,
                                                          "uv_scale": scale, "uv_offset": ADDRESS_OFFSET, "scale": 0.75 if name == "mirror" else 1.0}})
                    share.append(HUGE_POINT_RECORDS // 4 if (scale is HUGE_SCALE and filter_mode == "point") else None)
    rest = N - sum(s for s in share if s is not None)
    free = sum(1 for s in share if s is None)
    counts = [s if s is not None else rest // free for s in share]
    counts[0] += N - sum(counts)
    quad = np.repeat(np.arange(len(quads)), counts)
    prim = rng.integers(0, 2, N)
    u, v = _random_barycentrics(rng, N)
    return Family("generic", quads, images, quad, prim, u, v)


# ---- decode
def _decode_family(wide: bool) -> Family:
    """point lookups at the centres of 16 x 16 images: sRGB texels on both sides of the knee 0.04045 (the float32 next below, the knee, the next
    above), at 0 and at 1; gamma 2.2 / 2 / 3 with zeros and negative texels; scale 0.75.  (The host gives all channels one `scale`.)"""
    rng = np.random.default_rng(23)
    knee = np.float32(0.04045)
    srgb = rng.uniform(0.0, 2.5 if wide else 1.0, (16, 16, 3)).astype(np.float32)
    srgb[0, :8] = np.float32([0.0, 1.0, np.nextafter(knee, np.float32(0)), knee, np.nextafter(knee, np.float32(1)), 0.04, 0.041, 1e-6])[:, None]
    srgb[1] = rng.uniform(0.0, 0.09, (16, 3))
    gamma = rng.uniform(0.0, 2.5 if wide else 1.0, (16, 16, 3)).astype(np.float32)
    gamma[::3, ::2] = 0.0
    gamma[1::4, 1::3] *= -1.0
    images = {"decode_srgb.pfm": srgb, "decode_gamma.pfm": gamma}
    specs = [("decode_srgb.pfm", "sRGB", None), ("decode_gamma.pfm", "gamma", 2.2), ("decode_gamma.pfm", "gamma", 2.0), ("decode_gamma.pfm", "gamma", 3.0),
             ("decode_srgb.pfm", "linear", None)]
    quads = [{"uvs": UNIT, "texture": {"kind": "image", "file": f, "encoding": e, "gamma": g, "filter": "point", "address": "repeat", "scale": 0.75}}
             for f, e, g in specs]
    centre = (np.arange(16) + 0.5) / 16.0
    cx, cy = (a.reshape(-1) for a in np.meshgrid(centre, centre))
    quad = np.concatenate([np.repeat(np.arange(len(quads)), 256), np.arange(3)])  # (no multiple of 64)
    prim, u, v = records_for_unit_uv(np.concatenate([np.tile(cx, len(quads)), cx[:3]]), np.concatenate([np.tile(cy, len(quads)), cy[5:8]]))
    return Family("decode", quads, images, quad, prim, u, v)


# ---- bytes
def _bytes(wide: bool) -> Family:
    """8-bit images of both host conversions: a PNG (b * (1 / 255.f): form 1) and a PFM that holds b / 255.f (the form of the other readers: form 2),
    each with all 256 codes; a second PFM whose blue channel is ONE value over the image, and no 8-bit code's float (pad bits 4-7: read from
    lr_texture::v).  Linear encoding: the decoded texel must be the host's float.  (wide changes nothing: a code's float lies in [0, 1].)"""
    rng = np.random.default_rng(24)
    codes = rng.integers(0, 256, (16, 16, 3)).astype(np.uint8)
    codes[..., 0] = np.arange(256).reshape(16, 16)
    codes[..., 1] = np.arange(256)[::-1].reshape(16, 16)
    quotient = codes.astype(np.float32) / np.float32(255.0)
    one_value = quotient.copy()
    one_value[..., 2] = np.float32(0.3)
    images = {"bytes_product.png": codes, "bytes_quotient.pfm": quotient, "bytes_constant.pfm": one_value}
    quads = []
    for f in images:
        for filter_mode, address, s, o in (("point", "repeat", (1.0, 1.0), (0.0, 0.0)), ("bilinear", "mirror", ADDRESS_SCALE, ADDRESS_OFFSET)):
            quads.append({"uvs": UNIT, "texture": {"kind": "image", "file": f, "encoding": "linear", "filter": filter_mode, "address": address,
                                                   "uv_scale": s, "uv_offset": o, "scale": 1.0}})
    centre = (np.arange(16) + 0.5) / 16.0
    cx, cy = (a.reshape(-1) for a in np.meshgrid(centre, centre))
    n_free, first = 300, len(quads)
    quad = np.concatenate([np.repeat(np.arange(first), 256), rng.integers(0, first, n_free)])
    x, y = np.concatenate([np.tile(cx, first), rng.integers(0, GRID, n_free) / GRID]), np.concatenate([np.tile(cy, first), rng.integers(0, GRID, n_free) / GRID])
    # ... and two quads around +-2^20, where texel_wrap changes paths: steps inside their texels (_inside), for the band is an eighth of a texel there
    for f, filter_mode, address, centre_x, centre_y in (("bytes_product.png", "point", "repeat", 2.0 ** 20, -2.0 ** 20),
                                                        ("bytes_constant.pfm", "bilinear", "mirror", -2.0 ** 20, 2.0 ** 20)):
        (ex, kx), (ey, ky) = _inside_window(16, centre_x), _inside_window(16, centre_y)
        quads.append({"uvs": UNIT, "texture": {"kind": "image", "file": f, "encoding": "linear", "filter": filter_mode, "address": address,
                                               "uv_scale": (GRID * 2.0 ** ex, GRID * 2.0 ** ey), "uv_offset": (kx * 2.0 ** ex, ky * 2.0 ** ey), "scale": 1.0}})
        quad = np.concatenate([quad, np.full(150, len(quads) - 1)])
        x = np.concatenate([x, rng.choice(_inside_steps(16, ex, kx), 150) / GRID])
        y = np.concatenate([y, rng.choice(_inside_steps(16, ey, ky), 150) / GRID])
    prim, u, v = records_for_unit_uv(x, y)
    return Family("bytes", quads, images, quad, prim, u, v)


# ---- checker
def _checker(wide: bool) -> Family:
    """Checkerboard over Constant children, over Image children, over one of each and without children; uv on both sides of 0 (the parity of negative
    cells), on cell borders (multiples of 1 / scale on the uv grid: judged with the band) and inside cells"""
    rng = np.random.default_rng(25)
    images = {"checker_13x7.pfm": _picture(rng, 13, 7, wide), "checker_16x16.pfm": _picture(rng, 16, 16, wide)}
    image = lambda f, filter_mode: {"kind": "image", "file": f, "filter": filter_mode, "address": "repeat", "uv_scale": ADDRESS_SCALE,  # noqa: E731
                                    "uv_offset": ADDRESS_OFFSET, "scale": 1.0}
    top = 2.5 if wide else 0.9
    on, off = {"kind": "constant", "v": (top, 0.3, 0.2)}, {"kind": "constant", "v": (0.2, 0.5, 0.75)}
    boards = [{"kind": "checker", "on": on, "off": off, "scale": 4.0},
              {"kind": "checker", "on": image("checker_13x7.pfm", "point"), "off": image("checker_16x16.pfm", "bilinear"), "scale": 3.0},
              {"kind": "checker", "on": on, "off": image("checker_13x7.pfm", "bilinear"), "scale": 2.5},
              {"kind": "checker", "on": None, "off": None, "scale": 5.0}]
    quads = [{"uvs": square(-2.0, 2.0), "texture": b} for b in boards]
    quad = rng.integers(0, len(quads), N)
    prim = rng.integers(0, 2, N)
    u, v = _random_barycentrics(rng, N)
    # a few records ON cell borders: barycentrics on the 1 / 64 grid, uv = -2 + 4 (.) a multiple of 1 / 16
    k = 30
    p, uu, vv = records_for_unit_uv(rng.integers(0, 65, k) / 64.0, rng.integers(0, 65, k) / 64.0)
    prim[:k], u[:k], v[:k] = p, uu, vv
    return Family("checker", quads, images, quad, prim, u, v)


# ---- inside, alpha
def _inside_window(n: int, centre: float):
    """(e, k0) of a window of the `exact` kind around the texel coordinate `centre`: U in eighths of n's odd part, so that X = n (k + k0) 2^e has a
    fraction, and 21 + 3 bits at 2^20"""
    e = -3 - (n & -n).bit_length() + 1
    return e, int(round(centre / (n * 2.0 ** e))) - GRID // 2


def _inside_steps(n: int, e: int, k0: int) -> np.ndarray:
    """the steps k of a window whose texel coordinate lies a quarter of a texel or more from the texel's border"""
    x = n * (np.arange(GRID) + k0) * 2.0 ** e
    fraction = x - np.floor(x)
    return np.nonzero((fraction >= 0.25) & (fraction <= 0.75))[0]


def _inside(name: str, images: dict, prefix: str, filters: tuple, seed: int) -> Family:
    """coordinates of the `exact` family's kind -- its sizes and address modes, fine windows around 0 and around +-2^20 on both axes, every float32
    operation exact (exact_precondition) -- for the channels that TRACE their rays.  A traced uv is no dyadic number, and a record on a texel border
    would be undecided: here only steps INSIDE a texel are taken, a quarter or more from its border (at 2^20 the band of a uv that is not exact is an
    eighth of a texel, 2 eps 2^20), so that a point lookup stays SURE on both paths of texel_wrap"""
    rng = np.random.default_rng(seed)

    def windows(n, wrapping):
        return [_inside_window(n, c) for c in ((0.0, 2.0 ** 20, -2.0 ** 20) if wrapping else (0.0, 2.0 ** 20))]

    def steps(n, address, e, k0):
        must, special = _special_steps(n, address, True, e, k0)
        allowed = _inside_steps(n, e, k0)
        return np.intersect1d(np.concatenate([must, special]), allowed), allowed

    quads, plans = [], []
    for w, h in SIZES:
        for address_name, address in ADDRESSES.items():
            wx, wy = windows(w, address in (REPEAT, MIRROR)), windows(h, address in (REPEAT, MIRROR))
            for filter_mode in filters:
                for j in range(len(wx)):
                    (ex, kx), (ey, ky) = wx[j], wy[(j + 1) % len(wy)]
                    quads.append({"uvs": UNIT, "texture": {
                        "kind": "image", "file": f"{prefix}_{w}x{h}.pfm", "filter": filter_mode, "address": address_name,
                        "uv_scale": (GRID * 2.0 ** ex, GRID * 2.0 ** ey), "uv_offset": (kx * 2.0 ** ex, ky * 2.0 ** ey), "scale": 1.0}})
                    plans.append((steps(w, address, ex, kx), steps(h, address, ey, ky)))
    per_quad = N // len(quads)
    quad, x, y = [], [], []
    for q, plan in enumerate(plans):
        count = per_quad + (1 if q < N - per_quad * len(quads) else 0)
        picked = [rng.permutation(np.concatenate([rng.choice(special, count // 2), rng.choice(allowed, count - count // 2)])) for special, allowed in plan]
        quad += [q] * count
        x.append(picked[0])
        y.append(picked[1])
    prim, u, v = records_for_unit_uv(np.concatenate(x) / GRID, np.concatenate(y) / GRID)
    return Family(name, quads, images, quad, prim, u, v)


def _inside_family(wide: bool) -> Family:
    """_inside over pictures of distinct texels, both filters: what carries the +-2^20 coordinates of `exact` into the megakernels' copies of the lookup"""
    rng = np.random.default_rng(27)
    return _inside("inside", {f"inside_{w}x{h}.pfm": _picture(rng, w, h, wide) for w, h in SIZES}, "inside", ("point", "bilinear"), 28)


def _alpha(wide: bool) -> Family:
    """_inside over point-filtered opacity images whose texels are exactly 0 or 1 (opacity reads x).  Geometry::_alpha_skip (dev_shade.h: alpha_skip)
    skips a candidate when float(xxhash32(inst, prim, bits(u), bits(v))) * 2^-32 > opacity: never for opacity 1 (the hash's float is at most 2^32),
    and always for opacity 0 unless the hash IS 0 -- one chance in 2^32 per record, a function of the record's bits and no more random than that.
    So a closest-hit query under the alpha test hits exactly where the texel is 1."""
    rng = np.random.default_rng(26)
    images = {}
    for w, h in SIZES:
        bits = rng.integers(0, 2, (h, w)).astype(np.float32)
        bits.reshape(-1)[:2] = (0.0, 1.0)[:w * h] if w * h > 1 else (1.0,)
        images[f"alpha_{w}x{h}.pfm"] = np.repeat(bits[..., None], 3, axis=2)
    return _inside("alpha", images, "alpha", ("point",), 29)


# ---- a film: the lean megakernels hold copies of the lookup that no query reaches; a render does
FILM_QUADS = 40  # at most: a longer family gives every k-th of its quads
DISNEY_BESIDE = "Shape beside : InlineMesh { positions { 0,-3,0, 1,-3,0, 0,-2,0 } indices { 0,1,2 } surface : Disney { color : Constant { v { 0.5 } } } }\n"


def film_scene(folder, source: str, disney: bool) -> Scene:
    """textured emitters in a row under an orthographic camera that looks straight down at them, 16 x 16 pixels per quad (every second 16 columns see
    one): the quads of the family `source` with their own vertex uvs, every k-th of them where there are more than FILM_QUADS.  The uv are the pixels':
    free over each quad's uv rectangle, whatever the family's records are.  disney: a Disney-surfaced triangle beside them, out of the camera's sight
    -- the scene then needs the Disney kernels"""
    family_ = family(source, True)
    family_.write_images(folder)
    step = -(-len(family_.quads) // FILM_QUADS)
    quads = family_.quads[::step]
    middle = len(quads) * QUAD_PITCH / 2
    camera = (f"Camera cam : Ortho {{ zoom {{ -1 }} spp {{ 1 }} film : Color {{ resolution {{ {32 * len(quads)}, 16 }} }} "
              f"position {{ {middle}, 0.5, 3 }} look_at {{ {middle}, 0.5, 0 }} }}")
    path = folder / f"film_{source}_{int(disney)}.luisa"
    path.write_text(scene_text(quads, "emission", extra_shapes=DISNEY_BESIDE if disney else "", camera=camera))
    return Scene.load(str(path))


FAMILIES = {"exact": _exact, "seams": _seams, "generic": _generic, "decode": _decode_family, "bytes": _bytes, "checker": _checker, "inside": _inside_family,
            "alpha": _alpha}


@functools.lru_cache(maxsize=None)
def family(name: str, wide: bool = False) -> Family:
    """the family `name`; wide: its pictures hold what an emission may (negative values, values above 1) instead of values inside [0, 1]"""
    return FAMILIES[name](wide)
