"""tests/texture_reference.py without a GPU: the float64 reference against closed forms and against the oracle (whose wrap is pinned bit for bit to the
reference project's sampler, test_oracle_vs_ref.py), the judge against a float32 restatement of the device's lookup -- accepted on every family
within the caps -- and against that restatement with each of ten mistakes, every one of which a named family rejects."""
import numpy as np
import pytest

import texture_reference as T
from luisarender_amd import Scene
from oracle.check import Oracle

EXACT = ("exact", "inside", "alpha")  # the families whose float32 arithmetic up to the texel coordinate is exact: no band
ROLE = {"alpha": "alpha"}  # the role a family's scene is built in here; every other family: albedo


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """(family, tables, texture id of every record, uv of every record, candidates) per (family name, wide), built once"""
    cache = {}

    def get(name, wide=False):
        if (name, wide) not in cache:
            family = T.family(name, wide)
            role = "emission" if wide else ROLE.get(name, "albedo")
            tables = T.Tables(family.scene(tmp_path_factory.mktemp(f"{name}_{int(wide)}"), role))
            tex, uv = tables.texture_of(family.quad, role), family.uv()
            if name in EXACT:
                T.exact_precondition(family, tables, tex)
            cache[(name, wide)] = (family, tables, tex, uv, T.candidates(tables, tex, uv, None if name in EXACT else 0.0))
        return cache[(name, wide)]
    return get


# ---------------------------------------------------------------- 1. closed forms
TWO = np.float32([[1, 2], [3, 4]])[..., None] * np.float32([1, 10, 100])          # texel (x, y) = row y, column x
SEVEN = (np.arange(7, dtype=np.float32) + 1).reshape(7, 1, 1) * np.float32([1, 10, 100])  # 1 wide, 7 high: row y holds y + 1


def _lookup(pixels, uv, **fields):
    tables = T.Tables.of_images([{"pixels": pixels, **fields}])
    c = T.candidates(tables, [0], np.float32([uv]))
    assert not c["maybe"][0]
    return c["ref"][0, 0]


@pytest.mark.parametrize("address, point_2x2, corner_2x2, point_1x7, negative_1x7, bilinear_1x7",
                         [(T.REPEAT, 3, 2.5, 2, 5, 2.5), (T.MIRROR, 2, 1, 6, 3, 5.5), (T.EDGE, 2, 1, 7, 1, 7), (T.ZERO, 0, 0.25, 0, 0, 0)])
def test_hand_computed_lookups(address, point_2x2, corner_2x2, point_1x7, negative_1x7, bilinear_1x7):
    """2 x 2: the point lookup at texel coordinates (2.5, -0.5) = texel (2, -1) wraps to (0, 1) / mirrors to (1, 0) / clamps to (1, 0) / is zero;
    the bilinear lookup at uv (0, 0) mixes texels (-1 .. 0)^2 in equal parts: all four under REPEAT, four times (0, 0) under MIRROR and EDGE, one
    quarter of (0, 0) under ZERO.  1 x 7: row 8 is row 1 / 13 - 8 = 5 / 6 / none; row -3 is row 4 / 2 / 0 / none; rows 8 and 9 in equal parts"""
    rgb = np.float64([1, 10, 100])
    assert np.array_equal(_lookup(TWO, (0.25, 0.75), address=address)[:3], 3 * rgb)  # inside: texel (0, 1)
    assert np.array_equal(_lookup(TWO, (1.25, -0.25), address=address)[:3], point_2x2 * rgb)
    assert np.array_equal(_lookup(TWO, (0.5, 0.5), address=address, filter=T.BILINEAR)[:3], 2.5 * rgb)
    assert np.array_equal(_lookup(TWO, (0.0, 0.0), address=address, filter=T.BILINEAR)[:3], corner_2x2 * rgb)
    assert np.array_equal(_lookup(SEVEN, (0.3, 8.5 / 7), address=address)[:3], point_1x7 * rgb)
    assert np.array_equal(_lookup(SEVEN, (-5.3, -2.5 / 7), address=address)[:3], negative_1x7 * rgb)
    assert np.allclose(_lookup(SEVEN, (0.3, 9.0 / 7), address=address, filter=T.BILINEAR)[:3], bilinear_1x7 * rgb, rtol=1e-6, atol=0)
    # the uv transform and the scale: u * s + o = 1.25, -0.25 again
    assert np.array_equal(_lookup(TWO, (0.5, 0.25), address=address, uv_scale=(2, -3), uv_offset=(0.25, 0.5), scale=0.5)[:3], 0.5 * point_2x2 * rgb)


def test_hand_computed_decodes():
    knee = np.float32(0.04045)
    above = np.nextafter(knee, np.float32(1))
    px = np.float32([[[0.0, 1.0, knee], [above, 0.5, 0.0031308]]])
    tables = T.Tables.of_images([{"pixels": px, "encoding": T.SRGB}] +
                                [{"pixels": np.float32([[[0.0, -0.5, 0.5]]]), "encoding": T.GAMMA, "gamma": g} for g in (2.0, 3.0, 2.2)])
    srgb = T.candidates(tables, [0, 0], np.float32([[0.25, 0.5], [0.75, 0.5]]))["ref"][:, 0, :3]
    want = lambda c: ((float(c) + float(np.float32(0.055))) * float(np.float32(1 / 1.055))) ** 2.4  # noqa: E731
    assert srgb[0, 0] == 0.0 and abs(srgb[0, 1] - 1.0) < 1e-7
    assert srgb[0, 2] == float(knee) * float(np.float32(1 / 12.92))          # AT the knee: the linear piece
    assert srgb[1, 0] == want(above) and abs(srgb[1, 0] - srgb[0, 2]) < 1e-6  # next above it: the power, which continues the line
    assert srgb[1, 1] == want(0.5) and abs(srgb[1, 1] - 0.21404) < 1e-4
    assert srgb[1, 2] == float(np.float32(0.0031308)) * float(np.float32(1 / 12.92))  # (the knee of the ENCODED value is 0.04045, not 0.0031308)
    gamma = {g: T.candidates(tables, [i], np.float32([[0.5, 0.5]]))["ref"][0, 0, :3] for i, g in ((1, 2.0), (2, 3.0), (3, 2.2))}
    assert np.array_equal(gamma[2.0], [0.0, 0.25, 0.25]) and np.array_equal(gamma[3.0], [0.0, -0.125, 0.125])
    assert gamma[2.2][0] == 0.0 and np.isnan(gamma[2.2][1]) and gamma[2.2][2] == 0.5 ** float(np.float32(2.2))
    # the consumers: albedo saturates (a NaN becomes 0, as fmaxf makes it), emission clamps below only and takes the light's scale
    c = T.candidates(tables, [2, 3], np.float32([[0.5, 0.5]] * 2))
    assert np.array_equal(T.consume(c, "albedo", channels=[3, 3])["ref"][:, 0], [[0.0, 0.0, 0.125], [0.0, 0.0, gamma[2.2][2]]])
    assert np.array_equal(T.consume(c, "emission", light_scale=[4.0, 4.0])["ref"][0, 0], [0.0, 0.0, 0.5])
    one = T.candidates(T.Tables.of_images([{"pixels": np.float32([[[0.5, 0.25, 2.0]]])}]), [0], np.float32([[0.5, 0.5]]))
    assert np.array_equal(T.consume(one, "albedo", channels=[1])["ref"][0, 0], [0.5, 0.5, 0.5])
    assert np.array_equal(T.consume(one, "albedo", channels=[2])["ref"][0, 0], [0.5, 0.25, 1.0])
    assert np.array_equal(T.consume(one, "albedo", channels=[3])["ref"][0, 0], [0.5, 0.25, 1.0])  # saturated
    assert np.allclose(T.consume(one, "roughness", channels=[3], remap=True)["ref"][0, 0], [0.5, 0.25], rtol=1e-12)   # sqrt(max(r^2, 1e-4))
    assert np.allclose(T.consume(one, "roughness", channels=[1], remap=False)["ref"][0, 0], [0.5 ** 0.5, 0.5 ** 0.5], rtol=1e-12)


def test_wrap_is_the_double_modulo():
    """wrap() on Python integers against ((v % n) + n) % n in C's truncating arithmetic (the oracle's and the reference sampler's form)"""
    c_mod = lambda a, b: int(np.fmod(a, b))  # noqa: E731  (truncates towards zero, as C's %)
    for n in (1, 2, 3, 5, 7, 13, 16):
        for v in list(range(-3 * n - 1, 3 * n + 2)) + [2 ** 20, -2 ** 20, 2 ** 30 - 1, -2 ** 30]:
            assert T.wrap(T.REPEAT, v, n) == c_mod(c_mod(v, n) + n, n)
            m = c_mod(c_mod(v, 2 * n) + 2 * n, 2 * n)
            assert T.wrap(T.MIRROR, v, n) == (m if m < n else 2 * n - 1 - m)
            assert T.wrap(T.EDGE, v, n) == min(max(v, 0), n - 1) and T.wrap(T.ZERO, v, n) == (v if 0 <= v < n else None)


# ---------------------------------------------------------------- 2. the reference against the oracle
ORACLE_SCENE = """
Shape quad : InlineMesh {{ positions {{ 0,0,0, 1,0,0, 1,1,0, 0,1,0 }} uvs {{ 0,0, 1,0, 1,1, 0,1 }} indices {{ 0,1,2, 0,2,3 }}
  light : Diffuse {{ emission : {texture} scale {{ 1.5 }} }} }}
Camera cam : Pinhole {{ fov {{ 24 }} spp {{ 1 }} film : Color {{ resolution {{ 24, 24 }} }} position {{ 0.5, 0.5, 2.5 }} look_at {{ 0.5, 0.5, 0 }} }}
render {{ cameras {{ @cam }} shapes {{ @quad }} integrator : MegaPath {{ depth {{ 1 }} }} }}
"""
# what the oracle's decode may differ from float64 by, relative: x = (c + 0.055) * (1 / 1.055) rounds twice and the power 2.4 (3 under gamma: one rounding
# less in front) multiplies that, 5 eps; libm's powf is good to 1 ulp = 2 eps; 8 eps with the scale's rounding
ORACLE_DECODE = 8 * T.EPS


@pytest.mark.parametrize("encoding, gamma", [("linear", None), ("sRGB", None), ("gamma", 2.2)])
@pytest.mark.parametrize("filter_mode", ["point", "bilinear"])
@pytest.mark.parametrize("address", ["repeat", "mirror", "edge", "zero"])
def test_reference_against_the_oracle(tmp_path, address, filter_mode, encoding, gamma):
    """an emissive quad whose uv are its x and y, seen at depth 1: oracle_li of a pixel is the emission at oracle_camera_ray's hit, which the judge
    must accept at that hit's uv -- ADDRESS_SCENE's transform, a 13 x 7 picture with values an emission may hold"""
    rng = np.random.default_rng(7)
    T.write_pfm(str(tmp_path / "picture.pfm"), rng.uniform(-0.25 if encoding == "linear" else 0.0, 2.0, (7, 13, 3)).astype(np.float32))
    spec = {"kind": "image", "file": "picture.pfm", "encoding": encoding, "gamma": gamma, "filter": filter_mode, "address": address,
            "uv_scale": T.ADDRESS_SCALE, "uv_offset": T.ADDRESS_OFFSET, "scale": 0.75}
    (tmp_path / "scene.luisa").write_text(ORACLE_SCENE.format(texture=T.texture_sdl(spec)))
    scene = Scene.load(str(tmp_path / "scene.luisa"))
    tables = T.Tables(scene)
    oracle = Oracle(scene)
    prim, u, v, li = [], [], [], []
    for py in range(oracle.height):
        for px in range(oracle.width):
            ray = oracle.camera_ray(px, py, 0)
            inst, p, bu, bv, _ = oracle.trace_closest(ray[0:3], ray[3:6])
            if inst == 0:
                assert ray[6] == 1.0
                prim.append(p), u.append(bu), v.append(bv), li.append(oracle.li(px, py, 0))
    oracle.close()
    assert len(li) > 300
    uv = T.interpolate_uv(np.tile(np.float32(T.UNIT), (len(li), 1, 1)), np.array(prim), u, v)
    tex = tables.texture_of(np.zeros(len(li), np.int64), "emission")
    c = T.consume(T.candidates(tables, tex, uv, uv_ulps=2.0, decode_relative=ORACLE_DECODE), "emission", light_scale=np.full(len(li), 1.5))
    got = T.verdicts(c, np.array(li))
    assert got["ok"].all(), (np.nonzero(~got["ok"])[0][:5], got["excess"].max())
    assert c["maybe"].mean() <= T.MAYBE_CAP and np.unique(np.array(li), axis=0).shape[0] > 20


# ---------------------------------------------------------------- 3. the judge accepts the restatement, within the caps
@pytest.mark.parametrize("name", list(T.FAMILIES))
def test_caps_and_a_correct_restatement(built, name):
    """the share of MAYBE records is a function of inputs and reference alone: at most MAYBE_CAP, none in `exact` (and `alpha`, which takes its
    coordinates); the float32 restatement of the device's lookup -- contracted or not, float or 8-bit texels -- is accepted on every record, through
    every consumer; were a band too tight it would show here, and the derivation would be what is wrong"""
    for wide in (False, True):
        if name == "alpha" and wide:
            continue
        family, tables, tex, uv, c = built(name, wide)
        assert c["maybe"].mean() <= (0.0 if name in EXACT else T.MAYBE_CAP), c["maybe"].mean()
        assert len(family) <= T.N and len(family) > 256 and len(family) % 64 != 0
        assert name == "decode" or np.isfinite(c["bar"]).all()  # no band of a family's own records spans more than two texels
        channels = np.array([tables.textures[int(i)]["channels"] for i in tex])
        for contract in (False, True):
            for storage in (0, 2) if name == "bytes" else (0,):
                raw = T.device_lookup(tables, tex, uv, storage=storage, contract=contract)
                rules = [("raw", {}), ("emission", {"light_scale": np.full(len(tex), T.LIGHT_SCALE)}), ("albedo", {"channels": channels}),
                         ("roughness", {"channels": channels, "remap": True}), ("roughness", {"channels": channels, "remap": False})]
                for role, args in rules:
                    if name == "decode" and (T.MEASURED_SRGB is None or T.MEASURED_GAMMA is None):
                        continue  # (no bar yet: test_the_decode_bars_are_measured fails)
                    got = T.verdicts(T.consume(c, role, **args), T.consume32(raw, role, **args))
                    assert got["ok"].all(), (name, wide, contract, storage, role, np.nonzero(~got["ok"])[0][:5], got["excess"].max())


def test_the_decode_bars_are_measured():
    assert T.MEASURED_SRGB is not None and T.MEASURED_GAMMA is not None, "texture_reference.MEASURED_*: run tests/test_gpu_texture.py on the device and record what it prints"
    assert 0.0 < T.MEASURED_SRGB < 64 * T.EPS and 0.0 < T.MEASURED_GAMMA < 64 * T.EPS  # a few ulp: more would be a bug to find, not a bar to set


def test_the_families_hold_what_they_claim(built):
    family, tables, tex, uv, c = built("exact")
    x = T.exact_precondition(family, tables, tex)
    t = np.floor(x).astype(np.int64)
    assert (c["delta"] == 0).all() and x.min() < -2.0 ** 29 and x.max() > 2.0 ** 29 and (np.abs(x) < 2.0 ** 30 + 1).all()
    for special in (2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1):
        assert (t == special).any() and (t == -special).any(), special
    assert (np.abs(t) > 2 ** 24).sum() > 100
    seen = {(tables.textures[int(i)]["width"], tables.textures[int(i)]["height"], tables.textures[int(i)]["address"], tables.textures[int(i)]["filter"]) for i in tex}
    assert seen == {(w, h, a, f) for w, h in T.SIZES for a in range(4) for f in range(2)}
    wrapped = {}  # (period, filter) -> the integer coordinates that go through the wrap (bilinear: both columns / rows of the footprint)
    for i in np.unique(tex):
        tt = tables.textures[int(i)]
        if tt["address"] in (T.REPEAT, T.MIRROR):
            for axis, n in ((0, tt["width"]), (1, tt["height"])):
                ix = np.floor(x[tex == i, axis] - (0.5 if tt["filter"] == T.BILINEAR else 0.0)).astype(np.int64)
                both = ix if tt["filter"] == T.POINT else np.concatenate([ix, ix + 1])
                wrapped.setdefault((n * (2 if tt["address"] == T.MIRROR else 1), tt["filter"]), []).append(both)
    bilinear = np.array([tables.textures[int(i)]["filter"] == T.BILINEAR for i in tex])
    weights = (x[bilinear] - 0.5) - np.floor(x[bilinear] - 0.5)
    assert all((weights == q).sum() > 50 for q in (0.0, 0.25, 0.5, 0.75))
    assert {p for p, _ in wrapped} =={1, 2, 3, 5, 7, 13, 16, 4, 6, 10, 14, 26, 32}
    for (p, f), coordinates in wrapped.items():  # every period in use: multiples of it and of twice it, one below, one above
        v = np.concatenate(coordinates)
        for q in (p, 2 * p):
            assert {0, 1 % q, q - 1} <= set((v % q).tolist()), (p, f, q)
            assert ((v % q == 0) & (v < 0)).any() and ((v % q == 0) & (v > 0)).any(), (p, f, q)
    # seams: footprints over the border in x, in y, at corners; under ZERO two and three of the four texels are zero; u, v exactly 0.0, -0.0, 1.0
    family, tables, tex, uv, c = built("seams")
    assert (uv == 0.0).any() and (uv == 1.0).any() and (np.signbit(uv) & (uv == 0.0)).any()
    zeros = []
    for i in np.unique(tex):
        tt = tables.textures[int(i)]
        if tt["address"] == T.ZERO:
            _, _, f, _ = T._coordinates(tt, uv[tex == i], 0.0)
            ix = np.floor(f).astype(np.int64)
            out_x = [(ix[:, 0] + k < 0) | (ix[:, 0] + k >= tt["width"]) for k in (0, 1)]
            out_y = [(ix[:, 1] + k < 0) | (ix[:, 1] + k >= tt["height"]) for k in (0, 1)]
            zeros.append(sum((ox | oy).astype(int) for ox in out_x for oy in out_y))
    assert {0, 2, 3, 4} <= set(np.concatenate(zeros).tolist())
    # bytes: every code; decode: both sides of the knee
    family, tables, tex, uv, c = built("bytes")
    for name, pixels in family.images.items():
        codes = np.round(np.asarray(pixels, np.float64) * (1 if pixels.dtype == np.uint8 else 255)).astype(int)
        assert set(codes[..., 0].reshape(-1).tolist()) == set(range(256)), name
    forms = sorted((T.pack_bytes(tables.image(tables.textures[int(i)]))[1:3]) for i in np.unique(tex))
    assert forms == [(1, 0)] * 3 + [(2, 0)] * 2 + [(2, 4)] * 3  # (form, constant channels): the PNG, the quotient PFM, the one with one blue
    # inside and alpha: inside the texels, on both sides of +-2^20, every size and address mode; alpha: texels of both values
    for name in ("inside", "alpha"):
        family, tables, tex, uv, c = built(name)
        x = T.exact_precondition(family, tables, tex)
        fraction = x - np.floor(x)
        assert (fraction >= 0.25).all() and (fraction <= 0.75).all() and (np.abs(x) < 2.0 ** 19).any()
        for sign in (1, -1):
            near = np.abs(sign * x - 2.0 ** 20) < 2.0 ** 16
            assert (near & (sign * x > 2.0 ** 20)).sum() > 100 and (near & (sign * x < 2.0 ** 20)).sum() > 100  # either path of texel_wrap
        assert {(tables.textures[int(i)]["width"], tables.textures[int(i)]["height"], tables.textures[int(i)]["address"]) for i in tex} == \
            {(w, h, a) for w, h in T.SIZES for a in range(4)}
    assert {built("inside")[1].textures[int(i)]["filter"] for i in built("inside")[2]} == {T.POINT, T.BILINEAR}
    family, tables, tex, uv, c = built("bytes")  # two of its quads lie around +-2^20
    assert sum(1 for i in np.unique(tex) if abs(float(tables.textures[int(i)]["uv_offset"][0])) > 60000) == 2
    family, tables, tex, uv, c = built("alpha")
    assert set(np.unique(c["ref"][:, 0, 0]).tolist()) == {0.0, 1.0} and 0.2 < c["ref"][:, 0, 0].mean() < 0.8
    assert {(tables.textures[int(i)]["width"], tables.textures[int(i)]["height"], tables.textures[int(i)]["address"]) for i in tex} == \
        {(w, h, a) for w, h in T.SIZES for a in range(4)}
    family, tables, tex, uv, c = built("checker")
    assert (uv < 0).any() and (uv > 0).any() and 0 < c["maybe"].sum() <= T.MAYBE_CAP * len(family)


# ---------------------------------------------------------------- 4. the judge rejects mistakes
@pytest.mark.parametrize("mistake, name, storage",
                         [("no corrective step", "exact", 0), ("no 2^20 switch", "exact", 0), ("mirror period - m", "exact", 0), ("mirror period - m", "seams", 0),
                          ("no half texel", "seams", 0), ("tx and ty swapped", "seams", 0), ("tx and ty swapped", "generic", 0), ("a zero flag ignored", "seams", 0),
                          ("byte form 2 as form 1", "bytes", 2), ("constant channel from the word", "bytes", 2), ("sRGB knee at 0.0031308", "decode", 0),
                          ("no corrective step", "generic", 0), ("first step by n under MIRROR", "exact", 0), ("first step by n under MIRROR", "inside", 0), ("first step by n under MIRROR", "bytes", 2)])
def test_mistakes_are_rejected(built, mistake, name, storage):
    """the restatement with ONE mistake fails on the named family -- so would the device with it"""
    assert mistake in T.MISTAKES
    if name == "decode":
        assert T.MEASURED_SRGB is not None, "no bar yet (test_the_decode_bars_are_measured)"
    family, tables, tex, uv, c = built(name)
    rejected = {}
    for contract in (False, True):
        raw = T.device_lookup(tables, tex, uv, storage=storage, contract=contract, mistake=mistake)
        got = T.verdicts(T.consume(c, "raw"), raw)
        rejected[contract] = int((~got["ok"]).sum())
    assert min(rejected.values()) > 0, rejected


def test_every_mistake_is_tried():
    cases = [mark for mark in test_mistakes_are_rejected.pytestmark if mark.name == "parametrize"][0].args[1]
    assert {case[0] for case in cases} == set(T.MISTAKES)
