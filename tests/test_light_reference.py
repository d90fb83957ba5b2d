"""tests/light_reference.py held to closed forms on the CPU: the selection rule, the alias pick's frequencies against the triangles' areas,
the uniform triangle and sphere maps, the area light's pdf as a solid-angle density (its reciprocal integrates to the solid angle of the
emitter), the one-sided emitter's back, spawn_ray_to's 0.9999, and the properties of the inputs that tests/test_gpu_light.py relies on."""
import numpy as np

import light_reference as L
import surface_reference as R
from luisarender_amd import Scene
from luisarender_amd.render import check_light_args


def grid(n):
    """n x n stratified points of the unit square, cell centres"""
    a = (np.arange(n) + 0.5) / n
    x, y = np.meshgrid(a, a, indexing="ij")
    return x.ravel(), y.ravel()


def test_select():
    u = np.array([0.0, 0.24, 0.26, 0.49, 0.5, 0.99])
    is_env, tag, prob = L.select(0.0, 2, u)
    assert not is_env.any() and tag.tolist() == [0, 0, 0, 0, 1, 1] and (prob == 0.5).all()
    is_env, tag, prob = L.select(1.0, 0, u)
    assert is_env.all() and (prob == 1.0).all()
    is_env, tag, prob = L.select(0.25, 3, u)  # u < 0.25: the environment; the rest of [0, 1) is cut into three
    assert is_env.tolist() == [True, True, False, False, False, False] and tag[2:].tolist() == [0, 0, 1, 2]
    assert np.allclose(prob, [0.25, 0.25, 0.25, 0.25, 0.25, 0.25])  # (1 - 0.25) / 3
    assert L.select(0.25, 3, np.array([1.0]))[1].tolist() == [2]  # clamped


def test_uniform_triangle_and_sphere():
    x, y = grid(256)
    w = L.sample_uniform_triangle(x, y)
    assert (w >= 0.0).all() and np.allclose(w.sum(axis=1), 1.0) and np.allclose(w.mean(axis=0), 1.0 / 3.0, atol=1e-3)
    assert np.allclose((w * w).mean(axis=0), 1.0 / 6.0, atol=1e-3)  # E[b^2] of a uniform point's barycentric weight
    d = L.sample_uniform_sphere(x, y)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0) and np.allclose(d.mean(axis=0), 0.0, atol=1e-6)
    assert np.allclose((d * d).mean(axis=0), 1.0 / 3.0, atol=1e-4)


def test_alias_pick_follows_the_areas():
    """the fan's alias table picks each of its five unequal triangles as often as its share of the area, and remaps u uniformly"""
    t = L.light_tables(Scene.from_string(L.fan_scene()))
    fan = int(t["light_instances"][0, 0])
    first, count = (int(x) for x in t["meshes"][t["instances"][fan, 0] >> 10][2:4])
    assert count == 5
    prob, index = t["alias_prob"][first:first + count], t["alias_index"][first:first + count]
    n = 100000
    u = (np.arange(n) + 0.5) / n
    pick, ur = L.alias_pick(prob, index, u)
    area = R.shading_points(t, np.full(count, fan), np.arange(count), np.full(count, 0.3), np.full(count, 0.3))["area"]
    share = area / area.sum()
    assert share.max() / share.min() > 3.0  # unequal: no trivial table
    assert np.allclose(np.bincount(pick, minlength=count) / n, share, atol=2.0 * count / n + 1e-6)
    assert np.allclose(t["tri_pdf"][first:first + count], share, atol=1e-6)
    assert (ur >= 0.0).all() and (ur < 1.0).all() and abs(ur.mean() - 0.5) < 1e-2
    assert (L.alias_boundary_distance(prob, np.array([0.0, 0.2, (1 + prob[1]) / 5]))[[0, 1, 2]] < 1e-12).all()


def test_area_pdf_integrates_to_the_solid_angle():
    """1 / pdf of the samples of ONE emitter averages to the solid angle it subtends: for a rectangle a x b seen from h above its centre,
    4 atan(a b / (2 h sqrt(4 h^2 + a^2 + b^2))).  Two lights: the selection probability 1 / 2 is divided out."""
    t = L.light_tables(Scene.from_string(L.TWO_PANELS))
    assert t["env_prob"] == 0.0 and t["light_count"] == 2 and len(t["light_instances"]) == 2
    x, y = grid(128)
    centre = L.PANEL_A["corner"] + 0.5 * (L.PANEL_A["e1"] + L.PANEL_A["e2"])
    h = 1.25
    p = np.tile((centre - [0.0, h, 0.0]).astype(np.float32), (len(x), 1))
    ng, ns = L.floor_frame(len(x))
    tags = [k for k in range(2) if np.array_equal(t["light_L"][t["instances"][t["light_instances"][k, 0], 1] & 4095], L.PANEL_A["L"])]
    assert len(tags) == 1
    u = np.stack([np.full(len(x), (tags[0] + 0.5) / 2.0), x, y], axis=1).astype(np.float32)
    s = L.sample(t, p, ng, ns, np.zeros(len(x), np.int64), u)
    assert (s["kind"] == L.KIND_AREA).all() and (s["pdf"] > 0).all() and (s["L"] == L.PANEL_A["L"]).all()
    a, b = 1.5, 1.0
    omega = 4.0 * np.arctan(a * b / (2.0 * h * np.sqrt(4.0 * h * h + a * a + b * b)))
    assert abs((0.5 / s["pdf"]).mean() - omega) < 2e-3 * omega
    # the pdf itself, from the sampled point: dist^2 / (|cos| A) / 2
    d2 = ((s["point"] - p) ** 2).sum(axis=1)
    cos = np.abs((s["point"] - p)[:, 1]) / np.sqrt(d2)
    assert np.allclose(s["pdf"], d2 / (cos * a * b) / 2.0, rtol=1e-6)
    # the shadow ray: from just above the floor point towards the sampled point, 0.9999 of the way
    assert np.allclose(np.linalg.norm(s["d"], axis=1), 1.0) and (np.abs(s["o"] - p).max(axis=1) < 1e-3).all() and (s["o"][:, 1] > p[:, 1]).all()
    reach = s["o"] + s["d"] * (s["t_max"] / L.SHADOW_SCALE)[:, None]
    assert np.abs(reach - s["point"]).max() < 1e-9
    plane, inside = L.panel_of(s["point"], L.PANEL_A, 1e-6)
    assert plane.max() < 1e-6 and inside.all()


def test_one_sided_emitter_from_behind():
    t = L.light_tables(Scene.from_string(L.TWO_PANELS))
    tags = [k for k in range(2) if np.array_equal(t["light_L"][t["instances"][t["light_instances"][k, 0], 1] & 4095], L.PANEL_B["L"])]
    assert len(tags) == 1 and not t["light_two_sided"][t["instances"][t["light_instances"][tags[0], 0], 1] & 4095]
    x, y = grid(16)
    n = len(x)
    u = np.stack([np.full(n, (tags[0] + 0.5) / 2.0), x, y], axis=1).astype(np.float32)
    ng, ns = L.floor_frame(n)
    for px, lit in ((-2.0, False), (0.5, True)):  # behind the panel's plane x = -1 (its normal is +x), and in front of it
        p = np.tile(np.float32([px, 0.0, 0.2]), (n, 1))
        s = L.sample(t, p, ng, ns, np.zeros(n, np.int64), u)
        assert ((s["pdf"] > 0) == lit).all() and ((s["L"] == L.PANEL_B["L"]).all(axis=1) == lit).all() and ((s["L"] == 0).all(axis=1) != lit).all()
        plane, inside = L.panel_of(s["point"], L.PANEL_B, 1e-6)
        assert plane.max() < 1e-6 and inside.all()


def test_constant_environment_and_bare_points():
    t = L.light_tables(Scene.from_string(L.fan_scene()))
    assert 0.0 < t["env_prob"] < 1.0 and t["light_count"] == 2
    assert np.allclose(t["env_L"], np.float32([0.3, 0.5, 0.8]) * 1.5) and np.allclose(t["env_to_world"] @ t["env_to_world"].T, np.eye(3), atol=1e-6)
    x, y = grid(64)
    n = len(x)
    u = np.stack([np.full(n, 0.5 * t["env_prob"]), x, y], axis=1).astype(np.float32)
    p = np.tile(np.float32([0.3, 0.0, -0.4]), (n, 1))
    s = L.sample(t, p, None, None, None, u)  # bare points: the origin is p itself
    assert (s["kind"] == L.KIND_ENVIRONMENT).all() and np.array_equal(s["o"], p.astype(np.float64)) and (s["t_max"] == L.FLT_MAX).all()
    assert np.allclose(s["pdf"], t["env_prob"] / (4.0 * np.pi)) and np.allclose(s["L"], t["env_L"])
    assert np.allclose(np.linalg.norm(s["d"], axis=1), 1.0) and np.allclose(s["d"].mean(axis=0), 0.0, atol=1e-6)
    ng, ns = L.floor_frame(n)
    on_floor = L.sample(t, p, ng, ns, np.zeros(n, np.int64), u)  # on the floor: moved off it to the side the direction leaves on
    assert np.array_equal(np.sign(on_floor["o"][:, 1]), np.sign(s["d"][:, 1])) and np.abs(on_floor["o"] - p).max() < 1e-3


def test_inputs_stand_clear_of_every_boundary():
    """what tests/test_gpu_light.py relies on: the shared inputs stand at least BOUNDARY from every decision the sampler takes on u, so the
    reference alone gives no flip; under 1 % of the records see their emitter at a grazing angle; check_light_args takes them"""
    inp = L.inputs()
    assert check_light_args(None, inp["u"], inp["p"]) == "numpy" and len(inp["u"]) == L.COUNT == 1027
    u = inp["u"].astype(np.float64)
    for text in (L.TWO_PANELS, L.fan_scene()):
        t = L.light_tables(Scene.from_string(text))
        n, pe = t["light_count"], t["env_prob"]
        cuts = np.concatenate([[pe], pe + (1.0 - pe) * np.arange(1, n) / n])
        assert np.abs(u[:, 0:1] - cuts[None, :]).min() >= L.BOUNDARY
        is_env, tag, _ = L.select(pe, n, u[:, 0])
        for k in range(n):
            inst = int(t["light_instances"][k, 0])
            first, count = (int(x) for x in t["meshes"][t["instances"][inst, 0] >> 10][2:4])
            m = ~is_env & (tag == k)
            assert m.sum() > 100 and L.alias_boundary_distance(t["alias_prob"][first:first + count], u[m, 1]).min() >= L.BOUNDARY
        ng, ns = L.floor_frame(L.COUNT)
        s = L.sample(t, inp["p"], ng, ns, np.zeros(L.COUNT, np.int64), inp["u"])
        area = s["kind"] == L.KIND_AREA
        to_light = s["point"] - inp["p"]
        lp = R.shading_points(t, s["inst"][area], s["prim"][area], np.full(area.sum(), 0.3), np.full(area.sum(), 0.3))
        cos = np.abs(np.einsum("nk,nk->n", L._unit(to_light[area]), lp["ng"]))
        assert (cos < L.GRAZING).sum() < 0.01 * L.COUNT
        assert (s["pdf"][area] > 0).mean() > 0.5
    assert abs(np.diff(u[:, 1] - u[:, 2]).min()) > 0  # (not a constant column)
