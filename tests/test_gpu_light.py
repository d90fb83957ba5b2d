"""Light queries on the device (include/lrhip.h: lrhip_query_light): closed forms on two quad emitters, the numpy restatement of
the reference's light sampler (tests/light_reference.py) on a mesh emitter under a constant environment, sample against evaluate under every
kind of environment, MegaPath's Li composed from the five queries against the oracle, bare points, batch semantics and malformed records, a
moved emitter, pointers, errors."""
import ctypes as C

import numpy as np
import pytest

import bsdf_reference as B
import instance_scene as S
import light_reference as L
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import MegaPathRenderer, RayHits
from luisarender_amd.scenes import cornell_box
from oracle.check import Oracle

pytestmark = pytest.mark.gpu

LRHIP_ERROR_INVALID = -1
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def words(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


def bar(measured, what):
    """MARGIN x the value measured on the MI355X (light_reference.py: MEASURED_*), never above bsdf_reference.LARGEST_SOUND_ERROR"""
    assert measured is not None, f"{what}: not measured yet (light_reference.py: MEASURED_*)"
    return min(L.MARGIN * measured, B.LARGEST_SOUND_ERROR)


def floor_setup(renderer, text):
    """uploads the scene, traces L.inputs()' rays onto its floor -> (tables, hits, the floor's SurfacePoints)"""
    scene = Scene.from_string(text)
    renderer.upload(scene)
    hits = renderer.trace(L.inputs()["rays"])
    sp = renderer.surface(hits)
    assert np.asarray(hits.hit).all() and np.asarray(sp.has_surface).all() and not np.asarray(sp.has_light).any()
    assert (sp.ng == np.float32([0, 1, 0])).all() and np.abs(sp.p - L.inputs()["p"]).max() < 1e-6
    return L.light_tables(scene), hits, sp


def sampled_points(s) -> np.ndarray:
    """o + d t_max / 0.9999 in float64: where an area sample's shadow ray was aimed"""
    r = s.rays.astype(np.float64)
    return r[:, 0:3] + r[:, 4:7] * (r[:, 7] / L.SHADOW_SCALE)[:, None]


def emitter_of_tag(t, tag):
    """instance and light record of light_instances[tag]"""
    inst = t["light_instances"][tag, 0]
    return inst, (t["instances"][inst, 1] & 4095).astype(np.int64)


# ---------------------------------------------------------------- 1. closed forms

def test_closed_forms(renderer, capsys):
    """two quad emitters over a floor, no environment: unit directions, the sampled point in the plane and inside the rectangle of the emitter
    floor(u_sel * 2) names, that emitter's L bit for bit, pdf against dist^2 / (|cos| A) / 2 in float64 from the returned point, and exact
    zeros behind the one-sided emitter.

    MEASURED on the MI355X: see light_reference.py (MEASURED_CLOSED_FORM_*)."""
    inp = L.inputs()
    t, hits, sp = floor_setup(renderer, L.TWO_PANELS)
    s = renderer.light_sample(hits, inp["u"])
    assert np.asarray(s.valid).all() and (s.kind == L.KIND_AREA).all() and (words(s.buffer)[:, 5:8] == 0).all()
    assert np.isfinite(s.rays).all() and np.isfinite(s.buffer[:, 0:4]).all() and (s.rays[:, 3] == 0).all()
    assert np.abs(np.linalg.norm(s.rays[:, 4:7].astype(np.float64), axis=1) - 1.0).max() < 1e-5
    tag = np.clip(np.floor(inp["u"][:, 0].astype(np.float64) * 2.0), 0, 1).astype(np.int64)
    _, light = emitter_of_tag(t, tag)
    is_a = (t["light_L"][light] == L.PANEL_A["L"]).all(axis=1)
    assert 300 < is_a.sum() < L.COUNT - 300 and (t["light_L"][light][~is_a] == L.PANEL_B["L"]).all()
    point, p = sampled_points(s), sp.p.astype(np.float64)
    plane_err = 0.0
    pdf_err = 0.0
    for panel, mine, area in ((L.PANEL_A, is_a, 1.5), (L.PANEL_B, ~is_a, 1.0)):
        plane, inside = L.panel_of(point[mine], panel, 1e-4)
        assert inside.all(), panel
        plane_err = max(plane_err, float(plane.max()))
        normal = L._unit(np.cross(panel["e1"], panel["e2"]))
        to_p = p[mine] - point[mine]
        d2 = (to_p ** 2).sum(axis=1)
        cos = np.abs(to_p @ normal) / np.sqrt(d2)
        want = d2 / (cos * area) / 2.0
        lit = np.ones(mine.sum(), bool)
        if panel is L.PANEL_B:  # one-sided, its front towards +x: nothing reaches the floor behind its plane x = -1
            behind, lit = p[mine][:, 0] < -1.0 - 1e-3, p[mine][:, 0] > -1.0 + 1e-3
            assert behind.sum() > 50 and (s.pdf[mine][behind] == 0).all() and (s.L[mine][behind] == 0).all()
        keep = lit & (cos >= L.GRAZING)
        assert (~keep & lit).sum() < 0.01 * L.COUNT and keep.sum() > 100
        assert (s.pdf[mine][keep] > 0).all() and (words(s.L[mine][keep]) == words(panel["L"])).all()
        pdf_err = max(pdf_err, float(L.relative_error(s.pdf[mine][keep], want[keep]).max()))
    with capsys.disabled():
        print(f"\n[light] closed forms: pdf {pdf_err:.3e}, sampled point off its emitter's plane {plane_err:.3e}", end="")
    assert pdf_err <= B.LARGEST_SOUND_ERROR
    assert pdf_err <= bar(L.MEASURED_CLOSED_FORM_PDF, "pdf") and plane_err <= L.PLANE_BAR


# ---------------------------------------------------------------- 2. against the numpy reference

def test_against_the_numpy_reference(renderer, capsys):
    """a five-triangle fan of unequal triangles and a plain quad as emitters under a constant environment, 0 < env_prob < 1: rays, L, pdf and
    kind against light_reference.sample; at most MAX_FLIPS records may pick another triangle or the other kind of light.

    MEASURED on the MI355X: see light_reference.py (MEASURED_REFERENCE_*)."""
    inp = L.inputs()
    t, hits, sp = floor_setup(renderer, L.fan_scene())
    assert 0.0 < t["env_prob"] < 1.0
    s = renderer.light_sample(hits, inp["u"])
    assert np.asarray(s.valid).all() and np.isfinite(s.rays).all() and np.isfinite(s.buffer[:, 0:4]).all()
    offset_bits = t["instances"][hits.inst, 3]
    ref = L.sample(t, sp.p, sp.ng.astype(np.float64), sp.ns.astype(np.float64), offset_bits, inp["u"])
    env = ref["kind"] == L.KIND_ENVIRONMENT
    assert env.sum() > 100 and (~env).sum() > 300 and len(np.unique(ref["prim"][~env & (ref["inst"] == ref["inst"][~env][0])])) >= 4
    same = s.kind == ref["kind"]
    area = same & ~env
    same[area] = np.abs(sampled_points(s)[area] - ref["point"][area]).max(axis=1) < 1e-3  # the same triangle: the same point
    flips = np.nonzero(~same)[0]
    assert len(flips) <= L.MAX_FLIPS, (flips, s.buffer[flips], s.rays[flips])
    area, env = same & ~env, same & env
    assert (words(s.rays[env, 7]) == words(np.float32(L.FLT_MAX))).all() and (s.rays[:, 3] == 0).all()
    r = s.rays.astype(np.float64)
    err = {"origin": float(np.abs(r[same, 0:3] - ref["o"][same]).max()), "direction": float(np.abs(r[same, 4:7] - ref["d"][same]).max()),
           "t_max": float((np.abs(r[area, 7] - ref["t_max"][area]) / ref["t_max"][area]).max())}
    agree = same & ((s.pdf > 0) == (ref["pdf"] > 0))
    assert (same & ~agree).sum() <= L.MAX_FLIPS and (agree & (ref["pdf"] > 0)).sum() > 0.6 * L.COUNT
    both = agree & (ref["pdf"] > 0)
    to_light = L._unit(ref["point"] - sp.p.astype(np.float64))
    grazing = np.zeros(L.COUNT, bool)
    lp_ng = np.zeros((L.COUNT, 3))
    import surface_reference as R
    lp_ng[area] = R.shading_points(t, ref["inst"][area], ref["prim"][area], np.full(area.sum(), 0.3), np.full(area.sum(), 0.3))["ng"]
    grazing[area] = np.abs(np.einsum("nk,nk->n", to_light[area], lp_ng[area])) < L.GRAZING
    assert grazing.sum() < 0.01 * L.COUNT
    err["L"] = float(L.relative_error(s.L[both], ref["L"][both]).max())
    err["pdf"] = float(L.relative_error(s.pdf[both & ~grazing], ref["pdf"][both & ~grazing]).max())
    with capsys.disabled():
        print("\n[light] against the numpy reference: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()) + f", flips {len(flips)}", end="")
    assert max(err.values()) <= B.LARGEST_SOUND_ERROR, err
    for key, measured in (("pdf", L.MEASURED_REFERENCE_PDF), ("L", L.MEASURED_REFERENCE_L), ("origin", L.MEASURED_REFERENCE_ORIGIN),
                          ("direction", L.MEASURED_REFERENCE_DIRECTION), ("t_max", L.MEASURED_REFERENCE_T_MAX)):
        assert err[key] <= bar(measured, key), (key, err)


# ---------------------------------------------------------------- 3. sample agrees with evaluate

def environments(tmp_path) -> dict:
    from test_environment import sky_image
    from test_oracle_vs_ref import nested_combined_environment
    from luisarender_amd.scene import save_image
    path = str(tmp_path / "sky.exr")
    save_image(path, sky_image())
    sun = "Directional { emission : Constant { v { 3, 2.5, 2 } } angle { 40 } direction { 0.4, 1, 0.3 } }"
    return {"constant": L.FAN_CONSTANT,
            "image": f'Spherical {{ emission : Image {{ file {{ "{path}" }} }} scale {{ 2 }} transform : SRT {{ rotate {{ 0.2, 1, 0.1, 130 }} }} }}',
            "directional": sun,
            "combined": f'Combined {{ a : Spherical {{ emission : Image {{ file {{ "{path}" }} }} transform : SRT {{ rotate {{ 1, 0, 0, 20 }} }} }} '
                        f'b : {sun} scale_a {{ 0.7 }} scale_b {{ 1.5 }} transform : SRT {{ rotate {{ 0, 1, 0, 60 }} }} }}',
            "combined_nested": nested_combined_environment(f'Image {{ file {{ "{path}" }} }}')}


@pytest.mark.parametrize("kind", ["constant", "image", "directional", "combined", "combined_nested"])
def test_sample_agrees_with_evaluate(renderer, capsys, tmp_path, kind):
    """every sample with pdf > 0: its direction traced to the closest hit, then light_evaluate at what was found.  Where that is the sampled
    emitter at the sampled point, or a miss for an environment sample, L, pdf and kind are the sample's.  The nested Combined environment
    is served at all only because lrhip_light.hip compiles dev_shade.h's tree walk.

    MEASURED on the MI355X: see light_reference.py (MEASURED_EVALUATE_*)."""
    inp = L.inputs()
    t, hits, sp = floor_setup(renderer, L.fan_scene(environments(tmp_path)[kind]))
    assert 0.0 < t["env_prob"] < 1.0
    if kind == "combined_nested":
        assert int(Scene.from_string(L.fan_scene(environments(tmp_path)[kind])).view().environment_child_count) > 2
    s = renderer.light_sample(hits, inp["u"])  # (the call succeeds at all)
    assert np.asarray(s.valid).all() and np.isfinite(s.pdf).all()
    sampled = s.pdf > 0
    env = s.kind == L.KIND_ENVIRONMENT
    assert (sampled & env).sum() > 50 and (sampled & ~env).sum() > 300 and np.isfinite(s.rays[sampled]).all()
    rays = s.rays.copy()
    rays[:, 7] = INF
    rays[~sampled] = 0.0  # (a zero ray is screened)
    found = renderer.trace(rays)
    e = renderer.light_evaluate(found, rays)
    assert np.array_equal(np.asarray(e.valid), sampled) and (words(e.buffer[~sampled]) == L.invalid_result()).all()
    r = rays.astype(np.float64)
    reached = r[:, 0:3] + r[:, 4:7] * found.t.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        on_point = np.asarray(found.hit) & (np.abs(reached - sampled_points(s)).max(axis=1) < 1e-3)
    emitters = set(int(i) for i in t["light_instances"][:, 0])
    on_point &= np.isin(found.inst, list(emitters))
    compare = sampled & np.where(env, ~np.asarray(found.hit), on_point)
    assert (compare & env).sum() > 30 and (compare & ~env).sum() > 200
    assert np.array_equal(e.kind[compare], s.kind[compare])
    err_L = float(L.relative_error(e.L[compare], s.L[compare]).max())
    err_pdf = float(L.relative_error(e.pdf[compare], s.pdf[compare]).max())
    with capsys.disabled():
        print(f"\n[light] sample against evaluate, {kind}: L {err_L:.3e}, pdf {err_pdf:.3e} over {compare.sum()} records "
              f"({(compare & env).sum()} of the environment)", end="")
    assert max(err_L, err_pdf) <= B.LARGEST_SOUND_ERROR, (kind, err_L, err_pdf)
    assert err_L <= bar(L.MEASURED_EVALUATE_L, "L") and err_pdf <= bar(L.MEASURED_EVALUATE_PDF, "pdf"), (kind, err_L, err_pdf)
    # an environment sample that found geometry, an area sample that found something else: whatever it is, it is not the sampled light's kind
    # with another radiance -- a non-emitter answers KIND_NONE with zeros
    other = sampled & np.asarray(found.hit) & ~np.isin(found.inst, list(emitters))
    assert (e.kind[other] == L.KIND_NONE).all() and (e.buffer[other, 0:4] == 0).all()


# ---------------------------------------------------------------- 4. the queries compose into Li

def balance(f, g):
    total = f + g
    with np.errstate(all="ignore"):
        return np.where(total == 0, np.float32(0), f / total).astype(np.float32)


def test_queries_compose_into_li(renderer, capsys):
    """MegakernelPathTracingInstance::Li (src/integrators/mega_path.cpp:49-156) written as a numpy loop over trace -> surface -> light_evaluate
    -> light_sample -> trace(any_hit) -> bsdf_evaluate -> bsdf_sample for the Cornell box at depth 3 without Russian roulette, from the oracle's
    camera rays and sampler streams, against Oracle.li for 2 samples of 64 x 64 pixels.  Bar: rel-L1 <= max(1e-4, 2 d0), d0 = what radiance()
    (the parent commit's code) is away from the same oracle values."""
    scene = Scene.from_string(cornell_box(resolution=64, spp=2, depth=3, rr_depth=4))
    view = scene.view()
    assert int(view.integrator.max_depth) == 3 and int(view.integrator.rr_depth) > 3 and int(view.camera.kind) == 0
    t = L.light_tables(scene)
    oracle = Oracle(scene)
    w, h, depth = oracle.width, oracle.height, 3
    n = w * h
    want, got, d0_got = np.zeros((2, n, 3), np.float32), np.zeros((2, n, 3), np.float32), np.zeros((2, n, 3), np.float32)
    renderer.upload(scene)
    for sample in range(2):
        rays = np.zeros((n, 8), np.float32)
        us = np.zeros((n, 2 + 6 * depth), np.float32)
        for i in range(n):
            cam = oracle.camera_ray(i % w, i // w, sample)
            assert cam[6] == 1.0  # Box filter
            rays[i, 0:3], rays[i, 4:7], rays[i, 7] = cam[0:3], cam[3:6], INF
            oracle._lib.oracle_sampler_stream(C.byref(view), i % w, i // w, sample, 6 * depth, us[i].ctypes.data)
            want[sample, i] = oracle.li(i % w, i // w, sample)
        d0_got[sample] = renderer.radiance(rays, spp=1, spp_begin=sample)
        li, beta, pdf_bsdf = np.zeros((n, 3), np.float32), np.ones((n, 3), np.float32), np.full(n, 1e16, np.float32)
        idx = np.arange(n)  # the paths still alive; rays, beta[idx], pdf_bsdf[idx] are theirs
        for vertex in range(depth):
            hits = renderer.trace(rays)
            found = renderer.light_evaluate(hits, rays)  # an emitter, the environment, or nothing
            assert np.asarray(found.valid).all()
            li[idx] += beta[idx] * found.L * balance(pdf_bsdf[idx], found.pdf)[:, None]
            sp = renderer.surface(hits, rays)
            go = np.asarray(hits.hit) & np.asarray(sp.has_surface)
            idx, rays, hits, sp = idx[go], np.ascontiguousarray(rays[go]), RayHits(np.ascontiguousarray(hits.buffer[go])), sp.buffer[go]
            u = us[idx, 2 + 6 * vertex:8 + 6 * vertex]
            ls = renderer.light_sample(hits, np.ascontiguousarray(u[:, 0:3]))
            occluded = renderer.trace(ls.rays, any_hit=True)
            lit = (ls.pdf > 0) & ~occluded
            wi = np.where(lit[:, None], ls.rays[:, 4:7], np.float32([0, 1, 0]))
            ev = renderer.bsdf_evaluate(hits, np.ascontiguousarray(wi), rays)
            with np.errstate(all="ignore"):
                weight = balance(ls.pdf, ev.pdf) / ls.pdf
            li[idx] += np.where(lit[:, None], weight[:, None] * beta[idx] * ev.f * ls.L, np.float32(0))
            bs = renderer.bsdf_sample(hits, np.ascontiguousarray(u[:, 3:6]), rays)
            with np.errstate(all="ignore"):
                scale = np.where(bs.pdf > 0, np.float32(1) / bs.pdf, np.float32(0))
                b = beta[idx] * (scale[:, None] * bs.f)
            b[np.isnan(b).any(axis=1)] = 0  # zero_if_any_nan
            beta[idx], pdf_bsdf[idx] = b, bs.pdf
            go = ~(b <= 0).all(axis=1)
            p, ng, ns, inst = sp[:, 0:3], sp[:, 4:7], sp[:, 8:11], sp.view(np.uint32)[:, 11]
            nxt = np.zeros((len(idx), 8), np.float32)  # Interaction::spawn_ray, interaction.cpp:21-23
            nxt[:, 0:3] = L.robust_origin(p, ng.astype(np.float64), ns.astype(np.float64), t["instances"][inst, 3], bs.wi.astype(np.float64))
            nxt[:, 4:7], nxt[:, 7] = bs.wi, L.FLT_MAX
            idx, rays = idx[go], np.ascontiguousarray(nxt[go])
        got[sample] = li
    oracle.close()
    rel = lambda a: float(np.abs(a - want).sum() / np.abs(want).sum())  # noqa: E731
    d0, d = rel(d0_got), rel(got)
    with capsys.disabled():
        print(f"\n[light] Li from five queries, cornell 64 x 64 x 2 at depth 3: d0 (radiance) {d0:.3e}, composed {d:.3e}", end="")
    assert np.abs(want).sum() > 100 and np.isfinite(got).all()
    assert d <= max(1e-4, 2.0 * d0)


# ---------------------------------------------------------------- 5. points mode

def test_points_mode(renderer, capsys):
    """light_sample(points=p) for p = the hits' positions: the origin is p bit for bit, and L, pdf and d are the hit's sample's up to the
    offset the hit's origin takes off its surface (1 / 65536 of a unit here, against distances of about 2)

    MEASURED on the MI355X: see light_reference.py (MEASURED_POINTS)."""
    inp = L.inputs()
    t, hits, sp = floor_setup(renderer, L.fan_scene())
    at_hits = renderer.light_sample(hits, inp["u"])
    p = np.ascontiguousarray(sp.p)
    at_points = renderer.light_sample(points=p, u=inp["u"])
    assert np.asarray(at_points.valid).all() and np.array_equal(at_points.kind, at_hits.kind)
    assert np.array_equal(words(at_points.rays[:, 0:3]), words(p)) and (at_points.rays[:, 3] == 0).all()
    padded = np.concatenate([p, np.full((L.COUNT, 1), np.nan, np.float32)], axis=1)  # the fourth column is ignored
    assert np.array_equal(words(renderer.light_sample(points=padded, u=inp["u"]).buffer), words(at_points.buffer))
    both = (at_hits.pdf > 0) & (at_points.pdf > 0)
    assert both.sum() > 0.6 * L.COUNT and ((at_hits.pdf > 0) != (at_points.pdf > 0)).sum() <= L.MAX_FLIPS
    err = max(float(L.relative_error(at_points.L[both], at_hits.L[both]).max()), float(L.relative_error(at_points.pdf[both], at_hits.pdf[both]).max()),
              float(np.abs(at_points.rays[both, 4:7].astype(np.float64) - at_hits.rays[both, 4:7]).max()))
    with capsys.disabled():
        print(f"\n[light] points against hits: {err:.3e}", end="")
    assert err <= bar(L.MEASURED_POINTS, "points")
    bad = p.copy()
    bad[5, 1], bad[300, 0] = np.nan, np.inf
    got = renderer.light_sample(points=bad, u=inp["u"])
    spoiled = np.zeros(L.COUNT, bool)
    spoiled[[5, 300]] = True
    assert (words(got.buffer[spoiled]) == L.invalid_result()).all() and (words(got.rays[spoiled]) == 0).all()
    assert np.array_equal(words(got.buffer[~spoiled]), words(at_points.buffer[~spoiled])) and np.array_equal(words(got.rays[~spoiled]), words(at_points.rays[~spoiled]))


# ---------------------------------------------------------------- 6. batch semantics and malformed records

def test_batch_and_robustness(renderer):
    inp = L.inputs()
    n = L.COUNT
    t, hits, sp = floor_setup(renderer, L.fan_scene())
    u = np.ascontiguousarray(np.concatenate([inp["u"], np.zeros((n, 1), np.float32)], axis=1))
    full = renderer.light_sample(hits, u)
    rays = full.rays.copy()
    rays[:, 7] = INF
    found = renderer.trace(rays)
    full_e = renderer.light_evaluate(found, rays)
    assert np.asarray(full.valid).all() and np.asarray(full_e.valid).all() and len(np.unique(full_e.kind)) >= 2
    perm = np.random.default_rng(1).permutation(n)
    # a record's words are the same alone, first, last and in the middle of a shuffled batch
    shuffled = renderer.light_sample(np.ascontiguousarray(hits.buffer[perm]), np.ascontiguousarray(u[perm]))
    assert np.array_equal(words(shuffled.buffer), words(full.buffer)[perm]) and np.array_equal(words(shuffled.rays), words(full.rays)[perm])
    shuffled = renderer.light_evaluate(np.ascontiguousarray(found.buffer[perm]), np.ascontiguousarray(rays[perm]))
    assert np.array_equal(words(shuffled.buffer), words(full_e.buffer)[perm])
    for k in (0, 517, n - 1):
        one = renderer.light_sample(np.ascontiguousarray(hits.buffer[k:k + 1]), np.ascontiguousarray(u[k:k + 1]))
        assert np.array_equal(words(one.buffer)[0], words(full.buffer)[k]) and np.array_equal(words(one.rays)[0], words(full.rays)[k])
        one = renderer.light_evaluate(np.ascontiguousarray(found.buffer[k:k + 1]), np.ascontiguousarray(rays[k:k + 1]))
        assert np.array_equal(words(one.buffer)[0], words(full_e.buffer)[k])
    for m in (255, 256, 257):
        part = renderer.light_sample(np.ascontiguousarray(hits.buffer[:m]), np.ascontiguousarray(u[:m]))
        assert part.buffer.shape == (m, 8) and np.array_equal(words(part.buffer), words(full.buffer)[:m])
    junk = u.copy()
    junk[:, 3] = np.nan  # the fourth column is ignored, an [N, 3] array is the same question
    assert np.array_equal(words(renderer.light_sample(hits, junk).buffer), words(full.buffer))
    assert np.array_equal(words(renderer.light_sample(hits, inp["u"]).rays), words(full.rays))
    # count == 0 launches nothing
    empty = renderer.light_sample(np.zeros((0, 8), np.float32), np.zeros((0, 4), np.float32))
    assert len(empty) == 0 and empty.rays.shape == (0, 8) and renderer.last_light_ms() == 0.0
    assert len(renderer.light_evaluate(np.zeros((0, 8), np.float32), np.zeros((0, 8), np.float32))) == 0

    def spoil_all(mode):
        bad_hits, bad_u, bad_rays = (hits.buffer if mode == "sample" else found.buffer).copy(), u.copy(), rays.copy()
        ids = bad_hits.view(np.uint32)
        cases = {}
        k = iter(range(3, n, 7))  # spread over the blocks, valid neighbours in between

        def spoil(case):
            i = next(k)
            while mode == "evaluate" and not found.hit[i]:
                i = next(k)
            cases[case] = i
            return i

        ids[spoil("tri out of range"), 5] = 0x7FFFFFF0
        ids[spoil("tri far out of range"), 5] = 0xFFFFFFFE
        i = spoil("inst out of range")
        ids[i, 3], ids[i, 5] = 1000, L.INVALID
        i = spoil("prim out of range")
        ids[i, 4], ids[i, 5] = 0x7FFFFFFF, L.INVALID
        i = spoil("inst invalid, tri out of range")
        ids[i, 3], ids[i, 5] = L.INVALID, 0x7FFFFFF0
        bad_hits[spoil("u nan"), 1] = np.nan
        bad_hits[spoil("v inf"), 2] = np.inf
        if mode == "sample":
            i = spoil("miss")
            bad_hits[i, 0], bad_hits[i, 1:3], ids[i, 3:6] = np.inf, 0.0, L.INVALID
            bad_u[spoil("u_sel nan"), 0] = np.nan
            bad_u[spoil("u_x inf"), 1] = np.inf
            bad_u[spoil("u_y -inf"), 2] = -np.inf
            got = renderer.light_sample(bad_hits, bad_u)
        else:
            bad_rays[spoil("ray nan"), 0] = np.nan
            bad_rays[spoil("ray zero direction"), 4:7] = 0.0
            i = spoil("ray empty interval")
            bad_rays[i, 7] = bad_rays[i, 3]
            got = renderer.light_evaluate(bad_hits, bad_rays)
        spoiled = np.zeros(n, bool)
        spoiled[list(cases.values())] = True
        want = full if mode == "sample" else full_e
        for case, i in cases.items():
            assert np.array_equal(words(got.buffer)[i], L.invalid_result()), (mode, case)
        assert np.array_equal(words(got.buffer)[~spoiled], words(want.buffer)[~spoiled]), mode
        assert np.array_equal(np.asarray(got.valid), ~spoiled)
        if mode == "sample":
            assert (words(got.rays)[spoiled] == 0).all() and np.array_equal(words(got.rays)[~spoiled], words(full.rays)[~spoiled])

    spoil_all("sample")
    spoil_all("evaluate")


def test_scene_without_lighting(renderer):
    """neither lights nor an environment: no error; every record answers KIND_NONE with zeros, a malformed one included"""
    text = L.TWO_PANELS.replace("shapes { @floor, @panel_a, @panel_b }", "shapes { @floor }")
    scene = Scene.from_string(text)
    assert scene.view().light_count == 0 or scene.view().light_instance_count == 0
    renderer.upload(scene)
    inp = L.inputs()
    hits = renderer.trace(inp["rays"])
    bad = hits.buffer.copy()
    bad.view(np.uint32)[7, 5] = 0x7FFFFFF0
    s = renderer.light_sample(bad, inp["u"])
    none = np.zeros(8, np.uint32)
    none[4] = L.KIND_NONE
    assert (words(s.buffer) == none).all() and (words(s.rays) == 0).all() and np.asarray(s.valid).all()
    assert (words(renderer.light_sample(points=inp["p"], u=inp["u"]).buffer) == none).all()
    up = inp["rays"].copy()
    up[:, 5] = 1.0
    e = renderer.light_evaluate(renderer.trace(up), up)  # misses, and no environment to find
    assert (words(e.buffer) == none).all()
    assert (words(renderer.light_evaluate(hits, inp["rays"]).buffer) == none).all()


# ---------------------------------------------------------------- 7. a moved emitter, both which-triangle paths

def test_moved_emitter_and_both_paths(renderer, capsys):
    """after set_instance_transforms turns and shifts panel_a on the device, its samples lie on the moved rectangle; hit records from trace (the
    baked path) and the same points named by (inst, prim, u, v) with tri = LR_INVALID_ID (the instance path) give the same samples to last bits

    MEASURED on the MI355X: see light_reference.py (MEASURED_PATHS_P)."""
    inp = L.inputs()
    t, hits, sp = floor_setup(renderer, L.TWO_PANELS)
    tag = np.clip(np.floor(inp["u"][:, 0].astype(np.float64) * 2.0), 0, 1).astype(np.int64)
    inst, light = emitter_of_tag(t, tag)
    is_a = (t["light_L"][light] == L.PANEL_A["L"]).all(axis=1)
    panel_a = int(inst[is_a][0])
    matrix = S.srt(axis=(0, 0, 1), degrees=20.0, translate=(0.3, 0.4, -0.6))
    renderer.set_instance_transforms(matrix[None], np.array([panel_a]))
    m = matrix.T.astype(np.float64)  # row-major 4 x 4
    moved = {"corner": m[:3, :3] @ L.PANEL_A["corner"] + m[:3, 3], "e1": m[:3, :3] @ L.PANEL_A["e1"], "e2": m[:3, :3] @ L.PANEL_A["e2"]}
    hits = renderer.trace(inp["rays"])  # (the moved panel hangs above the rays' origins: the floor is found as before)
    assert np.asarray(hits.hit).all() and (hits.inst == hits.inst[0]).all()
    baked = renderer.light_sample(hits, inp["u"])
    plane, inside = L.panel_of(sampled_points(baked)[is_a], moved, 1e-4)
    assert inside.all() and plane.max() <= L.PLANE_BAR and (baked.pdf[is_a] > 0).all()
    unmoved, _ = L.panel_of(sampled_points(baked)[is_a], L.PANEL_A, 1e-4)
    assert unmoved.max() > 0.1
    texel = hits.buffer.copy()
    texel.view(np.uint32)[:, 5] = L.INVALID
    instance = renderer.light_sample(texel, inp["u"])
    assert np.array_equal(instance.kind, baked.kind) and np.array_equal(instance.pdf > 0, baked.pdf > 0)
    err = float(np.abs(sampled_points(instance) - sampled_points(baked)).max())
    with capsys.disabled():
        print(f"\n[light] moved emitter: sampled points of the two paths differ by {err:.3e}", end="")
    assert err <= bar(L.MEASURED_PATHS_P, "paths")
    lit = baked.pdf > 0
    assert float(L.relative_error(instance.pdf[lit], baked.pdf[lit]).max()) <= bar(L.MEASURED_CLOSED_FORM_PDF, "pdf")
    assert np.array_equal(words(instance.L), words(baked.L))


# ---------------------------------------------------------------- 8. pointers and errors

def test_device_pointers_equal_host_pointers(renderer):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    inp = L.inputs()
    t, hits, sp = floor_setup(renderer, L.fan_scene())
    host = renderer.light_sample(hits, inp["u"])
    d_rays = torch.from_numpy(inp["rays"].copy()).to("cuda:0")
    d_hits = torch.from_numpy(hits.buffer).to("cuda:0")
    d_u4 = torch.from_numpy(np.concatenate([inp["u"], np.zeros((L.COUNT, 1), np.float32)], axis=1)).to("cuda:0")
    got = renderer.light_sample(d_hits, d_u4)
    assert got.buffer.is_cuda and got.rays.is_cuda and got.buffer.shape == (L.COUNT, 8) and got.rays.shape == (L.COUNT, 8) and renderer.last_light_ms() > 0.0
    assert np.array_equal(words(got.buffer.cpu().numpy()), words(host.buffer)) and np.array_equal(words(got.rays.cpu().numpy()), words(host.rays))
    assert got.kind.dtype == torch.int32 and bool(got.valid.all())
    # [N, 3] tensors are padded by a copy; points too
    got = renderer.light_sample(d_hits, torch.from_numpy(inp["u"].copy()).to("cuda:0"))
    assert np.array_equal(words(got.buffer.cpu().numpy()), words(host.buffer))
    at_points = renderer.light_sample(points=torch.from_numpy(inp["p"].copy()).to("cuda:0"), u=d_u4)
    assert np.array_equal(words(at_points.buffer.cpu().numpy()), words(renderer.light_sample(points=inp["p"], u=inp["u"]).buffer))
    # trace + sample + occlusion + evaluate on the context's stream without a host round trip, then ONE synchronise
    torch.cuda.current_stream().synchronize()
    chained = renderer.light_sample(renderer.trace(d_rays, sync=False), d_u4, sync=False)
    occluded = renderer.trace(chained.rays, any_hit=True, sync=False)
    closest = renderer.trace(chained.rays, sync=False)
    evaluated = renderer.light_evaluate(closest, chained.rays, sync=False)
    renderer.synchronize()
    assert np.array_equal(words(chained.buffer.cpu().numpy()), words(host.buffer))
    assert np.array_equal(occluded.cpu().numpy(), renderer.trace(host.rays, any_hit=True))
    want = renderer.light_evaluate(renderer.trace(host.rays), host.rays)
    assert np.array_equal(words(evaluated.buffer.cpu().numpy()), words(want.buffer))
    for bad in (dict(hits=d_hits, u=inp["u"]), dict(hits=hits.buffer, u=d_u4), dict(hits=d_hits, u=d_u4[:10]), dict(hits=d_hits, u=d_u4.double()),
                dict(hits=d_hits, u=d_u4.cpu()), dict(points=d_u4, u=inp["u"])):
        with pytest.raises(ValueError):
            renderer.light_sample(**bad)
    with pytest.raises(ValueError):
        renderer.light_evaluate(d_hits, inp["rays"])


def test_errors_and_sentinels(renderer):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    lib = renderer._lib
    hits, dirs, rays = np.zeros((4, 8), np.float32), np.full((4, 4), 0.25, np.float32), np.zeros((4, 8), np.float32)
    out_rays, out = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32)
    rays[:, 5], rays[:, 7] = 1.0, np.inf

    def call(ctx, **fields):
        p = _ffi.LightQueryParams()
        p.hits, p.dirs, p.rays, p.out_rays, p.out, p.count = hits.ctypes.data, dirs.ctypes.data, rays.ctypes.data, out_rays.ctypes.data, out.ctypes.data, 4
        for field, value in fields.items():
            setattr(p, field, value)
        rc = lib.lrhip_query_light(ctx, C.byref(p))
        return rc, lib.lrhip_last_error().decode()

    fresh = MegaPathRenderer(0)
    try:
        rc, text = call(fresh._ctx)
        assert rc == LRHIP_ERROR_INVALID and "no scene uploaded" in text
        assert fresh.last_light_ms() == 0.0
    finally:
        fresh.close()
    renderer.upload(Scene.from_string(L.fan_scene()))
    ctx = renderer._ctx
    assert call(ctx)[0] == 0 and (out.view(np.uint32)[:, 4] <= 1).all()  # (a zero record names vertex 0 of BVH triangle 0)
    assert call(ctx, mode=_ffi.LIGHT_EVALUATE)[0] == 0
    assert call(ctx, mode=_ffi.LIGHT_EVALUATE, dirs=None, out_rays=None)[0] == 0  # evaluate mode reads no dirs and writes no rays
    assert call(ctx, rays=None)[0] == 0  # sample mode reads no rays
    assert call(ctx, flags=_ffi.LIGHT_FROM_POINTS)[0] == 0
    for fields in (dict(hits=None), dict(dirs=None), dict(out=None), dict(out_rays=None), dict(mode=_ffi.LIGHT_EVALUATE, rays=None),
                   dict(mode=_ffi.LIGHT_EVALUATE, hits=None), dict(flags=2), dict(flags=32), dict(flags=128 | 1), dict(mode=2), dict(mode=0xFFFFFFFF),
                   dict(mode=_ffi.LIGHT_EVALUATE, flags=_ffi.LIGHT_FROM_POINTS), dict(count=0x80000000)):
        rc, text = call(ctx, **fields)
        assert rc == LRHIP_ERROR_INVALID and "lrhip_query_light" in text, fields
    assert call(ctx, hits=None, dirs=None, rays=None, out_rays=None, out=None, count=0)[0] == 0  # count 0 launches nothing, whatever the pointers
    # misaligned device pointers: refused before anything is read (the addresses lie inside live allocations all the same)
    d = {k: torch.zeros((5, w), dtype=torch.float32, device="cuda:0") for k, w in (("hits", 8), ("rays", 8), ("dirs", 4), ("out_rays", 8), ("out", 8))}
    aligned = {k: v.data_ptr() for k, v in d.items()}
    assert all(a % 16 == 0 for a in aligned.values())
    for mode, fields in ((_ffi.LIGHT_SAMPLE, ("hits", "dirs", "out_rays", "out")), (_ffi.LIGHT_EVALUATE, ("hits", "rays", "out"))):
        for field in fields:
            rc, text = call(ctx, **{**aligned, "mode": mode, "flags": _ffi.RAY_DEVICE_POINTERS, field: aligned[field] + 4})
            assert rc == LRHIP_ERROR_INVALID and "16-byte aligned" in text, (mode, field)
    # a sentinel behind the device output buffers stays: count = 4, the fifth rows are not written
    sentinel = 1234.5
    d["out_rays"][:], d["out"][:], d["dirs"][:] = sentinel, sentinel, 0.25
    rc, _ = call(ctx, **aligned, flags=_ffi.RAY_DEVICE_POINTERS)
    renderer.synchronize()
    assert rc == 0 and bool((d["out"][:4].view(torch.int32)[:, 4] >= 0).all()) and bool((d["out"][:4, 5:8] == 0).all())
    assert bool((d["out"][4] == sentinel).all()) and bool((d["out_rays"][4] == sentinel).all()) and not bool((d["out_rays"][:4] == sentinel).any())
    d["out"][:], d["out_rays"][:] = sentinel, sentinel
    rc, _ = call(ctx, **aligned, mode=_ffi.LIGHT_EVALUATE, flags=_ffi.RAY_DEVICE_POINTERS)
    renderer.synchronize()
    assert rc == 0 and bool((d["out"][:4].view(torch.int32)[:, 4] == -1).all())  # (zero rays are screened: four invalid records)
    assert bool((d["out"][4] == sentinel).all()) and bool((d["out_rays"] == sentinel).all())  # evaluate mode writes no rays
