"""BSDF queries on the device (include/lrhip.h: lrhip_query_bsdf): every closure against the oracle's
Surface::Closure::evaluate / sample (tests/bsdf_reference.py), Lambert's closed form, sample against evaluate, Layered by its means, the lean
closures on the heavier kernels, batch semantics, the two which-triangle paths on a moved scene, pointers, errors."""
import ctypes as C

import numpy as np
import pytest

import bsdf_reference as B
import instance_scene as S
import raycast_reference as RR
import surface_reference as R
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import DeviceError, MegaPathRenderer

pytestmark = pytest.mark.gpu

LRHIP_ERROR_INVALID, LRHIP_ERROR_UNSUPPORTED = -1, -3
FEAT_MIX, FEAT_LAYERED = 32, 64  # dev_wavefront.h: kFeatMix, kFeatLayered


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def words(results) -> np.ndarray:
    return results.buffer.view(np.uint32)


def pad(a) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=1))


_DEVICE = {}


def device_answers(renderer, name) -> dict:
    """the device's answers for B.inputs(name), computed once per material: the scene's quad seen along B.rays(name), the hit records as
    trace() finds them (the renderer's path); {"hits", "evaluate", "sample"}.  The frame at every record is the oracle's flat patch."""
    if name not in _DEVICE:
        inp, rays = B.inputs(name), B.rays(name)
        renderer.upload(Scene.from_string(B.scene_text(name)))
        hits = renderer.trace(rays)
        assert np.asarray(hits.hit).all() and np.array_equal(hits.prim, inp["prim"])
        for records in (hits, B.hit_records(name)):
            s = renderer.surface(records, rays)
            assert np.asarray(s.valid).all() and np.asarray(s.has_surface).all()
            assert (s.ng == np.float32([0, 0, 1])).all() and (s.ns == np.float32([0, 0, 1])).all() and (s.tangent == np.float32([1, 0, 0])).all()
            assert np.array_equal(np.asarray(s.back_facing), inp["wo"][:, 2] < 0)
        _DEVICE[name] = {"hits": hits, "evaluate": renderer.bsdf_evaluate(hits, inp["wi"], rays), "sample": renderer.bsdf_sample(hits, inp["u"], rays)}
        for r in (_DEVICE[name]["evaluate"], _DEVICE[name]["sample"]):
            # (a failed sample -- pdf = 0 -- carries what the closure left in f and wi: NaN after a total internal reflection, as in the reference)
            assert np.asarray(r.valid).all() and np.isfinite(r.pdf).all() and np.isfinite(r.buffer[r.pdf > 0, 0:7]).all()
            r.buffer.setflags(write=False)
        assert np.isfinite(_DEVICE[name]["evaluate"].buffer[:, 0:7]).all()
    return _DEVICE[name]


# ---------------------------------------------------------------- 1. every deterministic closure against the oracle

def compare(name, mode, dev, ref) -> dict:
    """mode: "evaluate", "sample" or "sample_b" (B.excluded) -> {"f", "pdf"[, "wi"]}: the largest errors over the records that are not
    excluded and on which both sides say pdf > 0; asserts that they disagree about pdf > 0 (sampling: or about the event) on at most
    B.MAX_FLIPS of the records that are not excluded"""
    keep = ~B.excluded(name, mode)
    dev_answers, ref_answers = dev.pdf > 0.0, ref[:, 3] > 0.0
    agree = dev_answers == ref_answers
    if mode != "evaluate":
        agree &= ~(dev_answers & ref_answers) | (dev.event == ref[:, 7].astype(np.uint32))
    flips = np.nonzero(keep & ~agree)[0]
    assert len(flips) <= B.MAX_FLIPS, (name, mode, flips, dev.buffer[flips], ref[flips])
    both = keep & agree & ref_answers
    assert both.sum() > 0.3 * B.COUNT, (name, mode, both.sum())
    err = {"f": float(B.relative_error(dev.f[both], ref[both, 0:3]).max()), "pdf": float(B.relative_error(dev.pdf[both], ref[both, 3]).max())}
    if mode != "evaluate":
        err["wi"] = float(np.abs(dev.wi[both].astype(np.float64) - ref[both, 4:7]).max())
    return err


ZERO_BAR_NOTE = ("a bar of 4 x a measured 0.0 asks for the oracle's bits: the kernels are built with the oracle's arithmetic, so a last-bit difference "
                 "here may come from another host compiler or libm under the oracle, or another ROCm, and not from the device code -- compare the "
                 "printed errors with one ulp (1.2e-7 relative) before looking for a bug, and measure again (bsdf_reference.py: MEASURED_*)")


@pytest.mark.parametrize("name", B.DETERMINISTIC)
def test_closure_against_the_oracle(renderer, capsys, name):
    """evaluate and sample of one material for B.COUNT records against the oracle.  The largest errors are printed; the bars are 4 x the
    values recorded per class of material in bsdf_reference.py"""
    dev, ref, inp = device_answers(renderer, name), B.oracle_answers(name), B.inputs(name)
    cls = B.CLASS_OF[name]
    assert np.array_equal(dev["evaluate"].wi, inp["wi"]) and (dev["evaluate"].event == 0).all()  # the unit wi that was used: taken bit for bit
    e, s = compare(name, "evaluate", dev["evaluate"], ref["evaluate"]), compare(name, "sample", dev["sample"], ref["sample"])
    with capsys.disabled():
        print(f"\n[bsdf] {name} ({cls}): evaluate f {e['f']:.3e} pdf {e['pdf']:.3e}; sample f {s['f']:.3e} pdf {s['pdf']:.3e} wi {s['wi']:.3e}", end="")
    assert max(*e.values(), *s.values()) <= B.LARGEST_SOUND_ERROR, (name, e, s)  # beyond this it is a bug, whatever the bars say
    for got, measured in ((e["f"], B.MEASURED_EVALUATE_F), (e["pdf"], B.MEASURED_EVALUATE_PDF), (s["f"], B.MEASURED_SAMPLE_F),
                          (s["pdf"], B.MEASURED_SAMPLE_PDF), (s["wi"], B.MEASURED_SAMPLE_WI)):
        assert got <= B.MARGIN * measured[cls], (name, e, s, ZERO_BAR_NOTE)
    sampled = dev["sample"].pdf > 0
    assert np.abs(np.linalg.norm(dev["sample"].wi[sampled].astype(np.float64), axis=1) - 1.0).max() < 1e-5


@pytest.mark.parametrize("name", sorted(B.MIX_ROOT_RATIO))
def test_mix_sample_b_against_the_oracle(renderer, capsys, name):
    """the Mix materials with lobe numbers of the ROOT's "sample b" branch (B.sample_b_inputs), where the reference draws the direction from
    child a, evaluates child b there and mixes with the roles swapped: the case above confines u_lobe to "sample a" at the root, and the
    sample-against-evaluate case leaves the two trees out.  Same comparison, the bars 4 x the values recorded in bsdf_reference.py"""
    dev, inp, rays, ref = device_answers(renderer, name), B.sample_b_inputs(name), B.rays(name), B.oracle_sample_b(name)
    renderer.upload(Scene.from_string(B.scene_text(name)))
    got = renderer.bsdf_sample(dev["hits"], inp["u"], rays)
    assert np.asarray(got.valid).all() and np.isfinite(got.pdf).all() and np.isfinite(got.buffer[got.pdf > 0, 0:7]).all()
    assert not np.array_equal(words(got), words(dev["sample"]))
    s = compare(name, "sample_b", got, ref)
    with capsys.disabled():
        print(f"\n[bsdf] {name}, sample b at the root: f {s['f']:.3e} pdf {s['pdf']:.3e} wi {s['wi']:.3e}", end="")
    assert max(s.values()) <= B.LARGEST_SOUND_ERROR, (name, s)
    assert s["f"] <= B.MARGIN * B.MEASURED_SAMPLE_B_F and s["pdf"] <= B.MARGIN * B.MEASURED_SAMPLE_B_PDF, (name, s, ZERO_BAR_NOTE)
    assert s["wi"] <= B.MARGIN * B.MEASURED_SAMPLE_B_WI, (name, s, ZERO_BAR_NOTE)


# ---------------------------------------------------------------- 2. Lambert's closed form

def test_lambert_closed_form(renderer):
    """f = Kd / pi * wi.z and pdf = wi.z / pi above the surface (matte.cpp:95; tests/test_oracle_bsdf.py: rtol 1e-5), exact zeros below it"""
    got = device_answers(renderer, "matte")["evaluate"]
    z = got.wi[:, 2].astype(np.float64)
    above = z > 0
    assert 0.4 < above.mean() < 0.6
    kd = np.array([0.6, 0.5, 0.4])
    assert np.allclose(got.f[above], kd / np.pi * z[above, None], rtol=1e-5, atol=0.0)
    assert np.allclose(got.pdf[above], z[above] / np.pi, rtol=1e-5, atol=0.0)
    assert (got.f[~above] == 0).all() and (got.pdf[~above] == 0).all()


# ---------------------------------------------------------------- 3. sample agrees with evaluate

@pytest.mark.parametrize("name", B.SELF_CONSISTENT)
def test_sample_agrees_with_evaluate(renderer, name):
    """the device's sampled wi fed back through evaluate mode gives the sample's f and pdf (tests/test_oracle_bsdf.py's tolerances)"""
    dev, rays = device_answers(renderer, name), B.rays(name)
    sample = dev["sample"]
    sampled = sample.pdf > 0
    assert sampled.mean() > 0.5
    renderer.upload(Scene.from_string(B.scene_text(name)))
    wi = np.where(sampled[:, None], sample.wi, np.float32([0, 0, 1]))
    again = renderer.bsdf_evaluate(dev["hits"], wi, rays)
    f, f2 = sample.f[sampled].astype(np.float64), again.f[sampled].astype(np.float64)
    pdf, pdf2 = sample.pdf[sampled].astype(np.float64), again.pdf[sampled].astype(np.float64)
    bad = np.nonzero(~(np.abs(f - f2) <= 1e-6 + 2e-3 * np.abs(f2)).all(axis=1) | ~(np.abs(pdf - pdf2) <= 2e-3 * np.maximum(pdf, 1e-3)))[0]
    assert len(bad) == 0, (name, len(bad), sample.buffer[sampled][bad[:4]], again.buffer[sampled][bad[:4]])


# ---------------------------------------------------------------- 4. Layered

@pytest.mark.parametrize("name", B.LAYERED)
def test_layered_by_its_means(renderer, capsys, name):
    """Layered's evaluate is a random-walk estimator seeded from the bits of p and the directions: the device's records and the oracle's are
    independent draws of the same estimator, so their means over the batch agree within 4 standard errors, per channel; sample mode: the
    means of f and of wi.z.  A second run of both modes gives the same bits."""
    dev, ref, inp, rays = device_answers(renderer, name), B.oracle_answers(name), B.inputs(name), B.rays(name)
    n = B.COUNT

    def means_agree(what, a, b):
        a, b = np.asarray(a, np.float64).reshape(n, -1), np.asarray(b, np.float64).reshape(n, -1)
        diff, bar = np.abs(a.mean(axis=0) - b.mean(axis=0)), 4.0 * np.sqrt(a.var(axis=0, ddof=1) / n + b.var(axis=0, ddof=1) / n)
        with capsys.disabled():
            print(f"\n[bsdf] {name} {what}: device {a.mean(axis=0)}, oracle {b.mean(axis=0)}, |difference| / bar {diff / bar}", end="")
        assert (bar > 0).all() and (diff <= bar).all(), (name, what, a.mean(axis=0), b.mean(axis=0), bar)

    means_agree("evaluate f", dev["evaluate"].f, ref["evaluate"][:, 0:3])
    means_agree("sample f", dev["sample"].f, ref["sample"][:, 0:3])
    means_agree("sample wi.z", dev["sample"].wi[:, 2], ref["sample"][:, 6])
    assert (dev["evaluate"].pdf > 0).mean() > 0.3 and (dev["sample"].pdf > 0).mean() > 0.5
    assert set(dev["sample"].event.tolist()) <= {0, 1, 2}
    renderer.upload(Scene.from_string(B.scene_text(name)))
    assert np.array_equal(words(renderer.bsdf_evaluate(dev["hits"], inp["wi"], rays)), words(dev["evaluate"]))
    assert np.array_equal(words(renderer.bsdf_sample(dev["hits"], inp["u"], rays)), words(dev["sample"]))


# ---------------------------------------------------------------- 5. the lean closures on the Mix and Layered kernels

def test_forced_kernels_give_the_lean_kernels_bits(renderer):
    """lrhip_set_diagnostics(force_features) puts a Matte scene on the instantiation that holds Mix, then on the one that holds Mix and
    Layered: the basic closures are evaluated inline in all three, to the same bits"""
    dev, inp, rays = device_answers(renderer, "matte"), B.inputs("matte"), B.rays("matte")
    renderer.upload(Scene.from_string(B.scene_text("matte")))
    try:
        for force in (FEAT_MIX, FEAT_MIX | FEAT_LAYERED):
            renderer.set_diagnostics(force_features=force)
            assert np.array_equal(words(renderer.bsdf_evaluate(dev["hits"], inp["wi"], rays)), words(dev["evaluate"])), force
            assert np.array_equal(words(renderer.bsdf_sample(dev["hits"], inp["u"], rays)), words(dev["sample"])), force
    finally:
        renderer.set_diagnostics(force_features=0)


# the kernel is picked from the closures of the scene's surfaces, not from the renderer's feature mask: MegaVPTNaive clears that mask of the
# closure bits (its kernel holds everything), the AOV, Direct and Normal integrators set all of them
OTHER_INTEGRATORS = [("MegaVPTNaive", "mix"), ("MegaVPTNaive", "mix_deep"), ("MegaVPTNaive", "layered"), ("MegaVPTNaive", "disney"), ("MegaVPTNaive", "matte"),
                     ("Direct", "mix_glass"), ("Normal", "matte"), ('AOV { components { "albedo", "mask" }', "layered_medium"), ("AOV", "plastic")]


@pytest.mark.parametrize("integrator,name", OTHER_INTEGRATORS, ids=[f"{i.split()[0]}-{n}" for i, n in OTHER_INTEGRATORS])
def test_other_integrators_give_the_megapath_scenes_bits(renderer, integrator, name):
    """the same quad and material under another integrator: the same hit records, and both modes answer with the MegaPath scene's bits
    (Layered too: its walk is seeded from p and the directions, which are the same)"""
    dev, inp, rays = device_answers(renderer, name), B.inputs(name), B.rays(name)
    text = B.scene_text(name)
    assert "integrator : MegaPath {" in text
    renderer.upload(Scene.from_string(text.replace("integrator : MegaPath {", "integrator : " + (integrator if "{" in integrator else integrator + " {"))))
    hits = renderer.trace(rays)
    assert np.array_equal(hits.buffer.view(np.uint32), dev["hits"].buffer.view(np.uint32))
    assert np.array_equal(words(renderer.bsdf_evaluate(hits, inp["wi"], rays)), words(dev["evaluate"]))
    assert np.array_equal(words(renderer.bsdf_sample(hits, inp["u"], rays)), words(dev["sample"]))
    assert (dev["evaluate"].pdf > 0).mean() > 0.3 and (dev["sample"].pdf > 0).mean() > 0.5


# ---------------------------------------------------------------- 6. batch semantics

def test_batch_semantics(renderer):
    name = "plastic"
    inp, rays, hits = B.inputs(name), B.rays(name), B.hit_records(name)
    renderer.upload(Scene.from_string(B.scene_text(name)))
    n = B.COUNT
    dirs = {"evaluate": pad(inp["wi"]), "sample": pad(inp["u"])}
    call = {"evaluate": renderer.bsdf_evaluate, "sample": renderer.bsdf_sample}
    full = {mode: call[mode](hits, dirs[mode], rays) for mode in call}
    perm = np.random.default_rng(1).permutation(n)
    for mode in call:
        assert np.asarray(full[mode].valid).all() and (full[mode].pdf > 0).mean() > 0.4
        # the fourth column is ignored, an [N, 3] array is the same question
        junk = dirs[mode].copy()
        junk[:, 3] = np.nan
        assert np.array_equal(words(call[mode](hits, junk, rays)), words(full[mode]))
        assert np.array_equal(words(call[mode](hits, inp["wi" if mode == "evaluate" else "u"], rays)), words(full[mode]))
        # a permuted batch gives permuted bits; a prefix gives a prefix
        shuffled = call[mode](np.ascontiguousarray(hits[perm]), np.ascontiguousarray(dirs[mode][perm]), np.ascontiguousarray(rays[perm]))
        assert np.array_equal(words(shuffled), words(full[mode])[perm])
        for m in (0, 1, 255, 256, 257):
            part = call[mode](np.ascontiguousarray(hits[:m]), np.ascontiguousarray(dirs[mode][:m]), np.ascontiguousarray(rays[:m]))
            assert part.buffer.shape == (m, 8) and np.array_equal(words(part), words(full[mode])[:m]), m
    # count == 0 launches nothing
    empty = renderer.bsdf_evaluate(np.zeros((0, 8), np.float32), np.zeros((0, 4), np.float32))
    assert len(empty) == 0 and renderer.last_bsdf_ms() == 0.0

    # malformed records give the invalid record, their neighbours keep their bits
    for mode in call:
        bad_hits, bad_rays, bad_dirs = hits.copy(), rays.copy(), dirs[mode].copy()
        ids = bad_hits.view(np.uint32)
        cases = {}
        k = iter(range(3, n, 7))  # spread over the blocks, valid neighbours in between

        def spoil(case):
            i = next(k)
            cases[case] = i
            return i

        i = spoil("miss")
        bad_hits[i, 0], bad_hits[i, 1:3], ids[i, 3:6] = np.inf, 0.0, B.INVALID
        ids[spoil("tri out of range"), 5] = 2
        ids[spoil("tri far out of range"), 5] = 0xFFFFFFFE
        ids[spoil("inst out of range"), 3] = 1
        ids[spoil("inst invalid"), 3] = B.INVALID
        ids[spoil("prim out of range"), 4] = 2
        ids[spoil("prim far out of range"), 4] = 0x7FFFFFFF
        bad_hits[spoil("u nan"), 1] = np.nan
        bad_hits[spoil("v inf"), 2] = np.inf
        bad_rays[spoil("ray nan"), 0] = np.nan
        bad_rays[spoil("ray zero direction"), 4:7] = 0.0
        i = spoil("ray empty interval")
        bad_rays[i, 7] = bad_rays[i, 3]
        bad_dirs[spoil("dirs nan"), 0] = np.nan
        bad_dirs[spoil("dirs inf"), 1] = np.inf
        bad_dirs[spoil("dirs -inf"), 2] = -np.inf
        if mode == "evaluate":
            bad_dirs[spoil("wi zero"), 0:3] = 0.0
            bad_dirs[spoil("wi minus zero"), 0:3] = -0.0
        got = call[mode](bad_hits, bad_dirs, bad_rays)
        spoiled = np.zeros(n, bool)
        spoiled[list(cases.values())] = True
        for case, i in cases.items():
            assert np.array_equal(words(got)[i], B.invalid_record()), (mode, case)
        assert np.array_equal(words(got)[~spoiled], words(full[mode])[~spoiled]), mode
        assert np.array_equal(np.asarray(got.valid), ~spoiled)

    # wi need not be normalised: a scaled wi is the same direction to rounding; rays=None: wo = ng
    scaled = renderer.bsdf_evaluate(hits, pad(inp["wi"] * np.float32(3.0)), rays)
    assert np.abs(scaled.wi - inp["wi"]).max() < 2e-7 and np.allclose(scaled.f, full["evaluate"].f, rtol=1e-4, atol=1e-7)
    front = renderer.bsdf_evaluate(hits, dirs["evaluate"])
    up = np.zeros_like(rays)
    up[:, 0:3], up[:, 4:7], up[:, 7] = B.points(name) + [0, 0, 1], [0, 0, -1], np.inf
    assert np.array_equal(words(front), words(renderer.bsdf_evaluate(hits, dirs["evaluate"], up)))


# ---------------------------------------------------------------- 7. which-triangle paths and a moved scene

def test_both_paths_on_a_moved_scene(renderer, capsys):
    """the instanced room after set_instance_transforms on the device: on the moved Matte ball the baked path (tri from trace) and the instance
    path (tri = LR_INVALID_ID) agree, and f is Kd / pi * dot(ns, wi) for the MOVED shading normal (the float64 reference over the host scene
    moved the same way).  The bar: both normals are within R.BAR_NS of the reference componentwise, so dot(ns, wi) of a unit wi moves by at
    most sqrt(3) * BAR_NS against the reference and twice that between the paths, plus the float32 rounding of the dot product and the two
    multiplications (8 ulp of 1); Matte reads nothing else of the point, so R.BAR_P adds nothing."""
    scene = S.room()
    ids = S.check_room(scene)
    ball, lamp = ids["ball_a"], ids["lamp"]
    kd = np.array([0.7, 0.3, 0.2])
    renderer.upload(scene)
    n = 4 * B.COUNT
    rays = RR.make_rays(scene, n=n, seed=9)
    before_hits = renderer.trace(rays)
    matrix = S.srt(scale=(0.75, 0.5, 0.6), axis=(0, 1, 1), degrees=-110.0, translate=(0.5, 1.25, 1.0))[None]
    renderer.set_instance_transforms(matrix, np.array([ball]))
    scene.set_instance_transforms(matrix, np.array([ball]))  # the host mirror, for the reference only
    hits = renderer.trace(rays)
    on_ball = np.asarray(hits.hit) & (hits.inst == ball)
    assert on_ball.sum() > 20 and not np.array_equal(hits.buffer.view(np.uint32), before_hits.buffer.view(np.uint32))
    ref = R.shading_points(scene, hits.inst[on_ball], hits.prim[on_ball], hits.u[on_ball], hits.v[on_ball])
    rng = np.random.default_rng(5)
    wi = np.zeros((n, 3))
    wi[:, 1] = 1.0
    jitter = rng.normal(size=(int(on_ball.sum()), 3))
    wi[on_ball] = ref["ng"] + 0.5 * jitter / np.linalg.norm(jitter, axis=1, keepdims=True)
    wi = (wi / np.linalg.norm(wi, axis=1, keepdims=True)).astype(np.float32)
    texel = hits.buffer.copy()
    texel.view(np.uint32)[:, 5] = R.INVALID
    baked, instance = renderer.bsdf_evaluate(hits, wi), renderer.bsdf_evaluate(texel, wi)  # rays=None: wo = ng
    assert np.array_equal(np.asarray(baked.valid), np.asarray(instance.valid))
    assert not np.asarray(baked.valid)[np.asarray(hits.hit) & (hits.inst == lamp)].any()  # a valid hit on an instance without a surface
    assert np.array_equal(np.asarray(baked.valid), np.asarray(hits.hit) & (hits.inst != lamp))
    cos = np.einsum("nk,nk->n", ref["ns"], baked.wi[on_ball].astype(np.float64))
    clear = (cos > 0.2) & (np.einsum("nk,nk->n", ref["ng"], baked.wi[on_ball].astype(np.float64)) > 0.2)
    assert clear.sum() > 20
    one = np.sqrt(3.0) * R.BAR_NS + 8.0 * 2.0 ** -24
    want = kd[None, :] / np.pi * cos[clear, None]
    for path, got in (("baked", baked), ("instance", instance)):
        err = np.abs(got.f[on_ball][clear] - want).max(axis=0)
        with capsys.disabled():
            print(f"\n[bsdf] moved ball, {path}: |f - Kd / pi dot(ns, wi)| {err}, bar {kd / np.pi * one}", end="")
        assert (err <= kd / np.pi * one).all(), (path, err)
        assert np.allclose(got.pdf[on_ball][clear], cos[clear] / np.pi, rtol=0.0, atol=one / np.pi)
    between = np.abs(baked.f[on_ball][clear].astype(np.float64) - instance.f[on_ball][clear]).max(axis=0)
    assert (between <= kd / np.pi * 2.0 * one).all(), between


# ---------------------------------------------------------------- 8. pointers

def test_device_pointers_equal_host_pointers(renderer):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    name = "mix_glass"
    dev, inp, rays = device_answers(renderer, name), B.inputs(name), B.rays(name)
    renderer.upload(Scene.from_string(B.scene_text(name)))
    d_rays = torch.from_numpy(rays).to("cuda:0")
    d_hits = torch.from_numpy(dev["hits"].buffer).to("cuda:0")
    d_wi, d_u = torch.from_numpy(pad(inp["wi"])).to("cuda:0"), torch.from_numpy(pad(inp["u"])).to("cuda:0")
    got = renderer.bsdf_evaluate(d_hits, d_wi, d_rays)
    assert got.buffer.is_cuda and got.buffer.shape == (B.COUNT, 8) and renderer.last_bsdf_ms() > 0.0
    assert np.array_equal(got.buffer.cpu().numpy().view(np.uint32), words(dev["evaluate"]))
    got = renderer.bsdf_sample(d_hits, d_u, d_rays)
    assert np.array_equal(got.buffer.cpu().numpy().view(np.uint32), words(dev["sample"]))
    assert got.event.dtype == torch.int32 and bool(got.valid.all())
    # [N, 3] tensors are padded by a copy
    got = renderer.bsdf_sample(d_hits, torch.from_numpy(inp["u"].copy()).to("cuda:0"), d_rays)
    assert np.array_equal(got.buffer.cpu().numpy().view(np.uint32), words(dev["sample"]))
    # trace + sample on the context's stream without a host round trip, then ONE synchronise
    torch.cuda.current_stream().synchronize()
    chained = renderer.bsdf_sample(renderer.trace(d_rays, sync=False), d_u, d_rays, sync=False)
    renderer.synchronize()
    assert np.array_equal(chained.buffer.cpu().numpy().view(np.uint32), words(dev["sample"]))
    for bad in ((d_hits, inp["wi"], d_rays), (dev["hits"].buffer, d_wi, None), (d_hits, d_wi, rays), (d_hits, d_wi[:10], None), (d_hits, d_wi.double(), None),
                (d_hits, d_wi.cpu(), None)):
        with pytest.raises(ValueError):
            renderer.bsdf_evaluate(*bad)


# ---------------------------------------------------------------- 9. errors

def test_errors(renderer):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    lib = renderer._lib
    hits, dirs, out = np.zeros((4, 8), np.float32), np.ones((4, 4), np.float32), np.zeros((4, 8), np.float32)

    def call(ctx, **fields):
        p = _ffi.BsdfQueryParams()
        p.hits, p.dirs, p.out, p.count = hits.ctypes.data, dirs.ctypes.data, out.ctypes.data, 4
        for field, value in fields.items():
            setattr(p, field, value)
        rc = lib.lrhip_query_bsdf(ctx, C.byref(p))
        return rc, lib.lrhip_last_error().decode()

    fresh = MegaPathRenderer(0)
    try:
        rc, text = call(fresh._ctx)
        assert rc == LRHIP_ERROR_INVALID and "no scene uploaded" in text
        assert fresh.last_bsdf_ms() == 0.0
    finally:
        fresh.close()
    renderer.upload(Scene.from_string(B.scene_text("matte")))
    ctx = renderer._ctx
    assert call(ctx)[0] == 0 and (out.view(np.uint32)[:, 7] == 0).all() and (out[:, 3] > 0).all()  # (a zero record names vertex 0 of BVH triangle 0)
    assert call(ctx, mode=_ffi.BSDF_SAMPLE)[0] == 0
    for fields in (dict(hits=None), dict(dirs=None), dict(out=None), dict(flags=2), dict(flags=32), dict(flags=64 | 1), dict(mode=2), dict(mode=0xFFFFFFFF),
                   dict(count=0x80000000)):
        rc, text = call(ctx, **fields)
        assert rc == LRHIP_ERROR_INVALID and "lrhip_query_bsdf" in text, fields
    assert call(ctx, hits=None, dirs=None, out=None, count=0)[0] == 0  # count 0 launches nothing, whatever the pointers
    # misaligned device pointers: refused before anything is read (the addresses lie inside live allocations all the same)
    d = {k: torch.zeros((5, w), dtype=torch.float32, device="cuda:0") for k, w in (("hits", 8), ("rays", 8), ("dirs", 4), ("out", 8))}
    aligned = {k: t.data_ptr() for k, t in d.items()}
    assert all(a % 16 == 0 for a in aligned.values())
    for field in aligned:
        rc, text = call(ctx, **{**aligned, "flags": _ffi.RAY_DEVICE_POINTERS, field: aligned[field] + 4})
        assert rc == LRHIP_ERROR_INVALID and "16-byte aligned" in text, field
    rc, _ = call(ctx, **aligned, flags=_ffi.RAY_DEVICE_POINTERS)
    renderer.synchronize()
    assert rc == 0 and bool((d["out"][:4].view(torch.int32)[:, 7] == -1).all())  # (zero rays are screened: four invalid records)
    d["dirs"][:] = 1.0
    rc, _ = call(ctx, **{**aligned, "rays": None}, flags=_ffi.RAY_DEVICE_POINTERS)
    renderer.synchronize()
    assert rc == 0 and bool((d["out"][:4, 3] > 0).all()) and bool((d["out"][4] == 0).all())  # count = 4: the fifth row is not written
    # a scene with Mix / Layered surfaces nested in each other is refused
    for name in B.NESTED:
        renderer.upload(Scene.from_string(B.scene_text(name)))
        rc, text = call(renderer._ctx)
        assert rc == LRHIP_ERROR_UNSUPPORTED and "nested" in text, name
    with pytest.raises(DeviceError, match=f"lrhip error {LRHIP_ERROR_UNSUPPORTED}"):
        renderer.bsdf_sample(hits, dirs)
