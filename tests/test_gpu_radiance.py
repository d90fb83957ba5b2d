"""Radiance queries on the device (include/lrhip.h: lrhip_trace_radiance): MegaPath's estimator along caller-supplied rays.
The yardstick is the CPU oracle's film: a query whose rays ARE the oracle's camera rays, with the pixels' sampler streams, must walk the
film's paths.  Then the closed forms, the screening, the edges of a batch, order and grouping, the torch path and the error returns."""
import ctypes as C

import numpy as np
import pytest

from luisarender_amd import Scene, _ffi
from luisarender_amd.render import DeviceError, MegaPathRenderer
from luisarender_amd.scenes import cornell_box
from oracle.check import Oracle

pytestmark = pytest.mark.gpu

LRHIP_ERROR_INVALID, LRHIP_ERROR_UNSUPPORTED = -1, -3
INF = np.float32(np.inf)
SAMPLER_INDEPENDENT, SAMPLER_SOBOL, SAMPLER_PADDED_SOBOL = 0, 1, 2  # LR_SAMPLER_* (lr_scene.h)


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def _rel_l1(a, b):
    return float(np.abs(a[..., :3] - b[..., :3]).sum() / max(np.abs(b[..., :3]).sum(), 1e-20))


def _camera_rays(oracle, sample):
    """the oracle's camera ray of every pixel at one sample index as [H * W, 8] rows (o, t_min = 0, d, t_max = +inf), row py * W + px, and
    the rays' weights"""
    w, h = oracle.width, oracle.height
    raw = np.zeros((h * w, 7), np.float32)
    base, fn, ctx = raw.ctypes.data, oracle._lib.oracle_camera_ray, oracle._ctx
    for i in range(h * w):
        fn(ctx, i % w, i // w, sample, base + 28 * i)
    rays = np.empty((h * w, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = raw[:, 0:3], 0.0, raw[:, 3:6], INF
    return rays, raw[:, 6]


class Case:
    """a scene, the oracle's film of its first `spp` samples, and the oracle's camera rays of each of them"""

    def __init__(self, text, spp):
        self.scene = Scene.from_string(text)
        self.spp = spp
        oracle = Oracle(self.scene)
        self.width, self.height = oracle.width, oracle.height
        self.film, _ = oracle.render(0, spp)
        pairs = [_camera_rays(oracle, s) for s in range(spp)]
        self.rays = [p[0] for p in pairs]
        self.weights = np.stack([p[1] for p in pairs])
        oracle.close()
        self.film.setflags(write=False)

    def query(self, renderer, **kwargs):
        """sample s of every pixel's camera ray for s in 0 .. spp - 1, one call per sample, accumulated -> raw [H, W, 4]"""
        renderer.upload(self.scene)
        total = None
        for s in range(self.spp):
            total = renderer.radiance(self.rays[s], spp=1, spp_begin=s, raw=True, accumulate_into=total, **kwargs)
        return total.reshape(self.height, self.width, 4)


@pytest.fixture(scope="module")
def cornell128():
    return Case(cornell_box(resolution=128, spp=16), 16)


def test_camera_rays_reproduce_the_oracles_film(renderer, cornell128, capsys):
    """The bars of test_gpu_parity.py::test_cornell_same_paths_and_image, which the film kernel is held to at this size: the query walks the
    same paths, from the oracle's own ray bits."""
    case = cornell128
    assert (case.weights == 1.0).all()  # Box filter: Russian roulette sees the film's throughput
    renderer.upload(case.scene)
    before = renderer.counters()["paths"]
    got = case.query(renderer, counters=True)
    assert renderer.counters()["paths"] - before == 128 * 128 * 16
    rel = _rel_l1(got, case.film)
    px = np.abs(got[..., :3] - case.film[..., :3]).max(axis=-1) / (np.abs(case.film[..., :3]).max(axis=-1) + 1e-3)
    with capsys.disabled():
        print(f"\n[radiance] cornell 128 x 128 x 16: rel-L1 {rel:.3e}, 99.9 % quantile {np.quantile(px, 0.999):.3e}")
    assert (got[..., 3] == 16).all()
    assert rel < 1e-4
    assert np.quantile(px, 0.999) < 1e-3


def _variant_text(variant):
    if variant == "thin_lens":
        return cornell_box(resolution=64, spp=8).replace("Camera cam : Pinhole {",
                                                         "Camera cam : ThinLens {\n  aperture { 1.4 } focal_length { 50 } focus_distance { 900 }")
    return cornell_box(resolution=64, spp=8, sampler=variant)


@pytest.mark.parametrize("variant", ["PaddedSobol", "Sobol", "thin_lens"])
def test_stream_alignment_under_the_other_draws(renderer, capsys, variant):
    """The samplers whose pixel sample is not two plain draws, and the camera that draws a lens sample: the query must skip exactly what Li
    draws before its first bounce.  Bar: max(1e-4, 2 d0), d0 = what lrhip_render of the same scene on the all-closures one-path-per-lane
    kernel (mask 124 | sampler bit, the parent's code) is away from the oracle; one flipped path is a discrete event at 32 k paths."""
    case = Case(_variant_text(variant), 8)
    view = case.scene.view()
    assert int(view.camera.kind) == (1 if variant == "thin_lens" else 0)  # LR_CAMERA_THIN_LENS / LR_CAMERA_PINHOLE: the case is what its name says
    assert int(view.sampler.kind) == {"PaddedSobol": SAMPLER_PADDED_SOBOL, "Sobol": SAMPLER_SOBOL, "thin_lens": SAMPLER_INDEPENDENT}[variant]
    assert (case.weights == 1.0).all()
    renderer.upload(case.scene)
    renderer.set_diagnostics(force_features=124)
    try:
        renderer.render(0, 8, sync=True)
        assert renderer.last_variant() & ~3 == 124
        d0 = _rel_l1(renderer.download(converted=False), case.film)
    finally:
        renderer.set_diagnostics()
    got = case.query(renderer)
    d = _rel_l1(got, case.film)
    with capsys.disabled():
        print(f"\n[radiance] {variant}: d0 (lrhip_render, mask {renderer.last_variant()}) {d0:.3e}, query {d:.3e}")
    assert (got[..., 3] == 8).all()
    assert d < max(1e-4, 2.0 * d0)


# one one-sided emitter without a surface in the plane z = 0, its front (the side its geometric normal (v1 - v0) x (v2 - v0) = +z points to)
# towards +z, under a constant environment
CLOSED_FORM = """
Shape quad : InlineMesh { positions { -1,-1,0, 1,-1,0, 1,1,0, -1,1,0 } indices { 0,1,2, 0,2,3 }
  light : Diffuse { emission : Constant { v { 2, 3, 0.5 } } } }
Camera cam : Pinhole { fov { 40 } spp { 16 } film : Color { resolution { 16, 16 } } position { 0, 0, 5 } look_at { 0, 0, 0 } }
render { cameras { @cam } shapes { @quad }
  environment : Spherical { emission : Constant { v { 0.25, 0.5, 1.0 } } }
  integrator : MegaPath { depth { 4 } } }
"""
L_ENV, L_QUAD = np.float32([0.25, 0.5, 1.0]), np.float32([2.0, 3.0, 0.5])


def _ray(o, d, t_min=0.0, t_max=INF):
    return np.float32([*o, t_min, *d, t_max])


def test_closed_forms_bit_exact(renderer):
    renderer.upload(Scene.from_string(CLOSED_FORM))
    d_front = np.float32([0.1, -0.2, -1.0])
    d_front = d_front / np.float32(np.sqrt((d_front.astype(np.float64) ** 2).sum()))
    o_front = np.float32([0.1, 0.2, 3.0])
    rays = np.stack([
        _ray((0, 0, 3), (0, 0, 1)),                 # 0: away from everything
        _ray((5, 5, 3), (0, 0, -1)),                # 1: past the quad
        _ray((0.25, -0.5, 3), (0, 0, -1)),          # 2: the front, head on
        _ray(o_front, d_front),                     # 3: the front, obliquely
        _ray((0.25, -0.5, -3), (0, 0, 1)),          # 4: the back side
        _ray((0.25, -0.5, 3), (0, 0, -1), 0, 2.5),  # 5: t_max ends short of the quad
        _ray((0.25, -0.5, 3), (0, 0, -1), 3.5),     # 6: t_min starts behind it
    ])
    got = renderer.radiance(rays, spp=16, raw=True)
    env, quad, zero = [*(16 * L_ENV), 16.0], [*(16 * L_QUAD), 16.0], [0.0, 0.0, 0.0, 16.0]
    want = np.float32([env, env, quad, quad, zero, env, env])
    assert np.array_equal(got, want), got
    # directions need not be normalised: the same bits, and the interval is the caller's (in units of |d|)
    scaled = rays.copy()
    scaled[:, 4:7] *= np.float32(7.5)
    scaled[5, 7], scaled[6, 3] = 2.5 / 7.5, 3.5 / 7.5
    assert np.array_equal(renderer.radiance(scaled, spp=16, raw=True), want)
    means = renderer.radiance(rays, spp=16)
    assert means.shape == (7, 3) and np.array_equal(means, want[:, :3] / 16)
    # the clamp: per sample, on the largest component (ColorFilmInstance::_accumulate)
    clamped = renderer.radiance(rays[2:3], spp=16, raw=True, clamp=1.5)
    assert np.allclose(clamped[0], [*(16 * L_QUAD * np.float32(0.5)), 16.0], rtol=1e-6)


def _screened_rays():
    nan = np.float32(np.nan)
    return np.stack([
        _ray((nan, 0, 3), (0, 0, -1)), _ray((0, 0, 3), (0, nan, -1)), _ray((0, 0, 3), (0, 0, -1), nan), _ray((0, 0, 3), (0, 0, -1), 0, nan),
        _ray((INF, 0, 3), (0, 0, -1)), _ray((0, 0, 3), (0, -INF, -1)), _ray((0, 0, 3), (0, 0, -1), -INF), _ray((0, 0, 3), (0, 0, -1), INF, INF),
        _ray((0, 0, 3), (0, 0, 0)), _ray((0, 0, 3), (0, 0, -1), 1.0, 1.0), _ray((0, 0, 3), (0, 0, -1), 2.0, 1.0), _ray((0, 0, 3), (0, 0, -1), 0, -INF),
    ])


def test_screening_and_the_edges_of_a_batch(renderer):
    renderer.upload(Scene.from_string(CLOSED_FORM))
    bad = _screened_rays()
    good = _ray((0.25, -0.5, 3), (0, 0, -1))
    rays = np.concatenate([bad, good[None], bad])
    got = renderer.radiance(rays, spp=4, raw=True)
    hit = len(bad)
    assert (np.delete(got, hit, axis=0).view(np.uint32) == 0).all()  # (0, 0, 0, 0), to the bit
    assert np.array_equal(got[hit], np.float32([*(4 * L_QUAD), 4.0]))
    # under accumulate_into a screened ray's record is untouched
    acc = np.arange(len(rays) * 4, dtype=np.float32).reshape(-1, 4) + np.float32(0.5)
    before = acc.copy()
    assert renderer.radiance(rays, spp=4, raw=True, accumulate_into=acc) is acc
    assert np.array_equal(np.delete(acc, hit, axis=0), np.delete(before, hit, axis=0))
    assert np.array_equal(acc[hit], before[hit] + np.float32([*(4 * L_QUAD), 4.0]))
    # counts around a work item of 64 rays, with a sentinel behind the records
    for n in (0, 1, 63, 64, 65):
        batch = np.tile(good, (n, 1))
        buf = np.zeros(n * 4 + 4, np.float32)
        buf[n * 4:] = 12345.0
        out = renderer.radiance(batch, spp=2, raw=True, accumulate_into=buf[:n * 4].reshape(n, 4))
        assert out.shape == (n, 4) and (buf[n * 4:] == 12345.0).all(), n
        assert np.array_equal(out, np.tile(np.float32([*(2 * L_QUAD), 2.0]), (n, 1))), n
        assert renderer.radiance(batch, spp=2).shape == (n, 3)
        assert (renderer.last_radiance_ms() > 0.0) == (n > 0), n
    # no samples: nothing is launched, and a fresh result is zero
    none = renderer.radiance(np.tile(good, (65, 1)), spp=0, spp_begin=3, raw=True)
    assert renderer.last_radiance_ms() == 0.0 and (none.view(np.uint32) == 0).all()
    kept = renderer.radiance(rays, spp=0, raw=True, accumulate_into=acc.copy())
    assert renderer.last_radiance_ms() == 0.0 and np.array_equal(kept, acc)


def test_sentinel_behind_device_records(renderer):
    torch = pytest.importorskip("torch")
    renderer.upload(Scene.from_string(CLOSED_FORM))
    good = _ray((0.25, -0.5, 3), (0, 0, -1))
    for n in (1, 63, 64, 65):
        rays = torch.from_numpy(np.tile(good, (n, 1))).to("cuda:0")
        buf = torch.zeros(n * 4 + 64, dtype=torch.float32, device="cuda:0")
        buf[n * 4:] = 12345.0
        for spp in (2, 16):  # one chunk; 16 samples of so few rays are cut into several (the partial planes and their reduce)
            buf[:n * 4] = 0.0
            out = renderer.radiance(rays, spp=spp, raw=True, accumulate_into=buf[:n * 4].view(n, 4))
            assert out.data_ptr() == buf.data_ptr()
            host = buf.cpu().numpy()
            assert (host[n * 4:] == 12345.0).all(), (n, spp)
            assert np.array_equal(host[:n * 4].reshape(n, 4), np.tile(np.float32([*(spp * L_QUAD), spp]), (n, 1))), (n, spp)


def test_order_and_grouping(renderer, cornell128):
    case = cornell128
    renderer.upload(case.scene)
    rng = np.random.default_rng(7)
    streams = np.sort(rng.choice(128 * 128, 4096, replace=False)).astype(np.uint32)
    rays = np.ascontiguousarray(case.rays[3][streams])
    # one sample per call: a record is a function of (ray, stream, s, scene) only
    ref = renderer.radiance(rays, spp=1, spp_begin=3, streams=streams, raw=True)
    assert (ref[:, 3] == 1).all() and ref[:, :3].sum() > 0
    full = renderer.radiance(case.rays[3], spp=1, spp_begin=3, raw=True)  # streams = None: 0, 1, 2, ...
    assert np.array_equal(ref.view(np.uint32), full[streams].view(np.uint32))
    perm = rng.permutation(4096)
    shuffled = renderer.radiance(np.ascontiguousarray(rays[perm]), spp=1, spp_begin=3, streams=np.ascontiguousarray(streams[perm]), raw=True)
    assert np.array_equal(shuffled.view(np.uint32), ref[perm].view(np.uint32))
    for n in (1, 100, 1000):
        prefix = renderer.radiance(np.ascontiguousarray(rays[:n]), spp=1, spp_begin=3, streams=np.ascontiguousarray(streams[:n]), raw=True)
        assert np.array_equal(prefix.view(np.uint32), ref[:n].view(np.uint32)), n
    # several samples per call: the same call gives the same bits; sample ranges compose up to the order of float additions
    once = renderer.radiance(rays, spp=16, streams=streams, raw=True)
    again = renderer.radiance(rays, spp=16, streams=streams, raw=True)
    assert np.array_equal(once.view(np.uint32), again.view(np.uint32))
    split = renderer.radiance(rays, spp=8, streams=streams, raw=True)
    split = renderer.radiance(rays, spp=8, spp_begin=8, streams=streams, raw=True, accumulate_into=split)
    assert np.array_equal(split[:, 3], once[:, 3]) and (once[:, 3] == 16).all()
    assert _rel_l1(split, once) < 1e-6


def test_heavy_closure_scene(renderer, capsys):
    """A Disney and a Mix box: the out-of-line closures and the parking of heavy hits, at test_each_closure_in_a_cornell_box's bars"""
    from helpers import MATERIALS
    extra = MATERIALS["disney"].replace("Surface m ", "Surface disney ") + "\n" + MATERIALS["mix"].replace("Surface m ", "Surface mix ") + "\n"
    case = Case(cornell_box(resolution=64, spp=8, short_box_surface="disney", tall_box_surface="mix", extra_surfaces=extra), 8)
    got = case.query(renderer)
    rel = _rel_l1(got, case.film)
    bias = abs(got[..., :3].mean() - case.film[..., :3].mean()) / case.film[..., :3].mean()
    with capsys.disabled():
        print(f"\n[radiance] Disney + Mix boxes 64 x 64 x 8: rel-L1 {rel:.3e}, mean off by {bias:.3e}")
    assert (got[..., 3] == 8).all()
    assert rel < 3e-3
    assert bias < 1e-3


def test_nested_mix_and_layered_scene(renderer, capsys):
    """A Mix whose leaf is a Layered surface needs the kFeatNest query kernels.  A Layered surface seeds its random walk from the BITS of the hit
    point (test_gpu_parity.py::test_layered_closure), which the oracle's camera rays and the device's own do not share to the last bit, so
    against the film parity is statistical: a paired z-test over the 4096 pixels.  (The rays are the oracle's camera rays of each sample, one
    call per sample: one fixed ray per pixel would meet the surface in one point and repeat one walk in all its samples.)  d = (query - film) per pixel, summed over rgb, has mean zero if both estimate
    the same radiance, the pixels are independent, and the central limit theorem holds over 4096 of them (the film clamp bounds every
    sample): |mean d| < 5 standard errors, the standard error from d's own sample variance -- a bar from the estimator's noise as the test
    finds it, five standard deviations wide.  Exact: the sample counts, and the same call twice."""
    from helpers import MATERIALS
    spp = 16
    extra = MATERIALS["mix_layered"].replace("Surface m ", "Surface nested ") + "\n"
    scene = Scene.from_string(cornell_box(resolution=64, spp=spp, short_box_surface="nested", tall_box_surface="nested", extra_surfaces=extra))
    oracle = Oracle(scene)
    rays = [_camera_rays(oracle, s)[0] for s in range(spp)]
    oracle.close()
    renderer.upload(scene)
    renderer.set_wavefront(False)
    try:
        renderer.render(0, spp, sync=True)
        assert renderer.last_variant() & 512  # LRHIP_FEAT_NESTED: the scene does need it
        film = renderer.download(converted=False).reshape(-1, 4)
    finally:
        renderer.set_wavefront(True)
    got = None
    for s in range(spp):
        got = renderer.radiance(rays[s], spp=1, spp_begin=s, raw=True, accumulate_into=got)
    again = renderer.radiance(rays[0], spp=spp, raw=True)
    assert np.array_equal(again.view(np.uint32), renderer.radiance(rays[0], spp=spp, raw=True).view(np.uint32))
    d = (got[:, :3].astype(np.float64) - film[:, :3]).sum(axis=1) / spp
    z = float(d.mean() / (d.std(ddof=1) / np.sqrt(len(d))))
    with capsys.disabled():
        print(f"\n[radiance] Mix with a Layered leaf 64 x 64 x {spp}: frame mean query / film {got[:, :3].mean() / film[:, :3].mean():.4f}, z = {z:.2f}")
    assert (again[:, 3] == spp).all() and np.isfinite(again).all()
    assert (got[:, 3] == spp).all() and (film[:, 3] == spp).all() and np.isfinite(got).all() and (got[:, :3] >= 0).all()
    assert abs(z) < 5.0


def test_extreme_direction_lengths(renderer):
    """Any finite non-zero direction is a direction: denormal, or near FLT_MAX.  The closed-form rays of above with d scaled by powers of two
    (exact), the interval's ends scaled the other way where they stay in range."""
    renderer.upload(Scene.from_string(CLOSED_FORM))
    base = np.stack([
        _ray((0.25, -0.5, 3), (0, 0, -1)),          # the front of the emitter
        _ray((0.25, -0.5, -3), (0, 0, 1)),          # its back
        _ray((5, 5, 3), (0, 0, -1)),                # past it
        _ray((0.25, -0.5, 3), (0, 0, -1), 0, 2.5),  # t_max short of it
        _ray((0.25, -0.5, 3), (0, 0, -1), 3.5),     # t_min behind it
    ])
    env, quad, zero = [*(16 * L_ENV), 16.0], [*(16 * L_QUAD), 16.0], [0.0, 0.0, 0.0, 16.0]
    want = np.float32([quad, zero, env, env, env])
    assert np.array_equal(renderer.radiance(base, spp=16, raw=True), want)
    for exponent in (-140, -100, -30, 30, 100, 126):
        scale = np.float32(2.0) ** np.float32(exponent)
        rays = base.copy()
        rays[:, 4:7] *= scale
        assert np.isfinite(rays[:, 4:7]).all() and (np.abs(rays[:, 4:7]).max(axis=1) > 0).all()
        rays[3, 7] = np.float32(2.5) / scale if abs(exponent) <= 100 else (INF if exponent < 0 else 0.0)
        rays[4, 3] = np.float32(3.5) / scale if abs(exponent) <= 100 else (np.float32(3e38) if exponent < 0 else 0.0)
        got = renderer.radiance(rays, spp=16, raw=True)
        expect = want.copy()
        if exponent < -100:   # 2.5 / |d| is beyond the float range: t_max = +inf reaches the emitter; t_min = 3e38 |d| is still short of it
            expect[3], expect[4] = quad, quad
        elif exponent > 100:  # t_max = 0 is an empty interval: screened; t_min = 0 starts at the origin
            expect[3], expect[4] = [0.0, 0.0, 0.0, 0.0], quad
        assert np.array_equal(got, expect), (exponent, got)


def test_scene_without_lighting(renderer, cornell128):
    """Neither lights nor an environment: the reference renders nothing (mega_path.cpp:40-47; test_oracle_render.py::test_no_lights_renders_black:
    the film stays 0, n included), lrhip_render launches nothing, and neither does the query -- records of no sample."""
    text = cornell_box(resolution=128, spp=16).replace("light : Diffuse { emission : Constant { v { 17, 12, 4 } } }", "")
    dark = Scene.from_string(text)
    assert not dark.has_lighting
    rays = cornell128.rays[0]
    renderer.upload(dark)
    got = renderer.radiance(rays, spp=4, raw=True)
    assert renderer.last_radiance_ms() == 0.0 and (got.view(np.uint32) == 0).all()
    acc = np.arange(rays.shape[0] * 4, dtype=np.float32).reshape(-1, 4)
    kept = renderer.radiance(rays, spp=4, raw=True, accumulate_into=acc.copy())
    assert np.array_equal(kept, acc)
    torch = pytest.importorskip("torch")
    d_out = torch.full((rays.shape[0], 4), 7.0, dtype=torch.float32, device="cuda:0")
    d_rays = torch.from_numpy(rays).to("cuda:0")
    assert (renderer.radiance(d_rays, spp=4, raw=True).cpu().numpy().view(np.uint32) == 0).all()
    assert (renderer.radiance(d_rays, spp=4, raw=True, accumulate_into=d_out).cpu().numpy() == 7.0).all()
    renderer.render(0, 2, sync=True)
    assert (renderer.download(converted=False) == 0).all()
    # the context is as good as before
    renderer.upload(cornell128.scene)
    renderer.render(0, 2, sync=True)
    assert (renderer.download(converted=False)[..., 3] == 2).all()
    lit = renderer.radiance(rays, spp=1, raw=True)
    assert (lit[:, 3] == 1).all() and lit[:, :3].sum() > 0


def test_torch_path(renderer, cornell128):
    torch = pytest.importorskip("torch")
    case = cornell128
    renderer.upload(case.scene)
    streams = np.arange(1000, 1000 + 777, dtype=np.uint32)
    rays = np.ascontiguousarray(case.rays[0][streams])
    want = renderer.radiance(rays, spp=4, streams=streams, raw=True)
    d_rays = torch.from_numpy(rays).to("cuda:0")
    d_streams = torch.from_numpy(streams.astype(np.int32)).to("cuda:0")
    got = renderer.radiance(d_rays, spp=4, streams=d_streams, raw=True)
    assert isinstance(got, torch.Tensor) and got.device == d_rays.device and got.shape == (777, 4) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert renderer.last_radiance_ms() > 0.0
    means = renderer.radiance(d_rays, spp=4, streams=d_streams)
    assert isinstance(means, torch.Tensor) and means.shape == (777, 3)
    assert np.array_equal(means.cpu().numpy(), want[:, :3] / np.maximum(want[:, 3:4], np.float32(1)))
    more = renderer.radiance(d_rays, spp=4, spp_begin=4, streams=d_streams, raw=True, accumulate_into=got)
    assert more.data_ptr() == got.data_ptr() and (more[:, 3] == 8).all()
    with pytest.raises(ValueError):
        renderer.radiance(d_rays.cpu(), spp=1)
    with pytest.raises(ValueError):
        renderer.radiance(d_rays, spp=1, streams=d_streams.cpu())
    flat = torch.zeros(777 * 8 + 1, dtype=torch.float32, device="cuda:0")
    misaligned = flat[1:].view(777, 8)
    assert misaligned.is_contiguous() and misaligned.data_ptr() % 16 != 0
    with pytest.raises(ValueError):
        renderer.radiance(misaligned, spp=1)


def test_error_returns(cornell128):
    r = MegaPathRenderer(0)
    try:
        lib = r._lib
        rays = np.ascontiguousarray(cornell128.rays[0][64 * 128 + 32:64 * 128 + 96])  # the middle of the frame's middle row: every ray meets the box
        out = np.zeros((64, 4), np.float32)
        p = _ffi.RadianceQueryParams()
        p.rays, p.out, p.count, p.spp_begin, p.spp_end = rays.ctypes.data, out.ctypes.data, 64, 0, 1
        assert lib.lrhip_trace_radiance(r._ctx, C.byref(p)) == LRHIP_ERROR_INVALID  # before any upload
        r.upload(cornell128.scene)
        assert lib.lrhip_trace_radiance(r._ctx, C.byref(p)) == 0 and (out[:, 3] == 1).all()
        for change in (dict(rays=None), dict(out=None), dict(flags=16), dict(count=1 << 31), dict(clamp=-1.0), dict(clamp=float("nan"))):
            q = _ffi.RadianceQueryParams.from_buffer_copy(p)
            for k, v in change.items():
                setattr(q, k, v)
            assert lib.lrhip_trace_radiance(r._ctx, C.byref(q)) == LRHIP_ERROR_INVALID, change
        q = _ffi.RadianceQueryParams.from_buffer_copy(p)  # misaligned device pointers are refused before anything is read
        q.flags, q.rays = _ffi.RAY_DEVICE_POINTERS, 4096 + 8
        assert lib.lrhip_trace_radiance(r._ctx, C.byref(q)) == LRHIP_ERROR_INVALID
        aov = cornell_box(resolution=32, spp=4).replace("integrator : MegaPath {", "integrator : AOV {")
        direct = cornell_box(resolution=32, spp=4).replace("integrator : MegaPath {", "integrator : Direct {")
        for text in (aov, direct):
            r.upload(Scene.from_string(text))
            assert lib.lrhip_trace_radiance(r._ctx, C.byref(p)) == LRHIP_ERROR_UNSUPPORTED
            assert b"integrator" in lib.lrhip_last_error()
            with pytest.raises(DeviceError):
                r.radiance(rays)
        # the context is as good as before
        r.upload(cornell128.scene)
        r.render(0, 2, sync=True)
        assert (r.download(converted=False)[..., 3] == 2).all()
        assert np.asarray(r.trace(rays).hit).all()
        assert (r.radiance(rays, raw=True)[:, 3] == 1).all()
    finally:
        r.close()
