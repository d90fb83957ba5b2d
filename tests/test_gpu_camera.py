"""Camera, sampler and film queries on the device (include/lrhip.h: lrhip_query_sampler, lrhip_query_camera, lrhip_film_splat):
the sampler streams against the oracle's hook and the numpy restatement of the reference's samplers (tests/sampler_reference.py), the camera
rays against Oracle.camera_ray, the splat against a numpy restatement of ColorFilmInstance::_accumulate, malformed records and errors, the
torch path, and a whole render written as a loop over the queries against the oracle's film."""
import ctypes as C

import numpy as np
import pytest

import light_reference as L
import sampler_reference as R
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import MegaPathRenderer, RayHits
from luisarender_amd.scenes import cornell_box
from oracle.check import Oracle, oracle_lib

pytestmark = pytest.mark.gpu

LRHIP_ERROR_INVALID = -1
INVALID = 0xFFFFFFFF
W = H = 64
N = W * H
BIG = (1 << 20) + 65  # one record past the host staging chunk, and a ragged last wave
U = 2.0 ** -24        # unit roundoff of float32


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def words(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


def oracle_streams(view, streams, sample, n):
    """oracle_sampler_stream for stream ids (pixel (j mod W, j div W)), [len, 2 + n]"""
    lib = oracle_lib()
    return np.stack([R.oracle_stream(lib, view, j % W, (j // W) % H, sample, n) for j in streams])


# ---------------------------------------------------------------- 1. streams

STREAM_CASES = [("Independent", None, False), ("PCG32", None, False), ("Sobol", None, False), ("PaddedSobol", None, False),
                ("Independent", 8, False), ("PaddedSobol", 8, True)]


@pytest.mark.parametrize("sampler,tile,jitter", STREAM_CASES)
def test_sampler_streams(renderer, sampler, tile, jitter):
    """sampler_start + sampler_draw against oracle_sampler_stream (the pixel pair and 63 1-D draws) and against the numpy restatement (a mixed
    pattern with 2-D draws), bit for bit; one call against three; counts around a wave and past the host staging chunk; reversed streams;
    per-record sample indices; a stream carried past the Sobol sampler's 1024 dimensions."""
    scene = Scene.from_string(R.scene_text(sampler, tile, jitter, spp=8))
    view = scene.view()
    renderer.upload(scene)
    pattern = "p" + "1" * 63
    want = oracle_streams(view, range(65), 1, 63)
    for count in (1, 63, 64, 65):
        state = renderer.sampler_start(count=count, sample=1)
        assert state.shape == (count, 4) and state.dtype == np.uint32
        if sampler == "Independent":
            assert (state[:, 1:] == 0).all()
        u = renderer.sampler_draw(state, pattern)
        assert u.shape == (count, 65) and u.dtype == np.float32 and np.array_equal(words(u), words(want[:count])), count
    assert renderer.last_camera_ms() > 0.0
    # past the staging chunk: every stream of the frame, 256 times over, against the oracle's first three numbers
    state = renderer.sampler_start(count=BIG, sample=2)
    u = renderer.sampler_draw(state, "p1")
    frame = oracle_streams(view, range(N), 2, 1)
    assert np.array_equal(words(u), words(frame[np.arange(BIG) % N]))
    # a mixed pattern against the restatement; the same numbers in three calls with the state carried between them
    mixed = "p2" + "1212" * 3
    ref = R.Samplers(view)
    j = np.arange(N, dtype=np.uint32)
    ref.start(j % W, j // W, 1)
    want_mixed = ref.draw(mixed)
    state = renderer.sampler_start(count=N, sample=1)
    first = state.copy()
    u = renderer.sampler_draw(state, mixed)
    assert np.array_equal(words(u), words(want_mixed))
    assert not np.array_equal(state, first)  # the state moved, in place
    carried = first.copy()
    parts = [renderer.sampler_draw(carried, p) for p in ("p2", "1212", "12121212")]
    assert np.array_equal(words(np.concatenate(parts, axis=1)), words(u)) and np.array_equal(carried, state)
    # explicit streams in reversed order give the reversed rows; per-record indices equal per-call sample_index
    ids = np.arange(65, dtype=np.uint32)[::-1].copy()
    state = renderer.sampler_start(streams=ids, sample=1)
    assert np.array_equal(words(renderer.sampler_draw(state, pattern)), words(want[::-1]))
    state = renderer.sampler_start(indices=np.full(65, 1, np.uint32))
    assert np.array_equal(words(renderer.sampler_draw(state, pattern)), words(want))
    indices = (np.arange(65, dtype=np.uint32) % 3) * np.uint32(7)
    state = renderer.sampler_start(streams=ids, indices=indices)
    got = renderer.sampler_draw(state, "p1")
    for s in (0, 7, 14):
        rows = indices == s
        assert np.array_equal(words(got[rows]), words(oracle_streams(view, ids[rows], s, 1)))
    # 17 x 64 = 1088 draws behind the pixel pair: past dimension 1024, where the Sobol sampler wraps to dimension 2 as the oracle's does
    ids = np.array([0, 2077, N - 1], np.uint32)
    state = renderer.sampler_start(streams=ids, sample=7)
    long = np.concatenate([renderer.sampler_draw(state, "p")] + [renderer.sampler_draw(state, "1" * 64) for _ in range(17)], axis=1)
    assert np.array_equal(words(long), words(oracle_streams(view, ids, 7, 17 * 64)))


# ---------------------------------------------------------------- 2. camera rays

def camera_text(camera: str, filter_impl: str, radius: float, sampler: str = "Independent", **kwargs) -> str:
    text = cornell_box(resolution=W, sampler=sampler, filter_impl=filter_impl, filter_radius=radius, **kwargs)
    head = "Camera cam : Pinhole {"
    assert head in text
    if camera == "thin_lens":
        return text.replace(head, "Camera cam : ThinLens {\n  aperture { 1.4 } focal_length { 50 } focus_distance { 900 }")
    if camera == "ortho":
        return text.replace(head, "Camera cam : Ortho {\n  zoom { 8 }")
    if camera == "pinhole_clip":
        return text.replace(head, head + "\n  clip { 700, 1300 }")
    return text


CAMERA_CASES = [("pinhole_clip", "Box", 0.5), ("thin_lens", "Gaussian", 1.5), ("ortho", "Mitchell", 2.0)]


# MEASURED on the MI355X: the largest difference between a thin-lens direction and the oracle's, over 2 x 4096 camera samples; every
# other field of every camera is bit-identical.  The test asserts twice this value
MEASURED_THIN_LENS_DIRECTION = 2.3283064365386963e-10  # (2 of 8192 directions, one last bit of a small component; sample 0: none)


@pytest.mark.parametrize("camera,filter_impl,radius", CAMERA_CASES)
def test_camera_rays_against_the_oracle(renderer, capsys, camera, filter_impl, radius):
    """camera_samples(s) over all 4096 pixels at s = 0, 1 against Oracle.camera_ray: origin, direction and weight bit for bit (the unit is built
    with the oracle's arithmetic and makes the renderers' own calls) -- but for the thin lens' directions, held to twice the measured difference;
    t_min, t_max against clip / cos; the film position within the filter's radius; the weights of a Mitchell filter negative in its lobes, as
    oracle_filter_sample has them for the same numbers."""
    scene = Scene.from_string(camera_text(camera, filter_impl, radius, spp=8))
    view = scene.view()
    cam = view.camera
    assert int(cam.kind) == {"pinhole_clip": 0, "thin_lens": 1, "ortho": 2}[camera]
    if camera == "pinhole_clip":
        assert (float(cam.clip_near), float(cam.clip_far)) == (700.0, 1300.0)
    renderer.upload(scene)
    oracle = Oracle(scene)
    lib = oracle_lib()
    m = np.array(list(cam.camera_to_world), np.float64).reshape(4, 4).T  # row-major
    front = -m[:3, 2] / np.linalg.norm(m[:3, 2])
    centre = np.stack([np.arange(N) % W + 0.5, np.arange(N) // W + 0.5], axis=1).astype(np.float32)
    negative = 0
    for sample in (0, 1):
        got, state = renderer.camera_samples(sample)
        want = np.stack([oracle.camera_ray(i % W, i // W, sample) for i in range(N)])
        assert np.asarray(got.valid).all() and np.array_equal(got.pixel, np.arange(N, dtype=np.uint32))
        assert np.array_equal(words(got.rays[:, 0:3]), words(want[:, 0:3])), "origin"
        assert np.array_equal(words(got.weight), words(want[:, 6])), "weight"
        if camera == "thin_lens":
            # the lens point goes through the device's sincos_small (dev_bsdf.h: sample_disk_concentric, a 1-ulp polynomial, the renderers'
            # own) and through libm's sin / cos in the oracle: a last bit of the point can round a component of the direction the other way
            err = float(np.abs(got.rays[:, 4:7].astype(np.float64) - want[:, 3:6]).max())
            with capsys.disabled():
                print(f"\n[camera] thin lens, sample {sample}: directions differ from the oracle's by at most {err:.3e}", end="")
            assert MEASURED_THIN_LENS_DIRECTION is not None, "not measured yet"
            assert err <= 2.0 * MEASURED_THIN_LENS_DIRECTION
        else:
            assert np.array_equal(words(got.rays[:, 4:7]), words(want[:, 3:6])), "direction"
        # the clip planes over the cosine to the axis (camera.h:147-157).  The kernel takes the cosine of the camera-space direction in fp32, the
        # test of the world-space one in fp64: the fp32 rotation, two normalisations, the dot product and the division are below ten roundings
        cos = got.rays[:, 4:7].astype(np.float64) @ front
        assert (cos > 0.5).all()
        for column, clip in ((3, float(cam.clip_near)), (7, float(cam.clip_far))):
            assert np.abs(got.rays[:, column] * cos / clip - 1.0).max() <= 10 * U if clip != 0.0 else (got.rays[:, column] == 0).all()
        if camera == "ortho":
            assert (got.rays[:, 3] == cam.clip_near).all() and (got.rays[:, 7] == cam.clip_far).all()
        # the film position: pixel + 0.5 + the filter's offset, within its radius; the same numbers through the oracle's filter
        assert np.abs(got.film_xy - centre).max() <= radius
        state = renderer.sampler_start(count=N, sample=sample)
        u = renderer.sampler_draw(state, "p")
        rows = np.flatnonzero(got.weight < 0)[:64] if filter_impl == "Mitchell" else np.arange(0, N, 61)
        for i in rows:
            fs = np.zeros(3, np.float32)
            lib.oracle_filter_sample(C.byref(view.filter), float(u[i, 0]), float(u[i, 1]), fs.ctypes.data)
            assert words(fs[2]) == words(got.weight[i]) and np.array_equal(words(centre[i] + fs[0:2]), words(got.film_xy[i]))
        negative += int((got.weight < 0).sum())
        if filter_impl == "Box":
            assert (got.weight == 1.0).all()
    assert (negative > 0) == (filter_impl == "Mitchell")
    oracle.close()


# ---------------------------------------------------------------- 3. splat

def accumulate(film, pixels, values, clamp):
    """ColorFilmInstance::_accumulate (src/films/color.cpp:107-130, effective spp 1) record by record, in float32: film is [N, 4], in place"""
    clamp = np.float32(clamp)
    for p, v in zip(pixels, values[:, :3]):
        if p >= film.shape[0] or np.isnan(v).any() or np.isinf(v).any():
            continue
        strength = max(np.abs(v).max(), np.float32(0))
        c = v * (clamp / max(strength, clamp))
        if (c != 0).any():
            film[p, :3] += c
        film[p, 3] += np.float32(1)
    return film


def splat_values(rng, n, clamp):
    v = rng.uniform(-2.0, 6.0, (n, 4)).astype(np.float32)  # negative values are added like any other
    v[:, 3] = np.nan  # the fourth column is ignored
    v[5, 0], v[70, 1], v[700, 2] = np.nan, np.inf, -np.inf
    v[9] = (4 * clamp, clamp, -2 * clamp, 0)
    v[11] = (0.5 * clamp, -8 * clamp, clamp, 0)
    v[13, :3] = 0.0  # counted, nothing added
    return v


def test_film_splat(renderer):
    """film_splat against the numpy restatement of _accumulate: distinct pixels (identity, a permutation) bit for bit; NaN, +Inf and -Inf
    rejected with n unchanged; values above the clamp scaled by their largest component; the clamp override; negative values; pixel ids W * H
    and 0xffffffff skipped; every pixel named three times; a bound film; a splat in front of a render."""
    torch = pytest.importorskip("torch")
    scene = Scene.from_string(cornell_box(resolution=W, spp=2, depth=3, rr_depth=4))
    clamp = float(scene.view().film.clamp)
    assert 0.0 < clamp < 1e30
    renderer.upload(scene)
    rng = np.random.default_rng(16)
    v = splat_values(rng, N, clamp)
    raw = lambda: renderer.download(converted=False).reshape(N, 4)  # noqa: E731
    # identity
    renderer.film_splat(v)
    want = accumulate(np.zeros((N, 4), np.float32), range(N), v, clamp)
    got = raw()
    assert np.array_equal(words(got), words(want))
    assert got[5, 3] == 0 and got[70, 3] == 0 and got[700, 3] == 0 and (got[[5, 70, 700], :3] == 0).all() and got[13].tolist() == [0, 0, 0, 1]
    assert np.abs(got[9, :3]).max() == np.float32(clamp) and np.abs(got[11, :3]).max() == np.float32(clamp) and (got[:, :3] < 0).any()
    # a permutation on top, [N, 3] values, with the ids W * H and 0xffffffff among them
    perm = rng.permutation(N).astype(np.uint32)
    ids = np.concatenate([perm, np.array([N, INVALID], np.uint32)])
    v3 = np.concatenate([np.ascontiguousarray(v[:, :3]), np.ones((2, 3), np.float32)])
    renderer.film_splat(v3, ids)
    want = accumulate(want, ids, v3, clamp)
    assert np.array_equal(words(raw()), words(want))
    # the clamp override
    renderer.clear()
    renderer.film_splat(v, clamp=1.5)
    want = accumulate(np.zeros((N, 4), np.float32), range(N), v, 1.5)
    got = raw()
    assert np.array_equal(words(got), words(want)) and 1.49 < np.abs(got[:, :3]).max() <= 1.5 * (1 + 2 * U)  # (a product and a quotient round)
    # every pixel three times in one call: float atomics in no fixed order.  The film starts at 0, so a pixel's sum takes two rounded additions
    # of partial sums no larger than sum |c| (1 + u): within 3 u sum |c| of the exact sum, whatever the order; n = 3 exactly
    renderer.clear()
    ids = np.concatenate([rng.permutation(N), rng.permutation(N), rng.permutation(N)]).astype(np.uint32)
    v9 = rng.uniform(-2.0, 6.0, (3 * N, 4)).astype(np.float32)
    renderer.film_splat(v9, ids)
    got = raw()
    exact, total = np.zeros((N, 3)), np.zeros((N, 3))
    np.add.at(exact, ids, v9[:, :3].astype(np.float64))
    np.add.at(total, ids, np.abs(v9[:, :3]).astype(np.float64))
    assert np.abs(v9[:, :3]).max() < clamp and (got[:, 3] == 3).all()
    assert (np.abs(got[:, :3] - exact) <= 3 * U * total).all()
    # a bound film takes the splat; the context's own stays as it was
    own = raw()
    bound = torch.zeros((N, 4), dtype=torch.float32, device="cuda:0")
    renderer.bind_film(bound.data_ptr())
    try:
        renderer.film_splat(v)
        renderer.synchronize()
        assert np.array_equal(words(bound.cpu().numpy()), words(accumulate(np.zeros((N, 4), np.float32), range(N), v, clamp)))
    finally:
        renderer.bind_film(None)
    assert np.array_equal(words(raw()), words(own))
    # a splat in front of a render: the film holds both.  The render adds a pixel's two samples to what the film holds; against the sum of the
    # two films taken apart that is a handful of additions in another order
    renderer.clear()
    renderer.render(0, 2, sync=True)
    rendered = raw()
    renderer.clear()
    small = np.abs(rng.uniform(0.0, 1.0, (N, 4))).astype(np.float32)
    renderer.film_splat(small)
    renderer.render(0, 2)
    got = raw()
    assert (got[:, 3] == 3).all() and (rendered[:, 3] == 2).all()
    assert (np.abs(got[:, :3] - (small[:, :3].astype(np.float64) + rendered[:, :3])) <= 4 * U * (small[:, :3] + rendered[:, :3])).all()
    renderer.clear()


# ---------------------------------------------------------------- 4. edges and errors

def test_invalid_records_and_count_zero(renderer):
    scene = Scene.from_string(camera_text("thin_lens", "Box", 0.5, spp=2))
    renderer.upload(scene)
    rng = np.random.default_rng(4)
    u = rng.uniform(0, 1, (70, 4)).astype(np.float32)
    ids = rng.integers(0, N, 70).astype(np.uint32)
    good = renderer.camera_rays(u, ids)
    assert np.asarray(good.valid).all() and np.array_equal(good.pixel, ids)
    bad_u, bad_ids = u.copy(), ids.copy()
    bad_ids[3], bad_ids[64] = N, INVALID
    bad_u[7, 0], bad_u[20, 1], bad_u[33, 2], bad_u[69, 3] = np.nan, np.inf, -np.inf, np.nan  # (a thin lens looks at its lens pair)
    spoiled = np.zeros(70, bool)
    spoiled[[3, 64, 7, 20, 33, 69]] = True
    got = renderer.camera_rays(bad_u, bad_ids)
    assert np.array_equal(np.asarray(got.valid), ~spoiled)
    assert (words(got.rays[spoiled]) == 0).all() and (words(got.buffer[spoiled])[:, :3] == 0).all() and (got.pixel[spoiled] == INVALID).all()
    assert np.array_equal(words(got.rays[~spoiled]), words(good.rays[~spoiled])) and np.array_equal(words(got.buffer[~spoiled]), words(good.buffer[~spoiled]))
    assert not np.asarray(renderer.trace(got.rays).hit)[spoiled].any()  # the ray queries screen the zero ray
    # the same records anywhere in a batch: position independence
    order = rng.permutation(70)
    again = renderer.camera_rays(np.ascontiguousarray(u[order]), np.ascontiguousarray(ids[order]))
    assert np.array_equal(words(again.rays), words(good.rays[order])) and np.array_equal(words(again.buffer), words(good.buffer[order]))
    # a pinhole does not look at the lens pair
    renderer.upload(Scene.from_string(camera_text("pinhole", "Box", 0.5, spp=2)))
    lens_nan = u.copy()
    lens_nan[:, 2:] = np.nan
    assert np.array_equal(words(renderer.camera_rays(lens_nan, ids).rays), words(renderer.camera_rays(np.ascontiguousarray(u[:, :2]), ids).rays))
    # a damaged state never faults: every word of it set
    for sampler in ("Sobol", "PaddedSobol", "PCG32"):
        renderer.upload(Scene.from_string(R.scene_text(sampler, spp=6)))  # (a permutation length that is no power of two)
        state = np.full((65, 4), INVALID, np.uint32)
        numbers = renderer.sampler_draw(state, "p21")
        assert np.isfinite(numbers).all() and ((numbers >= 0) & (numbers < 1)).all()
    # count = 0 launches nothing
    assert renderer.sampler_start(count=0).shape == (0, 4)
    assert renderer.sampler_draw(np.zeros((0, 4), np.uint32), "p21").shape == (0, 5)
    empty = renderer.camera_rays(np.zeros((0, 4), np.float32))
    assert empty.rays.shape == (0, 8) and empty.buffer.shape == (0, 4)
    renderer.film_splat(np.zeros((0, 4), np.float32))
    assert renderer.last_camera_ms() == 0.0


def test_errors_and_sentinels(renderer):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    lib = renderer._lib
    pattern = (C.c_uint32 * 4)(_ffi.DRAW_PIXEL_2D, _ffi.DRAW_2D, _ffi.DRAW_1D, _ffi.DRAW_1D)
    host = {"state": np.zeros((4, 4), np.uint32), "streams": np.arange(4, dtype=np.uint32), "indices": np.zeros(4, np.uint32),
            "numbers": np.zeros((4, 6), np.float32), "u": np.full((4, 4), 0.25, np.float32), "rays": np.zeros((4, 8), np.float32),
            "samples": np.zeros((4, 4), np.float32), "values": np.ones((4, 4), np.float32)}
    at = {k: v.ctypes.data for k, v in host.items()}

    def sampler(ctx, where=at, **fields):
        p = _ffi.SamplerQueryParams()
        p.state, p.streams, p.indices, p.out, p.count = where["state"], where["streams"], where["indices"], where["numbers"], 4
        p.pattern, p.pattern_count, p.flags = C.cast(pattern, C.c_void_p), 4, _ffi.SAMPLER_START
        for field, value in fields.items():
            setattr(p, field, value)
        return lib.lrhip_query_sampler(ctx, C.byref(p)), lib.lrhip_last_error().decode()

    def camera(ctx, where=at, **fields):
        p = _ffi.CameraQueryParams()
        p.pixels, p.u, p.out_rays, p.out, p.count = where["streams"], where["u"], where["rays"], where["samples"], 4
        for field, value in fields.items():
            setattr(p, field, value)
        return lib.lrhip_query_camera(ctx, C.byref(p)), lib.lrhip_last_error().decode()

    def splat(ctx, where=at, **fields):
        p = _ffi.FilmSplatParams()
        p.pixels, p.values, p.count = where["streams"], where["values"], 4
        for field, value in fields.items():
            setattr(p, field, value)
        return lib.lrhip_film_splat(ctx, C.byref(p)), lib.lrhip_last_error().decode()

    fresh = MegaPathRenderer(0)
    try:
        for call in (sampler, camera, splat):
            rc, text = call(fresh._ctx)
            assert rc == LRHIP_ERROR_INVALID and "no scene uploaded" in text
        assert fresh.last_camera_ms() == 0.0
    finally:
        fresh.close()
    renderer.upload(Scene.from_string(cornell_box(resolution=W, spp=2)))
    renderer.clear()
    ctx = renderer._ctx
    assert sampler(ctx)[0] == 0 and camera(ctx)[0] == 0 and splat(ctx)[0] == 0
    assert sampler(ctx, streams=None, indices=None)[0] == 0 and camera(ctx, pixels=None)[0] == 0 and splat(ctx, pixels=None)[0] == 0
    assert sampler(ctx, flags=0, streams=None, indices=None)[0] == 0  # without the flag, streams and indices are not read
    assert sampler(ctx, pattern_count=0, out=None, pattern=None)[0] == 0  # an empty pattern only makes states: no out
    unknown = (C.c_uint32 * 4)(0, 1, 3, 0)
    for call, cases in ((sampler, (dict(state=None), dict(out=None), dict(pattern=None), dict(flags=2), dict(flags=64 | 128), dict(flags=256),
                                   dict(pattern=C.cast(unknown, C.c_void_p)), dict(pattern_count=65), dict(count=0x80000000))),
                        (camera, (dict(u=None), dict(out_rays=None), dict(out=None), dict(flags=2), dict(flags=128), dict(count=0x80000000),
                                  dict(pixels=None, count=N + 1))),
                        (splat, (dict(values=None), dict(flags=4), dict(flags=128), dict(clamp=-1.0), dict(clamp=float("nan")), dict(count=0x80000000),
                                 dict(pixels=None, count=N + 1)))):
        for fields in cases:
            rc, text = call(ctx, **fields)
            assert rc == LRHIP_ERROR_INVALID and call.__name__ in text, (call.__name__, fields)
    # count 0 launches nothing, whatever the pointers
    assert sampler(ctx, state=None, streams=None, indices=None, out=None, count=0)[0] == 0
    assert camera(ctx, pixels=None, u=None, out_rays=None, out=None, count=0)[0] == 0 and splat(ctx, pixels=None, values=None, count=0)[0] == 0
    # misaligned device pointers: refused before anything is read (the addresses lie inside live allocations all the same)
    widths = {"state": (4, torch.int32), "streams": (1, torch.int32), "indices": (1, torch.int32), "numbers": (6, torch.float32),
              "u": (4, torch.float32), "rays": (8, torch.float32), "samples": (4, torch.float32), "values": (4, torch.float32)}
    for count in (1, 63, 64, 65):  # a sentinel row behind every device output stays intact
        d = {k: torch.zeros((count + 2, w), dtype=t, device="cuda:0") for k, (w, t) in widths.items()}
        dev = {k: v.data_ptr() for k, v in d.items()}
        assert all(a % 16 == 0 for a in dev.values())
        if count == 1:
            for call, field, key, step in ((sampler, "state", "state", 4), (sampler, "out", "numbers", 4), (sampler, "streams", "streams", 2),
                                           (sampler, "indices", "indices", 1), (camera, "u", "u", 8), (camera, "out_rays", "rays", 4),
                                           (camera, "out", "samples", 4), (camera, "pixels", "streams", 2), (splat, "values", "values", 4),
                                           (splat, "pixels", "streams", 1)):
                flags = _ffi.RAY_DEVICE_POINTERS | (_ffi.SAMPLER_START if call is sampler else 0)
                rc, text = call(ctx, dev, **{"flags": flags, field: dev[key] + step})
                assert rc == LRHIP_ERROR_INVALID and "aligned" in text, (call.__name__, field)
        d["u"][:] = 0.25
        d["streams"][:, 0] = torch.arange(count + 2, dtype=torch.int32, device="cuda:0")
        for key in ("state", "numbers", "rays", "samples"):
            d[key][:] = 77
        rc, _ = sampler(ctx, dev, count=count, flags=_ffi.RAY_DEVICE_POINTERS | _ffi.SAMPLER_START)
        assert rc == 0
        rc, _ = camera(ctx, dev, count=count, flags=_ffi.RAY_DEVICE_POINTERS)
        assert rc == 0
        renderer.synchronize()
        for key in ("state", "numbers", "rays", "samples"):
            assert bool((d[key][count:] == 77).all()), (count, key)
            assert not bool((d[key][:count] == 77).all(dim=1).any()), (count, key)
        assert bool((d["samples"][:count].view(torch.int32)[:, 3] == d["streams"][:count, 0]).all())
    renderer.clear()


# ---------------------------------------------------------------- 5. the torch path

def test_device_tensors_equal_host_arrays(renderer):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    scene = Scene.from_string(camera_text("thin_lens", "Gaussian", 1.5, sampler="PaddedSobol", spp=4))
    renderer.upload(scene)
    rng = np.random.default_rng(5)
    ids = rng.permutation(N)[:1000].astype(np.uint32)
    h_state = renderer.sampler_start(streams=ids, sample=3)
    h_first = h_state.copy()
    h_u = renderer.sampler_draw(h_state, "p2")
    h_cam = renderer.camera_rays(h_u, ids)
    h_hits = renderer.trace(h_cam.rays)
    h_next = renderer.sampler_draw(h_state, "1212")
    d_ids = torch.from_numpy(ids.view(np.int32)).to("cuda:0")
    d_state = renderer.sampler_start(streams=d_ids, sample=3)
    assert d_state.is_cuda and d_state.dtype == torch.int32 and np.array_equal(d_state.cpu().numpy().view(np.uint32), h_first)
    address = d_state.data_ptr()
    d_u = renderer.sampler_draw(d_state, "p2")
    assert d_u.is_cuda and d_state.data_ptr() == address and np.array_equal(words(d_u.cpu().numpy()), words(h_u))  # the state moved in place
    d_cam = renderer.camera_rays(d_u, d_ids)
    assert d_cam.rays.is_cuda and d_cam.pixel.dtype == torch.int32 and bool(d_cam.valid.all())
    assert np.array_equal(words(d_cam.rays.cpu().numpy()), words(h_cam.rays)) and np.array_equal(words(d_cam.buffer.cpu().numpy()), words(h_cam.buffer))
    # start -> draw -> camera rays -> trace -> draw on the context's stream without a host round trip, then ONE synchronise
    torch.cuda.current_stream().synchronize()
    c_state = renderer.sampler_start(streams=d_ids, sample=3, sync=False)
    c_cam = renderer.camera_rays(renderer.sampler_draw(c_state, "p2", sync=False), d_ids, sync=False)
    c_hits = renderer.trace(c_cam.rays, sync=False)
    c_next = renderer.sampler_draw(c_state, "1212", sync=False)
    renderer.synchronize()
    assert np.array_equal(words(c_hits.buffer.cpu().numpy()), words(h_hits.buffer)) and np.array_equal(words(c_next.cpu().numpy()), words(h_next))
    assert np.array_equal(c_state.cpu().numpy().view(np.uint32), h_state)
    # on_device: no array fixes the kind
    cam, state = renderer.camera_samples(1, on_device=True)
    host_cam, host_state = renderer.camera_samples(1)
    assert cam.rays.is_cuda and state.is_cuda and np.array_equal(words(cam.rays.cpu().numpy()), words(host_cam.rays))
    assert np.array_equal(state.cpu().numpy().view(np.uint32), host_state)
    # the splat from the device equals the splat from the host
    values = rng.uniform(0, 2, (N, 4)).astype(np.float32)
    renderer.clear()
    renderer.film_splat(values)
    want = renderer.download(converted=False)
    renderer.clear()
    renderer.film_splat(torch.from_numpy(values).to("cuda:0"))
    assert np.array_equal(words(renderer.download(converted=False)), words(want))
    renderer.clear()
    for bad in (dict(streams=d_ids, indices=ids), dict(streams=d_ids.long()), dict(streams=d_ids.cpu())):
        with pytest.raises(ValueError):
            renderer.sampler_start(**bad)
    with pytest.raises(ValueError):
        renderer.camera_rays(d_u, ids)
    with pytest.raises(ValueError):
        renderer.film_splat(torch.from_numpy(values).to("cuda:0"), ids)


# ---------------------------------------------------------------- 6. a render written as a loop over the queries

def balance(f, g):
    total = f + g
    with np.errstate(all="ignore"):
        return np.where(total == 0, np.float32(0), f / total).astype(np.float32)


RENDER_CASES = [("pinhole", "Box", 0.5, "Independent"), ("thin_lens", "Gaussian", 1.5, "PaddedSobol")]


@pytest.mark.parametrize("camera,filter_impl,radius,sampler", RENDER_CASES)
def test_a_render_is_a_loop_over_the_queries(renderer, capsys, camera, filter_impl, radius, sampler):
    """lrhip_render written as tests/test_gpu_light.py::test_queries_compose_into_li's loop with camera_samples, sampler_draw(state, "1212") per
    vertex for the paths still alive and film_splat(weight x Li) in place of the oracle's hooks and the numpy sum: the Cornell box 64 x 64 at depth
    3 without Russian roulette, 2 spp, against the oracle's film.  Bar: rel-L1 <= max(1e-4, 2 d0), d0 = what lrhip_render's film (the parent
    commit's code) is away from the same oracle film; every pixel's n is 2.

    MEASURED on the MI355X: see DESIGN §4.16."""
    scene = Scene.from_string(camera_text(camera, filter_impl, radius, sampler=sampler, spp=2, depth=3, rr_depth=4))
    view = scene.view()
    depth = 3
    assert int(view.integrator.max_depth) == depth and int(view.integrator.rr_depth) > depth and int(view.sampler.spp) == 2
    t = L.light_tables(scene)
    want, _ = Oracle(scene).render(0, 2)
    want = want.reshape(N, 4)
    renderer.upload(scene)
    renderer.render(0, 2, sync=True)
    d0_film = renderer.download(converted=False).reshape(N, 4)
    renderer.clear()
    for sample in range(2):
        cam, state = renderer.camera_samples(sample)
        assert np.asarray(cam.valid).all()
        rays = cam.rays
        li, beta, pdf_bsdf = np.zeros((N, 3), np.float32), np.repeat(cam.weight[:, None], 3, axis=1), np.full(N, 1e16, np.float32)
        idx = np.arange(N)  # the paths still alive; rays, state, beta[idx], pdf_bsdf[idx] are theirs
        for vertex in range(depth):
            hits = renderer.trace(rays)
            found = renderer.light_evaluate(hits, rays)  # an emitter, the environment, or nothing
            assert np.asarray(found.valid).all()
            li[idx] += beta[idx] * found.L * balance(pdf_bsdf[idx], found.pdf)[:, None]
            sp = renderer.surface(hits, rays)
            go = np.asarray(hits.hit) & np.asarray(sp.has_surface)
            idx, rays, hits, sp = idx[go], np.ascontiguousarray(rays[go]), RayHits(np.ascontiguousarray(hits.buffer[go])), sp.buffer[go]
            state = np.ascontiguousarray(state[go])
            u = renderer.sampler_draw(state, "1212")  # light selection, light surface, lobe, BSDF (megapath_kernel.h)
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
            idx, rays, state = idx[go], np.ascontiguousarray(nxt[go]), np.ascontiguousarray(state[go])
        renderer.film_splat(li)  # (the camera weight is in beta from the start; one shutter sample: weight 1)
    got = renderer.download(converted=False).reshape(N, 4)
    renderer.clear()
    rel = lambda a: float(np.abs(a[:, :3] - want[:, :3]).sum() / np.abs(want[:, :3]).sum())  # noqa: E731
    d0, d = rel(d0_film), rel(got)
    with capsys.disabled():
        print(f"\n[camera] a render as a loop over the queries, {camera} / {filter_impl} / {sampler}, cornell 64 x 64 x 2 at depth 3: "
              f"d0 (lrhip_render) {d0:.3e}, composed {d:.3e}", end="")
    assert np.abs(want[:, :3]).sum() > 100 and np.isfinite(got).all()
    assert (want[:, 3] == 2).all() and (got[:, 3] == 2).all()
    assert d <= max(1e-4, 2.0 * d0)
