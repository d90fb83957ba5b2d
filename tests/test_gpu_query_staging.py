"""The one staged-call routine of the queries (lrhip_query.hip: staged_call) on a real MI355X: every query that takes host pointers,
over a batch of 2^20 + 65 records -- one full staging chunk and a ragged second one --, must give every record the bits it has in a small
batch, and the bits the same big batch gets through device pointers (one launch, no staging).  The ray and camera queries have such a case
in their own files; the inputs here are those files' small batches, tiled."""
import numpy as np
import pytest

import bsdf_reference as B
import instance_scene as S
import light_reference as L
import raycast_reference as RR
from luisarender_amd import Scene
from luisarender_amd.render import MegaPathRenderer
from luisarender_amd.scenes import cornell_box
from oracle.check import Oracle
from test_gpu_radiance import _camera_rays

pytestmark = pytest.mark.gpu

COUNT = (1 << 20) + 65


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    return torch


def tiled(a) -> np.ndarray:
    """the small batch's rows, repeated up to COUNT"""
    copies = -(-COUNT // len(a))
    return np.ascontiguousarray(np.tile(a, (copies,) + (1,) * (a.ndim - 1))[:COUNT])


def words(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


def on_device(torch, a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def check_staged(torch, call, last_ms, small: dict, tiles: bool = True) -> tuple:
    """call(**arrays) -> the result arrays.  The host-pointer call over the tiled inputs against the tiled results of the small batch
    (`tiles`) and against the device-pointer call over the same tiled inputs, word for word; and the host call's kernel time.  Returns the
    small batch's and the host call's results"""
    assert all(len(a) < (1 << 20) for a in small.values())
    small_results = call(**small)
    big = {name: tiled(a) for name, a in small.items()}
    host = call(**big)
    assert last_ms() > 0.0
    device = call(**{name: on_device(torch, a) for name, a in big.items()})
    assert len(host) == len(device) == len(small_results)
    for s, h, d in zip(small_results, host, device):
        assert len(h) == COUNT
        if tiles:
            assert np.array_equal(words(h), words(tiled(np.asarray(s))))
        assert np.array_equal(words(h), words(d.cpu().numpy()))
    return small_results, host


@pytest.mark.parametrize("geometry_only", [False, True], ids=["full", "geometry_only"])
def test_surface(renderer, torch, geometry_only):
    scene = S.room()
    rays = RR.make_rays(scene)
    renderer.upload(scene)
    hits = renderer.trace(rays).buffer
    check_staged(torch, lambda hits, rays: [renderer.surface(hits, rays, geometry_only=geometry_only).buffer], renderer.last_surface_ms,
                 {"hits": hits, "rays": rays})


@pytest.mark.parametrize("mode", ["evaluate", "sample"])
def test_bsdf(renderer, torch, mode):
    name = "disney"
    inp, rays = B.inputs(name), B.rays(name)
    renderer.upload(Scene.from_string(B.scene_text(name)))
    hits = renderer.trace(rays).buffer
    if mode == "evaluate":
        call = lambda hits, rays, dirs: [renderer.bsdf_evaluate(hits, dirs, rays).buffer]  # noqa: E731
    else:
        call = lambda hits, rays, dirs: [renderer.bsdf_sample(hits, dirs, rays).buffer]  # noqa: E731
    dirs = inp["wi"] if mode == "evaluate" else inp["u"]
    dirs = np.ascontiguousarray(np.concatenate([dirs, np.zeros((len(dirs), 4 - dirs.shape[1]), np.float32)], axis=1))
    check_staged(torch, call, renderer.last_bsdf_ms, {"hits": hits, "rays": rays, "dirs": dirs})


@pytest.mark.parametrize("mode", ["sample_from_hits", "sample_from_points", "evaluate"])
def test_light(renderer, torch, mode):
    inp = L.inputs()
    renderer.upload(Scene.from_string(L.fan_scene()))
    hits = renderer.trace(inp["rays"])
    u = np.ascontiguousarray(np.concatenate([inp["u"], np.zeros((len(inp["u"]), 4 - inp["u"].shape[1]), np.float32)], axis=1))

    def sample(**arrays):
        s = renderer.light_sample(**arrays)
        return [s.rays, s.buffer]

    if mode == "sample_from_hits":
        check_staged(torch, sample, renderer.last_light_ms, {"hits": hits.buffer, "u": u})
    elif mode == "sample_from_points":
        p = renderer.surface(hits).p
        points = np.ascontiguousarray(np.concatenate([p, np.zeros((len(p), 1), np.float32)], axis=1))
        check_staged(torch, sample, renderer.last_light_ms, {"points": points, "u": u})
    else:  # what the sampled shadow rays find at their ends: an emitter, the environment or nothing
        shadow = np.ascontiguousarray(renderer.light_sample(hits, u).rays)
        shadow[:, 7] = np.float32(np.inf)
        found = renderer.trace(shadow).buffer
        check_staged(torch, lambda hits, rays: [renderer.light_evaluate(hits, rays).buffer], renderer.last_light_ms, {"hits": found, "rays": shadow})


@pytest.mark.parametrize("spp", [1, 16])
def test_radiance(renderer, torch, spp):
    """explicit streams are tiled along with the rays (without them a record's stream is its index, and a tiled batch would not repeat).
    One sample per call: a record is a function of (ray, stream, sample, scene) only, so the tiled batch repeats the small one.  16 samples:
    the big batch's sample range is cut into two chunks and the small batch's into sixteen (a rule of the call's count, lrhip.h), so across
    the two batch sizes the sums agree up to the order of float additions only -- there the host-pointer call is held to the device-pointer
    call, which cuts the same chunks, and the sample counts to the small batch's"""
    scene = Scene.from_string(cornell_box(resolution=32, spp=16))
    oracle = Oracle(scene)
    rays, _ = _camera_rays(oracle, 0)
    oracle.close()
    rays = np.ascontiguousarray(rays[:1000])
    streams = np.arange(len(rays), dtype=np.uint32)
    renderer.upload(scene)
    call = lambda rays, streams: [renderer.radiance(rays, spp=spp, streams=streams, raw=True)]  # noqa: E731
    (small,), (big,) = check_staged(torch, call, renderer.last_radiance_ms, {"rays": rays, "streams": streams}, tiles=spp == 1)
    assert np.array_equal(big[:, 3], tiled(small[:, 3]))
