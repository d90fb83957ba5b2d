"""tests/sampler_reference.py, the numpy restatement of the reference's samplers, pinned to the oracle's sampler hook bit for bit -- every
sampler kind, TileShared with and without jitter -- and the relation between its 2-D and 1-D draws that the GPU tests rely on."""
import numpy as np
import pytest

import sampler_reference as R
from luisarender_amd import Scene
from oracle.check import oracle_lib

DRAWS = 1100  # past the Sobol sampler's wrap at 1024 dimensions


def words(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("sampler,tile,jitter", R.SAMPLER_CASES)
def test_restatement_equals_the_oracle_stream(sampler, tile, jitter):
    spp = 8
    scene = Scene.from_string(R.scene_text(sampler, tile, jitter, spp=spp), build_accel=False)
    view = scene.view()
    w, h = int(view.camera.width), int(view.camera.height)
    assert (int(view.sampler.tile_size[0]) != 0) == (tile is not None) and bool(view.sampler.tile_jitter) == jitter
    lib = oracle_lib()
    pixels = [(0, 0), (w - 1, h - 1), (23, 41)]
    cases = [(px, py, s) for px, py in pixels for s in (0, 1, spp - 1)]
    px, py, s = (np.array(c, np.uint32) for c in zip(*cases))
    ref = R.Samplers(view)
    ref.start(px, py, s)
    got = ref.draw("p" + "1" * 64)  # 64 draws per call, as a sampler_draw pattern holds
    rest = [ref.draw("1" * 64) for _ in range((DRAWS - 64 + 63) // 64)]
    got = np.concatenate([got] + rest, axis=1)[:, :2 + DRAWS]
    want = np.stack([R.oracle_stream(lib, view, *c, DRAWS) for c in cases])
    assert got.dtype == np.float32 and ((got >= 0) & (got < 1)).all()
    assert np.array_equal(words(got), words(want))
    if sampler != "Independent" or tile is None:
        assert len(np.unique(words(want[:, :16]), axis=0)) > 1  # (the streams differ from each other)


@pytest.mark.parametrize("sampler", ["Independent", "PCG32", "Sobol"])
def test_a_2d_draw_is_two_1d_draws_away_from_the_wrap(sampler):
    view = Scene.from_string(R.scene_text(sampler), build_accel=False).view()
    px, py, s = np.arange(40, dtype=np.uint32), np.arange(40, dtype=np.uint32)[::-1].copy(), np.arange(40, dtype=np.uint32) % 8
    a, b = R.Samplers(view), R.Samplers(view)
    a.start(px, py, s), b.start(px, py, s)
    assert np.array_equal(words(a.draw("p" + "2" * 20)), words(b.draw("p" + "1" * 40)))


def test_padded_sobol_2d_is_not_two_1d_draws_and_sobol_wraps_a_pair_early():
    view = Scene.from_string(R.scene_text("PaddedSobol"), build_accel=False).view()
    px = np.arange(40, dtype=np.uint32)
    a, b = R.Samplers(view), R.Samplers(view)
    a.start(px, px, 3), b.start(px, px, 3)
    two, ones = a.draw("2"), b.draw("11")
    assert np.array_equal(words(two[:, 0]), words(ones[:, 0])) and not np.array_equal(words(two[:, 1]), words(ones[:, 1]))
    # Sobol at dimension 1023: a 1-D draw takes dimension 1023, a pair wraps to 2 / 3 first (sobol.cpp:148 against :155)
    view = Scene.from_string(R.scene_text("Sobol"), build_accel=False).view()
    a, b = R.Samplers(view), R.Samplers(view)
    a.start(px, px, 3), b.start(px, px, 3)
    for sampler in (a, b):
        for _ in range(1021):
            sampler.next_1d()
        assert (sampler.dimension == 1023).all()
    two, ones = a.draw("2"), b.draw("11")
    assert not np.array_equal(words(two[:, 0]), words(ones[:, 0])) and (a.dimension == 4).all() and (b.dimension == 3).all()


def test_tile_shared_streams_are_shared_within_a_tile():
    view = Scene.from_string(R.scene_text("PaddedSobol", 8, False), build_accel=False).view()
    ref = R.Samplers(view)
    ref.start(np.array([8, 15, 16], np.uint32), np.array([8, 15, 8], np.uint32), 2)
    u = ref.draw("p2" + "1212")
    assert np.array_equal(words(u[0]), words(u[1])) and not np.array_equal(words(u[0]), words(u[2]))
