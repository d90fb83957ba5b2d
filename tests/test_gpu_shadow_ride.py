"""GPU test of the shadow ride of the pool kernels (csrc/hip/megapool_kernel.h: LR_POOL_SHADOW_RIDE).

A path's last vertex spawns no closest-hit ray.  Where it has a light sample the context used to stay open for one more job that held the shadow
ray alone; in the shipped pool kernels such a context takes the next sample at once, and the finished path's shadow ray is traced in one job with
the new path's camera ray.  Where that job is shaded the finished path joins the film -- the same `Li += nee`, the same completion code -- before
the new path's first vertex is shaded.  Every ray, every random number and every float operation of every path is unchanged; only which batch
starts which sample, and when a sample's integers are added to the film, differ.  `make noride` builds the pool kernels without it
(LR_POOL_SHADOW_RIDE=0); this test holds the shipped library to it, after set_scheduler(True):

  * films bit-identical, from the shipped binaries (no counters) and from their counting twins;
  * the twins' path, ray, vertex, node and triangle counters equal, and `shade_busy` (vertices shaded) with them;
  * the counting twins' own check of the early fetch reports nothing (lrhip_counters::probe[15]);
  * where the hand-over must fire the shipped twin runs strictly fewer shading batches (shade_calls).

The cases are the smallest that can go wrong: the Cornell box on <4096>; the same at depth 1, where every vertex is a last one and every path
is handed over by the one before it; the room stand-in (many batches, turnovers and work items per wave); a 45 x 27 frame at 1 and 3 spp (edge
tiles whose lanes must ask again, and a launch that is mostly its tail: no sample left, the shadow-only job must still finish the paths); an
image environment on <4100> (paths that end in misses); PaddedSobol on <20482>, Sobol and PCG32 on <4098> (the extra quad of the record sits at
index 4, 5 and 5); and a film clamp below the lamp's radiance (the clamp is not linear in Li: a sample's add must not be split in two)."""
import os

import numpy as np
import pytest

from luisarender_amd import Scene
from luisarender_amd.scenes import cornell_box, generate_room_scene

pytestmark = pytest.mark.gpu
POOL = 4096  # LRHIP_FEAT_POOL
GENERIC = 2  # LRHIP_FEAT_GENERIC: the run-time generic sampler
PADDED = 16384 | GENERIC  # kFeatPadded: the generic sampler's kind fixed to PaddedSobol
ENVIRONMENT = 4
EARLY_FETCH_BROKEN = 15  # dev_trace.h: kProbeEarlyFetchBroken
EQUAL_COUNTERS = ("paths", "closest_rays", "shadow_rays", "surface_hits", "nee_samples", "path_length_sum", "nodes_visited", "tris_tested", "nodes_empty",
                  "shade_busy")
CASES = ["cornell", "depth1", "room", "edge_1spp", "edge_3spp", "environment", "PaddedSobol", "Sobol", "PCG32", "clamp"]
FIRES = ("cornell", "depth1")  # (the room's 123 k paths are fewer than the launch has contexts: next to no path ends with a sample left to start)


def _variant_lib():
    from luisarender_amd import _ffi as ffi
    return os.path.join(ffi.LIB_DIR, "variants", "liblrhip_noride.so")


def _frames(lib_path, scene, spp):
    """film without counters, film and counters of the counting twin, the variants that ran"""
    from luisarender_amd.render import MegaPathRenderer
    r = MegaPathRenderer(0, lib_path=lib_path) if lib_path else MegaPathRenderer(0)
    try:
        r.set_scheduler(True)
        r.upload(scene)
        r.render(0, spp, sync=True)
        shipped, v_shipped = r.download(False), r.last_variant()
        r.clear()
        r.render(0, spp, counters=True, sync=True)
        return shipped, v_shipped, r.download(False), r.last_variant(), r.counters()
    finally:
        r.close()


def _scene(case, tmp_path):
    """scene, spp, feature bits of the kernel besides POOL"""
    if case == "cornell":
        return Scene.from_string(cornell_box(resolution=96, spp=16)), 16, 0
    if case == "depth1":
        return Scene.from_string(cornell_box(resolution=96, spp=16, depth=1)), 16, 0
    if case == "room":
        return Scene.load(generate_room_scene(str(tmp_path), target_triangles=60_000, resolution=(160, 96), spp=8)), 8, 0
    if case.startswith("edge_"):
        spp = int(case[5])
        return Scene.from_string(cornell_box(resolution=(45, 27), spp=spp)), spp, 0
    if case == "environment":  # (the image-environment Cornell box of tests/test_gpu_leaf_pair.py: rays that leave through the open front are lit)
        from test_environment import sky_image
        from luisarender_amd.scene import save_image
        sky = str(tmp_path / "sky.exr")
        save_image(sky, sky_image())
        env = f'render {{\n  environment : Spherical {{ emission : Image {{ file {{ "{sky}" }} }} }}'
        return Scene.from_string(cornell_box(resolution=96, spp=16).replace("render {", env)), 16, ENVIRONMENT
    if case in ("PaddedSobol", "Sobol", "PCG32"):
        return Scene.from_string(cornell_box(resolution=96, spp=16, sampler=case)), 16, PADDED if case == "PaddedSobol" else GENERIC
    assert case == "clamp"  # the lamp emits (17, 12, 4): a sample that sees it directly, or is lit by it strongly, is scaled down
    return Scene.from_string(cornell_box(resolution=96, spp=16).replace("resolution { 96, 96 }", "resolution { 96, 96 } clamp { 2 }")), 16, 0


@pytest.mark.parametrize("case", CASES)
def test_shadow_ride_renders_the_frames_of_the_shadow_only_job(tmp_path, case):
    lib = _variant_lib()
    if not os.path.exists(lib):
        pytest.skip("make noride (python __graft_entry__.py builds it)")
    scene, spp, feat = _scene(case, tmp_path)
    film_a, va, twin_a, vta, ca = _frames(None, scene, spp)
    film_b, vb, twin_b, vtb, cb = _frames(lib, scene, spp)
    print(f"{case}: shading batches {ca['shade_calls']} riding, {cb['shade_calls']} with the shadow-only job; vertices {ca['shade_busy']} / {cb['shade_busy']}, "
          f"paths {ca['paths']} / {cb['paths']}, shadow rays {ca['shadow_rays']} / {cb['shadow_rays']}")
    assert va == vb == (POOL | feat) and vta == vtb == (POOL | feat | 1), (va, vb, vta, vtb)
    assert np.isfinite(film_a).all()
    assert np.array_equal(film_a[..., 3], np.full_like(film_a[..., 3], spp)), "a pixel without its spp samples"
    assert np.array_equal(film_a, film_b), "shipped binaries: the films differ"
    assert np.array_equal(twin_a, twin_b), "counting twins: the films differ"
    assert np.array_equal(film_a[..., 3], twin_a[..., 3])  # (a binary and its twin: tests/test_gpu_pool.py)
    for k in EQUAL_COUNTERS:
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert ca["paths"] == spp * film_a.shape[0] * film_a.shape[1] and ca["shade_busy"] > 0
    assert ca["probe"][EARLY_FETCH_BROKEN] == 0, "a lane consumed a packet or a triangle that was not requested for it"
    assert cb["probe"][EARLY_FETCH_BROKEN] == 0, cb["probe"]
    if case == "clamp":  # (the clamp bites: no sample's largest component beyond 2, and some at it)
        assert 1.5 * spp < float(film_a[..., :3].max()) <= 2.0 * spp * (1.0 + 1e-5)
    if case in FIRES:
        assert ca["shade_calls"] < cb["shade_calls"], (ca["shade_calls"], cb["shade_calls"])
