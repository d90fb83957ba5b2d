"""GPU test of the early fetch of the pool kernels' traversal loop (csrc/hip/megapool_kernel.h: LR_POOL_EARLY_FETCH).

The shipped pool kernels send an iteration's memory requests -- the node packets, the leaf triangles -- right behind the node step of the
iteration BEFORE, so that the end of that iteration (votes, the turnover of ended rays, the exit tests) runs while they are on their way.
That moves memory requests and nothing else: every lane tests the same triangles and boxes in the same order with the same arithmetic.
`make noearly` builds the lean pool kernels with the former order (LR_POOL_EARLY_FETCH=0); this test holds the shipped library to it:

  * films bit-identical, from the shipped binaries (no counters) and from their counting twins;
  * the twins' ray, node and triangle counters equal (the number of REQUESTS may differ: a wave that leaves the loop drops the requests it
    has just sent, and the packet loads go out in iterations without a lane at an inner node, too -- no counter counts requests);
  * the counting twins' own check of the reorder -- in every iteration every lane consumes what was requested for it, or the root if a turnover
    has just started its ray -- reports nothing (lrhip_counters::probe[15], zero in every build without the stall probe)."""
import os

import numpy as np
import pytest

from luisarender_amd import Scene
from luisarender_amd.scenes import cornell_box, generate_room_scene

pytestmark = pytest.mark.gpu
POOL = 4096  # LRHIP_FEAT_POOL
EARLY_FETCH_BROKEN = 15  # dev_trace.h: kProbeEarlyFetchBroken


def _variant_lib():
    from luisarender_amd import _ffi as ffi
    return os.path.join(ffi.LIB_DIR, "variants", "liblrhip_noearly.so")


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


@pytest.mark.parametrize("case", ["cornell", "room", "environment"])
def test_early_fetch_renders_the_frames_of_the_former_order(tmp_path, case):
    lib = _variant_lib()
    if not os.path.exists(lib):
        pytest.skip("make noearly (python __graft_entry__.py builds it)")
    if case == "cornell":
        scene, spp, feat = Scene.from_string(cornell_box(resolution=96, spp=16)), 16, 0
    elif case == "room":  # deep walks, every lamp, many turnovers and shading batches per wave
        scene, spp, feat = Scene.load(generate_room_scene(str(tmp_path), target_triangles=60_000, resolution=(160, 96), spp=8)), 8, 0
    else:  # the <environment> kernels (an image environment: rays that leave through the open front are lit)
        from test_environment import sky_image
        from luisarender_amd.scene import save_image
        sky = str(tmp_path / "sky.exr")
        save_image(sky, sky_image())
        env = f'render {{\n  environment : Spherical {{ emission : Image {{ file {{ "{sky}" }} }} }}'
        scene, spp, feat = Scene.from_string(cornell_box(resolution=96, spp=16).replace("render {", env)), 16, 4
    film_a, va, twin_a, vta, ca = _frames(None, scene, spp)
    film_b, vb, twin_b, vtb, cb = _frames(lib, scene, spp)
    assert va == vb == (POOL | feat) and vta == vtb == (POOL | feat | 1), (va, vb, vta, vtb)
    assert np.isfinite(film_a).all() and float(film_a[..., 3].min()) == spp
    assert np.array_equal(film_a, film_b), "shipped binaries: the films differ"
    assert np.array_equal(twin_a, twin_b), "counting twins: the films differ"
    assert np.array_equal(film_a[..., 3], twin_a[..., 3])  # (a binary and its twin: tests/test_gpu_pool.py)
    for k in ("paths", "closest_rays", "shadow_rays", "surface_hits", "nee_samples", "path_length_sum", "nodes_visited", "tris_tested", "nodes_empty"):
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert ca["nodes_visited"] > 0 and ca["tris_tested"] > 0
    assert ca["probe"][EARLY_FETCH_BROKEN] == 0, "a lane consumed a packet or a triangle that was not requested for it"
    assert not any(cb["probe"]), cb["probe"]
