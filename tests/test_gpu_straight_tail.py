"""GPU test of the straight-line control flow of the pool kernels' traversal loop (csrc/hip/dev_trace.h: LR_STRAIGHT_TAIL).

In the shipped kernels a node step stores its three far references at the top of the lane's stack without EXEC regions -- the top advances only
behind a valid one, so a missed child's word lies above the top, dead -- instead of three conditional pushes, and the pool kernels without the alpha
test commit a closest hit by selects on a scalar mask.  That changes how an iteration's instructions are laid out and nothing else: every lane tests
the same boxes and triangles in the same order with the same arithmetic, and, this time, in the same wave iterations.  `make nostraight` builds the
lean kernels of both schedulers and the pool kernels of the larger configurations without it (LR_STRAIGHT_TAIL=0); this test holds the shipped
library to it:

  * films bit-identical, from the shipped binaries (no counters) and from their counting twins;
  * the twins' path, ray, node and triangle counters equal, and their lane-iterations (trace_steps_busy), counted where the counter is a function of
    the binary: with one work item per tile (_twin_with_one_item_per_tile);
  * the counting twins' own check of the early requests reports nothing (lrhip_counters::probe[15]);
  * `make shallow` (a four-entry LDS stack, built with the straight-line pushes): most node steps stand at the boundary between the straight-line and
    the `deep` flow, where a stray store would land in another lane's row -- its film of the room must be the shipped library's bit for bit."""
import os

import numpy as np
import pytest

from luisarender_amd import Scene
from luisarender_amd.scenes import cornell_box, generate_room_scene

pytestmark = pytest.mark.gpu
POOL = 4096  # LRHIP_FEAT_POOL
EARLY_FETCH_BROKEN = 15  # dev_trace.h: kProbeEarlyFetchBroken
EQUAL_COUNTERS = ("paths", "closest_rays", "shadow_rays", "surface_hits", "nee_samples", "path_length_sum", "nodes_visited", "tris_tested", "nodes_empty")
ROOM_SPP = 8


def _variant_lib(name):
    from luisarender_amd import _ffi as ffi
    return os.path.join(ffi.LIB_DIR, "variants", f"liblrhip_{name}.so")


def _frames(lib_path, scene, spp, twin=True):
    """film without counters and the variant that ran; with `twin` also film and counters of the counting twin and its variant"""
    from luisarender_amd.render import MegaPathRenderer
    r = MegaPathRenderer(0, lib_path=lib_path) if lib_path else MegaPathRenderer(0)
    try:
        r.set_scheduler(True)
        r.upload(scene)
        r.render(0, spp, sync=True)
        shipped, v_shipped = r.download(False), r.last_variant()
        if not twin:
            return shipped, v_shipped
        r.clear()
        r.render(0, spp, counters=True, sync=True)
        return shipped, v_shipped, r.download(False), r.last_variant(), r.counters()
    finally:
        r.close()


def _twin_with_one_item_per_tile(lib_path, scene, spp):
    """film, variant and counters of the counting twin when every tile is ONE work item (uniform items, lrhip_set_diagnostics: item_scale < 0).

    A wave that runs its item dry takes the next one and traces the new item's paths beside the old one's last; which item that is, is a race for
    an atomic counter.  Under the default partition (Cornell case: 1152 items of 3 or 1 spp for 1152 waves) a few waves get a second item before
    the last block has started, and how long a lane waits in its wave's loop -- trace_steps_busy, nothing else that is counted -- differs by 0.02 %
    between two launches of ONE library.  With one item per tile (144 items of 1024 paths) every item has a wave to itself and the counter is a
    function of the binary: the same in every launch of a library."""
    from luisarender_amd.render import MegaPathRenderer
    r = MegaPathRenderer(0, lib_path=lib_path) if lib_path else MegaPathRenderer(0)
    try:
        r.set_scheduler(True)
        r.set_diagnostics(0, -1000.0)
        r.upload(scene)
        r.render(0, spp, counters=True, sync=True)
        return r.download(False), r.last_variant(), r.counters()
    finally:
        r.close()


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    """the room stand-in (deep walks, every lamp, many turnovers and shading batches per wave), one description for every test that renders it"""
    return Scene.load(generate_room_scene(str(tmp_path_factory.mktemp("room")), target_triangles=60_000, resolution=(160, 96), spp=ROOM_SPP))


@pytest.fixture(scope="module")
def sides(room, tmp_path_factory):
    """case -> (spp, feature bits, frames of the shipped library, frames of `make nostraight`, the one-item-per-tile twins of both): rendered once per module"""
    done = {}

    def get(case):
        if case not in done:
            if case == "cornell":
                scene, spp, feat = Scene.from_string(cornell_box(resolution=96, spp=16)), 16, 0
            elif case == "room":
                scene, spp, feat = room, ROOM_SPP, 0
            else:  # the <environment> kernels (an image environment: rays that leave through the open front are lit)
                from test_environment import sky_image
                from luisarender_amd.scene import save_image
                sky = str(tmp_path_factory.mktemp("sky") / "sky.exr")
                save_image(sky, sky_image())
                env = f'render {{\n  environment : Spherical {{ emission : Image {{ file {{ "{sky}" }} }} }}'
                scene, spp, feat = Scene.from_string(cornell_box(resolution=96, spp=16).replace("render {", env)), 16, 4
            lib = _variant_lib("nostraight")
            done[case] = (spp, feat, _frames(None, scene, spp), _frames(lib, scene, spp),
                          _twin_with_one_item_per_tile(None, scene, spp), _twin_with_one_item_per_tile(lib, scene, spp))
        return done[case]
    return get


CASES = ["cornell", "room", "environment"]


@pytest.mark.parametrize("case", CASES)
def test_straight_line_pushes_render_the_frames_of_the_conditional_ones(sides, case):
    if not os.path.exists(_variant_lib("nostraight")):
        pytest.skip("make nostraight (python __graft_entry__.py builds it)")
    spp, feat, (film_a, va, twin_a, vta, ca), (film_b, vb, twin_b, vtb, cb), _, _ = sides(case)
    assert va == vb == (POOL | feat) and vta == vtb == (POOL | feat | 1), (va, vb, vta, vtb)
    assert np.isfinite(film_a).all() and float(film_a[..., 3].min()) == spp
    assert np.array_equal(film_a, film_b), "shipped binaries: the films differ"
    assert np.array_equal(twin_a, twin_b), "counting twins: the films differ"
    assert np.array_equal(film_a[..., 3], twin_a[..., 3])  # (a binary and its twin: tests/test_gpu_pool.py)
    print(f"{case}: " + ", ".join(f"{k} {ca[k]} / {cb[k]}" for k in EQUAL_COUNTERS))
    for k in EQUAL_COUNTERS:
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert ca["nodes_visited"] > 0 and ca["tris_tested"] > 0
    assert ca["probe"][EARLY_FETCH_BROKEN] == 0, "a lane consumed a packet or a triangle that was not requested for it"
    assert cb["probe"][EARLY_FETCH_BROKEN] == 0, cb["probe"]


@pytest.mark.parametrize("case", CASES)
def test_straight_line_pushes_keep_the_lane_iterations(sides, case):
    """The twins' lane-iterations (trace_steps_busy) are equal: the grouping of a lane's steps into wave iterations does not change this time.
    Counted with one work item per tile, where the counter is a function of the binary (_twin_with_one_item_per_tile); the other nine counters
    and the film are held to equality in that launch as well."""
    if not os.path.exists(_variant_lib("nostraight")):
        pytest.skip("make nostraight (python __graft_entry__.py builds it)")
    spp, feat, _, _, (film_a, va, ca), (film_b, vb, cb) = sides(case)
    assert va == vb == (POOL | feat | 1), (va, vb)
    assert np.isfinite(film_a).all() and float(film_a[..., 3].min()) == spp
    assert np.array_equal(film_a, film_b), "counting twins, one item per tile: the films differ"
    print(f"{case}: trace_steps_busy {ca['trace_steps_busy']} shipped, {cb['trace_steps_busy']} nostraight")
    for k in EQUAL_COUNTERS + ("trace_steps_busy",):
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert ca["trace_steps_busy"] > 0
    assert ca["probe"][EARLY_FETCH_BROKEN] == 0 and cb["probe"][EARLY_FETCH_BROKEN] == 0, (ca["probe"], cb["probe"])


def test_straight_line_pushes_in_the_one_path_kernels(room):
    """the serial flow shares the node step's tail: the one-path kernels <0> / <1> on the room, against the same library"""
    from luisarender_amd.render import MegaPathRenderer
    lib = _variant_lib("nostraight")
    if not os.path.exists(lib):
        pytest.skip("make nostraight (python __graft_entry__.py builds it)")
    scene = room
    got = []
    for path in (None, lib):
        r = MegaPathRenderer(0, lib_path=path) if path else MegaPathRenderer(0)
        try:
            r.set_scheduler(False)
            r.upload(scene)
            r.render(0, ROOM_SPP, sync=True)
            film, v = r.download(False), r.last_variant()
            r.clear()
            r.render(0, ROOM_SPP, counters=True, sync=True)
            got.append((film, v, r.download(False), r.last_variant(), r.counters()))
        finally:
            r.close()
    (film_a, va, twin_a, vta, ca), (film_b, vb, twin_b, vtb, cb) = got
    assert va == vb == 0 and vta == vtb == 1, (va, vb, vta, vtb)
    assert np.isfinite(film_a).all() and float(film_a[..., 3].min()) == ROOM_SPP
    assert np.array_equal(film_a, film_b), "shipped binaries: the films differ"
    assert np.array_equal(twin_a, twin_b), "counting twins: the films differ"
    for k in EQUAL_COUNTERS:
        assert ca[k] == cb[k], (k, ca[k], cb[k])
    assert ca["nodes_visited"] > 0 and ca["tris_tested"] > 0


def test_straight_line_pushes_at_the_boundary_of_the_overflow_area(room):
    lib = _variant_lib("shallow")
    if not os.path.exists(lib):
        pytest.skip("make shallow (python __graft_entry__.py builds it)")
    film_a, va = _frames(None, room, ROOM_SPP, twin=False)
    film_b, vb = _frames(lib, room, ROOM_SPP, twin=False)
    assert va == vb == POOL, (va, vb)
    assert np.isfinite(film_a).all() and float(film_a[..., 3].min()) == ROOM_SPP
    assert np.array_equal(film_a, film_b), "four-entry LDS stack: the film differs from the shipped library's"
