"""Ray queries on the device, judged ray by ray with error bands and no exclusions (tests/raycast_judge.py has the rules, the families and the
derivation of the bands): box corners, shared edges, grazing rays, segment ends on a surface, far origins, directions of any length, t_min <= -0.0,
degenerate neighbours -- through MegaPathRenderer.trace, closest hit and any hit, and once more through the alpha-test kernel."""
import numpy as np
import pytest

import raycast_judge as J
import raycast_reference as R
from luisarender_amd.render import MegaPathRenderer

pytestmark = pytest.mark.gpu

# The largest observed error of a reported closest hit as a share of its band, per family, on the MI355X -- for information: the bar is 1.0 and is
# derived (raycast_judge.py), not measured.
MEASURED_BAND_SHARE = {
    "base_soup": 0.188,
    "base_cornell": 0.235,
    "base_room": 0.200,
    "far_shell": 0.245,
    "far_shell_moved": 0.254,
    "far_shell_small": 0.246,
    "far_shell_large": 0.272,
    "far_room": 0.177,
    "direction_length_soup64": 0.217,
    "direction_length_cornell": 0.223,
    "direction_components": 0.229,
    "interval_soup": 0.217,
    "interval_cornell": 0.210,
    "planes": 0.233,
    "edge_aimed": 0.224,
    "degenerate": 0.245,
}


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def _report(bad, rays):
    return {rule: (len(rows), [(int(k), rays[k].tolist()) for k in rows[:3]]) for rule, rows in bad.items()}


# A FINDING IN THE TRAVERSAL LOOP, not in the query prologue, PINNED: ray 743 of interval_cornell starts 0.24 below the Cornell box's ceiling
# with t_min = t* - 4 bands = 1.0081624 under a SURE hit at t* = 1.0081696, and the device misses it in both modes; the float32 restatement of the triangle
# test accepts the hit, and the parent commit's kernel misses the ray as well.  Read from the code, not traced on the device: the ceiling's box is flat,
# and trav_slab_sort_q computes a child's plane distance as fma(byte, scale / d.y, (node origin - o.y) / d.y); under a node whose box starts at the floor
# that is 2263.98 - 2262.97 for this ray, an absolute error of some 1e-4 on a distance of 1, against the 7e-6 between t_min and the hit.  Clamped by t_min
# the entry distance of the flat box then lies behind its exit distance and the child is dropped; `tn <= tf * 1.0000004f` allows for 4 ulps of the RESULT
# only.  The same would cut a flat box off at t_max.  A fix belongs in dev_trace.h's node step (a slack on the interval clamps in proportion to the
# cancelled terms), costs instructions in the renderers' hot loop and has to be measured on C2 against the parent before it lands; this change does not
# touch dev_trace.h.  The test asserts that the violations are EXACTLY these: every other ray of the family is enforced, a fix of the loop fails the
# test until the entry is taken out, and nothing else may join it.
KNOWN = {("interval_cornell", "closest"): {"miss": [743]}, ("interval_cornell", "any"): {"not_occluded": [743]}}


@pytest.mark.parametrize("mode", ("closest", "any"))
@pytest.mark.parametrize("family", list(J.FAMILIES))
def test_every_ray_is_judged(renderer, capsys, family, mode):
    scene, tris, rays, tab = J.case(family)
    renderer.upload(scene)
    answer = renderer.trace(rays, any_hit=True) if mode == "any" else renderer.trace(rays).buffer
    bad, share = J.verdicts(tab, tris, mode, answer)
    with capsys.disabled():
        print(f"\n[edges] {family} {mode}: {len(rays)} rays, violations {({k: len(v) for k, v in bad.items()})}, largest error {share:.3f} of its band "
              f"(recorded {MEASURED_BAND_SHARE.get(family)})")
    assert {rule: rows.tolist() for rule, rows in bad.items()} == KNOWN.get((family, mode), {}), _report(bad, rays)
    assert share <= 1.0


def test_edge_aimed_leaks(renderer, capsys):
    """from inside the closed shell at its shared edges and vertices a miss is a leak: nothing else is behind.  The yardstick is the float32 restatement
    of the same triangle test with exact division, on the same rays; the two counts are samples of about the same rate, and the bar (twice the
    yardstick's plus 10 rays) only catches another order of magnitude, such as a lost equality in >= 0."""
    scene, tris, rays, tab = J.case("edge_aimed")
    renderer.upload(scene)
    device = J.leaks(renderer.trace(rays).buffer)
    occluded = renderer.trace(rays, any_hit=True)
    yardstick = J.leaks(J.restatement(tris, rays)[0])
    with capsys.disabled():
        print(f"\n[edges] edge_aimed: {len(rays)} rays, leaks: device {device} (any hit {int((~occluded).sum())}), float32 restatement {yardstick} "
              f"(recorded {J.MEASURED_LEAKS})")
    assert device <= 2 * yardstick + 10
    assert int((~occluded).sum()) <= 2 * yardstick + 10


@pytest.mark.parametrize("family", ("base_soup", "interval_soup"))
def test_alpha_kernel_returns_the_plain_kernel_bits(renderer, family):
    """the ALPHA kernel (trace_until_refill) over soup64 under an opacity texture that is 1 everywhere but is not folded: candidates are only parked and
    committed, the arithmetic is trav_leaf_test's, so the bits are the plain kernel's -- on the base rays and at the interval's edges"""
    scene = J.scene_of("alpha")
    assert scene.view().any_non_opaque == 1
    tris = R.baked_triangles(scene)
    plain_tris = R.baked_triangles(J.scene_of("soup64"))
    assert all(np.array_equal(tris[k], plain_tris[k]) for k in ("v0", "e1", "e2"))
    if family == "base_soup":
        rays = R.make_rays(scene)
    else:
        rays = np.array(J._interval("soup64")[1])
    tab = J.table(tris, rays)
    renderer.upload(scene)
    plain, tested = renderer.trace(rays).buffer, renderer.trace(rays, alpha_test=True).buffer
    plain_any, tested_any = renderer.trace(rays, any_hit=True), renderer.trace(rays, any_hit=True, alpha_test=True)
    for mode, answer in (("closest", plain), ("closest", tested), ("any", plain_any), ("any", tested_any)):
        bad, share = J.verdicts(tab, tris, mode, answer)
        assert bad == {} and share <= 1.0, (mode, _report(bad, rays))
    assert plain.view(np.uint32)[:, 3].min() != R.INVALID  # (some ray hits)
    assert np.array_equal(tested.view(np.uint32), plain.view(np.uint32))
    assert np.array_equal(tested_any, plain_any)
