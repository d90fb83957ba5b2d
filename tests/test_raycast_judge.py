"""The judge of the ray queries (tests/raycast_judge.py) must be able to fail: it accepts a float32 restatement of the device's triangle test on
every family, rejects seven wrong restatements, keeps the undecided caps, and decides hand-computed cases as the rules say.  No GPU."""
import numpy as np
import pytest

import raycast_judge as J
import raycast_reference as R


def _triangles(rows):
    tris = np.zeros(len(rows), R._TRIANGLE)
    for k, (v0, e1, e2, inst, prim, flags) in enumerate(rows):
        tris[k] = (v0, inst, e1, prim, e2, flags)
    return tris


ONE = _triangles([((0, 0, 0), (1, 0, 0), (0, 1, 0), 5, 9, 3)])


def _ray(o, d, t_min=1e-4, t_max=np.inf):
    return np.array([[*o, t_min, *d, t_max]], np.float32)


def _record(t, u, v, inst, prim, tri):
    out = np.zeros((1, 8), np.float32)
    out[0, :3] = (t, u, v)
    out.view(np.uint32)[0, 3:6] = (inst, prim, tri)
    return out


MISS = _record(np.inf, 0, 0, R.INVALID, R.INVALID, R.INVALID)


def test_the_constant_is_the_count_of_the_longest_chain():
    assert (J.C_NUM, J.C_DET, J.C_DIV) == (7, 6, 3) and J.C == 16 and J.EPS == 2.0 ** -24


def test_a_sure_hit_and_its_rules():
    rays = _ray((0.25, 0.5, 2.0), (0, 0, -1))
    tab = J.table(ONE, rays)
    assert tab.n_sure[0] == 1 and tab.n_maybe[0] == 1 and not tab.undecided_closest[0] and not tab.undecided_any[0]
    assert tab.t[0] == pytest.approx(2.0, abs=1e-12) and 0 < tab.dt[0] < 1e-5 and 0 < tab.du[0] < 1e-5
    assert J.verdicts(tab, ONE, "closest", _record(2.0, 0.25, 0.5, 5, 9, 0))[0] == {}
    assert set(J.verdicts(tab, ONE, "closest", MISS)[0]) == {"miss"}
    assert set(J.verdicts(tab, ONE, "closest", _record(2.0, 0.25, 0.5, 5, 8, 0))[0]) == {"ids"}
    assert set(J.verdicts(tab, ONE, "closest", _record(2.0 + 1e-4, 0.25, 0.5, 5, 9, 0))[0]) == {"values"}
    assert set(J.verdicts(tab, ONE, "closest", _record(2.0, 0.25 + 1e-4, 0.5, 5, 9, 0))[0]) == {"values"}
    assert set(J.verdicts(tab, ONE, "closest", _record(2.0, 0.25, 0.5, 5, 9, 1))[0]) == {"not_maybe"}
    assert J.verdicts(tab, ONE, "any", np.array([1]))[0] == {} and set(J.verdicts(tab, ONE, "any", np.array([0]))[0]) == {"not_occluded"}
    share = J.verdicts(tab, ONE, "closest", _record(2.0, np.float32(0.25) + np.float32(2.0 ** -25), 0.5, 5, 9, 0))[1]
    assert 0.0 < share < 1.0


def test_a_miss_and_an_undecided_ray():
    tab = J.table(ONE, _ray((-0.01, 0.5, 2.0), (0, 0, -1)))
    assert tab.n_maybe[0] == 0
    assert J.verdicts(tab, ONE, "closest", MISS)[0] == {} and set(J.verdicts(tab, ONE, "any", np.array([1]))[0]) == {"occluded"}
    assert set(J.verdicts(tab, ONE, "closest", _record(2.0, 0.0, 0.5, 5, 9, 0))[0]) == {"not_maybe"}
    # exactly on the edge u = 0: both answers are legal, and the ray counts as undecided
    tab = J.table(ONE, _ray((0.0, 0.5, 2.0), (0, 0, -1)))
    assert tab.n_sure[0] == 0 and tab.n_maybe[0] == 1 and tab.undecided_closest[0] and tab.undecided_any[0]
    assert J.verdicts(tab, ONE, "closest", MISS)[0] == {} and J.verdicts(tab, ONE, "closest", _record(2.0, 0.0, 0.5, 5, 9, 0))[0] == {}
    assert J.verdicts(tab, ONE, "any", np.array([0]))[0] == {} and J.verdicts(tab, ONE, "any", np.array([1]))[0] == {}


def test_depth_rule_and_the_interval():
    two = _triangles([((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, 0, 3), ((0, 0, 1), (1, 0, 0), (0, 1, 0), 1, 0, 3)])
    tab = J.table(two, _ray((0.25, 0.5, 2.0), (0, 0, -1)))
    assert tab.n_sure[0] == 2
    assert J.verdicts(tab, two, "closest", _record(1.0, 0.25, 0.5, 1, 0, 1))[0] == {}
    assert set(J.verdicts(tab, two, "closest", _record(2.0, 0.25, 0.5, 0, 0, 0))[0]) == {"depth"}
    # the interval: t_min < t < t_max, the search starts at max(t_min, +0), directions of any length, t in units of |d|
    for t_min, t_max, sure in ((1e-4, 2.5, 1), (1e-4, 1.5, 0), (1.5, np.inf, 1), (2.5, np.inf, 0), (-0.0, np.inf, 1), (-1.0, np.inf, 1)):
        tab = J.table(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -1), t_min, t_max))
        assert tab.n_sure[0] == sure and tab.n_maybe[0] == sure, (t_min, t_max)
    tab = J.table(ONE, _ray((0.25, 0.5, -2.0), (0, 0, -1), -5.0))  # behind the origin: a negative t_min does not reach it
    assert tab.n_maybe[0] == 0
    tab = J.table(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -2.0 ** -140)))
    assert tab.n_sure[0] == 1 and tab.t[0] == pytest.approx(2.0 ** 141, rel=1e-12)
    assert J.verdicts(tab, ONE, "closest", _record(np.inf, 0.25, 0.5, 5, 9, 0))[0] == {}  # the caller's t does not fit float32
    # t_max exactly at the hit: undecided, either answer is legal
    tab = J.table(ONE, _ray((0.25, 0.5, 2.0), (0, 0, -1), 1e-4, 2.0))
    assert tab.n_sure[0] == 0 and tab.n_maybe[0] == 1
    # invisible and zero-edge triangles are in neither set
    for tris in (_triangles([((0, 0, 0), (1, 0, 0), (0, 1, 0), 5, 9, 2)]), _triangles([((0, 0, 0), (0, 0, 0), (0, 1, 0), 5, 9, 3)])):
        assert J.table(tris, _ray((0.25, 0.5, 2.0), (0, 0, -1))).n_maybe[0] == 0


@pytest.fixture(scope="module")
def restated():
    """family -> the float32 restatement's answers, computed once"""
    cache = {}

    def get(family, wrong=None):
        if (family, wrong) not in cache:
            _, tris, rays, _ = J.case(family)
            cache[family, wrong] = J.restatement(tris, rays, wrong)
        return cache[family, wrong]
    return get


@pytest.mark.parametrize("family", list(J.FAMILIES))
def test_caps_and_a_correct_restatement(restated, family):
    """the undecided share keeps the cap (but in the family that is undecided by design), and the float32 brute-force restatement of
    trav_leaf_test behind the query prologue has no violation in either mode"""
    scene, tris, rays, tab = J.case(family)
    assert 0 < len(rays) <= R.RAY_COUNT and len(tris) <= 8000
    closest, occluded = restated(family)
    print(f"[judge] {family}: {len(rays)} rays, {len(tris)} triangles, {len(tab.key)} candidates, undecided closest {int(tab.undecided_closest.sum())} "
          f"any {int(tab.undecided_any.sum())}, sure hits {int((tab.n_sure > 0).sum())}, restatement hits {int(occluded.sum())}")
    if family not in J.UNCAPPED:
        assert tab.undecided_closest.mean() <= R.AMBIGUOUS_CAP and tab.undecided_any.mean() <= R.AMBIGUOUS_CAP
    assert family in J.UNCAPPED or 0.02 < (tab.n_sure > 0).mean()  # the family exercises hits
    bad, share = J.verdicts(tab, tris, "closest", closest)
    assert bad == {}, {k: (len(v), v[:5]) for k, v in bad.items()}
    assert share <= 1.0
    bad, _ = J.verdicts(tab, tris, "any", occluded)
    assert bad == {}, {k: (len(v), v[:5]) for k, v in bad.items()}


# the family on which each wrong restatement has to be caught (and by which rule, first of all)
CAUGHT = {"uv_sum_short": ("base_soup", "miss"), "uv_swapped": ("base_soup", "values"), "farthest_on_97th": ("base_cornell", "depth"),
          "t_min_ignored": ("interval_soup", "not_maybe"), "visibility_ignored": ("degenerate", "not_maybe"),
          "inverse_capped": ("direction_length_cornell", "miss"), "signed_keys_dropped": ("interval_cornell", "miss")}


@pytest.mark.parametrize("wrong", J.WRONG)
def test_wrong_restatements_are_rejected(restated, wrong):
    family, rule = CAUGHT[wrong]
    _, tris, rays, tab = J.case(family)
    closest, occluded = restated(family, wrong)
    bad, _ = J.verdicts(tab, tris, "closest", closest)
    print(f"[judge] {wrong} on {family}: " + ", ".join(f"{k} {len(v)}" for k, v in bad.items()))
    assert rule in bad
    if wrong not in ("uv_swapped", "farthest_on_97th"):  # (those two change which hit is reported, not whether there is one)
        assert J.verdicts(tab, tris, "any", occluded)[0] != {}


def test_pulled_back_parameters():
    """what the module records is what the families use, and a pulled-back distance is the most extreme that keeps the cap: one step further breaks it"""
    for key, scene_name, seed, centre in (("far_shell_diagonals", "shell", 13, J.SHELL_CENTRE), ("far_room_diagonals", "room", 17, None)):
        further = J.PULLED_BACK[key][:-1] + (J.NEXT_STEP[key],)
        assert J.PULLED_BACK[key][-1] < J.NEXT_STEP[key] <= 1e4
        _, rays = J._far(scene_name, further, seed, centre)
        tab = J.table(R.baked_triangles(J.scene_of(scene_name)), rays)
        print(f"[judge] {key} with {J.NEXT_STEP[key]:g} as the last distance: undecided closest {tab.undecided_closest.mean():.4f} any {tab.undecided_any.mean():.4f}")
        assert max(tab.undecided_closest.mean(), tab.undecided_any.mean()) > R.AMBIGUOUS_CAP
    assert set(J.PULLED_BACK) == {"far_shell_diagonals", "far_room_diagonals", "planes_in_plane_rays", "degenerate_aimed_rays", "secondary_rays_with_zero_t_min"}
    assert max(J.PULLED_BACK["far_shell_diagonals"]) <= 1e4 and max(J.PULLED_BACK["far_room_diagonals"]) <= 1e4
    assert J.PULLED_BACK["planes_in_plane_rays"] <= R.AMBIGUOUS_CAP * R.RAY_COUNT
    assert len(R.baked_triangles(J.scene_of("shell"))) == 1280
    assert J.scene_of("alpha").view().any_non_opaque == 1
    _, tris, rays, _ = J.case("direction_length_cornell")
    lengths = np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1)
    assert lengths.min() < 2.0 ** -139 and lengths.max() > 2.0 ** 125
    _, _, rays, _ = J.case("interval_soup")
    assert (rays[:, 7] == np.finfo(np.float32).max).any() and np.signbit(rays[:, 3]).any() and (rays[:, 3] == -1.0).any()
