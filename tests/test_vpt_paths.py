"""The corpus and the judge of tests/vpt_paths.py on the CPU: every case keeps the conditions that make a verdict on the device worth
something (few MAYBE paths, enough non-zero ones, the code it is named for is reached), the judge accepts the oracle's other two builds
standing in for the device, and rejects twelve planted mistakes -- each rendered by the oracle on an altered scene, or made by altering its
films, and handed in as "the device" on the case meant to catch it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import vpt_paths as vp  # noqa: E402

pytestmark = pytest.mark.skipif(not vp.oracles_present(), reason="oracle/liboracle.so, liboracle_fma.so and liboracle_ulp.so are not built")

HAS_SURFACE, HAS_MEDIUM = 4, 16  # lr_scene.h: LR_SHAPE_HAS_SURFACE, LR_SHAPE_HAS_MEDIUM
DISNEY, MIX, LAYERED = 6, 7, 8    # LR_SURFACE_*
MEDIA = {"vacuum": 0, "medium_box": 2, "index_matched": 2, "nested3": 4, "equal_priority": 3, "bare_shell": 2}  # 1 otherwise: the fog
SAMPLER = {"sobol": 1, "padded_sobol": 2, "pcg32": 3}  # LR_SAMPLER_*; Independent = 0 otherwise
WALKS_CROSS = ("glass", "medium_box", "index_matched", "nested3", "equal_priority", "pane")  # surfaces that shadow walks go through


def _reference(case, tmp_path_factory):
    return vp.case_reference(case, tmp_path_factory.getbasetemp())


@pytest.mark.parametrize("case", vp.CASES)
def test_corpus_conditions(case, tmp_path_factory):
    text, ref, counters = _reference(case, tmp_path_factory)
    verdict = vp.judge(ref, ref["plain"])
    print(f"{case}: {verdict}")
    assert ref["plain"].shape == ((vp.S, 11, 13, 4) if case == "ragged" else (vp.S, 16, 16, 4))
    assert verdict.maybe_share <= vp.MAYBE_CAP.get(case, 0.01)
    assert verdict.sure_nonzero >= vp.NONZERO_MIN * verdict.sure
    # the case reaches what it is named for
    view = vp.scene_of(text).view()
    depth = vp.DEPTH.get(case, 6)
    assert view.integrator.kind == 3 and view.integrator.max_depth == depth and view.film.clamp == 1e6
    assert view.medium_count == MEDIA.get(case, 1)
    assert view.light_count == (1 if case == "vacuum" else 0) and (view.environment.kind != 0) == (case != "vacuum")
    assert view.sampler.kind == SAMPLER.get(case, 0) and view.camera.kind == (1 if case == "thin_lens" else 0)
    assert view.integrator.rr_depth == {"vacuum": 0, "rr_first_vertex": 1}.get(case, 3)
    assert counters["paths"] == ref["plain"][..., 3].size and counters["nee_samples"] > 0
    if case in WALKS_CROSS:
        assert counters["closest_rays"] > counters["paths"] * (depth + 1)
    media = [view.media[i] for i in range(view.medium_count)]
    if case != "vacuum":
        fog = media[view.integrator.environment_medium_tag]
        g = {"isotropic": 5e-4, "forward": 0.9, "backward": -0.9}.get(case, 0.4)
        assert abs(fog.g - g) < 1e-7 and (abs(g) < 1e-3) == (case == "isotropic")
        assert (max(fog.sigma_s) == 0) == (case == "absorbing") and (max(fog.sigma_a) == 0) == (case == "scattering")
    kinds = {view.surfaces[i].kind for i in range(view.surface_count)}
    for name, kind in (("disney", DISNEY), ("mix", MIX), ("layered", LAYERED)):
        assert (kind in kinds) == (case == name)
    if case in ("directional_env", "image_env"):
        assert view.environment.kind == (2 if case == "directional_env" else 1)
        if case == "image_env":
            image = view.textures[view.environment.emission_tex]
            assert (image.width, image.height) == (8, 4)
    if case == "medium_box":
        assert sorted(m.eta for m in media) == pytest.approx([1.0, 1.3])
    if case == "nested3":  # priorities 2, 0, 1 from the outside in, tags 0, 1, 2; the fog, registered last, yields to all
        assert [m.priority for m in media] == [2, 0, 1, vp.FOG_PRIORITY] and view.integrator.environment_medium_tag == 3
    if case == "equal_priority":
        assert [m.priority for m in media] == [1, 1, vp.FOG_PRIORITY]
    if case == "bare_shell":
        flags = [view.instances[i].handle.x & 1023 for i in range(view.instance_count)]
        shell = [i for i, f in enumerate(flags) if f & HAS_MEDIUM and not f & HAS_SURFACE]
        assert len(shell) == 1
        # shadow walks cross the shell: it is the first thing over the floor between the blocks and over the short block's top (a walk that
        # enters it), and the tall block's top lies INSIDE it (a walk that leaves a medium the path never entered: exit of an absent entry)
        from oracle.check import Oracle
        o = Oracle(vp.scene_of(text))
        for point, inside in (((150, 1, 400), False), ((350, 1, 150), False), ((185, 166, 170), False), ((370, 331, 350), True)):
            inst, _, _, _, t = o.trace_closest(point, (0.05, 1.0, 0.02))
            assert inst == shell[0] and (t < 15) == inside, (point, inst, t)
        o.close()
        # ... and main rays meet it, where the path ends: fewer rays per path than the same set without it
        assert counters["closest_rays"] < vp.reference_paths(vp.case_text("fog"))[1]["closest_rays"]
    if case == "pane":
        flags = [view.instances[i].handle.x & 1023 for i in range(view.instance_count)]
        assert all(f & HAS_SURFACE and not f & HAS_MEDIUM for f in flags)


@pytest.mark.parametrize("case", vp.CASES)
def test_judge_accepts_the_other_oracle_builds(case, tmp_path_factory):
    _, ref, _ = _reference(case, tmp_path_factory)
    for build in list(ref)[1:]:
        verdict = vp.judge(ref, ref[build])
        assert verdict.accepted() and verdict.largest_agreeing <= vp.SURE_TOL, (case, build, str(verdict))


def _altered_film(kind, plain):
    film = plain.copy()
    nonzero = np.argwhere(np.abs(plain[..., :3]).max(axis=-1) > 0)
    if kind == "zeroed":  # 0.5 % of the non-zero paths
        pick = nonzero[np.random.default_rng(7).choice(len(nonzero), max(1, round(0.005 * len(nonzero))), replace=False)]
        film[pick[:, 0], pick[:, 1], pick[:, 2], :3] = 0
    elif kind == "scaled":
        film[..., :3] *= np.float32(1 + 3e-4)
    elif kind == "count":
        s, y, x = nonzero[len(nonzero) // 2]
        film[s, y, x, 3] = 0
    return film


MISTAKES = {
    # name: (case, the arguments of open_set that plant it)
    "g_negated": ("fog", {"fog": (vp.FOG_A, vp.FOG_S, -0.4)}),
    "g_takes_the_other_branch": ("isotropic", {"fog": (vp.FOG_A, vp.FOG_S, 0.002)}),
    "sigma_a_and_sigma_s_swapped": ("fog", {"fog": ("0.0003", vp.FOG_A, vp.FOG_G)}),
    "one_sigma_channel_times_1_01": ("fog", {"fog": (vp.FOG_A, "0.0003, 0.000303, 0.0003", vp.FOG_G)}),
    "inner_eta_dropped_to_1": ("medium_box", {"extra": vp.INNER.replace("eta { 1.3 }", "eta { 1 }") + vp.SKIN}),
    "nested3_priorities_in_list_order": ("nested3", {"extra": vp.nested3((0, 1, 2))}),
    "rr_depth_off_by_one": ("rr_first_vertex", {"rr_depth": 2}),
    "disney_replaced_by_white_lambert": ("disney", {"tall": "white"}),
    "mix_replaced_by_white_lambert": ("mix", {"tall": "white"}),
    "layered_replaced_by_white_lambert": ("layered", {"tall": "white"}),
}


@pytest.mark.parametrize("mistake", list(MISTAKES) + ["sample_index_shifted", "half_a_percent_zeroed", "scaled_by_1_0003", "one_count_zero"])
def test_judge_rejects_planted_mistakes(mistake, tmp_path_factory):
    """More than the two disagreeing paths the device is allowed, for every mistake but the single count set to 0, which is one path by
    construction: the judge names that very path."""
    case, changes = MISTAKES.get(mistake, ("fog", None))
    _, ref, _ = _reference(case, tmp_path_factory)
    if changes is not None:
        altered = vp.case_text(case, **changes)
        assert "eta { 1 }" in altered or mistake != "inner_eta_dropped_to_1"
        device, _ = vp.oracle_paths(altered)
    elif mistake == "sample_index_shifted":
        device, _ = vp.oracle_paths(vp.case_text(case), first=1)
    else:
        device = _altered_film({"half_a_percent_zeroed": "zeroed", "scaled_by_1_0003": "scaled", "one_count_zero": "count"}[mistake], ref["plain"])
    verdict = vp.judge(ref, device)
    print(f"{mistake} on {case}: {len(verdict.disagreeing)} of {verdict.sure} SURE paths disagree")
    assert not verdict.accepted()
    if mistake == "one_count_zero":
        (s, y, x, oracle, dev), = verdict.disagreeing
        assert oracle[3] == 1 and dev[3] == 0 and np.array_equal(oracle[:3], dev[:3])
    else:
        assert not verdict.accepted(allowed=2)
    if mistake == "scaled_by_1_0003":
        assert len(verdict.disagreeing) == verdict.sure_nonzero
