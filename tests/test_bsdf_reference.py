"""The reference side of the BSDF-query tests (tests/bsdf_reference.py), checked without a GPU: the inputs are what they are said to be, the
exclusion rule leaves out few records, and the oracle answers enough of the sample-mode records for a comparison to mean something."""
import re

import numpy as np
import pytest

import bsdf_reference as B
from helpers import MATERIALS
from luisarender_amd import Scene

SERVED = B.DETERMINISTIC + B.LAYERED


def test_every_material_is_in_exactly_one_group():
    assert sorted(SERVED + B.NESTED) == sorted(MATERIALS) and len(set(SERVED + B.NESTED)) == len(MATERIALS)
    assert set(B.CLASS_OF) == set(B.DETERMINISTIC) and set(B.CLASS_OF.values()) == {"basic", "disney", "mix"}
    for table in (B.MEASURED_EVALUATE_F, B.MEASURED_EVALUATE_PDF, B.MEASURED_SAMPLE_F, B.MEASURED_SAMPLE_PDF, B.MEASURED_SAMPLE_WI):
        assert set(table) == {"basic", "disney", "mix"}
        assert all(0.0 <= v <= B.LARGEST_SOUND_ERROR / B.MARGIN for v in table.values())  # no bar above what would be a bug


@pytest.mark.parametrize("name", SERVED)
def test_inputs(name):
    inp = B.inputs(name)
    wo, wi, u = inp["wo"], inp["wi"], inp["u"]
    assert wo.shape == wi.shape == u.shape == (B.COUNT, 3) and B.COUNT % 256 == 3 and B.COUNT > 256
    assert all(a.dtype == np.float32 for a in (wo, wi, u))
    for d in (wo, wi):  # unit to rounding: the device takes such a direction bit for bit
        assert np.abs(np.einsum("nk,nk->n", d.astype(np.float64), d.astype(np.float64)) - 1.0).max() < 4e-7
    theta = np.arccos(np.abs(wo[:, 2].astype(np.float64)))
    assert 0.049 < theta.min() and theta.max() < 1.451
    below = (wo[:, 2] < 0).mean()
    assert (0.4 < below < 0.6) if name in B.TRANSMISSIVE else below == 0.0
    assert 0.4 < (wi[:, 2] < 0).mean() < 0.6 and abs(wi[:, 2].mean()) < 0.1  # the whole sphere
    assert (u >= 0).all() and (u < 1).all()
    if name.startswith("mix"):
        assert u[:, 0].max() < (0.3 if name == "mix" else 0.6)
    assert inp is B.inputs(name)  # computed once, shared, read-only
    with pytest.raises(ValueError):
        wo[0, 0] = 0.0
    # the hand-made records stand inside the quad, and their rays look at them from wo
    p, rays, rec = B.points(name), B.rays(name), B.hit_records(name)
    assert np.abs(p[:, 2]).max() == 0.0 and np.abs(p[:, 0:2]).max() < 1.0
    assert (inp["bary"] > 0).all() and (inp["bary"].sum(axis=1) < 1).all()
    assert np.array_equal(rays[:, 4:7], -wo) and np.abs(rays[:, 0:3] - wo.astype(np.float64) - p).max() < 1e-6
    assert (rec.view(np.uint32)[:, 5] == B.INVALID).all() and set(rec.view(np.uint32)[:, 4].tolist()) == {0, 1}


def test_the_comparison_scene_is_a_quad_in_the_z_plane_without_uvs():
    scene = Scene.from_string(B.scene_text("matte"), build_accel=False)
    v = scene.view()
    assert v.instance_count == 1
    assert (v.instances[0].handle.x & 2) == 0  # LR_SHAPE_HAS_VERTEX_UV: the device takes the fallback frame
    positions, _ = scene.mesh_vertices(0)
    assert np.array_equal(positions, np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32))


@pytest.mark.parametrize("name", SERVED)
def test_the_rule_leaves_out_few_records_and_the_oracle_samples_most(name):
    ref = B.oracle_answers(name)
    assert ref is B.oracle_answers(name)
    # (a failed sample, pdf = 0, may carry NaN in f and wi: Glass after a total internal reflection)
    assert np.isfinite(ref["evaluate"]).all() and np.isfinite(ref["sample"][:, 3]).all() and np.isfinite(ref["sample"][ref["sample"][:, 3] > 0]).all()
    for mode in ("evaluate", "sample"):
        assert B.excluded(name, mode).mean() <= 0.05, mode
    sampled = ref["sample"][:, 3] > 0.0
    assert sampled.mean() >= 0.5
    wi = ref["sample"][sampled, 4:7].astype(np.float64)
    assert np.abs(np.linalg.norm(wi, axis=1) - 1.0).max() < 1e-4
    assert set(ref["sample"][:, 7].astype(int).tolist()) <= {0, 1, 2, 4}
    # evaluate: wi covers the sphere, so the opaque closures answer about half the records and no material answers none
    assert (ref["evaluate"][:, 3] > 0.0).mean() > 0.3


@pytest.mark.parametrize("name", sorted(B.MIX_ROOT_RATIO))
def test_the_sample_b_inputs(name):
    """the Mix materials once more with lobe numbers of the root's "sample b" branch: the ratio is the scene's, the rule leaves out few
    records and the oracle samples most of them"""
    assert set(B.MIX_ROOT_RATIO) == {m for m in B.DETERMINISTIC if m.startswith("mix")}
    root = MATERIALS[name][MATERIALS[name].index("Surface m : Mix"):]
    assert float(re.search(r"ratio : Constant \{ v \{ ([0-9.]+) \} \}", root).group(1)) == B.MIX_ROOT_RATIO[name]
    inp, again = B.sample_b_inputs(name), B.inputs(name)
    u = inp["u"]
    assert u.dtype == np.float32 and (u[:, 0] >= np.float32(B.MIX_ROOT_RATIO[name])).all() and (u < 1).all()
    assert np.array_equal(u[:, 1:], again["u"][:, 1:]) and all(inp[k] is again[k] for k in ("wo", "wi", "prim", "bary"))
    ref = B.oracle_sample_b(name)
    assert ref is B.oracle_sample_b(name)
    sampled = ref[:, 3] > 0.0
    assert np.isfinite(ref[:, 3]).all() and np.isfinite(ref[sampled]).all() and sampled.mean() >= 0.5
    assert B.excluded(name, "sample_b").mean() <= 0.05
    assert not np.array_equal(ref, B.oracle_answers(name)["sample"])
    for v in (B.MEASURED_SAMPLE_B_F, B.MEASURED_SAMPLE_B_PDF, B.MEASURED_SAMPLE_B_WI):
        assert 0.0 <= v <= B.LARGEST_SOUND_ERROR / B.MARGIN


def test_relative_error_and_the_invalid_record():
    assert np.allclose(B.relative_error([1.1, 0.001, -2.0], [1.0, 0.0, -2.5]), [0.1, 0.1, 0.2])
    assert B.invalid_record().tolist() == [0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF]
