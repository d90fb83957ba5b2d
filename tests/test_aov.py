"""The AOV integrator (src/integrators/aov.cpp) on the host: what the scene loader makes of `integrator : AOV { ... }`
(aov.cpp:48-87), the dump schedule and file names of its render loop (aov.cpp:380-433), and the 1- / 3-channel image writer
behind those files.  No GPU needed; tests/test_gpu_aov.py renders."""
import os

import numpy as np
import pytest

from luisarender_amd import Scene
from luisarender_amd.render import aov_dump_counts, aov_file_name
from luisarender_amd.scene import AOV_COMPONENTS, HostError, load_image, save_image
from luisarender_amd.scenes import cornell_box

LR_INTEGRATOR_AOV = 4


def _aov(props=""):
    text = cornell_box(resolution=16, spp=4).replace("integrator : MegaPath { depth { 8 }  rr_depth { 0 }", f"integrator : AOV {{ {props}")
    return Scene.from_string(text, build_accel=False)


def test_defaults():
    sc = _aov()
    v = sc.view()
    assert v.integrator.kind == LR_INTEGRATOR_AOV and v.integrator.max_depth == 10
    assert v.integrator.flags == 0x1FF  # "all": one LR_AOV_* bit per component
    assert sc.aov_settings() == {"components": list(AOV_COMPONENTS), "noisy_count": 8, "dump": "power2", "depth": 10}
    assert v.sampler.spp == 8  # noisy_count, not the camera's 4, is what the sampler is reset with (aov.cpp:205-216)


def test_clamping_and_the_unused_russian_roulette_settings():
    sc = _aov("depth { 0 } noisy_count { 3 } rr_depth { 2 } rr_threshold { 0.01 }")
    v = sc.view()
    assert v.integrator.max_depth == 1 and sc.aov_settings()["noisy_count"] == 8  # max(.., 1), max(.., 8)
    assert v.integrator.rr_depth == 2 and v.integrator.rr_threshold == pytest.approx(0.05)  # parsed like MegaPath's, never used
    sc = _aov("depth { 3 } noisy_count { 10 }")
    assert sc.view().integrator.max_depth == 3 and sc.aov_settings()["noisy_count"] == 10 and sc.view().sampler.spp == 10


def test_components_case_all_and_unknown_names(capfd):
    sc = _aov('components { "Albedo", "NORMAL", "depth", "fancy" }')
    assert sc.view().integrator.flags == (1 << 4) | (1 << 3) | (1 << 5)
    assert sc.aov_settings()["components"] == ["normal", "albedo", "depth"]
    assert "Ignoring unknown AOV component 'fancy'" in capfd.readouterr().err
    assert _aov('components { "mask", "ALL" }').view().integrator.flags == 0x1FF
    assert _aov('components { "roughness", "ndc", "mask", "sample", "diffuse", "specular" }').view().integrator.flags == \
        (1 << 6) | (1 << 7) | (1 << 8) | 1 | 2 | 4
    assert _aov('components { "fancy" }').view().integrator.flags == 0  # nothing enabled: the loader warns, nothing is written


def test_dump_strategies(capfd):
    for text, want in (('"all"', "all"), ('"Final"', "final"), ('"POWER2"', "power2")):
        assert _aov(f"dump {{ {text} }}").aov_settings()["dump"] == want
    capfd.readouterr()
    assert _aov('dump { "sometimes" }').aov_settings()["dump"] == "power2"
    assert "Unknown dump strategy 'sometimes'. Fallback to power2 strategy." in capfd.readouterr().err


def test_settings_of_another_integrator_are_an_error():
    with pytest.raises(HostError, match="not AOV"):
        Scene.from_string(cornell_box(resolution=16, spp=4), build_accel=False).aov_settings()


def test_dump_schedule_and_file_names():
    """should_dump (aov.cpp:383-392) and the paths of :418-421"""
    assert aov_dump_counts(8, "power2") == [1, 2, 4, 8]
    assert aov_dump_counts(10, "power2") == [1, 2, 4, 8]  # no file at 10
    assert aov_dump_counts(8, "all") == list(range(1, 9)) and aov_dump_counts(10, "all") == list(range(1, 11))
    assert aov_dump_counts(8, "final") == [8] and aov_dump_counts(10, "final") == [10]
    assert aov_file_name("/out/render.exr", "albedo", 8, "power2") == "/out/render_albedo_00008.exr"
    assert aov_file_name("/out/render.exr", "albedo", 10, "all") == "/out/render_albedo_00010.exr"
    assert aov_file_name("/out/render.exr", "depth", 10, "final") == "/out/render_depth.exr"
    assert aov_file_name("render.hdr", "mask", 123, "power2") == "render_mask_00123.hdr"


@pytest.mark.parametrize("ext", [".exr", ".hdr"])
def test_one_and_three_channel_images(tmp_path, ext):
    rng = np.random.default_rng(7)
    rgb = rng.uniform(0.05, 4.0, (5, 7, 3)).astype(np.float32)
    gray = rng.uniform(0.05, 4.0, (5, 7)).astype(np.float32)
    save_image(str(tmp_path / f"rgb{ext}"), rgb)
    save_image(str(tmp_path / f"gray{ext}"), gray)
    img, _ = load_image(str(tmp_path / f"rgb{ext}"))
    one, _ = load_image(str(tmp_path / f"gray{ext}"))
    assert img.shape == (5, 7, 4) and (img[..., 3] == 1).all()
    if ext == ".exr":  # FLOAT channels B, G, R: exact
        assert np.array_equal(img[..., :3], rgb)
        # a lone channel is named "A", as tinyexr's SaveEXR names it; the project's reader takes an "A" channel as alpha
        assert np.array_equal(one[..., 3], gray) and (one[..., :3] == 0).all()
    else:  # RGBE: 8 mantissa bits shared by the three channels; one channel is written as gray
        assert (np.abs(img[..., :3] - rgb) <= rgb.max(axis=-1, keepdims=True) * 2.0 ** -7).all()
        assert (np.abs(one[..., 0] - gray) <= gray * 2.0 ** -7).all()
        assert np.array_equal(one[..., 0], one[..., 1]) and np.array_equal(one[..., 0], one[..., 2])


def test_other_extensions_fall_back_to_exr(tmp_path, capfd):
    rgb = np.full((2, 3, 3), 0.5, np.float32)
    save_image(str(tmp_path / "x.png"), rgb)
    assert os.path.exists(tmp_path / "x.exr") and not os.path.exists(tmp_path / "x.png")
    assert "Falling back to '.exr'" in capfd.readouterr().err
    img, _ = load_image(str(tmp_path / "x.exr"))
    assert np.array_equal(img[..., :3], rgb)
