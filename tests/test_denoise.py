"""The denoiser of DESIGN §4.8 on the host: what the scene loader makes of the AOV integrator's `denoise...` properties, the C ABI's
new symbols and struct, and the numpy restatement the GPU tests compare the device with (tests/denoise_reference.py) held to the
filter's own properties.  No GPU needed; tests/test_gpu_denoise.py runs the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from denoise_reference import DEFAULTS, DEVICE_BAR, SIZES, SYNTHETIC_PARAMS, atrous, edge_case, synthetic, synthetic_reference, ulp_distance
from luisarender_amd import Scene, _ffi
from luisarender_amd.scene import HostError
from luisarender_amd.scenes import cornell_box


def _aov(props=""):
    text = cornell_box(resolution=16, spp=4).replace("integrator : MegaPath { depth { 8 }  rr_depth { 0 }", f"integrator : AOV {{ {props}")
    return Scene.from_string(text, build_accel=False)


def test_denoise_is_off_by_default_and_its_defaults_are_the_headers():
    sc = _aov()
    assert sc.aov_denoise() == {"enabled": False, **{k: pytest.approx(v) for k, v in DEFAULTS.items()}}
    assert "denoise" not in sc.aov_settings()  # a scene that does not ask for it reads as before
    on = _aov("denoise { true }")
    assert on.aov_denoise()["enabled"] and on.aov_settings()["denoise"] == {k: pytest.approx(v) for k, v in DEFAULTS.items()}
    header = open(os.path.join(_ffi.REPO_ROOT, "include", "lrhip.h")).read()
    fixed = dict(re.findall(r"#define LRHIP_DENOISE_DEFAULT_(\w+) ([0-9.]+)[uf]", header))
    assert {k.lower(): float(v) for k, v in fixed.items()} == {k: float(v) for k, v in DEFAULTS.items() if k != "demodulate"}


def test_the_properties_round_trip():
    sc = _aov("denoise { true } denoise_iterations { 3 } denoise_sigma_color { 2.5 } denoise_sigma_normal { 0.125 } "
              "denoise_sigma_depth { 0.25 } denoise_demodulate { false } noisy_count { 16 } dump { \"final\" }")
    settings = sc.aov_settings()
    assert settings["denoise"] == {"iterations": 3, "sigma_color": 2.5, "sigma_normal": 0.125, "sigma_depth": 0.25, "demodulate": False}
    assert settings["noisy_count"] == 16 and settings["dump"] == "final" and len(settings["components"]) == 9
    # the settings are parsed whether or not the filter is switched on
    off = _aov("denoise_iterations { 7 } denoise_sigma_depth { 0.5 }").aov_denoise()
    assert not off["enabled"] and off["iterations"] == 7 and off["sigma_depth"] == 0.5 and off["demodulate"]


@pytest.mark.parametrize("components, missing", [('"sample"', "albedo"), ('"albedo", "normal", "depth"', "sample"),
                                                 ('"sample", "albedo", "depth", "mask"', "normal"), ('"sample", "albedo", "normal"', "depth")])
def test_denoise_without_a_needed_component_fails_at_load(components, missing):
    with pytest.raises(HostError, match=f"needs the AOV component '{missing}'"):
        _aov(f"denoise {{ true }} components {{ {components} }}")
    _aov(f"components {{ {components} }}")  # fine without denoise


def test_invalid_settings_fail_at_load_only_when_switched_on():
    for props in ("denoise_iterations { 0 }", "denoise_iterations { 9 }", "denoise_sigma_color { 0 }", "denoise_sigma_normal { -1 }"):
        with pytest.raises(HostError, match="denoise_"):
            _aov("denoise { true } " + props)
        _aov(props)
    with pytest.raises(HostError, match="not AOV"):
        Scene.from_string(cornell_box(resolution=16, spp=4), build_accel=False).aov_denoise()


def test_the_new_symbols_are_exported_and_the_struct_matches():
    hip = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))  # loads without a GPU; only the device-free call is made
    for name in ("lrhip_denoise", "lrhip_aov_denoise", "lrhip_denoise_default_params", "lrhip_last_denoise_ms"):
        assert hasattr(hip, name), name
    assert hasattr(_ffi.host_lib(), "lrhost_scene_aov_denoise")
    assert C.sizeof(_ffi.DenoiseParams) == 28 == _ffi.host_lib().lrhost_sizeof(b"lrhip_denoise_params")
    p = _ffi.DenoiseParams(1, 2, 3, 4, 5.0, 6.0, 7.0)
    hip.lrhip_denoise_default_params.restype = None
    hip.lrhip_denoise_default_params(C.byref(p))
    assert (p.width, p.height, p.iterations, p.flags) == (0, 0, 5, _ffi.DENOISE_DEMODULATE)
    assert (p.sigma_color, p.sigma_normal, p.sigma_depth) == tuple(np.float32(DEFAULTS[k]) for k in ("sigma_color", "sigma_normal", "sigma_depth"))


# ---- the numpy restatement by itself


def test_restatement_float32_against_float64():
    """the definition is well conditioned: a float32 run of it stays within 1e-6 of the largest value of the float64 one"""
    for h, w in SIZES:
        noisy, albedo, normal, depth, _ = synthetic(h, w)
        ref = synthetic_reference(h, w)
        f32 = atrous(noisy, albedo, normal, depth, dtype=np.float32, **SYNTHETIC_PARAMS)
        assert f32.dtype == np.float32 and np.abs(f32 - ref).max() <= 1.0e-6 * np.abs(ref).max(), (h, w)


def test_restatement_is_sensitive_to_one_tap_and_one_step():
    """What the device's bar rests on: leaving the (2, 2) tap of pass 0 out moves the synthetic frames by at least twice DEVICE_BAR of
    their largest value, a step of 3 instead of 4 in pass 2 by more than a hundred times that -- so a kernel within the bar has every
    tap and every step right."""
    for h, w in SIZES[:2]:
        noisy, albedo, normal, depth, _ = synthetic(h, w)
        ref = synthetic_reference(h, w)
        tap = np.abs(atrous(noisy, albedo, normal, depth, drop_tap=(0, 2, 2), **SYNTHETIC_PARAMS) - ref).max() / np.abs(ref).max()
        step = np.abs(atrous(noisy, albedo, normal, depth, steps=[1, 2, 3, 8, 16], **SYNTHETIC_PARAMS) - ref).max() / np.abs(ref).max()
        print(f"[denoise] {h}x{w}: dropped tap {tap:.2e}, wrong step {step:.2e} of the largest value")
        assert tap >= 2 * DEVICE_BAR and step >= 4.5e-2, (h, w, tap, step)


def test_restatement_denoises_the_synthetic_frames():
    for h, w in SIZES[:2]:
        noisy, _, _, _, clean = synthetic(h, w)
        rmse = lambda x: float(np.sqrt(((x - clean) ** 2).mean()))
        assert rmse(noisy) > 0.1 and rmse(synthetic_reference(h, w)) < 0.4 * rmse(noisy), (h, w)
    noisy, albedo, _, _, _ = synthetic(1, 1)
    assert np.allclose(synthetic_reference(1, 1), noisy, rtol=1e-6)  # one pixel: its own centre tap


def test_restatement_keeps_a_constant_field():
    """a convex combination of equal values: the constant, whatever the guides do (demodulation off)"""
    _, albedo, normal, depth, _ = synthetic(23, 37)
    const = np.broadcast_to(np.array([0.37, 1.9, 0.052], np.float32), (23, 37, 3))
    out64 = atrous(const, albedo, normal, depth, **{**SYNTHETIC_PARAMS, "demodulate": False})
    assert np.abs(out64 / const.astype(np.float64) - 1).max() < 1e-14
    out32 = atrous(const, albedo, normal, depth, dtype=np.float32, **{**SYNTHETIC_PARAMS, "demodulate": False})
    assert ulp_distance(out32, const).max() <= 32


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_does_not_bleed_across_a_hard_edge(dtype):
    """orthogonal normals under sigma_normal 0.1: the cross weight is exp(-200) -- zero in float32, 1e-87 (far below an ulp of the sums)
    in float64 -- so side A's output does not depend on side B's colours"""
    color, other, albedo, normal, depth = edge_case()
    params = {**SYNTHETIC_PARAMS, "sigma_normal": 0.1}
    a = atrous(color, albedo, normal, depth, dtype=dtype, **params)
    b = atrous(other, albedo, normal, depth, dtype=dtype, **params)
    half = color.shape[1] // 2
    assert np.array_equal(a[:, :half], b[:, :half]) and not np.array_equal(a[:, half:], b[:, half:])
    # ... and with the normals equal it does
    flat = np.broadcast_to(np.array([0, 1, 0], np.float32), normal.shape)
    assert not np.array_equal(atrous(color, albedo, flat, depth, dtype=dtype, **params)[:, :half],
                              atrous(other, albedo, flat, depth, dtype=dtype, **params)[:, :half])
