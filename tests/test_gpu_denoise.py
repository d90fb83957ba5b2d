"""The denoiser of DESIGN §4.8 on the device: lrhip_denoise over synthetic frames against the float64 numpy restatement
(tests/denoise_reference.py) and the filter's own properties, lrhip_aov_denoise over rendered buffers, and the CLI plugin's files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from denoise_reference import (DEVICE_BAR, MEASURED_DEVICE_ERROR, SIZES, SYNTHETIC_PARAMS, edge_case, relative_error, synthetic,
                               synthetic_reference, ulp_distance)
from luisarender_amd import Scene
from luisarender_amd.render import DeviceError, MegaPathRenderer, aov_file_name
from luisarender_amd.scene import load_image
from luisarender_amd.scenes import cornell_box

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "luisarender_amd", "bin", "luisa-render-cli")
LRHIP_ERROR_INVALID = -1


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def _cornell_aov(props="", resolution=64, spp=8, depth=5, **kw):
    text = cornell_box(resolution=resolution, spp=spp, depth=depth, rr_depth=100, **kw)
    return text.replace(f"integrator : MegaPath {{ depth {{ {depth} }}  rr_depth {{ 100 }}", f"integrator : AOV {{ depth {{ {depth} }}  rr_depth {{ 100 }} {props}")


@pytest.mark.parametrize("height, width", SIZES)
def test_against_the_float64_restatement(renderer, capsys, height, width):
    """Measured on the MI355X: MEASURED_DEVICE_ERROR (denoise_reference.py) is the largest of the four sizes; the bar is 4 x that and
    at most 1e-4 -- half of what one dropped tap moves these frames by (test_denoise.py)."""
    noisy, albedo, normal, depth, _ = synthetic(height, width)
    out = renderer.denoise(noisy, albedo, normal, depth, **SYNTHETIC_PARAMS)
    err = relative_error(out, synthetic_reference(height, width))
    with capsys.disabled():
        print(f"\n[denoise] {height}x{width}: device vs float64 restatement {err:.3e} (recorded {MEASURED_DEVICE_ERROR:.1e}, bar {DEVICE_BAR:.1e})")
    assert out.dtype == np.float32 and out.shape == (height, width, 3) and np.isfinite(out).all()
    assert err <= DEVICE_BAR <= 1e-4


def test_a_constant_field_stays_constant(renderer):
    """a convex combination of equal values, whatever the guides: within 32 ulp (demodulation off)"""
    _, albedo, normal, depth, _ = synthetic(45, 70)
    const = np.ascontiguousarray(np.broadcast_to(np.array([0.37, 1.9, 0.052], np.float32), (45, 70, 3)))
    out = renderer.denoise(const, albedo, normal, depth, **{**SYNTHETIC_PARAMS, "demodulate": False})
    assert ulp_distance(out, const).max() <= 32


def test_no_bleeding_across_a_hard_edge(renderer):
    """orthogonal normals under sigma_normal 0.1: the cross weight is exp(-200) = 0 in float32, so side A's output has the same bits
    whatever side B's colours are"""
    color, other, albedo, normal, depth = edge_case()
    params = {**SYNTHETIC_PARAMS, "sigma_normal": 0.1}
    a = renderer.denoise(color, albedo, normal, depth, **params)
    b = renderer.denoise(other, albedo, normal, depth, **params)
    half = color.shape[1] // 2
    assert np.array_equal(a[:, :half], b[:, :half]) and not np.array_equal(a[:, half:], b[:, half:])
    assert not np.array_equal(a[:, :half], color[:, :half])  # side A was filtered


def test_deterministic(renderer):
    noisy, albedo, normal, depth, _ = synthetic(45, 70)
    first = renderer.denoise(noisy, albedo, normal, depth, **SYNTHETIC_PARAMS)
    small = renderer.denoise(*synthetic(7, 9)[:4], **SYNTHETIC_PARAMS)  # another size in between: the buffers are reused
    assert np.array_equal(renderer.denoise(noisy, albedo, normal, depth, **SYNTHETIC_PARAMS), first)
    assert np.array_equal(renderer.denoise(*synthetic(7, 9)[:4], **SYNTHETIC_PARAMS), small)


def test_invalid_calls_are_errors_and_leave_the_context_usable(renderer):
    lib, ctx = renderer._lib, renderer._ctx
    noisy, albedo, normal, depth, _ = synthetic(7, 9)
    before = renderer.denoise(noisy, albedo, normal, depth, **SYNTHETIC_PARAMS)
    out = np.empty((7, 9, 3), np.float32)
    arrays = [noisy.ctypes.data, albedo.ctypes.data, normal.ctypes.data, depth.ctypes.data, out.ctypes.data]
    good = renderer._denoise_params(9, 7)
    assert lib.lrhip_denoise(ctx, C.byref(good), *arrays) == 0
    for k in range(5):  # each array NULL in turn
        assert lib.lrhip_denoise(ctx, C.byref(good), *[None if j == k else a for j, a in enumerate(arrays)]) == LRHIP_ERROR_INVALID
    assert lib.lrhip_denoise(ctx, None, *arrays) == LRHIP_ERROR_INVALID
    assert lib.lrhip_denoise(None, C.byref(good), *arrays) == LRHIP_ERROR_INVALID
    for bad in (renderer._denoise_params(9, 7, iterations=0), renderer._denoise_params(9, 7, iterations=9), renderer._denoise_params(0, 7),
                renderer._denoise_params(9, 0), renderer._denoise_params(9, 7, sigma_color=0.0), renderer._denoise_params(9, 7, sigma_depth=-1.0)):
        assert lib.lrhip_denoise(ctx, C.byref(bad), *arrays) == LRHIP_ERROR_INVALID
    # lrhip_aov_denoise: a scene without albedo, samples = 0, a size that is not the scene's, a first-hit component, NULL
    frame = np.empty((32, 32, 3), np.float32)
    auto = renderer._denoise_params(0, 0)
    renderer.upload(Scene.from_string(_cornell_aov('components { "sample", "normal", "depth" }', resolution=32)))
    renderer.render(0, 8, sync=True)
    assert lib.lrhip_aov_denoise(ctx, C.byref(auto), 0, 8, frame.ctypes.data) == LRHIP_ERROR_INVALID
    assert "'albedo' is not enabled" in lib.lrhip_last_error().decode()
    with pytest.raises(DeviceError, match="albedo"):
        renderer.denoise_aov("sample")
    renderer.upload(Scene.from_string(_cornell_aov(resolution=32)))
    renderer.render(0, 8, sync=True)
    assert lib.lrhip_aov_denoise(ctx, C.byref(auto), 0, 0, frame.ctypes.data) == LRHIP_ERROR_INVALID
    assert lib.lrhip_aov_denoise(ctx, C.byref(renderer._denoise_params(16, 32)), 0, 8, frame.ctypes.data) == LRHIP_ERROR_INVALID
    assert lib.lrhip_aov_denoise(ctx, C.byref(auto), 3, 8, frame.ctypes.data) == LRHIP_ERROR_INVALID
    assert lib.lrhip_aov_denoise(ctx, C.byref(renderer._denoise_params(0, 0, iterations=9)), 0, 8, frame.ctypes.data) == LRHIP_ERROR_INVALID
    assert lib.lrhip_aov_denoise(ctx, C.byref(auto), 0, 8, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_aov_denoise(ctx, C.byref(renderer._denoise_params(32, 32)), 0, 8, frame.ctypes.data) == 0  # the scene's own size is fine
    assert np.array_equal(frame, renderer.denoise_aov("sample")) and np.isfinite(frame).all()
    assert np.array_equal(renderer.denoise(noisy, albedo, normal, depth, **SYNTHETIC_PARAMS), before)


# ---- rendered buffers: the Cornell box under AOV, 64 x 64, all components


@pytest.fixture(scope="module")
def cornell(renderer):
    """16 spp on the device, its downloaded means, and the 2048-spp `sample` of the same scene; rendered once"""
    scene = Scene.from_string(_cornell_aov("noisy_count { 16 }", spp=16))
    renderer.upload(scene)
    renderer.render(0, 2048, sync=True)
    converged = renderer.download_aov("sample")
    renderer.clear()
    renderer.render(0, 16, sync=True)
    means = {c: renderer.download_aov(c) for c in ("sample", "diffuse", "albedo", "normal", "depth")}
    return scene, means, converged


@pytest.mark.parametrize("component", ["sample", "diffuse"])
def test_device_resident_sums_equal_the_downloaded_means(renderer, cornell, component):
    """lrhip_aov_denoise reads the planar sums and scales them by float(1 / n) in the prepare kernel -- the product download_aov forms on
    the host -- and from there on runs the same kernels on the same floats: the same bits"""
    scene, means, _ = cornell
    assert renderer._scene is scene and renderer._aov_samples == 16  # the fixture's 16 spp are still on the device
    on_device = renderer.denoise_aov(component)
    through_host = renderer.denoise(means[component], means["albedo"], means["normal"], means["depth"])
    assert np.array_equal(on_device, through_host)
    assert not np.array_equal(on_device, means[component])
    other = renderer.denoise_aov(component, iterations=2, demodulate=False, sigma_color=1.5)
    assert np.array_equal(other, renderer.denoise(means[component], means["albedo"], means["normal"], means["depth"], iterations=2,
                                                  demodulate=False, sigma_color=1.5))
    assert not np.array_equal(other, on_device)


def test_quality_on_a_rendered_frame(renderer, cornell, capsys):
    """16 spp denoised with the defaults against 2048 spp of the same scene: the filter must bring the frame closer.  Measured on the
    MI355X with the defaults (sigma_color 0.9): RMSE 0.1024 noisy, 0.0998 denoised, ratio 0.975 (the sweep: DESIGN 4.8)"""
    _, means, converged = cornell
    denoised = renderer.denoise(means["sample"], means["albedo"], means["normal"], means["depth"])
    rmse = lambda x: float(np.sqrt(((x.astype(np.float64) - converged) ** 2).mean()))
    noisy_rmse, denoised_rmse = rmse(means["sample"]), rmse(denoised)
    with capsys.disabled():
        print(f"\n[denoise] Cornell 64x64, 16 spp against 2048 spp: RMSE noisy {noisy_rmse:.4f}, denoised {denoised_rmse:.4f}, "
              f"ratio {denoised_rmse / noisy_rmse:.3f}; {renderer.last_denoise_ms():.3f} ms")
    assert denoised_rmse < noisy_rmse


def test_cli_writes_the_denoised_file(tmp_path):
    """denoise { true } dump { "final" }: <stem>_denoised.exr beside the component files, holding what denoise_aov("sample") gives for
    the same launches (one per sample, as the plugin's loop renders) -- FLOAT EXR channels: the same bits"""
    props = 'noisy_count { 8 } denoise { true } denoise_iterations { 4 } components { "sample", "albedo", "normal", "depth" } dump { "final" }'
    scene_file = tmp_path / "cornell.luisa"
    scene_file.write_text(_cornell_aov(props, resolution=48, spp=8, file="out.exr"))
    r = subprocess.run([CLI, "-b", "hip", "-d", "0", str(scene_file)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert set(os.listdir(tmp_path)) == {"cornell.luisa", "out_denoised.exr"} | {f"out_{c}.exr" for c in ("sample", "albedo", "normal", "depth")}
    sc = Scene.load(str(scene_file))
    settings = sc.aov_settings()
    assert settings["denoise"]["iterations"] == 4
    rd = MegaPathRenderer(0)
    try:
        rd.upload(sc)
        rd.clear()
        for n in range(8):
            rd.render(n, n + 1, shutter_weight=1.0, sync=True)
        want = rd.denoise_aov("sample", **settings["denoise"])
        noisy = rd.download_aov("sample")
    finally:
        rd.close()
    img, _ = load_image(str(tmp_path / "out_denoised.exr"))
    assert np.array_equal(img[..., :3], want)
    sample, _ = load_image(aov_file_name(str(tmp_path / "out.exr"), "sample", 8, "final"))
    assert np.array_equal(sample[..., :3], noisy) and not np.array_equal(want, noisy)
