"""The AOV integrator (src/integrators/aov.cpp) on the device: the kFeatAov kernels through lrhip_aov_download, and the CLI plugin.
The oracle has no AOV integrator, so the buffers are pinned through relations and closed forms: `sample` is MegaPath's film of the
same paths, the light split adds up, the first-hit buffers are restated per sample from the oracle's own camera rays and closest
hits, albedo / roughness follow the closure table of the reference's surfaces, and the sums are bit-reproducible under sharding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from luisarender_amd import Scene
from luisarender_amd.render import MegaPathRenderer, aov_dump_counts, aov_file_name
from luisarender_amd.scene import load_image
from luisarender_amd.scenes import cornell_box
from oracle.check import Oracle

pytestmark = pytest.mark.gpu

AOV, SCENE_MASK = 32768, 4 | 8 | 16 | 32 | 64  # LRHIP_FEAT_AOV; the all-closures scene bits its kernels are built on
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "luisarender_amd", "bin", "luisa-render-cli")


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def _cornell_aov(props="", resolution=48, spp=8, depth=5, **kw):
    """the Cornell box with rr_depth beyond depth (no Russian roulette on either side) under the AOV integrator"""
    text = cornell_box(resolution=resolution, spp=spp, depth=depth, rr_depth=100, **kw)
    return text.replace(f"integrator : MegaPath {{ depth {{ {depth} }}  rr_depth {{ 100 }}", f"integrator : AOV {{ depth {{ {depth} }}  rr_depth {{ 100 }} {props}")


def _render(renderer, scene, spp, **kw):
    renderer.upload(scene)
    renderer.render(0, spp, sync=True, **kw)
    return {c: renderer.download_aov(c, normalized=False) for c in scene.aov_settings()["components"]}


def test_sample_is_the_megapath_film_of_the_same_paths(renderer, capsys):
    """No Russian roulette on either side and the film's clamp (256) out of reach: `sample` sums MegaPath's Li.  The MegaPath frame is
    rendered on the all-closures one-path-per-lane kernel <124> (set_diagnostics), the family the AOV kernel belongs to: same chunking, the
    same order of adds per wave -- what remains is how the compiler contracted the two kernels' arithmetic"""
    spp = 16
    mega = Scene.from_string(cornell_box(resolution=64, spp=spp, depth=5, rr_depth=100))
    a = _render(renderer, Scene.from_string(_cornell_aov(f"noisy_count {{ {spp} }}", resolution=64, spp=spp)), spp)
    assert renderer.last_variant() == SCENE_MASK | AOV
    renderer.set_diagnostics(SCENE_MASK)
    try:
        renderer.upload(mega)
        renderer.render(0, spp, sync=True)
        film = renderer.download(converted=False)
        assert renderer.last_variant() == SCENE_MASK
    finally:
        renderer.set_diagnostics(0)
    rel = float(np.abs(a["sample"] - film[..., :3]).sum() / np.abs(film[..., :3]).sum())
    with capsys.disabled():
        print(f"\n[aov] sample vs the MegaPath film (<124>): bit-identical {np.array_equal(a['sample'], film[..., :3])}, rel-L1 {rel:.3e}")
    assert rel <= 1e-6
    cpu, _ = Oracle(mega).render(0, spp)
    assert float(np.abs(a["sample"] - cpu[..., :3]).sum() / np.abs(cpu[..., :3]).sum()) < 1e-4  # test_cornell_same_paths_and_image's bar


MIRROR_ENV = """
Surface m : Mirror { color : Constant { v { 0.9, 0.8, 0.7 } } }
Shape plane : InlineMesh { positions { -50,0,-50, 50,0,-50, 50,0,50, -50,0,50 } indices { 0,2,1, 0,3,2 } surface { @m } }
Camera cam : Pinhole { fov { 60 } spp { 4 } film : Color { resolution { 32, 32 } } position { 0, 5, 0 } look_at { 0, 4, -8 } }
render { cameras { @cam } shapes { @plane } environment : Spherical { emission : Constant { v { 2, 3, 4 } } } integrator : AOV { } }
"""


def test_light_split(renderer):
    """Li_diffuse accumulates while the last bounce was not specular (roughness < 0.05 in both directions, aov.cpp:360)"""
    a = _render(renderer, Scene.from_string(_cornell_aov()), 8)
    # every surface of the Cornell box is Matte (roughness 1): no bounce is specular
    assert (a["specular"] == 0).all() and np.array_equal(a["diffuse"], a["sample"])
    m = _render(renderer, Scene.from_string(MIRROR_ENV), 4)
    mirror, sky = m["mask"][..., 0] == 4, m["mask"][..., 0] == 0
    assert mirror.mean() > 0.3 and sky.mean() > 0.1
    # What the mirror shows is the environment after a specular bounce (roughness 0.01): specular.  The mirror vertex's OWN light sample
    # is taken before specular_bounce is set (aov.cpp:333-342, then :360), so `diffuse` there is that sample through the near-delta GGX
    # lobe -- not zero, but a small fraction of the pixel (measured: at most ~1e-3 of it)
    assert m["sample"][mirror].min() > 0
    assert float(m["diffuse"][mirror].sum()) < 1e-3 * float(m["sample"][mirror].sum())
    assert np.allclose(m["specular"][mirror] + m["diffuse"][mirror], m["sample"][mirror], rtol=1e-6, atol=0)
    # the sky seen directly is "diffuse" (no bounce yet)
    assert (m["specular"][sky] == 0).all() and np.array_equal(m["diffuse"][sky], m["sample"][sky])
    for x in (a, m):
        assert np.allclose(x["diffuse"] + x["specular"], x["sample"], rtol=1e-6, atol=1e-6)


PLANE_BALL = """
Surface w : Matte { Kd : Constant { v { 0.5 } } }
Shape floor : InlineMesh { positions { -50,0,-50, 50,0,-50, 50,0,50, -50,0,50 } indices { 0,2,1, 0,3,2 } surface { @w } }
Shape ball : Sphere { subdivision { 4 } surface { @w } transform : SRT { scale { 1.5, 1.5, 1.5 } translate { 0, 1.5, -6 } } }
Camera cam : Pinhole { fov { 50 } spp { 4 } film : Color { resolution { 40, 30 } } filter : Gaussian { radius { 1.5 } }
  position { 0, 3, 2 } look_at { 0, 1, -6 } }
render { cameras { @cam } shapes { @floor, @ball } environment : Spherical { emission : Constant { v { 1 } } }
  integrator : AOV { components { "mask", "depth", "ndc", "normal" } } }
"""


def test_first_hit_buffers(renderer):
    """mask, depth, ndc and normal (aov.cpp:263-270) restated sample by sample from the oracle's entry points: the camera ray of (pixel,
    sample), its closest hit on the device's baked triangles, the pixel's filter offset from the sampler's first draw.  The floor's
    normal is exact; the ball's shading normal interpolates vertex normals, held to the analytic sphere normal at the tessellation's
    accuracy.  Silhouette pixels may flip (fma contraction on the device)."""
    spp = 4
    sc = Scene.from_string(PLANE_BALL)
    a = _render(renderer, sc, spp)
    o = Oracle(sc, bake_instances=True)
    v = sc.view()
    w, h = o.width, o.height
    mask, depth = np.zeros((h, w)), np.zeros((h, w))
    ndc, normal = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    on_ball = np.zeros((h, w), bool)
    centre = np.array([0.0, 1.5, -6.0])
    m = np.ctypeslib.as_array(v.camera.camera_to_world).reshape(4, 4)  # column-major: row k = column k of the matrix
    forward = -m[2, :3] / np.linalg.norm(m[2, :3])
    stream, offset = np.zeros(2, np.float32), np.zeros(3, np.float32)
    for py in range(h):
        for px in range(w):
            for s in range(spp):
                r = o.camera_ray(px, py, s)
                inst, _, _, _, t = o.trace_closest(r[:3], r[3:6])
                if inst == 0xFFFFFFFF:
                    continue
                cos_axis = float(np.dot(r[3:6], forward))  # clip planes, camera.h:147-157
                t_range = v.camera.clip_far / cos_axis - v.camera.clip_near / cos_axis
                o._lib.oracle_sampler_stream(C.byref(v), px, py, s, 0, stream.ctypes.data)
                o._lib.oracle_filter_sample(C.byref(v.filter), float(stream[0]), float(stream[1]), offset.ctypes.data)
                fx, fy = px + 0.5 + offset[0], py + 0.5 + offset[1]
                p = r[:3].astype(np.float64) + t * r[3:6]
                mask[py, px] += 1
                depth[py, px] += t
                ndc[py, px] += (fx / w * 2 - 1, -(fy / h * 2 - 1), t / t_range)
                if inst == 1:
                    normal[py, px] += (p - centre) / np.linalg.norm(p - centre)
                    on_ball[py, px] = True
                else:
                    normal[py, px] += (0.0, 1.0, 0.0)
    same = a["mask"][..., 0] == mask
    assert same.mean() >= 0.995 and (mask == 0).any() and (mask == spp).mean() > 0.5  # sky above the horizon, floor and ball below
    close = lambda got, want, tol: (np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))).reshape(h, w, -1).all(axis=-1)
    assert (close(a["depth"][..., 0], depth, 1e-5) & same).mean() >= 0.995
    assert (close(a["ndc"], ndc, 1e-5) & same).mean() >= 0.995
    floor = same & ~on_ball
    assert (close(a["normal"], normal, 1e-5) | ~floor).all()
    ball = same & on_ball
    assert ball.sum() > 50 and (close(a["normal"], normal, 5e-3) | ~ball).mean() >= 0.995


QUAD = """
SURFACES
Shape quad : InlineMesh { positions { -50,-50,0, 50,-50,0, 50,50,0, -50,50,0 } indices { 0,1,2, 0,2,3 } surface { @s } }
Camera cam : Pinhole { fov { 30 } spp { 2 } film : Color { resolution { 16, 16 } } position { 0, 0, 5 } look_at { 0, 0, 0 } }
render { cameras { @cam } shapes { @quad } environment : Spherical { emission : Constant { v { 1 } } }
  integrator : AOV { components { "albedo", "roughness", "mask" } } }
"""


def _rough(alpha):  # TrowbridgeReitzDistribution::alpha_to_roughness, scattering.cpp:141-143
    return np.sqrt(np.maximum(np.asarray(alpha, np.float64), 1e-4))


def _alpha(r, remap):  # roughness_to_alpha, scattering.cpp:129-135
    return max(r * r, 1e-4) if remap else r


def _fresnel_conductor_normal(n, k):  # fresnel_conductor(1, 1, n, k), scattering.cpp:54-74 at normal incidence
    n, k = np.asarray(n, np.float64), np.asarray(k, np.float64)
    return ((n - 1) ** 2 + k ** 2) / ((n + 1) ** 2 + k ** 2)


def _closure_cases(remap):
    rm = "true" if remap else "false"
    matte = "Surface a : Matte { Kd : Constant { v { 0.6, 0.4, 0.2 } } }\n"
    mirror = f"Surface b : Mirror {{ color : Constant {{ v {{ 0.9, 0.8, 0.7 }} }} roughness : Constant {{ v {{ 0.3 }} }} remap_roughness {{ {rm} }} }}\n"
    mirror_rough = _rough([_alpha(0.3, remap)] * 2)
    kd, eta = np.array([0.5, 0.3, 0.2]), 1.5
    x = 1 / eta  # fresnel_dielectric_integral, scattering.cpp:97-107 (eta > 1)
    fdi = 0.97945724 + x * (0.21762732 + x * -1.18995376)
    aspect = np.sqrt(1 - 0.5 * 0.9)
    r = _alpha(0.6, remap)
    return {
        "matte": (matte.replace("Surface a", "Surface s"), [0.6, 0.4, 0.2], [1.0, 1.0], 1e-6),
        "mirror": (mirror.replace("Surface b", "Surface s"), [0.9, 0.8, 0.7], mirror_rough, 1e-6),
        "glass": (f"Surface s : Glass {{ Kr : Constant {{ v {{ 0.8, 0.7, 0.6 }} }} Kt : Constant {{ v {{ 1 }} }} roughness : Constant {{ v {{ 0.2 }} }} "
                  f"remap_roughness {{ {rm} }} }}\n", [0.8, 0.7, 0.6], _rough([_alpha(0.2, remap)] * 2), 1e-6),
        "plastic": (f"Surface s : Plastic {{ Kd : Constant {{ v {{ 0.5, 0.3, 0.2 }} }} roughness : Constant {{ v {{ 0.4 }} }} eta : Constant {{ v {{ 1.5 }} }} "
                    f"remap_roughness {{ {rm} }} }}\n", kd / (1 - kd * fdi), _rough([_alpha(0.4, remap)] * 2), 1e-5),
        "metal": (f'Surface s : Metal {{ eta {{ "Cu" }} roughness : Constant {{ v {{ 0.35 }} }} remap_roughness {{ {rm} }} }}\n', None,
                  _rough([_alpha(0.35, remap)] * 2), 1e-5),
        "disney": (f"Surface s : Disney {{ color : Constant {{ v {{ 0.7, 0.5, 0.3 }} }} roughness : Constant {{ v {{ 0.6 }} }} "
                   f"anisotropic : Constant {{ v {{ 0.5 }} }} remap_roughness {{ {rm} }} }}\n", [0.7, 0.5, 0.3],
                   _rough([max(0.001, r / aspect), max(0.001, r * aspect)]), 1e-5),
        # Mix: albedo a * r + b * (1 - r), roughness lerp(b, a, r) (mix.cpp:124-138); Layered: its top's (layered.cpp:242-243)
        "mix": (matte + mirror + "Surface s : Mix { a { @a } b { @b } ratio : Constant { v { 0.25 } } }\n",
                np.array([0.6, 0.4, 0.2]) * 0.25 + np.array([0.9, 0.8, 0.7]) * 0.75, mirror_rough + 0.25 * (1.0 - mirror_rough), 1e-5),
        "layered": (matte + mirror + "Surface s : Layered { top { @b } bottom { @a } }\n", [0.9, 0.8, 0.7], mirror_rough, 1e-6),
    }


@pytest.mark.parametrize("remap", [True, False])
def test_albedo_and_roughness_of_every_closure(renderer, remap):
    """one full-frame quad per closure kind: every sample's first hit is the quad, so the normalised buffers are the closure's
    albedo() and (roughness(), 0) of aov.cpp's table everywhere"""
    for kind, (surfaces, albedo, rough, tol) in _closure_cases(remap).items():
        sc = Scene.from_string(QUAD.replace("SURFACES", surfaces))
        renderer.upload(sc)
        renderer.render(0, 2, sync=True)
        assert renderer.last_variant() == SCENE_MASK | AOV
        assert (renderer.download_aov("mask") == 1).all(), kind
        if albedo is None:  # Metal: F_conductor(1, n, k) * refl (metal.cpp:220-224), n and k from the loaded table, refl 1
            f = [s.f for s in sc.view().surfaces[:sc.view().surface_count]][-1]
            albedo = _fresnel_conductor_normal(f[0:3], f[3:6])
        want_albedo = np.broadcast_to(np.asarray(albedo, np.float64), (16, 16, 3))
        want_rough = np.broadcast_to(np.array([rough[0], rough[1], 0.0]), (16, 16, 3))
        assert np.allclose(renderer.download_aov("albedo"), want_albedo, rtol=tol, atol=tol), (kind, remap, renderer.download_aov("albedo")[0, 0], albedo)
        assert np.allclose(renderer.download_aov("roughness"), want_rough, rtol=tol, atol=tol), (kind, remap, renderer.download_aov("roughness")[0, 0], rough)


def test_deterministic_and_bit_identical_under_tile_sharding(renderer):
    """per-wave LDS tiles + per-chunk partial planes resolved in chunk order: the same sums run to run and under any tile sharding
    with the same balance_shards (64 spp on this frame: several chunks per tile, so the partial planes are exercised)"""
    sc = Scene.from_string(_cornell_aov(resolution=(48, 40), spp=64))
    whole = _render(renderer, sc, 64, balance_shards=2)
    again = _render(renderer, sc, 64, balance_shards=2)
    shards = [_render(renderer, sc, 64, rank=r, world=2, balance_shards=2) for r in range(2)]
    for c in whole:
        assert np.array_equal(whole[c], again[c]), c
        assert np.array_equal(shards[0][c] + shards[1][c], whole[c]), c
        assert (shards[0][c] != 0).any() and (shards[1][c] != 0).any() or not whole[c].any(), c
    assert whole["mask"].max() == 64  # (the frame is wider than the box: its edges see past it)


def _cli(scene_file):
    return subprocess.run([CLI, "-b", "hip", "-d", "0", str(scene_file)], capture_output=True, text=True, timeout=600)


def test_cli_writes_the_dumps_of_the_reference_loop(tmp_path):
    """The plugin's loop (aov.cpp:372-433): noisy_count 10 against the camera's 4 spp -> one shutter sample of weight 1; power2 dumps
    at 1, 2, 4, 8 (none at 10); exactly those files, each the buffer after n samples times float(1 / n) -- the Python driver replaying
    the same launches (one per sample) gives the same bits; the camera's own file is never written"""
    comps = ["sample", "albedo", "depth", "mask", "roughness"]
    props = "noisy_count { 10 } components { " + ", ".join(f'"{c}"' for c in comps) + ' } dump { "power2" }'
    scene_file = tmp_path / "cornell.luisa"
    scene_file.write_text(_cornell_aov(props, resolution=32, spp=4, file="out.exr"))
    r = _cli(scene_file)
    assert r.returncode == 0, r.stderr
    counts = aov_dump_counts(10, "power2")
    expected = {os.path.basename(aov_file_name(str(tmp_path / "out.exr"), c, n, "power2")) for c in comps for n in counts}
    assert set(os.listdir(tmp_path)) - {"cornell.luisa"} == expected
    sc = Scene.load(str(scene_file))
    assert sc.aov_settings()["noisy_count"] == 10
    rd = MegaPathRenderer(0)
    try:
        rd.upload(sc)
        rd.clear()
        for n in range(1, 11):
            rd.render(n - 1, n, shutter_weight=1.0, sync=True)
            if n not in counts:
                continue
            for c in comps:
                img, _ = load_image(aov_file_name(str(tmp_path / "out.exr"), c, n, "power2"))
                want = rd.download_aov(c)
                got = img[..., 3:4] if want.shape[-1] == 1 else img[..., :3]  # (a lone EXR channel "A" comes back as alpha)
                assert np.array_equal(got, want), (c, n)
    finally:
        rd.close()


def test_cli_final_dump_and_no_lights(tmp_path):
    final = tmp_path / "final"
    final.mkdir()
    scene_file = final / "cornell.luisa"
    scene_file.write_text(_cornell_aov('components { "normal", "mask" } dump { "final" }', resolution=16, spp=8, file="img.exr"))
    r = _cli(scene_file)
    assert r.returncode == 0, r.stderr
    assert set(os.listdir(final)) == {"cornell.luisa", "img_normal.exr", "img_mask.exr"}
    dark = tmp_path / "dark"
    dark.mkdir()
    scene_file = dark / "quad.luisa"
    scene_file.write_text(QUAD.replace("SURFACES", "Surface s : Matte { }\n")
                          .replace("environment : Spherical { emission : Constant { v { 1 } } }", "")
                          .replace("spp { 2 }", 'spp { 2 } file { "q.exr" }'))
    r = _cli(scene_file)
    assert r.returncode == 0, r.stderr
    assert "No lights in scene. Rendering aborted." in r.stderr
    assert os.listdir(dark) == ["quad.luisa"]
