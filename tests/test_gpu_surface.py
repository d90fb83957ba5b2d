"""Surface queries on the device (include/lrhip.h: lrhip_query_surface): geometry against the float64 restatement of
Geometry::shading_point (tests/surface_reference.py), albedo / roughness against the closure table of tests/test_gpu_aov.py, textures and
normal maps, agreement with the AOV kernel's first-hit buffers, emission, batch semantics, pointers, moved and deformed scenes, errors."""
import ctypes as C

import numpy as np
import pytest

import instance_scene as S
import mesh_deform_scene as M
import raycast_reference as RR
import surface_reference as R
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import DeviceError, MegaPathRenderer, RayHits
from luisarender_amd.scene import save_image
from test_surface_reference import BALL_CENTRE, PLANE_BALL, camera_rays

pytestmark = pytest.mark.gpu

LRHIP_ERROR_INVALID, LRHIP_ERROR_UNSUPPORTED = -1, -3
GEOMETRY_WORDS = [w for w in range(32) if w not in (16, 17, 18, 19, 22, 23, 24, 25, 26, 28, 29, 30)]  # all but n_closure, closure_kind, roughness, albedo, emission
MATERIAL_WORDS = [22, 23, 24, 25, 26, 28, 29, 30]  # roughness, albedo, emission: zeros under geometry_only
KINDS = {"matte": 1, "mirror": 2, "glass": 3, "plastic": 4, "metal": 5, "disney": 6, "mix": 7, "layered": 8}  # lr_scene.h: LR_SURFACE_*


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


def words(points) -> np.ndarray:
    return points.buffer.view(np.uint32)


def with_tri_invalid(hits: RayHits) -> np.ndarray:
    """the same records as a caller without a ray would make them: (inst, prim, u, v) with tri = LR_INVALID_ID"""
    rec = hits.buffer.copy()
    rec.view(np.uint32)[:, 5] = R.INVALID
    return rec


# ---------------------------------------------------------------- 1. geometry against the float64 reference

def test_geometry_against_the_float64_reference(renderer, capsys):
    """both paths (the baked record of hit.tri; instance + triangle + vertices for tri = LR_INVALID_ID) at the device's own (inst, prim, u, v)
    for 4133 rays in the instanced room and the Cornell box: no ray is ambiguous and none is left out.  The largest errors are printed; the
    bars are 4 x the values recorded in surface_reference.py"""
    worst = {}
    for name, scene in (("room", S.room()), ("cornell", RR.scene_of("cornell"))):
        rays = RR.make_rays(scene)
        renderer.upload(scene)
        hits = renderer.trace(rays)
        hit = np.asarray(hits.hit)
        assert 0.5 < hit.mean() and len(rays) % 64 != 0
        ref = R.shading_points(scene, hits.inst[hit], hits.prim[hit], hits.u[hit], hits.v[hit])
        for path, records in (("baked", hits), ("instance", with_tri_invalid(hits))):
            for with_rays in (True, False):
                got = renderer.surface(records, rays if with_rays else None)
                assert np.array_equal(np.asarray(got.valid), hit)
                assert (words(got)[~hit] == R.invalid_record()).all()
                assert np.array_equal(got.inst[hit], hits.inst[hit]) and np.array_equal(got.prim[hit], hits.prim[hit])
                valid = type(got)(got.buffer[hit])
                err = R.geometry_errors(valid, ref)
                for k, e in err.items():
                    worst[k] = max(worst.get(k, 0.0), e)
                with capsys.disabled():
                    print(f"\n[surface] {name} {path} rays={with_rays}: " + ", ".join(f"{k} {e:.3e}" for k, e in err.items()), end="")
                # the frame's invariants, everywhere: unit vectors, the tangent orthogonal to ns, ns on ng's side
                for a in (valid.ng, valid.ns, valid.tangent):
                    assert np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1.0).max() < 2e-6
                assert np.abs(np.einsum("nk,nk->n", valid.tangent.astype(np.float64), valid.ns.astype(np.float64))).max() < 2e-6
                assert (np.einsum("nk,nk->n", valid.ns, valid.ng) >= 0).all()
                flags = ref["flags"]
                assert np.array_equal(np.asarray(valid.has_surface), (flags & R.HAS_SURFACE) != 0)
                assert np.array_equal(np.asarray(valid.has_light), (flags & R.HAS_LIGHT) != 0)
                if with_rays:  # BACK_FACING = dot(wo, ng) < 0, away from grazing directions
                    cos = np.einsum("nk,nk->n", -rays[hit, 4:7].astype(np.float64), ref["ng"])
                    clear = np.abs(cos) > 1e-4
                    assert np.array_equal(np.asarray(valid.back_facing)[clear], cos[clear] < 0)
                else:
                    assert not np.asarray(valid.back_facing).any()
    with capsys.disabled():
        print("\n[surface] largest errors: " + ", ".join(f"{k} {e:.3e}" for k, e in worst.items()))
    assert max(worst.values()) <= R.LARGEST_SOUND_ERROR, worst  # beyond this it is a bug, whatever the bars say
    for k, bar in (("p", R.BAR_P), ("ng", R.BAR_NG), ("ns", R.BAR_NS), ("uv", R.BAR_UV), ("tangent", R.BAR_TANGENT), ("area", R.BAR_AREA)):
        assert worst[k] <= bar, (k, worst[k], bar)


# ---------------------------------------------------------------- 2. albedo and roughness of every closure

# tests/test_gpu_aov.py: QUAD, with the integrator left open
QUAD = """
SURFACES
Shape quad : InlineMesh { positions { -50,-50,0, 50,-50,0, 50,50,0, -50,50,0 } indices { 0,1,2, 0,2,3 } surface { @s } }
Camera cam : Pinhole { fov { 30 } spp { 2 } film : Color { resolution { 16, 16 } } position { 0, 0, 5 } look_at { 0, 0, 0 } }
render { cameras { @cam } shapes { @quad } environment : Spherical { emission : Constant { v { 1 } } }
  integrator : INTEGRATOR }
"""
INTEGRATORS = {"megapath": "MegaPath { }", "aov": 'AOV { components { "albedo", "roughness", "mask" } }'}


def quad_rays(n=67, seed=3, z=5.0, extent=40.0):
    """n rays straight down -z onto the quad of QUAD, origins uniform over its middle"""
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:2] = rng.uniform(-extent, extent, (n, 2))
    rays[:, 2], rays[:, 6], rays[:, 7] = z, -1.0, np.inf
    return rays


@pytest.mark.parametrize("remap", [True, False])
def test_albedo_and_roughness_of_every_closure(renderer, remap):
    """the closure table of test_gpu_aov.py, under a MegaPath integrator and again under AOV: every record's albedo and roughness are that
    table's within its tolerances, and closure_kind names the closure"""
    from test_gpu_aov import _closure_cases, _fresnel_conductor_normal
    rays = quad_rays()
    for kind, (surfaces, albedo, rough, tol) in _closure_cases(remap).items():
        for integrator in INTEGRATORS.values():
            sc = Scene.from_string(QUAD.replace("SURFACES", surfaces).replace("INTEGRATOR", integrator))
            renderer.upload(sc)
            got = renderer.surface(rays=rays)
            assert np.asarray(got.valid).all() and np.asarray(got.has_surface).all(), kind
            want = albedo
            if want is None:  # Metal: F_conductor(1, n, k) * refl (metal.cpp:220-224), n and k from the loaded table, refl 1
                f = [s.f for s in sc.view().surfaces[:sc.view().surface_count]][-1]
                want = _fresnel_conductor_normal(f[0:3], f[3:6])
            assert np.allclose(got.albedo, np.broadcast_to(np.asarray(want, np.float64), (len(rays), 3)), rtol=tol, atol=tol), (kind, remap, got.albedo[0], want)
            assert np.allclose(got.roughness, np.broadcast_to(np.asarray(rough, np.float64), (len(rays), 2)), rtol=tol, atol=tol), (kind, remap, got.roughness[0], rough)
            assert (got.closure_kind == KINDS[kind]).all(), (kind, got.closure_kind[0])
            assert len(set(got.surface.tolist())) == 1 and got.surface[0] < sc.view().surface_count
            assert (got.light == R.INVALID).all() and (got.emission == 0).all()
            assert np.array_equal(got.n_closure, got.ns) and not np.asarray(got.back_facing).any()


# ---------------------------------------------------------------- 3. textures

# a unit quad whose uv are its x and y; rays come straight down -z
UNIT_QUAD = """
SURFACE
Shape quad : InlineMesh { positions { 0,0,0, 1,0,0, 1,1,0, 0,1,0 } uvs { 0,0, 1,0, 1,1, 0,1 } indices { 0,1,2, 0,2,3 } surface { @s } }
Camera cam : Pinhole { fov { 30 } spp { 1 } film : Color { resolution { 8, 8 } } position { 0.5, 0.5, 3 } look_at { 0.5, 0.5, 0 } }
render { cameras { @cam } shapes { @quad } environment : Spherical { emission : Constant { v { 1 } } } integrator : MegaPath { } }
"""


def centre_rays(cells):
    """rays straight down onto the centres of a cells x cells grid over the unit quad, row by row (index = y * cells + x)"""
    c = (np.arange(cells) + 0.5) / cells
    x, y = np.meshgrid(c, c)
    rays = np.zeros((cells * cells, 8), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 6], rays[:, 7] = x.reshape(-1), y.reshape(-1), 1.0, -1.0, np.inf
    return rays


def test_checkerboard_albedo(renderer):
    on, off = (0.8, 0.3, 0.2), (0.2, 0.5, 0.75)
    kd = f"Checkerboard {{ on : Constant {{ v {{ {on[0]}, {on[1]}, {on[2]} }} }} off : Constant {{ v {{ {off[0]}, {off[1]}, {off[2]} }} }} scale {{ 4 }} }}"
    sc = Scene.from_string(UNIT_QUAD.replace("SURFACE", f"Surface s : Matte {{ Kd : {kd} }}"))
    renderer.upload(sc)
    rays = centre_rays(4)
    got = renderer.surface(rays=rays)
    assert np.asarray(got.valid).all() and np.abs(got.uv - rays[:, 0:2]).max() < 1e-6
    # the cell's value by the host's own table: child[parity] of the Checkerboard texture (checkerboard.cpp)
    v = sc.view()
    (board,) = [v.textures[i] for i in range(v.texture_count) if v.textures[i].kind == 2]
    values = [np.array(v.textures[board.child[k]].v[0:3], np.float64) for k in range(2)]
    assert np.array_equal(np.sort(np.array(values), axis=0), np.sort(np.float32([on, off]).astype(np.float64), axis=0))
    y, x = np.divmod(np.arange(16), 4)
    want = np.array([values[(xx + yy) & 1] for xx, yy in zip(x, y)])
    assert np.abs(got.albedo - want).max() <= 1e-6
    assert (got.closure_kind == 1).all() and (got.roughness == 1).all()


@pytest.mark.parametrize("tex_filter", ["point", "bilinear"])
def test_image_albedo_at_texel_centres(renderer, tmp_path, tex_filter):
    """a 4x4 linear image: at texel centres the point filter and the bilinear filter (weights 1, 0, 0, 0 there) both give the texel"""
    rng = np.random.default_rng(5)
    image = np.ones((4, 4, 4), np.float32)
    image[..., :3] = rng.uniform(0.05, 0.95, (4, 4, 3))
    path = str(tmp_path / "albedo.exr")
    save_image(path, image)
    kd = f'Image {{ file {{ "{path}" }} encoding {{ "linear" }} filter {{ "{tex_filter}" }} }}'
    sc = Scene.from_string(UNIT_QUAD.replace("SURFACE", f"Surface s : Matte {{ Kd : {kd} }}"))
    renderer.upload(sc)
    got = renderer.surface(rays=centre_rays(4))
    assert np.asarray(got.valid).all()
    # texel (x, y) of the host's table is row y, column x: floor(u w), floor(v h) (image.cpp:132-168)
    v = sc.view()
    (tex,) = [v.textures[i] for i in range(v.texture_count) if v.textures[i].kind == 1]
    assert (tex.width, tex.height) == (4, 4)
    texels = np.ctypeslib.as_array(v.texels, shape=((tex.texel_offset + 16) * 4,)).reshape(-1, 4)[tex.texel_offset:, :3]
    assert np.allclose(np.sort(texels.reshape(-1)), np.sort(image[..., :3].reshape(-1)), atol=2e-3)  # (the file holds half floats)
    assert np.abs(got.albedo.astype(np.float64) - texels).max() <= 1e-6
    assert len({tuple(a) for a in got.albedo.tolist()}) == 16


def test_normal_map_moves_the_closure_normal_only(renderer, tmp_path):
    tilt = np.zeros((4, 4, 4), np.float32)
    tilt[...] = [0.5 + 0.5 * 0.6, 0.5, 0.5 + 0.5 * 0.8, 1.0]  # tangent-space (0.6, 0, 0.8)
    path = str(tmp_path / "n.exr")
    save_image(path, tilt)
    plain = "Surface s : Matte { Kd : Constant { v { 0.5 } } }"
    mapped = plain.replace("Matte {", f'Matte {{ normal_map : Image {{ file {{ "{path}" }} }}')
    rays = centre_rays(5)
    out = {}
    for name, surface in (("plain", plain), ("mapped", mapped)):
        renderer.upload(Scene.from_string(UNIT_QUAD.replace("SURFACE", surface)))
        out[name] = renderer.surface(rays=rays)
        assert np.asarray(out[name].valid).all()
    assert np.array_equal(out["plain"].n_closure, out["plain"].ns)
    m = out["mapped"]
    assert np.array_equal(m.ns, out["plain"].ns) and np.array_equal(m.ng, out["plain"].ng)
    for a in (m.ns, m.n_closure):
        assert np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1.0).max() < 2e-6
    cos = np.einsum("nk,nk->n", m.n_closure, m.ns)
    assert np.abs(cos - 0.8).max() < 1e-3  # the map tilts the normal by acos(0.8) (half-float texels)
    assert np.array_equal(m.albedo, out["plain"].albedo)


# ---------------------------------------------------------------- 4. agreement with the AOV kernel

def test_agreement_with_the_aov_first_hit_buffers(renderer, capsys):
    """PLANE_BALL under the AOV integrator, ONE sample s of every pixel, raw sums: what the AOV kernel wrote for its own camera ray against
    what the surface query says for the oracle's camera ray of the same (pixel, s)"""
    s = 2
    text = PLANE_BALL.replace('components { "mask", "depth", "ndc", "normal" }', 'components { "mask", "depth", "normal", "albedo", "roughness" }')
    sc = Scene.from_string(text)
    renderer.upload(sc)
    renderer.render(s, s + 1, sync=True)
    a = {c: renderer.download_aov(c, normalized=False) for c in ("mask", "depth", "normal", "albedo", "roughness")}
    h, w = a["mask"].shape[:2]
    rays = camera_rays(sc, s)
    got = renderer.surface(rays=rays)
    valid = np.asarray(got.valid).reshape(h, w)
    same = valid == (a["mask"][..., 0] == 1)
    assert same.mean() >= 0.995 and valid.any() and (~valid).any()
    hit = (same & valid).reshape(-1)
    close = lambda x, want, tol: (np.abs(x - want) <= tol * np.maximum(1.0, np.abs(want))).reshape(len(x), -1).all(axis=1)
    depth = np.linalg.norm(got.p.astype(np.float64) - rays[:, 0:3], axis=1)
    assert close(depth[hit], a["depth"].reshape(-1)[hit], 1e-5).all()
    floor, ball = hit & (got.inst == 0), hit & (got.inst == 1)
    assert floor.sum() > 100 and ball.sum() > 50
    normal = a["normal"].reshape(-1, 3)
    assert close(got.ns[floor], normal[floor], 1e-5).all()
    assert np.allclose(got.albedo[hit], a["albedo"].reshape(-1, 3)[hit], rtol=1e-6, atol=1e-6)
    assert np.allclose(got.roughness[hit], a["roughness"].reshape(-1, 3)[hit][:, :2], rtol=1e-6, atol=1e-6)
    ball_error = float(np.abs(got.ns[ball].astype(np.float64) - normal[ball]).max())
    with capsys.disabled():
        print(f"\n[surface] ball ns against the AOV normal of the same sample: {ball_error:.3e} (bar {R.BAR_AOV_BALL_NORMAL:.3e}); "
              f"mask agrees on {same.mean():.4f} of the pixels")
    assert ball_error <= R.BAR_AOV_BALL_NORMAL
    analytic = got.p[ball].astype(np.float64) - BALL_CENTRE
    assert np.abs(got.ns[ball] - analytic / np.linalg.norm(analytic, axis=1, keepdims=True)).max() <= 5e-3


# ---------------------------------------------------------------- 5. emission

def lamp_rays(n, y, dy, seed=9):
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0], rays[:, 2] = rng.uniform(220, 336, n), rng.uniform(234, 325, n)  # inside the lamp quad (213..343, 227..332)
    rays[:, 1], rays[:, 5], rays[:, 7] = y, dy, np.inf
    return rays


def test_emission(renderer):
    sc = RR.scene_of("cornell")
    renderer.upload(sc)
    v = sc.view()
    assert v.light_count == 1 and v.lights[0].two_sided == 0
    tex = v.textures[v.lights[0].emission_tex]
    want = np.maximum(np.array(tex.v[0:3], np.float32), np.float32(0)) * np.float32(v.lights[0].scale)  # lrhip_upload.hip: upload_lights
    assert want.dtype == np.float32 and (want > 0).all()
    below = renderer.surface(rays=lamp_rays(65, 400.0, 1.0))
    assert np.asarray(below.valid).all() and np.asarray(below.has_light).all() and not np.asarray(below.back_facing).any()
    assert (below.light == 0).all() and np.array_equal(below.emission, np.broadcast_to(want, (65, 3)))
    above = renderer.surface(rays=lamp_rays(65, 548.75, -1.0))  # between the lamp (548.7) and the ceiling (548.8)
    assert np.array_equal(above.inst, below.inst) and np.asarray(above.has_light).all() and (above.light == 0).all()
    assert np.asarray(above.back_facing).all() and (above.emission == 0).all()
    assert np.array_equal(above.albedo, below.albedo) and (above.albedo > 0).all()  # the lamp has a surface as well
    # without rays the lamp is seen from its front, from p + ng
    front = renderer.surface(renderer.trace(lamp_rays(65, 400.0, 1.0)))
    assert np.array_equal(front.emission, below.emission) and not np.asarray(front.back_facing).any()
    # every other hit of the box: no light, no emission
    rays = RR.make_rays(sc)
    rest = renderer.surface(rays=rays)
    other = np.asarray(rest.valid) & ~np.asarray(rest.has_light)
    assert other.sum() > 1000 and (rest.emission[other] == 0).all() and (rest.light[other] == R.INVALID).all()
    lit = np.asarray(rest.valid) & np.asarray(rest.has_light)
    assert (rest.light[lit] == 0).all()
    assert np.array_equal(np.any(rest.emission[lit] != 0, axis=1), ~np.asarray(rest.back_facing)[lit])


# ---------------------------------------------------------------- 6. batch semantics

NESTED = ("Surface a : Matte { Kd : Constant { v { 0.6, 0.4, 0.2 } } }\nSurface b : Mirror { color : Constant { v { 0.9, 0.8, 0.7 } } }\n"
          "Surface l : Layered { top { @b } bottom { @a } }\nSurface s : Mix { a { @l } b { @a } ratio : Constant { v { 0.25 } } }\n")


def test_batch_semantics(renderer):
    scene = S.room()
    renderer.upload(scene)
    rays = RR.make_rays(scene, n=257, seed=4)
    hits = renderer.trace(rays)
    assert 0 < np.asarray(hits.hit).sum() < 257
    full = renderer.surface(hits, rays)
    for n in (0, 1, 63, 64, 65, 257):
        part = renderer.surface(RayHits(np.ascontiguousarray(hits.buffer[:n])), np.ascontiguousarray(rays[:n]))
        assert part.buffer.shape == (n, 32) and np.array_equal(words(part), words(full)[:n]), n
    perm = np.random.default_rng(1).permutation(257)
    shuffled = renderer.surface(np.ascontiguousarray(hits.buffer[perm]), np.ascontiguousarray(rays[perm]))
    assert np.array_equal(words(shuffled), words(full)[perm])
    assert np.array_equal(words(renderer.surface(rays=rays)), words(full))  # hits=None traces first

    # malformed records give the invalid record, their neighbours are unaffected
    good = np.nonzero(np.asarray(hits.hit))[0]
    v = scene.view()
    bad_hits, bad_rays = hits.buffer.copy(), rays.copy()
    ids = bad_hits.view(np.uint32)
    cases = {}
    k = iter(good[:12])

    def spoil(name):
        i = int(next(k))
        cases[name] = i
        return i

    ids[spoil("tri out of range"), 5] = v.accel.triangle_count
    ids[spoil("tri far out of range"), 5] = 0xFFFFFFFE
    i = spoil("inst out of range")
    ids[i, 5], ids[i, 3] = R.INVALID, v.instance_count
    i = spoil("inst invalid")
    ids[i, 5], ids[i, 3] = R.INVALID, R.INVALID
    i = spoil("prim out of range")  # the first primitive behind the instance's mesh
    tables = S.host_tables(scene)
    ids[i, 5], ids[i, 4] = R.INVALID, int(tables["meshes"][tables["instances"][ids[i, 3], 0] >> 10, 3])
    i = spoil("prim far out of range")
    ids[i, 5], ids[i, 4] = R.INVALID, 0x7FFFFFFF
    bad_hits[spoil("u nan"), 1] = np.nan
    bad_hits[spoil("v inf"), 2] = np.inf
    bad_hits[spoil("u -inf"), 1] = -np.inf
    bad_rays[spoil("ray nan"), 0] = np.nan
    bad_rays[spoil("ray zero direction"), 4:7] = 0.0
    i = spoil("ray empty interval")
    bad_rays[i, 7] = bad_rays[i, 3]
    got = renderer.surface(bad_hits, bad_rays)
    spoiled = np.zeros(257, bool)
    spoiled[list(cases.values())] = True
    for name, i in cases.items():
        assert np.array_equal(words(got)[i], R.invalid_record()), name
    assert np.array_equal(words(got)[~spoiled], words(full)[~spoiled])
    assert (words(full)[~np.asarray(hits.hit)] == R.invalid_record()).all()  # misses

    # rays=None: wo = ng, nothing is back facing; the geometry is the same
    front = renderer.surface(hits)
    assert np.array_equal(np.asarray(front.valid), np.asarray(hits.hit)) and not np.asarray(front.back_facing).any()
    geometry = [w for w in GEOMETRY_WORDS if w != 7]
    assert np.array_equal(words(front)[:, geometry], words(full)[:, geometry])

    # geometry_only: the same bytes in every geometry field, zeros in the material fields, n_closure = ns, closure_kind invalid
    lean = renderer.surface(hits, rays, geometry_only=True)
    assert np.array_equal(words(lean)[:, GEOMETRY_WORDS], words(full)[:, GEOMETRY_WORDS])
    assert (words(lean)[:, MATERIAL_WORDS] == 0).all() and (lean.closure_kind == R.INVALID).all()
    hit = np.asarray(hits.hit)
    assert np.array_equal(lean.n_closure[hit], lean.ns[hit])
    assert (full.albedo[hit & np.asarray(full.has_surface)] > 0).any()


def test_nested_surfaces_are_served_by_the_geometry_only_query(renderer):
    sc = Scene.from_string(QUAD.replace("SURFACES", NESTED).replace("INTEGRATOR", INTEGRATORS["megapath"]))
    renderer.upload(sc)
    rays = quad_rays()
    hits = renderer.trace(rays)
    with pytest.raises(DeviceError, match=f"lrhip error {LRHIP_ERROR_UNSUPPORTED}"):
        renderer.surface(hits, rays)
    lean = renderer.surface(hits, rays, geometry_only=True)
    assert np.asarray(lean.valid).all() and np.asarray(lean.has_surface).all() and (lean.surface < sc.view().surface_count).all()
    assert np.abs(lean.p[:, 0:2] - rays[:, 0:2]).max() < 1e-4 and np.abs(lean.p[:, 2]).max() < 1e-5
    assert (words(lean)[:, MATERIAL_WORDS] == 0).all()


# ---------------------------------------------------------------- 7. pointers

def test_device_pointers_equal_host_pointers(renderer):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    scene = S.room()
    renderer.upload(scene)
    rays = RR.make_rays(scene, n=1000, seed=6)
    hits = renderer.trace(rays)
    host = renderer.surface(hits, rays)
    assert renderer.last_surface_ms() > 0.0
    device_rays = torch.from_numpy(rays).to("cuda:0")
    device_hits = torch.from_numpy(hits.buffer).to("cuda:0")
    got = renderer.surface(device_hits, device_rays)
    assert got.buffer.is_cuda and got.buffer.shape == (1000, 32)
    assert np.array_equal(got.buffer.cpu().numpy().view(np.uint32), words(host))
    assert renderer.last_surface_ms() > 0.0
    # trace + surface on the context's stream without a host round trip, then ONE synchronise
    torch.cuda.current_stream().synchronize()
    chained = renderer.surface(rays=device_rays, sync=False)
    lean = renderer.surface(renderer.trace(device_rays, sync=False), None, geometry_only=True, sync=False)
    renderer.synchronize()
    assert np.array_equal(chained.buffer.cpu().numpy().view(np.uint32), words(host))
    assert np.array_equal(lean.buffer.cpu().numpy().view(np.uint32), words(renderer.surface(hits, geometry_only=True)))
    assert chained.inst.dtype == torch.int32 and bool((chained.inst[~chained.valid] == -1).all())
    for bad in ((device_hits, rays), (hits.buffer, device_rays), (device_hits[:, :7], None), (device_hits.double(), None), (device_hits[:10], device_rays)):
        with pytest.raises(ValueError):
            renderer.surface(*bad)


# ---------------------------------------------------------------- 8. moved and deformed scenes

def test_moved_and_deformed_scenes(capsys):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    scene_a, scene_b = M.room(), M.room()
    ids = M.check_room(scene_a)
    ra, rb = MegaPathRenderer(0), MegaPathRenderer(0)
    try:
        ra.upload(scene_a)
        rb.upload(scene_b)
        rays = RR.make_rays(scene_a, n=2000, seed=8)
        before_hits = ra.trace(rays).buffer.copy()
        before = words(ra.surface(RayHits(before_hits), rays)).copy()
        which = np.array([ids["ball_a"]])
        matrix = S.srt(scale=(0.75, 0.5, 0.6), axis=(0, 1, 1), degrees=-110.0, translate=(0.5, 1.25, 1.0))[None]
        p, _ = scene_a.mesh_vertices(1)
        moved = M.first_deformation(p)
        # context A: device pointers, asynchronous; the queries behind them on the stream see the new geometry
        device_matrix, device_which = torch.from_numpy(matrix).to("cuda:0"), torch.from_numpy(which.astype(np.int32)).to("cuda:0")
        device_moved = torch.from_numpy(moved).to("cuda:0")
        ra.set_instance_transforms(device_matrix, device_which)
        ra.set_mesh_vertices(1, device_moved, recompute_normals=True)
        hits_a = ra.trace(rays)
        surf_a = ra.surface(hits_a, rays)
        texel_a = ra.surface(with_tri_invalid(hits_a), rays)
        # context B: the host mirrors + lrhip_update_scene
        scene_b.set_instance_transforms(matrix, which)
        scene_b.set_mesh_vertices(1, moved, recompute_normals=True)
        rb.upload(scene_b, keep_film=True)
        hits_b = rb.trace(rays)
        assert np.array_equal(hits_a.buffer.view(np.uint32), hits_b.buffer.view(np.uint32))
        assert np.array_equal(words(surf_a), words(rb.surface(hits_b, rays)))
        assert np.array_equal(words(texel_a), words(rb.surface(with_tri_invalid(hits_b), rays)))
        assert not np.array_equal(hits_a.buffer.view(np.uint32), before_hits.view(np.uint32)) and not np.array_equal(words(surf_a), before)
        # hits on the moved ball follow the new matrix and the new vertices: the reference over the moved host scene, test 1's bars
        on_ball = np.asarray(hits_a.hit) & (hits_a.inst == ids["ball_a"])
        assert on_ball.sum() > 10
        ref = R.shading_points(scene_b, hits_a.inst[on_ball], hits_a.prim[on_ball], hits_a.u[on_ball], hits_a.v[on_ball])
        for name, got in (("baked", surf_a), ("instance", texel_a)):
            err = R.geometry_errors(type(got)(got.buffer[on_ball]), ref)
            with capsys.disabled():
                print(f"\n[surface] moved and deformed ball, {name}: " + ", ".join(f"{k} {e:.3e}" for k, e in err.items()), end="")
            assert err["p"] <= R.BAR_P, (name, err)
    finally:
        ra.close()
        rb.close()


# ---------------------------------------------------------------- 9. errors

def test_errors(renderer):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    lib = renderer._lib
    hits, out = np.zeros((4, 8), np.float32), np.zeros((4, 32), np.float32)

    def call(ctx, **fields):
        p = _ffi.SurfaceQueryParams()
        p.hits, p.out, p.count = hits.ctypes.data, out.ctypes.data, 4
        for name, value in fields.items():
            setattr(p, name, value)
        rc = lib.lrhip_query_surface(ctx, C.byref(p))
        return rc, lib.lrhip_last_error().decode()

    fresh = MegaPathRenderer(0)
    try:
        rc, text = call(fresh._ctx)
        assert rc == LRHIP_ERROR_INVALID and "no scene uploaded" in text
        assert fresh.last_surface_ms() == 0.0
    finally:
        fresh.close()
    renderer.upload(S.room())
    ctx = renderer._ctx
    assert call(ctx)[0] == 0 and (out.view(np.uint32)[:, 7] & _ffi.SURFACE_VALID).all()  # (a zero record names vertex 0 of BVH triangle 0)
    for fields in (dict(hits=None), dict(out=None), dict(flags=4), dict(flags=64 | 32), dict(flags=2), dict(count=0x80000000)):
        rc, text = call(ctx, **fields)
        assert rc == LRHIP_ERROR_INVALID and "lrhip_query_surface" in text, fields
    assert call(ctx, hits=None, out=None, count=0)[0] == 0  # count 0 launches nothing, whatever the pointers
    # misaligned device pointers: refused before anything is read (the addresses lie inside live allocations all the same)
    d_hits, d_rays = torch.zeros((5, 8), dtype=torch.float32, device="cuda:0"), torch.zeros((5, 8), dtype=torch.float32, device="cuda:0")
    d_out = torch.zeros((5, 32), dtype=torch.float32, device="cuda:0")
    aligned = dict(hits=d_hits.data_ptr(), rays=d_rays.data_ptr(), out=d_out.data_ptr(), flags=_ffi.RAY_DEVICE_POINTERS)
    assert all(a % 16 == 0 for a in (aligned["hits"], aligned["rays"], aligned["out"]))
    for name in ("hits", "rays", "out"):
        rc, text = call(ctx, **{**aligned, name: aligned[name] + 4})
        assert rc == LRHIP_ERROR_INVALID and "16-byte aligned" in text, name
    rc, _ = call(ctx, **aligned)
    renderer.synchronize()
    assert rc == 0
