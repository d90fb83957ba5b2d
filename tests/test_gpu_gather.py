"""Lightmap texels on the device (include/lrhip.h: lrhip_lightmap_texels): the UV rasteriser against the float64 numpy
rasteriser of tests/gather_reference.py on three meshes -- an inline quad, an inline fan with a mirrored and a degenerate triangle and parts
outside the map, and the icosphere -- the conservative mode's guarantees, the round trip through the surface query, a deformed mesh, the
host-pointer path's chunks against the device-pointer path, and the calls that must be refused.  Then the gather vertex
(lrhip_query_gather_vertex): its light sample and direction against the light and BSDF queries bit for bit, batches, bare points and the
records that must come back invalid, and the plan continued by the caller against the radiance query, statistically."""
import numpy as np
import pytest

import gather_reference as G
import mesh_deform_scene as M
from luisarender_amd import Scene, _ffi
from luisarender_amd.render import DeviceError, LightmapTexels, MegaPathRenderer

pytestmark = pytest.mark.gpu

SIZES = ((64, 64), (33, 17))
INVALID = 0xFFFFFFFF
BAND_LIMIT = 0.02  # of the texels of a map may lie in the band where either neighbour is right
UV_BAR = 1e-5

CHARTS = "\n".join([
    G.inline_mesh("quad", G.QUAD), G.inline_mesh("fan", G.FAN),
    "Shape bare : InlineMesh { positions { 0,0,-1, 1,0,-1, 0,1,-1 } indices { 0,1,2 } surface : Matte { } }",
    "Shape lamp : InlineMesh { positions { 0,0,4, 1,0,4, 0,1,4 } indices { 0,2,1 } light : Diffuse { emission : Constant { v { 5 } } two_sided { true } } }",
    "Camera cam : Pinhole { spp { 1 } film : Color { resolution { 8, 8 } } position { 0.5, 0.5, 3 } look_at { 0.5, 0.5, 0 } fov { 40 } }",
    "render { cameras { @cam } shapes { @quad, @fan, @bare, @lamp } integrator : MegaPath { depth { 2 } sampler : Independent { } } }"])


@pytest.fixture(scope="module")
def renderer():
    r = MegaPathRenderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def scenes():
    """{mesh name: (scene, instance, (uvs, triangles))}: the chart scene's quad and fan, the room's first ball"""
    charts = Scene.from_string(CHARTS)
    room = M.room()
    ids = M.check_room(room)
    ball = (room.mesh_uvs(ids["ball_mesh"]), room.mesh_triangles(ids["ball_mesh"]))
    assert np.array_equal(charts.mesh_uvs(charts.instance_mesh(0)), G.QUAD[0]) and np.array_equal(charts.mesh_uvs(charts.instance_mesh(1)), G.FAN[0])
    return {"quad": (charts, 0, G.QUAD), "fan": (charts, 1, G.FAN), "ball": (room, ids["ball_a"], ball), "ids": ids}


_reference = {}


def reference(name, chart, w, h, conservative):
    """the numpy rasteriser's answer, computed once per case and shared"""
    key = (name, w, h, conservative)
    if key not in _reference:
        _reference[key] = G.rasterise(*chart, w, h, conservative)
    return _reference[key]


def centres(w, h):
    t = np.arange(w * h)
    return np.stack([(t % w + 0.5) / w, (t // w + 0.5) / h], 1)


def check_records(texels: LightmapTexels, instance: int):
    """what every record is, whatever it says: t = 0, tri invalid, a texel record of the instance or the miss record"""
    words = texels.buffer.view(np.uint32)
    covered = np.asarray(texels.covered)
    assert (words[:, 0] == 0).all() and (words[:, 5] == INVALID).all() and (words[:, 7] == 0).all()
    assert (texels.inst[covered] == instance).all() and (texels.flags[covered] != 0).all() and ((texels.flags[covered] & ~np.uint32(3)) == 0).all()
    assert (words[~covered][:, [3, 4]] == INVALID).all() and (words[~covered][:, [1, 2, 6]] == 0).all()
    assert (texels.u >= 0).all() and (texels.v >= 0).all() and (texels.u + texels.v <= 1).all()


@pytest.mark.parametrize("conservative", (False, True))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ("quad", "fan", "ball"))
def test_texels_against_the_numpy_rasteriser(renderer, scenes, name, size, conservative, capsys):
    """owner, flags and u, v of every texel.  Judged with a band, as raycast_judge judges rays: a texel whose centre is within 2^-20 of a
    triangle edge may take either neighbour's answer, and at most 2 % of a map's texels may be such texels.  Centres EXACTLY on an edge
    (gather_reference.Texels.band: 17 of the icosphere's 561 texels at 33 x 17, 3 % of the map) are not in the band: both sides get an
    exact 0.0 there and the rule decides, so they must agree like every other texel."""
    scene, instance, chart = scenes[name]
    w, h = size
    ref = reference(name, chart, w, h, conservative)
    renderer.upload(scene)
    got = renderer.lightmap_texels(instance, w, h, conservative=conservative)
    assert isinstance(got, LightmapTexels) and got.buffer.shape == (w * h, 8) and (got.width, got.height) == (w, h)
    check_records(got, instance)
    band = ref.band
    assert band.mean() <= BAND_LIMIT
    strict = ~band
    differ = (got.prim != ref.prim) | (got.flags != ref.flags)
    same = ~differ & (ref.prim != G.NO_OWNER)
    du = max(float(np.abs(got.u[same].astype(np.float64) - ref.u[same]).max()), float(np.abs(got.v[same].astype(np.float64) - ref.v[same]).max()))
    with capsys.disabled():
        print(f"\n[lightmap] {name} {w}x{h} conservative={conservative}: covered {np.asarray(got.covered).mean():.3f}, band {band.mean():.4f}, "
              f"on an edge {ref.on_edge.mean():.4f}, owners that differ {int(differ.sum())} (outside the band {int((differ & strict).sum())}), "
              f"largest |du| {du:.2e}", end="")
    assert not (differ & strict).any(), np.nonzero(differ & strict)[0][:8]
    assert du <= UV_BAR
    # inside the band: one of the neighbours, i.e. a triangle of the chart that comes within the band's width of the centre, or nobody
    inside = np.nonzero(differ & band & np.asarray(got.covered))[0]
    if len(inside):
        d = G.distance_to_triangle(*chart, got.prim[inside], centres(w, h)[inside])
        limit = G.EPSILON if not conservative else G.EPSILON + 0.5 * np.hypot(1.0 / w, 1.0 / h)
        assert (d <= limit).all()
    assert (ref.prim != G.NO_OWNER).mean() > 0.125  # (the case is not empty)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ("quad", "fan", "ball"))
def test_conservative_mode(renderer, scenes, name, size):
    """every centre-covered texel keeps its record; every touched texel's point lies on its triangle, where the triangle is nearest to the
    centre; no texel further than half a texel diagonal from every triangle is owned"""
    scene, instance, chart = scenes[name]
    w, h = size
    renderer.upload(scene)
    plain, got = renderer.lightmap_texels(instance, w, h), renderer.lightmap_texels(instance, w, h, conservative=True)
    centre = np.asarray(plain.covered)
    assert np.array_equal(got.buffer.view(np.uint32)[centre], plain.buffer.view(np.uint32)[centre])
    assert np.array_equal(np.asarray(got.centre), centre) and (plain.flags[centre] == _ffi.LIGHTMAP_TEXEL_CENTRE).all()
    touched = np.asarray(got.touched)
    assert touched.sum() > 0 and not (touched & centre).any() and np.array_equal(np.asarray(got.covered), touched | centre)
    c = centres(w, h)
    p = G.chart_point(*chart, got.prim[touched], got.u[touched], got.v[touched])
    assert G.distance_to_triangle(*chart, got.prim[touched], p).max() < 2e-7
    nearest = G.distance_to_triangle(*chart, got.prim[touched], c[touched])
    assert np.abs(np.hypot(*(p - c[touched]).T) - nearest).max() < 2e-7
    ref = reference(name, chart, w, h, True)
    owned = np.asarray(got.covered)
    assert (ref.triangle_distance[owned] <= 0.5 * np.hypot(1.0 / w, 1.0 / h)).all()
    assert owned[ref.triangle_distance < 0.5 * min(1.0 / w, 1.0 / h) - G.EPSILON].all()  # and none that a triangle crosses is left out


@pytest.mark.parametrize("name", ("quad", "fan", "ball"))
def test_round_trip_through_the_surface_query(renderer, scenes, name):
    """surface(lightmap_texels(...)).uv gives each covered texel's centre back, on the device from end to end; a touched texel's uv is its
    triangle's nearest point; the texels nobody owns come back invalid"""
    import torch
    scene, instance, chart = scenes[name]
    renderer.upload(scene)
    for w, h in SIZES:
        texels = renderer.lightmap_texels(instance, w, h, conservative=True, on_device=True)
        assert isinstance(texels.buffer, torch.Tensor) and texels.buffer.is_cuda and texels.buffer.shape == (w * h, 8)
        points = renderer.surface(texels, geometry_only=True)
        assert isinstance(points.buffer, torch.Tensor)
        host = LightmapTexels(texels.buffer.cpu().numpy(), w, h)
        assert np.array_equal(host.buffer.view(np.uint32), renderer.lightmap_texels(instance, w, h, conservative=True).buffer.view(np.uint32))
        covered, centre = np.asarray(host.covered), np.asarray(host.centre)
        assert np.array_equal(points.valid.cpu().numpy(), covered)
        uv = points.uv.cpu().numpy().astype(np.float64)
        assert np.abs(uv[centre] - centres(w, h)[centre]).max() <= UV_BAR
        touched = np.asarray(host.touched)
        assert np.abs(uv[touched] - G.chart_point(*chart, host.prim[touched], host.u[touched], host.v[touched])).max() <= UV_BAR
        assert (points.inst.cpu().numpy()[covered] == instance).all()
        assert np.array_equal(points.prim.cpu().numpy()[covered].astype(np.uint32), host.prim[covered])
        if name != "ball":  # the inline charts lie in the plane z = 0 with x = u, y = v
            p = points.p.cpu().numpy().astype(np.float64)
            assert np.abs(p[centre][:, :2] - centres(w, h)[centre]).max() <= UV_BAR and np.abs(p[covered][:, 2]).max() == 0.0


def test_a_deformed_mesh_keeps_its_texels(renderer, scenes):
    """the rasteriser reads the device's tables as set_mesh_vertices left them: positions do not matter, so the records are the same
    bits, and surface() of them follows the new positions"""
    scene, instance, chart = scenes["ball"]
    mesh = scenes["ids"]["ball_mesh"]
    renderer.upload(scene)
    w, h = 33, 17
    before = renderer.lightmap_texels(instance, w, h, conservative=True)
    p_before = renderer.surface(before, geometry_only=True)
    positions, _ = scene.mesh_vertices(mesh)
    moved = M.first_deformation(positions)
    renderer.set_mesh_vertices(mesh, moved)
    after = renderer.lightmap_texels(instance, w, h, conservative=True)
    assert np.array_equal(after.buffer.view(np.uint32), before.buffer.view(np.uint32))
    p_after = renderer.surface(after, geometry_only=True)
    covered = np.asarray(after.covered)
    assert np.array_equal(np.asarray(p_after.valid), covered) and np.array_equal(p_after.uv[covered], p_before.uv[covered])
    # the point of record (prim, u, v) on the deformed mesh, through the instance's matrix, in float64
    tri = chart[1][after.prim[covered]]
    u, v = after.u[covered].astype(np.float64)[:, None], after.v[covered].astype(np.float64)[:, None]

    def world(vertices):
        q = vertices.astype(np.float64)
        local = (1.0 - u - v) * q[tri[:, 0]] + u * q[tri[:, 1]] + v * q[tri[:, 2]]
        m = np.array(scene.view().instances[instance].object_to_world, np.float64).reshape(4, 4).T  # column-major storage
        return local @ m[:3, :3].T + m[:3, 3]

    assert np.abs(p_after.p[covered] - world(moved)).max() < 1e-5 and np.abs(p_before.p[covered] - world(positions)).max() < 1e-5
    assert np.abs(p_after.p[covered].astype(np.float64) - p_before.p[covered]).max() > 0.05  # it did move
    renderer.upload(scene)  # the host's tables win again


def test_chunks_of_the_host_path_and_repeated_calls(renderer, scenes):
    """a map of more than 2^20 texels goes through the staging slot in two chunks whose records continue where the first chunk's end: the
    same bits as the one launch of the device-pointer path, and the same bits again from a second call (the owner pass is an atomicMin
    race whose outcome is not)"""
    import torch
    scene, instance, chart = scenes["fan"]
    renderer.upload(scene)
    w, h = 1100, 1000
    assert w * h > 1 << 20
    host = renderer.lightmap_texels(instance, w, h, conservative=True)
    assert renderer.last_lightmap_ms() > 0.0
    device = renderer.lightmap_texels(instance, w, h, conservative=True, on_device=True)
    assert torch.equal(device.buffer.view(torch.int32).cpu(), torch.from_numpy(host.buffer.view(np.int32)))
    again = renderer.lightmap_texels(instance, w, h, conservative=True)
    assert np.array_equal(again.buffer.view(np.uint32), host.buffer.view(np.uint32))
    check_records(host, instance)
    assert 0.3 < np.asarray(host.covered).mean() < 0.9 and np.asarray(host.touched).sum() > 1000
    # the second chunk's records are of ITS texels: every covered centre comes back through its barycentrics
    second = np.arange(1 << 20, w * h)
    second = second[np.asarray(host.centre)[second]][::37]
    p = G.chart_point(*chart, host.prim[second], host.u[second], host.v[second])
    assert np.abs(p - centres(w, h)[second]).max() < 2e-7


def test_calls_that_are_refused_and_maps_without_texels(renderer, scenes):
    scene, _, _ = scenes["quad"]
    renderer.upload(scene)
    with pytest.raises(DeviceError, match=r"lrhip error -3: .*no vertex UVs"):
        renderer.lightmap_texels(2, 16, 16)  # `bare` has no uvs
    with pytest.raises(ValueError, match="lightmap: instance 4 out of range"):
        renderer.lightmap_texels(4, 16, 16)
    lib, ctx = renderer._lib, renderer._ctx
    out = np.full((16, 8), 7.0, np.float32)
    assert lib.lrhip_lightmap_texels(ctx, 4, 4, 4, 0, out.ctypes.data) == -1 and b"out of range" in lib.lrhip_last_error()
    assert lib.lrhip_lightmap_texels(ctx, 0, 4, 4, 512, out.ctypes.data) == -1 and b"unknown flags" in lib.lrhip_last_error()
    assert lib.lrhip_lightmap_texels(ctx, 0, 4, 4, 0, None) == -1 and b"out is NULL" in lib.lrhip_last_error()
    assert lib.lrhip_lightmap_texels(ctx, 0, 65536, 32768, 0, out.ctypes.data) == -1 and b"2^31" in lib.lrhip_last_error()
    assert lib.lrhip_lightmap_texels(ctx, 0, 4, 4, _ffi.RAY_DEVICE_POINTERS, 8) == -1 and b"aligned" in lib.lrhip_last_error()
    assert (out == 7.0).all()
    for w, h in ((0, 0), (0, 16), (16, 0)):  # legal, nothing launched
        empty = renderer.lightmap_texels(0, w, h)
        assert empty.buffer.shape == (0, 8) and renderer.last_lightmap_ms() == 0.0
        assert lib.lrhip_lightmap_texels(ctx, 0, w, h, 0, None) == 0
    fresh = MegaPathRenderer(0)
    try:
        with pytest.raises(DeviceError, match="no scene uploaded"):
            fresh.lightmap_texels(0, 4, 4)
    finally:
        fresh.close()
    # the miss records of a map: every query answers them with its invalid record
    texels = renderer.lightmap_texels(0, 33, 17)
    missed = ~np.asarray(texels.covered)
    assert missed.sum() > 0
    assert not np.asarray(renderer.surface(texels, geometry_only=True).valid)[missed].any()
    u = np.full((len(texels), 4), 0.5, np.float32)
    assert not np.asarray(renderer.bsdf_sample(texels, u).valid)[missed].any()
    samples = renderer.light_sample(texels, u)
    assert not np.asarray(samples.valid)[missed].any() and np.asarray(samples.valid)[~missed].all()


# ---------------------------------------------------------------- the gather vertex: the plan of one irradiance sample

WHITE = """
Surface white : Matte { Kd : Constant { v { 1 } } }
Shape floor : InlineMesh { positions { -3,0,-3, 3,0,-3, 3,0,3, -3,0,3 } indices { 0,2,1, 0,3,2 } uvs { 0,0, 1,0, 1,1, 0,1 } surface { @white } }
Shape ball : Sphere { subdivision { 2 } surface { @white } transform : SRT { scale { 0.8, 0.8, 0.8 } translate { -0.5, 0.8, 0 } } }
Shape wall : InlineMesh { positions { 2,0,-2, 2,0,2, 2.5,3,2, 2.5,3,-2 } indices { 0,1,2, 0,2,3 } surface { @white } }
Shape lamp : InlineMesh { positions { -0.75,3.5,-0.75, 0.75,3.5,-0.75, 0.75,3.5,0.75, -0.75,3.5,0.75 } indices { 0,1,2, 0,2,3 }
  light : Diffuse { emission : Constant { v { 12, 11, 9 } } two_sided { true } } }
Camera cam : CAMERA { spp { 4 } film : Color { resolution { 24, 16 } } position { 0, 2.5, 7 } look_at { 0, 1, 0 } fov { 45 } LENS }
render { cameras { @cam } shapes { @floor, @ball, @wall, @lamp } environment : Spherical { emission : Constant { v { 0.5, 0.6, 0.8 } } }
  integrator : MegaPath { depth { 5 } sampler : SAMPLER } }
"""


def white_scene(camera="Pinhole", sampler="Independent { seed { 7 } }"):
    lens = "aperture { 2 } focal_length { 50 } focus_distance { 7 }" if camera == "ThinLens" else ""
    return Scene.from_string(WHITE.replace("CAMERA", camera).replace("LENS", lens).replace("SAMPLER", sampler))


def gather_records(renderer, n_side=17):
    """257 hit records of a grid of rays from above and from the camera's side into the white scene -- floor, ball (vertex normals: the
    shading frame is not the geometric one), the slanted wall, the lamp, misses -- as traced, as texel records (tri invalid), and a few
    damaged ones"""
    g = (np.arange(n_side * n_side) % n_side / (n_side - 1.0) - 0.5, np.arange(n_side * n_side) // n_side / (n_side - 1.0) - 0.5)
    rays = np.zeros((n_side * n_side, 8), np.float32)
    rays[:, 0:3] = np.stack([g[0] * 5.0, np.full_like(g[0], 3.0), g[1] * 5.0], 1)
    up = np.where(np.arange(n_side * n_side) % 4 == 0, 1.0, -1.0)  # every fourth ray looks up: the lamp from below, or a miss
    d = np.stack([g[0] * 0.3 - 0.05, up, g[1] * 0.3 - 0.1], 1)
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = np.inf
    hits = renderer.trace(rays).buffer
    records = hits[:257].copy()
    words = records.view(np.uint32)
    words[1::2, 5] = INVALID  # every other record names (inst, prim, u, v) as a texel does
    bad = {3: (3, 999), 10: (4, 0x7FFFFFF0), 17: (5, 123456789)}  # inst, prim out of range (on texel records), a tri that is none
    words[3, 5] = words[10, 5] = INVALID
    for k, (col, value) in bad.items():
        words[k, col] = value
    records[20, 1] = np.nan  # u
    return records


def unit_numbers(renderer, streams, sample, thin_lens):
    """the six numbers of the vertex, as the sampler queries give them: start, the pixel draw, the lens draw of a thin lens, then "1212" """
    state = renderer.sampler_start(streams, sample)
    renderer.sampler_draw(state, "p2" if thin_lens else "p")
    return renderer.sampler_draw(state, "1212")


@pytest.mark.parametrize("case", ("pinhole", "thin_lens", "padded_sobol"))
def test_the_gather_vertex_is_the_light_and_bsdf_queries_own(renderer, case, capsys):
    """the plan's light sample against light_sample(hits, u) and its direction against bsdf_sample on the scene itself, whose every surface IS
    white Matte, for the numbers sampler_start / sampler_draw give ("p", the lens draw, "1212"): shadow rays, light_pdf, the direction and
    its pdf bit for bit; nee and beta against the shading block's expressions in numpy float32"""
    scene = white_scene("ThinLens" if case == "thin_lens" else "Pinhole",
                        "PaddedSobol { seed { 3 } }" if case == "padded_sobol" else "Independent { seed { 7 } }")
    renderer.upload(scene)
    records = gather_records(renderer)
    n = len(records)
    assert n == 257
    streams = ((np.arange(n, dtype=np.uint64) * 2654435761) % 100003).astype(np.uint32)
    surface = renderer.surface(records, geometry_only=True)
    ok = np.asarray(surface.valid)
    assert 150 < ok.sum() < n and not ok[[3, 10, 17, 20]].any()
    for sample in (0, 5, 6, 9):
        got = renderer.gather_vertex(records, sample=sample, streams=streams)
        assert got.buffer.shape == (n, 24) and np.array_equal(np.asarray(got.valid), ok)
        assert not got.buffer[~ok].any()  # the invalid record: zeros
        u = unit_numbers(renderer, streams, sample, case == "thin_lens")
        assert u.shape == (n, 6)
        ls = renderer.light_sample(records, np.ascontiguousarray(u[:, 0:3]))
        lit = ok & (ls.pdf > 0)
        assert lit.sum() > 100
        assert np.array_equal(got.light_pdf[ok].view(np.uint32), ls.pdf[ok].view(np.uint32))
        assert np.array_equal(got.shadow[lit].view(np.uint32), ls.rays[lit].view(np.uint32))
        bs = renderer.bsdf_sample(records, np.ascontiguousarray(u[:, 3:6]))
        has_surface = ok & np.asarray(bs.valid)  # (the lamp carries a light and no surface: the gather's virtual surface has no twin there)
        assert has_surface.sum() > 140 and (ok & ~has_surface).sum() > 0
        assert np.array_equal(got.rays[has_surface][:, 4:7].view(np.uint32), bs.wi[has_surface].view(np.uint32))
        assert np.array_equal(got.pdf[has_surface].view(np.uint32), bs.pdf[has_surface].view(np.uint32))
        assert (got.rays[ok][:, 3] == 0).all() and (got.rays[ok][:, 7] == np.float32(3.402823466e+38)).all()
        # the ray leaves from the point, moved off the surface by less than a thousandth
        assert np.abs(got.rays[ok][:, 0:3] - surface.p[ok]).max() < 1e-3
        sound = ok & (got.pdf > 0)  # (a direction below the geometric surface fails the closure's side test: pdf = 0)
        assert sound.sum() > 140 and (np.einsum("nk,nk->n", got.rays[sound][:, 4:7], surface.ng[sound]) > 0).all()
        # beta = pi x ((1 / pdf) x f), nee = ((balance(light_pdf, eval.pdf) / light_pdf) x pi) x eval.f x L: float32, the shading block's order
        pi = np.float32(np.pi)
        alive = has_surface & (bs.pdf > 0)
        beta = pi * ((np.float32(1) / bs.pdf[alive])[:, None] * bs.f[alive])
        ev = renderer.bsdf_evaluate(records, np.ascontiguousarray(np.where(lit[:, None], got.shadow[:, 4:7], np.float32([0, 1, 0]))))
        both = lit & has_surface
        w = (ls.pdf[both] / (ls.pdf[both] + ev.pdf[both])) / ls.pdf[both]
        nee = ((w * pi)[:, None] * ev.f[both]) * ls.L[both]
        d_beta = float(np.abs(got.beta[alive] / beta - 1).max())
        # element by element, with a floor of 1e-30 under the denominator (a channel of nee that is 0 on both sides differs by 0)
        d_nee = float((np.abs(got.nee[both] - nee) / np.maximum(np.abs(nee), np.float32(1e-30))).max())
        with capsys.disabled():
            print(f"\n[gather vertex] {case} sample {sample}: valid {int(ok.sum())}, lit {int(lit.sum())}, beta rel {d_beta:.2e}, nee {d_nee:.2e}", end="")
        assert d_beta <= 4 * 2.0 ** -24 and d_nee <= 4 * 2.0 ** -24  # a handful of float32 operations on the device's own values
        assert np.abs(got.beta[alive] - pi).max() < 1e-5  # a white Lambert surface, cosine-sampled: f / pdf = 1, so beta stays pi
        assert (got.nee[ok & ~lit] == 0).all()


def test_gather_vertex_batches_points_and_edges(renderer):
    """position independence (each record alone and the batch reversed give the batch's bits), torch in / torch out, bare points with
    normals against the same points as hit records, and the records and scenes that must give the invalid record without a fault"""
    import torch
    scene = white_scene()
    renderer.upload(scene)
    records = gather_records(renderer)[:193]  # three blocks of 64 and one record
    n = len(records)
    streams = np.arange(100, 100 + n, dtype=np.uint32)
    got = renderer.gather_vertex(records, sample=5, streams=streams)
    back = renderer.gather_vertex(np.ascontiguousarray(records[::-1]), sample=5, streams=np.ascontiguousarray(streams[::-1]))
    assert np.array_equal(back.buffer[::-1].view(np.uint32), got.buffer.view(np.uint32))
    for k in (0, 1, 63, 64, 192):
        one = renderer.gather_vertex(records[k:k + 1].copy(), sample=5, streams=streams[k:k + 1].copy())
        assert np.array_equal(one.buffer.view(np.uint32), got.buffer[k:k + 1].view(np.uint32))
    default = renderer.gather_vertex(records, sample=5)  # streams None: record k has stream k
    assert np.array_equal(default.buffer.view(np.uint32), renderer.gather_vertex(records, sample=5, streams=np.arange(n, dtype=np.uint32)).buffer.view(np.uint32))
    device = torch.device("cuda", 0)
    t = renderer.gather_vertex(torch.from_numpy(records).to(device), sample=5, streams=torch.from_numpy(streams.view(np.int32)).to(device))
    assert isinstance(t.buffer, torch.Tensor) and t.buffer.is_cuda and np.array_equal(t.buffer.cpu().numpy().view(np.uint32), got.buffer.view(np.uint32))
    assert renderer.last_gather_ms() > 0.0
    # ---- bare points: the light sample is light_sample(points=...)'s, the direction is cosine-distributed about the caller's normal
    ok = np.asarray(got.valid)
    surface = renderer.surface(records, geometry_only=True)
    p, normal = np.ascontiguousarray(surface.p[ok]), np.ascontiguousarray(surface.ng[ok] * np.float32(3.0))  # any length
    pts = renderer.gather_vertex(points=p, normals=normal, sample=5, streams=np.ascontiguousarray(streams[ok]))
    assert np.asarray(pts.valid).all() and np.array_equal(pts.rays[:, 0:3], p)
    state = renderer.sampler_start(np.ascontiguousarray(streams[ok]), 5)
    renderer.sampler_draw(state, "p")
    u = renderer.sampler_draw(state, "1212")
    ls = renderer.light_sample(points=p, u=np.ascontiguousarray(u[:, 0:3]))
    lit = ls.pdf > 0
    assert np.array_equal(pts.light_pdf.view(np.uint32), ls.pdf.view(np.uint32)) and np.array_equal(pts.shadow[lit].view(np.uint32), ls.rays[lit].view(np.uint32))
    cos = np.einsum("nk,nk->n", pts.rays[:, 4:7].astype(np.float64), surface.ng[ok].astype(np.float64))
    assert (cos > 0).all() and np.abs(pts.pdf - cos / np.pi).max() < 1e-6 and np.abs(pts.beta[pts.pdf > 0] - np.float32(np.pi)).max() < 1e-5
    bad_p, bad_n = p[:6].copy(), normal[:6].copy()
    bad_n[0] = 0.0
    bad_n[1, 1] = np.nan
    bad_p[2, 0] = np.inf
    bad_n[3] = (0.0, -0.0, 0.0)
    edges = renderer.gather_vertex(points=bad_p, normals=bad_n, sample=5)
    assert np.asarray(edges.valid).tolist() == [False, False, False, False, True, True] and not edges.buffer[:4].any()
    # ---- nothing to gather from, nothing to gather with
    empty = renderer.gather_vertex(records[:0].copy(), sample=5)
    assert empty.buffer.shape == (0, 24) and renderer.last_gather_ms() == 0.0
    misses = np.zeros((70, 8), np.float32)
    misses.view(np.uint32)[:, 3:6] = INVALID
    assert not renderer.gather_vertex(misses).buffer.any()
    dark = Scene.from_string(WHITE.replace("CAMERA", "Pinhole").replace("LENS", "").replace("SAMPLER", "Independent { }")
                             .replace("environment : Spherical { emission : Constant { v { 0.5, 0.6, 0.8 } } }", "")
                             .replace("light : Diffuse { emission : Constant { v { 12, 11, 9 } } two_sided { true } }", "surface { @white }"))
    assert not dark.has_lighting
    renderer.upload(dark)
    assert not renderer.gather_vertex(records, sample=5).buffer.any()  # a scene without lighting: the records of no sample
    renderer.upload(scene)  # ... and the lit scene again: the same bits as before
    assert np.array_equal(renderer.gather_vertex(records, sample=5, streams=streams).buffer.view(np.uint32), got.buffer.view(np.uint32))


def test_the_plan_continued_by_the_caller_estimates_the_irradiance(renderer, capsys):
    """the plan's weights end to end, against the radiance query.  Every surface of the scene is black but for the two-sided lamp, under a
    constant environment, so nothing beyond the continuation ray's first hit contributes and the caller's one-vertex continuation is the
    whole estimator: E_s = free x nee + beta x L x balance(pdf, light_pdf_found), with free = ~trace(shadow, any_hit) and L, light_pdf_found
    = light_evaluate(trace(rays), rays).  The reference is pi x radiance() along the SAME cosine-distributed directions -- the existing
    query, which weighs what a camera ray finds with 1 -- i.e. the same integral without next-event estimation.  16 records on the floor and
    the ball, 4096 samples each on distinct streams: each of the 48 means agrees within 5 standard errors, and where the lamp is in direct
    view (its centre above the record's horizon, the segment to it free) the gather's standard deviation is below the reference's -- the light sample at the texel is the point of it."""
    black = Scene.from_string(WHITE.replace("CAMERA", "Pinhole").replace("LENS", "").replace("SAMPLER", "Independent { seed { 7 } }")
                              .replace("Kd : Constant { v { 1 } }", "Kd : Constant { v { 0 } }")
                              .replace("resolution { 24, 16 }", "resolution { 128, 64 }"))  # 8192 pixels: 4096 streams that are all different
    assert black.resolution() == (128, 64)
    renderer.upload(black)
    records = gather_records(renderer)
    records = records[np.asarray(renderer.surface(records, geometry_only=True).valid)]
    points = renderer.surface(records, geometry_only=True)
    faces_up = np.nonzero(points.ng[:, 1] > 0.2)[0]  # the lamp is above: the floor and the ball's upper half
    by_instance = [faces_up[points.inst[faces_up] == i] for i in np.unique(points.inst[faces_up])]
    assert len(by_instance) >= 2 and all(len(k) >= 8 for k in by_instance[:2])  # the floor and the ball
    pick = np.concatenate([k[np.linspace(0, len(k) - 1, 8).astype(np.int64)] for k in by_instance[:2]])
    assert len(set(pick.tolist())) == 16
    copies, calls = 256, 16
    batch = np.ascontiguousarray(np.tile(records[pick], (copies, 1)))  # record k % 16, copy k // 16
    streams = np.arange(len(batch), dtype=np.uint32) + np.uint32(11)  # (stream j is pixel j mod W x H's: beyond the frame they would repeat)
    gather, reference_series = [], []
    for s in range(calls):
        g = renderer.gather_vertex(batch, sample=s, streams=streams)
        rays, shadow = np.ascontiguousarray(g.rays), np.ascontiguousarray(g.shadow)
        sound = g.pdf > 0
        free = ~renderer.trace(shadow, any_hit=True) & (g.light_pdf > 0)
        found = renderer.light_evaluate(renderer.trace(rays), rays)
        weight = np.where(sound, g.pdf / np.maximum(g.pdf + found.pdf, np.float32(1e-30)), np.float32(0))
        gather.append(np.where(free[:, None], g.nee, np.float32(0)) + g.beta * found.L * weight[:, None])
        raw = renderer.radiance(rays, spp=1, spp_begin=s, streams=streams, clamp=1e9, raw=True)
        assert np.array_equal(raw[:, 3] == 1, sound | (raw[:, 3] == 1)) and (raw[sound, 3] == 1).all()
        reference_series.append(np.float32(np.pi) * np.where(sound[:, None], raw[:, :3], np.float32(0)))
    a = np.stack(gather).reshape(calls, copies, 16, 3).astype(np.float64).reshape(calls * copies, 16, 3)
    b = np.stack(reference_series).reshape(calls, copies, 16, 3).astype(np.float64).reshape(calls * copies, 16, 3)
    n = calls * copies
    mean_a, mean_b, sd_a, sd_b = a.mean(0), b.mean(0), a.std(0, ddof=1), b.std(0, ddof=1)
    z = np.abs(mean_a - mean_b) / np.sqrt(sd_a ** 2 / n + sd_b ** 2 / n)
    with capsys.disabled():
        print(f"\n[gather estimator] {n} samples x 16 records: largest |z| {z.max():.2f}, E from {mean_a.min():.3f} to {mean_a.max():.3f}, "
              f"sigma gather / reference: median {np.median(sd_a / sd_b):.3f}, largest {np.max(sd_a / sd_b):.3f}", end="")
    assert mean_a.min() > 0.1 and (z < 5.0).all(), z
    # in direct view of the lamp: its centre is above the record's horizon and the segment to it is free
    p0, ng = points.p[pick].astype(np.float64), points.ng[pick].astype(np.float64)
    to_lamp = np.array([0.0, 3.5, 0.0]) - p0
    distance = np.linalg.norm(to_lamp, axis=1)
    segment = np.zeros((16, 8), np.float32)
    segment[:, 0:3], segment[:, 4:7], segment[:, 7] = p0 + 1e-3 * ng, to_lamp / distance[:, None], distance * 0.999
    in_view = ~renderer.trace(segment, any_hit=True) & (np.einsum("nk,nk->n", ng, to_lamp / distance[:, None]) > 0.2)
    with capsys.disabled():
        print(f"; in direct view {int(in_view.sum())} of 16, sigma ratio there at most {np.max((sd_a / sd_b)[in_view]):.3f}", end="")
    assert in_view.sum() >= 8 and (sd_a[in_view] < sd_b[in_view]).all()


# ---------------------------------------------------------------- irradiance: the gather kernels (kFeatGather) behind lrhip_gather_irradiance

def cornell_records(renderer, n=193, every=83):
    """n records of the Cornell box at 128 x 128 -- the camera's hits, every `every`-th pixel, alternately as traced and as texel records
    (tri invalid), four of them damaged -- and a stream for each"""
    cam, _ = renderer.camera_samples(0)
    hits = renderer.trace(cam.rays).buffer[::every][:n].copy()
    assert len(hits) == n
    words = hits.view(np.uint32)
    words[1::2, 5] = INVALID
    words[3, 3], words[9, 4] = 999, 0x7FFFFFF0  # inst, prim out of range (on texel records)
    words[16, 3:6] = INVALID  # a miss
    hits[20, 1] = np.nan  # u
    streams = ((np.arange(n, dtype=np.uint64) * 2654435761) % 16381).astype(np.uint32)
    return hits, streams


def bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("sampler", ("Independent", "PaddedSobol"))
def test_irradiance_of_a_record_does_not_depend_on_its_place_in_the_batch(renderer, sampler):
    """193 records (three tiles of 64 and one record), some invalid, one sample at s = 0 and s = 5: the batch, each record alone and the batch
    reversed give the same bits with matching streams; n is 1 for valid records and 0 for invalid ones.  PaddedSobol: the generic-sampler
    kernel"""
    from luisarender_amd.scenes import cornell_box
    renderer.upload(Scene.from_string(cornell_box(resolution=128, spp=8, sampler=sampler)))
    records, streams = cornell_records(renderer)
    valid = np.asarray(renderer.surface(records, geometry_only=True).valid)
    assert 150 < valid.sum() < len(records) and not valid[[3, 9, 16, 20]].any()
    for s in (0, 5):
        whole = renderer.irradiance(records, spp=1, spp_begin=s, streams=streams, raw=True)
        assert whole.shape == (193, 4) and np.array_equal(whole[:, 3], valid.astype(np.float32)) and not whole[~valid].any()
        assert np.isfinite(whole).all() and (whole[valid, :3] >= 0).all() and (whole[valid, :3].sum(1) > 0).mean() > 0.5
        back = renderer.irradiance(np.ascontiguousarray(records[::-1]), spp=1, spp_begin=s, streams=np.ascontiguousarray(streams[::-1]), raw=True)
        assert np.array_equal(bits(np.ascontiguousarray(back[::-1])), bits(whole))
        for k in range(len(records)):
            one = renderer.irradiance(records[k:k + 1].copy(), spp=1, spp_begin=s, streams=streams[k:k + 1].copy(), raw=True)
            assert np.array_equal(bits(one), bits(whole[k:k + 1])), k
    assert renderer.last_gather_ms() > 0.0


@pytest.mark.parametrize("camera", ("Pinhole", "ThinLens"))
def test_one_irradiance_sample_is_the_plan_continued(renderer, camera, capsys):
    """every surface black but for the two-sided lamp, under a constant environment: nothing beyond the continuation ray's first hit
    contributes, so for 257 records and 4 sample indices the kernel's sample must equal visible x nee + beta x L x balance(pdf,
    light_pdf_found) with the plan's rays, shadow, nee, beta, pdf, visible = ~trace(shadow, any_hit) and L, light_pdf_found =
    light_evaluate(trace(rays), rays): a handful of float32 operations on values the device computed.  MEASURED on the MI355X: the largest
    relative difference (to the larger of the two, per record) is 2.001e-07 (5.6e-06 while the gather kernels were built with
    the renderers' approximate division and contraction: they take the plan kernel's arithmetic now, Makefile: variant_flags); the bar is four times that, and a bar above 1e-5 would be a
    different formula, not rounding.  ThinLens: the stream skips the lens draw"""
    measured = 2.001e-7
    bar = 4.0 * measured
    assert bar <= 1e-5
    lens = "aperture { 2 } focal_length { 50 } focus_distance { 7 }" if camera == "ThinLens" else ""
    renderer.upload(Scene.from_string(WHITE.replace("CAMERA", camera).replace("LENS", lens).replace("SAMPLER", "Independent { seed { 7 } }")
                                      .replace("Kd : Constant { v { 1 } }", "Kd : Constant { v { 0 } }").replace("resolution { 24, 16 }", "resolution { 128, 64 }")))
    records = gather_records(renderer)
    n = len(records)
    streams = np.arange(n, dtype=np.uint32) * np.uint32(13) + np.uint32(5)
    worst = 0.0
    for s in (0, 5, 6, 9):
        got = renderer.irradiance(records, spp=1, spp_begin=s, streams=streams, clamp=1e9, raw=True)
        g = renderer.gather_vertex(records, sample=s, streams=streams)
        ok = np.asarray(g.valid)
        assert np.array_equal(got[:, 3], ok.astype(np.float32)) and not got[~ok].any()
        rays, shadow = np.ascontiguousarray(g.rays), np.ascontiguousarray(g.shadow)
        visible = ~renderer.trace(shadow, any_hit=True) & (g.light_pdf > 0)
        found = renderer.light_evaluate(renderer.trace(rays), rays)
        weight = np.where(g.pdf > 0, g.pdf / np.maximum(g.pdf + found.pdf, np.float32(1e-30)), np.float32(0))
        want = np.where(visible[:, None], g.nee, np.float32(0)) + g.beta * found.L * weight[:, None]
        scale = np.maximum(np.abs(want).max(1), np.abs(got[:, :3]).max(1))
        lit = ok & (scale > 0)
        assert lit.sum() > 150
        d = float((np.abs(got[lit, :3].astype(np.float64) - want[lit]).max(1) / scale[lit]).max())
        worst = max(worst, d)
        with capsys.disabled():
            print(f"\n[irradiance = plan] {camera} sample {s}: {int(lit.sum())} lit records, largest relative difference {d:.3e}", end="")
        assert (got[ok & ~lit, :3] == 0).all()
    assert worst <= bar, (worst, bar)


def test_the_irradiance_estimator_against_the_radiance_query(renderer, capsys):
    """the whole estimator, statistically: Cornell with its coloured walls, depth 8, Independent sampler, 16 records over floor, walls, boxes
    and ceiling, 4096 samples each on distinct streams (16 sample indices x 256 streams).  The reference is pi x radiance() along
    cosine-distributed rays -- the directions gather_vertex gives, so the same directions -- the existing query and, the texel being the
    path's camera end, the same integral.  For each record and channel the means agree within 5 sqrt(sd_a^2 / S + sd_b^2 / S); for the
    records in direct view of the light the gather's standard deviation is below the reference's.  MEASURED on the MI355X:
    largest |z| 1.84 over the 48 means, E from 0.003 to 1.2; sigma gather / reference 0.093 in the median, at most 0.178 for the 11 records in
    direct view (0.96 at most elsewhere)"""
    from luisarender_amd.scenes import cornell_box
    renderer.upload(Scene.from_string(cornell_box(resolution=128, spp=8, depth=8)))
    records, _ = cornell_records(renderer)
    points = renderer.surface(records, geometry_only=True)
    valid = np.nonzero(np.asarray(points.valid) & ~np.asarray(points.has_light))[0]
    pick = valid[np.linspace(0, len(valid) - 1, 16).astype(np.int64)]
    assert len(set(pick.tolist())) == 16 and len(np.unique(np.round(points.ng[pick], 1), axis=0)) >= 4  # floor, walls, boxes, ceiling
    copies, calls = 256, 16
    batch = np.ascontiguousarray(np.tile(records[pick], (copies, 1)))
    streams = np.arange(len(batch), dtype=np.uint32) + np.uint32(17)  # 4096 < 128 x 128: all different
    a, b = [], []
    for s in range(calls):
        raw = renderer.irradiance(batch, spp=1, spp_begin=s, streams=streams, clamp=1e9, raw=True)
        assert (raw[:, 3] == 1).all()
        a.append(raw[:, :3])
        g = renderer.gather_vertex(batch, sample=s, streams=streams)
        # (streams of its own: on the record's stream the query would draw, at the ray's first hit, the very numbers the ray's direction
        # was made of, and the bounce would be correlated with the ray -- a biased reference, |z| = 10 on the short box's front)
        ref = renderer.radiance(np.ascontiguousarray(g.rays), spp=1, spp_begin=s, streams=streams + np.uint32(8192), clamp=1e9, raw=True)
        b.append(np.float32(np.pi) * np.where((g.pdf > 0)[:, None], ref[:, :3], np.float32(0)))
    n = calls * copies
    a = np.stack(a).astype(np.float64).reshape(n, 16, 3)
    b = np.stack(b).astype(np.float64).reshape(n, 16, 3)
    mean_a, mean_b, sd_a, sd_b = a.mean(0), b.mean(0), a.std(0, ddof=1), b.std(0, ddof=1)
    z = np.abs(mean_a - mean_b) / np.sqrt(sd_a ** 2 / n + sd_b ** 2 / n)
    # in direct view of the light: the centre of the ceiling light above the record's horizon, the segment to it free
    p0, ng = points.p[pick].astype(np.float64), points.ng[pick].astype(np.float64)
    to_lamp = np.array([278.0, 548.7, 279.5]) - p0
    distance = np.linalg.norm(to_lamp, axis=1)
    segment = np.zeros((16, 8), np.float32)
    segment[:, 0:3], segment[:, 4:7], segment[:, 7] = p0 + 1e-3 * distance[:, None] * ng, to_lamp / distance[:, None], distance * 0.99
    in_view = ~renderer.trace(segment, any_hit=True) & (np.einsum("nk,nk->n", ng, to_lamp / distance[:, None]) > 0.2)
    with capsys.disabled():
        print(f"\n[irradiance estimator] {n} samples x 16 records: largest |z| {z.max():.2f}, E from {mean_a.min():.3f} to {mean_a.max():.3f}, "
              f"sigma gather / reference: median {np.median(sd_a / sd_b):.3f}, largest {np.max(sd_a / sd_b):.3f}; in direct view "
              f"{int(in_view.sum())} of 16, sigma ratio there at most {np.max((sd_a / sd_b)[in_view]) if in_view.any() else float('nan'):.3f}", end="")
    assert mean_a.min() > 0 and (z < 5.0).all(), z
    assert in_view.sum() >= 4 and (sd_a[in_view] < sd_b[in_view]).all()


def test_irradiance_chunks_refinement_and_torch(renderer):
    """spp = 16 over 70 records is cut into several sample chunks whose partial planes are summed in another order than sixteen spp = 1 calls
    add up: the bound is float32 summation error, relative 16 x 2^-24 per component, times 4.  accumulate_into over [0, 8) then [8, 16): the
    same bound.  A torch tensor in gives a torch tensor out on the device, the numpy path's bits at spp = 1"""
    import torch
    from luisarender_amd.scenes import cornell_box
    renderer.upload(Scene.from_string(cornell_box(resolution=128, spp=8)))
    records, streams = cornell_records(renderer, n=70)
    bound = 16 * 2.0 ** -24 * 4
    single = np.zeros((70, 4), np.float64)
    for s in range(16):
        single += renderer.irradiance(records, spp=1, spp_begin=s, streams=streams, raw=True)
    whole = renderer.irradiance(records, spp=16, streams=streams, raw=True)
    assert np.array_equal(whole[:, 3], single[:, 3]) and set(whole[:, 3].tolist()) == {0.0, 16.0}
    assert (np.abs(whole[:, :3] - single[:, :3]) <= bound * np.abs(single[:, :3])).all()
    refined = renderer.irradiance(records, spp=8, streams=streams, raw=True)
    again = renderer.irradiance(records, spp=8, spp_begin=8, streams=streams, accumulate_into=refined, raw=True)
    assert again is refined and np.array_equal(refined[:, 3], single[:, 3])
    assert (np.abs(refined[:, :3] - single[:, :3]) <= bound * np.abs(single[:, :3])).all()
    means = renderer.irradiance(records, spp=16, streams=streams)
    assert means.shape == (70, 3) and np.array_equal(means, whole[:, :3] / np.maximum(whole[:, 3:4], np.float32(1)))
    device = torch.device("cuda", 0)
    t = renderer.irradiance(torch.from_numpy(records).to(device), spp=1, spp_begin=3, streams=torch.from_numpy(streams.view(np.int32)).to(device), raw=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    assert np.array_equal(bits(t.cpu().numpy()), bits(renderer.irradiance(records, spp=1, spp_begin=3, streams=streams, raw=True)))


def test_irradiance_edges_that_must_not_fault_or_hang(renderer):
    from luisarender_amd.scenes import cornell_box
    text = cornell_box(resolution=128, spp=8)
    renderer.upload(Scene.from_string(text))
    records, streams = cornell_records(renderer, n=70)
    valid = np.asarray(renderer.surface(records, geometry_only=True).valid)
    misses = np.zeros((70, 8), np.float32)
    misses.view(np.uint32)[:, 3:6] = INVALID
    assert not renderer.irradiance(misses, spp=4, raw=True).any()
    assert renderer.irradiance(records[:0].copy(), spp=4, raw=True).shape == (0, 4) and renderer.last_gather_ms() == 0.0
    kept = np.full((70, 4), 3.0, np.float32)
    assert renderer.irradiance(records, spp=0, spp_begin=7, raw=True).any() == False  # noqa: E712  (spp_begin >= spp_end: the sums of no sample)
    assert np.array_equal(renderer.irradiance(records, spp=0, spp_begin=7, accumulate_into=kept, raw=True), np.full((70, 4), 3.0, np.float32))
    # bare points: zero and NaN normals, a non-finite point
    surface = renderer.surface(records, geometry_only=True)
    p, nrm = np.ascontiguousarray(surface.p[valid][:8]), np.ascontiguousarray(surface.ng[valid][:8])
    nrm[0], nrm[1, 2], p[2, 1] = 0.0, np.nan, np.inf
    pts = renderer.irradiance(points=p, normals=nrm, spp=4, raw=True)
    assert pts[:, 3].tolist() == [0, 0, 0, 4, 4, 4, 4, 4] and not pts[:3].any() and np.isfinite(pts).all() and (pts[3:, :3].sum(1) > 0).any()
    same = renderer.irradiance(points=np.ascontiguousarray(surface.p[valid]), normals=np.ascontiguousarray(surface.ng[valid]), spp=64, streams=np.ascontiguousarray(streams[valid]))
    assert np.isfinite(same).all() and same.mean() > 0
    # a depth-0 scene: no ray starts, every valid record counts its samples with E = 0, and the call returns
    # (the scene language raises depth { 0 } to 1, so the depth is set in the host's tables, which upload() reads)
    shallow = Scene.from_string(cornell_box(resolution=128, spp=8, depth=1))
    assert shallow.view().integrator.max_depth == 1
    shallow.view().integrator.max_depth = 0
    renderer.upload(shallow)
    assert not renderer.gather_vertex(records, sample=2, streams=streams).nee.any()  # the plan: no light sample either
    flat = renderer.irradiance(records, spp=5, streams=streams, raw=True)
    assert np.array_equal(flat[:, 3], 5.0 * valid) and not flat[:, :3].any()
    # a scene without lighting: zeros, nothing launched
    dark = Scene.from_string(WHITE.replace("CAMERA", "Pinhole").replace("LENS", "").replace("SAMPLER", "Independent { }")
                             .replace("environment : Spherical { emission : Constant { v { 0.5, 0.6, 0.8 } } }", "")
                             .replace("light : Diffuse { emission : Constant { v { 12, 11, 9 } } two_sided { true } }", "surface { @white }"))
    renderer.upload(dark)
    assert not renderer.irradiance(gather_records(renderer), spp=4, raw=True).any() and renderer.last_gather_ms() == 0.0
    lib, ctx = renderer._lib, renderer._ctx
    q = _ffi.GatherParams()
    q.count, q.spp_end, q.clamp = 4, 1, -1.0
    assert lib.lrhip_gather_irradiance(ctx, q) == -1 and b"clamp" in lib.lrhip_last_error()
    q.clamp = 0.0
    assert lib.lrhip_gather_irradiance(ctx, q) == -1 and b"NULL" in lib.lrhip_last_error()
    q.flags = 1024
    assert lib.lrhip_gather_irradiance(ctx, q) == -1 and b"unknown flags" in lib.lrhip_last_error()
