"""The numpy UV rasteriser the device kernels are held to (tests/gather_reference.py; include/lrhip.h: lrhip_lightmap_texels) against hand-made
charts whose answers can be said without it: one triangle, a quad of two triangles that share an edge, a mirrored chart, triangles without
area, a chart partly outside [0, 1]^2, the conservative mode -- and the band of texel centres within 2^-20 of an edge, which the GPU tests
allow to go either way and which therefore has to be nearly empty for the charts they use."""
import numpy as np
import pytest

import gather_reference as G
import mesh_deform_scene as M
from luisarender_amd import Scene

SIZES = ((64, 64), (33, 17))


def centres(width, height):
    t = np.arange(width * height)
    return (t % width + 0.5) / width, (t // width + 0.5) / height


def brute_force_inside(chart, prim, width, height):
    """texel centres strictly inside triangle `prim`, by three cross products written out by hand in float64"""
    uvs, triangles = chart
    a, b, c = (uvs[int(i)].astype(np.float64) for i in triangles[prim])
    cx, cy = centres(width, height)
    d0 = (b[0] - a[0]) * (cy - a[1]) - (b[1] - a[1]) * (cx - a[0])
    d1 = (c[0] - b[0]) * (cy - b[1]) - (c[1] - b[1]) * (cx - b[0])
    d2 = (a[0] - c[0]) * (cy - c[1]) - (a[1] - c[1]) * (cx - c[0])
    return ((d0 > 0) & (d1 > 0) & (d2 > 0)) | ((d0 < 0) & (d1 < 0) & (d2 < 0))


@pytest.mark.parametrize("size", SIZES)
def test_one_triangle(size):
    w, h = size
    r = G.rasterise(*G.ONE_TRIANGLE, w, h)
    inside = brute_force_inside(G.ONE_TRIANGLE, 0, w, h)
    assert inside.sum() > w * h // 4
    assert np.array_equal(r.owner != G.NO_OWNER, inside) and not r.band.any()
    assert (r.prim[inside] == 0).all() and (r.flags[inside] == G.FLAG_CENTRE).all()
    assert (r.prim[~inside] == G.NO_OWNER).all() and (r.flags[~inside] == 0).all() and (r.u[~inside] == 0).all()
    # the record's barycentrics give the centre back: p = (1 - u - v) a + u b + v c
    cx, cy = centres(w, h)
    p = G.chart_point(*G.ONE_TRIANGLE, r.prim[inside], r.u[inside], r.v[inside])
    assert np.abs(p - np.stack([cx, cy], 1)[inside]).max() < 2e-7
    assert (r.u >= 0).all() and (r.v >= 0).all() and (r.u + r.v <= 1).all()
    assert (r.triangle_distance[inside] == 0).all() and (r.triangle_distance[~inside] > 0).all()


@pytest.mark.parametrize("size", SIZES)
def test_a_quad_of_two_triangles_has_one_owner_per_texel(size):
    w, h = size
    r = G.rasterise(*G.QUAD, w, h)
    cx, cy = centres(w, h)
    x, y = (cx - G._O[0]) / G._S[0], (cy - G._O[1]) / G._S[1]  # the quad's own coordinates
    in_quad = (x > 0) & (x < 1) & (y > 0) & (y < 1)
    assert np.array_equal(r.owner != G.NO_OWNER, in_quad) and not r.band.any()
    # below the diagonal: prim 0 (0, 1, 2); above it: prim 1
    assert np.array_equal(r.prim[in_quad] == 0, (x >= y)[in_quad]) and set(r.prim[in_quad].tolist()) == {0, 1}


def test_every_texel_on_a_shared_edge_goes_to_the_lower_prim():
    """the unit quad on a square map: the diagonal passes through the centres of the texels (i, i) exactly, both triangles cover them, and
    the lower prim owns each of them -- once"""
    w = h = 16
    r = G.rasterise(*G.UNIT_QUAD, w, h)
    diagonal = np.arange(w) * w + np.arange(w)
    assert (r.edge_distance[diagonal] == 0).all()
    assert (r.prim[diagonal] == 0).all() and (r.flags[diagonal] == G.FLAG_CENTRE).all()
    assert (r.u[diagonal] == 0).all() and np.array_equal(r.v[diagonal], ((np.arange(w) + 0.5) / w).astype(np.float32))  # on the edge a -> c
    assert (r.owner != G.NO_OWNER).all() and (r.prim == 0).sum() == w * (w + 1) // 2 and (r.prim == 1).sum() == w * (w - 1) // 2
    for prim in (0, 1):  # each triangle alone covers the diagonal too
        alone = G.rasterise(G.UNIT_QUAD[0], G.UNIT_QUAD[1][prim:prim + 1], w, h)
        assert (alone.owner[diagonal] == 0).all()


@pytest.mark.parametrize("size", SIZES)
def test_a_mirrored_chart_is_covered_like_the_original(size):
    w, h = size
    a, b = G.rasterise(*G.QUAD, w, h), G.rasterise(*G.FLIPPED, w, h)
    assert np.array_equal(a.owner, b.owner) and (a.owner != G.NO_OWNER).sum() > w * h // 2
    # (0, 1, 2) -> (0, 2, 1): the roles of u and v swap
    assert np.array_equal(a.u, b.v) and np.array_equal(a.v, b.u)


@pytest.mark.parametrize("conservative", (False, True))
def test_triangles_without_area_own_nothing(conservative):
    w, h = 64, 64
    r = G.rasterise(*G.DEGENERATE, w, h, conservative)
    assert [t[0] for t in G.sound_triangles(*G.DEGENERATE)] == [2]
    owned = r.owner != G.NO_OWNER
    assert owned.sum() > w * h // 4 and (r.prim[owned] == 2).all()
    alone = G.rasterise(G.DEGENERATE[0], G.DEGENERATE[1][2:3], w, h, conservative)
    assert np.array_equal(alone.owner != G.NO_OWNER, owned) and np.array_equal(alone.u, r.u) and np.array_equal(alone.v, r.v)
    # indices outside the mesh and non-finite UVs: the same
    uvs = G.DEGENERATE[0].copy()
    uvs[1] = (np.nan, 0.5)
    tris = np.array([(0, 1, 3), (0, 3, 9), (0, 3, 2)], np.uint32)
    assert [t[0] for t in G.sound_triangles(uvs, tris)] == [2]
    assert np.array_equal(G.rasterise(uvs, tris, w, h, conservative).owner, r.owner)


@pytest.mark.parametrize("size", SIZES)
def test_a_chart_partly_outside_the_unit_square(size):
    w, h = size
    r = G.rasterise(*G.OUTSIDE, w, h)
    inside = brute_force_inside(G.OUTSIDE, 0, w, h) | brute_force_inside(G.OUTSIDE, 1, w, h)
    assert 0 < inside.sum() < w * h and np.array_equal((r.owner != G.NO_OWNER) & ~r.band, inside & ~r.band)
    # nothing wraps: the same chart moved by a whole unit covers nothing
    far = G.rasterise(G.OUTSIDE[0] + np.float32(2.0), G.OUTSIDE[1], w, h, conservative=True)
    assert (far.owner == G.NO_OWNER).all()
    huge = G.rasterise(G.OUTSIDE[0] * np.float32(1e30), G.OUTSIDE[1], w, h)  # any finite UV is safe
    assert set(np.unique(huge.prim).tolist()) <= {0, 1, G.NO_OWNER}


@pytest.mark.parametrize("chart", ("ONE_TRIANGLE", "QUAD", "OUTSIDE", "FAN"))
@pytest.mark.parametrize("size", SIZES)
def test_conservative_mode(chart, size):
    w, h = size
    uvs, triangles = getattr(G, chart)
    plain, r = G.rasterise(uvs, triangles, w, h), G.rasterise(uvs, triangles, w, h, conservative=True)
    centre = plain.owner != G.NO_OWNER
    # every centre-covered texel keeps its record
    assert np.array_equal(r.owner[centre], plain.owner[centre]) and np.array_equal(r.u[centre], plain.u[centre])
    assert np.array_equal(r.v[centre], plain.v[centre]) and (r.flags[centre] == G.FLAG_CENTRE).all()
    touched = r.flags == G.FLAG_TOUCHED
    assert touched.sum() > 0 and not (touched & centre).any() and np.array_equal(touched, (r.owner != G.NO_OWNER) & ~centre)
    assert ((r.owner[touched] & G.TOUCHED) != 0).all()
    # every touched texel's point lies on its triangle, as near to the centre as the triangle comes
    cx, cy = centres(w, h)
    c = np.stack([cx, cy], 1)[touched]
    p = G.chart_point(uvs, triangles, r.prim[touched], r.u[touched], r.v[touched])
    assert G.distance_to_triangle(uvs, triangles, r.prim[touched], p).max() < 2e-7
    assert (r.u >= 0).all() and (r.v >= 0).all() and (r.u + r.v <= 1).all()
    nearest = G.distance_to_triangle(uvs, triangles, r.prim[touched], c)
    assert np.abs(np.hypot(*(p - c).T) - nearest).max() < 2e-7
    # no texel further than half a texel diagonal from every triangle is owned, and every texel whose square a triangle crosses is
    half_diagonal = 0.5 * np.hypot(1.0 / w, 1.0 / h)
    assert (r.triangle_distance[r.owner != G.NO_OWNER] <= half_diagonal).all()
    assert (r.owner[r.triangle_distance < 0.5 * min(1.0 / w, 1.0 / h) - 1e-12] != G.NO_OWNER).all()


def test_the_band_is_nearly_empty_for_the_charts_of_the_gpu_tests():
    """the GPU tests let a texel whose centre is within 2^-20 of an edge go either way, and allow 2 % of the texels there: the reference
    alone stays under 1 % for every chart and size they use, the icosphere's included"""
    scene = M.room()
    ids = M.check_room(scene)
    ball = (scene.mesh_uvs(ids["ball_mesh"]), scene.mesh_triangles(ids["ball_mesh"]))
    assert ball[0].shape == (642, 2) and ball[1].shape == (1280, 3) and ball[0].min() >= 0.0 and ball[0].max() <= 1.0
    for name, chart in (("quad", G.QUAD), ("fan", G.FAN), ("ball", ball)):
        for w, h in SIZES:
            for conservative in (False, True):
                r = G.rasterise(*chart, w, h, conservative)
                assert r.band.mean() < 0.01, (name, w, h, r.band.mean())
                assert (r.owner != G.NO_OWNER).sum() > w * h // 8, (name, w, h)
    # the icosphere has edges on the meridian u = 1/2 and on the equator v = 1/2, and the centres of column 16 and row 8 of a 33 x 17 map lie
    # on them EXACTLY: 17 texels of 561, 3 %.  Their edge function is an exact 0.0 on both sides, so they are not left to the band but judged
    # like every other texel
    r = G.rasterise(*ball, 33, 17)
    on = np.nonzero(r.on_edge)[0]
    assert len(on) == 17 and ((on % 33 == 16) | (on // 33 == 8)).all() and not (r.band & r.on_edge).any()
    assert (r.edge_distance <= G.EPSILON).mean() > 0.02  # (with them the band would be over the 2 % the GPU test allows)
    assert (r.prim[r.on_edge] != G.NO_OWNER).all()


def test_scene_tables_hold_the_charts_bit_for_bit():
    """Scene.mesh_uvs / mesh_triangles: an InlineMesh written by gather_reference.inline_mesh comes back with the chart's own float32 UVs"""
    text = "\n".join([G.inline_mesh("quad", G.QUAD), G.inline_mesh("fan", G.FAN),
                      "Camera cam : Pinhole { spp { 1 } film : Color { resolution { 8, 8 } } position { 0.5, 0.5, 3 } look_at { 0.5, 0.5, 0 } fov { 40 } }",
                      "render { cameras { @cam } shapes { @quad, @fan } integrator : MegaPath { depth { 2 } sampler : Independent { } } }"])
    scene = Scene.from_string(text)
    for instance, chart in enumerate((G.QUAD, G.FAN)):
        mesh = scene.instance_mesh(instance)
        assert np.array_equal(scene.mesh_uvs(mesh), chart[0]) and scene.mesh_uvs(mesh).dtype == np.float32
        assert np.array_equal(scene.mesh_triangles(mesh), chart[1]) and scene.mesh_triangles(mesh).dtype == np.uint32
        assert int(scene.view().instances[instance].handle.x) & 2  # LR_SHAPE_HAS_VERTEX_UV
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="out of range"):
            scene.mesh_uvs(bad)
        with pytest.raises(ValueError, match="out of range"):
            scene.mesh_triangles(bad)
