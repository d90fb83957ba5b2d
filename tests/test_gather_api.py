"""Lightmap texels (include/lrhip.h: lrhip_lightmap_texels), the parts that need no GPU: the flag values and the record layout
against a C translation unit of the header, the exported symbols, the NULL-argument returns, the argument checks of
MegaPathRenderer.lightmap_texels and the views of LightmapTexels."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from luisarender_amd import _ffi
from luisarender_amd.render import LightmapTexels, MegaPathRenderer, RayHits, check_lightmap_args, check_surface_args

LRHIP_ERROR_INVALID = -1
HIT_FIELDS = ("t", "u", "v", "inst", "prim", "tri", "reserved")
VALUES = ("LRHIP_LIGHTMAP_CONSERVATIVE", "LRHIP_LIGHTMAP_TEXEL_CENTRE", "LRHIP_LIGHTMAP_TEXEL_TOUCHED", "LRHIP_RAY_DEVICE_POINTERS", "LR_INVALID_ID")


def test_values_and_the_record_layout_match_the_header(tmp_path):
    """the flag values, and sizeof and every field offset of the lrhip_ray_hit a texel record is, against what the host compiler makes of
    lrhip.h; the prototype of lrhip_lightmap_texels is called through a function pointer of the type the bindings assume"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"',
             "typedef int (*texels_fn)(lrhip_ctx *, uint32_t, uint32_t, uint32_t, uint32_t, void *);",
             "typedef double (*ms_fn)(lrhip_ctx *);", "int main(void) {",
             # (typeof is not evaluated: the prototypes are checked, the symbols are not needed to link)
             "    texels_fn f = (__typeof__(&lrhip_lightmap_texels))0; ms_fn g = (__typeof__(&lrhip_last_lightmap_ms))0; (void)f; (void)g;",
             '    printf("%zu\\n", sizeof(lrhip_ray_hit));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_ray_hit, {f}));' for f in HIT_FIELDS]
    lines += ['    printf("' + " ".join(["%u"] * len(VALUES)) + '\\n", ' + ", ".join(VALUES) + ");", "    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [name for name, _ in _ffi.RayHit._fields_] == list(HIT_FIELDS)
    assert C.sizeof(_ffi.RayHit) == int(out[0]) == 32
    for f, line in zip(HIT_FIELDS, out[1:]):
        assert getattr(_ffi.RayHit, f).offset == int(line), f
    assert _ffi.RayHit.reserved.offset == 24  # word 6 of the record: the texel's flags
    assert [int(v) for v in out[1 + len(HIT_FIELDS)].split()] == [_ffi.LIGHTMAP_CONSERVATIVE, _ffi.LIGHTMAP_TEXEL_CENTRE, _ffi.LIGHTMAP_TEXEL_TOUCHED,
                                                                 _ffi.RAY_DEVICE_POINTERS, 0xFFFFFFFF]


def test_flag_values():
    assert (_ffi.LIGHTMAP_TEXEL_CENTRE, _ffi.LIGHTMAP_TEXEL_TOUCHED) == (1, 2)
    # the queries' flags share one word: the new bit is none of the others
    others = (_ffi.RAY_DEVICE_POINTERS, _ffi.RAY_ALPHA_TEST, _ffi.RADIANCE_ACCUMULATE, _ffi.RADIANCE_COUNTERS, _ffi.MESH_RECOMPUTE_NORMALS,
              _ffi.SURFACE_GEOMETRY_ONLY, _ffi.LIGHT_FROM_POINTS, _ffi.SAMPLER_START)
    assert _ffi.LIGHTMAP_CONSERVATIVE == 256 and all(_ffi.LIGHTMAP_CONSERVATIVE & o == 0 for o in others)


def test_library_exports_the_entry_points():
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))  # loads without a GPU; nothing is called
    for name in ("lrhip_lightmap_texels", "lrhip_last_lightmap_ms"):
        assert hasattr(lib, name), name
    assert all(hasattr(MegaPathRenderer, name) for name in ("lightmap_texels", "last_lightmap_ms"))


def test_null_arguments_are_invalid_without_a_device():
    lib = _ffi.hip_lib()
    out = np.zeros((4, 8), np.float32)
    assert lib.lrhip_lightmap_texels(None, 0, 2, 2, 0, out.ctypes.data) == LRHIP_ERROR_INVALID
    assert b"lrhip_lightmap_texels" in lib.lrhip_last_error()
    assert lib.lrhip_lightmap_texels(None, 0, 0, 0, 0, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_last_lightmap_ms(None) == 0.0
    assert not out.any()


def test_argument_checks():
    assert check_lightmap_args(0, 64, 64) == 4096 and check_lightmap_args(3, 33, 17, 4) == 561
    assert check_lightmap_args(np.uint32(1), np.int64(5), 0) == 0  # an empty map is legal
    assert check_lightmap_args(0, 46340, 46340) == 46340 * 46340 and check_lightmap_args(0, 0x7FFFFFFF, 1) == 0x7FFFFFFF
    bad = [dict(instance=-1, width=4, height=4), dict(instance=0, width=-4, height=4), dict(instance=0, width=4, height=2 ** 32),
           dict(instance=0, width=4.0, height=4), dict(instance=0, width=True, height=4), dict(instance="0", width=4, height=4),
           dict(instance=None, width=4, height=4),
           dict(instance=4, width=4, height=4, instance_count=4),    # instance out of range, where the count is known
           dict(instance=0, width=65536, height=32768),              # 2^31 texels: one more than a call takes
           dict(instance=0, width=2 ** 31, height=1)]
    for kwargs in bad:
        with pytest.raises(ValueError, match="lightmap"):
            check_lightmap_args(**kwargs)


def test_results_are_views_of_their_buffer():
    buffer = np.arange(6 * 8, dtype=np.float32).reshape(6, 8)
    words = buffer.view(np.uint32)
    words[:, 3], words[:, 4], words[:, 5] = 2, (7, 8, 9, 10, 11, 12), 0xFFFFFFFF
    words[:, 6] = (1, 2, 1, 0, 2, 1)
    words[3, 3] = words[3, 4] = 0xFFFFFFFF  # a texel nobody owns: the miss record
    r = LightmapTexels(buffer, 3, 2)
    assert isinstance(r, RayHits) and len(r) == 6 and r.buffer is buffer and (r.width, r.height) == (3, 2)
    for view in (r.t, r.u, r.v, r.inst, r.prim, r.tri, r.flags):
        assert np.shares_memory(view, buffer)
    assert np.array_equal(r.u, buffer[:, 1]) and np.array_equal(r.v, buffer[:, 2])
    assert r.flags.dtype == np.uint32 and r.flags.tolist() == [1, 2, 1, 0, 2, 1] and r.prim.tolist() == [7, 8, 9, 0xFFFFFFFF, 11, 12]
    assert r.covered.tolist() == r.hit.tolist() == [True, True, True, False, True, True]
    assert r.centre.tolist() == [True, False, True, False, False, True] and r.touched.tolist() == [False, True, False, False, True, False]
    # the queries take the records as they stand
    assert check_surface_args(r) == "numpy" and check_surface_args(r.buffer) == "numpy"


# ---------------------------------------------------------------- the gather vertex query (lrhip_query_gather_vertex)

VERTEX_FIELDS = ("ray", "shadow", "nee", "light_pdf", "beta", "pdf")
VERTEX_PARAM_FIELDS = ("records", "normals", "streams", "out", "count", "sample_index", "flags")


def test_gather_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of _ffi.GatherVertex and _ffi.GatherVertexParams, and LRHIP_GATHER_FROM_POINTS, against what the host
    compiler makes of lrhip.h"""
    from luisarender_amd.render import GatherVertices  # noqa: F401
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"', "int main(void) {", '    printf("%zu\\n", sizeof(lrhip_gather_vertex));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_gather_vertex, {f}));' for f in VERTEX_FIELDS]
    lines += ['    printf("%zu\\n", sizeof(lrhip_gather_vertex_params));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_gather_vertex_params, {f}));' for f in VERTEX_PARAM_FIELDS]
    lines += ['    printf("%u %u\\n", LRHIP_GATHER_FROM_POINTS, LRHIP_LIGHT_FROM_POINTS);', "    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    row = 0
    for st, fields, size in ((_ffi.GatherVertex, VERTEX_FIELDS, 96), (_ffi.GatherVertexParams, VERTEX_PARAM_FIELDS, None)):
        assert [name for name, _ in st._fields_] == list(fields)
        assert C.sizeof(st) == int(out[row]) and (size is None or C.sizeof(st) == size)
        for f, line in zip(fields, out[row + 1:]):
            assert getattr(st, f).offset == int(line), f
        row += 1 + len(fields)
    assert [int(v) for v in out[row].split()] == [_ffi.GATHER_FROM_POINTS, _ffi.LIGHT_FROM_POINTS] == [64, 64]
    assert _ffi.STRUCTS["lrhip_gather_vertex"] is _ffi.GatherVertex and _ffi.STRUCTS["lrhip_gather_vertex_params"] is _ffi.GatherVertexParams
    host = _ffi.host_lib()  # lrhost_sizeof knows both
    for name, st in (("lrhip_gather_vertex", _ffi.GatherVertex), ("lrhip_gather_vertex_params", _ffi.GatherVertexParams)):
        assert host.lrhost_sizeof(name.encode()) == C.sizeof(st), name


def test_gather_entry_points_and_null_arguments():
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))  # loads without a GPU; nothing is called
    for name in ("lrhip_query_gather_vertex", "lrhip_last_gather_ms"):
        assert hasattr(lib, name), name
    assert all(hasattr(MegaPathRenderer, name) for name in ("gather_vertex", "last_gather_ms"))
    lib = _ffi.hip_lib()
    p = _ffi.GatherVertexParams()
    assert lib.lrhip_query_gather_vertex(None, C.byref(p)) == LRHIP_ERROR_INVALID
    assert b"lrhip_query_gather_vertex" in lib.lrhip_last_error()
    assert lib.lrhip_query_gather_vertex(None, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_last_gather_ms(None) == 0.0


def test_gather_argument_checks():
    from luisarender_amd.render import check_gather_args
    hits = np.zeros((5, 8), np.float32)
    p3, p4, n3, n4 = np.zeros((5, 3), np.float32), np.zeros((5, 4), np.float32), np.ones((5, 3), np.float32), np.ones((5, 4), np.float32)
    streams = np.arange(5, dtype=np.uint32)
    assert check_gather_args(hits) == "numpy" and check_gather_args(RayHits(hits), sample=7, streams=streams) == "numpy"
    assert check_gather_args(LightmapTexels(hits, 5, 1)) == "numpy"
    assert check_gather_args(points=p3, normals=n3) == "numpy" and check_gather_args(points=p4, normals=n3, streams=streams) == "numpy"
    assert check_gather_args(points=p3, normals=n4) == "numpy" and check_gather_args(points=p4, normals=n4, sample=2 ** 32 - 1) == "numpy"
    assert check_gather_args(points=np.zeros((5, 6), np.float32)[:, :3], normals=n3) == "numpy"  # an [N, 3] array is copied: any strides
    assert check_gather_args(np.zeros((0, 8), np.float32)) == "numpy"
    bad = [
        dict(),                                                       # hits or points, one of them
        dict(hits=hits, points=p3, normals=n3),
        dict(points=p3),                                              # points and normals go together
        dict(hits=hits, normals=n3),
        dict(hits=np.zeros((5, 7), np.float32)),                      # hits: check_surface_args is reused
        dict(hits=np.zeros((5, 8), np.float64)),
        dict(hits=np.zeros((10, 8), np.float32)[::2]),
        dict(points=np.zeros((5, 2), np.float32), normals=n3),        # shape, dtype, strides, counts
        dict(points=p3, normals=np.zeros((5, 5), np.float32)),
        dict(points=np.zeros((5, 3), np.float64), normals=n3),
        dict(points=p3, normals=np.zeros((5, 3), np.float64)),
        dict(points=np.zeros((5, 8), np.float32)[:, :4], normals=n3),
        dict(points=p3, normals=np.zeros((5, 8), np.float32)[:, :4]),
        dict(points=p3, normals=np.ones((4, 3), np.float32)),
        dict(points=p4, normals=np.ones((6, 4), np.float32)),
        dict(hits=hits, sample=-1), dict(hits=hits, sample=2 ** 32), dict(hits=hits, sample=1.0), dict(hits=hits, sample=True),
        dict(hits=hits, streams=np.arange(5, dtype=np.int64)),        # streams: uint32 [N], contiguous
        dict(hits=hits, streams=np.arange(4, dtype=np.uint32)),
        dict(hits=hits, streams=np.arange(10, dtype=np.uint32)[::2]),
        dict(hits=hits, streams=np.zeros((5, 1), np.uint32)),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError, match="gather"):
            check_gather_args(**kwargs)
    for kwargs in (dict(hits=[[0.0] * 8] * 5), dict(points=[[0.0] * 3] * 5, normals=n3), dict(points=p3, normals=[[0.0] * 3] * 5),
                   dict(hits=hits, streams=[0, 1, 2, 3, 4])):
        with pytest.raises(TypeError, match="gather"):
            check_gather_args(**kwargs)


def test_gather_vertices_are_views_of_their_buffer():
    from luisarender_amd.render import GatherVertices
    buffer = np.arange(3 * 24, dtype=np.float32).reshape(3, 24) + 1.0
    buffer[1] = 0.0  # the invalid record
    g = GatherVertices(buffer)
    assert len(g) == 3 and g.buffer is buffer
    for view, columns in ((g.rays, slice(0, 8)), (g.shadow, slice(8, 16)), (g.nee, slice(16, 19)), (g.beta, slice(20, 23))):
        assert np.shares_memory(view, buffer) and np.array_equal(view, buffer[:, columns])
    assert np.array_equal(g.light_pdf, buffer[:, 19]) and np.array_equal(g.pdf, buffer[:, 23]) and np.shares_memory(g.pdf, buffer)
    assert g.valid.tolist() == [True, False, True]


# ---------------------------------------------------------------- the irradiance call (lrhip_gather_irradiance)

GATHER_PARAM_FIELDS = ("records", "normals", "streams", "out", "count", "spp_begin", "spp_end", "flags", "clamp")


def test_irradiance_params_layout_values_and_symbols(tmp_path):
    """sizeof and every field offset of _ffi.GatherParams and the values of LRHIP_GATHER_ACCUMULATE / LRHIP_FEAT_GATHER against the header; the
    entry point is exported and answers NULL arguments without a device"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"', "int main(void) {", '    printf("%zu\\n", sizeof(lrhip_gather_params));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_gather_params, {f}));' for f in GATHER_PARAM_FIELDS]
    lines += ['    printf("%u %u %u %u\\n", LRHIP_GATHER_ACCUMULATE, LRHIP_RADIANCE_ACCUMULATE, LRHIP_FEAT_GATHER, LRHIP_FEAT_QUERY);', "    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    st = _ffi.GatherParams
    assert [name for name, _ in st._fields_] == list(GATHER_PARAM_FIELDS) and C.sizeof(st) == int(out[0])
    for f, line in zip(GATHER_PARAM_FIELDS, out[1:]):
        assert getattr(st, f).offset == int(line), f
    assert [int(v) for v in out[1 + len(GATHER_PARAM_FIELDS)].split()] == [_ffi.GATHER_ACCUMULATE, _ffi.RADIANCE_ACCUMULATE, _ffi.FEAT_GATHER, _ffi.FEAT_QUERY]
    assert (_ffi.GATHER_ACCUMULATE, _ffi.FEAT_GATHER) == (4, 131072)
    assert _ffi.STRUCTS["lrhip_gather_params"] is st and _ffi.host_lib().lrhost_sizeof(b"lrhip_gather_params") == C.sizeof(st)
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))
    assert hasattr(lib, "lrhip_gather_irradiance") and hasattr(MegaPathRenderer, "irradiance")
    for mask in (196732, 196734, 197244, 197246):  # the four gather kernels: all closures x {Independent, generic} x {plain, nested}
        assert hasattr(lib, f"lrhip_variant_launch_{mask}"), mask
        assert mask & (_ffi.FEAT_GATHER | _ffi.FEAT_QUERY | 124) == _ffi.FEAT_GATHER | _ffi.FEAT_QUERY | 124 and mask & 1 == 0
    lib = _ffi.hip_lib()
    p = st()
    assert lib.lrhip_gather_irradiance(None, C.byref(p)) == LRHIP_ERROR_INVALID and b"lrhip_gather_irradiance" in lib.lrhip_last_error()
    assert lib.lrhip_gather_irradiance(None, None) == LRHIP_ERROR_INVALID


def test_irradiance_argument_checks():
    from luisarender_amd.render import check_irradiance_args
    hits, acc = np.zeros((5, 8), np.float32), np.zeros((5, 4), np.float32)
    p3, n3 = np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32)
    assert check_irradiance_args(hits) == "numpy" and check_irradiance_args(hits, spp=16, spp_begin=8, clamp=10.0, accumulate_into=acc) == "numpy"
    assert check_irradiance_args(points=p3, normals=n3, spp=0, streams=np.arange(5, dtype=np.uint32), accumulate_into=acc) == "numpy"
    assert check_irradiance_args(hits, spp=2 ** 32 - 1) == "numpy"
    bad = [dict(hits=hits, spp=-1), dict(hits=hits, spp_begin=-1), dict(hits=hits, spp=2 ** 32), dict(hits=hits, spp=1, spp_begin=2 ** 32 - 1),
           dict(hits=hits, spp=1.0), dict(hits=hits, spp=True),
           dict(hits=hits, clamp=0.0), dict(hits=hits, clamp=-1.0), dict(hits=hits, clamp=float("inf")), dict(hits=hits, clamp=float("nan")),
           dict(hits=hits, accumulate_into=np.zeros((4, 4), np.float32)), dict(hits=hits, accumulate_into=np.zeros((5, 3), np.float32)),
           dict(hits=hits, accumulate_into=np.zeros((5, 4), np.float64)), dict(hits=hits, accumulate_into=np.zeros((5, 8), np.float32)[:, :4]),
           dict(hits=hits, points=p3, normals=n3), dict(points=p3), dict()]  # the records: check_gather_args' rules
    for kwargs in bad:
        with pytest.raises(ValueError, match="gather"):
            check_irradiance_args(**kwargs)
    with pytest.raises(TypeError, match="gather"):
        check_irradiance_args(hits, accumulate_into=[[0.0] * 4] * 5)
