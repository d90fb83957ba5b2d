"""Surface queries (include/lrhip.h: lrhip_query_surface), the parts that need no GPU: the ctypes mirrors of the record and the
parameter struct against a C translation unit of the header, the exported symbols, the flag bits, the NULL-argument returns and the argument
checks of MegaPathRenderer.surface."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from luisarender_amd import _ffi
from luisarender_amd.render import RayHits, SurfacePoints, check_surface_args

LRHIP_ERROR_INVALID = -1
POINT_FIELDS = ("p", "area", "ng", "flags", "ns", "inst", "tangent", "prim", "n_closure", "closure_kind", "uv", "roughness", "albedo", "surface",
                "emission", "light")
PARAM_FIELDS = ("hits", "rays", "out", "count", "flags")
FLAGS = ("LRHIP_SURFACE_VALID", "LRHIP_SURFACE_BACK_FACING", "LRHIP_SURFACE_HAS_SURFACE", "LRHIP_SURFACE_HAS_LIGHT", "LRHIP_SURFACE_GEOMETRY_ONLY",
         "LRHIP_RAY_DEVICE_POINTERS")


def _header():
    return open(os.path.join(_ffi.REPO_ROOT, "include", "lrhip.h")).read()


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of _ffi.SurfacePoint and _ffi.SurfaceQueryParams, and the flag values, against what the host compiler
    makes of lrhip.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(lrhip_surface_point));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_surface_point, {f}));' for f in POINT_FIELDS]
    lines += ['    printf("%zu\\n", sizeof(lrhip_surface_query_params));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_surface_query_params, {f}));' for f in PARAM_FIELDS]
    lines += ['    printf("' + " ".join(["%u"] * len(FLAGS)) + '\\n", ' + ", ".join(FLAGS) + ");", "    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    row = 0
    for st, fields, size in ((_ffi.SurfacePoint, POINT_FIELDS, 128), (_ffi.SurfaceQueryParams, PARAM_FIELDS, None)):
        assert [name for name, _ in st._fields_] == list(fields)
        assert C.sizeof(st) == int(out[row]) and (size is None or C.sizeof(st) == size)
        for f, line in zip(fields, out[row + 1:]):
            assert getattr(st, f).offset == int(line), f
        row += 1 + len(fields)
    assert [int(v) for v in out[row].split()] == [_ffi.SURFACE_VALID, _ffi.SURFACE_BACK_FACING, _ffi.SURFACE_HAS_SURFACE, _ffi.SURFACE_HAS_LIGHT,
                                                  _ffi.SURFACE_GEOMETRY_ONLY, _ffi.RAY_DEVICE_POINTERS]
    assert _ffi.STRUCTS["lrhip_surface_point"] is _ffi.SurfacePoint and _ffi.STRUCTS["lrhip_surface_query_params"] is _ffi.SurfaceQueryParams


def test_record_is_eight_rows_of_four_words():
    """every float3 of the record starts a 16-byte row and an id or scalar closes it: eight dwordx4 stores"""
    st = _ffi.SurfacePoint
    for k, name in enumerate(("p", "ng", "ns", "tangent", "n_closure", "uv", "albedo", "emission")):
        assert getattr(st, name).offset == 16 * k, name
    for k, name in enumerate(("area", "flags", "inst", "prim", "closure_kind", None, "surface", "light")):
        assert name is None or getattr(st, name).offset == 16 * k + 12, name
    assert st.roughness.offset == 88


def test_library_exports_the_entry_points():
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))  # loads without a GPU; nothing is called
    for name in ("lrhip_query_surface", "lrhip_last_surface_ms"):
        assert hasattr(lib, name), name


def test_geometry_only_collides_with_no_flag_of_the_other_queries():
    """the calls that share LRHIP_RAY_DEVICE_POINTERS keep their flag bits apart: one word of flags can be told apart wherever it goes"""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    names = ("LRHIP_RAY_DEVICE_POINTERS", "LRHIP_RAY_ALPHA_TEST", "LRHIP_RADIANCE_ACCUMULATE", "LRHIP_RADIANCE_COUNTERS",
             "LRHIP_MESH_RECOMPUTE_NORMALS", "LRHIP_SURFACE_GEOMETRY_ONLY")
    bits = {name: int(value) for name, value in re.findall(r"#define\s+(LRHIP_[A-Z_]+)\s+(\d+)u", text) if name in names}
    assert set(bits) == set(names)
    assert bits["LRHIP_SURFACE_GEOMETRY_ONLY"] == 32 == _ffi.SURFACE_GEOMETRY_ONLY
    for name, value in bits.items():
        assert value & (value - 1) == 0, name
    assert len(set(bits.values())) == len(bits)


def test_null_arguments_are_invalid_without_a_device():
    lib = _ffi.hip_lib()
    p = _ffi.SurfaceQueryParams()
    assert lib.lrhip_query_surface(None, C.byref(p)) == LRHIP_ERROR_INVALID
    assert b"lrhip_query_surface" in lib.lrhip_last_error()
    assert lib.lrhip_query_surface(None, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_last_surface_ms(None) == 0.0


def test_argument_checks():
    hits, rays = np.zeros((5, 8), np.float32), np.zeros((5, 8), np.float32)
    assert check_surface_args(hits) == "numpy"
    assert check_surface_args(hits, rays) == "numpy"
    assert check_surface_args(None, rays) == "numpy"
    assert check_surface_args(RayHits(hits), rays) == "numpy"
    assert check_surface_args(np.zeros((0, 8), np.float32)) == "numpy"
    bad = [
        dict(),                                                  # neither
        dict(hits=np.zeros((5, 7), np.float32)),                 # shape
        dict(hits=np.zeros((5, 32), np.float32)),
        dict(hits=np.zeros(8, np.float32)),
        dict(hits=np.zeros((5, 8), np.float64)),                 # dtype
        dict(hits=np.zeros((5, 8), np.uint32)),
        dict(hits=np.zeros((5, 16), np.float32)[:, :8]),         # not contiguous
        dict(hits=np.zeros((10, 8), np.float32)[::2]),
        dict(hits=[[0.0] * 8] * 5),                              # not an array
        dict(hits=hits, rays=np.zeros((4, 8), np.float32)),      # counts differ
        dict(hits=hits, rays=np.zeros((5, 7), np.float32)),      # check_rays is reused
        dict(hits=hits, rays=np.zeros((5, 8), np.float64)),
        dict(hits=hits, rays=np.zeros((10, 8), np.float32)[::2]),
        dict(rays=np.zeros((5, 6), np.float32)),
        dict(hits=RayHits(np.zeros((5, 8), np.float32)), rays=np.zeros((6, 8), np.float32)),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError):
            check_surface_args(**kwargs)
    with pytest.raises(ValueError, match="surface: hits"):
        check_surface_args(np.zeros((5, 7), np.float32))


def test_surface_points_are_views_of_one_buffer():
    buffer = np.arange(3 * 32, dtype=np.float32).reshape(3, 32)
    words = buffer.view(np.uint32)
    words[:, 7] = (0, 1 | 4, 1 | 2 | 8)
    words[:, [11, 15, 19, 27, 31]] = 0xFFFFFFFF
    s = SurfacePoints(buffer)
    assert len(s) == 3 and s.buffer is buffer
    for name, first, width in (("p", 0, 3), ("ng", 4, 3), ("ns", 8, 3), ("tangent", 12, 3), ("n_closure", 16, 3), ("uv", 20, 2), ("roughness", 22, 2),
                               ("albedo", 24, 3), ("emission", 28, 3)):
        a = getattr(s, name)
        assert a.shape == (3, width) and np.shares_memory(a, buffer) and np.array_equal(a, buffer[:, first:first + width]), name
    assert np.array_equal(s.area, buffer[:, 3]) and np.shares_memory(s.area, buffer)
    for name in ("inst", "prim", "closure_kind", "surface", "light"):
        assert getattr(s, name).dtype == np.uint32 and (getattr(s, name) == 0xFFFFFFFF).all(), name
    assert s.valid.tolist() == [False, True, True] and s.back_facing.tolist() == [False, False, True]
    assert s.has_surface.tolist() == [False, True, False] and s.has_light.tolist() == [False, False, True]
