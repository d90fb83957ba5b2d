"""Light queries (include/lrhip.h: lrhip_query_light), the parts that need no GPU: the ctypes mirrors of the result and the
parameter struct against a C translation unit of the header, the exported symbols, the mode, kind and flag values, the NULL-argument returns
and the argument checks of MegaPathRenderer.light_sample / light_evaluate."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from luisarender_amd import _ffi
from luisarender_amd.render import LightResults, LightSamples, MegaPathRenderer, RayHits, check_light_args

LRHIP_ERROR_INVALID = -1
RESULT_FIELDS = ("L", "pdf", "kind", "reserved")
PARAM_FIELDS = ("hits", "rays", "dirs", "out_rays", "out", "count", "mode", "flags")
VALUES = ("LRHIP_LIGHT_SAMPLE", "LRHIP_LIGHT_EVALUATE", "LRHIP_LIGHT_KIND_AREA", "LRHIP_LIGHT_KIND_ENVIRONMENT", "LRHIP_LIGHT_KIND_NONE",
          "LRHIP_LIGHT_FROM_POINTS", "LRHIP_RAY_DEVICE_POINTERS", "LR_INVALID_ID")


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of _ffi.LightResult and _ffi.LightQueryParams, and the mode, kind and flag values, against what the host
    compiler makes of lrhip.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(lrhip_light_result));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_light_result, {f}));' for f in RESULT_FIELDS]
    lines += ['    printf("%zu\\n", sizeof(lrhip_light_query_params));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_light_query_params, {f}));' for f in PARAM_FIELDS]
    lines += ['    printf("' + " ".join(["%u"] * len(VALUES)) + '\\n", ' + ", ".join(VALUES) + ");", "    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    row = 0
    for st, fields, size in ((_ffi.LightResult, RESULT_FIELDS, 32), (_ffi.LightQueryParams, PARAM_FIELDS, None)):
        assert [name for name, _ in st._fields_] == list(fields)
        assert C.sizeof(st) == int(out[row]) and (size is None or C.sizeof(st) == size)
        for f, line in zip(fields, out[row + 1:]):
            assert getattr(st, f).offset == int(line), f
        row += 1 + len(fields)
    assert [int(v) for v in out[row].split()] == [_ffi.LIGHT_SAMPLE, _ffi.LIGHT_EVALUATE, _ffi.LIGHT_KIND_AREA, _ffi.LIGHT_KIND_ENVIRONMENT,
                                                  _ffi.LIGHT_KIND_NONE, _ffi.LIGHT_FROM_POINTS, _ffi.RAY_DEVICE_POINTERS, 0xFFFFFFFF]
    assert _ffi.STRUCTS["lrhip_light_result"] is _ffi.LightResult and _ffi.STRUCTS["lrhip_light_query_params"] is _ffi.LightQueryParams
    host = _ffi.host_lib()  # lrhost_sizeof knows both
    for name, st in (("lrhip_light_result", _ffi.LightResult), ("lrhip_light_query_params", _ffi.LightQueryParams)):
        assert host.lrhost_sizeof(name.encode()) == C.sizeof(st), name


def test_result_is_two_rows_of_four_words():
    """(L, pdf) and (kind, three reserved words): two dwordx4 stores"""
    st = _ffi.LightResult
    assert (st.L.offset, st.pdf.offset, st.kind.offset, st.reserved.offset) == (0, 12, 16, 20) and C.sizeof(st) == 32


def test_mode_kind_and_flag_values():
    assert (_ffi.LIGHT_SAMPLE, _ffi.LIGHT_EVALUATE) == (0, 1)
    assert (_ffi.LIGHT_KIND_AREA, _ffi.LIGHT_KIND_ENVIRONMENT, _ffi.LIGHT_KIND_NONE) == (0, 1, 2)
    # the queries' flags share one word: the new bit is none of the others
    others = (_ffi.RAY_DEVICE_POINTERS, _ffi.RAY_ALPHA_TEST, _ffi.RADIANCE_ACCUMULATE, _ffi.RADIANCE_COUNTERS, _ffi.MESH_RECOMPUTE_NORMALS,
              _ffi.SURFACE_GEOMETRY_ONLY)
    assert _ffi.LIGHT_FROM_POINTS == 64 and all(_ffi.LIGHT_FROM_POINTS & o == 0 for o in others)


def test_library_exports_the_entry_points():
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))  # loads without a GPU; nothing is called
    for name in ("lrhip_query_light", "lrhip_last_light_ms"):
        assert hasattr(lib, name), name
    assert all(hasattr(MegaPathRenderer, name) for name in ("light_sample", "light_evaluate", "last_light_ms"))


def test_null_arguments_are_invalid_without_a_device():
    lib = _ffi.hip_lib()
    p = _ffi.LightQueryParams()
    assert lib.lrhip_query_light(None, C.byref(p)) == LRHIP_ERROR_INVALID
    assert b"lrhip_query_light" in lib.lrhip_last_error()
    assert lib.lrhip_query_light(None, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_last_light_ms(None) == 0.0


def test_argument_checks():
    hits, rays = np.zeros((5, 8), np.float32), np.zeros((5, 8), np.float32)
    u3, u4, p3, p4 = np.zeros((5, 3), np.float32), np.zeros((5, 4), np.float32), np.zeros((5, 3), np.float32), np.zeros((5, 4), np.float32)
    assert check_light_args(hits, u3) == "numpy"
    assert check_light_args(RayHits(hits), u4) == "numpy"
    assert check_light_args(None, u3, p3) == "numpy" and check_light_args(None, u4, p4) == "numpy"
    assert check_light_args(hits, np.zeros((5, 6), np.float32)[:, :3]) == "numpy"  # an [N, 3] array is copied: any strides
    assert check_light_args(None, u3, np.zeros((5, 6), np.float32)[:, :3]) == "numpy"
    assert check_light_args(np.zeros((0, 8), np.float32), np.zeros((0, 4), np.float32)) == "numpy"
    assert check_light_args(hits, rays=rays, mode="evaluate") == "numpy"
    assert check_light_args(RayHits(hits), None, None, rays, None, "evaluate") == "numpy"
    bad = [
        dict(hits=np.zeros((5, 7), np.float32), u=u3),               # hits: check_surface_args is reused
        dict(hits=np.zeros((5, 8), np.float64), u=u3),
        dict(hits=np.zeros((10, 8), np.float32)[::2], u=u3),
        dict(hits=hits, u=np.zeros((5, 2), np.float32)),             # shape
        dict(hits=hits, u=np.zeros((5, 5), np.float32)),
        dict(hits=hits, u=np.zeros(3, np.float32)),
        dict(hits=hits, u=np.zeros((5, 3), np.float64)),             # dtype
        dict(hits=hits, u=np.zeros((5, 8), np.float32)[:, :4]),      # an [N, 4] array is read in place: contiguous
        dict(hits=hits, u=np.zeros((4, 3), np.float32)),             # counts differ
        dict(points=p3, u=np.zeros((6, 4), np.float32)),
        dict(points=np.zeros((5, 2), np.float32), u=u3),             # points: shape, dtype, strides
        dict(points=np.zeros((5, 3), np.float64), u=u3),
        dict(points=np.zeros((5, 8), np.float32)[:, :4], u=u3),
        dict(hits=hits, points=p3, u=u3),                            # hits or points, one of them
        dict(u=u3),
        dict(hits=hits),                                             # sample mode needs u
        dict(hits=hits, u=u3, rays=rays),                            # ... and reads no rays
        dict(hits=hits, u=u3, mode="both"),
        dict(hits=hits, rays=rays, u=u3, mode="evaluate"),           # evaluate mode: hits and rays, nothing else
        dict(hits=hits, rays=rays, points=p3, mode="evaluate"),
        dict(hits=hits, mode="evaluate"),
        dict(rays=rays, mode="evaluate"),
        dict(hits=hits, rays=np.zeros((4, 8), np.float32), mode="evaluate"),
        dict(hits=hits, rays=np.zeros((5, 7), np.float32), mode="evaluate"),
        dict(hits=hits, rays=np.zeros((5, 8), np.float64), mode="evaluate"),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError, match="light"):
            check_light_args(**kwargs)
    for kwargs in (dict(hits=[[0.0] * 8] * 5, u=u3), dict(hits=hits, u=[[0.0] * 3] * 5), dict(points=[[0.0] * 3] * 5, u=u3),
                   dict(hits=hits, rays=[[0.0] * 8] * 5, mode="evaluate")):
        with pytest.raises(TypeError, match="light"):
            check_light_args(**kwargs)


def test_results_are_views_of_their_buffers():
    buffer = np.arange(3 * 8, dtype=np.float32).reshape(3, 8)
    buffer.view(np.uint32)[:, 4] = (0, 0xFFFFFFFF, 2)
    rays = np.arange(3 * 8, dtype=np.float32).reshape(3, 8) + 100.0
    for r in (LightResults(buffer), LightSamples(rays, buffer)):
        assert len(r) == 3 and r.buffer is buffer
        assert r.L.shape == (3, 3) and np.shares_memory(r.L, buffer) and np.array_equal(r.L, buffer[:, 0:3])
        assert np.array_equal(r.pdf, buffer[:, 3]) and np.shares_memory(r.pdf, buffer)
        assert r.kind.dtype == np.uint32 and r.kind.tolist() == [0, 0xFFFFFFFF, 2] and np.shares_memory(r.kind, buffer)
        assert r.valid.tolist() == [True, False, True]
    s = LightSamples(rays, buffer)
    assert s.rays is rays and s.rays.shape == (3, 8) and isinstance(s, LightResults)  # two buffers: the rays go into trace() as they stand
