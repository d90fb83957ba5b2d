"""Camera, sampler and film queries (include/lrhip.h: lrhip_query_sampler, lrhip_query_camera, lrhip_film_splat), the parts that
need no GPU: the ctypes mirrors against a C translation unit of the header, the exported symbols, the draw codes and the flag, the
NULL-argument returns, pattern parsing and the argument checks of MegaPathRenderer.sampler_start / sampler_draw / camera_rays / film_splat."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from luisarender_amd import _ffi
from luisarender_amd.render import (CameraRays, MegaPathRenderer, check_camera_args, check_sampler_args, check_splat_args,
                                    parse_sampler_pattern)

LRHIP_ERROR_INVALID = -1
LAYOUTS = (("lrhip_sampler_query_params", _ffi.SamplerQueryParams,
            ("state", "streams", "indices", "pattern", "out", "count", "pattern_count", "sample_index", "flags", "reserved"), 64),
           ("lrhip_camera_sample", _ffi.CameraSample, ("weight", "film_x", "film_y", "pixel"), 16),
           ("lrhip_camera_query_params", _ffi.CameraQueryParams, ("pixels", "u", "out_rays", "out", "count", "flags", "reserved"), 48),
           ("lrhip_film_splat_params", _ffi.FilmSplatParams, ("pixels", "values", "count", "flags", "clamp"), 32))
VALUES = ("LRHIP_DRAW_1D", "LRHIP_DRAW_2D", "LRHIP_DRAW_PIXEL_2D", "LRHIP_SAMPLER_MAX_DRAWS", "LRHIP_SAMPLER_START", "LRHIP_RAY_DEVICE_POINTERS",
          "LR_INVALID_ID")


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of the four mirrors, and the draw codes and the flag, against what the host compiler makes of lrhip.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"', "int main(void) {"]
    for name, _, fields, _ in LAYOUTS:
        lines += [f'    printf("%zu\\n", sizeof({name}));'] + [f'    printf("%zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['    printf("' + " ".join(["%u"] * len(VALUES)) + '\\n", ' + ", ".join(VALUES) + ");", "    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    host = _ffi.host_lib()
    row = 0
    for name, st, fields, size in LAYOUTS:
        assert [f for f, _ in st._fields_] == list(fields), name
        assert C.sizeof(st) == int(out[row]) == size, name
        for f, line in zip(fields, out[row + 1:]):
            assert getattr(st, f).offset == int(line), (name, f)
        row += 1 + len(fields)
        assert _ffi.STRUCTS[name] is st and host.lrhost_sizeof(name.encode()) == C.sizeof(st), name
    assert [int(v) for v in out[row].split()] == [_ffi.DRAW_1D, _ffi.DRAW_2D, _ffi.DRAW_PIXEL_2D, _ffi.SAMPLER_MAX_DRAWS, _ffi.SAMPLER_START,
                                                  _ffi.RAY_DEVICE_POINTERS, 0xFFFFFFFF]


def test_camera_sample_is_one_row_of_four_words():
    st = _ffi.CameraSample
    assert (st.weight.offset, st.film_x.offset, st.film_y.offset, st.pixel.offset) == (0, 4, 8, 12) and C.sizeof(st) == 16


def test_codes_and_flag():
    assert (_ffi.DRAW_1D, _ffi.DRAW_2D, _ffi.DRAW_PIXEL_2D) == (0, 1, 2) and _ffi.SAMPLER_MAX_DRAWS == 64  # 64 two-bit codes in four words
    others = (_ffi.RAY_DEVICE_POINTERS, _ffi.RAY_ALPHA_TEST, _ffi.RADIANCE_ACCUMULATE, _ffi.RADIANCE_COUNTERS, _ffi.MESH_RECOMPUTE_NORMALS,
              _ffi.SURFACE_GEOMETRY_ONLY, _ffi.LIGHT_FROM_POINTS)
    assert _ffi.SAMPLER_START == 128 and all(_ffi.SAMPLER_START & o == 0 for o in others)  # the queries' flags share one word


def test_library_exports_the_entry_points():
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))  # loads without a GPU; nothing is called
    for name in ("lrhip_query_sampler", "lrhip_query_camera", "lrhip_film_splat", "lrhip_last_camera_ms"):
        assert hasattr(lib, name), name
    for name in ("sampler_start", "sampler_draw", "camera_rays", "camera_samples", "film_splat", "last_camera_ms"):
        assert hasattr(MegaPathRenderer, name), name


def test_null_arguments_are_invalid_without_a_device():
    lib = _ffi.hip_lib()
    for entry, params in ((lib.lrhip_query_sampler, _ffi.SamplerQueryParams()), (lib.lrhip_query_camera, _ffi.CameraQueryParams()),
                          (lib.lrhip_film_splat, _ffi.FilmSplatParams())):
        assert entry(None, C.byref(params)) == LRHIP_ERROR_INVALID
        assert entry.__name__.encode() in lib.lrhip_last_error()
        assert entry(None, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_last_camera_ms(None) == 0.0


def test_pattern_parsing():
    assert parse_sampler_pattern("") == ([], 0)
    assert parse_sampler_pattern("p2" + "1212") == ([2, 1, 0, 1, 0, 1], 10)
    codes, floats = parse_sampler_pattern("2" * 64)
    assert len(codes) == 64 and floats == 128
    assert parse_sampler_pattern("1" * 64) == ([0] * 64, 64)
    for bad in ("1" * 65, "2" * 65, "p" + "2" * 64, "3", "12x", "P", "1 2", None, 12, ["1"]):  # 65 entries; more than 128 floats; unknown characters
        with pytest.raises(ValueError, match="sampler"):
            parse_sampler_pattern(bad)


def test_sampler_argument_checks():
    ids, state = np.zeros(5, np.uint32), np.zeros((5, 4), np.uint32)
    assert check_sampler_args(count=7) == "numpy" and check_sampler_args(count=0) == "numpy"
    assert check_sampler_args(streams=ids, sample=3) == "numpy" and check_sampler_args(indices=ids) == "numpy"
    assert check_sampler_args(streams=ids, indices=ids, count=5, sample=0xFFFFFFFF) == "numpy"
    assert check_sampler_args(state, "p2") == "numpy" and check_sampler_args(np.zeros((0, 4), np.uint32), "") == "numpy"
    bad = [
        dict(),                                                        # start: streams, indices or count
        dict(count=-1), dict(count=1 << 31), dict(count=2.0), dict(count=True),
        dict(count=5, sample=-1), dict(count=5, sample=1 << 32), dict(count=5, sample=1.0),
        dict(streams=ids, count=4),                                    # counts differ
        dict(streams=ids, indices=np.zeros(4, np.uint32)),
        dict(streams=ids.astype(np.int32)), dict(streams=ids.astype(np.float32)), dict(indices=ids.astype(np.int64)),  # dtype
        dict(streams=np.zeros((5, 1), np.uint32)), dict(streams=np.zeros(10, np.uint32)[::2]),                          # shape, strides
        dict(count=5, pattern="1x"),
        dict(state=state, pattern="1" * 65),
        dict(state=state, streams=ids), dict(state=state, count=5), dict(state=state, indices=ids),                    # draw: a state and a pattern
        dict(state=np.zeros((5, 4), np.int32)), dict(state=np.zeros((5, 4), np.float32)), dict(state=np.zeros((5, 3), np.uint32)),
        dict(state=np.zeros(20, np.uint32)), dict(state=np.zeros((5, 8), np.uint32)[:, :4]),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError, match="sampler"):
            check_sampler_args(**kwargs)
    for kwargs in (dict(streams=[0, 1, 2]), dict(state=[[0] * 4] * 5), dict(indices=(1, 2))):
        with pytest.raises(TypeError, match="sampler"):
            check_sampler_args(**kwargs)


def test_camera_and_splat_argument_checks():
    u4, u2, ids = np.zeros((5, 4), np.float32), np.zeros((5, 2), np.float32), np.zeros(5, np.uint32)
    assert check_camera_args(u4) == "numpy" and check_camera_args(u2, ids) == "numpy" and check_camera_args(u4, None, 5) == "numpy"
    assert check_camera_args(np.zeros((0, 4), np.float32), np.zeros(0, np.uint32)) == "numpy"
    assert check_camera_args(np.zeros((9, 4), np.float32), np.zeros(9, np.uint32), 5) == "numpy"  # with pixels the frame does not bound N
    for kwargs in (dict(u=u4, pixel_count=4), dict(u=np.zeros((5, 3), np.float32)), dict(u=np.zeros((5, 4), np.float64)), dict(u=np.zeros(20, np.float32)),
                   dict(u=np.zeros((5, 8), np.float32)[:, :4]), dict(u=u4, pixels=np.zeros(4, np.uint32)), dict(u=u4, pixels=ids.astype(np.int32)),
                   dict(u=u4, pixels=np.zeros((5, 1), np.uint32)), dict(u=u4, pixels=np.zeros(10, np.uint32)[::2])):
        with pytest.raises(ValueError, match="camera"):
            check_camera_args(**kwargs)
    for kwargs in (dict(u=[[0.0] * 4] * 5), dict(u=u4, pixels=[0] * 5)):
        with pytest.raises(TypeError, match="camera"):
            check_camera_args(**kwargs)
    v4, v3 = np.zeros((5, 4), np.float32), np.zeros((5, 3), np.float32)
    assert check_splat_args(v4) == "numpy" and check_splat_args(v3, ids, 2.5, 5) == "numpy" and check_splat_args(v4, None, None, 5) == "numpy"
    for kwargs in (dict(values=v4, pixel_count=4), dict(values=np.zeros((5, 2), np.float32)), dict(values=np.zeros((5, 4), np.float64)),
                   dict(values=np.zeros((5, 8), np.float32)[:, :4]), dict(values=v4, pixels=np.zeros(6, np.uint32)), dict(values=v4, pixels=ids.astype(np.int64)),
                   dict(values=v4, clamp=0.0), dict(values=v4, clamp=-1.0), dict(values=v4, clamp=float("inf")), dict(values=v4, clamp=float("nan"))):
        with pytest.raises(ValueError, match="splat"):
            check_splat_args(**kwargs)
    with pytest.raises(TypeError, match="splat"):
        check_splat_args([[0.0] * 4] * 5)


def test_camera_rays_are_views_of_their_buffers():
    buffer = np.arange(3 * 4, dtype=np.float32).reshape(3, 4)
    buffer.view(np.uint32)[:, 3] = (7, 0xFFFFFFFF, 4095)
    rays = np.arange(3 * 8, dtype=np.float32).reshape(3, 8) + 100.0
    r = CameraRays(rays, buffer)
    assert len(r) == 3 and r.buffer is buffer and r.rays is rays
    assert np.shares_memory(r.weight, buffer) and np.array_equal(r.weight, buffer[:, 0])
    assert r.film_xy.shape == (3, 2) and np.shares_memory(r.film_xy, buffer) and np.array_equal(r.film_xy, buffer[:, 1:3])
    assert r.pixel.dtype == np.uint32 and r.pixel.tolist() == [7, 0xFFFFFFFF, 4095] and np.shares_memory(r.pixel, buffer)
    assert r.valid.tolist() == [True, False, True]
