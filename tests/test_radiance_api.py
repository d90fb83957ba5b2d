"""Radiance queries (include/lrhip.h: lrhip_trace_radiance), the parts that need no GPU: the ctypes mirror of the parameter
struct against a C translation unit of the header, the exported symbols, the feature bit, the NULL-argument returns and the argument
checks of MegaPathRenderer.radiance."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from luisarender_amd import _ffi
from luisarender_amd.render import check_radiance_args

LRHIP_ERROR_INVALID = -1
FIELDS = ("rays", "streams", "out", "count", "spp_begin", "spp_end", "flags", "clamp")


def _header():
    return open(os.path.join(_ffi.REPO_ROOT, "include", "lrhip.h")).read()


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of _ffi.RadianceQueryParams, and the flag values, against what the host compiler makes of lrhip.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(lrhip_radiance_query_params));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_radiance_query_params, {f}));' for f in FIELDS]
    lines += ['    printf("%u %u %u %u\\n", LRHIP_RADIANCE_ACCUMULATE, LRHIP_RADIANCE_COUNTERS, LRHIP_RAY_DEVICE_POINTERS, LRHIP_FEAT_QUERY);',
              "    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    st = _ffi.RadianceQueryParams
    assert [name for name, _ in st._fields_] == list(FIELDS)
    assert C.sizeof(st) == int(out[0])
    for f, line in zip(FIELDS, out[1:]):
        assert getattr(st, f).offset == int(line), f
    assert [int(v) for v in out[1 + len(FIELDS)].split()] == [_ffi.RADIANCE_ACCUMULATE, _ffi.RADIANCE_COUNTERS, _ffi.RAY_DEVICE_POINTERS,
                                                              _ffi.FEAT_QUERY]
    assert _ffi.STRUCTS["lrhip_radiance_query_params"] is st


def test_library_exports_the_entry_points():
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))  # loads without a GPU; nothing is called
    for name in ("lrhip_trace_radiance", "lrhip_last_radiance_ms"):
        assert hasattr(lib, name), name


def test_feature_bit_collides_with_no_other():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    bits = {name: int(value) for name, value in re.findall(r"#define\s+(LRHIP_FEAT_[A-Z_]+)\s+(\d+)u", text)}
    assert bits["LRHIP_FEAT_QUERY"] == 65536 and len(bits) >= 14
    for name, value in bits.items():
        assert value & (value - 1) == 0, name  # every feature is one bit
        assert name == "LRHIP_FEAT_QUERY" or value != bits["LRHIP_FEAT_QUERY"], name
    assert len(set(bits.values())) == len(bits)


def test_null_arguments_are_invalid_without_a_device():
    lib = _ffi.hip_lib()
    p = _ffi.RadianceQueryParams()
    assert lib.lrhip_trace_radiance(None, C.byref(p)) == LRHIP_ERROR_INVALID
    assert b"lrhip_trace_radiance" in lib.lrhip_last_error()
    assert lib.lrhip_trace_radiance(None, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_last_radiance_ms(None) == 0.0


def test_argument_checks():
    rays = np.zeros((5, 8), np.float32)
    assert check_radiance_args(rays) == "numpy"
    assert check_radiance_args(rays, spp=0, spp_begin=7, streams=np.arange(5, dtype=np.uint32), clamp=10.0,
                               accumulate_into=np.zeros((5, 4), np.float32)) == "numpy"
    bad = [
        dict(streams=np.arange(5, dtype=np.int64)),             # dtype
        dict(streams=np.arange(5, dtype=np.float32)),
        dict(streams=np.arange(4, dtype=np.uint32)),            # shape
        dict(streams=np.zeros((5, 1), np.uint32)),
        dict(streams=np.arange(10, dtype=np.uint32)[::2]),      # not contiguous
        dict(streams=[0, 1, 2, 3, 4]),                          # not an array
        dict(spp=-1),
        dict(spp_begin=-1),
        dict(spp=1.5),
        dict(spp=2, spp_begin=0xFFFFFFFF),
        dict(clamp=0.0),
        dict(clamp=-1.0),
        dict(clamp=float("nan")),
        dict(clamp=float("inf")),
        dict(accumulate_into=np.zeros((5, 3), np.float32)),     # shape
        dict(accumulate_into=np.zeros((4, 4), np.float32)),
        dict(accumulate_into=np.zeros((5, 4), np.float64)),     # dtype
        dict(accumulate_into=np.zeros((5, 8), np.float32)[:, :4]),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError):
            check_radiance_args(rays, **kwargs)
    for bad_rays in (np.zeros((5, 7), np.float32), np.zeros((5, 8), np.float64), np.zeros(8, np.float32)):  # check_rays is reused
        with pytest.raises(ValueError):
            check_radiance_args(bad_rays)
