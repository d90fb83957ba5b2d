"""BSDF queries (include/lrhip.h: lrhip_query_bsdf), the parts that need no GPU: the ctypes mirrors of the result and the
parameter struct against a C translation unit of the header, the exported symbols, the mode, flag and event values, the NULL-argument returns
and the argument checks of MegaPathRenderer.bsdf_evaluate / bsdf_sample."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from luisarender_amd import _ffi
from luisarender_amd.render import BsdfResults, MegaPathRenderer, RayHits, check_bsdf_args

LRHIP_ERROR_INVALID = -1
RESULT_FIELDS = ("f", "pdf", "wi", "event")
PARAM_FIELDS = ("hits", "rays", "dirs", "out", "count", "mode", "flags")
VALUES = ("LRHIP_BSDF_EVALUATE", "LRHIP_BSDF_SAMPLE", "LRHIP_BSDF_EVENT_REFLECT", "LRHIP_BSDF_EVENT_ENTER", "LRHIP_BSDF_EVENT_EXIT",
          "LRHIP_BSDF_EVENT_THROUGH", "LRHIP_RAY_DEVICE_POINTERS", "LR_INVALID_ID")


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of _ffi.BsdfResult and _ffi.BsdfQueryParams, and the mode, event and flag values, against what the host
    compiler makes of lrhip.h"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrhip.h"', "int main(void) {",
             '    printf("%zu\\n", sizeof(lrhip_bsdf_result));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_bsdf_result, {f}));' for f in RESULT_FIELDS]
    lines += ['    printf("%zu\\n", sizeof(lrhip_bsdf_query_params));']
    lines += [f'    printf("%zu\\n", offsetof(lrhip_bsdf_query_params, {f}));' for f in PARAM_FIELDS]
    lines += ['    printf("' + " ".join(["%u"] * len(VALUES)) + '\\n", ' + ", ".join(VALUES) + ");", "    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(_ffi.REPO_ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    row = 0
    for st, fields, size in ((_ffi.BsdfResult, RESULT_FIELDS, 32), (_ffi.BsdfQueryParams, PARAM_FIELDS, None)):
        assert [name for name, _ in st._fields_] == list(fields)
        assert C.sizeof(st) == int(out[row]) and (size is None or C.sizeof(st) == size)
        for f, line in zip(fields, out[row + 1:]):
            assert getattr(st, f).offset == int(line), f
        row += 1 + len(fields)
    assert [int(v) for v in out[row].split()] == [_ffi.BSDF_EVALUATE, _ffi.BSDF_SAMPLE, _ffi.BSDF_EVENT_REFLECT, _ffi.BSDF_EVENT_ENTER,
                                                  _ffi.BSDF_EVENT_EXIT, _ffi.BSDF_EVENT_THROUGH, _ffi.RAY_DEVICE_POINTERS, 0xFFFFFFFF]
    assert _ffi.STRUCTS["lrhip_bsdf_result"] is _ffi.BsdfResult and _ffi.STRUCTS["lrhip_bsdf_query_params"] is _ffi.BsdfQueryParams
    host = _ffi.host_lib()  # lrhost_sizeof knows both
    for name, st in (("lrhip_bsdf_result", _ffi.BsdfResult), ("lrhip_bsdf_query_params", _ffi.BsdfQueryParams)):
        assert host.lrhost_sizeof(name.encode()) == C.sizeof(st), name


def test_result_is_two_rows_of_four_words():
    """(f, pdf) and (wi, event): each float3 starts a 16-byte row and a scalar closes it -- two dwordx4 stores"""
    st = _ffi.BsdfResult
    assert (st.f.offset, st.pdf.offset, st.wi.offset, st.event.offset) == (0, 12, 16, 28) and C.sizeof(st) == 32


def test_mode_and_event_values():
    assert (_ffi.BSDF_EVALUATE, _ffi.BSDF_SAMPLE) == (0, 1)
    # Surface::event_reflect / _enter / _exit / _through (the reference's src/base/surface.h:46-50)
    assert (_ffi.BSDF_EVENT_REFLECT, _ffi.BSDF_EVENT_ENTER, _ffi.BSDF_EVENT_EXIT, _ffi.BSDF_EVENT_THROUGH) == (0, 1, 2, 4)


def test_library_exports_the_entry_points():
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))  # loads without a GPU; nothing is called
    for name in ("lrhip_query_bsdf", "lrhip_last_bsdf_ms"):
        assert hasattr(lib, name), name
    assert all(hasattr(MegaPathRenderer, name) for name in ("bsdf_evaluate", "bsdf_sample", "last_bsdf_ms"))


def test_null_arguments_are_invalid_without_a_device():
    lib = _ffi.hip_lib()
    p = _ffi.BsdfQueryParams()
    assert lib.lrhip_query_bsdf(None, C.byref(p)) == LRHIP_ERROR_INVALID
    assert b"lrhip_query_bsdf" in lib.lrhip_last_error()
    assert lib.lrhip_query_bsdf(None, None) == LRHIP_ERROR_INVALID
    assert lib.lrhip_last_bsdf_ms(None) == 0.0


def test_argument_checks():
    hits, rays = np.zeros((5, 8), np.float32), np.zeros((5, 8), np.float32)
    wi3, wi4 = np.zeros((5, 3), np.float32), np.zeros((5, 4), np.float32)
    assert check_bsdf_args(hits, wi3) == "numpy"
    assert check_bsdf_args(hits, wi4, rays) == "numpy"
    assert check_bsdf_args(RayHits(hits), wi4, rays) == "numpy"
    assert check_bsdf_args(hits, np.zeros((5, 6), np.float32)[:, :3]) == "numpy"  # an [N, 3] array is copied: any strides
    assert check_bsdf_args(np.zeros((0, 8), np.float32), np.zeros((0, 4), np.float32)) == "numpy"
    bad = [
        dict(hits=np.zeros((5, 7), np.float32), dirs=wi3),           # hits: check_surface_args is reused
        dict(hits=np.zeros((5, 8), np.float64), dirs=wi3),
        dict(hits=np.zeros((10, 8), np.float32)[::2], dirs=wi3),
        dict(hits=hits, dirs=np.zeros((5, 2), np.float32)),          # shape
        dict(hits=hits, dirs=np.zeros((5, 5), np.float32)),
        dict(hits=hits, dirs=np.zeros(3, np.float32)),
        dict(hits=hits, dirs=np.zeros((5, 3), np.float64)),          # dtype
        dict(hits=hits, dirs=np.zeros((5, 4), np.uint32)),
        dict(hits=hits, dirs=np.zeros((5, 8), np.float32)[:, :4]),   # an [N, 4] array is read in place: contiguous
        dict(hits=hits, dirs=np.zeros((4, 3), np.float32)),          # counts differ
        dict(hits=hits, dirs=np.zeros((6, 4), np.float32)),
        dict(hits=hits, dirs=wi3, rays=np.zeros((4, 8), np.float32)),
        dict(hits=hits, dirs=wi3, rays=np.zeros((5, 7), np.float32)),
        dict(hits=hits, dirs=wi3, rays=np.zeros((5, 8), np.float64)),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError, match="bsdf"):
            check_bsdf_args(**kwargs)
    for kwargs in (dict(hits=None, dirs=wi3), dict(hits=hits, dirs=None), dict(hits=[[0.0] * 8] * 5, dirs=wi3), dict(hits=hits, dirs=[[0.0] * 3] * 5),
                   dict(hits=hits, dirs=wi3, rays=[[0.0] * 8] * 5)):
        with pytest.raises(TypeError, match="bsdf"):
            check_bsdf_args(**kwargs)
    with pytest.raises(ValueError, match="bsdf: u must have shape"):
        check_bsdf_args(hits, np.zeros((5, 2), np.float32), what="u")


def test_bsdf_results_are_views_of_one_buffer():
    buffer = np.arange(3 * 8, dtype=np.float32).reshape(3, 8)
    buffer.view(np.uint32)[:, 7] = (0, 0xFFFFFFFF, 4)
    r = BsdfResults(buffer)
    assert len(r) == 3 and r.buffer is buffer
    for name, first, width in (("f", 0, 3), ("wi", 4, 3)):
        a = getattr(r, name)
        assert a.shape == (3, width) and np.shares_memory(a, buffer) and np.array_equal(a, buffer[:, first:first + width]), name
    assert np.array_equal(r.pdf, buffer[:, 3]) and np.shares_memory(r.pdf, buffer)
    assert r.event.dtype == np.uint32 and r.event.tolist() == [0, 0xFFFFFFFF, 4] and np.shares_memory(r.event, buffer)
    assert r.valid.tolist() == [True, False, True]
