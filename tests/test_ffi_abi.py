"""C ABI surface: struct layouts match between C and the ctypes mirrors, and the shared libraries
export every symbol their header declares (no compute calls: runs without a GPU)."""
import ctypes as C
import os
import re

from luisarender_amd import _ffi
from oracle.check import oracle_lib


def _declared(header, prefix):
    text = open(os.path.join(_ffi.REPO_ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(rf"\b({prefix}_[a-z0-9_]+)\s*\(", text)))


def test_struct_layouts_match():
    lib = _ffi.host_lib()
    for name, st in _ffi.STRUCTS.items():
        assert C.sizeof(st) == lib.lrhost_sizeof(name.encode()), name


def test_host_library_exports_header_symbols():
    lib = _ffi.host_lib()
    names = _declared("lrhost.h", "lrhost")
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), n


def test_hip_library_exports_header_symbols():
    path = os.path.join(_ffi.LIB_DIR, "liblrhip.so")
    assert os.path.exists(path), "liblrhip.so missing: run __graft_entry__.build()"
    lib = C.CDLL(path)  # loads without a GPU; nothing is called
    names = _declared("lrhip.h", "lrhip")
    assert {"lrhip_create", "lrhip_upload_scene", "lrhip_render", "lrhip_film_download", "lrhip_destroy"} <= set(names)
    for n in names:
        assert hasattr(lib, n), n


def test_scene_table_ids_match_the_header():
    """lrhip_read_scene_table's table ids (LRHIP_TABLE_*): every one of the header has its _ffi.TABLE_* twin with the same number and a record size"""
    text = open(os.path.join(_ffi.REPO_ROOT, "include", "lrhip.h")).read()
    ids = {name: int(value) for name, value in re.findall(r"^#define LRHIP_TABLE_([A-Z_]+) (\d+)u$", text, flags=re.M)}
    assert len(ids) == 8 and len(set(ids.values())) == 8
    for name, value in ids.items():
        assert getattr(_ffi, "TABLE_" + name) == value and value in _ffi.TABLE_RECORD_BYTES, name
    assert sorted(_ffi.TABLE_RECORD_BYTES) == sorted(ids.values())
    assert ids["LIGHT_TRIANGLES_EXACT"] == ids["LIGHT_TRIANGLES"] + 1 == 18  # the next free number
    assert _ffi.TABLE_RECORD_BYTES[_ffi.TABLE_LIGHT_TRIANGLES_EXACT] == _ffi.TABLE_RECORD_BYTES[_ffi.TABLE_LIGHT_TRIANGLES] == 80


def test_oracle_exports():
    lib = oracle_lib()
    for n in _declared("../oracle/oracle.h", "oracle"):
        assert hasattr(lib, n), n


def test_plugin_exports_reference_plugin_abi():
    path = os.path.join(_ffi.REPO_ROOT, "luisarender_amd", "bin", "libluisa-render-integrator-megapath.so")
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-C", _ffi.REPO_ROOT, "cli"], stdout=subprocess.DEVNULL)
    _ffi.host_lib()
    lib = C.CDLL(path)
    assert hasattr(lib, "create") and hasattr(lib, "destroy")  # scene_node.h:58-67


def test_work_items_partition_the_sample_range():
    """lrhip_work_items (no device needed): the tapered work items of lrhip_render -- big chunks first, small ones at the end of the
    launch -- must partition [0, spp) exactly, within the 64 partial planes, for every frame size / spp / shard count."""
    import ctypes as C
    lib = C.CDLL(os.path.join(_ffi.REPO_ROOT, "luisarender_amd", "lib", "liblrhip.so"))
    lib.lrhip_work_items.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32 * 4)]
    out = (C.c_uint32 * 4)()
    tapered = 0
    for width, height in ((16, 16), (96, 64), (512, 512), (1024, 1024), (1280, 720), (3840, 2160)):
        for shards in (1, 2, 8, 64):
            for spp in list(range(1, 40)) + [63, 64, 65, 256, 1000, 1024, 4096, 65536]:
                assert lib.lrhip_work_items(width, height, spp, shards, C.byref(out)) == 0
                count, big_count, big, small = out
                assert 1 <= count <= 64 and big_count <= count and big >= 1 and small >= 1, (width, height, spp, shards, list(out))
                covered = 0
                for k in range(count):
                    b = k * big if k < big_count else big_count * big + (k - big_count) * small
                    e = min(b + (big if k < big_count else small), spp)
                    assert min(b, spp) == covered or b >= spp, (width, height, spp, shards, list(out), k)
                    covered = max(covered, e)
                assert covered == spp, (width, height, spp, shards, list(out))
                tapered += big_count < count
    assert tapered > 100  # the taper is what is normally used
    assert lib.lrhip_work_items(0, 16, 1, 1, C.byref(out)) != 0


def test_scheduler_rule_is_a_function_of_the_scene():
    """lrhip_pool_auto_triangles (no device needed): from how many BVH triangles on the automatic scheduler takes the pool kernels -- the
    rule of tools/sched_sweep.py's sweep (profiles/r05j_scheduler_sweep.txt): ~100 thousand triangles, twice that for shallow paths, half of
    it for scenes of few samples per pixel; a function of the SCENE (depth, its own spp), never of a call's sample range."""
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))
    lib.lrhip_pool_auto_triangles.argtypes = [C.c_uint32, C.c_uint32]
    lib.lrhip_pool_auto_triangles.restype = C.c_uint32
    base = lib.lrhip_pool_auto_triangles(16, 1024)
    assert base == 98304
    assert lib.lrhip_pool_auto_triangles(4, 1024) == 2 * base and lib.lrhip_pool_auto_triangles(6, 1024) == 2 * base and lib.lrhip_pool_auto_triangles(7, 1024) == base
    assert lib.lrhip_pool_auto_triangles(16, 16) == base // 2 and lib.lrhip_pool_auto_triangles(16, 64) == base and lib.lrhip_pool_auto_triangles(16, 0) == base
    assert lib.lrhip_pool_auto_triangles(4, 16) == base
    # the sweep's break-even points lie on the right side of it: (triangles, depth, spp) -> pool is the faster family
    for tris, depth, spp, pool_faster in ((30_000, 16, 256, False), (60_000, 16, 16, True), (60_000, 16, 256, False), (100_000, 16, 256, True),
                                          (100_000, 4, 256, False), (400_000, 4, 256, True), (400_000, 16, 16, True), (5_000, 4, 16, False)):
        assert (tris >= lib.lrhip_pool_auto_triangles(depth, spp)) == pool_faster, (tris, depth, spp)


def test_kernel_selection_over_its_input_space():
    """lrhip_plan_kernels (no device needed): the one rule that decides which kernels a call of lrhip_render runs on, over every scene-feature
    set lrhip_upload_scene can produce x counters x sampler x scheduler x packed texels x nested environments x "the fixed-point film
    holds the call" x wavefront mode x depth.  Every kernel of every plan is in the shipped library; the upload's rule for packing 8-bit
    texels agrees with where the packed scenes land; and the cases the project records (GPU tests' last_variant assertions)
    come out with the masks recorded there."""
    import itertools
    lib = C.CDLL(os.path.join(_ffi.LIB_DIR, "liblrhip.so"))
    lib.lrhip_plan_kernels.argtypes = [C.c_uint32] * 6 + [C.POINTER(C.c_uint32 * 8)]
    ENV, ALPHA, DISNEY, MIX, LAYERED, AUX, VPT, NEST, WF, CONT, POOL, BYTE, PADDED, AOV = 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768
    SCENE = ENV | ALPHA | DISNEY | MIX | LAYERED
    NONE, LANE, POOLED, WAVEFRONT, AOV_FAMILY = range(5)
    COUNT, TREE, PACKED, WANTS_POOL, FITS = 1, 2, 4, 8, 16
    INDEPENDENT, SOBOL, PADDED_SOBOL, PCG32 = 0, 1, 2, 3
    NO = 0xFFFFFFFF

    def plan(features, flags=FITS, sampler=INDEPENDENT, wf_mode=0, depth=16, force=0):
        out = (C.c_uint32 * 8)()
        rc = lib.lrhip_plan_kernels(features, force, flags, sampler, wf_mode, depth, C.byref(out))
        return rc, list(out)

    # ---- what the uploader produces: MegaPath scenes keep their own bits (Layered brings the Disney interpreter; nesting needs a Layered
    # surface), the sibling integrators and AOV sit on the all-closures mask, the volumetric kernel is one kernel with everything in it
    closures = [0, DISNEY, MIX, DISNEY | MIX, DISNEY | LAYERED, DISNEY | MIX | LAYERED, DISNEY | LAYERED | NEST, DISNEY | MIX | LAYERED | NEST]
    scenes = [e | a | c for e in (0, ENV) for a in (0, ALPHA) for c in closures] + [SCENE | AUX, SCENE | AOV, VPT]
    rejected = []  # packed texels on kernels that do not decode them: lrhip_upload_scene refuses to pack (mode 2: LRHIP_ERROR_UNSUPPORTED)
    points = 0
    for features in scenes:
        megapath = not features & (AUX | AOV | VPT)
        trees = (False, True) if features & ENV or not megapath else (False,)
        for count, sampler, pool, packed, tree, fits, wf_mode, depth in itertools.product(
                (0, 1), (INDEPENDENT, SOBOL, PADDED_SOBOL, PCG32), (False, True), (False, True), trees, (False, True), (0, 1, 2), (16, 65536)):
            flags = count * COUNT | tree * TREE | packed * PACKED | pool * WANTS_POOL | fits * FITS
            rc, (family, main, cont, h0, h1, h2, fixed, packs) = plan(features, flags, sampler, wf_mode, depth)
            where = (features, flags, sampler, wf_mode, depth, family, main, cont)
            points += 1
            # the upload-time rule, stated here independently: MegaPath scenes with alpha tests, Mix / Layered surfaces or nested environments keep floats
            assert bool(packs) == (not megapath or not (features & (ALPHA | MIX | LAYERED) or tree)), where
            if packed and not packs:
                rejected.append(where)
                continue
            assert rc == 0 and family != NONE, where  # every kernel of the plan is in the shipped library
            generic = sampler != INDEPENDENT
            assert main & 1 == count and bool(main & 2) == generic, where
            assert bool(fixed) == (family in (POOLED, WAVEFRONT)), where
            assert fits or family in (LANE, AOV_FAMILY), where
            assert pool or not main & POOL, where
            # kernels compiled for PaddedSobol: every lean pool set; of the wavefront passes the plain and the alpha-tested ones (variants.h) --
            # the others fall back to the run-time generic sampler's kernel
            assert bool(main & PADDED) == bool(main & POOL and sampler == PADDED_SOBOL and not (main & WF and main & ENV)), where
            assert not (family == WAVEFRONT and wf_mode == 1) and not (family == POOLED and depth >= 65536), where
            if packed:  # ... lands on kernels that decode: the lean ones of the BYTE bit or the call-making variants, never in wavefront mode
                assert family != WAVEFRONT and main & (BYTE | MIX | LAYERED | VPT), where
            else:
                assert not main & BYTE, where
            if family == WAVEFRONT:
                assert megapath and (features & (MIX | LAYERED) or features & (ALPHA | DISNEY) == ALPHA | DISNEY), where
                assert main & ~(1 | 2 | POOL | PADDED) == WF | features & (ENV | ALPHA) and cont == main | CONT, where
                nest = 512 if features & NEST else 0
                assert [h0, h1, h2] == [count | generic << 1, 4 | nest | count | generic << 1, 8 | nest | count | generic << 1], where
            else:
                assert (family == POOLED) == bool(main & POOL) and [cont, h0, h1, h2] == [NO] * 4 and not main & (WF | CONT), where
                if family == AOV_FAMILY:
                    assert features & AOV and main & ~3 == SCENE | AOV, where
                else:
                    need = features & (SCENE | AUX | VPT | NEST)
                    assert main & need == need, where  # a superset of what the scene needs
    assert points > 20000
    # the rejected combinations, explicitly: packed texels with alpha tests, Mix / Layered or nested environments, under MegaPath only
    assert rejected and all(not f & (AUX | AOV | VPT) and (f & (ALPHA | MIX | LAYERED) or fl & TREE) for f, fl, *_ in rejected)
    assert {f for f, *_ in rejected} >= {ALPHA, MIX, DISNEY | LAYERED, ENV}

    # ---- the recorded cases: (features, flags, sampler, wf_mode, depth) -> family, main [, cont, heavy kernels]
    P, K = FITS | WANTS_POOL, ALPHA | DISNEY | MIX  # K: the kitchen class (C5)
    for name, args, want in (
            ("lean (tests/test_gpu_parity.py::test_kernel_variant_selection)", (0,), (LANE, 0)),
            ("lean, Sobol", (0, FITS, SOBOL), (LANE, 2)),
            ("lean, pool: C2 <4096>", (0, P), (POOLED, 4096)),
            ("lean, pool, PCG32", (0, P, PCG32), (POOLED, 4098)),
            ("Disney", (DISNEY,), (LANE, 16)),
            ("alpha-tested traversal on the lean kernel", (ALPHA,), (LANE, 8)),
            ("environment, pool: C3 <4100>", (ENV, P), (POOLED, 4100)),
            ("environment + counters: <5>", (ENV, FITS | COUNT), (LANE, 5)),
            ("environment + Disney", (ENV | DISNEY,), (LANE, 20)),
            ("environment + Disney, pool: C4 before the packed texels <4116>", (ENV | DISNEY, P), (POOLED, 4116)),
            ("C4 class with packed texels <12308>", (ENV | DISNEY, P | PACKED), (POOLED, 12308)),
            ("packed texels, one path per lane <8212>", (ENV | DISNEY, FITS | PACKED), (LANE, 8212)),
            ("Mix: wavefront mode", (MIX,), (WAVEFRONT, WF, WF | CONT, 0, 4, 8)),
            ("Mix, wavefront mode off: <60>", (MIX, FITS, INDEPENDENT, 1), (LANE, 60)),
            ("Layered, wavefront mode off: <124>", (DISNEY | LAYERED, FITS, INDEPENDENT, 1), (LANE, 124)),
            ("nested, wavefront mode off: <636>", (DISNEY | MIX | LAYERED | NEST, FITS, INDEPENDENT, 1), (LANE, 636)),
            ("kitchen class: camera <5128>, continuation <7176>", (K, P), (WAVEFRONT, 5128, 7176, 0, 4, 8)),
            ("kitchen class, counting twins", (K, P | COUNT), (WAVEFRONT, 5129, 7177, 1, 5, 9)),
            ("kitchen class without the pool", (K, FITS), (WAVEFRONT, 1032, 3080, 0, 4, 8)),
            ("kitchen class, nested closures", (K | LAYERED | NEST, P), (WAVEFRONT, 5128, 7176, 0, 516, 520)),
            ("kitchen class under PaddedSobol: <21514> / <23562>", (K, P, PADDED_SOBOL), (WAVEFRONT, 21514, 23562, 2, 6, 10)),
            ("kitchen class deeper than 65535: the lean passes stay pooled", (K, P, INDEPENDENT, 0, 65536), (WAVEFRONT, 5128, 7176, 0, 4, 8)),
            ("Disney + alpha test: wavefront mode, no lean <Alpha | Disney>", (ALPHA | DISNEY,), (WAVEFRONT, WF | ALPHA, WF | CONT | ALPHA, 0, 4, 8)),
            ("PaddedSobol pool: C2 <20482>", (0, P, PADDED_SOBOL), (POOLED, 4096 | 2 | 16384)),
            ("PaddedSobol, one path per lane: the run-time generic sampler", (0, FITS, PADDED_SOBOL), (LANE, 2)),
            ("PaddedSobol, packed camera class <28694>", (ENV | DISNEY, P | PACKED, PADDED_SOBOL), (POOLED, 28694)),
            ("AOV <32892>", (SCENE | AOV, P), (AOV_FAMILY, 32892)),
            ("AOV, counters + generic sampler <32895>", (SCENE | AOV, P | COUNT, SOBOL), (AOV_FAMILY, 32895)),
            ("Direct / Normal <252>", (SCENE | AUX, P), (LANE, 252)),
            ("Direct / Normal <255>", (SCENE | AUX, P | COUNT, PCG32), (LANE, 255)),
            ("VPT <256>", (VPT, P), (LANE, 256)),
            ("VPT <259>", (VPT, P | COUNT, PCG32), (LANE, 259)),
            ("paths deeper than 65535: no pool", (0, P, INDEPENDENT, 0, 65536), (LANE, 0)),
            ("fixed point does not fit: the float-accumulating lean kernel", (0, WANTS_POOL), (LANE, 0)),
            ("fixed point does not fit: the kitchen class on the all-in-one variant", (K, WANTS_POOL), (LANE, 60)),
            ("nested Combined environments: a call-making variant, never wavefront mode", (ENV, P | TREE), (LANE, 60))):
        rc, out = plan(*args)
        assert rc == 0, name
        got = tuple(out[:2]) if len(want) == 2 else tuple(out[:6])
        assert got == want and out[6] == (want[0] in (POOLED, WAVEFRONT)), (name, out)
    # lrhip_set_diagnostics' forced features: a larger variant, and never wavefront mode
    assert plan(0, FITS, force=DISNEY)[1][:2] == [LANE, 16] and plan(0, FITS, force=MIX)[1][:2] == [LANE, 60]
    assert plan(0, P, force=DISNEY)[1][:2] == [POOLED, 4112]
