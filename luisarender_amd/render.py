"""Thin Python driver over the device C ABI (include/lrhip.h).  No torch types cross the ABI;
torch is only used by callers that want the film in a tensor (bench.py, multi-GPU reduce)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _ffi
from .scene import AOV_COMPONENTS, Scene, aov_channels


class DeviceError(RuntimeError):
    pass


def tile_count(width: int, height: int) -> int:
    return ((width + 7) // 8) * ((height + 7) // 8)


def aov_dump_counts(noisy_count: int, dump: str) -> list[int]:
    """The AOV integrator's should_dump (aov.cpp:383-392): the sample counts after which its buffers are written -- powers of two
    (so none at noisy_count 10 itself), every count, or noisy_count alone"""
    if dump == "all":
        return list(range(1, noisy_count + 1))
    if dump == "final":
        return [noisy_count]
    return [n for n in range(1, noisy_count + 1) if n & (n - 1) == 0]


def aov_file_name(camera_file: str, component: str, n: int, dump: str) -> str:
    """aov.cpp:418-421: <parent>/<stem>_<component>_<n:05><ext>, or <parent>/<stem>_<component><ext> for the final dump"""
    parent, name = os.path.split(camera_file)
    stem, ext = os.path.splitext(name)
    return os.path.join(parent, f"{stem}_{component}{'' if dump == 'final' else f'_{n:05d}'}{ext}")


def check_rays(rays, device: int | None = None, prefix: str = "trace") -> str:
    """What MegaPathRenderer.trace accepts (no device needed): a C-contiguous float32 numpy array [N, 8] laid out (ox, oy, oz, t_min,
    dx, dy, dz, t_max) -> "numpy", or a contiguous float32 torch tensor of that shape on GPU `device` (None: any GPU) -> "torch".
    ValueError for anything else; `prefix` names the caller in its message."""
    if isinstance(rays, np.ndarray):
        kind = "numpy"
        contiguous = rays.flags["C_CONTIGUOUS"]
        is_float32 = rays.dtype == np.float32
    elif type(rays).__module__.split(".")[0] == "torch" and hasattr(rays, "data_ptr"):
        import torch
        kind = "torch"
        contiguous = rays.is_contiguous()
        is_float32 = rays.dtype == torch.float32
        if rays.device.type != "cuda":
            raise ValueError(f"{prefix}: the ray tensor is on {rays.device}, not on a GPU")
        if device is not None and rays.device.index != device:
            raise ValueError(f"{prefix}: the ray tensor is on {rays.device}, the renderer on GPU {device}")
    else:
        raise ValueError(f"{prefix}: rays must be a numpy array or a torch tensor, not {type(rays).__name__}")
    if not is_float32:
        raise ValueError(f"{prefix}: rays must be float32, not {rays.dtype}")
    if rays.ndim != 2 or rays.shape[1] != 8:
        raise ValueError(f"{prefix}: rays must have shape [N, 8] (ox, oy, oz, t_min, dx, dy, dz, t_max), not {tuple(rays.shape)}")
    if not contiguous:
        raise ValueError(f"{prefix}: rays must be contiguous")
    return kind


def check_radiance_args(rays, spp: int = 1, spp_begin: int = 0, streams=None, clamp=None, accumulate_into=None, device: int | None = None) -> str:
    """What MegaPathRenderer.radiance accepts besides check_rays' rays (no device needed): spp, spp_begin >= 0 with spp_begin + spp < 2^32;
    streams None or uint32 (torch: int32, read as uint32) of shape [N]; clamp None or a positive finite number; accumulate_into None or a float32
    raw result [N, 4].  streams and accumulate_into are of the same kind as rays (numpy / torch on the same GPU) and contiguous.  Returns
    check_rays' answer; ValueError for anything else."""
    kind = check_rays(rays, device)
    n = int(rays.shape[0])
    if isinstance(spp, bool) or isinstance(spp_begin, bool) or not isinstance(spp, (int, np.integer)) or not isinstance(spp_begin, (int, np.integer)):
        raise ValueError("radiance: spp and spp_begin must be integers")
    if spp < 0 or spp_begin < 0 or spp_begin + spp > 0xFFFFFFFF:
        raise ValueError(f"radiance: samples [{spp_begin}, {spp_begin} + {spp}) are not a range of 32-bit sample indices")
    if clamp is not None and not (0.0 < float(clamp) < float("inf")):
        raise ValueError(f"radiance: clamp must be a positive finite number or None (the scene's film clamp), not {clamp}")

    def check(name, a, shape, dtype_name):
        if kind == "numpy":
            ok_kind = isinstance(a, np.ndarray)
        else:
            ok_kind = type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")
        if not ok_kind:
            raise ValueError(f"radiance: {name} must be a {kind} array like rays, not {type(a).__name__}")
        if kind == "torch" and a.device != rays.device:
            raise ValueError(f"radiance: {name} is on {a.device}, rays on {rays.device}")
        if str(a.dtype).split(".")[-1] != dtype_name:
            raise ValueError(f"radiance: {name} must be {dtype_name}, not {a.dtype}")
        if tuple(a.shape) != shape:
            raise ValueError(f"radiance: {name} must have shape {list(shape)}, not {tuple(a.shape)}")
        if not (a.flags["C_CONTIGUOUS"] if kind == "numpy" else a.is_contiguous()):
            raise ValueError(f"radiance: {name} must be contiguous")

    if streams is not None:
        check("streams", streams, (n,), "uint32" if kind == "numpy" else "int32")
    if accumulate_into is not None:
        check("accumulate_into", accumulate_into, (n, 4), "float32")
    return kind


def check_surface_args(hits=None, rays=None, device: int | None = None, prefix: str | None = None) -> str:
    """What MegaPathRenderer.surface accepts (no device needed).  hits: a RayHits, or a float32 [N, 8] array of lrhip_ray_hit records
    (t, u, v, inst, prim, tri, 0, 0 -- the ids as the bits of uint32), or None: then rays are traced first.  rays: what check_rays accepts,
    or None: every point is seen from its front.  Both are of one kind (numpy, or torch on one GPU), contiguous, and have the same N.
    Returns check_rays' answer; ValueError for anything else.  `prefix` names the caller in every message (None: "surface", and "trace" where
    check_rays speaks about the rays)."""
    own, of_rays = prefix or "surface", prefix or "trace"
    if hits is None and rays is None:
        raise ValueError(f"{own}: neither hits nor rays")
    kind = None
    if rays is not None:
        kind = check_rays(rays, device, of_rays)
    if hits is not None:
        buffer = hits.buffer if isinstance(hits, RayHits) else hits
        try:
            hits_kind = check_rays(buffer, device, of_rays)
        except ValueError as e:
            raise ValueError(str(e).replace(f"{of_rays}: rays", f"{own}: hits").replace(f"{of_rays}: the ray tensor", f"{own}: the hit tensor")
                             .replace("(ox, oy, oz, t_min, dx, dy, dz, t_max)", "(t, u, v, inst, prim, tri, 0, 0)")) from None
        if kind is not None and hits_kind != kind:
            raise ValueError(f"{own}: hits are a {hits_kind} array, rays a {kind} array")
        if kind is not None and int(buffer.shape[0]) != int(rays.shape[0]):
            raise ValueError(f"{own}: {int(buffer.shape[0])} hits for {int(rays.shape[0])} rays")
        if kind == "torch" and buffer.device != rays.device:
            raise ValueError(f"{own}: hits are on {buffer.device}, rays on {rays.device}")
        kind = hits_kind
    return kind


def check_bsdf_args(hits, dirs, rays=None, device: int | None = None, what: str = "wi") -> str:
    """What MegaPathRenderer.bsdf_evaluate / bsdf_sample accept (no device needed).  hits: a RayHits, or a float32 [N, 8] array of lrhip_ray_hit
    records, as check_surface_args takes them.  dirs (`what` names it in messages): float32 [N, 3] or [N, 4] -- wi, or (u_lobe, u_x, u_y); an
    [N, 4] array must be contiguous (it is read in place), an [N, 3] one is padded by a copy.  rays: what check_rays accepts, or None.  All are
    of one kind (numpy, or torch on one GPU) and have the same N.  Returns check_rays' answer; TypeError for an argument that is no array or
    tensor at all, ValueError for anything else."""
    for name, a in (("hits", hits.buffer if isinstance(hits, RayHits) else hits), (what, dirs)):
        if not isinstance(a, np.ndarray) and not (type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")):
            raise TypeError(f"bsdf: {name} must be a numpy array or a torch tensor, not {type(a).__name__}")
    if rays is not None and not isinstance(rays, np.ndarray) and not (type(rays).__module__.split(".")[0] == "torch" and hasattr(rays, "data_ptr")):
        raise TypeError(f"bsdf: rays must be a numpy array, a torch tensor or None, not {type(rays).__name__}")
    kind = check_surface_args(hits, rays, device, prefix="bsdf")
    n = len(hits)
    if kind == "numpy":
        if not isinstance(dirs, np.ndarray):
            raise ValueError(f"bsdf: hits are a numpy array, {what} a torch tensor")
        is_float32, contiguous = dirs.dtype == np.float32, dirs.flags["C_CONTIGUOUS"]
    else:
        import torch
        if isinstance(dirs, np.ndarray):
            raise ValueError(f"bsdf: hits are a torch tensor, {what} a numpy array")
        is_float32, contiguous = dirs.dtype == torch.float32, dirs.is_contiguous()
        buffer = hits.buffer if isinstance(hits, RayHits) else hits
        if dirs.device != buffer.device:
            raise ValueError(f"bsdf: hits are on {buffer.device}, {what} on {dirs.device}")
    if not is_float32:
        raise ValueError(f"bsdf: {what} must be float32, not {dirs.dtype}")
    if dirs.ndim != 2 or dirs.shape[1] not in (3, 4):
        raise ValueError(f"bsdf: {what} must have shape [N, 3] or [N, 4], not {tuple(dirs.shape)}")
    if int(dirs.shape[0]) != n:
        raise ValueError(f"bsdf: {n} hits for {int(dirs.shape[0])} rows of {what}")
    if dirs.shape[1] == 4 and not contiguous:
        raise ValueError(f"bsdf: an [N, 4] {what} is read in place and must be contiguous")
    return kind


def check_light_args(hits=None, u=None, points=None, rays=None, device: int | None = None, mode: str = "sample") -> str:
    """What MegaPathRenderer.light_sample (mode "sample") / light_evaluate (mode "evaluate") accept (no device needed).
    sample: exactly one of hits -- a RayHits, or a float32 [N, 8] array of lrhip_ray_hit records, as check_surface_args takes them -- and
    points -- float32 [N, 3] or [N, 4] world-space positions; u: float32 [N, 3] or [N, 4], (u_light_selection, u_surface_x, u_surface_y);
    rays must be None.  An [N, 4] array must be contiguous (it is read in place), an [N, 3] one is padded by a copy.
    evaluate: hits and rays, as check_surface_args takes them; u and points must be None.
    All are of one kind (numpy, or torch on one GPU) and have the same N.  Returns check_rays' answer; TypeError for an argument that is no
    array or tensor at all, ValueError for anything else."""
    def is_array(a):
        return isinstance(a, np.ndarray) or (type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr"))

    if mode not in ("sample", "evaluate"):
        raise ValueError(f"light: unknown mode {mode!r}")
    buffer = hits.buffer if isinstance(hits, RayHits) else hits
    for name, a in (("hits", buffer), ("u", u), ("points", points), ("rays", rays)):
        if a is not None and not is_array(a):
            raise TypeError(f"light: {name} must be a numpy array or a torch tensor, not {type(a).__name__}")
    if mode == "evaluate":
        if u is not None or points is not None:
            raise ValueError("light: light_evaluate takes hits and rays, neither u nor points")
        if hits is None or rays is None:
            raise ValueError("light: light_evaluate needs both the hits and the rays that found them")
        return check_surface_args(hits, rays, device, prefix="light")
    if rays is not None:
        raise ValueError("light: light_sample reads no viewing rays")
    if (hits is None) == (points is None):
        raise ValueError("light: light_sample takes hits or points, one of them")
    if u is None:
        raise ValueError("light: light_sample needs u")

    def check_rows(name, a, like):
        # a float32 [N, 3] or [N, 4] array of `like`'s kind (and device); returns its kind
        if isinstance(a, np.ndarray):
            kind, is_float32, contiguous = "numpy", a.dtype == np.float32, a.flags["C_CONTIGUOUS"]
        else:
            import torch
            kind, is_float32, contiguous = "torch", a.dtype == torch.float32, a.is_contiguous()
            if a.device.type != "cuda":
                raise ValueError(f"light: the {name} tensor is on {a.device}, not on a GPU")
            if device is not None and a.device.index != device:
                raise ValueError(f"light: the {name} tensor is on {a.device}, the renderer on GPU {device}")
        if like is not None:
            like_kind = "numpy" if isinstance(like, np.ndarray) else "torch"
            if kind != like_kind:
                raise ValueError(f"light: {name} is a {kind} array, the records a {like_kind} array")
            if kind == "torch" and a.device != like.device:
                raise ValueError(f"light: {name} is on {a.device}, the records on {like.device}")
        if not is_float32:
            raise ValueError(f"light: {name} must be float32, not {a.dtype}")
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise ValueError(f"light: {name} must have shape [N, 3] or [N, 4], not {tuple(a.shape)}")
        if a.shape[1] == 4 and not contiguous:
            raise ValueError(f"light: an [N, 4] {name} is read in place and must be contiguous")
        return kind

    if points is not None:
        kind = check_rows("points", points, None)
        records = points
    else:
        kind = check_surface_args(hits, None, device, prefix="light")
        records = buffer
    check_rows("u", u, records)
    if int(u.shape[0]) != int(records.shape[0]):
        raise ValueError(f"light: {int(records.shape[0])} records for {int(u.shape[0])} rows of u")
    return kind


def parse_sampler_pattern(pattern: str) -> tuple[list[int], int]:
    """A draw pattern for MegaPathRenderer.sampler_draw: a string over "1" (LRHIP_DRAW_1D), "2" (LRHIP_DRAW_2D) and "p" (LRHIP_DRAW_PIXEL_2D),
    at most 64 draws.  Returns (the codes, the number of floats per record: 1 per "1", 2 per other, at most 128).  ValueError for anything else."""
    if not isinstance(pattern, str):
        raise ValueError(f"sampler: the pattern must be a string over '1', '2', 'p', not {type(pattern).__name__}")
    codes = []
    for c in pattern:
        if c not in "12p":
            raise ValueError(f"sampler: unknown draw {c!r} in the pattern (known: '1', '2', 'p')")
        codes.append({"1": _ffi.DRAW_1D, "2": _ffi.DRAW_2D, "p": _ffi.DRAW_PIXEL_2D}[c])
    if len(codes) > _ffi.SAMPLER_MAX_DRAWS:
        raise ValueError(f"sampler: {len(codes)} draws in one pattern, at most {_ffi.SAMPLER_MAX_DRAWS}")
    floats = sum(1 if c == _ffi.DRAW_1D else 2 for c in codes)
    if floats > 2 * _ffi.SAMPLER_MAX_DRAWS:  # (cannot happen with 64 draws of at most 2 floats: kept as the stated bound of `out`)
        raise ValueError(f"sampler: {floats} floats per record, at most {2 * _ffi.SAMPLER_MAX_DRAWS}")
    return codes, floats


def _query_array(prefix: str, name: str, a, shapes, dtype_name: str, device: int | None, like=None) -> str:
    # `a` is a contiguous numpy array, or torch tensor on GPU `device`, of one of `shapes` (None = any N) and of dtype `dtype_name` (a uint32
    # array is int32 in torch); of `like`'s kind, device and N where `like` is given.  Returns its kind
    if isinstance(a, np.ndarray):
        kind, contiguous = "numpy", a.flags["C_CONTIGUOUS"]
    elif type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr"):
        kind, contiguous = "torch", a.is_contiguous()
        if a.device.type != "cuda":
            raise ValueError(f"{prefix}: the {name} tensor is on {a.device}, not on a GPU")
        if device is not None and a.device.index != device:
            raise ValueError(f"{prefix}: the {name} tensor is on {a.device}, the renderer on GPU {device}")
    else:
        raise TypeError(f"{prefix}: {name} must be a numpy array or a torch tensor, not {type(a).__name__}")
    want = "int32" if (kind == "torch" and dtype_name == "uint32") else dtype_name
    if str(a.dtype).split(".")[-1] != want:
        raise ValueError(f"{prefix}: {name} must be {want}, not {a.dtype}")
    if not any(a.ndim == len(s) and all(w is None or int(d) == w for d, w in zip(a.shape, s)) for s in shapes):
        raise ValueError(f"{prefix}: {name} must have shape {' or '.join(str(['N' if w is None else w for w in s]) for s in shapes)}, "
                         f"not {tuple(a.shape)}")
    if not contiguous:
        raise ValueError(f"{prefix}: {name} is read in place and must be contiguous")
    if like is not None:
        like_kind = "numpy" if isinstance(like, np.ndarray) else "torch"
        if kind != like_kind:
            raise ValueError(f"{prefix}: {name} is a {kind} array, the other arrays are {like_kind} arrays")
        if kind == "torch" and a.device != like.device:
            raise ValueError(f"{prefix}: {name} is on {a.device}, the other arrays on {like.device}")
        if int(a.shape[0]) != int(like.shape[0]):
            raise ValueError(f"{prefix}: {int(a.shape[0])} rows of {name} for {int(like.shape[0])} records")
    return kind


def check_irradiance_args(hits=None, points=None, normals=None, spp: int = 1, spp_begin: int = 0, streams=None, clamp=None, accumulate_into=None,
                          device: int | None = None) -> str:
    """What MegaPathRenderer.irradiance accepts (no device needed): the records and streams of check_gather_args; spp, spp_begin >= 0 integers
    with spp_begin + spp < 2^32; clamp None or a positive finite number; accumulate_into None or a float32 raw result [N, 4] of the records'
    kind (and device), contiguous.  Returns check_rays' answer; TypeError / ValueError as check_gather_args."""
    kind = check_gather_args(hits, points, normals, 0, streams, device)
    if isinstance(spp, bool) or isinstance(spp_begin, bool) or not isinstance(spp, (int, np.integer)) or not isinstance(spp_begin, (int, np.integer)):
        raise ValueError("gather: spp and spp_begin must be integers")
    if spp < 0 or spp_begin < 0 or spp_begin + spp > 0xFFFFFFFF:
        raise ValueError(f"gather: samples [{spp_begin}, {spp_begin} + {spp}) are not a range of 32-bit sample indices")
    if clamp is not None and not (0.0 < float(clamp) < float("inf")):
        raise ValueError(f"gather: clamp must be a positive finite number or None (the scene's film clamp), not {clamp}")
    if accumulate_into is not None:
        records = points if points is not None else (hits.buffer if isinstance(hits, RayHits) else hits)
        _query_array("gather", "accumulate_into", accumulate_into, ((None, 4),), "float32", device, records)
    return kind


def check_gather_args(hits=None, points=None, normals=None, sample: int = 0, streams=None, device: int | None = None) -> str:
    """What MegaPathRenderer.gather_vertex accepts (no device needed).  Exactly one of hits -- a RayHits (a LightmapTexels is one), or a float32
    [N, 8] array of lrhip_ray_hit records, as check_surface_args takes them -- and points -- float32 [N, 3] or [N, 4] world-space positions,
    together with normals of the same shape rules (any length but 0); normals without points are refused.  An [N, 4] array must be
    contiguous (it is read in place), an [N, 3] one is padded by a copy.  sample: an integer in [0, 2^32); streams: None or uint32 (torch:
    int32, read as uint32) [N], contiguous.  All arrays are of one kind (numpy, or torch on one GPU) and have the same N.  Returns
    check_rays' answer; TypeError for an argument that is no array or tensor at all, ValueError for anything else."""
    def is_array(a):
        return isinstance(a, np.ndarray) or (type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr"))

    buffer = hits.buffer if isinstance(hits, RayHits) else hits
    for name, a in (("hits", buffer), ("points", points), ("normals", normals), ("streams", streams)):
        if a is not None and not is_array(a):
            raise TypeError(f"gather: {name} must be a numpy array or a torch tensor, not {type(a).__name__}")
    if (hits is None) == (points is None):
        raise ValueError("gather: hits or points, one of them")
    if (points is None) != (normals is None):
        raise ValueError("gather: points and normals go together")
    if isinstance(sample, bool) or not isinstance(sample, (int, np.integer)) or not 0 <= int(sample) <= 0xFFFFFFFF:
        raise ValueError(f"gather: sample must be an integer in [0, 2^32), not {sample!r}")
    if points is not None:
        for name, a in (("points", points), ("normals", normals)):
            if a.ndim != 2 or a.shape[1] not in (3, 4):
                raise ValueError(f"gather: {name} must have shape [N, 3] or [N, 4], not {tuple(a.shape)}")
        kinds = []
        for name, a, like in (("points", points, None), ("normals", normals, points)):
            if a.shape[1] == 4:  # read in place
                kinds.append(_query_array("gather", name, a, ((None, 4),), "float32", device, like))
            else:
                kinds.append(_rows_kind("gather", name, a, device, like))
        kind = kinds[0]
        records = points
    else:
        kind = check_surface_args(hits, None, device, prefix="gather")
        records = buffer
    if streams is not None:
        _query_array("gather", "streams", streams, ((None,),), "uint32", device, records)
    return kind


def _rows_kind(prefix: str, name: str, a, device: int | None, like=None) -> str:
    # a float32 [N, 3] array (padded by a copy later: any strides) of `like`'s kind, device and N; returns its kind
    if isinstance(a, np.ndarray):
        kind, is_float32 = "numpy", a.dtype == np.float32
    else:
        import torch
        kind, is_float32 = "torch", a.dtype == torch.float32
        if a.device.type != "cuda":
            raise ValueError(f"{prefix}: the {name} tensor is on {a.device}, not on a GPU")
        if device is not None and a.device.index != device:
            raise ValueError(f"{prefix}: the {name} tensor is on {a.device}, the renderer on GPU {device}")
    if not is_float32:
        raise ValueError(f"{prefix}: {name} must be float32, not {a.dtype}")
    if like is not None:
        like_kind = "numpy" if isinstance(like, np.ndarray) else "torch"
        if kind != like_kind:
            raise ValueError(f"{prefix}: {name} is a {kind} array, the other arrays are {like_kind} arrays")
        if kind == "torch" and a.device != like.device:
            raise ValueError(f"{prefix}: {name} is on {a.device}, the other arrays on {like.device}")
        if int(a.shape[0]) != int(like.shape[0]):
            raise ValueError(f"{prefix}: {int(a.shape[0])} rows of {name} for {int(like.shape[0])} records")
    return kind


def check_sampler_args(state=None, pattern: str = "", streams=None, indices=None, count: int | None = None, sample: int = 0,
                       device: int | None = None) -> str:
    """What MegaPathRenderer.sampler_start (state None) / sampler_draw (state given) accept (no device needed).
    start: streams and indices None or uint32 [N] (torch: int32, read as uint32); count None or the number of records -- required when neither
    array is given, and equal to N otherwise; sample an integer in [0, 2^32).
    draw: state uint32 [N, 4] (torch: int32), as sampler_start returned it; streams, indices and count must be None.
    pattern: what parse_sampler_pattern accepts.  All arrays are of one kind (numpy, or torch on one GPU), contiguous, with the same N.  Returns
    "numpy" or "torch" ("numpy" for a start without arrays); TypeError for an argument that is no array or tensor at all, ValueError otherwise."""
    parse_sampler_pattern(pattern)
    if state is not None:
        if streams is not None or indices is not None or count is not None:
            raise ValueError("sampler: sampler_draw takes a state and a pattern; streams, indices and count belong to sampler_start")
        return _query_array("sampler", "state", state, [(None, 4)], "uint32", device)
    if isinstance(sample, bool) or not isinstance(sample, (int, np.integer)) or not 0 <= sample <= 0xFFFFFFFF:
        raise ValueError(f"sampler: sample must be a 32-bit sample index, not {sample!r}")
    if count is not None and (isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 0 <= count <= 0x7FFFFFFF):
        raise ValueError(f"sampler: count must be an integer in [0, 2^31), not {count!r}")
    kind, first = "numpy", None
    for name, a in (("streams", streams), ("indices", indices)):
        if a is not None:
            kind = _query_array("sampler", name, a, [(None,)], "uint32", device, first)
            first = a if first is None else first
    if first is None and count is None:
        raise ValueError("sampler: sampler_start needs streams, indices or count")
    if first is not None and count is not None and int(first.shape[0]) != count:
        raise ValueError(f"sampler: count is {count}, the arrays have {int(first.shape[0])} rows")
    return kind


def check_camera_args(u, pixels=None, pixel_count: int | None = None, device: int | None = None) -> str:
    """What MegaPathRenderer.camera_rays accepts (no device needed).  u: float32 [N, 4] = (u_filter.x, u_filter.y, u_lens.x, u_lens.y), read in
    place, or [N, 2] = u_filter alone, padded by a copy (for a camera that is no thin lens).  pixels: None (record k is pixel k; then
    N <= pixel_count where that is given) or uint32 [N] pixel ids py * W + px (torch: int32, read as uint32).  Both of one kind (numpy, or torch
    on one GPU) and contiguous.  Returns "numpy" or "torch"; TypeError for an argument that is no array or tensor, ValueError otherwise."""
    kind = _query_array("camera", "u", u, [(None, 4), (None, 2)], "float32", device)
    if pixels is not None:
        _query_array("camera", "pixels", pixels, [(None,)], "uint32", device, u)
    elif pixel_count is not None and int(u.shape[0]) > pixel_count:
        raise ValueError(f"camera: {int(u.shape[0])} records without pixels, the frame has {pixel_count} pixels")
    return kind


def check_splat_args(values, pixels=None, clamp=None, pixel_count: int | None = None, device: int | None = None) -> str:
    """What MegaPathRenderer.film_splat accepts (no device needed).  values: float32 [N, 4] = (r, g, b, ignored), read in place, or [N, 3],
    padded by a copy.  pixels: as for check_camera_args.  clamp: None (the scene's film clamp) or a positive finite number.  Returns "numpy" or
    "torch"; TypeError for an argument that is no array or tensor, ValueError otherwise."""
    kind = _query_array("splat", "values", values, [(None, 4), (None, 3)], "float32", device)
    if pixels is not None:
        _query_array("splat", "pixels", pixels, [(None,)], "uint32", device, values)
    elif pixel_count is not None and int(values.shape[0]) > pixel_count:
        raise ValueError(f"splat: {int(values.shape[0])} records without pixels, the frame has {pixel_count} pixels")
    if clamp is not None and not (0.0 < float(clamp) < float("inf")):
        raise ValueError(f"splat: clamp must be a positive finite number or None (the scene's film clamp), not {clamp}")
    return kind


def check_instance_transforms(matrices, instances=None, instance_count: int | None = None, device: int | None = None) -> str:
    """What MegaPathRenderer.set_instance_transforms and Scene.set_instance_transforms accept (no device needed).  matrices: float32,
    contiguous, [N, 4, 4] or [N, 16] in COLUMN-MAJOR storage -- matrices[i, c, r] (flat: [i, 4 c + r]) is row r of column c, the layout of
    lr_instance.object_to_world; a numpy row-major 4 x 4 matrix M goes in as M.T.  instances: None (matrix i moves instance i; then
    N <= instance_count) or the N instance ids, a one-dimensional integer array.  A numpy array -> "numpy": every element finite, every id
    in [0, instance_count) and listed once (the range checks need instance_count).  A torch tensor on GPU `device` (None: any GPU) ->
    "torch": ids int32 on the same device; values on the device are not looked at (the kernel skips an id out of range).  matrices and
    instances are of the same kind.  ValueError for anything else."""
    what = "set_instance_transforms"
    if isinstance(matrices, np.ndarray):
        kind = "numpy"
        contiguous = matrices.flags["C_CONTIGUOUS"]
        is_float32 = matrices.dtype == np.float32
    elif type(matrices).__module__.split(".")[0] == "torch" and hasattr(matrices, "data_ptr"):
        import torch
        kind = "torch"
        contiguous = matrices.is_contiguous()
        is_float32 = matrices.dtype == torch.float32
        if matrices.device.type != "cuda":
            raise ValueError(f"{what}: the matrix tensor is on {matrices.device}, not on a GPU")
        if device is not None and matrices.device.index != device:
            raise ValueError(f"{what}: the matrix tensor is on {matrices.device}, the renderer on GPU {device}")
    else:
        raise ValueError(f"{what}: matrices must be a numpy array or a torch tensor, not {type(matrices).__name__}")
    if not is_float32:
        raise ValueError(f"{what}: matrices must be float32, not {matrices.dtype}")
    shape = tuple(matrices.shape)
    if not ((len(shape) == 3 and shape[1:] == (4, 4)) or (len(shape) == 2 and shape[1] == 16)):
        raise ValueError(f"{what}: matrices must have shape [N, 4, 4] or [N, 16] (column-major), not {shape}")
    if not contiguous:
        raise ValueError(f"{what}: matrices must be contiguous")
    n = shape[0]
    if kind == "numpy" and not np.isfinite(matrices).all():
        raise ValueError(f"{what}: a matrix has a non-finite element")
    if instances is None:
        if instance_count is not None and n > instance_count:
            raise ValueError(f"{what}: {n} matrices without ids for {instance_count} instances")
        return kind
    if kind == "numpy":
        if not isinstance(instances, np.ndarray) or instances.dtype.kind not in "iu":
            raise ValueError(f"{what}: instances must be an integer numpy array like matrices")
    else:
        import torch
        if not (type(instances).__module__.split(".")[0] == "torch" and hasattr(instances, "data_ptr")) or instances.dtype != torch.int32:
            raise ValueError(f"{what}: instances must be an int32 torch tensor like matrices")
        if instances.device != matrices.device:
            raise ValueError(f"{what}: instances is on {instances.device}, matrices on {matrices.device}")
        if not instances.is_contiguous():
            raise ValueError(f"{what}: instances must be contiguous")
    if tuple(instances.shape) != (n,):
        raise ValueError(f"{what}: instances must have shape [{n}], not {tuple(instances.shape)}")
    if kind == "numpy":
        if n and (int(instances.min()) < 0 or int(instances.max()) > 0xFFFFFFFF or (instance_count is not None and int(instances.max()) >= instance_count)):
            raise ValueError(f"{what}: an instance id is out of range")
        if np.unique(instances).size != n:
            raise ValueError(f"{what}: an instance id is listed twice")
    return kind


def check_mesh_vertices(positions, normals=None, mesh: int = 0, first: int = 0, meshes=None, device: int | None = None) -> str:
    """What MegaPathRenderer.set_mesh_vertices and Scene.set_mesh_vertices accept (no device needed).  positions: float32, contiguous,
    [N, 3], object space; normals: None or an array of the same kind, dtype and shape.  mesh, first: the mesh (an index into
    lr_scene.meshes) and the first vertex within it; meshes: the vertex count of every mesh of the scene (None: no range checks).  numpy
    arrays -> "numpy": every element finite.  torch tensors on GPU `device` (None: any GPU) -> "torch": values on the device are not looked
    at.  ValueError for anything else."""
    what = "set_mesh_vertices"

    def kind_of(array, name):
        if isinstance(array, np.ndarray):
            kind, contiguous, is_float32 = "numpy", array.flags["C_CONTIGUOUS"], array.dtype == np.float32
        elif type(array).__module__.split(".")[0] == "torch" and hasattr(array, "data_ptr"):
            import torch
            kind, contiguous, is_float32 = "torch", array.is_contiguous(), array.dtype == torch.float32
            if array.device.type != "cuda":
                raise ValueError(f"{what}: the {name} tensor is on {array.device}, not on a GPU")
            if device is not None and array.device.index != device:
                raise ValueError(f"{what}: the {name} tensor is on {array.device}, the renderer on GPU {device}")
        else:
            raise ValueError(f"{what}: {name} must be a numpy array or a torch tensor, not {type(array).__name__}")
        if not is_float32:
            raise ValueError(f"{what}: {name} must be float32, not {array.dtype}")
        if len(array.shape) != 2 or array.shape[1] != 3:
            raise ValueError(f"{what}: {name} must have shape [N, 3], not {tuple(array.shape)}")
        if not contiguous:
            raise ValueError(f"{what}: {name} must be contiguous")
        if kind == "numpy" and not np.isfinite(array).all():
            raise ValueError(f"{what}: {name} has a non-finite element")
        return kind

    kind = kind_of(positions, "positions")
    if normals is not None:
        if kind_of(normals, "normals") != kind:
            raise ValueError(f"{what}: positions and normals must both be numpy arrays or both torch tensors")
        if tuple(normals.shape) != tuple(positions.shape):
            raise ValueError(f"{what}: normals must have positions' shape {tuple(positions.shape)}, not {tuple(normals.shape)}")
        if kind == "torch" and normals.device != positions.device:
            raise ValueError(f"{what}: normals is on {normals.device}, positions on {positions.device}")
    for name, value in (("mesh", mesh), ("first", first)):
        if not isinstance(value, (int, np.integer)) or isinstance(value, bool) or not 0 <= int(value) <= 0xFFFFFFFF:
            raise ValueError(f"{what}: {name} must be an integer in [0, 2^32), not {value!r}")
    if meshes is not None:
        if int(mesh) >= len(meshes):
            raise ValueError(f"{what}: mesh {mesh} out of range ({len(meshes)} meshes)")
        if int(first) + int(positions.shape[0]) > int(meshes[int(mesh)]):
            raise ValueError(f"{what}: vertices {first} + {positions.shape[0]} are not inside the mesh's {int(meshes[int(mesh)])}")
    return kind


def check_lightmap_args(instance, width, height, instance_count: int | None = None) -> int:
    """What MegaPathRenderer.lightmap_texels accepts (no device needed): instance, width and height are integers (no bools, no floats) in
    [0, 2^32), instance < instance_count where the caller knows it, and width * height <= 2^31 - 1, the most records one call takes.
    Returns the number of texels; ValueError for anything else."""
    for name, value in (("instance", instance), ("width", width), ("height", height)):
        if not isinstance(value, (int, np.integer)) or isinstance(value, bool) or not 0 <= int(value) <= 0xFFFFFFFF:
            raise ValueError(f"lightmap: {name} must be an integer in [0, 2^32), not {value!r}")
    if instance_count is not None and int(instance) >= int(instance_count):
        raise ValueError(f"lightmap: instance {instance} out of range ({int(instance_count)} instances)")
    if int(width) * int(height) > 0x7FFFFFFF:
        raise ValueError(f"lightmap: {width} x {height} texels are more than the 2^31 - 1 records of one call")
    return int(width) * int(height)


class RayHits:
    """Closest hits of MegaPathRenderer.trace: views (no copies) of ONE [N, 8] 32-bit buffer of lrhip_ray_hit records -- `buffer`, a
    float32 numpy array or, for the torch path, the float32 tensor on the device.  t (+inf: a miss), u, v: float32; inst, prim, tri:
    uint32 (torch: int32, LR_INVALID_ID reads -1); hit = inst != 0xffffffff."""

    def __init__(self, buffer):
        self.buffer = buffer
        if isinstance(buffer, np.ndarray):
            ids = buffer.view(np.uint32)
            invalid = np.uint32(0xFFFFFFFF)
        else:
            import torch
            ids = buffer.view(torch.int32)
            invalid = -1
        self.t, self.u, self.v = buffer[:, 0], buffer[:, 1], buffer[:, 2]
        self.inst, self.prim, self.tri = ids[:, 3], ids[:, 4], ids[:, 5]
        self._invalid = invalid

    @property
    def hit(self):
        return self.inst != self._invalid

    def __len__(self) -> int:
        return int(self.buffer.shape[0])


class LightmapTexels(RayHits):
    """Texel records of MegaPathRenderer.lightmap_texels: RayHits (t = 0, tri = 0xffffffff: a point without a ray) that surface(),
    bsdf_evaluate / bsdf_sample and light_sample take as they stand, record j * width + i for texel (i, j), and `flags`, a view of word 6 of
    the same buffer: _ffi.LIGHTMAP_TEXEL_CENTRE (the centre lies in the owner triangle) or LIGHTMAP_TEXEL_TOUCHED (conservative: only the
    texel's square meets it); 0 with the miss record for a texel nobody owns.  covered = hit; centre, touched: the flag bits as bool."""

    def __init__(self, buffer, width: int, height: int):
        super().__init__(buffer)
        self.width, self.height = int(width), int(height)
        if isinstance(buffer, np.ndarray):
            self.flags = buffer.view(np.uint32)[:, 6]
        else:
            import torch
            self.flags = buffer.view(torch.int32)[:, 6]

    @property
    def covered(self):
        return self.hit

    @property
    def centre(self):
        return (self.flags & _ffi.LIGHTMAP_TEXEL_CENTRE) != 0

    @property
    def touched(self):
        return (self.flags & _ffi.LIGHTMAP_TEXEL_TOUCHED) != 0


class SurfacePoints:
    """Results of MegaPathRenderer.surface: views (no copies) of ONE [N, 32] 32-bit buffer of lrhip_surface_point records -- `buffer`, a
    float32 numpy array or, for the torch path, the float32 tensor on the device.  p, ng, ns, tangent, n_closure, albedo, emission: [N, 3];
    uv, roughness: [N, 2]; area: [N]; inst, prim, surface, light, closure_kind, flags: uint32 (torch: int32, LR_INVALID_ID reads -1);
    valid, back_facing, has_surface, has_light: the flag bits as bool."""

    def __init__(self, buffer):
        self.buffer = buffer
        if isinstance(buffer, np.ndarray):
            ids = buffer.view(np.uint32)
        else:
            import torch
            ids = buffer.view(torch.int32)
        self.p, self.area = buffer[:, 0:3], buffer[:, 3]
        self.ng, self.flags = buffer[:, 4:7], ids[:, 7]
        self.ns, self.inst = buffer[:, 8:11], ids[:, 11]
        self.tangent, self.prim = buffer[:, 12:15], ids[:, 15]
        self.n_closure, self.closure_kind = buffer[:, 16:19], ids[:, 19]
        self.uv, self.roughness = buffer[:, 20:22], buffer[:, 22:24]
        self.albedo, self.surface = buffer[:, 24:27], ids[:, 27]
        self.emission, self.light = buffer[:, 28:31], ids[:, 31]

    @property
    def valid(self):
        return (self.flags & _ffi.SURFACE_VALID) != 0

    @property
    def back_facing(self):
        return (self.flags & _ffi.SURFACE_BACK_FACING) != 0

    @property
    def has_surface(self):
        return (self.flags & _ffi.SURFACE_HAS_SURFACE) != 0

    @property
    def has_light(self):
        return (self.flags & _ffi.SURFACE_HAS_LIGHT) != 0

    def __len__(self) -> int:
        return int(self.buffer.shape[0])


class BsdfResults:
    """Results of MegaPathRenderer.bsdf_evaluate / bsdf_sample: views (no copies) of ONE [N, 8] 32-bit buffer of lrhip_bsdf_result records --
    `buffer`, a float32 numpy array or, for the torch path, the float32 tensor on the device.  f (the closure's value times |cos theta_i|)
    and wi (unit, world space): [N, 3]; pdf: [N]; event: uint32 (torch: int32, LR_INVALID_ID reads -1), _ffi.BSDF_EVENT_*; valid: bool,
    false for the invalid record."""

    def __init__(self, buffer):
        self.buffer = buffer
        if isinstance(buffer, np.ndarray):
            ids = buffer.view(np.uint32)
        else:
            import torch
            ids = buffer.view(torch.int32)
        self.f, self.pdf = buffer[:, 0:3], buffer[:, 3]
        self.wi, self.event = buffer[:, 4:7], ids[:, 7]

    @property
    def valid(self):
        return self.event != (0xFFFFFFFF if isinstance(self.buffer, np.ndarray) else -1)

    def __len__(self) -> int:
        return int(self.buffer.shape[0])


class LightResults:
    """Results of MegaPathRenderer.light_evaluate: views (no copies) of ONE [N, 8] 32-bit buffer of lrhip_light_result records -- `buffer`, a
    float32 numpy array or, for the torch path, the float32 tensor on the device.  L: [N, 3]; pdf: [N], the solid-angle density times the
    selection probability; kind: uint32 (torch: int32, LR_INVALID_ID reads -1), _ffi.LIGHT_KIND_*; valid: bool, false for the invalid record."""

    def __init__(self, buffer):
        self.buffer = buffer
        if isinstance(buffer, np.ndarray):
            ids = buffer.view(np.uint32)
        else:
            import torch
            ids = buffer.view(torch.int32)
        self.L, self.pdf, self.kind = buffer[:, 0:3], buffer[:, 3], ids[:, 4]

    @property
    def valid(self):
        return self.kind != (0xFFFFFFFF if isinstance(self.buffer, np.ndarray) else -1)

    def __len__(self) -> int:
        return int(self.buffer.shape[0])


class LightSamples(LightResults):
    """Results of MegaPathRenderer.light_sample: LightResults, and `rays`, the [N, 8] float32 buffer of shadow rays (ox, oy, oz, 0, dx, dy,
    dz, t_max) that trace(rays, any_hit=True) takes as it stands.  pdf = 0 marks a failed sample, whose ray may be non-finite."""

    def __init__(self, rays, buffer):
        super().__init__(buffer)
        self.rays = rays


class GatherVertices:
    """Results of MegaPathRenderer.gather_vertex: views (no copies) of ONE [N, 24] float32 buffer of lrhip_gather_vertex records -- `buffer`, a
    numpy array or, for the torch path, the tensor on the device.  rays, shadow: [N, 8] (ox, oy, oz, t_min, dx, dy, dz, t_max), strided views
    (trace() wants np.ascontiguousarray / .contiguous() of them); nee, beta: [N, 3]; light_pdf, pdf: [N]; valid: bool, false for the invalid
    record (pdf = 0 and a zero direction)."""

    def __init__(self, buffer):
        self.buffer = buffer
        self.rays, self.shadow = buffer[:, 0:8], buffer[:, 8:16]
        self.nee, self.light_pdf = buffer[:, 16:19], buffer[:, 19]
        self.beta, self.pdf = buffer[:, 20:23], buffer[:, 23]

    @property
    def valid(self):
        return (self.rays[:, 4:7] != 0).any(1) if isinstance(self.buffer, np.ndarray) else (self.rays[:, 4:7] != 0).any(dim=1)

    def __len__(self) -> int:
        return int(self.buffer.shape[0])


class CameraRays:
    """Results of MegaPathRenderer.camera_rays: `rays`, the [N, 8] float32 buffer of camera rays (ox, oy, oz, t_min, dx, dy, dz, t_max) that
    trace(rays) takes as it stands, and views (no copies) of ONE [N, 4] 32-bit buffer of lrhip_camera_sample records -- `buffer`, a float32
    numpy array or, for the torch path, the float32 tensor on the device.  weight: [N], the filter's f / pdf; film_xy: [N, 2], the continuous
    film position; pixel: uint32 (torch: int32, LR_INVALID_ID reads -1); valid: bool, false for the invalid record."""

    def __init__(self, rays, buffer):
        self.rays, self.buffer = rays, buffer
        if isinstance(buffer, np.ndarray):
            ids = buffer.view(np.uint32)
        else:
            import torch
            ids = buffer.view(torch.int32)
        self.weight, self.film_xy, self.pixel = buffer[:, 0], buffer[:, 1:3], ids[:, 3]

    @property
    def valid(self):
        return self.pixel != (0xFFFFFFFF if isinstance(self.buffer, np.ndarray) else -1)

    def __len__(self) -> int:
        return int(self.buffer.shape[0])


class _Arrays:
    """The arrays of one library call: numpy (host pointers, the call synchronises) or torch on the renderer's GPU (device pointers)."""

    def __init__(self, kind: str, device: int):
        self.torch = kind == "torch"
        self.device = device
        self.padded = False  # a padding copy was made on torch's stream

    def empty(self, shape, dtype=np.float32):
        if not self.torch:
            return np.empty(shape, dtype)
        import torch
        return torch.empty(shape, dtype=torch.int32 if dtype == np.uint32 else torch.float32, device=torch.device("cuda", self.device))

    def pad(self, a, width: int, value: float = 0.0):
        """[N, w] -> [N, width]: the columns the caller left out hold `value`"""
        missing = width - a.shape[1]
        if missing == 0:
            return a
        if not self.torch:
            return np.concatenate([a, np.full((a.shape[0], missing), value, np.float32)], axis=1)
        import torch
        self.padded = True
        return torch.nn.functional.pad(a, (0, missing), value=value).contiguous()

    def ptr(self, a):
        if a is None:
            return None
        return a.data_ptr() if self.torch else a.ctypes.data


class MegaPathRenderer:
    """One lrhip_ctx on one GPU.  Mirrors the reference's ProgressiveIntegrator::Instance::render
    (src/base/integrator.cpp:34-49): prepare film -> render spp -> download (convert) -> save."""

    def __init__(self, device: int = 0, lib_path: str | None = None):
        self._lib = _ffi.hip_lib(lib_path)  # raises if liblrhip.so is missing: there is no CPU fallback
        self._ctx = C.c_void_p()
        self._device = device
        self._check(self._lib.lrhip_create(device, C.byref(self._ctx)))
        self._scene = None
        self.width = self.height = 0
        self._aov_samples = 0  # samples per pixel rendered since the last upload / clear (download_aov's normalisation)

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise DeviceError(f"lrhip error {rc}: {self._lib.lrhip_last_error().decode()}")

    def _call(self, function, p, a: _Arrays, sync: bool, wait_after: bool = True) -> None:
        # One call over the arrays of `a`.  torch: device pointers; torch's current stream is synchronised before the call if `sync`, or if a
        # padding copy runs on it (the call runs on the context's stream), and the context after it for the same reasons (the copy must outlive
        # the kernel that reads it).  wait_after=False: the call stays asynchronous on the context's stream
        if a.torch:
            import torch
            p.flags |= _ffi.RAY_DEVICE_POINTERS
            if sync or a.padded:
                torch.cuda.current_stream(torch.device("cuda", a.device)).synchronize()
        self._check(function(self._ctx, C.byref(p)))
        if a.torch and wait_after and (sync or a.padded):
            self.synchronize()

    def set_stream(self, hip_stream: int | None) -> None:
        self._check(self._lib.lrhip_set_stream(self._ctx, C.c_void_p(hip_stream or 0)))

    def upload(self, scene: Scene, camera: int = 0, keep_film: bool = False) -> None:
        """keep_film: lrhip_update_scene (the next shutter sample of a frame: film and counters carry on)"""
        view = scene.view(camera)
        self._check((self._lib.lrhip_update_scene if keep_film else self._lib.lrhip_upload_scene)(self._ctx, C.byref(view)))
        self._scene = scene
        self.width, self.height = int(view.camera.width), int(view.camera.height)
        if not keep_film:
            self._aov_samples = 0

    def bind_film(self, device_ptr: int | None) -> None:
        self._check(self._lib.lrhip_bind_film(self._ctx, C.c_void_p(device_ptr or 0)))

    def clear(self) -> None:
        """lrhip_film_clear: the film and, for the AOV integrator, its buffers"""
        self._check(self._lib.lrhip_film_clear(self._ctx))
        self._aov_samples = 0

    def render(self, spp_begin: int, spp_end: int, rank: int = 0, world: int = 1, counters: bool = False,
               sync: bool = False, balance_shards: int = 1, shutter_weight: float | None = None, tile_end: int | None = None) -> None:
        """Render samples [spp_begin, spp_end) of the round-robin tile shard `rank` of `world`.
        `balance_shards` sizes the work items for a frame split into that many shards (lrhip.h): films rendered with
        the same value are bit-identical under any sharding; the multi-GPU bench passes its world size."""
        p = _ffi.RenderParams()
        p.balance_shards = balance_shards
        p.spp_begin, p.spp_end = spp_begin, spp_end
        tiles = tile_count(self.width, self.height)
        tiles = min(tiles, tile_end) if tile_end is not None else tiles  # (tile_end: only the first tiles of the frame, for checks)
        p.tile_begin, p.tile_end, p.tile_stride = min(rank, tiles), tiles, world  # rank >= tiles: an empty shard
        p.flags = 1 if counters else 0
        if shutter_weight is not None:  # Camera::ShutterSample weight of these samples (integrator.cpp:74)
            p.flags |= 2
            p.shutter_weight = shutter_weight
        self._check(self._lib.lrhip_render(self._ctx, C.byref(p)))
        self._aov_samples += spp_end - spp_begin
        if sync:
            self.synchronize()

    def render_frame(self, scene: Scene, camera: int = 0, rank: int = 0, world: int = 1, balance_shards: int = 1) -> None:
        """ProgressiveIntegrator::Instance::_render_one_camera's loop over shutter samples (src/base/integrator.cpp:86-107):
        move the scene to each sample's time, upload it, render the sample's spp range with its weight."""
        samples = scene.shutter_samples(camera)
        begin = 0
        for i, (time, weight, spp) in enumerate(samples):
            moved = scene.set_time(time)
            if i == 0 or moved:
                self.upload(scene, camera, keep_film=i > 0)
            self.render(begin, begin + spp, rank=rank, world=world, balance_shards=balance_shards,
                        shutter_weight=weight if len(samples) > 1 else None)
            begin += spp
            if moved:
                self.synchronize()  # the next set_time rewrites the host tables the upload reads from

    def synchronize(self) -> None:
        self._check(self._lib.lrhip_synchronize(self._ctx))

    def download(self, converted: bool = True) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._lib.lrhip_film_download(self._ctx, out.ctypes.data, 1 if converted else 0))
        return out

    def download_aov(self, name: str, normalized: bool = True) -> np.ndarray:
        """lrhip_aov_download: the AOV integrator's buffer `name` (AOV_COMPONENTS) as [H, W, channels], row 0 at the top.
        normalized: times float(1 / n) for the n samples per pixel rendered since the last upload or clear(), as the reference
        writes its files (AuxiliaryBuffer::save, aov.cpp:184-185); otherwise the raw sums"""
        out = np.empty((self.height, self.width, aov_channels(name)), np.float32)
        self._check(self._lib.lrhip_aov_download(self._ctx, AOV_COMPONENTS.index(name), out.ctypes.data))
        if normalized:
            out *= np.float32(1.0 / max(self._aov_samples, 1))
        return out

    def _denoise_params(self, width: int, height: int, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None,
                        demodulate=None) -> _ffi.DenoiseParams:
        p = _ffi.DenoiseParams()
        self._lib.lrhip_denoise_default_params(C.byref(p))
        p.width, p.height = width, height
        for name, value in (("iterations", iterations), ("sigma_color", sigma_color), ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth)):
            if value is not None:
                setattr(p, name, value)
        if demodulate is not None:
            p.flags = _ffi.DENOISE_DEMODULATE if demodulate else 0
        return p

    def denoise(self, color: np.ndarray, albedo: np.ndarray, normal: np.ndarray, depth: np.ndarray, **params) -> np.ndarray:
        """lrhip_denoise: the edge-avoiding wavelet filter over per-pixel means -- color, albedo, normal [H, W, 3] and depth
        [H, W] or [H, W, 1], as download_aov gives them -- on the device; needs no uploaded scene.  params: iterations (1 .. 8), sigma_color,
        sigma_normal, sigma_depth, demodulate; lrhip.h's defaults otherwise.  Returns [H, W, 3]."""
        color, albedo, normal, depth = (np.ascontiguousarray(a, dtype=np.float32) for a in (color, albedo, normal, depth))
        h, w = color.shape[:2]
        if color.shape != (h, w, 3) or albedo.shape != color.shape or normal.shape != color.shape or depth.size != h * w:
            raise ValueError(f"denoise: shapes {color.shape}, {albedo.shape}, {normal.shape}, {depth.shape}")
        out = np.empty((h, w, 3), np.float32)
        self._check(self._lib.lrhip_denoise(self._ctx, C.byref(self._denoise_params(w, h, **params)), color.ctypes.data, albedo.ctypes.data,
                                            normal.ctypes.data, depth.ctypes.data, out.ctypes.data))
        return out

    def denoise_aov(self, component: str = "sample", **params) -> np.ndarray:
        """lrhip_aov_denoise: the same filter over the buffers on the device -- `component` (sample, diffuse or specular) under the scene's
        albedo, normal and depth, each divided by the samples per pixel rendered since the last upload or clear().  Whole frames only.
        Equals denoise(download_aov(component), download_aov("albedo"), ...) bit for bit."""
        out = np.empty((self.height, self.width, 3), np.float32)
        self._check(self._lib.lrhip_aov_denoise(self._ctx, C.byref(self._denoise_params(0, 0, **params)), AOV_COMPONENTS.index(component),
                                                self._aov_samples, out.ctypes.data))
        return out

    def last_denoise_ms(self) -> float:
        return float(self._lib.lrhip_last_denoise_ms(self._ctx))

    def trace(self, rays, any_hit: bool = False, alpha_test: bool = False, sync: bool = True):
        """lrhip_trace_rays (lrhip.h has the semantics): closest hit or occlusion of caller-supplied rays against the uploaded scene.
        rays: what check_rays accepts.  A numpy array goes through host pointers (the call synchronises).  A torch tensor on this
        renderer's GPU is read in place and the result is a tensor on that device, without a copy through the host: torch's current
        stream is synchronised before the call and the context after it; a caller who has bound the context to torch's stream
        (set_stream) may pass sync=False.  Returns RayHits, or with any_hit a bool array / tensor [N] (True: occluded)."""
        a = _Arrays(check_rays(rays, self._device), self._device)
        n = int(rays.shape[0])
        p = _ffi.RayQueryParams()
        p.count = n
        p.mode = _ffi.RAY_ANY if any_hit else _ffi.RAY_CLOSEST
        p.flags = _ffi.RAY_ALPHA_TEST if alpha_test else 0
        out = a.empty(n, np.uint32) if any_hit else a.empty((n, 8))
        p.rays, p.out = a.ptr(rays), a.ptr(out)
        self._call(self._lib.lrhip_trace_rays, p, a, sync)
        return out != 0 if any_hit else RayHits(out)

    def last_trace_ms(self) -> float:
        """lrhip_last_trace_ms: HIP-event time of the kernel(s) of the last trace()"""
        return float(self._lib.lrhip_last_trace_ms(self._ctx))

    def radiance(self, rays, spp: int = 1, spp_begin: int = 0, streams=None, clamp: float | None = None, accumulate_into=None,
                 raw: bool = False, counters: bool = False, sync: bool = True):
        """lrhip_trace_radiance (lrhip.h has the semantics): MegaPath's radiance estimate along caller-supplied rays, samples
        [spp_begin, spp_begin + spp) of each.  rays, streams, accumulate_into: what check_radiance_args accepts; numpy arrays go through host
        pointers, torch tensors on this renderer's GPU are read in place and the result stays on the device (synchronisation as in trace()).
        streams: the sampler stream of each ray (None: 0, 1, 2, ...; stream py * W + px is pixel (px, py)'s).  clamp: per-sample clamp (None:
        the scene's film clamp).  accumulate_into: a previous raw result, refined IN PLACE by these samples and returned.  Returns the [N, 3]
        means sum / max(n, 1), or with raw the [N, 4] sums (sum r, sum g, sum b, n).  counters: the counting kernel (counters())."""
        a = _Arrays(check_radiance_args(rays, spp, spp_begin, streams, clamp, accumulate_into, self._device), self._device)
        n = int(rays.shape[0])
        p = _ffi.RadianceQueryParams()
        p.count = n
        p.spp_begin, p.spp_end = spp_begin, spp_begin + spp
        p.clamp = 0.0 if clamp is None else clamp
        p.flags = (_ffi.RADIANCE_ACCUMULATE if accumulate_into is not None else 0) | (_ffi.RADIANCE_COUNTERS if counters else 0)
        out = accumulate_into if accumulate_into is not None else a.empty((n, 4))
        p.rays, p.out, p.streams = a.ptr(rays), a.ptr(out), a.ptr(streams)
        if a.torch and n != 0 and (p.rays % 16 != 0 or p.out % 16 != 0):
            raise ValueError("radiance: rays and accumulate_into must be 16-byte aligned on the device")
        self._call(self._lib.lrhip_trace_radiance, p, a, sync)
        if raw:
            return out
        if a.torch:
            import torch
            return out[:, :3] / torch.clamp(out[:, 3:4], min=1.0)
        return out[:, :3] / np.maximum(out[:, 3:4], np.float32(1.0))

    def last_radiance_ms(self) -> float:
        """lrhip_last_radiance_ms: HIP-event time of the kernel(s) of the last radiance()"""
        return float(self._lib.lrhip_last_radiance_ms(self._ctx))

    def surface(self, hits=None, rays=None, geometry_only: bool = False, sync: bool = True) -> SurfacePoints:
        """lrhip_query_surface (lrhip.h has the semantics): what is at each hit -- position, normals, uv, the closure's albedo and roughness,
        the light's emission.  hits, rays: what check_surface_args accepts.  hits: a RayHits from trace(), or [N, 8] records the caller made
        (tri = 0xffffffff with inst, prim, u, v names a point without a ray); None: rays are traced first, on the same stream.  rays: the
        viewing rays (emission and back_facing are taken from them), or None: every point is seen from its front.  geometry_only: material and
        emission are skipped (zeros) -- this form serves every scene.  numpy arrays go through host pointers; torch tensors on this renderer's
        GPU are read in place and the result stays on the device (synchronisation as in trace())."""
        a = _Arrays(check_surface_args(hits, rays, self._device), self._device)
        if hits is None:  # (the trace and the query are ordered on the context's stream: no host round trip between them)
            if a.torch and sync:
                import torch
                torch.cuda.current_stream(rays.device).synchronize()
            hits = self.trace(rays, sync=False)
        buffer = hits.buffer if isinstance(hits, RayHits) else hits
        n = int(buffer.shape[0])
        p = _ffi.SurfaceQueryParams()
        p.count = n
        p.flags = _ffi.SURFACE_GEOMETRY_ONLY if geometry_only else 0
        out = a.empty((n, 32))
        p.hits, p.rays, p.out = a.ptr(buffer), a.ptr(rays), a.ptr(out)
        self._call(self._lib.lrhip_query_surface, p, a, sync)
        return SurfacePoints(out)

    def last_surface_ms(self) -> float:
        """lrhip_last_surface_ms: HIP-event time of the kernel(s) of the last surface()"""
        return float(self._lib.lrhip_last_surface_ms(self._ctx))

    def _bsdf(self, mode: int, hits, dirs, rays, sync: bool, what: str) -> BsdfResults:
        a = _Arrays(check_bsdf_args(hits, dirs, rays, self._device, what), self._device)
        buffer = hits.buffer if isinstance(hits, RayHits) else hits
        n = int(buffer.shape[0])
        p = _ffi.BsdfQueryParams()
        p.count, p.mode = n, mode
        dirs, out = a.pad(dirs, 4), a.empty((n, 8))
        p.hits, p.rays, p.dirs, p.out = a.ptr(buffer), a.ptr(rays), a.ptr(dirs), a.ptr(out)
        self._call(self._lib.lrhip_query_bsdf, p, a, sync)
        return BsdfResults(out)

    def bsdf_evaluate(self, hits, wi, rays=None, sync: bool = True) -> BsdfResults:
        """lrhip_query_bsdf, LRHIP_BSDF_EVALUATE (lrhip.h has the semantics): value and pdf of the closure at each hit for the direction wi --
        float32 [N, 3] or [N, 4] (the fourth column is ignored), world space, pointing away from the surface, of any length.  hits: a RayHits
        from trace(), or [N, 8] records the caller made; rays: the viewing rays (wo = -d / |d|), or None: wo = ng.  f includes |cos theta_i|.
        numpy arrays go through host pointers; torch tensors on this renderer's GPU are read in place (an [N, 3] wi is padded by a copy) and
        the result stays on the device (synchronisation as in trace())."""
        return self._bsdf(_ffi.BSDF_EVALUATE, hits, wi, rays, sync, "wi")

    def bsdf_sample(self, hits, u, rays=None, sync: bool = True) -> BsdfResults:
        """lrhip_query_bsdf, LRHIP_BSDF_SAMPLE: a direction sampled from the closure at each hit with its value, pdf and event, from the three
        random numbers u = (u_lobe, u_x, u_y) per record -- float32 [N, 3] or [N, 4].  The caller supplies them: no sampler is touched and the
        result is a pure function of the arguments.  pdf = 0 marks a failed sample, whose f and wi may be non-finite: test pdf > 0 first.
        Otherwise as bsdf_evaluate."""
        return self._bsdf(_ffi.BSDF_SAMPLE, hits, u, rays, sync, "u")

    def last_bsdf_ms(self) -> float:
        """lrhip_last_bsdf_ms: HIP-event time of the kernel(s) of the last bsdf_evaluate() / bsdf_sample()"""
        return float(self._lib.lrhip_last_bsdf_ms(self._ctx))

    def light_sample(self, hits=None, u=None, points=None, sync: bool = True) -> LightSamples:
        """lrhip_query_light, LRHIP_LIGHT_SAMPLE (lrhip.h has the semantics): one light or the environment sampled from each hit -- a RayHits
        from trace(), or [N, 8] records the caller made -- or, with points instead of hits, from bare world-space positions [N, 3] or [N, 4]
        (LRHIP_LIGHT_FROM_POINTS: no offset off a surface), with the three random numbers u = (u_light_selection, u_surface_x, u_surface_y) per
        record, float32 [N, 3] or [N, 4].  Returns LightSamples: the shadow rays, ready for trace(rays, any_hit=True), L, and pdf, which
        includes the selection probability; pdf = 0 marks a failed sample.  numpy arrays go through host pointers; torch tensors on this
        renderer's GPU are read in place (an [N, 3] array is padded by a copy) and the results stay on the device (synchronisation as in
        trace())."""
        a = _Arrays(check_light_args(hits, u, points, None, self._device, "sample"), self._device)
        records = a.pad(points, 4) if points is not None else (hits.buffer if isinstance(hits, RayHits) else hits)
        n = int(records.shape[0])
        p = _ffi.LightQueryParams()
        p.count, p.mode = n, _ffi.LIGHT_SAMPLE
        p.flags = _ffi.LIGHT_FROM_POINTS if points is not None else 0
        u, rays, out = a.pad(u, 4), a.empty((n, 8)), a.empty((n, 8))
        p.hits, p.dirs, p.out_rays, p.out = a.ptr(records), a.ptr(u), a.ptr(rays), a.ptr(out)
        self._call(self._lib.lrhip_query_light, p, a, sync)
        return LightSamples(rays, out)

    def light_evaluate(self, hits, rays, sync: bool = True) -> LightResults:
        """lrhip_query_light, LRHIP_LIGHT_EVALUATE: what each ray found at its end -- hits are the records trace(rays) wrote.  A hit on an
        emitter gives its L towards the ray's origin and the pdf light_sample would have had for that point (kind _ffi.LIGHT_KIND_AREA), a miss
        the environment's (LIGHT_KIND_ENVIRONMENT), anything else L = 0, pdf = 0 (LIGHT_KIND_NONE): what a path tracer weighs a BSDF-sampled
        ray's emission with.  Otherwise as light_sample."""
        a = _Arrays(check_light_args(hits, None, None, rays, self._device, "evaluate"), self._device)
        buffer = hits.buffer if isinstance(hits, RayHits) else hits
        n = int(buffer.shape[0])
        p = _ffi.LightQueryParams()
        p.count, p.mode = n, _ffi.LIGHT_EVALUATE
        out = a.empty((n, 8))
        p.hits, p.rays, p.out = a.ptr(buffer), a.ptr(rays), a.ptr(out)
        self._call(self._lib.lrhip_query_light, p, a, sync)
        return LightResults(out)

    def last_light_ms(self) -> float:
        """lrhip_last_light_ms: HIP-event time of the kernel(s) of the last light_sample() / light_evaluate()"""
        return float(self._lib.lrhip_last_light_ms(self._ctx))

    def _sampler(self, kind: str, state, pattern: str, streams, indices, sample: int, start: bool, sync: bool):
        # one lrhip_query_sampler call over `state` ([N, 4], written in place); returns the drawn numbers [N, D]
        codes, floats = parse_sampler_pattern(pattern)
        n = int(state.shape[0])
        p = _ffi.SamplerQueryParams()
        p.count, p.pattern_count, p.sample_index = n, len(codes), sample
        p.flags = _ffi.SAMPLER_START if start else 0
        table = (C.c_uint32 * max(len(codes), 1))(*codes)
        p.pattern = C.cast(table, C.c_void_p)
        a = _Arrays(kind, self._device)
        out = a.empty((n, floats))
        p.state, p.out = a.ptr(state), a.ptr(out) if floats else None
        p.streams, p.indices = a.ptr(streams), a.ptr(indices)
        if a.torch and n != 0 and (p.state % 16 != 0 or (floats and p.out % 16 != 0)):
            raise ValueError("sampler: the state must be 16-byte aligned on the device")
        self._call(self._lib.lrhip_query_sampler, p, a, sync)
        return out

    def sampler_start(self, streams=None, sample: int = 0, count: int | None = None, indices=None, on_device: bool = False, sync: bool = True):
        """lrhip_query_sampler with LRHIP_SAMPLER_START and an empty pattern (lrhip.h has the semantics): the states of the scene's sampler
        streams as Li starts them -- stream streams[k] (None: k; stream py * W + px is pixel (px, py)'s, as in radiance()) at sample index
        indices[k] (None: `sample`).  streams, indices, count: what check_sampler_args accepts.  Returns the [N, 4] state, uint32 numpy or,
        for tensors on this renderer's GPU (or on_device=True where no array says so), int32 torch on the device.  The state is opaque and
        valid for this upload only; sampler_draw advances it."""
        kind = check_sampler_args(None, "", streams, indices, count, sample, self._device)
        first = streams if streams is not None else indices
        n = int(first.shape[0]) if first is not None else int(count)
        if kind == "numpy" and not (on_device and first is None):
            state = np.empty((n, 4), np.uint32)
        else:
            import torch
            kind = "torch"
            state = torch.empty((n, 4), dtype=torch.int32, device=first.device if first is not None else torch.device("cuda", self._device))
        self._sampler(kind, state, "", streams, indices, int(sample), True, sync)
        return state

    def sampler_draw(self, state, pattern: str, sync: bool = True):
        """lrhip_query_sampler: draws `pattern` -- a string over "1" (1-D), "2" (2-D) and "p" (pixel 2-D), at most 64 draws; the three are NOT
        interchangeable (lrhip.h) -- from every stream of `state`, which is advanced IN PLACE.  Returns the numbers, float32 [N, D], of the
        state's kind (numpy, or torch on the device; synchronisation as in trace()).  MegaPath's Li draws "p", "2" iff the camera is a thin
        lens, then per shaded vertex "1212" (light selection, light surface, lobe, BSDF) and from rr_depth on one more "1"."""
        kind = check_sampler_args(state, pattern, device=self._device)
        return self._sampler(kind, state, pattern, None, None, 0, False, sync)

    def camera_rays(self, u, pixels=None, sync: bool = True) -> CameraRays:
        """lrhip_query_camera (lrhip.h has the semantics): the scene's camera ray for each pixel id (None: record k is pixel k) and the numbers
        u = (u_filter.x, u_filter.y, u_lens.x, u_lens.y) -- what sampler_draw gave for "p2" (a camera that is no thin lens: "p" alone, [N, 2]).
        u, pixels: what check_camera_args accepts.  Returns CameraRays: the rays, ready for trace(), the filter weight a path's throughput
        starts as, the film position and the pixel.  numpy arrays go through host pointers; torch tensors on this renderer's GPU are read in
        place and the results stay on the device (synchronisation as in trace())."""
        a = _Arrays(check_camera_args(u, pixels, self.width * self.height, self._device), self._device)
        n = int(u.shape[0])
        if u.shape[1] == 2 and self._scene is not None and int(self._scene.view().camera.kind) == 1:  # LR_CAMERA_THIN_LENS
            raise ValueError("camera: a thin lens needs u = (u_filter, u_lens), [N, 4]")
        p = _ffi.CameraQueryParams()
        p.count = n
        u, rays, out = a.pad(u, 4, 0.5), a.empty((n, 8)), a.empty((n, 4))
        p.u, p.pixels, p.out_rays, p.out = a.ptr(u), a.ptr(pixels), a.ptr(rays), a.ptr(out)
        if a.torch and n != 0 and p.u % 16 != 0:
            raise ValueError("camera: u must be 16-byte aligned on the device")
        self._call(self._lib.lrhip_query_camera, p, a, sync)
        return CameraRays(rays, out)

    def camera_samples(self, sample: int, pixels=None, on_device: bool = False, sync: bool = True):
        """The camera samples of sample index `sample` as lrhip_render takes them: sampler_start for the pixels' streams (None: every pixel of
        the frame, in order), the pixel draw and, for a thin lens, the lens draw, then camera_rays.  Returns (CameraRays, state): the state is
        ready for the first vertex's sampler_draw(state, "1212")."""
        if pixels is None:
            state = self.sampler_start(None, sample, self.width * self.height, on_device=on_device, sync=sync)
        else:
            state = self.sampler_start(pixels, sample, sync=sync)
        thin_lens = int(self._scene.view().camera.kind) == 1  # LR_CAMERA_THIN_LENS
        u = self.sampler_draw(state, "p2" if thin_lens else "p", sync=sync)
        return self.camera_rays(u, pixels, sync=sync), state

    def film_splat(self, values, pixels=None, clamp: float | None = None, sync: bool = True) -> None:
        """lrhip_film_splat (lrhip.h has the semantics): one sample per record into the film by the reference's accumulate rule -- a NaN or
        infinite value is rejected, a value above the clamp (None: the scene's) is scaled down by its largest component, and (r, g, b, 1) is
        added to pixel pixels[k] (None: k) of the film the context accumulates into, in stream order with render() and download().  values,
        pixels: what check_splat_args accepts; the caller has multiplied the camera weight and the shutter weight in.  Distinct pixels in one
        call give a bit-determined film; several records of one pixel are added in no fixed order."""
        a = _Arrays(check_splat_args(values, pixels, clamp, self.width * self.height, self._device), self._device)
        n = int(values.shape[0])
        p = _ffi.FilmSplatParams()
        p.count, p.clamp = n, 0.0 if clamp is None else clamp
        values = a.pad(values, 4)
        p.values, p.pixels = a.ptr(values), a.ptr(pixels)
        if a.torch and n != 0 and p.values % 16 != 0:
            raise ValueError("splat: values must be 16-byte aligned on the device")
        self._call(self._lib.lrhip_film_splat, p, a, sync)

    def last_camera_ms(self) -> float:
        """lrhip_last_camera_ms: HIP-event time of the kernel(s) of the last sampler_start() / sampler_draw() / camera_rays() / film_splat()"""
        return float(self._lib.lrhip_last_camera_ms(self._ctx))

    def set_instance_transforms(self, matrices, instances=None, sync: bool = True) -> None:
        """lrhip_set_instance_transforms (lrhip.h has the semantics): move instances of the uploaded scene on the device -- their records, baked
        triangles and shading records are rewritten and the BVH is refitted and quantised again, in stream order behind earlier renders and
        queries; film, counters and everything else stay.  matrices, instances: what check_instance_transforms accepts -- float32 [N, 4, 4]
        or [N, 16] in COLUMN-MAJOR storage (a numpy row-major matrix M goes in as M.T), and the N instance ids or None for instances
        0 .. N-1.  numpy arrays go through host pointers (checked, the call synchronises).  torch tensors on this renderer's GPU are read in
        place and the call is asynchronous on the context's stream: torch's current stream is synchronised before it; sync=False skips that
        for a caller who has bound the context to torch's stream (set_stream).  The host Scene is not touched: a later upload() of it, with
        or without keep_film, brings the host's tables back; Scene.set_instance_transforms keeps it in step."""
        count = int(self._scene.view().instance_count) if self._scene is not None else None
        a = _Arrays(check_instance_transforms(matrices, instances, count, self._device), self._device)
        p = _ffi.InstanceUpdateParams()
        p.count = int(matrices.shape[0])
        if not a.torch and instances is not None:
            instances = np.ascontiguousarray(instances, dtype=np.uint32)
        p.object_to_world, p.instances = a.ptr(matrices), a.ptr(instances)
        self._call(self._lib.lrhip_set_instance_transforms, p, a, sync, wait_after=False)

    def last_instance_update_ms(self) -> float:
        """lrhip_last_instance_update_ms: HIP-event time of the kernels of the last set_instance_transforms()"""
        return float(self._lib.lrhip_last_instance_update_ms(self._ctx))

    def set_mesh_vertices(self, mesh: int, positions, normals=None, first: int = 0, recompute_normals: bool = False, sync: bool = True) -> None:
        """lrhip_set_mesh_vertices (lrhip.h has the semantics): deform one mesh of the uploaded scene on the device -- vertices first ..
        first + N - 1 of mesh `mesh` (Scene.instance_mesh gives an instance's) get the object-space positions [N, 3] and, if given, the
        normals [N, 3]; the baked triangles and shading records of every instance of the mesh are rewritten and the BVH is refitted and
        quantised again, in stream order behind earlier renders and queries; film, counters and everything else stay.  normals None: kept,
        or with recompute_normals recomputed for the whole mesh from the new positions (area-weighted; the first such call on a mesh
        synchronises).  A mesh with an emissive instance is refused.  float32 numpy arrays go through host pointers (checked, the call
        synchronises).  torch tensors on this renderer's GPU are read in place and the call is asynchronous on the context's stream: torch's
        current stream is synchronised before it; sync=False skips that for a caller who has bound the context to torch's stream
        (set_stream).  The kernels read the tensors' memory when the stream reaches them, not when this method returns: keep the tensors
        referenced and unmodified until the context's stream has passed the call (synchronize(), or any later call that synchronises).  A mesh or
        range outside the uploaded scene is a DeviceError.  The host Scene is not touched: a later upload() of it, with or without
        keep_film, brings the host's tables back; Scene.set_mesh_vertices keeps it in step."""
        if recompute_normals and normals is not None:
            raise ValueError("set_mesh_vertices: normals must be None with recompute_normals")
        a = _Arrays(check_mesh_vertices(positions, normals, mesh, first, None, self._device), self._device)  # mesh and range: the library's to check
        p = _ffi.MeshUpdateParams()
        p.mesh, p.first_vertex, p.count = int(mesh), int(first), int(positions.shape[0])
        p.flags = _ffi.MESH_RECOMPUTE_NORMALS if recompute_normals else 0
        p.positions, p.normals = a.ptr(positions), a.ptr(normals)
        self._call(self._lib.lrhip_set_mesh_vertices, p, a, sync, wait_after=False)

    def last_mesh_update_ms(self) -> float:
        """lrhip_last_mesh_update_ms: HIP-event time of the kernels of the last set_mesh_vertices()"""
        return float(self._lib.lrhip_last_mesh_update_ms(self._ctx))

    def gather_vertex(self, hits=None, points=None, normals=None, sample: int = 0, streams=None, sync: bool = True) -> GatherVertices:
        """lrhip_query_gather_vertex (lrhip.h has the semantics): the plan of ONE irradiance sample at each record -- a path that starts at a
        surface point: MegaPath's shading vertex for a virtual white Lambert surface there, with the throughput started at pi.  hits: a
        RayHits from trace(), the LightmapTexels of lightmap_texels(), or [N, 8] records the caller made; or points with normals, float32
        [N, 3] or [N, 4] (LRHIP_GATHER_FROM_POINTS: rays start at the point itself).  sample: the sample index; streams: the sampler stream
        of each record (None: 0, 1, 2, ...; as in radiance()).  What check_gather_args accepts.  Returns GatherVertices: the irradiance sample
        is (shadow unoccluded ? nee : 0) + beta x what `rays` finds, an emitter or the environment weighted by balance(pdf, its light pdf).
        numpy arrays go through host pointers; torch tensors on this renderer's GPU are read in place (an [N, 3] array is padded by a copy)
        and the result stays on the device (synchronisation as in trace())."""
        a = _Arrays(check_gather_args(hits, points, normals, sample, streams, self._device), self._device)
        records = a.pad(points, 4) if points is not None else (hits.buffer if isinstance(hits, RayHits) else hits)
        n = int(records.shape[0])
        p = _ffi.GatherVertexParams()
        p.count, p.sample_index = n, int(sample)
        p.flags = _ffi.GATHER_FROM_POINTS if points is not None else 0
        out = a.empty((n, 24))
        normals = a.pad(normals, 4) if normals is not None else None
        p.records, p.normals, p.streams, p.out = a.ptr(records), a.ptr(normals), a.ptr(streams), a.ptr(out)
        self._call(self._lib.lrhip_query_gather_vertex, p, a, sync)
        return GatherVertices(out)

    def irradiance(self, hits=None, points=None, normals=None, spp: int = 1, spp_begin: int = 0, streams=None, clamp: float | None = None,
                   accumulate_into=None, raw: bool = False, sync: bool = True):
        """lrhip_gather_irradiance (lrhip.h has the semantics): the irradiance at each record, samples [spp_begin, spp_begin + spp) of MegaPath's
        estimator for paths that start AT the record's point -- next-event estimation at the point itself, then the scene's path tracing to
        its depth -- on the device from end to end.  hits: a RayHits from trace(), the LightmapTexels of lightmap_texels(), or [N, 8] records;
        or points with normals, float32 [N, 3] or [N, 4].  streams: the sampler stream of each record (None: 0, 1, 2, ...; stream py * W + px is
        pixel (px, py)'s, so a map larger than the camera's frame repeats streams: correlated noise, unbiased mean).  clamp: per-sample clamp
        (None: the scene's film clamp).  accumulate_into: a previous raw result, refined IN PLACE and returned.  What check_irradiance_args
        accepts.  Returns the [N, 3] means sum / max(n, 1), or with raw the [N, 4] sums (sum r, sum g, sum b, n); n = 0 marks an invalid
        record.  numpy arrays go through host pointers; torch tensors on this renderer's GPU are read in place and the result stays on the
        device (synchronisation as in trace())."""
        a = _Arrays(check_irradiance_args(hits, points, normals, spp, spp_begin, streams, clamp, accumulate_into, self._device), self._device)
        records = a.pad(points, 4) if points is not None else (hits.buffer if isinstance(hits, RayHits) else hits)
        n = int(records.shape[0])
        p = _ffi.GatherParams()
        p.count = n
        p.spp_begin, p.spp_end = spp_begin, spp_begin + spp
        p.clamp = 0.0 if clamp is None else clamp
        p.flags = (_ffi.GATHER_ACCUMULATE if accumulate_into is not None else 0) | (_ffi.GATHER_FROM_POINTS if points is not None else 0)
        out = accumulate_into if accumulate_into is not None else a.empty((n, 4))
        normals = a.pad(normals, 4) if normals is not None else None
        p.records, p.normals, p.streams, p.out = a.ptr(records), a.ptr(normals), a.ptr(streams), a.ptr(out)
        if a.torch and n != 0 and (p.records % 16 != 0 or p.out % 16 != 0):
            raise ValueError("gather: records and accumulate_into must be 16-byte aligned on the device")
        self._call(self._lib.lrhip_gather_irradiance, p, a, sync)
        if raw:
            return out
        if a.torch:
            import torch
            return out[:, :3] / torch.clamp(out[:, 3:4], min=1.0)
        return out[:, :3] / np.maximum(out[:, 3:4], np.float32(1.0))

    def last_gather_ms(self) -> float:
        """lrhip_last_gather_ms: HIP-event time of the kernel(s) of the last irradiance() / gather_vertex()"""
        return float(self._lib.lrhip_last_gather_ms(self._ctx))

    def lightmap_texels(self, instance: int, width: int, height: int, conservative: bool = False, on_device: bool = False,
                        sync: bool = True) -> LightmapTexels:
        """lrhip_lightmap_texels (lrhip.h has the semantics): the UV rasteriser of a bake -- for each texel of a width x height lightmap over
        the UV chart of instance `instance`, the point of the instance's mesh under the texel's centre ((i + 1/2) / width, (j + 1/2) / height),
        as the record (inst, prim, u, v) without a ray that surface(), bsdf_sample() and light_sample() take.  Centre coverage by edge
        functions, the lowest prim wins where charts overlap; conservative: a texel whose square only touches a triangle gets that triangle's
        nearest point.  Texels nobody owns get the miss record.  instance, width, height: what check_lightmap_args accepts.  Returns
        LightmapTexels over a [height * width, 8] buffer: numpy, or with on_device a float32 tensor on this renderer's GPU, written without a
        copy through the host (synchronisation as in trace()).  A mesh without vertex UVs is a DeviceError."""
        count = self._scene.view().instance_count if self._scene is not None else None
        n = check_lightmap_args(instance, width, height, count)
        a = _Arrays("torch" if on_device else "numpy", self._device)
        out = a.empty((n, 8))
        flags = (_ffi.LIGHTMAP_CONSERVATIVE if conservative else 0) | (_ffi.RAY_DEVICE_POINTERS if a.torch else 0)
        if a.torch and sync:
            import torch
            torch.cuda.current_stream(torch.device("cuda", self._device)).synchronize()
        self._check(self._lib.lrhip_lightmap_texels(self._ctx, int(instance), int(width), int(height), flags, a.ptr(out)))
        if a.torch and sync:
            self.synchronize()
        return LightmapTexels(out, width, height)

    def last_lightmap_ms(self) -> float:
        """lrhip_last_lightmap_ms: HIP-event time of the kernels of the last lightmap_texels()"""
        return float(self._lib.lrhip_last_lightmap_ms(self._ctx))

    def scene_table(self, which: int) -> np.ndarray:
        """tests / tools only (lrhip_read_scene_table): the bytes of one of the device tables that move with the geometry
        (_ffi.TABLE_NODES, TABLE_BVH_TRIANGLES -- with the sentinel behind the last triangle --, TABLE_INSTANCES, TABLE_SHADE_TRIANGLES) or
        of the object-space vertex table (TABLE_VERTICES)
        as a uint8 array [records, bytes per record]"""
        size = int(self._lib.lrhip_scene_table_bytes(self._ctx, which))
        out = np.empty(size, np.uint8)
        self._check(self._lib.lrhip_read_scene_table(self._ctx, which, 0, size, out.ctypes.data))
        return out.reshape(-1, _ffi.TABLE_RECORD_BYTES[which])

    # ---- the one collective of the multi-GPU path, through the C ABI
    def comm_unique_id(self) -> bytes:
        buf = (C.c_ubyte * 128)()
        self._check(self._lib.lrhip_comm_unique_id(buf))
        return bytes(buf)

    def comm_init_rank(self, world: int, rank: int, unique_id: bytes) -> C.c_void_p:
        comm = C.c_void_p()
        self._check(self._lib.lrhip_comm_init_rank(self._ctx, world, rank, (C.c_ubyte * 128).from_buffer_copy(unique_id), C.byref(comm)))
        return comm

    def film_reduce(self, comm, root: int = 0) -> None:
        """sum-reduce of the bound film to `root` over RCCL, in stream order behind the renders (lrhip_film_reduce)"""
        self._check(self._lib.lrhip_film_reduce(self._ctx, comm, root))

    def comm_info(self, comm) -> dict:
        """lrhip_comm_info: what the communicator spans -- ranks, this rank, its device"""
        out = (C.c_int * 3)()
        self._check(self._lib.lrhip_comm_info(comm, out))
        return {"ranks": int(out[0]), "rank": int(out[1]), "device": int(out[2])}

    def comm_destroy(self, comm) -> None:
        self._check(self._lib.lrhip_comm_destroy(comm))

    def counters(self) -> dict:
        c = _ffi.HipCounters()
        self._check(self._lib.lrhip_get_counters(self._ctx, C.byref(c)))
        return c.as_dict()

    def last_render_ms(self) -> float:
        return float(self._lib.lrhip_last_render_ms(self._ctx))

    def last_variant(self) -> int:
        """feature mask of the precompiled megakernel variant the last render() launched (lrhip.h LRHIP_FEAT_*)"""
        return int(self._lib.lrhip_last_variant(self._ctx))

    def set_diagnostics(self, force_features: int = 0, item_scale: float = 0.0) -> None:
        """tests / tools only (lrhip_set_diagnostics): render with a larger precompiled variant than the scene needs, or sweep
        the work-item size; the library itself reads no environment variable"""
        self._check(self._lib.lrhip_set_diagnostics(self._ctx, force_features, item_scale))

    def set_wavefront(self, enabled: bool = True, slice_paths: int = 0, tiny_tile_groups: bool = False, carry_rounds: int = 0) -> None:
        """lrhip_set_wavefront: scenes with Mix / Layered surfaces render in wavefront mode by default (lean megakernel + heavy-closure
        kernel + continuation pass); enabled=False keeps them on the all-in-one megakernel variants (A/B, tests); tiny_tile_groups
        sends seven tiles through the queues at a time (tests: what a GPU short of memory does)"""
        # carry_rounds: rounds before a slice hands its parked paths over to the next one (0 = the library's default, 65535 = never)
        self._check(self._lib.lrhip_set_wavefront(self._ctx, ((2 if tiny_tile_groups else 0) if enabled else 1) | (carry_rounds << 8), slice_paths))

    def set_texture_storage(self, mode: int = 1) -> None:
        """lrhip_set_texture_storage: 8-bit images as 8-bit texels on the device from the next upload on (0 never, 1 automatic: scenes
        whose images exceed 192 MB as floats, 2 every image that qualifies)"""
        self._check(self._lib.lrhip_set_texture_storage(self._ctx, mode))

    def packed_texels(self) -> int:
        """lrhip_packed_texels: how many texels of the uploaded scene the device holds as 8-bit codes"""
        return int(self._lib.lrhip_packed_texels(self._ctx))

    def set_scheduler(self, pool: bool | None = None) -> None:
        """lrhip_set_scheduler: None = automatic (the path-pool kernels of round 4 -- two path contexts per lane, fixed-point film sums,
        overlapping work items -- where they are the faster family (from ~100 thousand BVH triangles; lrhip.h), the one-path-per-lane kernels below), False = one path per
        lane everywhere, True = the pool kernels wherever one exists for the scene"""
        self._check(self._lib.lrhip_set_scheduler(self._ctx, 0 if pool is None else (2 if pool else 1)))

    def close(self) -> None:
        if self._ctx:
            self._lib.lrhip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
