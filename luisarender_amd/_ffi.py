"""ctypes mirrors of include/lr_scene.h and loaders for the in-tree shared libraries.

Python here is plumbing (tests, bench, graft entry): the product is liblrhost.so (C++ host
side) + liblrhip.so (HIP kernels) behind the C ABIs of include/lrhost.h and include/lrhip.h.
"""
from __future__ import annotations

import ctypes as C
import os

_ROOT = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_ROOT)
LIB_DIR = os.path.join(_ROOT, "lib")

u32, u64, i32, f32 = C.c_uint32, C.c_uint64, C.c_int32, C.c_float


class Vertex(C.Structure):
    _fields_ = [(n, f32) for n in ("px", "py", "pz", "nx", "ny", "nz", "u", "v")]


class Triangle(C.Structure):
    _fields_ = [("i0", u32), ("i1", u32), ("i2", u32)]


class AliasEntry(C.Structure):
    _fields_ = [("prob", f32), ("alias", u32)]


class UInt4(C.Structure):
    _fields_ = [("x", u32), ("y", u32), ("z", u32), ("w", u32)]


class LightHandle(C.Structure):
    _fields_ = [("instance_id", u32), ("light_tag", u32)]


class Mesh(C.Structure):
    _fields_ = [("vertex_offset", u32), ("vertex_count", u32), ("triangle_offset", u32), ("triangle_count", u32)]


class Instance(C.Structure):
    _fields_ = [("handle", UInt4), ("object_to_world", f32 * 16), ("visible", u32), ("pad", u32 * 3)]


class Texture(C.Structure):
    _fields_ = [("kind", u32), ("channels", u32), ("v", f32 * 4), ("width", u32), ("height", u32),
                ("texel_offset", u64), ("address", u32), ("filter", u32), ("encoding", u32),
                ("gamma", f32 * 3), ("uv_scale", f32 * 2), ("uv_offset", f32 * 2), ("scale", f32 * 4),
                ("child", i32 * 2), ("checker_scale", f32), ("pad", u32)]


class Surface(C.Structure):
    _fields_ = [("kind", u32), ("flags", u32), ("tex", i32 * 16), ("f", f32 * 8), ("u", u32 * 4),
                ("alpha_tex", i32), ("normal_tex", i32), ("normal_strength", f32), ("pad", u32)]


class Light(C.Structure):
    _fields_ = [("kind", u32), ("emission_tex", i32), ("scale", f32), ("two_sided", u32)]


class Environment(C.Structure):
    _fields_ = [("kind", u32), ("emission_tex", i32), ("scale", f32), ("compensate_mis", u32),
                ("world_to_env", f32 * 9), ("env_to_world", f32 * 9), ("map_width", u32), ("map_height", u32),
                ("alias", C.c_void_p), ("pdf", C.c_void_p), ("direction", f32 * 3), ("cos_half_angle", f32),
                ("visible", u32), ("child_scale", f32 * 2), ("child", u32 * 2), ("pad", u32)]


class Camera(C.Structure):
    _fields_ = [("kind", u32), ("width", u32), ("height", u32), ("spp", u32), ("camera_to_world", f32 * 16),
                ("tan_half_fov", f32), ("focus_distance", f32), ("lens_radius", f32), ("projected_pixel_size", f32),
                ("ortho_scale", f32), ("clip_near", f32), ("clip_far", f32), ("pad", u32)]


class Filter(C.Structure):
    _fields_ = [("radius", f32), ("shift", f32 * 2), ("pad", f32), ("lut", f32 * 64), ("pdf", f32 * 63),
                ("alias_prob", f32 * 63), ("alias_index", u32 * 63), ("pad2", u32 * 3)]


class Film(C.Structure):
    _fields_ = [("scale", f32 * 3), ("clamp", f32)]


class Sampler(C.Structure):
    _fields_ = [("kind", u32), ("seed", u32), ("spp", u32), ("scale", u32), ("sobol_matrices", C.c_void_p),
                ("vdc_sobol", C.c_void_p), ("vdc_sobol_inv", C.c_void_p), ("tile_size", u32 * 2), ("tile_jitter", u32), ("tile_pad", u32)]


class Integrator(C.Structure):
    _fields_ = [("max_depth", u32), ("rr_depth", u32), ("rr_threshold", f32), ("env_prob", f32),
                ("light_count", u32), ("kind", u32), ("flags", u32), ("environment_medium_tag", u32)]


class Medium(C.Structure):
    _fields_ = [("kind", u32), ("priority", u32), ("eta", f32), ("g", f32), ("sigma_a", f32 * 3), ("sigma_s", f32 * 3),
                ("le", f32 * 3), ("pad", u32 * 3)]


class Bvh4Node(C.Structure):
    _fields_ = [("lo_x", f32 * 4), ("lo_y", f32 * 4), ("lo_z", f32 * 4), ("hi_x", f32 * 4), ("hi_y", f32 * 4),
                ("hi_z", f32 * 4), ("child", u32 * 4), ("pad", u32 * 4)]


class BvhTriangle(C.Structure):
    _fields_ = [("v0", f32 * 3), ("inst", u32), ("e1", f32 * 3), ("prim", u32), ("e2", f32 * 3), ("flags", u32)]


class Accel(C.Structure):
    _fields_ = [("nodes", C.POINTER(Bvh4Node)), ("node_count", u32), ("triangles", C.POINTER(BvhTriangle)),
                ("triangle_count", u32), ("world_min", f32 * 3), ("world_max", f32 * 3)]


class Scene(C.Structure):
    _fields_ = [("vertices", C.POINTER(Vertex)), ("vertex_count", u64),
                ("triangles", C.POINTER(Triangle)), ("triangle_count", u64),
                ("tri_alias", C.POINTER(AliasEntry)), ("tri_pdf", C.POINTER(f32)),
                ("meshes", C.POINTER(Mesh)), ("mesh_count", u32),
                ("instances", C.POINTER(Instance)), ("instance_count", u32),
                ("light_instances", C.POINTER(LightHandle)), ("light_instance_count", u32),
                ("surfaces", C.POINTER(Surface)), ("surface_count", u32),
                ("lights", C.POINTER(Light)), ("light_count", u32),
                ("textures", C.POINTER(Texture)), ("texture_count", u32),
                ("texels", C.POINTER(f32)), ("texel_count", u64),
                ("environment", Environment), ("camera", Camera), ("filter", Filter), ("film", Film),
                ("sampler", Sampler), ("integrator", Integrator), ("accel", Accel),
                ("any_non_opaque", u32), ("environment_child_count", u32), ("environment_children", C.c_void_p),
                ("media", C.POINTER(Medium)), ("medium_count", u32), ("pad_media", u32)]


class DenoiseParams(C.Structure):
    """lrhip_denoise_params (include/lrhip.h)"""
    _fields_ = [("width", u32), ("height", u32), ("iterations", u32), ("flags", u32),
                ("sigma_color", f32), ("sigma_normal", f32), ("sigma_depth", f32)]


DENOISE_DEMODULATE = 1  # LRHIP_DENOISE_DEMODULATE


class Ray(C.Structure):
    """lrhip_ray (include/lrhip.h): one row of the [N, 8] float32 array MegaPathRenderer.trace takes"""
    _fields_ = [("o", f32 * 3), ("t_min", f32), ("d", f32 * 3), ("t_max", f32)]


class RayHit(C.Structure):
    """lrhip_ray_hit (include/lrhip.h): one row of the [N, 8] 32-bit buffer behind RayHits"""
    _fields_ = [("t", f32), ("u", f32), ("v", f32), ("inst", u32), ("prim", u32), ("tri", u32), ("reserved", u32 * 2)]


class RayQueryParams(C.Structure):
    """lrhip_ray_query_params (include/lrhip.h)"""
    _fields_ = [("rays", C.c_void_p), ("out", C.c_void_p), ("count", u64), ("mode", u32), ("flags", u32)]


class RadianceQueryParams(C.Structure):
    """lrhip_radiance_query_params (include/lrhip.h)"""
    _fields_ = [("rays", C.c_void_p), ("streams", C.c_void_p), ("out", C.c_void_p), ("count", u64), ("spp_begin", u32), ("spp_end", u32),
                ("flags", u32), ("clamp", f32)]


class SurfacePoint(C.Structure):
    """lrhip_surface_point (include/lrhip.h): one row of the [N, 32] 32-bit buffer behind SurfacePoints"""
    _fields_ = [("p", f32 * 3), ("area", f32), ("ng", f32 * 3), ("flags", u32), ("ns", f32 * 3), ("inst", u32),
                ("tangent", f32 * 3), ("prim", u32), ("n_closure", f32 * 3), ("closure_kind", u32), ("uv", f32 * 2), ("roughness", f32 * 2),
                ("albedo", f32 * 3), ("surface", u32), ("emission", f32 * 3), ("light", u32)]


class SurfaceQueryParams(C.Structure):
    """lrhip_surface_query_params (include/lrhip.h)"""
    _fields_ = [("hits", C.c_void_p), ("rays", C.c_void_p), ("out", C.c_void_p), ("count", u64), ("flags", u32)]


class BsdfResult(C.Structure):
    """lrhip_bsdf_result (include/lrhip.h): one row of the [N, 8] 32-bit buffer behind BsdfResults"""
    _fields_ = [("f", f32 * 3), ("pdf", f32), ("wi", f32 * 3), ("event", u32)]


class BsdfQueryParams(C.Structure):
    """lrhip_bsdf_query_params (include/lrhip.h)"""
    _fields_ = [("hits", C.c_void_p), ("rays", C.c_void_p), ("dirs", C.c_void_p), ("out", C.c_void_p), ("count", u64), ("mode", u32),
                ("flags", u32)]


class LightResult(C.Structure):
    """lrhip_light_result (include/lrhip.h): one row of the [N, 8] 32-bit buffer behind LightSamples / LightResults"""
    _fields_ = [("L", f32 * 3), ("pdf", f32), ("kind", u32), ("reserved", u32 * 3)]


class LightQueryParams(C.Structure):
    """lrhip_light_query_params (include/lrhip.h)"""
    _fields_ = [("hits", C.c_void_p), ("rays", C.c_void_p), ("dirs", C.c_void_p), ("out_rays", C.c_void_p), ("out", C.c_void_p), ("count", u64),
                ("mode", u32), ("flags", u32)]


class GatherVertex(C.Structure):
    """lrhip_gather_vertex (include/lrhip.h): one row of the [N, 24] float32 buffer behind GatherVertices"""
    _fields_ = [("ray", Ray), ("shadow", Ray), ("nee", f32 * 3), ("light_pdf", f32), ("beta", f32 * 3), ("pdf", f32)]


class GatherVertexParams(C.Structure):
    """lrhip_gather_vertex_params (include/lrhip.h)"""
    _fields_ = [("records", C.c_void_p), ("normals", C.c_void_p), ("streams", C.c_void_p), ("out", C.c_void_p), ("count", u64),
                ("sample_index", u32), ("flags", u32)]


class GatherParams(C.Structure):
    """lrhip_gather_params (include/lrhip.h)"""
    _fields_ = [("records", C.c_void_p), ("normals", C.c_void_p), ("streams", C.c_void_p), ("out", C.c_void_p), ("count", u64),
                ("spp_begin", u32), ("spp_end", u32), ("flags", u32), ("clamp", f32)]


class SamplerQueryParams(C.Structure):
    """lrhip_sampler_query_params (include/lrhip.h)"""
    _fields_ = [("state", C.c_void_p), ("streams", C.c_void_p), ("indices", C.c_void_p), ("pattern", C.c_void_p), ("out", C.c_void_p),
                ("count", u64), ("pattern_count", u32), ("sample_index", u32), ("flags", u32), ("reserved", u32)]


class CameraSample(C.Structure):
    """lrhip_camera_sample (include/lrhip.h): one row of the [N, 4] 32-bit buffer behind CameraRays"""
    _fields_ = [("weight", f32), ("film_x", f32), ("film_y", f32), ("pixel", u32)]


class CameraQueryParams(C.Structure):
    """lrhip_camera_query_params (include/lrhip.h)"""
    _fields_ = [("pixels", C.c_void_p), ("u", C.c_void_p), ("out_rays", C.c_void_p), ("out", C.c_void_p), ("count", u64), ("flags", u32),
                ("reserved", u32)]


class FilmSplatParams(C.Structure):
    """lrhip_film_splat_params (include/lrhip.h)"""
    _fields_ = [("pixels", C.c_void_p), ("values", C.c_void_p), ("count", u64), ("flags", u32), ("clamp", f32)]


class InstanceUpdateParams(C.Structure):
    """lrhip_instance_update_params (include/lrhip.h)"""
    _fields_ = [("object_to_world", C.c_void_p), ("instances", C.c_void_p), ("count", u64), ("flags", u32)]


class MeshUpdateParams(C.Structure):
    """lrhip_mesh_update_params (include/lrhip.h)"""
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("mesh", u32), ("first_vertex", u32), ("count", u64), ("flags", u32)]


# lrhip_read_scene_table's tables (LRHIP_TABLE_*) and the bytes of one record of each (ids 4 to 7 name no table)
TABLE_NODES, TABLE_BVH_TRIANGLES, TABLE_INSTANCES, TABLE_SHADE_TRIANGLES, TABLE_VERTICES = 0, 1, 2, 3, 8
TABLE_LIGHT_INSTANCES, TABLE_LIGHT_TRIANGLES, TABLE_LIGHT_TRIANGLES_EXACT = 16, 17, 18  # the light sample's records, built on the device
TABLE_RECORD_BYTES = {TABLE_NODES: 64, TABLE_BVH_TRIANGLES: 48, TABLE_INSTANCES: 128, TABLE_SHADE_TRIANGLES: 128, TABLE_VERTICES: 32,
                      TABLE_LIGHT_INSTANCES: 96, TABLE_LIGHT_TRIANGLES: 80, TABLE_LIGHT_TRIANGLES_EXACT: 80}

RAY_CLOSEST, RAY_ANY = 0, 1  # LRHIP_RAY_CLOSEST / LRHIP_RAY_ANY
RAY_DEVICE_POINTERS, RAY_ALPHA_TEST = 1, 2  # LRHIP_RAY_DEVICE_POINTERS / LRHIP_RAY_ALPHA_TEST
RADIANCE_ACCUMULATE, RADIANCE_COUNTERS = 4, 8  # LRHIP_RADIANCE_ACCUMULATE / LRHIP_RADIANCE_COUNTERS
FEAT_QUERY = 65536  # LRHIP_FEAT_QUERY
MESH_RECOMPUTE_NORMALS = 16  # LRHIP_MESH_RECOMPUTE_NORMALS
SURFACE_GEOMETRY_ONLY = 32  # LRHIP_SURFACE_GEOMETRY_ONLY
# lrhip_surface_point::flags: LRHIP_SURFACE_VALID / BACK_FACING / HAS_SURFACE / HAS_LIGHT
SURFACE_VALID, SURFACE_BACK_FACING, SURFACE_HAS_SURFACE, SURFACE_HAS_LIGHT = 1, 2, 4, 8
BSDF_EVALUATE, BSDF_SAMPLE = 0, 1  # lrhip_bsdf_query_params::mode: LRHIP_BSDF_EVALUATE / LRHIP_BSDF_SAMPLE
# lrhip_bsdf_result::event: LRHIP_BSDF_EVENT_REFLECT / ENTER / EXIT / THROUGH (LR_INVALID_ID in the invalid record)
BSDF_EVENT_REFLECT, BSDF_EVENT_ENTER, BSDF_EVENT_EXIT, BSDF_EVENT_THROUGH = 0, 1, 2, 4
LIGHT_SAMPLE, LIGHT_EVALUATE = 0, 1  # lrhip_light_query_params::mode: LRHIP_LIGHT_SAMPLE / LRHIP_LIGHT_EVALUATE
LIGHT_FROM_POINTS = 64  # LRHIP_LIGHT_FROM_POINTS
# lrhip_light_result::kind: LRHIP_LIGHT_KIND_AREA / ENVIRONMENT / NONE (LR_INVALID_ID in the invalid record)
LIGHT_KIND_AREA, LIGHT_KIND_ENVIRONMENT, LIGHT_KIND_NONE = 0, 1, 2
# lrhip_sampler_query_params::pattern: LRHIP_DRAW_1D / LRHIP_DRAW_2D / LRHIP_DRAW_PIXEL_2D; LRHIP_SAMPLER_MAX_DRAWS; LRHIP_SAMPLER_START
DRAW_1D, DRAW_2D, DRAW_PIXEL_2D = 0, 1, 2
SAMPLER_MAX_DRAWS = 64
SAMPLER_START = 128
GATHER_FROM_POINTS = 64  # LRHIP_GATHER_FROM_POINTS
GATHER_ACCUMULATE = 4  # LRHIP_GATHER_ACCUMULATE
FEAT_GATHER = 131072  # LRHIP_FEAT_GATHER
LIGHTMAP_CONSERVATIVE = 256  # LRHIP_LIGHTMAP_CONSERVATIVE
# word 6 of a texel record of lrhip_lightmap_texels: LRHIP_LIGHTMAP_TEXEL_CENTRE / TOUCHED
LIGHTMAP_TEXEL_CENTRE, LIGHTMAP_TEXEL_TOUCHED = 1, 2

STRUCTS = {"lrhip_surface_point": SurfacePoint, "lrhip_surface_query_params": SurfaceQueryParams,
"lrhip_bsdf_result": BsdfResult, "lrhip_bsdf_query_params": BsdfQueryParams,
"lrhip_light_result": LightResult, "lrhip_light_query_params": LightQueryParams,
"lrhip_gather_vertex": GatherVertex, "lrhip_gather_vertex_params": GatherVertexParams, "lrhip_gather_params": GatherParams,
"lrhip_sampler_query_params": SamplerQueryParams, "lrhip_camera_sample": CameraSample, "lrhip_camera_query_params": CameraQueryParams,
"lrhip_film_splat_params": FilmSplatParams,
"lrhip_denoise_params": DenoiseParams, "lrhip_ray": Ray, "lrhip_ray_hit": RayHit, "lrhip_ray_query_params": RayQueryParams,
           "lrhip_radiance_query_params": RadianceQueryParams, "lrhip_instance_update_params": InstanceUpdateParams,
           "lrhip_mesh_update_params": MeshUpdateParams,
           "lr_scene": Scene, "lr_vertex": Vertex, "lr_triangle": Triangle, "lr_alias_entry": AliasEntry,
           "lr_mesh": Mesh, "lr_instance": Instance, "lr_texture": Texture, "lr_surface": Surface,
           "lr_light": Light, "lr_environment": Environment, "lr_camera": Camera, "lr_filter": Filter,
           "lr_film": Film, "lr_sampler": Sampler, "lr_integrator": Integrator, "lr_bvh4_node": Bvh4Node,
           "lr_bvh_triangle": BvhTriangle, "lr_accel": Accel, "lr_light_handle": LightHandle, "lr_medium": Medium}


class HipCounters(C.Structure):
    _fields_ = [(n, u64) for n in ("paths", "closest_rays", "shadow_rays", "nodes_visited", "tris_tested",
                                   "surface_hits", "nee_samples", "path_length_sum", "trace_steps", "trace_steps_busy",
                                   "shade_calls", "shade_busy", "trace_steps_starved", "shade_cycles", "trace_cycles", "wave_cycles", "nodes_empty",
                                   "shade_light_cycles", "shade_closure_cycles", "shade_regen_cycles")] + [("probe", u64 * 16)]

    def as_dict(self):
        return {n: (int(getattr(self, n)) if n != "probe" else [int(x) for x in self.probe]) for n, _ in self._fields_}


class RenderParams(C.Structure):
    """lrhip_render_params (include/lrhip.h)"""
    _fields_ = [("spp_begin", u32), ("spp_end", u32), ("tile_begin", u32), ("tile_end", u32),
                ("tile_stride", u32), ("flags", u32), ("balance_shards", u32), ("shutter_weight", f32)]


_libs: dict[str, C.CDLL] = {}


def _load(path: str) -> C.CDLL:
    if path not in _libs:
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make` (or __graft_entry__.build()) first")
        _libs[path] = C.CDLL(path)
    return _libs[path]


def host_lib() -> C.CDLL:
    lib = _load(os.path.join(LIB_DIR, "liblrhost.so"))
    if not getattr(lib, "_lr_ready", False):
        lib.lrhost_last_error.restype = C.c_char_p
        lib.lrhost_scene_camera_file.restype = C.c_char_p
        lib.lrhost_sizeof.restype = u64
        lib.lrhost_sizeof.argtypes = [C.c_char_p]
        lib.lrhost_scene_destroy.argtypes = [C.c_void_p]
        lib.lrhost_scene_view.argtypes = [C.c_void_p, C.c_int, C.POINTER(Scene)]
        lib.lrhost_scene_build_accel.argtypes = [C.c_void_p]
        lib.lrhost_scene_set_time.argtypes = [C.c_void_p, f32, C.POINTER(C.c_int)]
        lib.lrhost_scene_set_instance_transforms.argtypes = [C.c_void_p, u64, C.c_void_p, C.c_void_p]
        lib.lrhost_scene_set_mesh_vertices.argtypes = [C.c_void_p, u32, u32, u64, C.c_void_p, C.c_void_p, u32]
        lib.lrhost_scene_shutter_sample_count.argtypes = [C.c_void_p, C.c_int]
        lib.lrhost_scene_shutter_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(f32), C.POINTER(f32), C.POINTER(u32)]
        lib.lrhost_scene_camera_count.argtypes = [C.c_void_p]
        lib.lrhost_scene_camera_file.argtypes = [C.c_void_p, C.c_int]
        lib.lrhost_scene_has_lighting.argtypes = [C.c_void_p]
        lib.lrhost_save_image.argtypes = [C.c_char_p, C.c_void_p, u32, u32]
        lib.lrhost_save_image_channels.argtypes = [C.c_char_p, C.c_void_p, u32, u32, u32]
        lib.lrhost_scene_aov_settings.argtypes = [C.c_void_p, C.POINTER(u32), C.POINTER(u32)]
        lib.lrhost_scene_aov_denoise.argtypes = [C.c_void_p, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(f32 * 3)]
        lib._lr_ready = True
    return lib


def hip_lib(path: str | None = None) -> C.CDLL:
    """The product's device library.  Fails loudly when the HIP extension is missing.  `path`: another build of the same library
    (tests: the IEEE-arithmetic build of the lean kernel; tools: A/B variants) beside the shipped one in the same process."""
    # One HIP runtime and one RCCL per process: PyTorch-ROCm bundles its own libamdhip64 / librccl (same sonames as /opt/rocm's,
    # older versions), and whichever is loaded first serves both.  A Python host shares device pointers and streams with torch
    # (bench.py's film tensor, torch.distributed's process group), so torch's copies must be the ones: import it BEFORE the
    # library pulls /opt/rocm's through its RUNPATH.  (Loaded the other way round, torch ran on a HIP runtime it was not built
    # for and the process died in a double free at exit.)  C / C++ hosts have no torch and use /opt/rocm's alone.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # LRHIP_LIB selects an experimental build variant (tools/ only); the default is the shipped library
    lib = _load(path or os.environ.get("LRHIP_LIB") or os.path.join(LIB_DIR, "liblrhip.so"))
    if not getattr(lib, "_lr_ready", False):
        lib.lrhip_last_error.restype = C.c_char_p
        lib.lrhip_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.lrhip_destroy.argtypes = [C.c_void_p]
        lib.lrhip_upload_scene.argtypes = [C.c_void_p, C.POINTER(Scene)]
        lib.lrhip_update_scene.argtypes = [C.c_void_p, C.POINTER(Scene)]
        lib.lrhip_film_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.lrhip_comm_unique_id.argtypes = [C.c_void_p]
        lib.lrhip_comm_init_rank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        lib.lrhip_comm_init_all.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
        lib.lrhip_comm_destroy.argtypes = [C.c_void_p]
        lib.lrhip_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        lib.lrhip_device_count.argtypes = [C.POINTER(C.c_int)]
        lib.lrhip_bind_film.argtypes = [C.c_void_p, C.c_void_p]
        lib.lrhip_film_clear.argtypes = [C.c_void_p]
        lib.lrhip_render.argtypes = [C.c_void_p, C.POINTER(RenderParams)]
        lib.lrhip_synchronize.argtypes = [C.c_void_p]
        lib.lrhip_film_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.lrhip_get_counters.argtypes = [C.c_void_p, C.POINTER(HipCounters)]
        lib.lrhip_last_render_ms.restype = C.c_double
        lib.lrhip_last_render_ms.argtypes = [C.c_void_p]
        lib.lrhip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.lrhip_last_variant.restype = C.c_uint32
        lib.lrhip_last_variant.argtypes = [C.c_void_p]
        lib.lrhip_set_diagnostics.argtypes = [C.c_void_p, C.c_uint32, C.c_double]
        lib.lrhip_set_wavefront.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        lib.lrhip_set_scheduler.argtypes = [C.c_void_p, C.c_uint32]
        lib.lrhip_set_texture_storage.argtypes = [C.c_void_p, C.c_uint32]
        lib.lrhip_packed_texels.restype = C.c_uint64
        lib.lrhip_packed_texels.argtypes = [C.c_void_p]
        lib.lrhip_aov_download.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        lib.lrhip_denoise_default_params.restype = None
        lib.lrhip_denoise_default_params.argtypes = [C.POINTER(DenoiseParams)]
        lib.lrhip_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams)] + [C.c_void_p] * 5
        lib.lrhip_aov_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_uint32, C.c_uint32, C.c_void_p]
        lib.lrhip_last_denoise_ms.restype = C.c_double
        lib.lrhip_last_denoise_ms.argtypes = [C.c_void_p]
        lib.lrhip_trace_rays.argtypes = [C.c_void_p, C.POINTER(RayQueryParams)]
        lib.lrhip_last_trace_ms.restype = C.c_double
        lib.lrhip_last_trace_ms.argtypes = [C.c_void_p]
        lib.lrhip_trace_radiance.argtypes = [C.c_void_p, C.POINTER(RadianceQueryParams)]
        lib.lrhip_last_radiance_ms.restype = C.c_double
        lib.lrhip_last_radiance_ms.argtypes = [C.c_void_p]
        lib.lrhip_query_surface.argtypes = [C.c_void_p, C.POINTER(SurfaceQueryParams)]
        lib.lrhip_last_surface_ms.restype = C.c_double
        lib.lrhip_last_surface_ms.argtypes = [C.c_void_p]
        lib.lrhip_query_bsdf.argtypes = [C.c_void_p, C.POINTER(BsdfQueryParams)]
        lib.lrhip_last_bsdf_ms.restype = C.c_double
        lib.lrhip_last_bsdf_ms.argtypes = [C.c_void_p]
        lib.lrhip_query_light.argtypes = [C.c_void_p, C.POINTER(LightQueryParams)]
        lib.lrhip_last_light_ms.restype = C.c_double
        lib.lrhip_last_light_ms.argtypes = [C.c_void_p]
        lib.lrhip_query_sampler.argtypes = [C.c_void_p, C.POINTER(SamplerQueryParams)]
        lib.lrhip_query_camera.argtypes = [C.c_void_p, C.POINTER(CameraQueryParams)]
        lib.lrhip_film_splat.argtypes = [C.c_void_p, C.POINTER(FilmSplatParams)]
        lib.lrhip_last_camera_ms.restype = C.c_double
        lib.lrhip_last_camera_ms.argtypes = [C.c_void_p]
        lib.lrhip_set_instance_transforms.argtypes = [C.c_void_p, C.POINTER(InstanceUpdateParams)]
        lib.lrhip_last_instance_update_ms.restype = C.c_double
        lib.lrhip_last_instance_update_ms.argtypes = [C.c_void_p]
        lib.lrhip_set_mesh_vertices.argtypes = [C.c_void_p, C.POINTER(MeshUpdateParams)]
        lib.lrhip_last_mesh_update_ms.restype = C.c_double
        lib.lrhip_last_mesh_update_ms.argtypes = [C.c_void_p]
        lib.lrhip_query_gather_vertex.argtypes = [C.c_void_p, C.POINTER(GatherVertexParams)]
        lib.lrhip_gather_irradiance.argtypes = [C.c_void_p, C.POINTER(GatherParams)]
        lib.lrhip_last_gather_ms.restype = C.c_double
        lib.lrhip_last_gather_ms.argtypes = [C.c_void_p]
        lib.lrhip_lightmap_texels.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.lrhip_last_lightmap_ms.restype = C.c_double
        lib.lrhip_last_lightmap_ms.argtypes = [C.c_void_p]
        lib.lrhip_read_scene_table.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
        lib.lrhip_scene_table_bytes.restype = C.c_uint64
        lib.lrhip_scene_table_bytes.argtypes = [C.c_void_p, C.c_uint32]
        lib._lr_ready = True
    return lib
