"""Scene loading through liblrhost.so (host C ABI, include/lrhost.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi


class HostError(RuntimeError):
    pass


# the AOV integrator's components in lr_scene.h LR_AOV_* order (bit k of lr_integrator.flags) and its dump strategies (LR_AOV_DUMP_*)
AOV_COMPONENTS = ("sample", "diffuse", "specular", "normal", "albedo", "depth", "roughness", "ndc", "mask")
AOV_DUMPS = ("power2", "all", "final")


def aov_channels(component: str) -> int:
    """floats per pixel of an AOV buffer: depth and mask 1, every other component 3 (roughness is (rx, ry, 0), aov.cpp:157)"""
    return 1 if component in ("depth", "mask") else 3


class _MeshVertexCounts:
    """the vertex count of every mesh of a view as a read-only sequence (render.check_mesh_vertices looks at one entry)"""

    def __init__(self, view):
        self._view = view

    def __len__(self) -> int:
        return int(self._view.mesh_count)

    def __getitem__(self, mesh: int) -> int:
        return int(self._view.meshes[mesh].vertex_count)


class Scene:
    """A parsed + flattened scene (lrhost_scene) and its POD view (lr_scene)."""

    def __init__(self, handle: C.c_void_p):
        self._lib = _ffi.host_lib()
        self._handle = handle
        self._views: dict[int, _ffi.Scene] = {}

    @staticmethod
    def _macros(macros):
        macros = macros or {}
        keys = (C.c_char_p * len(macros))(*[k.encode() for k in macros])
        vals = (C.c_char_p * len(macros))(*[str(v).encode() for v in macros.values()])
        return keys, vals, len(macros)

    @classmethod
    def load(cls, path: str, macros: dict | None = None, build_accel: bool = True) -> "Scene":
        lib = _ffi.host_lib()
        keys, vals, n = cls._macros(macros)
        handle = C.c_void_p()
        if lib.lrhost_scene_load_file(path.encode(), keys, vals, n, C.byref(handle)) != 0:
            raise HostError(lib.lrhost_last_error().decode())
        scene = cls(handle)
        if build_accel:
            scene.build_accel()
        return scene

    @classmethod
    def from_string(cls, source: str, virtual_path: str = "", macros: dict | None = None, json: bool = False,
                    build_accel: bool = True) -> "Scene":
        lib = _ffi.host_lib()
        keys, vals, n = cls._macros(macros)
        handle = C.c_void_p()
        rc = lib.lrhost_scene_load_string(source.encode(), virtual_path.encode(), 1 if json else 0, keys, vals, n,
                                          C.byref(handle))
        if rc != 0:
            raise HostError(lib.lrhost_last_error().decode())
        scene = cls(handle)
        if build_accel:
            scene.build_accel()
        return scene

    def build_accel(self) -> None:
        if self._lib.lrhost_scene_build_accel(self._handle) != 0:
            raise HostError(self._lib.lrhost_last_error().decode())
        self._views.clear()

    def set_time(self, time: float) -> bool:
        """Pipeline::update (src/base/pipeline.cpp:101-113): move every animated transform to `time`; the tables behind
        view() change in place (upload / create the oracle again).  -> whether anything moved"""
        updated = C.c_int(0)
        if self._lib.lrhost_scene_set_time(self._handle, time, C.byref(updated)) != 0:
            raise HostError(self._lib.lrhost_last_error().decode())
        self._views.clear()
        return bool(updated.value)

    def set_instance_transforms(self, matrices, instances=None) -> None:
        """lrhost_scene_set_instance_transforms: the host mirror of MegaPathRenderer.set_instance_transforms -- matrices[i] becomes the
        object-to-world matrix of instance instances[i] (None: of instance i), the moved instances are re-baked and the BVH is refitted when
        it is built; the tables behind view() change in place (upload again, with keep_film to carry the film on).  matrices: a float32 numpy
        array [N, 4, 4] or [N, 16] in COLUMN-MAJOR storage, the layout of lr_instance.object_to_world (a numpy row-major matrix M goes in as
        M.T); instances: N integer ids or None (render.check_instance_transforms has the rules)."""
        from .render import check_instance_transforms
        if check_instance_transforms(matrices, instances, int(self.view().instance_count)) != "numpy":
            raise ValueError("set_instance_transforms: the host scene takes numpy arrays")
        ids = np.ascontiguousarray(instances, dtype=np.uint32) if instances is not None else None
        rc = self._lib.lrhost_scene_set_instance_transforms(self._handle, int(matrices.shape[0]), ids.ctypes.data if ids is not None else None,
                                                            matrices.ctypes.data)
        if rc != 0:
            raise HostError(self._lib.lrhost_last_error().decode())
        self._views.clear()

    def set_mesh_vertices(self, mesh: int, positions, normals=None, first: int = 0, recompute_normals: bool = False) -> None:
        """lrhost_scene_set_mesh_vertices: the host mirror of MegaPathRenderer.set_mesh_vertices -- vertices first .. first + N - 1 of mesh
        `mesh` get the object-space positions [N, 3] and, if given, the normals [N, 3] (None: kept, or with recompute_normals recomputed
        for the whole mesh); every instance of the mesh is re-baked and the BVH is refitted when it is built; the tables behind view()
        change in place (upload again, with keep_film to carry the film on).  float32 numpy arrays only (render.check_mesh_vertices has
        the rules); HostError for a mesh with an emissive instance."""
        from .render import check_mesh_vertices
        if recompute_normals and normals is not None:
            raise ValueError("set_mesh_vertices: normals must be None with recompute_normals")
        if check_mesh_vertices(positions, normals, mesh, first, _MeshVertexCounts(self.view())) != "numpy":
            raise ValueError("set_mesh_vertices: the host scene takes numpy arrays")
        rc = self._lib.lrhost_scene_set_mesh_vertices(self._handle, int(mesh), int(first), int(positions.shape[0]), positions.ctypes.data,
                                                      normals.ctypes.data if normals is not None else None,
                                                      _ffi.MESH_RECOMPUTE_NORMALS if recompute_normals else 0)
        if rc != 0:
            raise HostError(self._lib.lrhost_last_error().decode())
        self._views.clear()

    def instance_mesh(self, instance: int) -> int:
        """the mesh of an instance: lr_instance.handle.x >> 10, an index into lr_scene.meshes (instances may share a mesh)"""
        view = self.view()
        if not 0 <= int(instance) < int(view.instance_count):
            raise ValueError(f"instance_mesh: instance {instance} out of range ({int(view.instance_count)} instances)")
        return int(view.instances[int(instance)].handle.x) >> 10

    def mesh_vertices(self, mesh: int) -> tuple[np.ndarray, np.ndarray]:
        """copies of a mesh's object-space vertex positions and normals -> (positions [V, 3], normals [V, 3]), float32"""
        view = self.view()
        if not 0 <= int(mesh) < int(view.mesh_count):
            raise ValueError(f"mesh_vertices: mesh {mesh} out of range ({int(view.mesh_count)} meshes)")
        record = view.meshes[int(mesh)]
        offset, count = int(record.vertex_offset), int(record.vertex_count)
        if count == 0:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
        address = C.addressof(view.vertices.contents) + offset * 32
        table = np.frombuffer(C.string_at(address, count * 32), np.float32).reshape(count, 8)
        return np.ascontiguousarray(table[:, 0:3]), np.ascontiguousarray(table[:, 3:6])

    def mesh_uvs(self, mesh: int) -> np.ndarray:
        """a copy of a mesh's vertex UVs -> [V, 2] float32 (what the UV rasteriser of MegaPathRenderer.lightmap_texels reads; meaningful where
        the mesh's instances carry LR_SHAPE_HAS_VERTEX_UV)"""
        view = self.view()
        if not 0 <= int(mesh) < int(view.mesh_count):
            raise ValueError(f"mesh_uvs: mesh {mesh} out of range ({int(view.mesh_count)} meshes)")
        record = view.meshes[int(mesh)]
        offset, count = int(record.vertex_offset), int(record.vertex_count)
        if count == 0:
            return np.zeros((0, 2), np.float32)
        address = C.addressof(view.vertices.contents) + offset * 32
        table = np.frombuffer(C.string_at(address, count * 32), np.float32).reshape(count, 8)
        return np.ascontiguousarray(table[:, 6:8])

    def mesh_triangles(self, mesh: int) -> np.ndarray:
        """a copy of a mesh's triangles -> [T, 3] uint32, indices into the mesh's own vertices (mesh_vertices, mesh_uvs); row `prim` is the
        triangle a hit or texel record names"""
        view = self.view()
        if not 0 <= int(mesh) < int(view.mesh_count):
            raise ValueError(f"mesh_triangles: mesh {mesh} out of range ({int(view.mesh_count)} meshes)")
        record = view.meshes[int(mesh)]
        offset, count = int(record.triangle_offset), int(record.triangle_count)
        if count == 0:
            return np.zeros((0, 3), np.uint32)
        address = C.addressof(view.triangles.contents) + offset * 12
        return np.frombuffer(C.string_at(address, count * 12), np.uint32).reshape(count, 3).copy()

    def shutter_samples(self, camera: int = 0) -> list[tuple[float, float, int]]:
        """Camera::shutter_samples (src/base/camera.cpp:163-203) -> [(time, weight, spp)]"""
        out = []
        for i in range(self._lib.lrhost_scene_shutter_sample_count(self._handle, camera)):
            t, w, n = C.c_float(), C.c_float(), C.c_uint32()
            if self._lib.lrhost_scene_shutter_sample(self._handle, camera, i, C.byref(t), C.byref(w), C.byref(n)) != 0:
                raise HostError(self._lib.lrhost_last_error().decode())
            out.append((t.value, w.value, n.value))
        return out

    @property
    def camera_count(self) -> int:
        return self._lib.lrhost_scene_camera_count(self._handle)

    def view(self, camera: int = 0) -> _ffi.Scene:
        if camera not in self._views:
            v = _ffi.Scene()
            if self._lib.lrhost_scene_view(self._handle, camera, C.byref(v)) != 0:
                raise HostError(self._lib.lrhost_last_error().decode())
            v._owner = self  # keep the host tables alive as long as the view is referenced
            self._views[camera] = v
        return self._views[camera]

    def camera_file(self, camera: int = 0) -> str:
        return self._lib.lrhost_scene_camera_file(self._handle, camera).decode()

    @property
    def has_lighting(self) -> bool:
        return bool(self._lib.lrhost_scene_has_lighting(self._handle))

    def aov_denoise(self) -> dict:
        """lrhost_scene_aov_denoise: the AOV integrator's denoise properties -- "enabled" (denoise { false }) and, with lrhip.h's
        defaults where the scene sets none, MegaPathRenderer.denoise_aov's keywords iterations, sigma_color, sigma_normal, sigma_depth and
        demodulate.  HostError for any other integrator."""
        enabled, iterations, demodulate, sigmas = C.c_uint32(), C.c_uint32(), C.c_uint32(), (C.c_float * 3)()
        if self._lib.lrhost_scene_aov_denoise(self._handle, C.byref(enabled), C.byref(iterations), C.byref(demodulate), C.byref(sigmas)) != 0:
            raise HostError(self._lib.lrhost_last_error().decode())
        return {"enabled": bool(enabled.value), "iterations": iterations.value, "sigma_color": float(sigmas[0]),
                "sigma_normal": float(sigmas[1]), "sigma_depth": float(sigmas[2]), "demodulate": bool(demodulate.value)}

    def aov_settings(self) -> dict:
        """The AOV integrator's settings (src/integrators/aov.cpp:48-87): the enabled components (AOV_COMPONENTS order), noisy_count (samples
        per pixel, in place of the camera's spp), the dump strategy and the path depth.  A scene with denoise { true } has one more key,
        "denoise": aov_denoise() without "enabled", i.e. the keywords of MegaPathRenderer.denoise_aov.  HostError for any other integrator."""
        n, dump = C.c_uint32(), C.c_uint32()
        if self._lib.lrhost_scene_aov_settings(self._handle, C.byref(n), C.byref(dump)) != 0:
            raise HostError(self._lib.lrhost_last_error().decode())
        integrator = self.view().integrator
        settings = {"components": [c for k, c in enumerate(AOV_COMPONENTS) if (integrator.flags >> k) & 1], "noisy_count": n.value,
                    "dump": AOV_DUMPS[dump.value], "depth": int(integrator.max_depth)}
        denoise = self.aov_denoise()
        if denoise.pop("enabled"):
            settings["denoise"] = denoise
        return settings

    def resolution(self, camera: int = 0) -> tuple[int, int]:
        v = self.view(camera)
        return int(v.camera.width), int(v.camera.height)

    def close(self) -> None:
        if self._handle:
            self._lib.lrhost_scene_destroy(self._handle)
            self._handle = None
            self._views.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def save_image(path: str, rgba: np.ndarray) -> None:
    """save_image of the reference (src/util/imageio.cpp:694-726): float RGBA -> .exr / .hdr.  [H, W, 3] is written as RGB and
    [H, W] / [H, W, 1] as one channel (the AOV integrator's buffers: EXR channel "A", HDR gray)"""
    lib = _ffi.host_lib()
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    h, w = rgba.shape[:2]
    channels = 1 if rgba.ndim == 2 else rgba.shape[2]
    if channels == 4:
        rc = lib.lrhost_save_image(path.encode(), rgba.ctypes.data, w, h)
    else:
        rc = lib.lrhost_save_image_channels(path.encode(), rgba.ctypes.data, w, h, channels)
    if rc != 0:
        raise HostError(lib.lrhost_last_error().decode())


def load_image(path: str):
    """LoadedImage::load of the reference (src/util/imageio.cpp:419-538) -> (float RGBA array [H, W, 4], channels)"""
    import ctypes as C
    lib = _ffi.host_lib()
    lib.lrhost_load_image.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.lrhost_free.argtypes = [C.c_void_p]
    ptr = C.POINTER(C.c_float)()
    w, h, ch = C.c_uint32(), C.c_uint32(), C.c_uint32()
    if lib.lrhost_load_image(path.encode(), C.byref(ptr), C.byref(w), C.byref(h), C.byref(ch)) != 0:
        raise HostError(lib.lrhost_last_error().decode())
    try:
        return np.ctypeslib.as_array(ptr, shape=(h.value, w.value, 4)).copy(), ch.value
    finally:
        lib.lrhost_free(ptr)
