"""ctypes binding of libportrayer_host.so (include/portrayer_host.h): the C++ host layer that mirrors
the portrayer crate's API above the pixel loop (scene graph, flattening, k-d build, camera,
Image::render) and drives the gfx950 kernels through the C ABI. No CPU fallback exists."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import numpy as np

from . import _hip as H

LIB_PATH = os.path.join(H.PKG_DIR, "libportrayer_host.so")
REPO_ROOT = os.path.dirname(H.PKG_DIR)
DEFAULT_ASSETS = os.path.join(REPO_ROOT, "tests", "golden", "assets")

_dp, _ip, _up, _u64p, _u8p = H._dp, H._ip, H._up, H._u64p, H._u8p

EXPORTS = ["ph_last_error", "ph_scene_create", "ph_example_scene", "ph_scene_destroy", "ph_scene_counts", "ph_scene_export", "ph_scene_export_textures",
           "ph_scene_flatten", "ph_scene_kdtree", "ph_scene_kdmesh_tree", "ph_camera", "ph_obj_load", "ph_renderer_create", "ph_renderer_destroy",
           "ph_renderer_context", "ph_renderer_ranks", "ph_renderer_node", "ph_renderer_prepare_ms", "ph_renderer_render", "ph_renderer_aov", "ph_renderer_rays", "ph_renderer_segments", "ph_renderer_ao", "ph_renderer_ao_camera", "ph_renderer_gather", "ph_renderer_gather_camera", "ph_renderer_probe", "ph_renderer_chart_triangles", "ph_renderer_chart_mesh", "ph_renderer_chart", "ph_renderer_ao_chart", "ph_renderer_gather_chart", "ph_renderer_direct", "ph_renderer_direct_camera", "ph_renderer_direct_chart", "ph_renderer_radiance", "ph_renderer_film_create", "ph_renderer_film_destroy", "ph_renderer_film_reset", "ph_renderer_film_add", "ph_renderer_film_add_lens", "ph_renderer_film_resolve", "ph_renderer_film_counts", "ph_renderer_film_create_moments", "ph_renderer_film_add_map", "ph_renderer_film_error", "ph_renderer_film_refine", "ph_renderer_film_denoise", "ph_renderer_guides", "ph_renderer_film_denoise_albedo", "ph_renderer_update", "ph_scene_same_structure", "ph_renderer_deform", "ph_scene_same_topology", "ph_renderer_deform_device", "ph_renderer_mesh_count", "ph_renderer_mesh_vertices", "ph_example_render_to_png", "ph_png_read", "ph_png_write", "ph_image_read", "ph_scene_graph"]


class PortrayerHostError(RuntimeError):
    pass


class PortrayerPanic(PortrayerHostError):
    """Raised where the reference would panic (e.g. ImageSliceMut::new, render.rs:79-90)."""


class PhDeviceMesh(C.Structure):
    """ph_device_mesh: one mesh of ph_renderer_deform_device, its vertices in device memory"""
    _fields_ = [("mesh", C.c_uint32), ("d_positions", C.c_void_p), ("d_normals", C.c_void_p)]


class PhSceneDesc(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32), ("ops", C.c_char_p), ("ops_off", _up), ("args", _dp), ("args_off", _up),
        ("prim_type", _ip), ("prim_data", _ip), ("prim_flags", _ip), ("material", _ip), ("child_off", _up), ("children", _up),
        ("root", C.c_uint32),
        ("n_meshes", C.c_uint32), ("mesh_vert_off", _u64p), ("mesh_tri_off", _u64p), ("mesh_positions", _dp), ("mesh_normals", _dp),
        ("mesh_has_normals", _u8p), ("mesh_indices", _up),
        ("n_triangles", C.c_uint32), ("tri_vertices", _dp), ("tri_normals", _dp), ("tri_has_normals", _u8p),
        ("n_materials", C.c_uint32), ("materials", _dp), ("n_lights", C.c_uint32), ("lights", _dp), ("ambient", C.c_double * 3),
        ("mesh_texcoords", _dp), ("mesh_has_texcoords", _u8p), ("tri_texcoords", _dp), ("tri_has_texcoords", _u8p),
        ("material_texture", _ip), ("material_normal_map", _ip), ("material_uv_trans", _dp),
        ("n_textures", C.c_uint32), ("texture_size", _up), ("texture_offset", _u64p), ("texture_rgb", _u8p),
    ]


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        H.lib()
        if not os.path.exists(LIB_PATH):
            raise PortrayerHostError(f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build())")
        l = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        l.ph_last_error.restype = C.c_char_p
        l.ph_scene_create.restype = C.c_int; l.ph_scene_create.argtypes = [C.POINTER(PhSceneDesc), C.POINTER(vp)]
        l.ph_example_scene.restype = C.c_int; l.ph_example_scene.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp), _dp, _up]
        l.ph_scene_destroy.restype = None; l.ph_scene_destroy.argtypes = [vp]
        l.ph_scene_counts.restype = C.c_int; l.ph_scene_counts.argtypes = [vp, _u64p]
        l.ph_scene_export.restype = C.c_int
        l.ph_scene_export.argtypes = [vp, _dp, _ip, _ip, _ip, _ip, _up, _up, _up, _u64p, _u64p, _dp, _dp, _u8p, _up, _dp, _dp, _u8p, _dp, _dp, _dp]
        l.ph_scene_flatten.restype = C.c_int; l.ph_scene_flatten.argtypes = [vp, C.c_uint32, _dp, _dp, _dp, _ip, _ip, _dp]
        l.ph_scene_kdtree.restype = C.c_int
        l.ph_scene_kdtree.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, _ip, _dp, _ip, _ip, _ip, _ip, _ip, _up, _dp, _ip]
        l.ph_scene_kdmesh_tree.restype = C.c_int
        l.ph_scene_kdmesh_tree.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, _ip, _dp, _ip, _ip, _ip, _ip, _ip, _up, _dp, _ip]
        l.ph_camera.restype = C.c_int; l.ph_camera.argtypes = [_dp, C.c_double, C.c_double, C.POINTER(H.PtCamera)]
        l.ph_obj_load.restype = C.c_int; l.ph_obj_load.argtypes = [C.c_char_p, _u64p, _dp, _dp, _up, C.c_uint64, C.c_uint64]
        l.ph_renderer_create.restype = C.c_int; l.ph_renderer_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        l.ph_renderer_destroy.restype = None; l.ph_renderer_destroy.argtypes = [vp]
        l.ph_renderer_context.restype = vp; l.ph_renderer_context.argtypes = [vp]
        l.ph_renderer_ranks.restype = C.c_int; l.ph_renderer_ranks.argtypes = [vp]
        l.ph_renderer_node.restype = vp; l.ph_renderer_node.argtypes = [vp]
        l.ph_renderer_prepare_ms.restype = C.c_int; l.ph_renderer_prepare_ms.argtypes = [vp, _dp]
        l.ph_renderer_render.restype = C.c_int
        l.ph_renderer_render.argtypes = [vp, _dp, C.POINTER(H.PtRenderParams), _dp, _u8p, _dp, C.POINTER(H.PtStats)]
        l.ph_renderer_aov.restype = C.c_int
        l.ph_renderer_aov.argtypes = [vp, _dp, C.POINTER(H.PtAovParams), C.POINTER(H.PtAovBuffers), _dp]
        l.ph_renderer_guides.restype = C.c_int
        l.ph_renderer_guides.argtypes = [vp, _dp, C.POINTER(H.PtAovParams), C.POINTER(H.PtGuidesBuffers), _dp]
        l.ph_renderer_rays.restype = C.c_int
        l.ph_renderer_rays.argtypes = [vp, C.POINTER(H.PtRaysParams), _dp, _dp, C.POINTER(H.PtRaysBuffers), _dp]
        l.ph_renderer_segments.restype = C.c_int
        l.ph_renderer_segments.argtypes = [vp, C.POINTER(H.PtRaysParams), _dp, _dp, _dp, C.POINTER(H.PtRaysBuffers), _dp]
        l.ph_renderer_ao.restype = C.c_int
        l.ph_renderer_ao.argtypes = [vp, C.POINTER(H.PtAoParams), _dp, _dp, C.POINTER(H.PtAoBuffers), _dp]
        l.ph_renderer_ao_camera.restype = C.c_int
        l.ph_renderer_ao_camera.argtypes = [vp, _dp, C.c_uint32, C.c_uint32, C.POINTER(H.PtAoParams), C.POINTER(H.PtAoBuffers), _dp]
        l.ph_renderer_gather.restype = C.c_int
        l.ph_renderer_gather.argtypes = [vp, C.POINTER(H.PtGatherParams), _dp, _dp, _dp, C.POINTER(H.PtGatherBuffers), _dp]
        l.ph_renderer_gather_camera.restype = C.c_int
        l.ph_renderer_gather_camera.argtypes = [vp, _dp, C.c_uint32, C.c_uint32, C.POINTER(H.PtGatherParams), _dp, C.POINTER(H.PtGatherBuffers), _dp]
        l.ph_renderer_chart_triangles.restype = C.c_int
        l.ph_renderer_chart_triangles.argtypes = [vp, C.c_uint32, _u64p]
        l.ph_renderer_chart_mesh.restype = C.c_int
        l.ph_renderer_chart_mesh.argtypes = [vp, C.c_uint32, _u64p, C.c_uint32, _up]
        l.ph_renderer_chart.restype = C.c_int
        l.ph_renderer_chart.argtypes = [vp, C.POINTER(H.PtChartParams), _dp, C.POINTER(H.PtChartBuffers), _dp]
        l.ph_renderer_probe.restype = C.c_int
        l.ph_renderer_probe.argtypes = [vp, C.POINTER(H.PtProbeParams), _dp, _dp, C.POINTER(H.PtProbeBuffers), _dp]
        l.ph_renderer_direct.restype = C.c_int
        l.ph_renderer_direct.argtypes = [vp, C.POINTER(H.PtDirectParams), _dp, _dp, C.POINTER(H.PtDirectBuffers), _dp]
        l.ph_renderer_direct_camera.restype = C.c_int
        l.ph_renderer_direct_camera.argtypes = [vp, _dp, C.c_uint32, C.c_uint32, C.POINTER(H.PtDirectParams), C.POINTER(H.PtDirectBuffers), _dp]
        l.ph_renderer_direct_chart.restype = C.c_int
        l.ph_renderer_direct_chart.argtypes = [vp, C.POINTER(H.PtChartParams), _dp, C.POINTER(H.PtDirectParams), C.POINTER(H.PtDirectBuffers), _dp]
        l.ph_renderer_ao_chart.restype = C.c_int
        l.ph_renderer_ao_chart.argtypes = [vp, C.POINTER(H.PtChartParams), _dp, C.POINTER(H.PtAoParams), C.POINTER(H.PtAoBuffers), _dp]
        l.ph_renderer_gather_chart.restype = C.c_int
        l.ph_renderer_gather_chart.argtypes = [vp, C.POINTER(H.PtChartParams), _dp, C.POINTER(H.PtGatherParams), _dp, C.POINTER(H.PtGatherBuffers), _dp]
        l.ph_renderer_radiance.restype = C.c_int
        l.ph_renderer_radiance.argtypes = [vp, C.POINTER(H.PtRadianceParams), _dp, _dp, _dp, _dp, _dp]
        l.ph_renderer_film_create.restype = C.c_int; l.ph_renderer_film_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        l.ph_renderer_film_destroy.restype = C.c_int; l.ph_renderer_film_destroy.argtypes = [vp, vp]
        l.ph_renderer_film_reset.restype = C.c_int; l.ph_renderer_film_reset.argtypes = [vp, vp]
        l.ph_renderer_film_add.restype = C.c_int; l.ph_renderer_film_add.argtypes = [vp, vp, _dp, _dp, C.POINTER(H.PtFilmParams), _dp]
        l.ph_renderer_film_add_lens.restype = C.c_int; l.ph_renderer_film_add_lens.argtypes = [vp, vp, _dp, C.POINTER(H.PtLens), _dp, C.POINTER(H.PtFilmParams), _dp]
        l.ph_renderer_film_resolve.restype = C.c_int; l.ph_renderer_film_resolve.argtypes = [vp, vp, _u8p, _dp]
        l.ph_renderer_film_counts.restype = C.c_int; l.ph_renderer_film_counts.argtypes = [vp, vp, _up]
        l.ph_renderer_film_create_moments.restype = C.c_int; l.ph_renderer_film_create_moments.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        l.ph_renderer_film_add_map.restype = C.c_int; l.ph_renderer_film_add_map.argtypes = [vp, vp, _dp, _dp, C.POINTER(H.PtFilmMapParams), _up, _dp]
        l.ph_renderer_film_error.restype = C.c_int; l.ph_renderer_film_error.argtypes = [vp, vp, _dp]
        l.ph_renderer_film_refine.restype = C.c_int
        l.ph_renderer_film_refine.argtypes = [vp, vp, _dp, _dp, C.POINTER(H.PtFilmMapParams), C.POINTER(H.PtFilmRefineParams), C.c_uint32, _u64p, _dp]
        l.ph_renderer_film_denoise.restype = C.c_int
        l.ph_renderer_film_denoise.argtypes = [vp, vp, _dp, C.POINTER(H.PtDenoiseParams), C.POINTER(H.PtDenoiseGuides), _u8p, _dp, _dp]
        l.ph_renderer_film_denoise_albedo.restype = C.c_int
        l.ph_renderer_film_denoise_albedo.argtypes = [vp, vp, _dp, C.POINTER(H.PtDenoiseParams), C.POINTER(H.PtDenoiseGuides), _dp, _u8p, _dp, _dp]
        l.ph_renderer_update.restype = C.c_int; l.ph_renderer_update.argtypes = [vp, vp]
        l.ph_scene_same_structure.restype = C.c_int; l.ph_scene_same_structure.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
        l.ph_renderer_deform.restype = C.c_int; l.ph_renderer_deform.argtypes = [vp, vp, C.c_int]
        l.ph_renderer_deform_device.restype = C.c_int; l.ph_renderer_deform_device.argtypes = [vp, C.c_uint32, C.POINTER(PhDeviceMesh), C.c_int, vp]
        l.ph_renderer_mesh_count.restype = C.c_int64; l.ph_renderer_mesh_count.argtypes = [vp]
        l.ph_renderer_mesh_vertices.restype = C.c_int64; l.ph_renderer_mesh_vertices.argtypes = [vp, C.c_uint32]
        l.ph_scene_same_topology.restype = C.c_int; l.ph_scene_same_topology.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
        l.ph_scene_export_textures.restype = C.c_int
        l.ph_scene_export_textures.argtypes = [vp, _u64p, _ip, _ip, _dp, _up, _u64p, _u8p, _dp, _u8p, _dp, _u8p]
        l.ph_example_render_to_png.restype = C.c_int
        l.ph_example_render_to_png.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p]
        l.ph_png_read.restype = C.c_int; l.ph_png_read.argtypes = [C.c_char_p, _up, _u8p, C.c_uint64]
        l.ph_scene_graph.restype = C.c_int
        l.ph_scene_graph.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _up, _up, _up, _dp, _dp, _dp, _up]
        l.ph_image_read.restype = C.c_int; l.ph_image_read.argtypes = [C.c_char_p, _up, _u8p, C.c_uint64]
        l.ph_png_write.restype = C.c_int; l.ph_png_write.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, _u8p]
        _lib = l
    return _lib


def _check(rc: int, what: str):
    if rc < 0:
        msg = lib().ph_last_error().decode()
        raise (PortrayerPanic if rc == -2 else PortrayerHostError)(f"{what} failed with {rc}: {msg}")
    return rc


def _p(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


class SameStructure:
    """Scene.same_structure()'s answer: truthy or not, with the first difference in `reason`."""

    def __init__(self, same: bool, reason: str):
        self.same, self.reason = same, reason

    def __bool__(self):
        return self.same

    def __repr__(self):
        return "SameStructure(%r, %r)" % (self.same, self.reason)


class Scene:
    """A scene::HierScene owned by the C++ host library."""

    def __init__(self, handle, camera=None, size=None):
        self._h = handle
        self.camera = camera  # 10 doubles: eye, center, up, fovy (radians), for example scenes
        self.size = size

    @staticmethod
    def from_description(d: dict) -> "Scene":
        """d: arrays named like ph_scene_desc's fields (see tests/host_glue.py for a producer)."""
        keep = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        s = PhSceneDesc()
        s.n_nodes = len(keep["prim_type"])
        s.ops = keep["ops"]; s.ops_off = _p(keep["ops_off"], _up); s.args = _p(keep["args"], _dp); s.args_off = _p(keep["args_off"], _up)
        s.prim_type = _p(keep["prim_type"], _ip); s.prim_data = _p(keep["prim_data"], _ip); s.prim_flags = _p(keep["prim_flags"], _ip)
        s.material = _p(keep["material"], _ip); s.child_off = _p(keep["child_off"], _up); s.children = _p(keep["children"], _up)
        s.root = int(keep["root"])
        s.n_meshes = len(keep["mesh_vert_off"]) - 1
        s.mesh_vert_off = _p(keep["mesh_vert_off"], _u64p); s.mesh_tri_off = _p(keep["mesh_tri_off"], _u64p)
        s.mesh_positions = _p(keep["mesh_positions"], _dp); s.mesh_normals = _p(keep["mesh_normals"], _dp)
        s.mesh_has_normals = _p(keep["mesh_has_normals"], _u8p); s.mesh_indices = _p(keep["mesh_indices"], _up)
        s.n_triangles = int(keep["n_triangles"])
        s.tri_vertices = _p(keep["tri_vertices"], _dp); s.tri_normals = _p(keep["tri_normals"], _dp); s.tri_has_normals = _p(keep["tri_has_normals"], _u8p)
        s.n_materials = int(keep["n_materials"]); s.materials = _p(keep["materials"], _dp)
        s.n_lights = int(keep["n_lights"]); s.lights = _p(keep["lights"], _dp)
        s.ambient = (C.c_double * 3)(*map(float, keep["ambient"]))
        if keep.get("n_textures"):
            s.mesh_texcoords = _p(keep["mesh_texcoords"], _dp); s.mesh_has_texcoords = _p(keep["mesh_has_texcoords"], _u8p)
            s.tri_texcoords = _p(keep["tri_texcoords"], _dp); s.tri_has_texcoords = _p(keep["tri_has_texcoords"], _u8p)
            s.material_texture = _p(keep["material_texture"], _ip); s.material_normal_map = _p(keep["material_normal_map"], _ip)
            s.material_uv_trans = _p(keep["material_uv_trans"], _dp)
            s.n_textures = int(keep["n_textures"]); s.texture_size = _p(keep["texture_size"], _up)
            s.texture_offset = _p(keep["texture_offset"], _u64p); s.texture_rgb = _p(keep["texture_rgb"], _u8p)
        h = C.c_void_p()
        _check(lib().ph_scene_create(C.byref(s), C.byref(h)), "ph_scene_create")
        return Scene(h)

    @staticmethod
    def example(name: str, n: int = 10, assets: str = DEFAULT_ASSETS) -> "Scene":
        h = C.c_void_p()
        cam = np.zeros(10); size = np.zeros(2, dtype=np.uint32)
        _check(lib().ph_example_scene(name.encode(), assets.encode(), n, C.byref(h), _p(cam, _dp), _p(size, _up)), "ph_example_scene")
        return Scene(h, cam, (int(size[0]), int(size[1])))

    def close(self):
        if self._h:
            lib().ph_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def export(self) -> dict:
        """The scene DAG as arrays (layout of the oracle's po_scene)."""
        c = np.zeros(8, dtype=np.uint64)
        _check(lib().ph_scene_counts(self._h, _p(c, _u64p)), "ph_scene_counts")
        n, nch, nm, nv, nmt, nt, nmat, nl = map(int, c)
        a = dict(node_trans=np.zeros((n, 16)), prim_type=np.zeros(n, dtype=np.int32), prim_data=np.zeros(n, dtype=np.int32),
                 prim_flags=np.zeros(n, dtype=np.int32), material=np.zeros(n, dtype=np.int32), child_off=np.zeros(n + 1, dtype=np.uint32),
                 children=np.zeros(nch + 1, dtype=np.uint32), mesh_vert_off=np.zeros(nm + 1, dtype=np.uint64),
                 mesh_tri_off=np.zeros(nm + 1, dtype=np.uint64), mesh_positions=np.zeros((max(nv, 1), 3)), mesh_normals=np.zeros((max(nv, 1), 3)),
                 mesh_has_normals=np.zeros(nm + 1, dtype=np.uint8), mesh_indices=np.zeros((max(nmt, 1), 3), dtype=np.uint32),
                 tri_vertices=np.zeros((max(nt, 1), 9)), tri_normals=np.zeros((max(nt, 1), 9)), tri_has_normals=np.zeros(nt + 1, dtype=np.uint8),
                 materials=np.zeros((max(nmat, 1), 10)), lights=np.zeros((max(nl, 1), 15)), ambient=np.zeros(3))
        root = C.c_uint32(0)
        _check(lib().ph_scene_export(self._h, _p(a["node_trans"], _dp), _p(a["prim_type"], _ip), _p(a["prim_data"], _ip), _p(a["prim_flags"], _ip),
                                     _p(a["material"], _ip), _p(a["child_off"], _up), _p(a["children"], _up), C.byref(root),
                                     _p(a["mesh_vert_off"], _u64p), _p(a["mesh_tri_off"], _u64p), _p(a["mesh_positions"], _dp),
                                     _p(a["mesh_normals"], _dp), _p(a["mesh_has_normals"], _u8p), _p(a["mesh_indices"], _up),
                                     _p(a["tri_vertices"], _dp), _p(a["tri_normals"], _dp), _p(a["tri_has_normals"], _u8p),
                                     _p(a["materials"], _dp), _p(a["lights"], _dp), _p(a["ambient"], _dp)), "ph_scene_export")
        a.update(root=root.value, n_meshes=nm, n_triangles=nt, n_materials=nmat, n_lights=nl)
        tc = np.zeros(2, dtype=np.uint64)
        _check(lib().ph_scene_export_textures(self._h, _p(tc, _u64p), None, None, None, None, None, None, None, None, None, None), "ph_scene_export_textures")
        ntex, nbytes = int(tc[0]), int(tc[1])
        if ntex:
            t = dict(material_texture=np.zeros(max(nmat, 1), dtype=np.int32), material_normal_map=np.zeros(max(nmat, 1), dtype=np.int32),
                     material_uv_trans=np.zeros((max(nmat, 1), 9)), texture_size=np.zeros((ntex, 2), dtype=np.uint32), texture_offset=np.zeros(ntex, dtype=np.uint64),
                     texture_rgb=np.zeros(max(nbytes, 1), dtype=np.uint8), mesh_texcoords=np.zeros((max(nv, 1), 2)), mesh_has_texcoords=np.zeros(nm + 1, dtype=np.uint8),
                     tri_texcoords=np.zeros((max(nt, 1), 6)), tri_has_texcoords=np.zeros(nt + 1, dtype=np.uint8))
            _check(lib().ph_scene_export_textures(self._h, _p(tc, _u64p), _p(t["material_texture"], _ip), _p(t["material_normal_map"], _ip),
                                                  _p(t["material_uv_trans"], _dp), _p(t["texture_size"], _up), _p(t["texture_offset"], _u64p),
                                                  _p(t["texture_rgb"], _u8p), _p(t["mesh_texcoords"], _dp), _p(t["mesh_has_texcoords"], _u8p),
                                                  _p(t["tri_texcoords"], _dp), _p(t["tri_has_texcoords"], _u8p)), "ph_scene_export_textures")
            a.update(t, n_textures=ntex)
        return a

    def same_structure(self, other: "Scene"):
        """Whether `other` is this scene moved - the same flattened nodes in the same order (primitive kinds, meshes / triangles, shading, materials, paths
        through the graph) and as many lights; transforms, lights' values and ambient light may differ - which is what Renderer.update() accepts. Returns a
        value that is true or false and carries the first difference as `.reason` ("" when true). Needs no GPU."""
        why = C.create_string_buffer(512)
        rc = _check(lib().ph_scene_same_structure(self._h, other._h, why, len(why)), "ph_scene_same_structure")
        return SameStructure(rc == 1, why.value.decode())

    def same_topology(self, other: "Scene"):
        """Whether `other` is this scene moved and DEFORMED: same_structure(), except that a mesh may differ in the values of its vertex positions and
        normals (vertex count, triangles, texture coordinates and the presence of normals must be equal) - which is what Renderer.deform() accepts.
        Returns a value like same_structure()'s. Needs no GPU."""
        why = C.create_string_buffer(512)
        rc = _check(lib().ph_scene_same_topology(self._h, other._h, why, len(why)), "ph_scene_same_topology")
        return SameStructure(rc == 1, why.value.decode())

    def flatten(self) -> dict:
        n = _check(lib().ph_scene_flatten(self._h, 0, None, None, None, None, None, None), "ph_scene_flatten")
        tr, inv, nrm = np.zeros((n, 16)), np.zeros((n, 16)), np.zeros((n, 16))
        pt, mat, b = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, 6))
        _check(lib().ph_scene_flatten(self._h, n, _p(tr, _dp), _p(inv, _dp), _p(nrm, _dp), _p(pt, _ip), _p(mat, _ip), _p(b, _dp)), "ph_scene_flatten")
        return dict(trans=tr.reshape(n, 4, 4), invtrans=inv.reshape(n, 4, 4), normal_trans=nrm.reshape(n, 4, 4), prim_type=pt, material=mat, bounds=b)

    def graph(self) -> dict:
        """The ABI-4 scene-graph arrays PT_TRAVERSE_HIER takes (host logic, no GPU needed)."""
        counts = np.zeros(2, dtype=np.uint32)
        n = _check(lib().ph_scene_graph(self._h, 0, 0, 0, None, None, None, None, None, None, _p(counts, _up)), "ph_scene_graph")
        nc, ng = int(counts[0]), int(counts[1])
        off, chain, rank = np.zeros(n + 1, dtype=np.uint32), np.zeros(max(nc, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        tr, inv, nrm = np.zeros((ng, 16)), np.zeros((ng, 16)), np.zeros((ng, 16))
        _check(lib().ph_scene_graph(self._h, n, nc, ng, _p(off, _up), _p(chain, _up), _p(rank, _up), _p(tr, _dp), _p(inv, _dp), _p(nrm, _dp), _p(counts, _up)), "ph_scene_graph")
        return dict(chain_off=off, chain=chain[:nc], dfs_rank=rank[:n], trans=tr.reshape(ng, 4, 4), invtrans=inv.reshape(ng, 4, 4), normal_trans=nrm.reshape(ng, 4, 4))

    def kdtree(self, kd_depth: int = 10, node_cap: int = 1 << 16, item_cap: int = 1 << 20) -> dict:
        axis = np.zeros(node_cap, dtype=np.int32); plane = np.zeros(node_cap)
        front, back, first, count = (np.zeros(node_cap, dtype=np.int32) for _ in range(4))
        items = np.zeros(item_cap, dtype=np.int32)
        n_items = C.c_uint32(0); rb = np.zeros(6); md = C.c_int32(0)
        n = _check(lib().ph_scene_kdtree(self._h, kd_depth, node_cap, item_cap, _p(axis, _ip), _p(plane, _dp), _p(front, _ip), _p(back, _ip),
                                         _p(first, _ip), _p(count, _ip), _p(items, _ip), C.byref(n_items), _p(rb, _dp), C.byref(md)), "ph_scene_kdtree")
        return dict(axis=axis[:n], plane=plane[:n], front=front[:n], back=back[:n], first=first[:n], count=count[:n],
                    items=items[:n_items.value], root_bounds=rb, max_depth=md.value)

    def kdmesh_tree(self, mesh: int, kd_mesh_depth: int = -1, node_cap: int = 1 << 16, item_cap: int = 1 << 20) -> dict:
        """The tree the upload builds for a KDMesh of mesh `mesh` (numbered by first use among the flattened nodes); host logic, no GPU needed."""
        axis = np.zeros(node_cap, dtype=np.int32); plane = np.zeros(node_cap)
        front, back, first, count = (np.zeros(node_cap, dtype=np.int32) for _ in range(4))
        items = np.zeros(item_cap, dtype=np.int32)
        n_items = C.c_uint32(0); rb = np.zeros(6); md = C.c_int32(0)
        n = _check(lib().ph_scene_kdmesh_tree(self._h, mesh, kd_mesh_depth, node_cap, item_cap, _p(axis, _ip), _p(plane, _dp), _p(front, _ip), _p(back, _ip),
                                              _p(first, _ip), _p(count, _ip), _p(items, _ip), C.byref(n_items), _p(rb, _dp), C.byref(md)), "ph_scene_kdmesh_tree")
        return dict(axis=axis[:n], plane=plane[:n], front=front[:n], back=back[:n], first=first[:n], count=count[:n],
                    items=items[:n_items.value], root_bounds=rb, max_depth=md.value)


def camera(cam10, width: float, height: float) -> H.PtCamera:
    out = H.PtCamera()
    c = np.ascontiguousarray(cam10, dtype=np.float64)
    _check(lib().ph_camera(_p(c, _dp), float(width), float(height), C.byref(out)), "ph_camera")
    return out


def load_obj(path: str):
    c = np.zeros(3, dtype=np.uint64)
    _check(lib().ph_obj_load(path.encode(), _p(c, _u64p), None, None, None, 0, 0), "ph_obj_load")
    nv, nt, hn = map(int, c)
    pos, nrm, idx = np.zeros((nv, 3)), np.zeros((nv, 3)), np.zeros((nt, 3), dtype=np.uint32)
    _check(lib().ph_obj_load(path.encode(), _p(c, _u64p), _p(pos, _dp), _p(nrm, _dp), _p(idx, _up), nv, nt), "ph_obj_load")
    return pos, (nrm if hn else None), idx


def sh_basis(directions) -> np.ndarray:
    """The nine real spherical harmonics to order 2 at unit `directions` (..., 3), in probe()'s order: 1, y, z, x, xy, yz, 3 z^2 - 1, xz, x^2 - y^2, each with its
    constant. Plain numpy (the device's own values are the probe contract's: pt_test_probe_host)."""
    d = np.asarray(directions, dtype=np.float64)
    if d.ndim < 1 or d.shape[-1] != 3:
        raise ValueError("directions must be (..., 3), got shape %r" % (d.shape,))
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c0, c1, c2 = 0.5 / np.sqrt(np.pi), np.sqrt(3.0 / (4.0 * np.pi)), np.sqrt(15.0 / (4.0 * np.pi))
    c3, c4 = np.sqrt(5.0 / (16.0 * np.pi)), np.sqrt(15.0 / (16.0 * np.pi))
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3.0 * z * z - 1.0), c2 * x * z, c4 * (x * x - y * y)], axis=-1)


def sh_irradiance(coeffs, normals) -> np.ndarray:
    """Irradiance from order-2 SH radiance coefficients - probe()'s `coeffs`, (..., 9, 3) - at unit `normals` (..., 3), the leading shapes broadcast against
    each other: the coefficients of band l scaled by the cosine lobe's (pi, 2 pi / 3, pi / 4) and the series evaluated at the normal; (..., 3). A constant
    radiance L has coeffs[0] = 2 sqrt(pi) L and the rest zero, and gives pi L for any normal. Numpy only."""
    c = np.asarray(coeffs, dtype=np.float64)
    if c.ndim < 2 or c.shape[-2:] != (9, 3):
        raise ValueError("coeffs must be (..., 9, 3), got shape %r" % (c.shape,))
    lobe = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    return np.sum((sh_basis(normals) * lobe)[..., :, None] * c, axis=-2)


def _device_tensor_pointer(t, shape, device: int, what: str) -> int:
    """The device address of a torch tensor after checking that pt_scene_deform_device can read it as `shape` float64 values on HIP device `device`."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor, got %s" % (what, type(t).__name__))
    if t.dtype != torch.float64:
        raise ValueError("%s must be float64, got %s" % (what, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %r (the mesh's vertex count x 3), got %r" % (what, tuple(shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    if t.device.type != "cuda":
        raise ValueError("%s must be on the renderer's GPU (cuda:%d), got a tensor on %s: use deform() for host data" % (what, device, t.device))
    if t.device.index != device:
        raise ValueError("%s is on %s, the renderer is on cuda:%d" % (what, t.device, device))
    return int(t.data_ptr())


_POINTER = {np.float64: _dp, np.int32: _ip, np.uint32: _up, np.uint8: _u8p}


def _want_names(table, want) -> tuple:
    """`want` as a tuple of names of `table`, a pass's *_BUFFERS"""
    want = tuple(want)
    unknown = [n for n in want if n not in table]
    if unknown or not want:
        raise ValueError("want must name some of %s, got %r" % (", ".join(table), want))
    return want


def _want_buffers(table, struct_type, want, into, shape):
    """What a pass writes into: for every name of `want` the caller's array in `into`, or zeros - of `shape` and the tail `table` (a pass's *_BUFFERS) gives the
    name, as components (1: none) or as a tuple. Returns them by name, and the pass's buffer struct pointed at them."""
    out, b = {}, struct_type()
    for name in _want_names(table, want):
        dtype, tail = table[name]
        if not isinstance(tail, tuple):
            tail = () if tail == 1 else (tail,)
        full = shape + tail
        a = into[name] if into is not None and name in into else np.zeros(full, dtype=dtype)
        if not isinstance(a, np.ndarray) or a.shape != full or a.dtype != dtype or not a.flags.c_contiguous:
            raise ValueError("into[%r] must be a C-contiguous %s array of shape %r" % (name, np.dtype(dtype).name, full))
        out[name] = a
        setattr(b, name, _p(a, _POINTER[dtype]))
    return out, b


def _points_and_normals(points, normals):
    """(n, 3) float64 points and normals, C-contiguous"""
    P, N = np.asarray(points), np.asarray(normals)
    if P.ndim != 2 or P.shape[1] != 3 or P.shape != N.shape:
        raise ValueError("points and normals must both be (n, 3), got %r and %r" % (P.shape, N.shape))
    if P.dtype != np.float64 or N.dtype != np.float64:
        raise ValueError("points and normals must be float64, got %s and %s" % (P.dtype, N.dtype))
    return np.ascontiguousarray(P), np.ascontiguousarray(N)


def _positive_size(width, height):
    for name, v in (("width", width), ("height", height)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError("%s must be a positive integer, got %r" % (name, v))


def _camera_numbers(cam10) -> np.ndarray:
    c = np.ascontiguousarray(cam10, dtype=np.float64)
    if c.shape != (10,):
        raise ValueError("cam10 must hold 10 numbers, got shape %r" % (c.shape,))
    return c


def _uv_on_the_host(method: str, uv):
    """the forms that chain two passes in the library take the chart's UV set from the host"""
    if uv is not None and not isinstance(uv, np.ndarray):
        raise ValueError("%s takes uv as a numpy array or None; chart() takes tensors" % method)


class Lens:
    """What stands in for the pinhole when a film takes samples (Film.add(..., lens=)): made by Lens.thin, Lens.ortho or Lens.fisheye. The rays are a contract
    (pt_film_add_lens): every sample is, to the bit, what Renderer.radiance answers for the ray the contract states."""

    def __init__(self, model: int, aperture: float = 0.0, focus: float = 1.0, extent: float = 1.0):
        self.model, self.aperture, self.focus, self.extent = model, aperture, focus, extent

    @staticmethod
    def _number(name, v, positive):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (0.0 < float(v) if positive else 0.0 <= float(v)) or not float(v) < float("inf"):
            raise ValueError("%s must be a finite number %s 0, got %r" % (name, ">" if positive else ">=", v))
        return float(v)

    @classmethod
    def thin(cls, aperture: float, focus: float) -> "Lens":
        """A thin lens of radius `aperture` (world units; 0 is the pinhole, bit for bit) that is sharp at the distance `focus` along the view axis. The lens
        points of 64 consecutive samples of a pixel are stratified over the disc."""
        return cls(H.LENS_THIN, aperture=cls._number("aperture", aperture, False), focus=cls._number("focus", focus, True))

    @classmethod
    def ortho(cls, half_height: float) -> "Lens":
        """An orthographic view: parallel rays along the view axis from a window of height 2 x half_height (world units) through the eye."""
        return cls(H.LENS_ORTHO, extent=cls._number("half_height", half_height, True))

    @classmethod
    def fisheye(cls, fov_degrees: float) -> "Lens":
        """A stereographic fisheye of `fov_degrees` (0 .. 360, exclusive) across the image height."""
        fov = cls._number("fov_degrees", fov_degrees, True)
        if not fov < 360.0:
            raise ValueError("fov_degrees must be below 360, got %r" % (fov_degrees,))
        return cls(H.LENS_STEREO, extent=math.tan(math.radians(fov) / 4.0))

    def struct(self) -> "H.PtLens":
        """The pt_lens of this lens, checked as pt_film_add_lens checks it."""
        if isinstance(self.model, bool) or self.model not in (H.LENS_THIN, H.LENS_ORTHO, H.LENS_STEREO):
            raise ValueError("lens: unknown model %r" % (self.model,))
        if self.model == H.LENS_THIN:
            self._number("aperture", self.aperture, False)
            self._number("focus", self.focus, True)
        else:
            self._number("extent", self.extent, True)
        return H.PtLens(int(self.model), float(self.aperture), float(self.focus), float(self.extent))


class Film:
    """A width x height accumulator in the renderer's device memory (pt_film_*): add() gives pixels their next samples, resolve() gives at every pixel the
    bits of Renderer.render(samples = that pixel's count) - provided every add used the same camera, background, seed and sample mode and the scene did not
    change in between. Made by Renderer.film(); close it before its renderer."""

    def __init__(self, renderer: "Renderer", width: int, height: int, moments: bool = False):
        for name, v in (("width", width), ("height", height)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 < int(v) < 1 << 32:
                raise ValueError("%s must be a positive integer, got %r" % (name, v))
        self._h = C.c_void_p()
        self._r = renderer
        self.width, self.height = int(width), int(height)
        self.moments = bool(moments)
        if self.moments:
            _check(lib().ph_renderer_film_create_moments(renderer._h, self.width, self.height, C.byref(self._h)), "ph_renderer_film_create_moments")
        else:
            _check(lib().ph_renderer_film_create(renderer._h, self.width, self.height, C.byref(self._h)), "ph_renderer_film_create")

    def close(self):
        if self._h and self._r._h:
            lib().ph_renderer_film_destroy(self._r._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, cam10, background, samples: int = 1, seed: int = 0, sample_mode: int = H.SAMPLE_CENTRE, rect=None, lens: Optional[Lens] = None) -> float:
        """`samples` more samples for every pixel of `rect` (x0, y0, x1, y1 inclusive; default: the whole film), each taken as render() takes that sample of
        that pixel. `background` is (H, 3) or (H, W, 3) as for render(). Returns the device time in ms.
        lens: a Lens (Lens.thin for depth of field, Lens.ortho, Lens.fisheye) whose primary rays replace the pinhole's (pt_film_add_lens); everything behind
        the primary ray, the counts and the fold are the same, and a film may mix lens and plain adds. None is the pinhole."""
        if lens is not None and not isinstance(lens, Lens):
            raise ValueError("lens must be a host.Lens or None, got %r" % (lens,))
        lens_struct = lens.struct() if lens is not None else None
        bg = np.ascontiguousarray(background, dtype=np.float64)
        rows = 1 if bg.shape == (self.height, 3) else 0
        if not rows and bg.shape != (self.height, self.width, 3):
            raise ValueError("background must be (H, 3) or (H, W, 3)")
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 0 < int(samples) <= 1 << 31:
            raise ValueError("samples must be an integer in [1, 2^31], got %r" % (samples,))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, self.width - 1, self.height - 1)
        p = H.PtFilmParams(H.PtRect(x0, y0, x1, y1), int(samples), int(seed), sample_mode, rows)
        c = np.ascontiguousarray(cam10, dtype=np.float64)
        ms = C.c_double(0.0)
        if lens_struct is not None:
            _check(lib().ph_renderer_film_add_lens(self._r._h, self._h, _p(c, _dp), C.byref(lens_struct), _p(bg, _dp), C.byref(p), C.byref(ms)), "ph_renderer_film_add_lens")
            return ms.value
        _check(lib().ph_renderer_film_add(self._r._h, self._h, _p(c, _dp), _p(bg, _dp), C.byref(p), C.byref(ms)), "ph_renderer_film_add")
        return ms.value

    def _background(self, background):
        bg = np.ascontiguousarray(background, dtype=np.float64)
        rows = 1 if bg.shape == (self.height, 3) else 0
        if not rows and bg.shape != (self.height, self.width, 3):
            raise ValueError("background must be (H, 3) or (H, W, 3)")
        return bg, rows

    @staticmethod
    def _integer(name, v, lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
        return int(v)

    def add_map(self, cam10, background, budget, seed: int = 0, sample_mode: int = H.SAMPLE_CENTRE, rect=None, max_samples: Optional[int] = None) -> float:
        """Pixel p of `rect` gets its next min(budget[p], max_samples) samples, each taken as add() takes it: `budget` is an (H, W) uint32 array, of which only
        `rect` is read; max_samples (default: the largest budget inside rect, at most 4096) bounds what any pixel gets. A budget of zeros adds nothing.
        Returns the device time in ms."""
        bg, rows = self._background(background)
        if not isinstance(budget, np.ndarray) or budget.dtype != np.uint32 or budget.shape != (self.height, self.width):
            raise ValueError("budget must be a uint32 array of shape %r" % ((self.height, self.width),))
        b = np.ascontiguousarray(budget)
        seed = self._integer("seed", seed, 0, (1 << 64) - 1)
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, self.width - 1, self.height - 1)
        if max_samples is None:
            inside = b[y0:y1 + 1, x0:x1 + 1] if 0 <= x0 <= x1 < self.width and 0 <= y0 <= y1 < self.height else b[:0]
            max_samples = min(max(int(inside.max()) if inside.size else 1, 1), H.FILM_MAP_MAX)
        max_samples = self._integer("max_samples", max_samples, 1, H.FILM_MAP_MAX)
        p = H.PtFilmMapParams(H.PtRect(x0, y0, x1, y1), max_samples, seed, sample_mode, rows)
        c = np.ascontiguousarray(cam10, dtype=np.float64)
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_film_add_map(self._r._h, self._h, _p(c, _dp), _p(bg, _dp), C.byref(p), _p(b, _up), C.byref(ms)), "ph_renderer_film_add_map")
        return ms.value

    def error(self, into: Optional[np.ndarray] = None) -> np.ndarray:
        """(H, W) float64: the standard error of every pixel's mean (of r + g + b, linear units); +inf where a pixel has fewer than 2 samples. Needs a film
        made with moments=True."""
        if not self.moments:
            raise ValueError("error() needs a film that keeps moments: Renderer.film(w, h, moments=True)")
        err = into if into is not None else np.zeros((self.height, self.width), dtype=np.float64)
        if not isinstance(err, np.ndarray) or err.shape != (self.height, self.width) or err.dtype != np.float64 or not err.flags.c_contiguous:
            raise ValueError("into must be a C-contiguous float64 array of shape %r" % ((self.height, self.width),))
        _check(lib().ph_renderer_film_error(self._r._h, self._h, _p(err, _dp)), "ph_renderer_film_error")
        return err

    def refine(self, cam10, background, threshold: float, min_count: int = 8, max_count: int = 64, step: int = 8, max_passes: int = 64, seed: int = 0,
               sample_mode: int = H.SAMPLE_CENTRE, rect=None) -> dict:
        """The closed loop on the device: every pixel of `rect` is brought to min_count samples, then pixels whose error() is above `threshold` get up to
        `step` more per pass until they fall below it or reach max_count, or max_passes have run. Returns {"passes", "samples", "pixels_left", "kernel_ms"}."""
        if not self.moments:
            raise ValueError("refine() needs a film that keeps moments: Renderer.film(w, h, moments=True)")
        bg, rows = self._background(background)
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or threshold != threshold:
            raise ValueError("threshold must be a number, got %r" % (threshold,))
        step = self._integer("step", step, 1, H.FILM_MAP_MAX)
        max_count = self._integer("max_count", max_count, 0, 1 << 31)
        min_count = self._integer("min_count", min_count, 0, max_count)
        max_passes = self._integer("max_passes", max_passes, 0, (1 << 32) - 1)
        seed = self._integer("seed", seed, 0, (1 << 64) - 1)
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, self.width - 1, self.height - 1)
        sp = H.PtFilmMapParams(H.PtRect(x0, y0, x1, y1), step, seed, sample_mode, rows)
        rp = H.PtFilmRefineParams(H.PtRect(x0, y0, x1, y1), float(threshold), min_count, max_count, step)
        c = np.ascontiguousarray(cam10, dtype=np.float64)
        out = np.zeros(3, dtype=np.uint64)
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_film_refine(self._r._h, self._h, _p(c, _dp), _p(bg, _dp), C.byref(sp), C.byref(rp), max_passes, _p(out, _u64p), C.byref(ms)), "ph_renderer_film_refine")
        return {"passes": int(out[0]), "samples": int(out[1]), "pixels_left": int(out[2]), "kernel_ms": ms.value}

    def resolve(self, want_linear: bool = True, into: Optional[np.ndarray] = None, linear_into: Optional[np.ndarray] = None):
        """(rgb, linear): (H, W, 3) uint8 and (H, W, 3) float64 (None without want_linear). Pixels that have no sample yet keep what `into` / `linear_into`
        hold (zeros when the arrays are made here)."""
        rgb = into if into is not None else np.zeros((self.height, self.width, 3), dtype=np.uint8)
        if not isinstance(rgb, np.ndarray) or rgb.shape != (self.height, self.width, 3) or rgb.dtype != np.uint8 or not rgb.flags.c_contiguous:
            raise ValueError("into must be a C-contiguous uint8 array of shape %r" % ((self.height, self.width, 3),))
        linear = None
        if want_linear or linear_into is not None:
            linear = linear_into if linear_into is not None else np.zeros((self.height, self.width, 3), dtype=np.float64)
            if not isinstance(linear, np.ndarray) or linear.shape != (self.height, self.width, 3) or linear.dtype != np.float64 or not linear.flags.c_contiguous:
                raise ValueError("linear_into must be a C-contiguous float64 array of shape %r" % ((self.height, self.width, 3),))
        _check(lib().ph_renderer_film_resolve(self._r._h, self._h, _p(rgb, _u8p), _p(linear, _dp)), "ph_renderer_film_resolve")
        return rgb, linear

    def denoise(self, cam10, iterations: int = 5, sigma_color: float = 2.0, sigma_plane: float = 0.0, normal_power: Optional[int] = 32, same_node: bool = False,
                want_variance: bool = False, guides: Optional[dict] = None, into: Optional[np.ndarray] = None, linear_into: Optional[np.ndarray] = None,
                variance_into: Optional[np.ndarray] = None, albedo=False):
        """(rgb, linear[, variance]): the film's mean after `iterations` levels of an edge-avoiding a-trous filter (pt_film_denoise) - a lossy read, the film
        itself is not changed and resolve() keeps its promise. The filter is steered by what is under each pixel for camera `cam10` (a primary-visibility
        pass on the device) - or by the caller's `guides`, a dict of "node" (H, W) int32, "normal" and "position" (H, W, 3) float64 as Renderer.aov() returns
        them, of which only what the weights read is needed - and by the film's noise estimate: sigma_color is the colour tolerance in standard errors (0: off;
        a film without moments takes 0 only), sigma_plane the plane-distance tolerance in world units (0: off), normal_power the power of two from 1 to 128
        the clamped dot of the normals is raised to (None: off), same_node=True keeps every tap on the centre's node. variance is (H, W) float64, the filtered
        variance of r + g + b. Pixels without samples keep what `into` / `linear_into` / `variance_into` hold (zeros when the arrays are made here).
        albedo=True filters DEMODULATED colour (pt_film_denoise_albedo): the diffuse colour under each pixel, from one guides pass on the device that also writes
        the guides, is divided out before the levels and multiplied back after them, so texture detail is not blurred. An (H, W, 3) float64 array is the caller's
        albedo, as Renderer.guides() returns it, and needs `guides`. False is the plain filter.
        The guides made here come from a PINHOLE primary-visibility pass: for a film whose samples came through a lens (add(lens=)) supply your own `guides=`
        or leave the filter out."""
        iterations = self._integer("iterations", iterations, 1, 8)
        sig = []
        for name, v in (("sigma_color", sigma_color), ("sigma_plane", sigma_plane)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) < float("inf"):
                raise ValueError("%s must be a finite number >= 0, got %r" % (name, v))
            sig.append(float(v))
        if normal_power is None:
            npl2 = -1
        else:
            if isinstance(normal_power, bool) or not isinstance(normal_power, (int, np.integer)) or int(normal_power) not in (1, 2, 4, 8, 16, 32, 64, 128):
                raise ValueError("normal_power must be a power of two from 1 to 128 or None, got %r" % (normal_power,))
            npl2 = int(normal_power).bit_length() - 1
        if sig[0] > 0.0 and not self.moments:
            raise ValueError("sigma_color > 0 needs a film that keeps moments: Renderer.film(w, h, moments=True)")
        shape3, shape1 = (self.height, self.width, 3), (self.height, self.width)
        alb = None
        if not isinstance(albedo, (bool, np.bool_)):
            if not isinstance(albedo, np.ndarray) or albedo.dtype != np.float64 or albedo.shape != shape3:
                raise ValueError("albedo must be True, False or a float64 array of shape %r" % (shape3,))
            if guides is None:
                raise ValueError("an albedo array needs guides=: the caller's albedo comes with the caller's guides")
            alb = np.ascontiguousarray(albedo)
        elif albedo and guides is not None:
            raise ValueError("albedo=True runs the guides pass on the device: with guides= pass the albedo array too")
        g = None
        if guides is not None:
            if not isinstance(guides, dict):
                raise ValueError("guides must be a dict with 'node' and, where the weights read them, 'normal' and 'position'")
            needed = ["node"] + (["normal"] if npl2 >= 0 or sig[1] > 0.0 else []) + (["position"] if sig[1] > 0.0 else [])
            g, keep = H.PtDenoiseGuides(), []
            for name in needed:
                a = guides.get(name)
                dtype, shape = (np.int32, shape1) if name == "node" else (np.float64, shape3)
                if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape:
                    raise ValueError("guides[%r] must be a %s array of shape %r" % (name, np.dtype(dtype).name, shape))
                a = np.ascontiguousarray(a)
                keep.append(a)
                setattr(g, name, a.ctypes.data)
        out = []
        for name, a, dtype, shape, wanted in (("into", into, np.uint8, shape3, True), ("linear_into", linear_into, np.float64, shape3, True),
                                              ("variance_into", variance_into, np.float64, shape1, want_variance or variance_into is not None)):
            if not wanted:
                out.append(None)
                continue
            a = a if a is not None else np.zeros(shape, dtype=dtype)
            if not isinstance(a, np.ndarray) or a.shape != shape or a.dtype != dtype or not a.flags.c_contiguous:
                raise ValueError("%s must be a C-contiguous %s array of shape %r" % (name, np.dtype(dtype).name, shape))
            out.append(a)
        c = None if cam10 is None else np.ascontiguousarray(cam10, dtype=np.float64)
        if g is None and (c is None or c.shape != (10,)):
            raise ValueError("cam10 must hold the camera's 10 numbers unless guides are given")
        p = H.PtDenoiseParams(iterations, H.DENOISE_SAME_NODE if same_node else 0, sig[0], sig[1], npl2)
        if alb is not None or (isinstance(albedo, (bool, np.bool_)) and albedo):
            _check(lib().ph_renderer_film_denoise_albedo(self._r._h, self._h, _p(c, _dp), C.byref(p), C.byref(g) if g is not None else None, _p(alb, _dp), _p(out[0], _u8p), _p(out[1], _dp),
                                                         _p(out[2], _dp)), "ph_renderer_film_denoise_albedo")
        else:
            _check(lib().ph_renderer_film_denoise(self._r._h, self._h, _p(c, _dp), C.byref(p), C.byref(g) if g is not None else None, _p(out[0], _u8p), _p(out[1], _dp), _p(out[2], _dp)),
                   "ph_renderer_film_denoise")
        return (out[0], out[1], out[2]) if out[2] is not None else (out[0], out[1])

    def counts(self) -> np.ndarray:
        """(H, W) uint32: samples every pixel holds."""
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        _check(lib().ph_renderer_film_counts(self._r._h, self._h, _p(out, _up)), "ph_renderer_film_counts")
        return out

    def reset(self):
        """Every count back to zero: the next add starts at sample 0."""
        _check(lib().ph_renderer_film_reset(self._r._h, self._h), "ph_renderer_film_reset")


class Renderer:
    """A flattened scene resident on one MI355X (what render.rs:121-126 prepares, kept across renders)."""

    def __init__(self, scene: Scene, traverse: int = H.TRAVERSE_FLAT, kd_depth: int = 10, device: int = 0):
        self._h = C.c_void_p()
        self.scene = scene
        self._device = device
        _check(lib().ph_renderer_create(scene._h, traverse, kd_depth, device, C.byref(self._h)), "ph_renderer_create")

    def close(self):
        if self._h:
            lib().ph_renderer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def context(self):
        return lib().ph_renderer_context(self._h)

    @property
    def ranks(self) -> int:
        return int(lib().ph_renderer_ranks(self._h))

    @property
    def node(self):
        """The pt_node behind this renderer when PORTRAYER_GPUS / PORTRAYER_DEVICES spread it over several ranks, else None."""
        return lib().ph_renderer_node(self._h)

    def prepare_ms(self) -> dict:
        out = np.zeros(5)
        _check(lib().ph_renderer_prepare_ms(self._h, _p(out, _dp)), "ph_renderer_prepare_ms")
        return dict(zip(("flatten", "pack_arrays", "context", "kd_build", "upload_and_device_trees"), map(float, out)))

    def render(self, cam10, width: int, height: int, background: np.ndarray, samples: int = 1, seed: int = 0,
               sample_mode: int = H.SAMPLE_CENTRE, rect=None, stats: bool = False, into: Optional[np.ndarray] = None, want_linear: bool = True):
        bg = np.ascontiguousarray(background, dtype=np.float64)
        rows = 1 if bg.shape == (height, 3) else 0
        if not rows and bg.shape != (height, width, 3):
            raise ValueError("background must be (H, 3) or (H, W, 3)")
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, width - 1, height - 1)
        p = H.PtRenderParams(width, height, H.PtRect(x0, y0, x1, y1), samples, seed, sample_mode, rows, 0, 1, 1 if stats else 0)
        rgb = into if into is not None else np.zeros((height, width, 3), dtype=np.uint8)
        linear = np.zeros((height, width, 3), dtype=np.float64) if want_linear else None
        st = H.PtStats()
        c = np.ascontiguousarray(cam10, dtype=np.float64)
        _check(lib().ph_renderer_render(self._h, _p(c, _dp), C.byref(p), _p(bg, _dp), _p(rgb, _u8p), _p(linear, _dp), C.byref(st)), "ph_renderer_render")
        return rgb, linear, st.as_dict()

    def film(self, width: int, height: int, moments: bool = False) -> Film:
        """A film of this renderer (pt_film_create): samples accumulate on the device, add after add; see Film. moments=True (pt_film_create_moments): the
        film also keeps what error() and refine() need."""
        return Film(self, width, height, moments)

    def update(self, scene: Scene):
        """The resident scene moved (pt_scene_update): `scene` must be the renderer's scene with other transforms, lights' values or ambient light
        (Scene.same_structure). Meshes, their trees and textures stay on the device; only the scene-level tree is rebuilt. Every later call answers as
        a new Renderer on `scene` would, bit for bit."""
        _check(lib().ph_renderer_update(self._h, scene._h), "ph_renderer_update")
        self.scene = scene

    def deform(self, scene: Scene, rebuild: bool = False):
        """Resident meshes deformed (pt_scene_deform; on several ranks pt_node_scene_deform): `scene` must be the renderer's scene with other vertex
        positions / normals in its meshes and, as for update(), other transforms, lights' values or ambient light (Scene.same_topology). Only the vertices
        of the meshes that changed go to the device, where their triangle records are expanded and their trees refitted - or, with rebuild=True, rebuilt
        where the device built them at upload. Every later call answers as a new Renderer on `scene` would, bit for bit."""
        _check(lib().ph_renderer_deform(self._h, scene._h, 1 if rebuild else 0), "ph_renderer_deform")
        self.scene = scene

    def mesh_count(self) -> int:
        """Distinct meshes of the renderer's scene; deform_device() numbers them in the order the flattened nodes first use them."""
        return int(_check(lib().ph_renderer_mesh_count(self._h), "ph_renderer_mesh_count"))

    def mesh_vertices(self, m: int) -> int:
        """Vertices of mesh `m` in the renderer's numbering."""
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= int(m) < self.mesh_count():
            raise ValueError("mesh must be an index in [0, %d), got %r" % (self.mesh_count(), m))
        return int(_check(lib().ph_renderer_mesh_vertices(self._h, int(m)), "ph_renderer_mesh_vertices"))

    def deform_device(self, positions: dict, normals: Optional[dict] = None, rebuild: bool = False, moved: Optional[Scene] = None):
        """Resident meshes deformed from vertices that are already on the renderer's GPU (pt_vertex_bounds_device + pt_scene_deform_device): `positions`
        maps a mesh index (the renderer's numbering, see mesh_count()) to a torch tensor - float64, contiguous, of shape (mesh_vertices(m), 3), on the
        renderer's device; `normals` optionally maps some of those indices to tensors of the same kind (meshes uploaded with normals only; without, the
        resident normals stay). Anything else raises ValueError before a library call. Nothing per vertex crosses the bus: the mesh's box is a reduction on
        the device and the triangle records are expanded from the tensor in place. `moved` (optional) is the renderer's scene with other transforms, lights'
        values or ambient light, as for update(). The call is synchronous and waits for all work queued on the device before it reads the tensors, whichever
        torch stream produced them; they are free again when it returns. Every later call answers as after deform() with the same numbers. A mesh deformed this
        way is remembered as posed on the device: a later deform(scene) sends it again whatever the comparison with the host's copy says. Not available with
        the k-d traversal or on a renderer of several ranks (PortrayerHostError says why)."""
        normals = {} if normals is None else normals
        if not isinstance(positions, dict) or not isinstance(normals, dict):
            raise ValueError("positions and normals must be dicts {mesh index: tensor}")
        extra = [m for m in normals if m not in positions]
        if extra:
            raise ValueError("normals for meshes without positions: %r" % (extra,))
        n_meshes = self.mesh_count()
        for m in positions:
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= int(m) < n_meshes:
                raise ValueError("mesh must be an index in [0, %d), got %r" % (n_meshes, m))
        arr = (PhDeviceMesh * max(len(positions), 1))()
        for k, (m, pos) in enumerate(positions.items()):
            shape = (self.mesh_vertices(int(m)), 3)
            arr[k].mesh = int(m)
            arr[k].d_positions = _device_tensor_pointer(pos, shape, self._device, "positions[%d]" % m)
            arr[k].d_normals = _device_tensor_pointer(normals[m], shape, self._device, "normals[%d]" % m) if m in normals else None
        _check(lib().ph_renderer_deform_device(self._h, len(positions), arr, 1 if rebuild else 0, moved._h if moved is not None else None), "ph_renderer_deform_device")
        if moved is not None:
            self.scene = moved

    def aov(self, cam10, width: int, height: int, rect=None, offset=(0.5, 0.5), want=("depth", "position", "normal", "node", "sub", "material"),
            into: Optional[dict] = None) -> dict:
        """What is under each pixel (pt_aov): one primary ray per pixel of `rect` at (x + offset[0], y + offset[1]). Returns the arrays named in
        `want` - (H, W) or (H, W, 3); depth +inf, ids -1, point and normal 0 where nothing is hit - and `kernel_ms`. Buffers not in `want` are not
        computed. Pixels outside `rect` are not written: they keep what `into` (a dict of arrays of the right shape and dtype) holds there; without `into` the
        arrays start zero-filled (so outside `rect` depth is 0.0 and the ids are 0, not the miss values). `material` indexes the Renderer's material table: the
        numbering of Scene.flatten()["material"], materials in the order the flattened nodes first use them (not the order of Scene.export()["materials"])."""
        want = _want_names(H.AOV_BUFFERS, want)
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, width - 1, height - 1)
        p = H.PtAovParams(width, height, H.PtRect(x0, y0, x1, y1), (C.c_double * 2)(float(offset[0]), float(offset[1])))
        out, b = {}, H.PtAovBuffers()
        for name in want:
            dtype, comps = H.AOV_BUFFERS[name]
            shape = (height, width) if comps == 1 else (height, width, comps)
            a = into[name] if into is not None and name in into else np.zeros(shape, dtype=dtype)
            if a.shape != shape or a.dtype != dtype or not a.flags.c_contiguous:
                raise ValueError("into[%r] must be a C-contiguous %s array of shape %r" % (name, np.dtype(dtype).name, shape))
            out[name] = a
            setattr(b, name, _p(a, _dp if dtype is np.float64 else _ip))
        ms = C.c_double(0.0)
        c = np.ascontiguousarray(cam10, dtype=np.float64)
        _check(lib().ph_renderer_aov(self._h, _p(c, _dp), C.byref(p), C.byref(b), C.byref(ms)), "ph_renderer_aov")
        out["kernel_ms"] = ms.value
        return out

    def guides(self, cam10, width: int, height: int, rect=None, offset=(0.5, 0.5), want=("albedo", "position", "normal", "node"), into: Optional[dict] = None) -> dict:
        """What a denoiser needs of each pixel (pt_guides), in one trace: aov()'s `position`, `normal` and `node` - the same bits - and `albedo`, (H, W, 3) float64,
        the diffuse colour at the primary hit (the material's, or its texture's texel as the render path reads it; 0 where nothing is hit). `rect`, `offset`,
        `want` and `into` work as in aov(); returns the arrays named in `want` and `kernel_ms`."""
        want = _want_names(H.GUIDES_BUFFERS, want)
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, width - 1, height - 1)
        p = H.PtAovParams(width, height, H.PtRect(x0, y0, x1, y1), (C.c_double * 2)(float(offset[0]), float(offset[1])))
        out, b = _want_buffers(H.GUIDES_BUFFERS, H.PtGuidesBuffers, want, into, (height, width))
        ms = C.c_double(0.0)
        c = np.ascontiguousarray(cam10, dtype=np.float64)
        _check(lib().ph_renderer_guides(self._h, _p(c, _dp), C.byref(p), C.byref(b), C.byref(ms)), "ph_renderer_guides")
        out["kernel_ms"] = ms.value
        return out

    def rays(self, origins, directions, any_hit: bool = False, reorder: bool = False, want=None, into: Optional[dict] = None, t_max=None) -> dict:
        """Rays of the caller's own (pt_rays): `origins` and `directions` are (n, 3) float64 in world space, directions used as given (t is the ray parameter).
        Returns the arrays named in `want` - (n,) or (n, 3); t +inf, ids -1, point and normal 0, occluded 0 where nothing is hit - and `kernel_ms`.
        `want=None` is every buffer. any_hit=True asks only whether anything is in the way: `want` must then be ("occluded",), which is also what None means there. reorder=True lets the
        device group like rays before tracing; the results are the same bits. `into`: a dict of C-contiguous arrays of the right shape and dtype to write into.
        Rays with a non-finite component, an all-zero direction or a component beyond 1e18 are not traced and report a miss. `material` is numbered as in aov().
        `t_max` (pt_segments): a scalar or an (n,) float64 array, in units of the direction like t; ray i then answers for the segment [EPSILON, t_max[i]) only -
        the nearest hit inside it, or with any_hit whether there is one - and a bound that is NaN or <= EPSILON reports a miss. None is the unbounded pass."""
        want = _want_names(H.RAYS_BUFFERS, (("occluded",) if any_hit else tuple(H.RAYS_BUFFERS)) if want is None else want)
        if any_hit and want != ("occluded",):
            raise ValueError("any_hit=True answers only 'occluded', got want=%r" % (want,))
        o, d = np.asarray(origins), np.asarray(directions)
        if o.ndim != 2 or o.shape[1] != 3 or o.shape != d.shape:
            raise ValueError("origins and directions must both be (n, 3), got %r and %r" % (o.shape, d.shape))
        if o.dtype != np.float64 or d.dtype != np.float64:
            raise ValueError("origins and directions must be float64, got %s and %s" % (o.dtype, d.dtype))
        n = o.shape[0]
        if n > H.RAYS_MAX:
            raise ValueError("at most %d rays per call" % H.RAYS_MAX)
        o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
        if t_max is not None:
            tm = np.asarray(t_max)
            if tm.ndim == 0:
                tm = np.full(n, float(tm), dtype=np.float64)
            if tm.shape != (n,) or tm.dtype != np.float64:
                raise ValueError("t_max must be a scalar or an (n,) float64 array, got %s %r" % (tm.dtype, tm.shape))
            tm = np.ascontiguousarray(tm)
        out, b = {}, H.PtRaysBuffers()
        for name in want:
            dtype, comps = H.RAYS_BUFFERS[name]
            shape = (n,) if comps == 1 else (n, comps)
            a = into[name] if into is not None and name in into else np.zeros(shape, dtype=dtype)
            if a.shape != shape or a.dtype != dtype or not a.flags.c_contiguous:
                raise ValueError("into[%r] must be a C-contiguous %s array of shape %r" % (name, np.dtype(dtype).name, shape))
            out[name] = a
            setattr(b, name, _p(a, _dp if dtype is np.float64 else (_u8p if dtype is np.uint8 else _ip)))
        p = H.PtRaysParams(n, 1 if any_hit else 0, 1 if reorder else 0)
        ms = C.c_double(0.0)
        if t_max is None:
            _check(lib().ph_renderer_rays(self._h, C.byref(p), _p(o, _dp), _p(d, _dp), C.byref(b), C.byref(ms)), "ph_renderer_rays")
        else:
            _check(lib().ph_renderer_segments(self._h, C.byref(p), _p(o, _dp), _p(d, _dp), _p(tm, _dp), C.byref(b), C.byref(ms)), "ph_renderer_segments")
        out["kernel_ms"] = ms.value
        return out

    @staticmethod
    def _ao_params(n, samples, radius, bias, seed, pass_index, first_index, eye):
        """ao()'s and ao_camera()'s argument checks, and the pt_ao_params they describe"""
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or int(samples) not in H.AO_SAMPLES:
            raise ValueError("samples must be one of %r, got %r" % (H.AO_SAMPLES, samples))
        for name, v, top in (("seed", seed, 1 << 64), ("first_index", first_index, 1 << 64), ("pass_index", pass_index, 1 << 32)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < top:
                raise ValueError("%s must be an integer in [0, 2^%d), got %r" % (name, top.bit_length() - 1, v))
        for name, v in (("radius", radius), ("bias", bias)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("%s must be a number, got %r" % (name, v))
        if not float(radius) > 1e-5:  # PT_EPSILON; false for NaN
            raise ValueError("radius must be greater than EPSILON = 1e-5 (inf is allowed), got %r" % (radius,))
        if not np.isfinite(float(bias)) or float(bias) < 0.0:
            raise ValueError("bias must be finite and not negative, got %r" % (bias,))
        if n > H.AO_MAX:
            raise ValueError("at most %d points per call" % H.AO_MAX)
        flags, e = 0, np.zeros(3)
        if eye is not None:
            e = np.asarray(eye, dtype=np.float64)
            if e.shape != (3,) or not np.all(np.isfinite(e)):
                raise ValueError("eye must be three finite numbers, got %r" % (eye,))
            flags = H.AO_FACE_EYE
        return H.PtAoParams(n, int(samples), int(pass_index), int(seed), int(first_index), float(radius), float(bias), flags, (C.c_double * 3)(*e))

    @staticmethod
    def _ao_result(out, samples, ms):
        if "occluded" in out:
            out["visibility"] = 1.0 - out["occluded"].astype(np.float64) / float(samples)  # (1.0 at invalid points: they count no occluder)
        out["kernel_ms"] = ms.value
        return out

    def ao(self, points, normals, samples: int = 16, radius: float = float("inf"), bias: float = 0.0, seed: int = 0, pass_index: int = 0, first_index: int = 0,
           eye=None, want=("occluded",), into: Optional[dict] = None) -> dict:
        """Ambient occlusion at points of the caller's own (pt_ao): `points` and `normals` are (n, 3) float64 in world space - aov()'s position and normal, a
        baker's texel centres. The device makes `samples` (1, 2, 4 .. 64) cosine-weighted rays per point about its normal, in registers, and counts those that
        meet something within `radius` (in world units; inf: anywhere); the origin is lifted by `bias` along the normal. `eye` (three numbers) first turns every
        normal towards that point. Returns the arrays named in `want` - `occluded` (n,) uint32, `valid` (n,) uint8, `bent` (n, 3) float64: the sum of the
        unoccluded directions, not normalised - with `visibility` = 1 - occluded / samples (float64, computed here) where `occluded` was asked for, and
        `kernel_ms`. A point with a non-finite component, one beyond 1e18 or a zero normal is invalid: occluded 0, valid 0, bent 0, visibility 1. Point i draws
        its rotation from the stream (seed, first_index + i, pass_index): a slice [k, k + m) with first_index=k gives that slice of the whole, and another
        pass_index gives other rays to sum. `into`: a dict of C-contiguous arrays of the right shape and dtype to write into."""
        P, N = _points_and_normals(points, normals)
        n = P.shape[0]
        p = self._ao_params(n, samples, radius, bias, seed, pass_index, first_index, eye)
        out, b = _want_buffers(H.AO_BUFFERS, H.PtAoBuffers, want, into, (n,))
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_ao(self._h, C.byref(p), _p(P, _dp), _p(N, _dp), C.byref(b), C.byref(ms)), "ph_renderer_ao")
        return self._ao_result(out, samples, ms)

    def ao_camera(self, cam10, width: int, height: int, samples: int = 16, radius: float = float("inf"), bias: float = 0.0, seed: int = 0, pass_index: int = 0,
                  want=("occluded",), into: Optional[dict] = None) -> dict:
        """Ambient occlusion under every pixel (pt_aov_device then pt_ao_device on the device): the points are what aov() finds at the pixel centres, the normals
        turned towards the camera's eye, pixel (x, y) the stream index y * width + x - the bits of ao(aov's position, aov's normal, eye=the eye). Nothing per
        pixel crosses the bus but the results: arrays of shape (H, W) - `bent` (H, W, 3) - as in ao(); pixels that see nothing are invalid points."""
        _positive_size(width, height)
        p = self._ao_params(int(width) * int(height), samples, radius, bias, seed, pass_index, 0, None)
        out, b = _want_buffers(H.AO_BUFFERS, H.PtAoBuffers, want, into, (int(height), int(width)))
        c = _camera_numbers(cam10)
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_ao_camera(self._h, _p(c, _dp), int(width), int(height), C.byref(p), C.byref(b), C.byref(ms)), "ph_renderer_ao_camera")
        return self._ao_result(out, samples, ms)

    @staticmethod
    def _gather_params(n, background, samples, bias, seed, pass_index, first_index, eye):
        """gather()'s and gather_camera()'s argument checks: the pt_gather_params they describe and the background as three doubles"""
        a = Renderer._ao_params(n, samples, float("inf"), bias, seed, pass_index, first_index, eye)  # (the same checks; a gather ray has no radius)
        bg = np.ascontiguousarray(background, dtype=np.float64)
        if bg.shape != (3,):
            raise ValueError("background must be 3 numbers, got shape %r" % (bg.shape,))
        return H.PtGatherParams(a.n, a.samples, a.pass_index, a.seed, a.first_index, a.bias, a.flags, a.eye), bg

    @staticmethod
    def _gather_result(out, samples, ms):
        if "sum" in out:
            out["mean"] = out["sum"] / float(samples)  # (zeros at invalid points)
        out["kernel_ms"] = ms.value
        return out

    def gather(self, points, normals, background=(0.0, 0.0, 0.0), samples: int = 16, bias: float = 0.0, seed: int = 0, pass_index: int = 0, first_index: int = 0,
               eye=None, want=("sum",), into: Optional[dict] = None) -> dict:
        """Gathered radiance at points of the caller's own (pt_gather): `points` and `normals` are (n, 3) float64 in world space - aov()'s position and normal, a
        baker's texel centres. The device makes ao()'s `samples` (1, 2, 4 .. 64) cosine-weighted rays per point about its normal, in registers, shades each as
        radiance() would - everything render() shades, `background` (three numbers, the sky) for a ray that leaves the scene - and sums them per point; no ray and
        no per-ray colour is ever in memory. The origin is lifted by `bias` along the normal; `eye` (three numbers) first turns every normal towards that point.
        Returns the arrays named in `want` - `sum` (n, 3) float64: the samples added in order, `valid` (n,) uint8 - with `mean` = sum / samples (computed here)
        where `sum` was asked for, and `kernel_ms`. The directions are cosine-weighted, so the irradiance estimate at a point is pi x mean. A point with a
        non-finite component, one beyond 1e18 or a zero normal is invalid: sum 0, valid 0. The bits are those of radiance() on ao()'s rays, flattened point-major,
        with stream_base = first_index * samples and sample = pass_index, summed in order: a slice [k, k + m) with first_index=k gives that slice of the whole, and
        another pass_index gives other rays and draws to sum. `into`: a dict of C-contiguous arrays of the right shape and dtype to write into."""
        P, N = _points_and_normals(points, normals)
        n = P.shape[0]
        p, bg = self._gather_params(n, background, samples, bias, seed, pass_index, first_index, eye)
        out, b = _want_buffers(H.GATHER_BUFFERS, H.PtGatherBuffers, want, into, (n,))
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_gather(self._h, C.byref(p), _p(P, _dp), _p(N, _dp), _p(bg, _dp), C.byref(b), C.byref(ms)), "ph_renderer_gather")
        return self._gather_result(out, samples, ms)

    def gather_camera(self, cam10, width: int, height: int, background=(0.0, 0.0, 0.0), samples: int = 16, bias: float = 0.0, seed: int = 0, pass_index: int = 0,
                      want=("sum",), into: Optional[dict] = None) -> dict:
        """Gathered radiance under every pixel (pt_aov_device then pt_gather_device on the device): the points are what aov() finds at the pixel centres, the
        normals turned towards the camera's eye, pixel (x, y) the stream index y * width + x - the bits of gather(aov's position, aov's normal, eye=the eye).
        Nothing per pixel crosses the bus but the results: `sum` and `mean` (H, W, 3), `valid` (H, W), as in gather(); the irradiance estimate is pi x mean;
        pixels that see nothing are invalid points."""
        _positive_size(width, height)
        p, bg = self._gather_params(int(width) * int(height), background, samples, bias, seed, pass_index, 0, None)
        out, b = _want_buffers(H.GATHER_BUFFERS, H.PtGatherBuffers, want, into, (int(height), int(width)))
        c = _camera_numbers(cam10)
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_gather_camera(self._h, _p(c, _dp), int(width), int(height), C.byref(p), _p(bg, _dp), C.byref(b), C.byref(ms)), "ph_renderer_gather_camera")
        return self._gather_result(out, samples, ms)

    def _chart_node(self, node):
        """chart()'s node check: the flattened node's index, and its mesh's vertex count, triangle count and (T, 3) vertex indices (ph_renderer_chart_mesh)"""
        if isinstance(node, bool) or not isinstance(node, (int, np.integer)) or not 0 <= int(node) < 1 << 32:
            raise ValueError("node must index the flattened nodes (Scene.flatten()), got %r" % (node,))
        counts = np.zeros(2, dtype=np.uint64)
        rc = lib().ph_renderer_chart_mesh(self._h, int(node), _p(counts, _u64p), 0, None)
        if rc == H.ERR_ARGUMENT:
            raise ValueError("node %d: %s" % (int(node), lib().ph_last_error().decode()))
        _check(rc, "ph_renderer_chart_mesh")
        n_verts, n_tris = int(counts[0]), int(counts[1])
        idx = np.zeros((n_tris, 3), dtype=np.uint32)
        if n_tris:
            _check(lib().ph_renderer_chart_mesh(self._h, int(node), _p(counts, _u64p), n_tris, _p(idx, _up)), "ph_renderer_chart_mesh")
        return int(node), n_verts, n_tris, idx

    def _chart_params(self, node, width, height, uv, flip_normal):
        """chart()'s, ao_chart()'s and gather_chart()'s argument checks: the pt_chart_params, and the UV set as a (T, 6) float64 array per corner, a torch tensor
        on the renderer's GPU, or None (the mesh's own texture coordinates)"""
        _positive_size(width, height)
        if int(width) * int(height) > H.AO_MAX:
            raise ValueError("at most %d texels per map" % H.AO_MAX)
        if not isinstance(flip_normal, (bool, np.bool_)):
            raise ValueError("flip_normal must be a bool, got %r" % (flip_normal,))
        node, n_verts, n_tris, idx = self._chart_node(node)
        if uv is not None and not isinstance(uv, np.ndarray) and type(uv).__module__.split(".")[0] == "torch":
            _device_tensor_pointer(uv, tuple(uv.shape) if tuple(uv.shape) in ((n_tris, 6), (n_tris, 3, 2)) else (n_tris, 6), self._device, "uv")
        elif uv is not None:
            uv = np.asarray(uv)
            if uv.dtype != np.float64:
                raise ValueError("uv must be float64, got %s" % uv.dtype)
            if uv.shape == (n_tris, 3, 2) or uv.shape == (n_tris, 6):
                uv = np.ascontiguousarray(uv.reshape(n_tris, 6))
            elif uv.shape == (n_verts, 2):
                uv = np.ascontiguousarray(uv[idx.astype(np.int64)].reshape(n_tris, 6))  # per vertex -> per corner, through the mesh's indices
            else:
                raise ValueError("uv must be (%d, 3, 2) or (%d, 6) per corner or (%d, 2) per vertex, got %r" % (n_tris, n_tris, n_verts, uv.shape))
        return H.PtChartParams(node, int(width), int(height), H.CHART_FLIP_NORMAL if flip_normal else 0), uv

    def chart(self, node: int, width: int, height: int, uv=None, flip_normal: bool = False, want=("position", "normal", "tri", "covered"),
              into: Optional[dict] = None) -> dict:
        """The texels of a mesh's light map as surface points (pt_chart): `node` indexes Scene.flatten()'s nodes (as g["node"] of aov() does) and must be a mesh;
        `uv` is its light-map unwrap - (T, 3, 2) or (T, 6) float64 per triangle corner, or (n_verts, 2) per vertex (expanded here through the mesh's indices), or
        None for the mesh's own texture coordinates (a scene with a textured material only). Texel (x, y) is sampled at its centre, v = 1 at the top row; it
        belongs to the lowest triangle that covers it. Returns the arrays named in `want` - `position` and `normal` (H, W, 3) float64 in world space, from the
        vertices and matrices RESIDENT on the device (after deform(), deform_device() and update(): the new ones), `tri` (H, W) int32 (-1: no triangle),
        `covered` (H, W) uint8 - and `kernel_ms`. Unowned texels hold zeros: invalid points for ao() and gather(). flip_normal negates every normal (the inside
        of a room). `uv` and the arrays of `into` may be torch tensors on the renderer's GPU (float64 / int32 / uint8, contiguous): the pass is then queued on
        torch's current stream (pt_chart_device), waited for, and what `into` does not hold comes back as tensors too."""
        want = _want_names(H.CHART_BUFFERS, want)
        p, uv = self._chart_params(node, width, height, uv, flip_normal)
        shape = (int(height), int(width))
        on_device = (uv is not None and not isinstance(uv, np.ndarray)) or (into is not None and any(not isinstance(into[n], np.ndarray) for n in want if n in into))
        if on_device:
            return self._chart_on_device(p, uv, want, into, shape)
        out, b = _want_buffers(H.CHART_BUFFERS, H.PtChartBuffers, want, into, shape)
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_chart(self._h, C.byref(p), _p(uv, _dp) if uv is not None else None, C.byref(b), C.byref(ms)), "ph_renderer_chart")
        out["kernel_ms"] = ms.value
        return out

    def _chart_on_device(self, p, uv, want, into, shape):
        """chart() with tensors: pt_chart_device on torch's current stream, closed by pt_aov_finish before it returns"""
        import torch
        dev = torch.device("cuda", self._device)
        kinds = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}
        if isinstance(uv, np.ndarray):
            uv = torch.from_numpy(uv).to(dev)
        out, b = {}, H.PtChartBuffers()
        for name in want:
            dtype, comps = H.CHART_BUFFERS[name]
            full = shape if comps == 1 else shape + (comps,)
            t = into[name] if into is not None and name in into else torch.zeros(full, dtype=kinds[dtype], device=dev)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != full or t.dtype != kinds[dtype] or not t.is_contiguous() or t.device != dev:
                raise ValueError("into[%r] must be a contiguous %s tensor of shape %r on %s (all of `into` numpy arrays, or all tensors)" % (name, kinds[dtype], full, dev))
            out[name] = t
            setattr(b, name, C.cast(C.c_void_p(t.data_ptr()), {np.int32: _ip, np.uint8: _u8p, np.float64: _dp}[dtype]))
        ctx, l = self.context, H.lib()
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = l.pt_chart_device(ctx, C.byref(p), C.c_void_p(uv.data_ptr()) if uv is not None else None, C.byref(b), C.c_void_p(stream))
        if rc != H.OK:
            why = l.pt_last_error(ctx).decode()
            if rc == H.ERR_ARGUMENT:
                raise ValueError("pt_chart_device: " + why)
            raise PortrayerHostError("pt_chart_device failed (%d): %s" % (rc, why))
        ms = C.c_double(0.0)
        rc = l.pt_aov_finish(ctx, C.byref(ms))
        if rc != H.OK:
            raise PortrayerHostError("pt_aov_finish failed (%d): %s" % (rc, l.pt_last_error(ctx).decode()))
        out["kernel_ms"] = ms.value
        return out

    def ao_chart(self, node: int, width: int, height: int, uv=None, samples: int = 16, radius: float = float("inf"), bias: float = 0.0, seed: int = 0,
                 pass_index: int = 0, flip_normal: bool = False, want=("occluded",), into: Optional[dict] = None) -> dict:
        """Ambient occlusion at every texel of a mesh's light map (pt_chart_device then pt_ao_device on the device): the bits of
        ao(chart's position, chart's normal, first_index=0, ...), texel (x, y) the stream index y * width + x. Nothing per texel crosses the bus but the results:
        arrays of shape (H, W) - `bent` (H, W, 3) - as in ao(), with `visibility`; texels no triangle owns are invalid points (valid 0, visibility 1). `node`,
        `uv` (numpy, or None) and flip_normal as in chart()."""
        cp, uv = self._chart_params(node, width, height, uv, flip_normal)
        _uv_on_the_host("ao_chart", uv)
        p = self._ao_params(int(width) * int(height), samples, radius, bias, seed, pass_index, 0, None)
        out, b = _want_buffers(H.AO_BUFFERS, H.PtAoBuffers, want, into, (int(height), int(width)))
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_ao_chart(self._h, C.byref(cp), _p(uv, _dp) if uv is not None else None, C.byref(p), C.byref(b), C.byref(ms)), "ph_renderer_ao_chart")
        return self._ao_result(out, samples, ms)

    def gather_chart(self, node: int, width: int, height: int, background=(0.0, 0.0, 0.0), uv=None, samples: int = 16, bias: float = 0.0, seed: int = 0,
                     pass_index: int = 0, flip_normal: bool = False, want=("sum",), into: Optional[dict] = None) -> dict:
        """Gathered radiance at every texel of a mesh's light map (pt_chart_device then pt_gather_device on the device): the bits of
        gather(chart's position, chart's normal, background, first_index=0, ...). `sum` and `mean` (H, W, 3), `valid` (H, W), as in gather(); the irradiance
        estimate is pi x mean; texels no triangle owns are invalid points. `node`, `uv` (numpy, or None) and flip_normal as in chart()."""
        cp, uv = self._chart_params(node, width, height, uv, flip_normal)
        _uv_on_the_host("gather_chart", uv)
        p, bg = self._gather_params(int(width) * int(height), background, samples, bias, seed, pass_index, 0, None)
        out, b = _want_buffers(H.GATHER_BUFFERS, H.PtGatherBuffers, want, into, (int(height), int(width)))
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_gather_chart(self._h, C.byref(cp), _p(uv, _dp) if uv is not None else None, C.byref(p), _p(bg, _dp), C.byref(b), C.byref(ms)),
               "ph_renderer_gather_chart")
        return self._gather_result(out, samples, ms)

    @staticmethod
    def _direct_params(n, samples, bias, seed, pass_index, first_index, eye, to_light):
        """direct()'s, direct_camera()'s and direct_chart()'s argument checks, and the pt_direct_params they describe"""
        if not isinstance(to_light, (bool, np.bool_)):
            raise ValueError("to_light must be a bool, got %r" % (to_light,))
        a = Renderer._ao_params(n, samples, float("inf"), bias, seed, pass_index, first_index, eye)  # (the same checks; a shadow ray has no radius)
        return H.PtDirectParams(a.n, a.samples, a.pass_index, a.seed, a.first_index, a.bias, a.flags | (H.DIRECT_TO_LIGHT if to_light else 0), a.eye)

    @staticmethod
    def _direct_result(out, samples, ms):
        if "sum" in out:
            out["mean"] = out["sum"] / float(samples)  # (zeros at invalid points)
        out["kernel_ms"] = ms.value
        return out

    def direct(self, points, normals, samples: int = 1, bias: float = 0.0, seed: int = 0, pass_index: int = 0, first_index: int = 0, eye=None,
               to_light: bool = False, want=("sum",), into: Optional[dict] = None) -> dict:
        """Direct light at points of the caller's own (pt_direct): `points` and `normals` are (n, 3) float64 in world space - aov()'s or chart()'s position and
        normal. The device makes each point's shadow rays at the lights RESIDENT on the device (after update(): the new ones) in registers - one at a point
        light, `samples` (1, 2, 4 .. 64) at an area light, sampled as render() samples it - walks them as occlusion queries and sums per point what arrives:
        colour x max(cos, 0) / attenuation per light, no material (multiply by guides()'s albedo). The origin is lifted by `bias` along the normal; `eye` (three
        numbers) first turns every normal towards that point. A shadow ray is render()'s, unbounded: anything along it shadows, also behind the light;
        to_light=True ends it at the light, which is what a baker wants. Returns the arrays named in `want` - `sum` (n, 3) float64: a point light's term added
        `samples` times, an area light's samples once each, in order; `lit` (n,) uint32: how many were added; `valid` (n,) uint8 - with `mean` = sum / samples
        (computed here) where `sum` was asked for, and `kernel_ms`. In a scene of point lights only samples=1 is what to ask for. A point with a non-finite
        component, one beyond 1e18 or a zero normal is invalid: sum 0, lit 0, valid 0. Point i draws from the streams (seed, (first_index + i) * samples + k,
        pass_index): a slice [k, k + m) with first_index=k gives that slice of the whole. `into`: a dict of C-contiguous arrays of the right shape and dtype."""
        P, N = _points_and_normals(points, normals)
        n = P.shape[0]
        p = self._direct_params(n, samples, bias, seed, pass_index, first_index, eye, to_light)
        out, b = _want_buffers(H.DIRECT_BUFFERS, H.PtDirectBuffers, want, into, (n,))
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_direct(self._h, C.byref(p), _p(P, _dp), _p(N, _dp), C.byref(b), C.byref(ms)), "ph_renderer_direct")
        return self._direct_result(out, samples, ms)

    def direct_camera(self, cam10, width: int, height: int, samples: int = 1, bias: float = 0.0, seed: int = 0, pass_index: int = 0, to_light: bool = False,
                      want=("sum",), into: Optional[dict] = None) -> dict:
        """Direct light under every pixel (pt_aov_device then pt_direct_device on the device): the points are what aov() finds at the pixel centres, the normals
        turned towards the camera's eye, pixel (x, y) the stream index y * width + x - the bits of direct(aov's position, aov's normal, eye=the eye). Nothing
        per pixel crosses the bus but the results: `sum` and `mean` (H, W, 3), `lit` and `valid` (H, W), as in direct(); pixels that see nothing are invalid
        points."""
        _positive_size(width, height)
        p = self._direct_params(int(width) * int(height), samples, bias, seed, pass_index, 0, None, to_light)
        out, b = _want_buffers(H.DIRECT_BUFFERS, H.PtDirectBuffers, want, into, (int(height), int(width)))
        c = _camera_numbers(cam10)
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_direct_camera(self._h, _p(c, _dp), int(width), int(height), C.byref(p), C.byref(b), C.byref(ms)), "ph_renderer_direct_camera")
        return self._direct_result(out, samples, ms)

    def direct_chart(self, node: int, width: int, height: int, uv=None, samples: int = 1, bias: float = 0.0, seed: int = 0, pass_index: int = 0,
                     to_light: bool = False, flip_normal: bool = False, want=("sum",), into: Optional[dict] = None) -> dict:
        """Direct light at every texel of a mesh's light map (pt_chart_device then pt_direct_device on the device): the bits of
        direct(chart's position, chart's normal, first_index=0, ...), texel (x, y) the stream index y * width + x. `sum` and `mean` (H, W, 3), `lit` and `valid`
        (H, W), as in direct(); texels no triangle owns are invalid points. `node`, `uv` (numpy, or None) and flip_normal as in chart()."""
        cp, uv = self._chart_params(node, width, height, uv, flip_normal)
        _uv_on_the_host("direct_chart", uv)
        p = self._direct_params(int(width) * int(height), samples, bias, seed, pass_index, 0, None, to_light)
        out, b = _want_buffers(H.DIRECT_BUFFERS, H.PtDirectBuffers, want, into, (int(height), int(width)))
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_direct_chart(self._h, C.byref(cp), _p(uv, _dp) if uv is not None else None, C.byref(p), C.byref(b), C.byref(ms)),
               "ph_renderer_direct_chart")
        return self._direct_result(out, samples, ms)

    def probe(self, points, background=(0.0, 0.0, 0.0), samples: int = 256, seed: int = 0, pass_index: int = 0, first_index: int = 0, want=("sh",),
              into: Optional[dict] = None) -> dict:
        """Light probes at points in free space (pt_probe): `points` is (n, 3) float64 in world space, no normals. The device makes `samples` (64, 128, 256, 512
        or 1024) rays per probe, uniform over the whole sphere and turned each probe's own way, in registers, shades each as radiance() would - everything
        render() shades, `background` (three numbers) for a ray that leaves the scene - and sums each colour weighted with the nine order-2 spherical-harmonic
        basis values of its direction; no ray and no per-ray colour is ever in memory. Returns the arrays named in `want` - `sh` (n, 9, 3) float64: the sums,
        `valid` (n,) uint8 - with `coeffs` = sh * 4 pi / samples, the estimate of the radiance's SH coefficients (computed here; sh_irradiance(coeffs, normals)
        lights a surface from them), where `sh` was asked for, and `kernel_ms`. A probe with a non-finite component or one beyond 1e18 is invalid: zeros,
        valid 0. The bits are those of radiance() on the contract's rays (pt_test_probe_host), flattened probe-major, with stream_base = first_index * samples
        and sample = pass_index, weighted and summed in the contract's order: a slice [k, k + m) with first_index=k gives that slice of the whole, and another
        pass_index gives other rays and draws to sum. `into`: a dict of C-contiguous arrays of the right shape and dtype to write into."""
        P = np.asarray(points)
        if P.ndim != 2 or P.shape[1] != 3:
            raise ValueError("points must be (n, 3), got %r" % (P.shape,))
        if P.dtype != np.float64:
            raise ValueError("points must be float64, got %s" % (P.dtype,))
        n = P.shape[0]
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or int(samples) not in H.PROBE_SAMPLES:
            raise ValueError("samples must be one of %r, got %r" % (H.PROBE_SAMPLES, samples))
        for name, v, top in (("seed", seed, 1 << 64), ("first_index", first_index, 1 << 64), ("pass_index", pass_index, 1 << 32)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < top:
                raise ValueError("%s must be an integer in [0, 2^%d), got %r" % (name, top.bit_length() - 1, v))
        if n > H.PROBE_MAX:
            raise ValueError("at most %d probes per call" % H.PROBE_MAX)
        try:
            bg = np.ascontiguousarray(background, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("background must be 3 numbers, got %r" % (background,)) from None
        if bg.shape != (3,):
            raise ValueError("background must be 3 numbers, got shape %r" % (bg.shape,))
        if isinstance(want, str):
            raise ValueError("want must be a sequence of names, got %r" % (want,))
        want = _want_names(H.PROBE_BUFFERS, want)
        if into is not None and not isinstance(into, dict):
            raise ValueError("into must be a dict of arrays, got %s" % type(into).__name__)
        out, b = _want_buffers(H.PROBE_BUFFERS, H.PtProbeBuffers, want, into, (n,))
        p = H.PtProbeParams(n, int(samples), int(pass_index), int(seed), int(first_index))
        P = np.ascontiguousarray(P)
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_probe(self._h, C.byref(p), _p(P, _dp), _p(bg, _dp), C.byref(b), C.byref(ms)), "ph_renderer_probe")
        if "sh" in out:
            out["coeffs"] = out["sh"] * (4.0 * np.pi / float(samples))  # (zeros at invalid probes)
        out["kernel_ms"] = ms.value
        return out

    def probe_grid(self, lo, hi, shape, background=(0.0, 0.0, 0.0), samples: int = 256, seed: int = 0, pass_index: int = 0, first_index: int = 0,
                   want=("sh",)) -> dict:
        """Probes on a regular grid: `shape` = (nx, ny, nz) points from corner `lo` to corner `hi` inclusive along each axis (an axis of one point sits at lo),
        made here in numpy, x slowest and z fastest - probe (i, j, k) has the stream index first_index + (i * ny + j) * nz + k - and handed to probe(). The
        arrays come back reshaped to shape + (9, 3) (`sh`, `coeffs`) and shape (`valid`), with `points` shape + (3,)."""
        lo3, hi3 = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        if lo3.shape != (3,) or hi3.shape != (3,):
            raise ValueError("lo and hi must be three numbers each, got %r and %r" % (lo, hi))
        try:
            dims = tuple(shape)
        except TypeError:
            raise ValueError("shape must be three positive integers, got %r" % (shape,)) from None
        if len(dims) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1 for v in dims):
            raise ValueError("shape must be three positive integers, got %r" % (shape,))
        dims = tuple(int(v) for v in dims)
        axes = [np.linspace(lo3[a], hi3[a], dims[a]) if dims[a] > 1 else lo3[a:a + 1] for a in range(3)]  # (both ends exact)
        pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
        out = self.probe(pts.reshape(-1, 3), background, samples, seed, pass_index, first_index, want)
        for name in list(out):
            if name != "kernel_ms":
                out[name] = out[name].reshape(dims + out[name].shape[1:])
        out["points"] = pts
        return out

    def radiance(self, origins, directions, background=(0.0, 0.0, 0.0), seed: int = 0, sample: int = 0, stream_base: int = 0, reorder: bool = False,
                 into: Optional[np.ndarray] = None) -> dict:
        """Radiance along rays of the caller's own (pt_radiance): `origins` and `directions` are (n, 3) float64 in world space, directions used as given.
        Returns {"rgb": (n, 3) float64, "kernel_ms": float}: per ray one linear sample of what render() shades (shadow rays, area lights, glossy reflection,
        reflection and refraction, textures), no mean, no gamma, no clamp. `background` is one colour (3,) or one per ray (n, 3). Ray i draws its random
        numbers from the stream (seed, stream_base + i, sample): the result depends on neither the order of the batch (reorder=True lets the device group like
        rays first; same bits) nor on how it is cut (a slice [k, k + m) with stream_base=k gives that slice of the whole). With the pixel-centre rays of a
        full image in pixel order it equals render()'s `linear` at samples=1, SAMPLE_CENTRE and the same seed. Rays with a non-finite component, an all-zero
        direction or a component beyond 1e18 are not traced and report their background colour. `into`: a C-contiguous (n, 3) float64 array to write into."""
        o, d = np.asarray(origins), np.asarray(directions)
        if o.ndim != 2 or o.shape[1] != 3 or o.shape != d.shape:
            raise ValueError("origins and directions must both be (n, 3), got %r and %r" % (o.shape, d.shape))
        if o.dtype != np.float64 or d.dtype != np.float64:
            raise ValueError("origins and directions must be float64, got %s and %s" % (o.dtype, d.dtype))
        n = o.shape[0]
        if n > H.RAYS_MAX:
            raise ValueError("at most %d rays per call" % H.RAYS_MAX)
        bg = np.ascontiguousarray(background, dtype=np.float64)
        if bg.shape != (3,) and bg.shape != (n, 3):
            raise ValueError("background must be (3,) or (n, 3) = %r, got %r" % ((n, 3), bg.shape))
        per_ray = 1 if bg.ndim == 2 else 0
        for name, v, top in (("seed", seed, 1 << 64), ("stream_base", stream_base, 1 << 64), ("sample", sample, 1 << 32)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < top:
                raise ValueError("%s must be an integer in [0, 2^%d), got %r" % (name, top.bit_length() - 1, v))
        if not isinstance(reorder, (bool, np.bool_)) and not (isinstance(reorder, (int, np.integer)) and int(reorder) in (0, 1)):
            raise ValueError("reorder is a flag (False or True), got %r" % (reorder,))
        rgb = into if into is not None else np.zeros((n, 3), dtype=np.float64)
        if not isinstance(rgb, np.ndarray) or rgb.shape != (n, 3) or rgb.dtype != np.float64 or not rgb.flags.c_contiguous:
            raise ValueError("into must be a C-contiguous float64 array of shape %r" % ((n, 3),))
        o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
        p = H.PtRadianceParams(n, 1 if reorder else 0, per_ray, int(seed), int(stream_base), int(sample))
        ms = C.c_double(0.0)
        _check(lib().ph_renderer_radiance(self._h, C.byref(p), _p(o, _dp), _p(d, _dp), _p(bg, _dp), _p(rgb, _dp), C.byref(ms)), "ph_renderer_radiance")
        return {"rgb": rgb, "kernel_ms": ms.value}
