"""ctypes binding of libportrayer_hip.so (include/portrayer_hip.h): the gfx950 kernels' C ABI.

There is no CPU fallback: if the shared library is missing or no MI355X is visible the calls fail
loudly (PortrayerHipError)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libportrayer_hip.so")

TRAVERSE_FLAT, TRAVERSE_KD, TRAVERSE_HIER = 1, 2, 3
SAMPLE_CENTRE, SAMPLE_RNG = 0, 1
# the header's error codes (include/portrayer_hip.h: every entry point returns 0 or one of these)
OK, ERR_ARGUMENT, ERR_DEVICE, ERR_NO_SCENE, ERR_SLICE, ERR_SCENE, ERR_TRAVERSAL = 0, -1, -2, -3, -4, -5, -6
# pt_stats.kernel_variant (ABI 6): low four bits = waves per SIMD
KERNEL_WAVES_MASK, KERNEL_INTERPRETER, KERNEL_PARK, KERNEL_COUNTING, KERNEL_TEXTURED, KERNEL_FORK, KERNEL_CHAIN = 15, 16, 32, 64, 128, 256, 512

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)


class PortrayerHipError(RuntimeError):
    pass


class PtScene(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32), ("trans", _dp), ("invtrans", _dp), ("normal_trans", _dp),
        ("prim_type", _ip), ("prim_data", _ip), ("prim_flags", _ip), ("material", _ip),
        ("n_meshes", C.c_uint32), ("mesh_vert_off", _u64p), ("mesh_tri_off", _u64p), ("mesh_positions", _dp),
        ("mesh_normals", _dp), ("mesh_has_normals", _u8p), ("mesh_indices", _up), ("mesh_bounds_invtrans", _dp),
        ("n_triangles", C.c_uint32), ("tri_vertices", _dp), ("tri_normals", _dp),
        ("n_materials", C.c_uint32), ("materials", _dp),
        ("n_lights", C.c_uint32), ("lights", _dp),
        ("ambient", C.c_double * 3),
        ("mesh_texcoords", _dp), ("mesh_has_texcoords", _u8p), ("tri_texcoords", _dp), ("tri_has_texcoords", _u8p),
        ("material_texture", _ip), ("material_normal_map", _ip), ("material_uv_trans", _dp),
        ("n_textures", C.c_uint32), ("texture_size", _up), ("texture_offset", _u64p), ("texture_rgb", _u8p),
        ("mesh_kd_root", _ip), ("mesh_kd_depth", _ip), ("mesh_kd_bounds", _dp), ("mesh_kd_bounds_invtrans", _dp),
        ("n_kdm_nodes", C.c_uint32), ("kdm_axis", _ip), ("kdm_plane", _dp), ("kdm_front", _ip), ("kdm_back", _ip), ("kdm_first", _ip), ("kdm_count", _ip),
        ("n_kdm_items", C.c_uint32), ("kdm_items", _ip),
        # ABI 4: the scene graph, for TRAVERSE_HIER (the reference's default traversal, scene.rs:80-120)
        ("n_graph_nodes", C.c_uint32), ("graph_trans", _dp), ("graph_invtrans", _dp), ("graph_normal_trans", _dp),
        ("node_chain_off", _up), ("node_chain", _up), ("node_dfs_rank", _up),
    ]


class PtKdTree(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32), ("axis", _ip), ("plane", _dp), ("front", _ip), ("back", _ip), ("first", _ip), ("count", _ip),
        ("n_items", C.c_uint32), ("leaf_items", _ip),
        ("root_min", C.c_double * 3), ("root_max", C.c_double * 3), ("max_depth", C.c_int32),
    ]


class PtCamera(C.Structure):
    _fields_ = [("eye", C.c_double * 3), ("view_to_world", C.c_double * 16), ("fov_factor", C.c_double),
                ("aspect_ratio", C.c_double), ("width", C.c_double), ("height", C.c_double)]


class PtRect(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32)]


class PtRenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("slice", PtRect), ("samples", C.c_uint32), ("seed", C.c_uint64),
                ("sample_mode", C.c_int32), ("background_rows", C.c_int32), ("tile_rank", C.c_uint32), ("tile_ranks", C.c_uint32),
                ("collect_stats", C.c_int32)]


class PtSceneTraits(C.Structure):
    """pt_scene_traits: what an uploaded scene says that the choice of its render kernel depends on."""
    _fields_ = [("traverse", C.c_int32), ("n_nodes", C.c_uint32), ("n_lights", C.c_uint32), ("has_meshes", C.c_int32), ("has_kdmesh", C.c_int32),
                ("reflective", C.c_int32), ("reflective_opaque", C.c_int32), ("glossy", C.c_int32), ("area_light", C.c_int32), ("pad", C.c_int32),
                ("instanced_tris", C.c_uint64)]


class PtLaunchQuery(C.Structure):
    """pt_launch_query: what a render launch's plan depends on besides the PORTRAYER_* switches (pt_test_launch_plan)."""
    _fields_ = [("traits", PtSceneTraits), ("mode", C.c_int32), ("textured", C.c_int32), ("stats", C.c_int32), ("n_nodes", C.c_uint32), ("n_lights", C.c_uint32),
                ("stack_cap", C.c_int32), ("n_slots", C.c_uint32), ("n_items", C.c_uint32), ("n_chunks", C.c_uint32), ("k_log2", C.c_uint32), ("c_log2", C.c_uint32),
                ("tiles_x", C.c_uint32), ("tile_ranks", C.c_uint32), ("grid", C.c_uint32)]


# the words of a plan, in the header's order (PT_PLAN_*), and the bits of PLAN_HAS
PLAN_NAMES = ("KERNEL_MODE", "KERNEL_VARIANT", "RUN_VARIANT", "MORE_WAVES", "PARK_SLOTS", "BLOCK_BUDGET", "NEEDS_SPILL", "STACK_LDS_CAP", "GRID_SHARE", "N_LANES", "WORK_DIV",
              "BATCH_MAX", "FINE_QUEUES", "ITEM_STRIDE", "SPILL_BYTES", "STACK_SPILL_BYTES", "MISC_BYTES", "ACCUM_BYTES", "EYE_TAB_BYTES", "DARK_OFF", "DARK_BYTES", "OCC_OFF",
              "OCC_BYTES", "CERTAIN_OFF", "HEADER_OFF", "RECORDS_OFF", "QUEUE_OFF", "HAS", "LIST_CAP", "LIST_PENDING", "OCC_ROW", "OCC_SEED", "OCC_SEED_VALUE", "HEADER_FILL")
for _k, _name in enumerate(PLAN_NAMES):
    globals()["PLAN_" + _name] = _k
PLAN_WORDS = len(PLAN_NAMES)
(PLAN_HAS_OCCLUDERS, PLAN_HAS_EYE_TABLE, PLAN_HAS_CERTAIN_TABLE, PLAN_HAS_DARK_RECORDS, PLAN_HAS_DARK_LIGHTS, PLAN_HAS_LIST_HEADER, PLAN_HAS_PIXEL_LISTS,
 PLAN_HAS_QUEUE) = (1 << k for k in range(8))


class PtAovParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("slice", PtRect), ("offset", C.c_double * 2)]


class PtAovBuffers(C.Structure):
    _fields_ = [("depth", _dp), ("position", _dp), ("normal", _dp), ("node", _ip), ("sub", _ip), ("material", _ip)]


# pt_aov's outputs in the order of pt_aov_buffers: name -> (numpy dtype, components per pixel)
AOV_BUFFERS = {"depth": (np.float64, 1), "position": (np.float64, 3), "normal": (np.float64, 3), "node": (np.int32, 1), "sub": (np.int32, 1), "material": (np.int32, 1)}


class PtGuidesBuffers(C.Structure):
    """pt_guides_buffers: the guides pass's outputs - albedo, position and normal (H, W, 3) f64, node (H, W) i32; each optional."""
    _fields_ = [("albedo", _dp), ("position", _dp), ("normal", _dp), ("node", _ip)]


# pt_guides' outputs in the order of pt_guides_buffers: name -> (numpy dtype, components per pixel)
GUIDES_BUFFERS = {"albedo": (np.float64, 3), "position": (np.float64, 3), "normal": (np.float64, 3), "node": (np.int32, 1)}


class PtSceneMotion(C.Structure):
    """pt_scene_motion: the resident scene's new node matrices (graph matrices in PT_TRAVERSE_HIER), lights and ambient light for pt_scene_update."""
    _fields_ = [("n_nodes", C.c_uint32), ("trans", _dp), ("invtrans", _dp), ("normal_trans", _dp),
                ("n_graph_nodes", C.c_uint32), ("graph_trans", _dp), ("graph_invtrans", _dp), ("graph_normal_trans", _dp),
                ("n_lights", C.c_uint32), ("lights", _dp), ("ambient", _dp)]


class PtMeshDeform(C.Structure):
    """pt_mesh_deform: one resident mesh's new vertex positions (and normals), its new bounds, and whether its tree is refitted or rebuilt."""
    _fields_ = [("mesh", C.c_uint32), ("positions", _dp), ("normals", _dp), ("bounds_invtrans", _dp), ("rebuild", C.c_int32)]


class PtMeshDeformDevice(C.Structure):
    """pt_mesh_deform_device: pt_mesh_deform with the positions (and normals) in DEVICE memory; bounds_invtrans stays a host pointer."""
    _fields_ = [("mesh", C.c_uint32), ("d_positions", C.c_void_p), ("d_normals", C.c_void_p), ("bounds_invtrans", _dp), ("rebuild", C.c_int32)]


class PtRaysParams(C.Structure):
    _fields_ = [("n", C.c_uint64), ("any_hit", C.c_int32), ("reorder", C.c_int32)]


class PtRaysBuffers(C.Structure):
    _fields_ = [("t", _dp), ("position", _dp), ("normal", _dp), ("node", _ip), ("sub", _ip), ("material", _ip), ("occluded", _u8p)]


# pt_rays' outputs in the order of pt_rays_buffers: name -> (numpy dtype, components per ray)
RAYS_BUFFERS = {"t": (np.float64, 1), "position": (np.float64, 3), "normal": (np.float64, 3), "node": (np.int32, 1), "sub": (np.int32, 1), "material": (np.int32, 1),
                "occluded": (np.uint8, 1)}
RAYS_MAX = 1 << 30  # PT_RAYS_MAX


class PtAoParams(C.Structure):
    """pt_ao_params: the points of one ambient-occlusion call and what fixes their rays - samples per point, which rotation (pass, seed, first_index), radius, bias,
    and with AO_FACE_EYE the eye every normal is first turned towards."""
    _fields_ = [("n", C.c_uint64), ("samples", C.c_uint32), ("pass_index", C.c_uint32), ("seed", C.c_uint64), ("first_index", C.c_uint64), ("radius", C.c_double),
                ("bias", C.c_double), ("flags", C.c_uint32), ("eye", C.c_double * 3)]


class PtAoBuffers(C.Structure):
    """pt_ao_buffers: occluded (n,) u32, valid (n,) u8, bent (n, 3) f64; each optional."""
    _fields_ = [("occluded", _up), ("valid", _u8p), ("bent", _dp)]


# pt_ao's outputs in the order of pt_ao_buffers: name -> (numpy dtype, components per point)
AO_BUFFERS = {"occluded": (np.uint32, 1), "valid": (np.uint8, 1), "bent": (np.float64, 3)}
AO_FACE_EYE = 1  # PT_AO_FACE_EYE
AO_MAX = RAYS_MAX // 64  # PT_AO_MAX
AO_SAMPLES = (1, 2, 4, 8, 16, 32, 64)


class PtGatherParams(C.Structure):
    """pt_gather_params: the points of one gather call and what fixes their rays and draws - samples per point, pass, seed, first_index, bias, and with
    AO_FACE_EYE the eye every normal is first turned towards. pt_ao_params without the radius: a gather ray is unbounded."""
    _fields_ = [("n", C.c_uint64), ("samples", C.c_uint32), ("pass_index", C.c_uint32), ("seed", C.c_uint64), ("first_index", C.c_uint64), ("bias", C.c_double),
                ("flags", C.c_uint32), ("eye", C.c_double * 3)]


class PtGatherBuffers(C.Structure):
    """pt_gather_buffers: sum (n, 3) f64, valid (n,) u8; each optional."""
    _fields_ = [("sum", _dp), ("valid", _u8p)]


# pt_gather's outputs in the order of pt_gather_buffers: name -> (numpy dtype, components per point)
GATHER_BUFFERS = {"sum": (np.float64, 3), "valid": (np.uint8, 1)}


class PtProbeParams(C.Structure):
    """pt_probe_params: the probes of one call and what fixes their rays and draws - samples per probe, pass, seed, first_index. No normal, no bias: a probe is a
    point in free space and its rays cover the sphere."""
    _fields_ = [("n", C.c_uint64), ("samples", C.c_uint32), ("pass_index", C.c_uint32), ("seed", C.c_uint64), ("first_index", C.c_uint64)]


class PtProbeBuffers(C.Structure):
    """pt_probe_buffers: sh (n, 9, 3) f64, valid (n,) u8; each optional."""
    _fields_ = [("sh", _dp), ("valid", _u8p)]


# pt_probe's outputs in the order of pt_probe_buffers: name -> (numpy dtype, trailing shape per probe)
PROBE_BUFFERS = {"sh": (np.float64, (9, 3)), "valid": (np.uint8, ())}
PROBE_MAX = RAYS_MAX // 1024  # PT_PROBE_MAX
PROBE_SAMPLES = (64, 128, 256, 512, 1024)


class PtDirectParams(C.Structure):
    """pt_direct_params: the points of one direct-light call and what fixes their shadow rays - samples per area light, pass, seed, first_index, bias, and the
    flags AO_FACE_EYE (with the eye every normal is first turned towards) and DIRECT_TO_LIGHT. pt_ao_params without the radius."""
    _fields_ = [("n", C.c_uint64), ("samples", C.c_uint32), ("pass_index", C.c_uint32), ("seed", C.c_uint64), ("first_index", C.c_uint64), ("bias", C.c_double),
                ("flags", C.c_uint32), ("eye", C.c_double * 3)]


class PtDirectBuffers(C.Structure):
    """pt_direct_buffers: sum (n, 3) f64, lit (n,) u32, valid (n,) u8; each optional."""
    _fields_ = [("sum", _dp), ("lit", _up), ("valid", _u8p)]


# pt_direct's outputs in the order of pt_direct_buffers: name -> (numpy dtype, components per point)
DIRECT_BUFFERS = {"sum": (np.float64, 3), "lit": (np.uint32, 1), "valid": (np.uint8, 1)}
DIRECT_TO_LIGHT = 2  # PT_DIRECT_TO_LIGHT


class PtChartParams(C.Structure):
    """pt_chart_params: the flattened mesh node whose light map is charted, the map's size, CHART_FLIP_NORMAL or 0."""
    _fields_ = [("node", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32)]


class PtChartBuffers(C.Structure):
    """pt_chart_buffers: position and normal (H, W, 3) f64, tri (H, W) i32, covered (H, W) u8; each optional."""
    _fields_ = [("position", _dp), ("normal", _dp), ("tri", _ip), ("covered", _u8p)]


# pt_chart's outputs in the order of pt_chart_buffers: name -> (numpy dtype, components per texel)
CHART_BUFFERS = {"position": (np.float64, 3), "normal": (np.float64, 3), "tri": (np.int32, 1), "covered": (np.uint8, 1)}
CHART_FLIP_NORMAL = 1  # PT_CHART_FLIP_NORMAL


class PtRadianceParams(C.Structure):
    _fields_ = [("n", C.c_uint64), ("reorder", C.c_int32), ("background_per_ray", C.c_int32), ("seed", C.c_uint64), ("stream_base", C.c_uint64), ("sample", C.c_uint32)]


class PtFilmParams(C.Structure):
    """pt_film_params: one add to a film - the slice that gets samples, how many per pixel, and the render's seed, sample mode and background shape."""
    _fields_ = [("slice", PtRect), ("samples", C.c_uint32), ("seed", C.c_uint64), ("sample_mode", C.c_int32), ("background_rows", C.c_int32)]


LENS_THIN, LENS_ORTHO, LENS_STEREO = 0, 1, 2  # PT_LENS_*


class PtLens(C.Structure):
    """pt_lens: what stands in for the pinhole in pt_film_add_lens - a thin lens (aperture, focus), an orthographic or a stereographic camera (extent)."""
    _fields_ = [("model", C.c_int32), ("aperture", C.c_double), ("focus", C.c_double), ("extent", C.c_double)]


FILM_MAP_MAX = 4096  # PT_FILM_MAP_MAX


class PtFilmMapParams(C.Structure):
    """pt_film_map_params: one add with a budget per pixel - the slice, the most any pixel gets, and the render's seed, sample mode and background shape."""
    _fields_ = [("slice", PtRect), ("max_samples", C.c_uint32), ("seed", C.c_uint64), ("sample_mode", C.c_int32), ("background_rows", C.c_int32)]


class PtFilmRefineParams(C.Structure):
    """pt_film_refine_params: what a refine pass gives a pixel - up to `step` samples while it is below min_count, or below max_count with an error above the threshold."""
    _fields_ = [("slice", PtRect), ("threshold", C.c_double), ("min_count", C.c_uint32), ("max_count", C.c_uint32), ("step", C.c_uint32)]


DENOISE_SAME_NODE = 1  # PT_DENOISE_SAME_NODE
DENOISE_ALBEDO_EPS = 0.0078125  # PT_DENOISE_ALBEDO_EPS


class PtDenoiseParams(C.Structure):
    """pt_denoise_params: the levels of the a-trous filter and its three edge-stopping weights (0 / -1 switch one off)."""
    _fields_ = [("iterations", C.c_int32), ("flags", C.c_uint32), ("sigma_color", C.c_double), ("sigma_plane", C.c_double), ("normal_power_log2", C.c_int32)]


class PtDenoiseGuides(C.Structure):
    """pt_denoise_guides: full images laid out as pt_aov writes them - position and normal (H, W, 3) f64, node (H, W) i32; host or device pointers."""
    _fields_ = [("position", C.c_void_p), ("normal", C.c_void_p), ("node", C.c_void_p)]


class PtStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("primary", "shadow", "reflect", "refract", "depth11_skipped", "hits", "n_inner", "n_leaf",
                                          "n_analytic", "n_tri", "n_bbox", "kd_plane_miss", "stack_overflow")] + \
               [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("diag", C.c_uint64 * 8), ("kernel_mode", C.c_uint32), ("kernel_variant", C.c_uint32)]

    def as_dict(self):
        d = {n: (float if n.endswith("_ms") else int)(getattr(self, n)) for n, _ in self._fields_ if n != "diag"}
        d["diag"] = [int(x) for x in self.diag]
        return d


_lib: Optional[C.CDLL] = None

EXPORTS = ["pt_abi_version", "pt_device_count", "pt_context_create", "pt_context_destroy", "pt_last_error", "pt_scene_upload",
           "pt_render", "pt_render_device", "pt_render_finish", "pt_context_stream", "pt_context_next_slot", "pt_compact_bytes", "pt_untile_device", "pt_tile_slot_pixel", "pt_untile_host", "pt_device_alloc",
           "pt_device_free", "pt_copy_to_device", "pt_copy_from_device", "pt_synchronize", "pt_measure_copy_bandwidth", "pt_test_cast_rays",
           "pt_test_math", "pt_test_work_items", "pt_node_create", "pt_node_destroy", "pt_node_last_error", "pt_node_ranks", "pt_node_uses_rccl", "pt_node_context",
           "pt_node_scene_upload", "pt_node_render", "pt_node_upload_background", "pt_node_render_resident", "pt_node_download_image",
           "pt_node_device", "pt_node_frame_begin", "pt_node_frame_end", "pt_node_frames_in_flight", "pt_node_last_frame_host_ms", "pt_node_last_frame_rank_kernel_ms", "pt_test_pow_host", "pt_test_libm_host",
           "pt_aov", "pt_aov_device", "pt_aov_finish", "pt_rays", "pt_rays_device", "pt_rays_finish", "pt_segments", "pt_segments_device",
           "pt_radiance", "pt_radiance_device", "pt_radiance_finish", "pt_scene_update", "pt_node_scene_update", "pt_scene_deform", "pt_node_scene_deform", "pt_scene_mesh_rebuildable", "pt_test_scene_bytes", "pt_test_scene_info",
           "pt_vertex_bounds_device", "pt_scene_deform_device", "pt_test_vertex_box_shape", "pt_test_raypk", "pt_test_certain_shadow", "pt_test_pixel_beam", "pt_test_pixel_list_summary", "pt_test_rect_beam", "pt_test_pixel_list_records",
           "pt_test_pixel_list_queue", "pt_test_background_sum",
           "pt_test_dark_light", "pt_test_dark_lights",
           "pt_film_create", "pt_film_destroy", "pt_film_reset", "pt_film_add", "pt_film_add_device", "pt_film_resolve", "pt_film_resolve_device", "pt_film_counts",
           "pt_test_film_fold_host",
           "pt_film_create_moments", "pt_film_add_map", "pt_film_add_map_device", "pt_film_error", "pt_film_error_device", "pt_film_budget_device",
           "pt_test_film_moments_host", "pt_test_film_plan_host", "pt_test_film_plan",
           "pt_film_denoise", "pt_film_denoise_device", "pt_test_denoise_host",
           "pt_guides", "pt_guides_device", "pt_guides_finish", "pt_film_denoise_albedo", "pt_film_denoise_albedo_device", "pt_test_denoise_albedo_host",
           "pt_ao", "pt_ao_device", "pt_ao_finish", "pt_test_ao_rays_host", "pt_test_ao_tables",
           "pt_gather", "pt_gather_device", "pt_gather_finish", "pt_test_kernel_choice", "pt_test_launch_plan",
           "pt_chart_triangles", "pt_chart", "pt_chart_device", "pt_test_chart_host",
           "pt_direct", "pt_direct_device", "pt_direct_finish", "pt_test_direct_host",
           "pt_probe", "pt_probe_device", "pt_probe_finish", "pt_test_probe_host", "pt_test_probe_tables",
           "pt_film_add_lens", "pt_film_add_lens_device", "pt_test_lens_rays_host"]


def header_functions():
    """Names of the functions include/portrayer_hip.h declares (every `pt_*(` outside comments)."""
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", text)))


def missing_symbols():
    """Functions the header declares that the loaded library does not export (must be empty)."""
    l = lib()
    return [n for n in header_functions() if not hasattr(l, n)]


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PortrayerHipError(f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()); there is no CPU fallback")
        l = C.CDLL(LIB_PATH)
        l.pt_abi_version.restype = C.c_int
        l.pt_device_count.restype = C.c_int
        l.pt_context_create.restype = C.c_int
        l.pt_context_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        l.pt_context_destroy.restype = None
        l.pt_context_destroy.argtypes = [C.c_void_p]
        l.pt_last_error.restype = C.c_char_p
        l.pt_last_error.argtypes = [C.c_void_p]
        l.pt_scene_upload.restype = C.c_int
        l.pt_scene_upload.argtypes = [C.c_void_p, C.POINTER(PtScene), C.c_int, C.POINTER(PtKdTree)]
        l.pt_scene_update.restype = C.c_int
        l.pt_scene_update.argtypes = [C.c_void_p, C.POINTER(PtSceneMotion), C.POINTER(PtKdTree)]
        l.pt_node_scene_update.restype = C.c_int
        l.pt_node_scene_update.argtypes = [C.c_void_p, C.POINTER(PtSceneMotion), C.POINTER(PtKdTree)]
        l.pt_scene_deform.restype = C.c_int
        l.pt_scene_deform.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(PtMeshDeform), C.POINTER(PtSceneMotion), C.POINTER(PtKdTree)]
        l.pt_node_scene_deform.restype = C.c_int
        l.pt_node_scene_deform.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(PtMeshDeform), C.POINTER(PtSceneMotion), C.POINTER(PtKdTree)]
        l.pt_scene_mesh_rebuildable.restype = C.c_int
        l.pt_scene_mesh_rebuildable.argtypes = [C.c_void_p, C.c_uint32]
        l.pt_vertex_bounds_device.restype = C.c_int
        l.pt_vertex_bounds_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, _dp, _u64p]
        l.pt_scene_deform_device.restype = C.c_int
        l.pt_scene_deform_device.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(PtMeshDeformDevice), C.POINTER(PtSceneMotion), C.POINTER(PtKdTree)]
        l.pt_test_vertex_box_shape.restype = C.c_int
        l.pt_test_vertex_box_shape.argtypes = [C.c_void_p, C.POINTER(C.c_uint64 * 2)]
        l.pt_test_scene_bytes.restype = C.c_uint64
        l.pt_test_scene_bytes.argtypes = [C.c_void_p]
        l.pt_test_scene_info.restype = C.c_int
        l.pt_test_scene_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64 * 4)]
        l.pt_render.restype = C.c_int
        l.pt_render.argtypes = [C.c_void_p, C.POINTER(PtCamera), _dp, C.POINTER(PtRenderParams), _u8p, _dp, C.POINTER(PtStats)]
        l.pt_render_device.restype = C.c_int
        l.pt_render_device.argtypes = [C.c_void_p, C.POINTER(PtCamera), C.c_void_p, C.POINTER(PtRenderParams), C.c_int, C.c_void_p, C.c_void_p]
        l.pt_render_finish.restype = C.c_int
        l.pt_render_finish.argtypes = [C.c_void_p, C.POINTER(PtStats)]
        l.pt_context_stream.restype = C.c_void_p
        l.pt_context_stream.argtypes = [C.c_void_p, C.c_int]
        l.pt_context_next_slot.restype = C.c_int
        l.pt_context_next_slot.argtypes = [C.c_void_p]
        l.pt_compact_bytes.restype = C.c_uint64
        l.pt_compact_bytes.argtypes = [C.POINTER(PtRenderParams)]
        l.pt_untile_device.restype = C.c_int
        l.pt_untile_device.argtypes = [C.c_void_p, C.POINTER(PtRenderParams), C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_tile_slot_pixel.restype = C.c_int
        l.pt_tile_slot_pixel.argtypes = [C.POINTER(PtRenderParams), C.c_uint32, C.c_uint32, _up, _up]
        l.pt_untile_host.restype = C.c_int
        l.pt_untile_host.argtypes = [C.POINTER(PtRenderParams), _u8p, _u8p]
        l.pt_device_alloc.restype = C.c_int
        l.pt_device_alloc.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        l.pt_device_free.restype = C.c_int
        l.pt_device_free.argtypes = [C.c_void_p, C.c_void_p]
        l.pt_copy_to_device.restype = C.c_int
        l.pt_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        l.pt_copy_from_device.restype = C.c_int
        l.pt_copy_from_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        l.pt_synchronize.restype = C.c_int
        l.pt_synchronize.argtypes = [C.c_void_p]
        l.pt_measure_copy_bandwidth.restype = C.c_int
        l.pt_measure_copy_bandwidth.argtypes = [C.c_void_p, C.c_uint64, C.c_int, _dp]
        l.pt_test_cast_rays.restype = C.c_int
        l.pt_test_cast_rays.argtypes = [C.c_void_p, C.c_uint64, _dp, _dp, C.c_int, _dp, _ip, _ip]
        l.pt_test_work_items.restype = C.c_int
        l.pt_test_work_items.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        l.pt_test_certain_shadow.restype = C.c_int
        l.pt_test_certain_shadow.argtypes = [C.c_uint64, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip]
        l.pt_test_dark_light.restype = C.c_int
        l.pt_test_dark_light.argtypes = [C.c_uint64, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip]
        l.pt_test_dark_lights.restype = C.c_int
        l.pt_test_dark_lights.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64)]
        l.pt_test_raypk.restype = C.c_int
        l.pt_test_raypk.argtypes = [C.c_uint64, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_float), C.POINTER(C.c_float), _ip, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        l.pt_test_launch_plan.restype = C.c_int
        l.pt_test_launch_plan.argtypes = [C.POINTER(PtLaunchQuery), _u64p, C.c_char_p, C.c_uint64]
        l.pt_test_pixel_list_summary.restype = C.c_int
        l.pt_test_pixel_list_summary.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        l.pt_test_pixel_beam.restype = C.c_int
        l.pt_test_pixel_beam.argtypes = [C.c_uint64, _dp, C.POINTER(C.c_uint32), _dp, C.POINTER(C.c_float), C.POINTER(C.c_float), _ip, C.POINTER(C.c_float), _ip, _dp]
        l.pt_test_rect_beam.restype = C.c_int
        l.pt_test_rect_beam.argtypes = l.pt_test_pixel_beam.argtypes
        l.pt_test_pixel_list_records.restype = C.c_int
        l.pt_test_pixel_list_records.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64)]
        l.pt_test_pixel_list_queue.restype = C.c_int
        l.pt_test_pixel_list_queue.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64)]
        l.pt_test_background_sum.restype = C.c_int
        l.pt_test_background_sum.argtypes = [_dp, C.c_uint32, _dp]
        l.pt_test_math.restype = C.c_int
        l.pt_test_math.argtypes = [C.c_void_p, C.c_int, C.c_uint64, _dp, _dp, _dp]
        l.pt_node_create.restype = C.c_int
        l.pt_node_create.argtypes = [C.c_int, _ip, C.POINTER(C.c_void_p)]
        l.pt_node_destroy.restype = None
        l.pt_node_destroy.argtypes = [C.c_void_p]
        l.pt_node_last_error.restype = C.c_char_p
        l.pt_node_last_error.argtypes = [C.c_void_p]
        l.pt_node_ranks.restype = C.c_int
        l.pt_node_ranks.argtypes = [C.c_void_p]
        l.pt_node_uses_rccl.restype = C.c_int
        l.pt_node_uses_rccl.argtypes = [C.c_void_p]
        l.pt_node_context.restype = C.c_void_p
        l.pt_node_context.argtypes = [C.c_void_p, C.c_int]
        l.pt_node_scene_upload.restype = C.c_int
        l.pt_node_scene_upload.argtypes = [C.c_void_p, C.POINTER(PtScene), C.c_int, C.POINTER(PtKdTree)]
        l.pt_node_render.restype = C.c_int
        l.pt_node_render.argtypes = [C.c_void_p, C.POINTER(PtCamera), _dp, C.POINTER(PtRenderParams), _u8p, C.POINTER(PtStats)]
        l.pt_node_upload_background.restype = C.c_int
        l.pt_node_upload_background.argtypes = [C.c_void_p, _dp, C.POINTER(PtRenderParams), _u8p]
        l.pt_node_render_resident.restype = C.c_int
        l.pt_node_render_resident.argtypes = [C.c_void_p, C.POINTER(PtCamera), C.POINTER(PtRenderParams), C.POINTER(PtStats)]
        l.pt_node_download_image.restype = C.c_int
        l.pt_node_download_image.argtypes = [C.c_void_p, C.POINTER(PtRenderParams), _u8p]
        l.pt_node_device.restype = C.c_int
        l.pt_node_device.argtypes = [C.c_void_p, C.c_int]
        l.pt_node_frame_begin.restype = C.c_int
        l.pt_node_frame_begin.argtypes = [C.c_void_p, C.POINTER(PtCamera), C.POINTER(PtRenderParams)]
        l.pt_node_frame_end.restype = C.c_int
        l.pt_node_frame_end.argtypes = [C.c_void_p, C.POINTER(PtStats)]
        l.pt_node_frames_in_flight.restype = C.c_int
        l.pt_node_frames_in_flight.argtypes = [C.c_void_p]
        l.pt_node_last_frame_host_ms.restype = C.c_int
        l.pt_node_last_frame_host_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double * 5)]
        l.pt_node_last_frame_rank_kernel_ms.restype = C.c_int
        l.pt_node_last_frame_rank_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        l.pt_test_pow_host.restype = C.c_int
        l.pt_test_pow_host.argtypes = [C.c_uint64, _dp, _dp, _dp, _dp]
        l.pt_test_libm_host.restype = C.c_int
        l.pt_test_libm_host.argtypes = [C.c_int, C.c_uint64, _dp, _dp, _dp]
        l.pt_aov.restype = C.c_int
        l.pt_aov.argtypes = [C.c_void_p, C.POINTER(PtCamera), C.POINTER(PtAovParams), C.POINTER(PtAovBuffers), _dp]
        l.pt_aov_device.restype = C.c_int
        l.pt_aov_device.argtypes = [C.c_void_p, C.POINTER(PtCamera), C.POINTER(PtAovParams), C.POINTER(PtAovBuffers), C.c_void_p]
        l.pt_aov_finish.restype = C.c_int
        l.pt_aov_finish.argtypes = [C.c_void_p, _dp]
        l.pt_guides.restype = C.c_int
        l.pt_guides.argtypes = [C.c_void_p, C.POINTER(PtCamera), C.POINTER(PtAovParams), C.POINTER(PtGuidesBuffers), _dp]
        l.pt_guides_device.restype = C.c_int
        l.pt_guides_device.argtypes = [C.c_void_p, C.POINTER(PtCamera), C.POINTER(PtAovParams), C.POINTER(PtGuidesBuffers), C.c_void_p]
        l.pt_guides_finish.restype = C.c_int
        l.pt_guides_finish.argtypes = [C.c_void_p, _dp]
        l.pt_rays.restype = C.c_int
        l.pt_rays.argtypes = [C.c_void_p, C.POINTER(PtRaysParams), _dp, _dp, C.POINTER(PtRaysBuffers), _dp]
        l.pt_rays_device.restype = C.c_int
        l.pt_rays_device.argtypes = [C.c_void_p, C.POINTER(PtRaysParams), C.c_void_p, C.c_void_p, C.POINTER(PtRaysBuffers), C.c_void_p]
        l.pt_segments.restype = C.c_int
        l.pt_segments.argtypes = [C.c_void_p, C.POINTER(PtRaysParams), _dp, _dp, _dp, C.POINTER(PtRaysBuffers), _dp]
        l.pt_segments_device.restype = C.c_int
        l.pt_segments_device.argtypes = [C.c_void_p, C.POINTER(PtRaysParams), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PtRaysBuffers), C.c_void_p]
        l.pt_rays_finish.restype = C.c_int
        l.pt_rays_finish.argtypes = [C.c_void_p, _dp]
        l.pt_ao.restype = C.c_int
        l.pt_ao.argtypes = [C.c_void_p, C.POINTER(PtAoParams), _dp, _dp, C.POINTER(PtAoBuffers), _dp]
        l.pt_ao_device.restype = C.c_int
        l.pt_ao_device.argtypes = [C.c_void_p, C.POINTER(PtAoParams), C.c_void_p, C.c_void_p, C.POINTER(PtAoBuffers), C.c_void_p]
        l.pt_ao_finish.restype = C.c_int
        l.pt_ao_finish.argtypes = [C.c_void_p, _dp]
        l.pt_test_ao_rays_host.restype = C.c_int
        l.pt_test_ao_rays_host.argtypes = [C.c_uint64, C.POINTER(PtAoParams), _dp, _dp, _dp, _dp, _u8p]
        l.pt_test_ao_tables.restype = C.c_int
        l.pt_test_ao_tables.argtypes = [_dp, _dp]
        l.pt_gather.restype = C.c_int
        l.pt_gather.argtypes = [C.c_void_p, C.POINTER(PtGatherParams), _dp, _dp, _dp, C.POINTER(PtGatherBuffers), _dp]
        l.pt_gather_device.restype = C.c_int
        l.pt_gather_device.argtypes = [C.c_void_p, C.POINTER(PtGatherParams), C.c_void_p, C.c_void_p, _dp, C.POINTER(PtGatherBuffers), C.c_void_p]
        l.pt_gather_finish.restype = C.c_int
        l.pt_gather_finish.argtypes = [C.c_void_p, _dp]
        l.pt_direct.restype = C.c_int
        l.pt_direct.argtypes = [C.c_void_p, C.POINTER(PtDirectParams), _dp, _dp, C.POINTER(PtDirectBuffers), _dp]
        l.pt_direct_device.restype = C.c_int
        l.pt_direct_device.argtypes = [C.c_void_p, C.POINTER(PtDirectParams), C.c_void_p, C.c_void_p, C.POINTER(PtDirectBuffers), C.c_void_p]
        l.pt_direct_finish.restype = C.c_int
        l.pt_direct_finish.argtypes = [C.c_void_p, _dp]
        l.pt_probe.restype = C.c_int
        l.pt_probe.argtypes = [C.c_void_p, C.POINTER(PtProbeParams), _dp, _dp, C.POINTER(PtProbeBuffers), _dp]
        l.pt_probe_device.restype = C.c_int
        l.pt_probe_device.argtypes = [C.c_void_p, C.POINTER(PtProbeParams), C.c_void_p, _dp, C.POINTER(PtProbeBuffers), C.c_void_p]
        l.pt_probe_finish.restype = C.c_int
        l.pt_probe_finish.argtypes = [C.c_void_p, _dp]
        l.pt_test_probe_host.restype = C.c_int
        l.pt_test_probe_host.argtypes = [C.c_uint64, C.POINTER(PtProbeParams), _dp, _dp, _dp, _dp, _u8p]
        l.pt_test_probe_tables.restype = C.c_int
        l.pt_test_probe_tables.argtypes = [_dp, _dp]
        l.pt_test_direct_host.restype = C.c_int
        l.pt_test_direct_host.argtypes = [C.c_uint64, C.POINTER(PtDirectParams), _dp, _dp, C.c_uint32, _dp, _dp, _dp, _dp, _dp, _u8p]
        l.pt_chart_triangles.restype = C.c_int
        l.pt_chart_triangles.argtypes = [C.c_void_p, C.c_uint32, _u64p]
        l.pt_chart.restype = C.c_int
        l.pt_chart.argtypes = [C.c_void_p, C.POINTER(PtChartParams), _dp, C.POINTER(PtChartBuffers), _dp]
        l.pt_chart_device.restype = C.c_int
        l.pt_chart_device.argtypes = [C.c_void_p, C.POINTER(PtChartParams), C.c_void_p, C.POINTER(PtChartBuffers), C.c_void_p]
        l.pt_test_chart_host.restype = C.c_int
        l.pt_test_chart_host.argtypes = [_dp, _dp, C.c_uint64, _dp, _dp, _dp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PtChartBuffers)]
        l.pt_radiance.restype = C.c_int
        l.pt_radiance.argtypes = [C.c_void_p, C.POINTER(PtRadianceParams), _dp, _dp, _dp, _dp, _dp]
        l.pt_radiance_device.restype = C.c_int
        l.pt_radiance_device.argtypes = [C.c_void_p, C.POINTER(PtRadianceParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_radiance_finish.restype = C.c_int
        l.pt_radiance_finish.argtypes = [C.c_void_p, _dp]
        l.pt_film_create.restype = C.c_int
        l.pt_film_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        for name in ("pt_film_destroy", "pt_film_reset"):
            getattr(l, name).restype = C.c_int
            getattr(l, name).argtypes = [C.c_void_p, C.c_void_p]
        l.pt_film_add.restype = C.c_int
        l.pt_film_add.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtCamera), _dp, C.POINTER(PtFilmParams), _dp]
        l.pt_film_add_device.restype = C.c_int
        l.pt_film_add_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtCamera), C.c_void_p, C.POINTER(PtFilmParams), C.c_void_p]
        l.pt_film_add_lens.restype = C.c_int
        l.pt_film_add_lens.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtCamera), C.POINTER(PtLens), _dp, C.POINTER(PtFilmParams), _dp]
        l.pt_film_add_lens_device.restype = C.c_int
        l.pt_film_add_lens_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtCamera), C.POINTER(PtLens), C.c_void_p, C.POINTER(PtFilmParams), C.c_void_p]
        l.pt_test_lens_rays_host.restype = C.c_int
        l.pt_test_lens_rays_host.argtypes = [C.POINTER(PtCamera), C.POINTER(PtLens), C.c_uint32, C.c_uint32, C.c_uint64, C.c_int32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _dp, _dp]
        l.pt_film_resolve.restype = C.c_int
        l.pt_film_resolve.argtypes = [C.c_void_p, C.c_void_p, _u8p, _dp]
        l.pt_film_resolve_device.restype = C.c_int
        l.pt_film_resolve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_film_counts.restype = C.c_int
        l.pt_film_counts.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        l.pt_test_film_fold_host.restype = C.c_int
        l.pt_test_film_fold_host.argtypes = [C.c_uint32, _dp, C.POINTER(C.c_uint32), C.c_uint32, _dp]
        _u32p = C.POINTER(C.c_uint32)
        l.pt_film_create_moments.restype = C.c_int
        l.pt_film_create_moments.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        l.pt_film_add_map.restype = C.c_int
        l.pt_film_add_map.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtCamera), _dp, C.POINTER(PtFilmMapParams), _u32p, _dp]
        l.pt_film_add_map_device.restype = C.c_int
        l.pt_film_add_map_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtCamera), C.c_void_p, C.POINTER(PtFilmMapParams), C.c_void_p, C.c_void_p]
        l.pt_film_error.restype = C.c_int
        l.pt_film_error.argtypes = [C.c_void_p, C.c_void_p, _dp]
        l.pt_film_error_device.restype = C.c_int
        l.pt_film_error_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_film_budget_device.restype = C.c_int
        l.pt_film_budget_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtFilmRefineParams), C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_test_film_moments_host.restype = C.c_int
        l.pt_test_film_moments_host.argtypes = [C.c_uint32, _dp, _u32p, C.c_uint32, _dp, _dp, _dp]
        l.pt_test_film_plan_host.restype = C.c_int
        l.pt_test_film_plan_host.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(PtRect), _u32p, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _u32p]
        l.pt_film_denoise.restype = C.c_int
        l.pt_film_denoise.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtDenoiseParams), C.POINTER(PtDenoiseGuides), _u8p, _dp, _dp]
        l.pt_film_denoise_device.restype = C.c_int
        l.pt_film_denoise_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtDenoiseParams), C.POINTER(PtDenoiseGuides), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_test_denoise_host.restype = C.c_int
        l.pt_test_denoise_host.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(PtDenoiseParams), _dp, _dp, _u32p, C.POINTER(PtDenoiseGuides), _dp, _dp]
        l.pt_film_denoise_albedo.restype = C.c_int
        l.pt_film_denoise_albedo.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtDenoiseParams), C.POINTER(PtDenoiseGuides), _dp, _u8p, _dp, _dp]
        l.pt_film_denoise_albedo_device.restype = C.c_int
        l.pt_film_denoise_albedo_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PtDenoiseParams), C.POINTER(PtDenoiseGuides), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.pt_test_denoise_albedo_host.restype = C.c_int
        l.pt_test_denoise_albedo_host.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(PtDenoiseParams), _dp, _dp, _u32p, C.POINTER(PtDenoiseGuides), _dp, _dp, _dp]
        l.pt_test_film_plan.restype = C.c_int
        l.pt_test_film_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PtRect), _u32p, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _u32p]
        _lib = l
    return _lib


def _p(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


class Context:
    """One pt_context (one GPU)."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        rc = lib().pt_context_create(device, C.byref(self._h))
        if rc != 0:
            raise PortrayerHipError(f"pt_context_create(device={device}) failed with {rc}: no usable MI355X (there is no CPU fallback)")

    def close(self):
        if self._h:
            lib().pt_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int, what: str):
        if rc != 0:
            raise PortrayerHipError(f"{what} failed with {rc}: {lib().pt_last_error(self._h).decode()}")

    @property
    def handle(self):
        return self._h

    def upload(self, scene: PtScene, traverse: int, kd: Optional[PtKdTree] = None):
        self.check(lib().pt_scene_upload(self._h, C.byref(scene), traverse, C.byref(kd) if kd is not None else None), "pt_scene_upload")

    def update(self, motion: "PtSceneMotion", kd: Optional[PtKdTree] = None):
        self.check(lib().pt_scene_update(self._h, C.byref(motion), C.byref(kd) if kd is not None else None), "pt_scene_update")

    def deform(self, deforms, motion: "PtSceneMotion", kd: Optional[PtKdTree] = None):
        """pt_scene_deform with a list of PtMeshDeform"""
        arr = (PtMeshDeform * max(len(deforms), 1))(*deforms)
        self.check(lib().pt_scene_deform(self._h, len(deforms), arr, C.byref(motion), C.byref(kd) if kd is not None else None), "pt_scene_deform")

    def deform_device(self, deforms, motion: "PtSceneMotion", kd: Optional[PtKdTree] = None):
        """pt_scene_deform_device with a list of PtMeshDeformDevice (device pointers as integers, e.g. a torch tensor's data_ptr())"""
        arr = (PtMeshDeformDevice * max(len(deforms), 1))(*deforms)
        self.check(lib().pt_scene_deform_device(self._h, len(deforms), arr, C.byref(motion), C.byref(kd) if kd is not None else None), "pt_scene_deform_device")

    def vertex_bounds_device(self, d_positions: int, n_vertices: int):
        """pt_vertex_bounds_device: (box, non_finite) of n_vertices x 3 f64 at the device address d_positions; box = 6 doubles, min then max per axis"""
        box = np.zeros(6)
        bad = C.c_uint64(0)
        self.check(lib().pt_vertex_bounds_device(self._h, n_vertices, C.c_void_p(d_positions), _p(box, _dp), C.byref(bad)), "pt_vertex_bounds_device")
        return box, int(bad.value)

    def render(self, cam: PtCamera, background: np.ndarray, params: PtRenderParams, rgb: np.ndarray, linear: Optional[np.ndarray] = None) -> dict:
        st = PtStats()
        bg = np.ascontiguousarray(background, dtype=np.float64)
        self.check(lib().pt_render(self._h, C.byref(cam), _p(bg, _dp), C.byref(params), _p(rgb, _u8p), _p(linear, _dp), C.byref(st)), "pt_render")
        return st.as_dict()

    def cast_rays(self, origins, directions, any_hit=False):
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        n = len(o)
        t = np.zeros(n); node = np.zeros(n, dtype=np.int32); sub = np.zeros(n, dtype=np.int32)
        self.check(lib().pt_test_cast_rays(self._h, n, _p(o, _dp), _p(d, _dp), int(any_hit), _p(t, _dp), _p(node, _ip), _p(sub, _ip)), "pt_test_cast_rays")
        return t, node, sub

    def math(self, op: int, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
        out = np.zeros_like(a)
        self.check(lib().pt_test_math(self._h, op, a.size, _p(a, _dp), _p(b, _dp), _p(out, _dp)), "pt_test_math")
        return out

    def copy_bandwidth(self, nbytes: int = 1 << 30, iters: int = 5) -> float:
        g = C.c_double(0.0)
        self.check(lib().pt_measure_copy_bandwidth(self._h, nbytes, iters, C.byref(g)), "pt_measure_copy_bandwidth")
        return g.value
