"""Host-side mirror of the reference's pass classes over the C ABI (include/hr_api.h).

Class / method names follow the reference (src/ray_traced_shadows.h etc.): a pass is constructed
for a resolution + scale, ``render()`` records one frame on a HIP stream, ``output()`` replaces
``output_ds()``.  torch is used only for device memory and streams; every kernel is the in-tree HIP
library ``libhybrid_rendering_amd.so``.  There is NO CPU fallback: if the library cannot be loaded
the import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HR_LIBRARY: developer A/B builds (python -m hybrid_rendering_amd.build --variant NAME with HR_CFLAGS=...) — a HIP library either way
LIB_PATH = os.environ.get("HR_LIBRARY") or os.path.join(_HERE, "libhybrid_rendering_amd.so")

# ------------------------------------------------------------------------------ ctypes structs


class hr_light(C.Structure):
    _fields_ = [("data0", C.c_float * 4), ("data1", C.c_float * 4), ("data2", C.c_float * 4), ("data3", C.c_float * 4)]


class hr_ubo(C.Structure):
    _fields_ = [("view_inverse", C.c_float * 16), ("proj_inverse", C.c_float * 16), ("view_proj_inverse", C.c_float * 16),
                ("prev_view_proj", C.c_float * 16), ("view_proj", C.c_float * 16), ("cam_pos", C.c_float * 4),
                ("current_prev_jitter", C.c_float * 4), ("light", hr_light)]


assert C.sizeof(hr_ubo) == 416


class hr_gbuffer_level(C.Structure):
    _fields_ = [("gb1", C.c_void_p), ("gb2", C.c_void_p), ("gb3", C.c_void_p), ("depth", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class hr_frame_inputs(C.Structure):
    _fields_ = [("cur", hr_gbuffer_level), ("prev", hr_gbuffer_level), ("cur_full", hr_gbuffer_level), ("ubo", hr_ubo),
                ("num_frames", C.c_uint32), ("ping_pong", C.c_int32), ("sobol", C.c_void_p), ("scrambling_ranking", C.c_void_p),
                ("z_buffer_params", C.c_float * 4)]


class hr_image_view(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("row_pitch_bytes", C.c_int32), ("format", C.c_int)]


class hr_texture(C.Structure):
    _fields_ = [("rgba8", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class hr_scene_desc(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("tri_material", C.c_void_p), ("tri_mesh_id", C.c_void_p),
                ("n_tris", C.c_int32), ("materials", C.c_void_p), ("n_materials", C.c_int32),
                ("uvs", C.c_void_p), ("tangents", C.c_void_p), ("material_textures", C.c_void_p), ("textures", C.POINTER(hr_texture)),
                ("n_textures", C.c_int32)]


class hr_scene_info(C.Structure):
    _fields_ = [("n_tris", C.c_int32), ("n_nodes", C.c_int32), ("max_depth", C.c_int32), ("node_bytes", C.c_uint64), ("tri_bytes", C.c_uint64),
                ("bounds_lo", C.c_float * 3), ("bounds_hi", C.c_float * 3), ("box_pad", C.c_float)]


class hr_band(C.Structure):
    _fields_ = [("band_y0", C.c_int32), ("band_y1", C.c_int32), ("halo", C.c_int32), ("history_halo", C.c_int32)]


HR_MAX_STAGES = 16


class hr_stage_times(C.Structure):
    _fields_ = [("n_stages", C.c_int32), ("name", C.c_char_p * HR_MAX_STAGES), ("ms", C.c_float * HR_MAX_STAGES), ("bytes", C.c_uint64 * HR_MAX_STAGES)]


class hr_shadows_params(C.Structure):
    _fields_ = [("denoise", C.c_int32), ("bias", C.c_float), ("alpha", C.c_float), ("moments_alpha", C.c_float), ("phi_visibility", C.c_float),
                ("phi_normal", C.c_float), ("sigma_depth", C.c_float), ("power", C.c_float), ("radius", C.c_int32),
                ("filter_iterations", C.c_int32), ("feedback_iteration", C.c_int32), ("exact", C.c_int32)]


class hr_ao_params(C.Structure):
    _fields_ = [("denoise", C.c_int32), ("ray_length", C.c_float), ("bias", C.c_float), ("alpha", C.c_float), ("blur_radius", C.c_int32),
                ("power", C.c_float), ("spp", C.c_int32), ("exact", C.c_int32)]


HR_FORMAT = {1: ("R32_UINT", 4), 2: ("R16F", 2), 3: ("RG16F", 4), 4: ("RGBA16F", 8), 5: ("R32F", 4), 6: ("RGBA8", 4), 0: ("R8", 1)}
OUTPUT_RAY_TRACE, OUTPUT_TEMPORAL_ACCUMULATION, OUTPUT_ATROUS, OUTPUT_UPSAMPLE = 0, 1, 2, 3
SCALE_FULL_RES, SCALE_HALF_RES, SCALE_QUARTER_RES = 0, 1, 2

# every symbol include/hr_api.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "hr_status_string", "hr_last_error", "hr_version", "hr_api_revision", "hr_ctx_create", "hr_ctx_destroy", "hr_ctx_device", "hr_scene_create", "hr_scene_get_info", "hr_scene_id", "hr_scene_create_instanced", "hr_scene_update_instances", "hr_scene_instance_count", "hr_scene_rebuild_top_level", "hr_scene_top_level_rebuilds", "hr_scene_read_bvh", "hr_set_markers", "hr_markers_log",
    "hr_scene_destroy", "hr_trace_any_hit", "hr_trace_closest_hit", "hr_gbuffer_raycast", "hr_shadows_default_params", "hr_shadows_create",
    "hr_shadows_render", "hr_shadows_output", "hr_shadows_reset_history", "hr_shadows_destroy", "hr_shadows_ray_trace", "hr_shadows_denoise", "hr_shadows_temporal",
    "hr_shadows_atrous_iteration", "hr_shadows_upsample", "hr_shadows_image", "hr_shadows_history_apron_exceeded", "hr_shadows_set_profiling", "hr_shadows_get_stage_times",
    "hr_gbuffer_mip_nearest", "hr_bvh_build_info", "hr_bvh_selfcheck", "hr_bvh_child_boxes", "hr_shadows_ray_count", "hr_shadows_tile_ray_counts", "hr_shadows_trace_stats", "hr_shadows_trace_stats_timed", "hr_shadows_launch_order", "hr_shadows_trace_divergence", "hr_selftest_math",
    "hr_selftest_math_sweep", "hr_selftest_fast_math", "hr_selftest_shading",
    "hr_scene_create_instanced_shared", "hr_scene_is_shared", "hr_instanced_scene_footprint", "hr_scene_enable_two_level_passes", "hr_scene_two_level_passes",
    "hr_scene_create_deformable", "hr_scene_update_vertices", "hr_scene_refit_cost", "hr_scene_rebuild", "hr_bvh_build_info_deformable",
    "hr_scene_create_instanced_shared_deformable", "hr_scene_update_meshes", "hr_scene_mesh_refit_cost", "hr_scene_update_meshes_stats", "hr_scene_read_instance_records",
    "hr_scene_motion_begin_frame", "hr_gbuffer_raycast_motion",
    "hr_scene_update_instances_device", "hr_scene_device_update_status", "hr_scene_device_update_stats",
    "hr_scene_rebuild_top_level_device", "hr_scene_set_device_rebuild_threshold", "hr_scene_device_rebuild_status", "hr_shared_top_fixed_shape", "hr_shared_top_sort_keys",
    "hr_scene_rebuild_device", "hr_scene_rebuild_meshes_device", "hr_scene_device_rebuild_counts", "hr_deform_leaf_order",
    "hr_scene_set_instance_masks", "hr_scene_set_instance_masks_device", "hr_scene_get_instance_masks", "hr_scene_set_cull_mask", "hr_scene_get_cull_mask",
    "hr_scene_set_alpha_cutoffs", "hr_scene_get_alpha_cutoffs", "hr_scene_set_ray_class_opaque", "hr_scene_get_ray_class_opaque",
]

# hr_ray_class (include/hr_api_post.h): the ray classes a shared scene keeps a cull mask for
RAY_QUERY, RAY_PRIMARY, RAY_SHADOW, RAY_AO, RAY_REFLECTION, RAY_GI, RAY_CLASS_COUNT = 0, 1, 2, 3, 4, 5, 6
# argtypes of the instance-mask entry points (include/hr_api_post.h)
MASK_ARGTYPES = {
    "hr_scene_set_instance_masks": [C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_scene_set_instance_masks_device": [C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_scene_get_instance_masks": [C.c_void_p, C.c_void_p],
    "hr_scene_set_cull_mask": [C.c_void_p, C.c_int32, C.c_uint32],
    "hr_scene_get_cull_mask": [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32)],
}

# argtypes of the cutout-material entry points (include/hr_api_post.h)
CUTOUT_ARGTYPES = {
    "hr_scene_set_alpha_cutoffs": [C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_scene_get_alpha_cutoffs": [C.c_void_p, C.c_void_p],
    "hr_scene_set_ray_class_opaque": [C.c_void_p, C.c_int32, C.c_int32],
    "hr_scene_get_ray_class_opaque": [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
}

# argtypes of the device-side instance update's entry points (include/hr_api_stages.h)
DEVICE_UPDATE_ARGTYPES = {
    "hr_scene_update_instances_device": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "hr_scene_device_update_status": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "hr_scene_device_update_stats": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "hr_scene_rebuild_top_level_device": [C.c_void_p, C.c_void_p],
    "hr_scene_set_device_rebuild_threshold": [C.c_void_p, C.c_float, C.c_void_p],
    "hr_scene_device_rebuild_status": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)],
    "hr_shared_top_fixed_shape": [C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "hr_shared_top_sort_keys": [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
}

# argtypes of the device re-deal's entry points (include/hr_api_stages.h)
DEVICE_REDEAL_ARGTYPES = {
    "hr_scene_rebuild_device": [C.c_void_p, C.c_void_p],
    "hr_scene_rebuild_meshes_device": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p],
    "hr_scene_device_rebuild_counts": [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "hr_deform_leaf_order": [C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)],
}

_lib = None


class HRError(RuntimeError):
    pass


def lib():
    """Load the HIP library.  Raises if it is missing — there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HRError(f"{LIB_PATH} not built: run `python -m hybrid_rendering_amd.build` (hipcc, gfx950). No CPU fallback exists.")
        try:
            import torch  # noqa: F401  (loads the HIP runtime first so both share one libamdhip64)
        except Exception:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.hr_status_string.restype = C.c_char_p
        _lib.hr_last_error.restype = C.c_char_p
        _lib.hr_version.restype = C.c_char_p
        _lib.hr_scene_id.restype = C.c_uint64
        _lib.hr_scene_id.argtypes = [C.c_void_p]
    return _lib


def _check(status: int, what: str):
    if status != 0:
        L = lib()
        raise HRError(f"{what}: {L.hr_status_string(status).decode()} — {L.hr_last_error().decode()}")


def make_ubo(np_ubo: np.ndarray) -> hr_ubo:
    assert np_ubo.nbytes == 416
    u = hr_ubo()
    C.memmove(C.byref(u), np_ubo.ctypes.data, 416)
    return u


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


# ------------------------------------------------------------------------------ context / scene


class hr_mesh_desc(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("tri_material", C.c_void_p), ("uvs", C.c_void_p), ("tangents", C.c_void_p), ("n_tris", C.c_int32)]


class hr_instance(C.Structure):
    _fields_ = [("model_matrix", C.c_float * 16), ("mesh_idx", C.c_uint32), ("mesh_id", C.c_uint32)]


class hr_instanced_scene_desc(C.Structure):
    _fields_ = [("meshes", C.POINTER(hr_mesh_desc)), ("n_meshes", C.c_int32), ("instances", C.POINTER(hr_instance)), ("n_instances", C.c_int32),
                ("materials", C.c_void_p), ("n_materials", C.c_int32), ("material_textures", C.c_void_p), ("textures", C.c_void_p), ("n_textures", C.c_int32)]


class hr_mesh_update(C.Structure):
    _fields_ = [("mesh_idx", C.c_uint32), ("first_tri", C.c_int32), ("n_tris", C.c_int32), ("positions", C.c_void_p), ("normals", C.c_void_p), ("bounds", C.c_void_p)]


class Context:
    def __init__(self, device: int = 0):
        self.h = C.c_void_p()
        _check(lib().hr_ctx_create(C.c_int(device), C.byref(self.h)), "hr_ctx_create")
        self.device = device

    def close(self):
        if self.h:
            lib().hr_ctx_destroy(self.h)
            self.h = C.c_void_p()


class Scene:
    """Replaces dw::RayTracedScene: host triangles -> compressed 8-wide BVH in HBM.
    ``deformable=True``: hr_scene_create_deformable — the same scene to every pass, built without spatial splits, whose vertices
    ``update_vertices`` replaces on the GPU (the BVH is refitted; ``refit_cost`` / ``rebuild`` for when the refitted tree has gone bad)."""

    def __init__(self, ctx: Context, sd, deformable: bool = False):
        self.ctx, self.deformable, self.n_materials = ctx, bool(deformable), len(sd.materials)
        self._keep = [np.ascontiguousarray(sd.verts, np.float32), None if sd.normals is None else np.ascontiguousarray(sd.normals, np.float32),
                      np.ascontiguousarray(sd.tri_material, np.uint32), np.ascontiguousarray(sd.tri_mesh_id, np.uint32),
                      np.ascontiguousarray(sd.materials, np.float32)]
        v, n, m, i, mats = self._keep
        d = hr_scene_desc(v.ctypes.data, n.ctypes.data if n is not None else None, m.ctypes.data, i.ctypes.data, sd.n_tris, mats.ctypes.data, len(mats))
        if getattr(sd, "material_textures", None) is not None:        # textured materials (optional)
            uv = None if sd.uvs is None else np.ascontiguousarray(sd.uvs, np.float32)
            tg = None if sd.tangents is None else np.ascontiguousarray(sd.tangents, np.float32)
            mt = np.ascontiguousarray(sd.material_textures, np.int32)
            tex = [np.ascontiguousarray(t, np.uint8) for t in sd.textures]
            arr = (hr_texture * len(tex))(*[hr_texture(t.ctypes.data, t.shape[1], t.shape[0]) for t in tex])
            self._keep += [uv, tg, mt, tex, arr]
            d.uvs, d.tangents = (uv.ctypes.data if uv is not None else None), (tg.ctypes.data if tg is not None else None)
            d.material_textures, d.textures, d.n_textures = mt.ctypes.data, arr, len(tex)
        self.h = C.c_void_p()
        if deformable:
            _check(lib().hr_scene_create_deformable(ctx.h, C.byref(d), C.byref(self.h)), "hr_scene_create_deformable")
        else:
            _check(lib().hr_scene_create(ctx.h, C.byref(d), C.byref(self.h)), "hr_scene_create")
        self.info = hr_scene_info()
        _check(lib().hr_scene_get_info(self.h, C.byref(self.info)), "hr_scene_get_info")

    @property
    def id(self) -> int:
        """dw::Scene::id() (hr_scene_id)"""
        return int(lib().hr_scene_id(self.h))

    def close(self):
        if self.h:
            lib().hr_scene_destroy(self.h)
            self.h = C.c_void_p()

    def read_bvh(self):
        """(nodes [n][80] uint8, triangle references [m][48] uint8): host copies of the device BVH (csrc/bvh.h layouts)"""
        self.refresh_info()
        nodes, tris = np.zeros((self.info.n_nodes, 80), np.uint8), np.zeros((int(self.info.tri_bytes) // 48, 48), np.uint8)
        _check(lib().hr_scene_read_bvh(self.h, C.c_void_p(nodes.ctypes.data), C.c_void_p(tris.ctypes.data)), "hr_scene_read_bvh")
        return nodes, tris

    def refresh_info(self):
        _check(lib().hr_scene_get_info(self.h, C.byref(self.info)), "hr_scene_get_info")
        return self.info

    def update_vertices(self, positions, normals=None, first_tri: int = 0, stream=None):
        """hr_scene_update_vertices: ``positions`` (and ``normals``, None: keep) are cuda float32 tensors [n,3,3] for the original triangles
        [first_tri, first_tri + n); enqueued on ``stream`` (default: torch's current stream), no host synchronisation"""
        import torch
        assert positions.is_cuda and positions.dtype == torch.float32 and positions.shape[1:] == (3, 3), "positions: cuda float32 [n,3,3]"
        positions = positions.contiguous()
        if normals is not None:
            assert normals.is_cuda and normals.dtype == torch.float32 and normals.shape == positions.shape, "normals: cuda float32, the shape of positions"
            normals = normals.contiguous()
        L = lib()
        L.hr_scene_update_vertices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        _check(L.hr_scene_update_vertices(self.h, _ptr(positions), _ptr(normals), C.c_int32(first_tri), C.c_int32(positions.shape[0]), _stream_ptr(stream)),
               "hr_scene_update_vertices")

    def refit_cost(self) -> float:
        """hr_scene_refit_cost: sum of the BVH nodes' half areas after the last update / as built (1.0: as built)"""
        r = C.c_float(0.0)
        _check(lib().hr_scene_refit_cost(self.h, C.byref(r)), "hr_scene_refit_cost")
        return float(r.value)

    def rebuild(self, stream=None):
        """hr_scene_rebuild: the slow path — host build over the current vertices; synchronises"""
        _check(lib().hr_scene_rebuild(self.h, _stream_ptr(stream)), "hr_scene_rebuild")
        self.refresh_info()

    def rebuild_device(self, stream=None):
        """hr_scene_rebuild_device (deformable scenes): the triangles re-dealt among the standing tree's leaves in Morton order by kernels on
        ``stream`` (default: torch's current stream), then the refit; no host synchronisation, the answers stand.  ``refit_cost`` afterwards is
        still relative to the host build."""
        L = lib()
        L.hr_scene_rebuild_device.argtypes = DEVICE_REDEAL_ARGTYPES["hr_scene_rebuild_device"]
        _check(L.hr_scene_rebuild_device(self.h, _stream_ptr(stream)), "hr_scene_rebuild_device")

    def device_rebuild_counts(self) -> dict:
        """hr_scene_device_rebuild_counts (host counters): meshes re-dealt on the device and kernel launches enqueued for that so far"""
        a, b = C.c_int64(0), C.c_int64(0)
        L = lib()
        L.hr_scene_device_rebuild_counts.argtypes = DEVICE_REDEAL_ARGTYPES["hr_scene_device_rebuild_counts"]
        _check(L.hr_scene_device_rebuild_counts(self.h, C.byref(a), C.byref(b)), "hr_scene_device_rebuild_counts")
        return dict(rebuilds_enqueued=int(a.value), launches_enqueued=int(b.value))

    def any_hit(self, rays, stats=False, stream=None):
        """rays: cuda float32 [n,8] (origin, t_max, dir, t_min) -> uint8 [n] (1 = occluded)."""
        import torch
        rays = rays.contiguous()
        out = torch.zeros(rays.shape[0], dtype=torch.uint8, device=rays.device)
        st = torch.zeros(2, dtype=torch.int64, device=rays.device) if stats else None
        _check(lib().hr_trace_any_hit(self.h, C.c_int64(rays.shape[0]), _ptr(rays), _ptr(out), _ptr(st), _stream_ptr(stream)), "hr_trace_any_hit")
        return (out, st) if stats else out

    def closest_hit(self, rays, stream=None):
        import torch
        rays = rays.contiguous()
        tuv = torch.zeros((rays.shape[0], 3), dtype=torch.float32, device=rays.device)
        prim = torch.zeros(rays.shape[0], dtype=torch.int32, device=rays.device)
        _check(lib().hr_trace_closest_hit(self.h, C.c_int64(rays.shape[0]), _ptr(rays), _ptr(tuv), _ptr(prim), _stream_ptr(stream)), "hr_trace_closest_hit")
        return tuv, prim

    # ---- alpha-tested cutout materials.  Flat, deformable and shared instanced scenes; a private-copy instanced scene raises
    # HRError (HR_ERR_UNSUPPORTED).  Bad arguments are refused here, before the library is touched.
    def _cutout_call(self, name):
        f = getattr(lib(), name)
        f.argtypes = CUTOUT_ARGTYPES[name]
        return f


    def set_alpha_cutoffs(self, cutoffs, stream=None):
        """hr_scene_set_alpha_cutoffs: one cutoff per material (host, copied before the call returns; <= 0: opaque, the default).  A hit on a
        triangle of material m whose albedo texture's alpha at the hit is below cutoffs[m] does not exist for the ray.  A cutoff above 0 needs an
        albedo texture on the material and uvs in the scene.  Ordered on ``stream`` (default: torch's current stream)."""
        c = np.asarray(cutoffs)
        if c.ndim != 1 or c.shape[0] != self.n_materials:
            raise ValueError(f"cutoffs: one value per material ({self.n_materials}), got shape {c.shape}")
        c = np.ascontiguousarray(c, np.float32)
        if not np.all(np.isfinite(c)):
            raise ValueError("cutoffs: every value must be finite")
        _check(self._cutout_call("hr_scene_set_alpha_cutoffs")(self.h, C.c_void_p(c.ctypes.data), _stream_ptr(stream)), "hr_scene_set_alpha_cutoffs")
        return self

    def alpha_cutoffs(self) -> np.ndarray:
        """hr_scene_get_alpha_cutoffs: float32 [n_materials] as last set (zeros before the first call)"""
        out = np.zeros(self.n_materials, np.float32)
        _check(self._cutout_call("hr_scene_get_alpha_cutoffs")(self.h, C.c_void_p(out.ctypes.data)), "hr_scene_get_alpha_cutoffs")
        return out

    def set_ray_class_opaque(self, cls: int, force_opaque: bool = True):
        """hr_scene_set_ray_class_opaque: rays of class ``cls`` (RAY_QUERY .. RAY_GI) skip the alpha test (gl_RayFlagsOpaqueEXT: the reference's
        behaviour) or, the default, run it.  Host state, read when a pass or query enqueues its launch."""
        if not (isinstance(cls, (int, np.integer)) and 0 <= int(cls) < RAY_CLASS_COUNT):
            raise ValueError(f"ray class {cls!r} is outside [0, {RAY_CLASS_COUNT})")
        _check(self._cutout_call("hr_scene_set_ray_class_opaque")(self.h, C.c_int32(int(cls)), C.c_int32(1 if force_opaque else 0)), "hr_scene_set_ray_class_opaque")
        return self

    def ray_class_opaque(self, cls: int) -> bool:
        if not (isinstance(cls, (int, np.integer)) and 0 <= int(cls) < RAY_CLASS_COUNT):
            raise ValueError(f"ray class {cls!r} is outside [0, {RAY_CLASS_COUNT})")
        v = C.c_int32(0)
        _check(self._cutout_call("hr_scene_get_ray_class_opaque")(self.h, C.c_int32(int(cls)), C.byref(v)), "hr_scene_get_ray_class_opaque")
        return bool(v.value)

    def motion_begin_frame(self, stream=None):
        """hr_scene_motion_begin_frame: remember the geometry as "previous frame" — once per frame, BEFORE that frame's update calls, on their
        stream.  The first call allocates (not under stream capture); a plain hr_scene_create scene takes it as a no-op."""
        L = lib()
        L.hr_scene_motion_begin_frame.argtypes = [C.c_void_p, C.c_void_p]
        _check(L.hr_scene_motion_begin_frame(self.h, _stream_ptr(stream)), "hr_scene_motion_begin_frame")

    def gbuffer(self, np_ubo, w, h, device="cuda", stream=None, motion: bool = False):
        """GPU G-buffer synthesis (stands in for the raster GBuffer pass).  Returns dict of cuda tensors.
        ``motion=True``: hr_gbuffer_raycast_motion — GB2.zw follows the hit point's own motion since the last ``motion_begin_frame``."""
        import torch
        gb1 = torch.zeros((h, w, 4), dtype=torch.uint8, device=device)
        gb2 = torch.zeros((h, w, 4), dtype=torch.float16, device=device)
        gb3 = torch.zeros((h, w, 4), dtype=torch.float16, device=device)
        depth = torch.zeros((h, w), dtype=torch.float32, device=device)
        u = make_ubo(np_ubo)
        if motion:
            L = lib()
            L.hr_gbuffer_raycast_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            _check(L.hr_gbuffer_raycast_motion(self.h, C.byref(u), C.c_int32(w), C.c_int32(h), _ptr(gb1), _ptr(gb2), _ptr(gb3), _ptr(depth), _stream_ptr(stream)),
                   "hr_gbuffer_raycast_motion")
            return dict(gb1=gb1, gb2=gb2, gb3=gb3, depth=depth)
        _check(lib().hr_gbuffer_raycast(self.h, C.byref(u), C.c_int32(w), C.c_int32(h), _ptr(gb1), _ptr(gb2), _ptr(gb3), _ptr(depth), _stream_ptr(stream)),
               "hr_gbuffer_raycast")
        return dict(gb1=gb1, gb2=gb2, gb3=gb3, depth=depth)

    # ---- emissive materials (include/hr_emission.h, emission.py; DESIGN.md §7 "Emissive materials"): opt-in per scene, off by default, every kind of scene
    def set_emission(self, enable: bool = True, scale: float = 1.0, stream=None):
        """hr_scene_set_emission: hits on emitting materials add ``scale`` x their emissive colour (or emissive texture) in the DDGI, reflection and
        ground-truth hit shaders.  Enabling validates the emissive constants (finite, >= 0)."""
        from . import emission
        emission.set_emission(self.h, enable, scale, stream)
        return self

    def emission_state(self):
        """hr_scene_get_emission -> (enabled, scale)"""
        from . import emission
        return emission.get_emission(self.h)

    def set_emissive(self, rgb, stream=None):
        """hr_scene_set_emissive: per-material emissive rgb [n_materials, 3] (initially materials[:, 5:8]).  A cuda float32 tensor goes through
        hr_scene_set_emissive_device: one device copy, capturable, unchecked."""
        from . import emission
        emission.set_emissive(self.h, self.n_materials, rgb, stream)
        return self

    def set_emissive_textures(self, tex, stream=None):
        """hr_scene_set_emissive_textures: per material an index into the scene's textures (-1: none); the texture replaces the constant"""
        from . import emission
        emission.set_emissive_textures(self.h, self.n_materials, tex, stream)
        return self

    def emission(self, prim, tuv, stream=None):
        """hr_scene_emission: E (cuda float32 [n, 3]) of hits as ``closest_hit`` reports them (``tuv`` [n, 3], ``prim`` [n])"""
        from . import emission
        return emission.emission(self.h, prim, tuv, stream)

    def emissive_image(self, np_ubo, w, h, device="cuda", stream=None):
        """hr_gbuffer_emissive: the E of every pixel's primary hit, cuda float16 [h, w, 4]; zeros where the G-buffer has sky"""
        from . import emission
        return emission.emissive_image(self.h, np_ubo, w, h, device, stream)

    # ---- extra lights (include/hr_lights.h, lights.py): a per-scene list beside the UBO light, empty by default, every kind of scene
    def set_lights(self, lights, stream=None):
        """hr_scene_set_lights: up to HR_MAX_LIGHTS hr_light records (host float32 [n, 4, 4]; ``lights.light`` makes one) that the DDGI, reflection and
        ground-truth hit shaders add to the UBO light, and that ``lights.Lights`` draws on the primary surfaces.  An empty list is off."""
        from . import lights as _lights
        _lights.set_lights(self.h, lights, stream)
        return self

    def set_lights_device(self, lights, stream=None):
        """hr_scene_set_lights_device: the same count as the last ``set_lights``, from a cuda float32 tensor; one device copy, capturable, unchecked"""
        from . import lights as _lights
        _lights.set_lights_device(self.h, lights, stream)
        return self

    def get_lights(self):
        """hr_scene_get_lights -> float32 [n, 4, 4], what the host last set"""
        from . import lights as _lights
        return _lights.get_lights(self.h)


def _instanced_desc(isd):
    """(hr_instanced_scene_desc, the host arrays it points into) of a synth.InstancedSceneData"""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    keep, meshes = [], (hr_mesh_desc * len(isd.meshes))()
    for k, m in enumerate(isd.meshes):
        arrs = [f32(m.verts), f32(m.normals), np.ascontiguousarray(m.tri_material, np.uint32), f32(m.uvs), f32(m.tangents)]
        keep.append(arrs)
        meshes[k] = hr_mesh_desc(*[(a.ctypes.data if a is not None else None) for a in arrs], m.n_tris)
    inst = (hr_instance * len(isd.instances))()
    for i, (mat, mesh_idx, mesh_id) in enumerate(isd.instances):
        inst[i].model_matrix[:] = [float(v) for v in np.asarray(mat, np.float32).reshape(16)]
        inst[i].mesh_idx, inst[i].mesh_id = int(mesh_idx), int(mesh_id)
    mats = np.ascontiguousarray(isd.materials, np.float32)
    d = hr_instanced_scene_desc(meshes, len(isd.meshes), inst, len(isd.instances), mats.ctypes.data, len(mats), None, None, 0)
    if isd.material_textures is not None:
        mt = np.ascontiguousarray(isd.material_textures, np.int32)
        tex = [np.ascontiguousarray(t, np.uint8) for t in isd.textures]
        arr = (hr_texture * len(tex))(*[hr_texture(t.ctypes.data, t.shape[1], t.shape[0]) for t in tex])
        keep += [mt, tex, arr]
        d.material_textures, d.textures, d.n_textures = mt.ctypes.data, C.cast(arr, C.c_void_p), len(tex)
    return d, [keep, meshes, inst, mats]


def instanced_scene_footprint(isd, shared: bool):
    """hr_instanced_scene_footprint (host only): (status, hr_scene_info) of the scene either kind would build for ``isd`` — status 0, or
    5 (HR_ERR_UNSUPPORTED) with the sizes filled in when that kind cannot hold it"""
    d, keep = _instanced_desc(isd)
    info = hr_scene_info()
    st = lib().hr_instanced_scene_footprint(C.byref(d), C.c_int32(1 if shared else 0), C.byref(info))
    del keep
    return int(st), info


class InstancedScene(Scene):
    """dw::RayTracedScene as the reference holds it — meshes + instances — with the per-frame update of main.cpp:74 (build_tlas):
    hr_scene_create_instanced / hr_scene_update_instances.  ``isd``: synth.InstancedSceneData.  Every pass takes it like a Scene.
    ``shared=True``: hr_scene_create_instanced_shared — one BVH per mesh, walked on two levels; same answers, O(meshes + instances) memory;
    queries, the G-buffer synthesiser and the shadows pass take it; AO, DDGI, reflections, the ground truth and the hybrid frame take it after
    ``enable_two_level_passes()`` and raise HRError (HR_ERR_UNSUPPORTED) before it (the default, until the next API revision).
    ``deformable=[...]`` (with ``shared=True``): hr_scene_create_instanced_shared_deformable — one flag per mesh; a flagged mesh is built without
    spatial splits and ``update_meshes`` replaces its vertices on the GPU (``mesh_refit_cost`` for when its refitted tree has gone bad)."""

    def __init__(self, ctx: Context, isd, shared: bool = False, deformable=None):
        self.ctx, self.isd, self.shared, self.n_materials = ctx, isd, bool(shared), len(isd.materials)
        d, self._keep = _instanced_desc(isd)
        self.h = C.c_void_p()
        if deformable is not None:
            assert shared, "deformable meshes live in a shared scene (shared=True)"
            flags = np.ascontiguousarray(np.asarray(deformable).astype(bool), np.uint8)
            assert flags.shape == (len(isd.meshes),), "deformable: one flag per mesh"
            L = lib()
            L.hr_scene_create_instanced_shared_deformable.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            _check(L.hr_scene_create_instanced_shared_deformable(ctx.h, C.byref(d), C.c_void_p(flags.ctypes.data), C.byref(self.h)), "hr_scene_create_instanced_shared_deformable")
        elif shared:
            _check(lib().hr_scene_create_instanced_shared(ctx.h, C.byref(d), C.byref(self.h)), "hr_scene_create_instanced_shared")
        else:
            _check(lib().hr_scene_create_instanced(ctx.h, C.byref(d), C.byref(self.h)), "hr_scene_create_instanced")
        self.info = hr_scene_info()
        self.refresh_info()

    def enable_two_level_passes(self, on: bool = True):
        """hr_scene_enable_two_level_passes: let AO, DDGI, reflections, the ground truth and the hybrid frame walk this SHARED scene on two levels
        (off by default: they refuse it).  Changes nothing about the scene's arrays or its answers; HRError (HR_ERR_INVALID_ARG) for another kind."""
        _check(lib().hr_scene_enable_two_level_passes(self.h, C.c_int32(1 if on else 0)), "hr_scene_enable_two_level_passes")
        return self

    @property
    def two_level_passes(self) -> bool:
        return bool(lib().hr_scene_two_level_passes(self.h))

    def rebuild_top_level(self, stream=None):
        _check(lib().hr_scene_rebuild_top_level(self.h, _stream_ptr(stream)), "hr_scene_rebuild_top_level")

    @property
    def top_level_rebuilds(self) -> int:
        return int(lib().hr_scene_top_level_rebuilds(self.h))

    def update_meshes(self, updates, stream=None):
        """hr_scene_update_meshes: ``updates`` is a list of (mesh_idx, positions) or dicts with keys mesh_idx, positions (cuda float32 [n,3,3],
        object space), and optionally normals (cuda, the shape of positions; default: keep), first_tri (default 0) and bounds (host, (lo xyz, hi xyz)
        of the WHOLE mesh after the update; default: measured on the GPU, which makes the call wait once).  Enqueued on ``stream``."""
        import torch
        arr, keep = (hr_mesh_update * max(1, len(updates)))(), []
        for i, u in enumerate(updates):
            if not isinstance(u, dict):
                u = dict(mesh_idx=u[0], positions=u[1])
            pos, nrm, bounds = u["positions"], u.get("normals"), u.get("bounds")
            assert pos.is_cuda and pos.dtype == torch.float32 and pos.shape[1:] == (3, 3), "positions: cuda float32 [n,3,3]"
            pos = pos.contiguous()
            if nrm is not None:
                assert nrm.is_cuda and nrm.dtype == torch.float32 and nrm.shape == pos.shape, "normals: cuda float32, the shape of positions"
                nrm = nrm.contiguous()
            if bounds is not None:
                bounds = np.ascontiguousarray(np.concatenate([np.asarray(b, np.float32).reshape(3) for b in bounds]), np.float32)
            keep.append((pos, nrm, bounds))
            arr[i] = hr_mesh_update(int(u["mesh_idx"]), int(u.get("first_tri", 0)), int(pos.shape[0]), pos.data_ptr() if pos.shape[0] else None,
                                    nrm.data_ptr() if nrm is not None else None, bounds.ctypes.data if bounds is not None else None)
        L = lib()
        L.hr_scene_update_meshes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        _check(L.hr_scene_update_meshes(self.h, C.cast(arr, C.c_void_p), C.c_int32(len(updates)), _stream_ptr(stream)), "hr_scene_update_meshes")
        del keep

    def rebuild_meshes_device(self, mesh_idx, stream=None):
        """hr_scene_rebuild_meshes_device (shared deformable scenes): the flagged meshes ``mesh_idx`` (distinct) re-dealt by kernels on ``stream``
        (default: torch's current stream), then refitted; the vertices do not change, so the top level stands untouched"""
        m = np.ascontiguousarray(np.asarray(mesh_idx, np.int64).reshape(-1).astype(np.uint32))
        L = lib()
        L.hr_scene_rebuild_meshes_device.argtypes = DEVICE_REDEAL_ARGTYPES["hr_scene_rebuild_meshes_device"]
        _check(L.hr_scene_rebuild_meshes_device(self.h, C.c_void_p(m.ctypes.data) if len(m) else None, C.c_int32(len(m)), _stream_ptr(stream)), "hr_scene_rebuild_meshes_device")

    def mesh_refit_cost(self, mesh_idx: int) -> float:
        """hr_scene_mesh_refit_cost: sum of mesh ``mesh_idx``'s BVH nodes' half areas after its last update / as built (synchronises); raises HRError
        (HR_ERR_INVALID_ARG) when the bounds given with the last update do not contain the mesh"""
        r = C.c_float(0.0)
        L = lib()
        L.hr_scene_mesh_refit_cost.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        _check(L.hr_scene_mesh_refit_cost(self.h, C.c_uint32(mesh_idx), C.byref(r)), "hr_scene_mesh_refit_cost")
        return float(r.value)

    def update_meshes_stats(self) -> dict:
        """hr_scene_update_meshes_stats: launches of the per-level refit kernel, of the one-workgroup-per-mesh kernel, and stream waits so far"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(lib().hr_scene_update_meshes_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "hr_scene_update_meshes_stats")
        return dict(level_launches=int(a.value), top_launches=int(b.value), stream_waits=int(c.value))

    def read_records(self) -> np.ndarray:
        """hr_scene_read_instance_records: the shared scene's instance records, [n_instances][160] uint8, in the order of the top level's leaves"""
        out = np.zeros((int(lib().hr_scene_instance_count(self.h)), 160), np.uint8)
        _check(lib().hr_scene_read_instance_records(self.h, C.c_void_p(out.ctypes.data)), "hr_scene_read_instance_records")
        return out

    def update_device(self, matrices_cuda, bounds=None, stream=None):
        """hr_scene_update_instances_device (shared scenes): ``matrices_cuda`` is a cuda float32 contiguous tensor [n_instances, 16], column-major,
        read when the kernels RUN (a captured call picks up the buffer's contents at replay).  ``bounds``: host (lo xyz, hi xyz), conservative for
        the whole scene after this update — then nothing but kernels is enqueued on ``stream`` (default: torch's current stream); None: measured on
        the GPU, the call waits once (HRError while the stream is capturing).  The top level is refitted, not re-built (``device_update_status``) —
        unless ``set_device_rebuild_threshold`` is on: then the device re-builds it behind the refit when its cost ratio exceeds the threshold."""
        import torch
        n = int(lib().hr_scene_instance_count(self.h))
        assert matrices_cuda.is_cuda and matrices_cuda.dtype == torch.float32 and matrices_cuda.is_contiguous() and tuple(matrices_cuda.shape) == (n, 16), \
            "matrices: cuda float32 contiguous [n_instances, 16]"
        b = None
        if bounds is not None:
            b = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in bounds]), np.float32)
            assert b.shape == (6,), "bounds: (lo xyz, hi xyz)"
        L = lib()
        L.hr_scene_update_instances_device.argtypes = DEVICE_UPDATE_ARGTYPES["hr_scene_update_instances_device"]
        _check(L.hr_scene_update_instances_device(self.h, _ptr(matrices_cuda), C.c_void_p(b.ctypes.data) if b is not None else None, _stream_ptr(stream)),
               "hr_scene_update_instances_device")

    def device_update_status(self) -> dict:
        """hr_scene_device_update_status (synchronises when it lags): top_cost_ratio — the top level's half-area sum after the last device update /
        at its last build (the host path re-builds beyond 1.5; here the caller decides: ``rebuild_top_level``); rejected_instances — non-finite
        matrices of the last update (those instances kept their record); bounds_violated — an instance box left the given bounds"""
        r, a, b = C.c_float(1.0), C.c_int32(0), C.c_int32(0)
        L = lib()
        L.hr_scene_device_update_status.argtypes = DEVICE_UPDATE_ARGTYPES["hr_scene_device_update_status"]
        _check(L.hr_scene_device_update_status(self.h, C.byref(r), C.byref(a), C.byref(b)), "hr_scene_device_update_status")
        return dict(top_cost_ratio=float(r.value), rejected_instances=int(a.value), bounds_violated=int(b.value))

    def device_update_stats(self) -> dict:
        """hr_scene_device_update_stats: kernel launches of the device updates and device re-builds so far, and stream waits (measured bounds; the read-back a host
        call makes after a device update)"""
        a, b = C.c_int64(0), C.c_int64(0)
        L = lib()
        L.hr_scene_device_update_stats.argtypes = DEVICE_UPDATE_ARGTYPES["hr_scene_device_update_stats"]
        _check(L.hr_scene_device_update_stats(self.h, C.byref(a), C.byref(b)), "hr_scene_device_update_stats")
        return dict(launches=int(a.value), stream_waits=int(b.value))

    def rebuild_top_level_device(self, stream=None):
        """hr_scene_rebuild_top_level_device (shared scenes): the top level re-built by kernels on ``stream`` (default: torch's current stream) over
        the boxes and bounds of the last update; nothing is read back.  The call that changes the shape (the first, or the first after
        ``rebuild_top_level``) raises HRError while the stream is capturing; later ones may be captured."""
        L = lib()
        L.hr_scene_rebuild_top_level_device.argtypes = DEVICE_UPDATE_ARGTYPES["hr_scene_rebuild_top_level_device"]
        _check(L.hr_scene_rebuild_top_level_device(self.h, _stream_ptr(stream)), "hr_scene_rebuild_top_level_device")

    def set_device_rebuild_threshold(self, ratio: float, stream=None):
        """hr_scene_set_device_rebuild_threshold: 0 switches it off (the default); ``ratio`` > 1 brings the scene to the fixed shape at once and
        makes every ``update_device`` enqueue the re-build behind its refit, run on the device only when top_cost_ratio exceeds ``ratio``."""
        L = lib()
        L.hr_scene_set_device_rebuild_threshold.argtypes = DEVICE_UPDATE_ARGTYPES["hr_scene_set_device_rebuild_threshold"]
        _check(L.hr_scene_set_device_rebuild_threshold(self.h, C.c_float(ratio), _stream_ptr(stream)), "hr_scene_set_device_rebuild_threshold")

    def device_rebuild_status(self) -> dict:
        """hr_scene_device_rebuild_status (synchronises when it lags): rebuilds_done — device re-builds that ran, counted on the device;
        launches_enqueued — kernel launches enqueued for re-builds so far; fixed_shape — the top level has the shape of hr_shared_top_fixed_shape"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        L = lib()
        L.hr_scene_device_rebuild_status.argtypes = DEVICE_UPDATE_ARGTYPES["hr_scene_device_rebuild_status"]
        _check(L.hr_scene_device_rebuild_status(self.h, C.byref(a), C.byref(b), C.byref(c)), "hr_scene_device_rebuild_status")
        return dict(rebuilds_done=int(a.value), launches_enqueued=int(b.value), fixed_shape=int(c.value))

    def _mask_call(self, name):
        f = getattr(lib(), name)
        f.argtypes = MASK_ARGTYPES[name]
        return f

    def set_instance_masks(self, masks, stream=None):
        """hr_scene_set_instance_masks / _device (shared scenes): one 8-bit mask per instance, in the order of the scene desc.  A numpy array (or
        anything array-like on the host) is copied before the call returns; a cuda uint8 tensor [n_instances] is read when the kernel RUNS on
        ``stream`` (default: torch's current stream) — that form may be captured, and a replay picks up the tensor's contents.  A ray walks into
        an instance iff its mask and the cull mask of the ray's class share a bit (``set_cull_mask``); all masks start at 0xFF."""
        import torch
        n = int(lib().hr_scene_instance_count(self.h))
        if isinstance(masks, torch.Tensor) and masks.is_cuda:
            assert masks.dtype == torch.uint8 and masks.is_contiguous() and tuple(masks.shape) == (n,), "masks: cuda uint8 contiguous [n_instances]"
            _check(self._mask_call("hr_scene_set_instance_masks_device")(self.h, _ptr(masks), _stream_ptr(stream)), "hr_scene_set_instance_masks_device")
            return
        m = np.ascontiguousarray(np.asarray(masks.cpu() if isinstance(masks, torch.Tensor) else masks))
        assert m.shape == (n,) and (m.size == 0 or (int(m.min()) >= 0 and int(m.max()) <= 0xFF)), "masks: [n_instances] values in 0..0xFF"
        m = np.ascontiguousarray(m, np.uint8)
        _check(self._mask_call("hr_scene_set_instance_masks")(self.h, C.c_void_p(m.ctypes.data), _stream_ptr(stream)), "hr_scene_set_instance_masks")

    def instance_masks(self) -> np.ndarray:
        """hr_scene_get_instance_masks: the instances' masks, uint8 [n_instances] in the order of the scene desc (synchronises when a device call
        set them since the host last knew them)"""
        out = np.zeros(int(lib().hr_scene_instance_count(self.h)), np.uint8)
        _check(self._mask_call("hr_scene_get_instance_masks")(self.h, C.c_void_p(out.ctypes.data)), "hr_scene_get_instance_masks")
        return out

    def set_cull_mask(self, cls: int, mask: int):
        """hr_scene_set_cull_mask: the 8-bit cull mask of ray class ``cls`` (RAY_QUERY .. RAY_GI; 0xFF by default).  Host state, read when a pass or
        query enqueues its launch: a graph the caller captured keeps the masks of capture time."""
        assert 0 <= int(mask) <= 0xFFFFFFFF
        _check(self._mask_call("hr_scene_set_cull_mask")(self.h, C.c_int32(cls), C.c_uint32(int(mask))), "hr_scene_set_cull_mask")
        return self

    def cull_mask(self, cls: int) -> int:
        m = C.c_uint32(0)
        _check(self._mask_call("hr_scene_get_cull_mask")(self.h, C.c_int32(cls), C.byref(m)), "hr_scene_get_cull_mask")
        return int(m.value)

    def update(self, matrices, stream=None):
        """hr_scene_update_instances: matrices [n_instances][16] column-major (host); enqueued on ``stream`` (default: torch's current stream)"""
        m = np.ascontiguousarray(np.asarray(matrices, np.float32).reshape(-1, 16))
        assert m.shape[0] == lib().hr_scene_instance_count(self.h)
        _check(lib().hr_scene_update_instances(self.h, m.ctypes.data_as(C.POINTER(C.c_float)), _stream_ptr(stream)), "hr_scene_update_instances")


def bvh_build_info(verts, deformable: bool = False) -> hr_scene_info:
    """Host-only BVH build (no GPU): the shape hr_scene_create (``deformable``: hr_scene_create_deformable, no spatial splits) would produce
    for triangles ``verts`` [n,3,3]."""
    v = np.ascontiguousarray(verts, np.float32)
    info = hr_scene_info()
    fn, name = (lib().hr_bvh_build_info_deformable, "hr_bvh_build_info_deformable") if deformable else (lib().hr_bvh_build_info, "hr_bvh_build_info")
    _check(fn(v.ctypes.data_as(C.POINTER(C.c_float)), C.c_int32(v.shape[0]), C.byref(info)), name)
    return info


def bvh_selfcheck(verts, samples_per_triangle: int = 12) -> int:
    """Host-only: (triangle, surface point) pairs that the BVH built over ``verts`` fails to cover (0 for a correct tree)."""
    v = np.ascontiguousarray(verts, np.float32)
    bad = C.c_int64(-1)
    L = lib()
    L.hr_bvh_selfcheck.argtypes = [C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    _check(L.hr_bvh_selfcheck(v.ctypes.data_as(C.POINTER(C.c_float)), C.c_int32(v.shape[0]), C.c_int32(samples_per_triangle), C.byref(bad)), "hr_bvh_selfcheck")
    return int(bad.value)


def deform_leaf_order(nodes, root: int = 0, capacity: int = None) -> np.ndarray:
    """Host-only (hr_deform_leaf_order): the reference slots of the tree under ``root`` in ``nodes`` ([n][80] uint8, csrc/bvh.h) in depth-first
    order — slots of a node in slot order, a leaf's triangles in offset order — relative to the tree's first reference.  ``capacity``: room
    for that many (default: 32 per node, more than any tree has); HRError (HR_ERR_INVALID_ARG) when it is too small"""
    nd = np.ascontiguousarray(np.asarray(nodes, np.uint8).reshape(-1, 80))
    cap = int(capacity) if capacity is not None else 32 * len(nd)
    out, n = np.full(max(cap, 1), -1, np.int32), C.c_int32(0)
    L = lib()
    L.hr_deform_leaf_order.argtypes = DEVICE_REDEAL_ARGTYPES["hr_deform_leaf_order"]
    _check(L.hr_deform_leaf_order(C.c_void_p(nd.ctypes.data), C.c_int32(len(nd)), C.c_uint32(root), C.c_void_p(out.ctypes.data), C.c_int32(cap), C.byref(n)), "hr_deform_leaf_order")
    return out[:int(n.value)].copy()


SHARED_TOP_NODE_DTYPE = np.dtype([(k, np.int32) for k in ("n_internal", "n_leaves", "child_base", "leaf_base", "axis", "depth")])


def shared_top_fixed_shape(n_instances: int):
    """Host-only: (nodes, n_depths) of the fixed 8-wide top level a device re-build gives a shared scene of ``n_instances`` instances — a
    structured array (SHARED_TOP_NODE_DTYPE), slots breadth-first"""
    L = lib()
    L.hr_shared_top_fixed_shape.argtypes = DEVICE_UPDATE_ARGTYPES["hr_shared_top_fixed_shape"]
    n, d = C.c_int32(0), C.c_int32(0)
    _check(L.hr_shared_top_fixed_shape(C.c_int32(n_instances), None, C.c_int64(0), C.byref(n), C.byref(d)), "hr_shared_top_fixed_shape")
    out = np.zeros(int(n.value), SHARED_TOP_NODE_DTYPE)
    _check(L.hr_shared_top_fixed_shape(C.c_int32(n_instances), C.c_void_p(out.ctypes.data), C.c_int64(len(out)), C.byref(n), C.byref(d)), "hr_shared_top_fixed_shape")
    return out, int(d.value)


def shared_top_sort_keys(inst_boxes, bounds) -> np.ndarray:
    """Host-only: the uint64 sort keys (30-bit Morton code << 32 | instance) of ``inst_boxes`` [n,6] (lo xyz, hi xyz) inside ``bounds`` (lo xyz, hi xyz)"""
    b = np.ascontiguousarray(np.asarray(inst_boxes, np.float32).reshape(-1, 6))
    w = np.ascontiguousarray(np.asarray(bounds, np.float32).reshape(6))
    out = np.zeros(len(b), np.uint64)
    L = lib()
    L.hr_shared_top_sort_keys.argtypes = DEVICE_UPDATE_ARGTYPES["hr_shared_top_sort_keys"]
    _check(L.hr_shared_top_sort_keys(C.c_void_p(b.ctypes.data), C.c_int32(len(b)), C.c_void_p(w.ctypes.data), C.c_void_p(out.ctypes.data)), "hr_shared_top_sort_keys")
    return out


CHILD_BOX_DTYPE = np.dtype([("lo", np.float32, 3), ("hi", np.float32, 3), ("step", np.float32, 3), ("node", np.int32), ("slot", np.int32), ("depth", np.int32), ("is_leaf", np.int32)])


def bvh_child_boxes(verts) -> np.ndarray:
    """Host-only: the de-quantised child boxes of the BVH hr_scene_create would build over ``verts`` [n,3,3], as the traversal's box
    test sees them — a structured array (CHILD_BOX_DTYPE): lo, hi, the node's quantisation step per axis, node, slot, depth, is_leaf."""
    v = np.ascontiguousarray(verts, np.float32)
    L = lib()
    L.hr_bvh_child_boxes.argtypes = [C.POINTER(C.c_float), C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    n = C.c_int64(0)
    _check(L.hr_bvh_child_boxes(v.ctypes.data_as(C.POINTER(C.c_float)), C.c_int32(v.shape[0]), None, C.c_int64(0), C.byref(n)), "hr_bvh_child_boxes")
    out = np.zeros(int(n.value), CHILD_BOX_DTYPE)
    _check(L.hr_bvh_child_boxes(v.ctypes.data_as(C.POINTER(C.c_float)), C.c_int32(v.shape[0]), C.c_void_p(out.ctypes.data), C.c_int64(len(out)), C.byref(n)), "hr_bvh_child_boxes")
    assert int(n.value) == len(out)
    return out


def gbuffer_mip(g, level, stream=None):
    """Nearest mip `level` of a G-buffer dict of cuda tensors (g_buffer.cpp:240-243) -> new dict at (H >> level, W >> level)."""
    import torch
    h, w = g["depth"].shape
    hh, ww = h >> level, w >> level
    out = dict(gb2=torch.empty((hh, ww, 4), dtype=torch.float16, device="cuda"), gb3=torch.empty((hh, ww, 4), dtype=torch.float16, device="cuda"),
               depth=torch.empty((hh, ww), dtype=torch.float32, device="cuda"))
    if g.get("gb1") is not None:
        out["gb1"] = torch.empty((hh, ww, 4), dtype=torch.uint8, device="cuda")
    src, dst = gbuffer_level(g), gbuffer_level(out)
    _check(lib().hr_gbuffer_mip_nearest(C.byref(src), C.byref(dst), C.c_int32(level), _stream_ptr(stream)), "hr_gbuffer_mip_nearest")
    return out


# ------------------------------------------------------------------------------ frame inputs


def gbuffer_level(g) -> hr_gbuffer_level:
    if g is None:
        return hr_gbuffer_level()
    h, w = g["depth"].shape
    return hr_gbuffer_level(_ptr(g.get("gb1")), _ptr(g["gb2"]), _ptr(g["gb3"]), _ptr(g["depth"]), w, h)


def frame_inputs(cur, prev, np_ubo, num_frames, ping_pong, sobol, scrambling_ranking, cur_full=None, z_buffer_params=(0, 0, 0, 0)) -> hr_frame_inputs:
    """cur/prev/cur_full: dicts of cuda tensors gb1 (u8 HxWx4), gb2/gb3 (f16 HxWx4), depth (f32 HxW)."""
    f = hr_frame_inputs()
    f.cur = gbuffer_level(cur)
    f.prev = gbuffer_level(prev if prev is not None else cur)
    f.cur_full = gbuffer_level(cur_full if cur_full is not None else cur)
    f.ubo = make_ubo(np_ubo)
    f.num_frames = int(num_frames)
    f.ping_pong = int(bool(ping_pong))
    f.sobol = _ptr(sobol)
    f.scrambling_ranking = _ptr(scrambling_ranking)
    for i in range(4):
        f.z_buffer_params[i] = float(z_buffer_params[i])
    f._keep = (cur, prev, cur_full, sobol, scrambling_ranking)
    return f


def view_to_tensor(v: hr_image_view, device="cuda"):
    """Zero-copy torch view of a pass-owned image (valid until the next render()/destroy)."""
    import torch
    name, bpp = HR_FORMAT[int(v.format)]
    # build a tensor from the raw device pointer via __cuda_array_interface__
    dt = {"R32_UINT": ("<i4", 1, torch.int32), "R16F": ("<f2", 1, torch.float16), "RG16F": ("<f2", 2, torch.float16),
          "RGBA16F": ("<f2", 4, torch.float16), "R32F": ("<f4", 1, torch.float32), "RGBA8": ("|u1", 4, torch.uint8), "R8": ("|u1", 1, torch.uint8)}[name]

    class _W:
        pass

    w = _W()
    shape = (v.height, v.width, dt[1]) if dt[1] > 1 else (v.height, v.width)
    w.__cuda_array_interface__ = dict(shape=shape, typestr=dt[0], data=(int(v.data), False), version=2)
    return torch.as_tensor(w, device=device)


# ------------------------------------------------------------------------------ RayTracedShadows


class _Pass:
    _prefix = ""

    def stage_times(self):
        st = hr_stage_times()
        _check(getattr(lib(), self._prefix + "_get_stage_times")(self.h, C.byref(st)), self._prefix + "_get_stage_times")
        return [(st.name[i].decode(), float(st.ms[i]), int(st.bytes[i])) for i in range(st.n_stages)]

    def set_profiling(self, on=True):
        _check(getattr(lib(), self._prefix + "_set_profiling")(self.h, C.c_int32(int(on))), self._prefix + "_set_profiling")

    def image(self, which):
        v = hr_image_view()
        _check(getattr(lib(), self._prefix + "_image")(self.h, C.c_int32(which), C.byref(v)), self._prefix + "_image")
        return view_to_tensor(v)

    def output(self, kind=OUTPUT_UPSAMPLE):
        v = hr_image_view()
        _check(getattr(lib(), self._prefix + "_output")(self.h, C.c_int(kind), C.byref(v)), self._prefix + "_output")
        return view_to_tensor(v)

    def history_apron_exceeded(self) -> bool:
        """row bands: a history tap fell on an image row this GPU does not hold since the last call (motion beyond history_halo)"""
        v = C.c_int32(0)
        _check(getattr(lib(), self._prefix + "_history_apron_exceeded")(self.h, C.byref(v)), self._prefix + "_history_apron_exceeded")
        return bool(v.value)

    def reset_history(self):
        _check(getattr(lib(), self._prefix + "_reset_history")(self.h), self._prefix + "_reset_history")

    def launch_order(self) -> np.ndarray:
        """the trace kernel's launch list (launch slot -> 8x8 tile) as its next launch will read it: always a permutation; the identity
        until the first sort has run (hr_shadows_launch_order / hr_ao_launch_order)"""
        fn = getattr(lib(), self._prefix + "_launch_order")
        n = C.c_int32(0)
        _check(fn(self.h, None, C.byref(n)), self._prefix + "_launch_order")
        out = np.zeros(n.value, np.uint32)
        if n.value:
            _check(fn(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), None), self._prefix + "_launch_order")
        return out

    def close(self):
        if self.h:
            getattr(lib(), self._prefix + "_destroy")(self.h)
            self.h = C.c_void_p()


class RayTracedShadows(_Pass):
    """src/ray_traced_shadows.h:7-142.  ``render(scene, frame_inputs)`` = RayTracedShadows::render(cmd_buf)."""
    _prefix = "hr_shadows"
    IMG_MASK, IMG_TEMPORAL, IMG_MOMENTS0, IMG_MOMENTS1, IMG_PREV, IMG_ATROUS0, IMG_ATROUS1, IMG_UPSAMPLE, IMG_TILES, IMG_GEO = range(10)   # IMG_GEO: tolerance mode, the geometry records of the last temporal stage

    def __init__(self, ctx: Context, width: int, height: int, scale: int = SCALE_FULL_RES, band=None):
        self.ctx = ctx
        self.params = hr_shadows_params()
        lib().hr_shadows_default_params(C.byref(self.params))
        self.h = C.c_void_p()
        b = hr_band(*band) if band else None
        _check(lib().hr_shadows_create(ctx.h, C.c_int32(width), C.c_int32(height), C.c_int(scale), C.byref(b) if b else None, C.byref(self.h)), "hr_shadows_create")
        self.scale = scale
        self.width, self.height = width >> scale, height >> scale

    def render(self, scene: Scene, inputs: hr_frame_inputs, stream=None):
        _check(lib().hr_shadows_render(self.h, scene.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_shadows_render")

    # stage-level entry points (multi-GPU halo exchange happens between them)
    def ray_trace(self, scene, inputs, stream=None):
        _check(lib().hr_shadows_ray_trace(self.h, scene.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_shadows_ray_trace")

    def denoise(self, inputs, stream=None):
        """everything of render() after the trace (the fused launches in tolerance mode)"""
        _check(lib().hr_shadows_denoise(self.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_shadows_denoise")

    def temporal(self, inputs, stream=None):
        _check(lib().hr_shadows_temporal(self.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_shadows_temporal")

    def atrous_iteration(self, inputs, i, stream=None):
        _check(lib().hr_shadows_atrous_iteration(self.h, C.byref(inputs), C.byref(self.params), C.c_int32(i), _stream_ptr(stream)), "hr_shadows_atrous_iteration")

    def upsample(self, inputs, stream=None):
        _check(lib().hr_shadows_upsample(self.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_shadows_upsample")

    def ray_count(self) -> int:
        n = C.c_uint64(0)
        _check(lib().hr_shadows_ray_count(self.h, C.byref(n)), "hr_shadows_ray_count")
        return n.value

    def tile_ray_counts(self) -> np.ndarray:
        """[tiles_y, tiles_x] uint16: rays fired per 8x8 tile by the last ray_trace"""
        tx, ty = C.c_int32(0), C.c_int32(0)
        _check(lib().hr_shadows_tile_ray_counts(self.h, None, C.byref(tx), C.byref(ty)), "hr_shadows_tile_ray_counts")
        out = np.zeros((ty.value, tx.value), np.uint16)
        _check(lib().hr_shadows_tile_ray_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_uint16)), None, None), "hr_shadows_tile_ray_counts")
        return out

    def trace_stats(self, scene, inputs, stream=None, timed=False):
        """(rays, nodes visited, triangles tested) from the instrumented trace kernel.  timed=False: the full walk (occluder cache bypassed);
        timed=True: the kernel render() launches in the pass's present state, cache on (hr_shadows_trace_stats_timed)"""
        out = (C.c_uint64 * 3)()
        fn = lib().hr_shadows_trace_stats_timed if timed else lib().hr_shadows_trace_stats
        _check(fn(self.h, scene.h, C.byref(inputs), C.byref(self.params), out, _stream_ptr(stream)), "hr_shadows_trace_stats")
        return int(out[0]), int(out[1]), int(out[2])


class RayTracedAO(_Pass):
    """src/ray_traced_ao.h:7-126.  ``render(scene, frame_inputs)`` = RayTracedAO::render(cmd_buf)."""
    _prefix = "hr_ao"
    IMG_MASK, IMG_AO0, IMG_AO1, IMG_LEN0, IMG_LEN1, IMG_BLUR0, IMG_BLUR1, IMG_UPSAMPLE, IMG_TILES = range(9)

    def __init__(self, ctx: Context, width: int, height: int, scale: int = SCALE_HALF_RES, band=None):
        self.ctx = ctx
        self.params = hr_ao_params()
        lib().hr_ao_default_params(C.byref(self.params))
        self.h = C.c_void_p()
        b = hr_band(*band) if band else None
        _check(lib().hr_ao_create(ctx.h, C.c_int32(width), C.c_int32(height), C.c_int(scale), C.byref(b) if b else None, C.byref(self.h)), "hr_ao_create")
        self.scale = scale
        self.width, self.height = width >> scale, height >> scale

    def render(self, scene: Scene, inputs: hr_frame_inputs, stream=None):
        _check(lib().hr_ao_render(self.h, scene.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_ao_render")

    def ray_trace(self, scene, inputs, stream=None):
        _check(lib().hr_ao_ray_trace(self.h, scene.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_ao_ray_trace")

    def denoise(self, inputs, stream=None):
        _check(lib().hr_ao_denoise(self.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_ao_denoise")

    def temporal(self, inputs, stream=None):
        _check(lib().hr_ao_temporal(self.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_ao_temporal")

    def blur(self, inputs, which, stream=None):
        _check(lib().hr_ao_blur(self.h, C.byref(inputs), C.byref(self.params), C.c_int32(which), _stream_ptr(stream)), "hr_ao_blur")

    def upsample(self, inputs, stream=None):
        _check(lib().hr_ao_upsample(self.h, C.byref(inputs), C.byref(self.params), _stream_ptr(stream)), "hr_ao_upsample")

    def ray_count(self) -> int:
        n = C.c_uint64(0)
        _check(lib().hr_ao_ray_count(self.h, C.byref(n)), "hr_ao_ray_count")
        return n.value

    def trace_stats(self, scene, inputs, stream=None):
        out = (C.c_uint64 * 3)()
        _check(lib().hr_ao_trace_stats(self.h, scene.h, C.byref(inputs), C.byref(self.params), out, _stream_ptr(stream)), "hr_ao_trace_stats")
        return int(out[0]), int(out[1]), int(out[2])


ABI_SYMBOLS += ["hr_ao_default_params", "hr_ao_create", "hr_ao_render", "hr_ao_output", "hr_ao_reset_history", "hr_ao_destroy", "hr_ao_ray_trace",
                "hr_ao_denoise", "hr_ao_temporal", "hr_ao_blur", "hr_ao_upsample", "hr_ao_image", "hr_ao_history_apron_exceeded", "hr_ao_set_profiling", "hr_ao_get_stage_times", "hr_ao_ray_count",
                "hr_ao_trace_stats", "hr_ao_launch_order"]
