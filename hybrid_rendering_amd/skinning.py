"""Python mirror of include/hr_skin.h: linear-blend skinning and morph targets on the GPU (csrc/skinning.hip; the arithmetic is specified in
hr_skin.h and written once in csrc/skin_math.h).  ``Skin`` owns an hr_skin: ``pose`` fills its device buffers, ``positions`` / ``normals`` view
them as cuda tensors that ``Scene.update_vertices`` and ``InstancedScene.update_meshes`` take as they are.  ``assets.load_gltf_skinned`` reads
the meshes and samples the animations that feed it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .api import HR_MAX_STAGES, _check, _stream_ptr, hr_stage_times, lib

# every symbol include/hr_skin.h declares (tests/test_skin_host.py); kept apart from api.ABI_SYMBOLS
ABI_SYMBOLS = ["hr_skin_check_desc", "hr_skin_create", "hr_skin_destroy", "hr_skin_info", "hr_skin_pose_device", "hr_skin_pose", "hr_skin_output",
               "hr_skin_bounds", "hr_skin_pose_host", "hr_skin_set_profiling", "hr_skin_get_stage_times"]


class hr_skin_desc(C.Structure):
    _fields_ = [("n_tris", C.c_int32), ("n_joints", C.c_int32), ("rest_positions", C.c_void_p), ("rest_normals", C.c_void_p), ("joints", C.c_void_p),
                ("weights", C.c_void_p), ("n_targets", C.c_int32), ("target_positions", C.c_void_p), ("target_normals", C.c_void_p)]


class hr_skin_info_data(C.Structure):
    _fields_ = [("n_tris", C.c_int32), ("n_joints", C.c_int32), ("n_targets", C.c_int32), ("lds_joint_cap", C.c_int32), ("max_weight_sum_error", C.c_float)]


class SkinArrays:
    """The host arrays of a skin, contiguous in the layouts hr_skin_desc names.  ``source``: anything with rest positions and normals (``verts`` /
    ``normals`` or a ``rest`` SceneData), ``joints``, ``weights``, ``n_joints`` and optionally ``target_positions`` / ``target_normals`` — an
    assets.SkinnedMesh, or a dict with those keys."""

    def __init__(self, source):
        get = (lambda k, d=None: source.get(k, d)) if isinstance(source, dict) else (lambda k, d=None: getattr(source, k, d))
        rest = get("rest")
        verts = get("verts") if rest is None else rest.verts
        normals = get("normals") if rest is None else rest.normals
        self.verts = np.ascontiguousarray(verts, np.float32)
        self.normals = np.ascontiguousarray(normals, np.float32)
        self.n_tris = int(self.verts.shape[0])
        assert self.verts.shape == (self.n_tris, 3, 3) and self.normals.shape == self.verts.shape, "rest positions / normals: [n_tris,3,3]"
        self.joints = np.ascontiguousarray(get("joints"), np.uint16)
        self.weights = np.ascontiguousarray(get("weights"), np.float32)
        assert self.joints.shape == (self.n_tris, 3, 4) and self.weights.shape == (self.n_tris, 3, 4), "joints / weights: [n_tris,3,4]"
        self.n_joints = int(get("n_joints"))
        tp, tn = get("target_positions"), get("target_normals")
        self.n_targets = 0 if tp is None else int(np.asarray(tp).shape[0])
        self.target_positions = None if self.n_targets == 0 else np.ascontiguousarray(tp, np.float32)
        self.target_normals = None if (self.n_targets == 0 or tn is None) else np.ascontiguousarray(tn, np.float32)
        for a in (self.target_positions, self.target_normals):
            assert a is None or a.shape == (self.n_targets, self.n_tris, 3, 3), "targets: [n_targets,n_tris,3,3]"

    def desc(self) -> hr_skin_desc:
        p = lambda a: None if a is None else a.ctypes.data
        return hr_skin_desc(self.n_tris, self.n_joints, p(self.verts), p(self.normals), p(self.joints), p(self.weights), self.n_targets,
                            p(self.target_positions), p(self.target_normals))


def _arrays(source) -> SkinArrays:
    return source if isinstance(source, SkinArrays) else SkinArrays(source)


def _host_pose_args(arrays: SkinArrays, matrices, morph_weights):
    m = np.ascontiguousarray(np.asarray(matrices, np.float32).reshape(-1, 16))
    assert m.shape[0] == arrays.n_joints, f"matrices: [{arrays.n_joints},16]"
    w = None
    if morph_weights is not None and arrays.n_targets > 0:
        w = np.ascontiguousarray(np.asarray(morph_weights, np.float32).reshape(-1))
        assert w.shape[0] == arrays.n_targets, f"morph_weights: [{arrays.n_targets}]"
    return m, w


def check_desc(source) -> int:
    """hr_skin_check_desc: the status code (0: fine; 1 = HR_ERR_INVALID_ARG, hr_last_error names the cause).  Host only."""
    a = _arrays(source)
    d = a.desc()
    return int(lib().hr_skin_check_desc(C.byref(d)))


def pose_host(source, matrices, morph_weights=None):
    """hr_skin_pose_host: (positions, normals), each [n_tris,3,3] float32 — the contract on the CPU.  Host only."""
    a = _arrays(source)
    m, w = _host_pose_args(a, matrices, morph_weights)
    d = a.desc()
    op, on = np.zeros_like(a.verts), np.zeros_like(a.verts)
    _check(lib().hr_skin_pose_host(C.byref(d), C.c_void_p(m.ctypes.data), C.c_void_p(w.ctypes.data) if w is not None else None, C.c_void_p(op.ctypes.data),
                                   C.c_void_p(on.ctypes.data)), "hr_skin_pose_host")
    return op, on


class Skin:
    """hr_skin over a context: ``Skin(ctx, skinned_mesh_or_arrays)``."""

    def __init__(self, ctx, source):
        self.ctx, self.arrays = ctx, _arrays(source)
        d = self.arrays.desc()
        self.h = C.c_void_p()
        L = lib()
        L.hr_skin_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _check(L.hr_skin_create(ctx.h if ctx is not None else None, C.byref(d), C.byref(self.h)), "hr_skin_create")
        self._views = None

    def close(self):
        if self.h:
            self._views = None
            lib().hr_skin_destroy(self.h)
            self.h = C.c_void_p()

    def info(self) -> dict:
        i = hr_skin_info_data()
        _check(lib().hr_skin_info(self.h, C.byref(i)), "hr_skin_info")
        return dict(n_tris=i.n_tris, n_joints=i.n_joints, n_targets=i.n_targets, lds_joint_cap=i.lds_joint_cap, max_weight_sum_error=float(i.max_weight_sum_error))

    def pose(self, matrices, morph_weights=None, stream=None):
        """cuda float32 tensors ([n_joints,16], [n_targets] or None) -> hr_skin_pose_device: kernels only, capturable, the tensors are read when
        the launch runs.  numpy / lists -> hr_skin_pose: checked for finite values and staged through the skin's pinned buffer."""
        L, a = lib(), self.arrays
        if hasattr(matrices, "is_cuda"):
            import torch
            assert matrices.is_cuda and matrices.dtype == torch.float32 and matrices.is_contiguous() and matrices.numel() == a.n_joints * 16, \
                f"matrices: contiguous cuda float32 [{a.n_joints},16]"
            mw = None
            if morph_weights is not None and a.n_targets > 0:
                mw = morph_weights
                assert mw.is_cuda and mw.dtype == torch.float32 and mw.is_contiguous() and mw.numel() == a.n_targets, f"morph_weights: contiguous cuda float32 [{a.n_targets}]"
            L.hr_skin_pose_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            _check(L.hr_skin_pose_device(self.h, C.c_void_p(matrices.data_ptr()), C.c_void_p(mw.data_ptr()) if mw is not None else None, _stream_ptr(stream)),
                   "hr_skin_pose_device")
            return self
        m, w = _host_pose_args(a, matrices, morph_weights)
        L.hr_skin_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(L.hr_skin_pose(self.h, C.c_void_p(m.ctypes.data), C.c_void_p(w.ctypes.data) if w is not None else None, _stream_ptr(stream)), "hr_skin_pose")
        return self

    def _outputs(self):
        if self._views is None:
            from .api import hr_image_view, view_to_tensor
            p, n = C.c_void_p(), C.c_void_p()
            _check(lib().hr_skin_output(self.h, C.byref(p), C.byref(n)), "hr_skin_output")
            nt = self.arrays.n_tris
            # a [n_tris][9] R32F image over each buffer: view_to_tensor wraps device memory without copying it
            self._views = tuple(view_to_tensor(hr_image_view(q.value, 9, nt, 36, 5), device=f"cuda:{self.ctx.device}").view(nt, 3, 3) for q in (p, n))
        return self._views

    @property
    def positions(self):
        """cuda float32 [n_tris,3,3] viewing the skin's position buffer (no copy; valid until close())"""
        return self._outputs()[0]

    @property
    def normals(self):
        return self._outputs()[1]

    def bounds(self, matrices, morph_weights=None):
        """hr_skin_bounds: (lo xyz, hi xyz) float32 [2,3], conservative for every position ``pose`` writes with these arguments.  Host only.
        Raises HRError (HR_ERR_UNSUPPORTED) for a skin whose weights do not sum to 1 within 2^-10."""
        m, w = _host_pose_args(self.arrays, matrices, morph_weights)
        out = np.zeros(6, np.float32)
        _check(lib().hr_skin_bounds(self.h, C.c_void_p(m.ctypes.data), C.c_void_p(w.ctypes.data) if w is not None else None, C.c_void_p(out.ctypes.data)), "hr_skin_bounds")
        return out.reshape(2, 3)

    def pose_host(self, matrices, morph_weights=None):
        return pose_host(self.arrays, matrices, morph_weights)

    def set_profiling(self, on=True):
        _check(lib().hr_skin_set_profiling(self.h, C.c_int32(1 if on else 0)), "hr_skin_set_profiling")

    def stage_times(self):
        """[(stage, ms, algorithmic bytes)] since the last call, as the passes report theirs: the stage is skin_pose"""
        t = hr_stage_times()
        _check(lib().hr_skin_get_stage_times(self.h, C.byref(t)), "hr_skin_get_stage_times")
        return [(t.name[i].decode(), float(t.ms[i]), int(t.bytes[i])) for i in range(min(t.n_stages, HR_MAX_STAGES))]
