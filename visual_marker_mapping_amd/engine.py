"""BundleAdjuster: Python handle on the device-resident bundle-adjustment engine (libvmm_ba.so).

This is the flat-array layer under TagReconstructor.doBundleAdjustment; it mirrors what
/root/reference/src/TagReconstructor.cpp:646-743 builds (a ceres::Problem) and solves.
"""
import ctypes as C
import functools

import numpy as np

from . import _lib
from ._lib import (CONVERGENCE, ELIM_AUTO, ELIM_CAMERAS, ELIM_TAGS, FAILURE, LANDMARK_POINTS,  # noqa: F401
                   LANDMARK_TAG_POSES, NO_CONVERGENCE, PRECISION_F32_ACCUM, PRECISION_F64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _fields(cls, skip=()):
    """The field names of a struct class in order, without `reserved` and `skip` (cached: solve() asks per call)."""
    return tuple(k for k, _ in cls._fields_ if k != "reserved" and k not in skip)


def _set_fields(struct, kw, what, nested=None):
    """Sets the keyword fields of an options struct and returns it.  nested = (prefix, member): `<prefix><field>` sets a
    field of that member struct.  An unknown name, `reserved` and the member itself are refused."""
    names = _fields(type(struct), nested[1:] if nested else ())
    for k, v in kw.items():
        if k in names:
            setattr(struct, k, v)
        elif nested and k.startswith(nested[0]) and k[len(nested[0]):] in _fields(type(getattr(struct, nested[1]))):
            setattr(getattr(struct, nested[1]), k[len(nested[0]):], v)
        else:
            raise AttributeError("unknown %s option %r" % (what, k))
    return struct


def _options(cls, default_fn, kw, what, nested=None):
    """An options struct with the library's defaults (vmm_ba_default_*_options), then the keyword fields."""
    o = cls()
    getattr(_lib.lib(), default_fn)(C.byref(o))
    return _set_fields(o, kw, what, nested)


def _struct_dict(s, skip=()):
    """Field -> value in field order, without `reserved`: every report, summary and kernel-times struct."""
    return {k: getattr(s, k) for k in _fields(type(s), skip)}


def _summary(trace_capacity):
    """A vmm_ba_summary for a solve and its optional trace buffer."""
    s, buf = _lib.Summary(), None
    if trace_capacity > 0:
        buf = (_lib.Iteration * trace_capacity)()
        s.trace, s.trace_capacity = buf, trace_capacity
    return s, buf


def _summary_dict(s, buf, capacity):
    out = _struct_dict(s, ("trace", "trace_capacity"))
    out["trace"] = [_struct_dict(buf[i]) for i in range(min(s.iterations, capacity))] if buf is not None else []
    return out


def _model_arrays(intr, dist, rows=None):
    """The camera model as the C entries take it: intr (4,) and dist (5,), or with `rows` one row per camera."""
    lead = () if rows is None else (rows,)
    return (np.ascontiguousarray(intr, np.float64).reshape(lead + (4,)),
            np.ascontiguousarray(dist, np.float64).reshape(lead + (5,)))


def default_options(**kw):
    return _options(_lib.Options, "vmm_ba_default_options", kw, "solver")


class BundleAdjuster:
    def __init__(self, intr, dist, cam_qt, tag_qt, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px,
                 device=0, elimination=ELIM_AUTO, rank=0, world_size=1, precision=PRECISION_F64,
                 landmarks=LANDMARK_TAG_POSES, structure_obs=None):
        L = _lib.lib()
        self._h = C.c_void_p()
        self.intr, self.dist = _model_arrays(intr, dist)
        cam_qt = np.ascontiguousarray(cam_qt, np.float64).reshape(-1, 7)
        tag_qt = np.ascontiguousarray(tag_qt, np.float64).reshape(-1, 7)
        tag_wh = np.ascontiguousarray(tag_wh, np.float64).reshape(-1, 2)
        obs_cam = np.ascontiguousarray(obs_cam, np.int32).reshape(-1)
        obs_tag = np.ascontiguousarray(obs_tag, np.int32).reshape(-1)
        obs_px = np.ascontiguousarray(obs_px, np.float64).reshape(-1, 8)
        if not (len(obs_cam) == len(obs_tag) == len(obs_px)):
            raise ValueError("observation arrays differ in length")
        if len(tag_wh) != len(tag_qt):
            raise ValueError("tag_wh and tag_qt differ in length")
        self.n_cams, self.n_tags, self.n_obs = len(cam_qt), len(tag_qt), len(obs_cam)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        p = _lib.Problem()
        p.intr[:] = list(self.intr)
        p.dist[:] = list(self.dist)
        p.n_cams, p.n_tags = self.n_cams, self.n_tags
        p.cam_qt, p.tag_qt, p.tag_wh = dp(cam_qt), dp(tag_qt), dp(tag_wh)
        p.fixed_tag = int(fixed_tag)
        p.n_obs, p.obs_cam, p.obs_tag, p.obs_px = self.n_obs, ip(obs_cam), ip(obs_tag), dp(obs_px)
        co = _lib.CreateOptions()
        L.vmm_ba_default_create_options(C.byref(co))
        co.device, co.elimination, co.rank, co.world_size = device, elimination, rank, world_size
        co.precision = int(precision)
        co.landmarks = int(landmarks)
        self.landmarks = int(landmarks)
        if structure_obs is not None:
            # world_size > 1: the (camera, tag) pairs of ALL ranks' observations, the same on every rank, so that every
            # rank orders the kept family identically (vmm_ba_create_options.structure_obs_*)
            s_cam = np.ascontiguousarray(structure_obs[0], np.int32).reshape(-1)
            s_tag = np.ascontiguousarray(structure_obs[1], np.int32).reshape(-1)
            if len(s_cam) != len(s_tag):
                raise ValueError("structure_obs arrays differ in length")
            co.n_structure_obs, co.structure_obs_cam, co.structure_obs_tag = len(s_cam), ip(s_cam), ip(s_tag)
        _lib.check(L.vmm_ba_create(C.byref(p), C.byref(co), C.byref(self._h)))
        self._allreduce_cb = None
        self.constant_poses = (None, None)   # the flags of the last set_constant_poses call, as bytes

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().vmm_ba_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- state ----
    def set_state(self, cam_qt=None, tag_qt=None):
        cam = None if cam_qt is None else np.ascontiguousarray(cam_qt, np.float64).reshape(self.n_cams, 7)
        tag = None if tag_qt is None else np.ascontiguousarray(tag_qt, np.float64).reshape(self.n_tags, 7)
        _lib.check(_lib.lib().vmm_ba_set_state(self._h, _ptr(cam), _ptr(tag)))

    def set_observation_mask(self, mask=None):
        """Switches observations off/on (caller's order; None = all on) without rebuilding the handle."""
        if mask is None:
            _lib.check(_lib.lib().vmm_ba_set_observation_mask(self._h, None))
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(-1)
        if len(m) != self.n_obs:
            raise ValueError("mask length differs from the number of observations")
        _lib.check(_lib.lib().vmm_ba_set_observation_mask(self._h, m.ctypes.data_as(C.c_void_p)))

    def set_constant_poses(self, cam_const=None, tag_const=None):
        """Holds poses constant (vmm_ba_set_constant_poses; Ceres' SetParameterBlockConstant): cam_const (n_cams,) and
        tag_const (n_tags,), non-zero = constant, None = no pose of that family.  Replaces any earlier set; the
        problem's fixed tag stays constant regardless.  Every rank of a multi-GPU run passes the same arrays."""
        flags = []
        for name, a, n in (("cam_const", cam_const, self.n_cams), ("tag_const", tag_const, self.n_tags)):
            if a is None:
                flags.append(None)
                continue
            a = np.asarray(a)
            if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
                raise TypeError("%s must be a boolean or integer array, not %s" % (name, a.dtype))
            if a.shape != (n,):
                raise ValueError("%s must have shape (%d,), not %s" % (name, n, a.shape))
            flags.append(np.ascontiguousarray(a != 0, np.uint8))
        _lib.check(_lib.lib().vmm_ba_set_constant_poses(self._h, _ptr(flags[0]), _ptr(flags[1])))
        self.constant_poses = tuple(None if f is None or not f.any() else f.tobytes() for f in flags)

    def get_state(self):
        cam, tag = np.zeros((self.n_cams, 7)), np.zeros((self.n_tags, 7))
        _lib.check(_lib.lib().vmm_ba_get_state(self._h, _ptr(cam), _ptr(tag)))
        return cam, tag

    def get_points(self):
        """LANDMARK_POINTS handles: (n_tags, 4, 3) world corners LL, LR, UR, UL -- the parameter blocks of
        doBundleAdjustment_points (/root/reference/src/TagReconstructor.cpp:485-492)."""
        pts = np.zeros((self.n_tags, 4, 3))
        _lib.check(_lib.lib().vmm_ba_get_points(self._h, _ptr(pts)))
        return pts

    def set_allreduce(self, fn):
        """fn(device_ptr:int, count:int, hip_stream:int) -> None; sum-all-reduce in place."""
        def tramp(_user, buf, count, stream):
            try:
                fn(int(buf), int(count), int(stream or 0))
                return 0
            except Exception:  # surfaced as VMM_BA_ERR_COLLECTIVE by the library
                import traceback
                traceback.print_exc()
                return 1
        self._allreduce_cb = _lib.ALLREDUCE_FN(tramp)
        _lib.check(_lib.lib().vmm_ba_set_allreduce(self._h, self._allreduce_cb, None))

    def enable_rccl(self, unique_id):
        """Native collective path: ncclAllReduce issued by the library on its own stream, recorded into the LM
        iteration's hipGraph.  `unique_id` = the 128 bytes rank 0 drew with rccl_unique_id(), identical on every
        rank; collective call (every rank of the world must make it)."""
        buf = bytes(unique_id)
        if len(buf) != _lib.RCCL_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % _lib.RCCL_ID_BYTES)
        _lib.check(_lib.lib().vmm_ba_enable_rccl(self._h, C.c_char_p(buf)))

    # ---- the hot path ----
    def solve(self, options=None, trace_capacity=0, **kw):
        o = options or default_options(**kw)
        s, buf = _summary(trace_capacity)
        _lib.check(_lib.lib().vmm_ba_solve(self._h, C.byref(o), C.byref(s)))
        return _summary_dict(s, buf, trace_capacity)

    def initialize(self, **options):
        """Initial poses from the detections alone (vmm_ba_initialize): overwrites the device state of every pose
        reachable from the constant poses (the fixed tag, set_constant_poses), whose current poses are kept.
        options: the fields of vmm_ba_init_options (sweeps, min_tag_observations, score_cap_px, refine_iterations).
        Returns (report dict, cam_reached, tag_reached) with boolean masks; unreached poses keep their state."""
        o = _options(_lib.InitOptions, "vmm_ba_default_init_options", options, "initialisation")
        r = _lib.InitReport()
        cam, tag = np.zeros(self.n_cams, np.uint8), np.zeros(self.n_tags, np.uint8)
        _lib.check(_lib.lib().vmm_ba_initialize(self._h, C.byref(o), C.byref(r), _ptr(cam), _ptr(tag)))
        return _struct_dict(r), cam.astype(bool), tag.astype(bool)

    def cost(self, robustify=True, huber_a=1.0):
        c = C.c_double(0)
        _lib.check(_lib.lib().vmm_ba_cost(self._h, int(bool(robustify)), float(huber_a), C.byref(c)))
        return c.value

    def reprojection_stats(self, per_corner=True):
        pc, pt = np.zeros(self.n_cams), np.zeros(self.n_tags)
        avg = C.c_double(0)
        corner = np.zeros((self.n_obs, 8)) if per_corner else None
        _lib.check(_lib.lib().vmm_ba_reprojection_stats(self._h, _ptr(pc), _ptr(pt), C.byref(avg), _ptr(corner)))
        return pc, pt, avg.value, corner

    def tag_translation_covariance(self, robustify=False, huber_a=1.0):
        """(n_tags, 3, 3) covariance blocks of the tag translations at the current state -- the
        ceres::Covariance block of /root/reference/src/TagReconstructor.cpp:744-783."""
        cov = np.zeros((self.n_tags, 3, 3))
        _lib.check(_lib.lib().vmm_ba_tag_translation_covariance(self._h, int(bool(robustify)), float(huber_a),
                                                               _ptr(cov)))
        return cov

    def covariance_blocks(self, pairs, robustify=False, huber_a=1.0):
        """(n_pairs, 6, 6) blocks of (J^T J)^-1 in tangent coordinates (translation, then rotation) at the current state
        for `pairs` = (n_pairs, 2) pose indices, cameras 0 .. n_cams - 1, then tags n_cams .. n_cams + n_tags - 1
        (vmm_ba_covariance_blocks; Ceres' Covariance::Compute + GetCovarianceBlockInTangentSpace).  Equal indices give
        the marginal; a pair that names a constant, origin or residual-free pose gives zeros."""
        pr = np.asarray(pairs, np.int64).reshape(-1, 2)
        if len(pr) and (pr.min() < -2 ** 31 or pr.max() >= 2 ** 31):
            raise ValueError("pose index out of the int32 range")
        a, b = np.ascontiguousarray(pr[:, 0], np.int32), np.ascontiguousarray(pr[:, 1], np.int32)
        cov = np.zeros((len(pr), 6, 6))
        _lib.check(_lib.lib().vmm_ba_covariance_blocks(self._h, int(bool(robustify)), float(huber_a), len(pr), _ptr(a),
                                                       _ptr(b), _ptr(cov)))
        return cov

    def pose_covariances(self, robustify=False, huber_a=1.0):
        """(cam_cov (n_cams, 6, 6), tag_cov (n_tags, 6, 6)): the 6x6 marginal of every pose, one covariance_blocks call."""
        idx = np.arange(self.n_cams + self.n_tags)
        cov = self.covariance_blocks(np.stack([idx, idx], axis=1), robustify, huber_a)
        return cov[:self.n_cams], cov[self.n_cams:]

    def tag_joint_covariance(self, robustify=False, huber_a=1.0):
        """(n_tags, n_tags, 6, 6): the tags' joint covariance, block [s, t] the cross block of tags s and t in tangent
        order.  One covariance_blocks call for the pairs s >= t; the upper block triangle is filled here by transposition,
        so that the array, read as a 6 n_tags x 6 n_tags matrix, is symmetric.  What predict_localization's
        tag_cov_joint takes."""
        T = self.n_tags
        s, t = np.tril_indices(T)
        cov = self.covariance_blocks(np.stack([self.n_cams + s, self.n_cams + t], axis=1), robustify, huber_a)
        out = np.zeros((T, T, 6, 6))
        out[t, s] = np.swapaxes(cov, 1, 2)
        out[s, t] = cov   # last: the diagonal blocks as the call gave them
        return out

    # ---- the camera model ----
    def set_intrinsics(self, intr, dist):
        """Replaces the handle's camera model (vmm_ba_set_intrinsics): every later call behaves as a handle created with
        it; the next solve captures its iteration graph again."""
        intr, dist = _model_arrays(intr, dist)
        _lib.check(_lib.lib().vmm_ba_set_intrinsics(self._h, _ptr(intr), _ptr(dist)))
        self.intr, self.dist = intr.copy(), dist.copy()

    def get_intrinsics(self):
        intr, dist = np.zeros(4), np.zeros(5)
        _lib.check(_lib.lib().vmm_ba_get_intrinsics(self._h, _ptr(intr), _ptr(dist)))
        return intr, dist

    def intrinsics_system(self, robustify=True, huber_a=1.0):
        """The camera-model part of the joint problem at the current state (vmm_ba_intrinsics_system): cost, g_k = Jk' r
        and C = Jk' Jk over the active observations, and the reduced system with every pose eliminated,
        r_k = g_k - B' A^-1 g and S_k = C - B' A^-1 B.  inv(S_k) is the covariance of the nine parameters."""
        c = C.c_double(0)
        gk, Ck, rk, Sk = np.zeros(9), np.zeros((9, 9)), np.zeros(9), np.zeros((9, 9))
        _lib.check(_lib.lib().vmm_ba_intrinsics_system(self._h, int(bool(robustify)), float(huber_a), C.byref(c),
                                                       _ptr(gk), _ptr(Ck), _ptr(rk), _ptr(Sk)))
        return {"cost": c.value, "g_k": gk, "C": Ck, "r_k": rk, "S_k": Sk}

    def solve_selfcal(self, options=None, trace_capacity=0, max_outer_iterations=None, refine_mask=None,
                      parameter_tolerance=None, function_tolerance=None, **kw):
        """Bundle adjustment with the camera model refined (vmm_ba_solve_selfcal).  options / **kw: the inner solver's
        options as solve() takes them; the four named arguments are the fields of vmm_ba_selfcal_options.
        Returns (intr, dist, intr_cov (9, 9), report dict, summary of the last inner solve as solve() returns it)."""
        o = options or default_options(**kw)
        named = dict(max_outer_iterations=max_outer_iterations, refine_mask=refine_mask,
                     parameter_tolerance=parameter_tolerance, function_tolerance=function_tolerance)
        so = _options(_lib.SelfcalOptions, "vmm_ba_default_selfcal_options",
                      {k: v for k, v in named.items() if v is not None}, "self-calibration")
        (s, buf), r = _summary(trace_capacity), _lib.SelfcalReport()
        intr, dist, cov = np.zeros(4), np.zeros(5), np.zeros((9, 9))
        _lib.check(_lib.lib().vmm_ba_solve_selfcal(self._h, C.byref(o), C.byref(so), C.byref(s), C.byref(r), _ptr(intr),
                                                   _ptr(dist), _ptr(cov)))
        self.intr, self.dist = intr.copy(), dist.copy()
        return intr, dist, cov, _struct_dict(r), _summary_dict(s, buf, trace_capacity)

    # ---- diagnostics ----
    def eval_blocks(self, robustify=True, huber_a=1.0, want_W=True):
        V, U = np.zeros((self.n_cams, 6, 6)), np.zeros((self.n_tags, 6, 6))
        W = np.zeros((self.n_obs, 6, 6)) if want_W else None
        gc, gt = np.zeros((self.n_cams, 6)), np.zeros((self.n_tags, 6))
        if self.landmarks == LANDMARK_POINTS:   # the landmark-side blocks live in the library's point-pair index space
            U = W = gt = None
        c = C.c_double(0)
        _lib.check(_lib.lib().vmm_ba_eval_blocks(self._h, int(bool(robustify)), float(huber_a), C.byref(c),
                                                 _ptr(V), _ptr(U), _ptr(W), _ptr(gc), _ptr(gt)))
        return {"cost": c.value, "V": V, "U": U, "W": W, "g_cam": gc, "g_tag": gt}

    def debug_overlap(self, reps=10):
        """ms of: rank-k update + sum alone, factorisation + solves alone, both back to back, both at once on two streams."""
        out = np.zeros(8)
        _lib.check(_lib.lib().vmm_ba_debug_overlap(self._h, int(reps), _ptr(out)))
        return dict(zip(("syrk_ms", "cholesky_ms", "sequential_ms", "concurrent_ms", "cholesky_in_concurrent_ms",
                         "syrk_in_concurrent_ms", "concurrent_syrk_first_ms", "cholesky_in_concurrent_syrk_first_ms"), out.tolist()))

    def time_kernels(self, options=None, reps=5):
        o = options or default_options()
        t = _lib.KernelTimes()
        _lib.check(_lib.lib().vmm_ba_time_kernels(self._h, C.byref(o), int(reps), C.byref(t)))
        return _struct_dict(t)


_PROBLEM_ARGS = ("intr", "dist", "cam_qt", "tag_qt", "tag_wh", "fixed_tag", "obs_cam", "obs_tag", "obs_px")


def _const_flags(flags, sizes, what):
    """The constant flags of a batch as vmm_ba_solve_small takes them: one array per problem (or None) -> one uint8
    array over all problems, or None when no problem names a constant pose."""
    if flags is None:
        return None
    if len(flags) != len(sizes):
        raise ValueError("%s needs one entry per problem" % what)
    out = []
    for a, n in zip(flags, sizes):
        if a is None:
            out.append(np.zeros(n, np.uint8))
            continue
        a = np.asarray(a)
        if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
            raise TypeError("%s must hold boolean or integer arrays, not %s" % (what, a.dtype))
        if a.shape != (n,):
            raise ValueError("%s: an entry must have shape (%d,), not %s" % (what, n, a.shape))
        out.append(np.ascontiguousarray(a != 0, np.uint8))
    return np.ascontiguousarray(np.concatenate(out))


def solve_small(problems, cam_const=None, tag_const=None, options=None, elimination=ELIM_AUTO, trace_capacity=0, device=0):
    """Many independent small bundle adjustments in one launch (vmm_ba_solve_small): one workgroup runs the whole
    Levenberg-Marquardt loop of one problem.  problems: a list of dicts or tuples with the arguments of
    BundleAdjuster.__init__ (intr, dist, cam_qt, tag_qt, tag_wh, fixed_tag, obs_cam, obs_tag, obs_px); the family that
    is not eliminated may have at most _lib.SMALL_MAX_KEPT poses.  cam_const / tag_const: None, or one entry per problem
    (an array of flags as BundleAdjuster.set_constant_poses takes it, or None).  Returns a list of
    (cam_qt, tag_qt, summary) per problem, the summary in the vocabulary of BundleAdjuster.solve."""
    n = len(problems)
    if n == 0:
        return []
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    ps, keep = (_lib.Problem * n)(), []
    for p, src in zip(ps, problems):
        v = [src[k] for k in _PROBLEM_ARGS] if isinstance(src, dict) else list(src)
        if len(v) != len(_PROBLEM_ARGS):
            raise ValueError("a problem needs %s" % ", ".join(_PROBLEM_ARGS))
        intr, dist = _model_arrays(v[0], v[1])
        cam_qt = np.ascontiguousarray(v[2], np.float64).reshape(-1, 7)
        tag_qt = np.ascontiguousarray(v[3], np.float64).reshape(-1, 7)
        tag_wh = np.ascontiguousarray(v[4], np.float64).reshape(-1, 2)
        obs_cam = np.ascontiguousarray(v[6], np.int32).reshape(-1)
        obs_tag = np.ascontiguousarray(v[7], np.int32).reshape(-1)
        obs_px = np.ascontiguousarray(v[8], np.float64).reshape(-1, 8)
        if not (len(obs_cam) == len(obs_tag) == len(obs_px)):
            raise ValueError("observation arrays differ in length")
        if len(tag_wh) != len(tag_qt):
            raise ValueError("tag_wh and tag_qt differ in length")
        keep.append((cam_qt, tag_qt, tag_wh, obs_cam, obs_tag, obs_px))
        p.intr[:] = list(intr)
        p.dist[:] = list(dist)
        p.n_cams, p.n_tags = len(cam_qt), len(tag_qt)
        p.cam_qt, p.tag_qt, p.tag_wh = dp(cam_qt), dp(tag_qt), dp(tag_wh)
        p.fixed_tag = int(v[5])
        p.n_obs, p.obs_cam, p.obs_tag, p.obs_px = len(obs_cam), ip(obs_cam), ip(obs_tag), dp(obs_px)
    cc = _const_flags(cam_const, [p.n_cams for p in ps], "cam_const")
    tc = _const_flags(tag_const, [p.n_tags for p in ps], "tag_const")
    cam = np.zeros((sum(p.n_cams for p in ps), 7))
    tag = np.zeros((sum(p.n_tags for p in ps), 7))
    ss, bufs = (_lib.Summary * n)(), []
    for s in ss:
        buf = None
        if trace_capacity > 0:
            buf = (_lib.Iteration * trace_capacity)()
            s.trace, s.trace_capacity = buf, trace_capacity
        bufs.append(buf)
    o = options or default_options()
    _lib.check(_lib.lib().vmm_ba_solve_small(n, ps, _ptr(cc), _ptr(tc), C.byref(o), int(elimination), _ptr(cam), _ptr(tag),
                                             ss, int(device)))
    out, c0, t0 = [], 0, 0
    for p, s, buf in zip(ps, ss, bufs):
        out.append((cam[c0:c0 + p.n_cams].copy(), tag[t0:t0 + p.n_tags].copy(), _summary_dict(s, buf, trace_capacity)))
        c0, t0 = c0 + p.n_cams, t0 + p.n_tags
    return out


def joint_covariance(caa, cab, cbb):
    """The 12x12 covariance [[Caa, Cab], [Cab^T, Cbb]] of two poses from their marginals and their cross block."""
    caa, cab, cbb = (np.asarray(m, np.float64).reshape(6, 6) for m in (caa, cab, cbb))
    return np.block([[caa, cab], [cab.T, cbb]])


def rccl_available():
    """True when librccl.so was resolved in this process (vmm_ba_rccl_available; no device call)."""
    return bool(_lib.lib().vmm_ba_rccl_available())


def rccl_unique_id():
    """128 bytes identifying a new RCCL communicator (ncclGetUniqueId); drawn on rank 0, handed to every rank."""
    buf = C.create_string_buffer(_lib.RCCL_ID_BYTES)
    _lib.check(_lib.lib().vmm_ba_rccl_unique_id(buf))
    return buf.raw


def project_points(intr, dist, points_cam, device=0):
    """CameraModel::projectPoint (/root/reference/src/CameraModel.cpp:6-26) for an (n,3) batch."""
    intr, dist = _model_arrays(intr, dist)
    pts = np.ascontiguousarray(points_cam, np.float64).reshape(-1, 3)
    uv = np.zeros((len(pts), 2))
    _lib.check(_lib.lib().vmm_ba_project_points(_ptr(intr), _ptr(dist), len(pts), _ptr(pts), _ptr(uv), device))
    return uv


def quad_poses(intr, dist, tag_wh, obs_px, device=0):
    """Both planar tag->camera poses of n tag observations from each tag's own four corners (vmm_ba_quad_poses; the
    role of solvePnPEigen at src/TagReconstructor.cpp:208 of the reference).  tag_wh (n, 2), obs_px (n, 8).
    Returns qt2 (n, 2, 7), lower RMS first, and rms2 (n, 2) in pixels (+inf: degenerate)."""
    intr, dist = _model_arrays(intr, dist)
    px = np.ascontiguousarray(obs_px, np.float64).reshape(-1, 8)
    wh = np.ascontiguousarray(tag_wh, np.float64).reshape(-1, 2)
    if len(wh) != len(px):
        raise ValueError("tag_wh and obs_px differ in length")
    qt2, rms2 = np.zeros((len(px), 2, 7)), np.zeros((len(px), 2))
    _lib.check(_lib.lib().vmm_ba_quad_poses(_ptr(intr), _ptr(dist), len(px), _ptr(wh), _ptr(px), _ptr(qt2), _ptr(rms2),
                                            device))
    return qt2, rms2


def default_localize_options(**kw):
    return _options(_lib.LocalizeOptions, "vmm_ba_default_localize_options", kw, "localisation")


# one result layout for images, frames and points
assert _lib.LocalizeResult._fields_ == _lib.TriangulateResult._fields_


def _results(n):
    """n vmm_ba_localize_result (or vmm_ba_triangulate_result) as one structured array, handed to C by pointer."""
    return np.zeros(n, np.dtype(_lib.LocalizeResult))


def _result_dicts(arr):
    """One dict per item of _results: status, n_obs, n_inlier_obs, trials, rms_px, cost."""
    return [dict(zip(arr.dtype.names, row)) for row in arr.tolist()]


def _map_batch_arrays(tag_qt, tag_wh, img_start, obs_tag, obs_px):
    """The map and the batch of images as vmm_ba_localize and vmm_ba_calibrate take them: contiguous arrays of the C
    types, refused when their lengths do not fit together."""
    tag_qt = np.ascontiguousarray(tag_qt, np.float64).reshape(-1, 7)
    tag_wh = np.ascontiguousarray(tag_wh, np.float64).reshape(-1, 2)
    img_start = np.ascontiguousarray(img_start, np.int64).reshape(-1)
    obs_tag = np.ascontiguousarray(obs_tag, np.int32).reshape(-1)
    obs_px = np.ascontiguousarray(obs_px, np.float64).reshape(-1, 8)
    if len(tag_wh) != len(tag_qt):
        raise ValueError("tag_wh and tag_qt differ in length")
    if len(obs_tag) != len(obs_px):
        raise ValueError("observation arrays differ in length")
    if len(img_start) < 1 or img_start[-1] != len(obs_tag):
        raise ValueError("img_start must have n_imgs + 1 entries and end at the number of observations")
    return tag_qt, tag_wh, img_start, obs_tag, obs_px


def localize(intr, dist, tag_qt, tag_wh, img_start, obs_tag, obs_px, device=0, **options):
    """Poses of a batch of images against a finished map (vmm_ba_localize; the batch form of
    TagReconstructor::computeRelativeCameraPoseFromImg, src/TagReconstructor.cpp:280-312 of the reference).
    tag_qt (n_tags, 7) tag->world and tag_wh (n_tags, 2): the map.  img_start (n_imgs + 1,): image i owns the
    observations [img_start[i], img_start[i + 1]) of obs_tag (n_obs,) and obs_px (n_obs, 8).  options: the fields of
    vmm_ba_localize_options.  Returns (cam_qt (n_imgs, 7) world->camera, cam_cov (n_imgs, 6, 6), obs_inlier (n_obs,)
    bool, results: one dict per image with status, n_obs, n_inlier_obs, trials, rms_px, cost)."""
    intr, dist = _model_arrays(intr, dist)
    tag_qt, tag_wh, img_start, obs_tag, obs_px = _map_batch_arrays(tag_qt, tag_wh, img_start, obs_tag, obs_px)
    o = default_localize_options(**options)
    n_imgs = len(img_start) - 1
    cam_qt, cam_cov = np.zeros((n_imgs, 7)), np.zeros((n_imgs, 6, 6))
    inl, res = np.zeros(len(obs_tag), np.uint8), _results(n_imgs)
    _lib.check(_lib.lib().vmm_ba_localize(_ptr(intr), _ptr(dist), len(tag_qt), _ptr(tag_qt), _ptr(tag_wh), n_imgs,
                                          _ptr(img_start), _ptr(obs_tag), _ptr(obs_px), C.byref(o), _ptr(cam_qt),
                                          _ptr(cam_cov), _ptr(inl), _ptr(res), device))
    return cam_qt, cam_cov, inl.astype(bool), _result_dicts(res)


def _rig_arrays(intr, dist, ext_qt, tag_qt, tag_wh, img_start, obs_tag, obs_px):
    """The models and extrinsics of a rig's K cameras, the map and the batch of frames as vmm_ba_rig_localize takes them;
    returns the eight arrays, K and the number of frames."""
    intr, dist = _model_arrays(intr, dist, -1)
    ext_qt = np.ascontiguousarray(ext_qt, np.float64).reshape(-1, 7)
    if not len(intr) == len(dist) == len(ext_qt):
        raise ValueError("intr, dist and ext_qt must have one row per camera of the rig")
    tag_qt, tag_wh, img_start, obs_tag, obs_px = _map_batch_arrays(tag_qt, tag_wh, img_start, obs_tag, obs_px)
    n_rig_cams, n_slots = len(ext_qt), len(img_start) - 1
    if n_rig_cams < 1 or n_slots % n_rig_cams:
        raise ValueError("img_start must have n_frames * K + 1 entries for the K >= 1 cameras of the rig")
    return intr, dist, ext_qt, tag_qt, tag_wh, img_start, obs_tag, obs_px, n_rig_cams, n_slots // n_rig_cams


def rig_localize(intr, dist, ext_qt, tag_qt, tag_wh, img_start, obs_tag, obs_px, device=0, **options):
    """Poses of a rig of K rigidly mounted cameras, one per frame, against a finished map (vmm_ba_rig_localize).
    intr (K, 4), dist (K, 5): one model per camera; ext_qt (K, 7): rig->camera.  The map and the observations as
    engine.localize takes them, image (f, c) being slot f * K + c of img_start (n_frames * K + 1,); a missing image is an
    empty range.  options: the fields of vmm_ba_localize_options.  Returns (rig_qt (n_frames, 7) world->rig, rig_cov
    (n_frames, 6, 6), obs_inlier (n_obs,) bool, results: one dict per frame as engine.localize gives per image)."""
    intr, dist, ext_qt, tag_qt, tag_wh, img_start, obs_tag, obs_px, n_rig_cams, n_frames = _rig_arrays(
        intr, dist, ext_qt, tag_qt, tag_wh, img_start, obs_tag, obs_px)
    o = default_localize_options(**options)
    rig_qt, rig_cov = np.zeros((n_frames, 7)), np.zeros((n_frames, 6, 6))
    inl, res = np.zeros(len(obs_tag), np.uint8), _results(n_frames)
    _lib.check(_lib.lib().vmm_ba_rig_localize(n_rig_cams, _ptr(intr), _ptr(dist), _ptr(ext_qt), len(tag_qt), _ptr(tag_qt),
                                              _ptr(tag_wh), n_frames, _ptr(img_start), _ptr(obs_tag), _ptr(obs_px),
                                              C.byref(o), _ptr(rig_qt), _ptr(rig_cov), _ptr(inl), _ptr(res), device))
    return rig_qt, rig_cov, inl.astype(bool), _result_dicts(res)


def default_rig_calibrate_options(**kw):
    """vmm_ba_rig_calibrate_options with its defaults; keywords are its fields, `loc_<field>` sets a field of the initial
    localisation's options."""
    return _options(_lib.RigCalibrateOptions, "vmm_ba_default_rig_calibrate_options", kw, "rig calibration", ("loc_", "loc"))


def rig_calibrate(intr, dist, ext_qt0, tag_qt, tag_wh, img_start, obs_tag, obs_px, device=0, **options):
    """The extrinsics of a rig's cameras and one rig pose per frame from a batch of frames of a finished map, the map and
    the camera models held fixed (vmm_ba_rig_calibrate).  Arguments as engine.rig_localize, ext_qt0 (K, 7) the starting
    extrinsics; options: the fields of vmm_ba_rig_calibrate_options (`refine_mask`: bit c = extrinsic c is refined,
    default every camera but 0), `loc_<field>` for those of the initial localisation.  Returns (ext_qt (K, 7), ext_cov
    (6 K, 6 K), rig_qt (n_frames, 7), rig_cov (n_frames, 6, 6) the joint marginals, obs_inlier (n_obs,) bool, results:
    one dict per frame, report: dict of vmm_ba_rig_calibrate_report)."""
    intr, dist, ext_qt0, tag_qt, tag_wh, img_start, obs_tag, obs_px, n_rig_cams, n_frames = _rig_arrays(
        intr, dist, ext_qt0, tag_qt, tag_wh, img_start, obs_tag, obs_px)
    o = default_rig_calibrate_options(**options)
    ext_qt, ext_cov = np.zeros((n_rig_cams, 7)), np.zeros((6 * n_rig_cams, 6 * n_rig_cams))
    rig_qt, rig_cov = np.zeros((n_frames, 7)), np.zeros((n_frames, 6, 6))
    inl, res, rep = np.zeros(len(obs_tag), np.uint8), _results(n_frames), _lib.RigCalibrateReport()
    _lib.check(_lib.lib().vmm_ba_rig_calibrate(n_rig_cams, _ptr(intr), _ptr(dist), _ptr(ext_qt0), len(tag_qt), _ptr(tag_qt),
                                               _ptr(tag_wh), n_frames, _ptr(img_start), _ptr(obs_tag), _ptr(obs_px),
                                               C.byref(o), _ptr(ext_qt), _ptr(ext_cov), _ptr(rig_qt), _ptr(rig_cov),
                                               _ptr(inl), _ptr(res), C.byref(rep), device))
    return ext_qt, ext_cov, rig_qt, rig_cov, inl.astype(bool), _result_dicts(res), _struct_dict(rep)


def _pose_matrix(qt):
    w, x, y, z = qt[:4] / np.linalg.norm(qt[:4])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, np.asarray(qt[4:], np.float64)


def rig_extrinsics_start(n_rig_cams, n_frames, cam_qt, results):
    """Starting extrinsics of a rig from the poses of its images, each localised on its own (host numpy, no device call).
    cam_qt (n_frames * K, 7) and results: what engine.localize returned for the images in slot order f * K + c, each
    camera under its own model.  Camera 0 is the rig.  For each camera c > 0, of the frames in which images (f, 0) and
    (f, c) are both LOC_OK the one with the most inlier observations over the two images (ties: the lowest frame) gives
    ext_c = cam(f, c) o cam(f, 0)^-1.  Returns ext_qt (K, 7); raises ValueError naming the camera that never shares a
    localised frame with camera 0."""
    from .pnp import quat_from_R
    cam_qt = np.asarray(cam_qt, np.float64).reshape(n_frames * n_rig_cams, 7)
    if len(results) != n_frames * n_rig_cams:
        raise ValueError("results must have one entry per image, n_frames * K")
    ext_qt = np.zeros((n_rig_cams, 7))
    ext_qt[:, 0] = 1.0
    for c in range(1, n_rig_cams):
        best, best_f = -1, -1
        for f in range(n_frames):
            r0, rc = results[f * n_rig_cams], results[f * n_rig_cams + c]
            if r0["status"] != _lib.LOC_OK or rc["status"] != _lib.LOC_OK:
                continue
            n = r0["n_inlier_obs"] + rc["n_inlier_obs"]
            if n > best:
                best, best_f = n, f
        if best_f < 0:
            raise ValueError("camera %d of the rig shares no localised frame with camera 0: no starting extrinsic" % c)
        R0, t0 = _pose_matrix(cam_qt[best_f * n_rig_cams])
        Rc, tc = _pose_matrix(cam_qt[best_f * n_rig_cams + c])
        R = Rc @ R0.T
        ext_qt[c, :4] = quat_from_R(R)
        ext_qt[c, 4:] = tc - R @ t0
    return ext_qt


def default_calibrate_options(**kw):
    """vmm_ba_calibrate_options with its defaults; keywords are its fields, `loc_<field>` sets a field of the initial
    localisation's options (vmm_ba_calibrate_options.loc)."""
    return _options(_lib.CalibrateOptions, "vmm_ba_default_calibrate_options", kw, "calibration", ("loc_", "loc"))


def calibrate(intr0, dist0, tag_qt, tag_wh, img_start, obs_tag, obs_px, device=0, **options):
    """The camera model (fx, fy, cx, cy | k1, k2, p1, p2, k3) and one pose per image from a batch of images of a finished
    map, the map held fixed (vmm_ba_calibrate).  intr0 (4,), dist0 (5,): the starting model; the map and the
    observations as engine.localize takes them.  options: the fields of vmm_ba_calibrate_options, `loc_<field>` for
    those of the initial localisation.  Returns (intr (4,), dist (5,), intr_cov (9, 9), cam_qt (n_imgs, 7) world->camera,
    cam_cov (n_imgs, 6, 6) the joint marginals, obs_inlier (n_obs,) bool, results: one dict per image as
    engine.localize, report: dict of vmm_ba_calibrate_report)."""
    intr0, dist0 = _model_arrays(intr0, dist0)
    tag_qt, tag_wh, img_start, obs_tag, obs_px = _map_batch_arrays(tag_qt, tag_wh, img_start, obs_tag, obs_px)
    o = default_calibrate_options(**options)
    n_imgs = len(img_start) - 1
    intr, dist, intr_cov = np.zeros(4), np.zeros(5), np.zeros((9, 9))
    cam_qt, cam_cov = np.zeros((n_imgs, 7)), np.zeros((n_imgs, 6, 6))
    inl, res, rep = np.zeros(len(obs_tag), np.uint8), _results(n_imgs), _lib.CalibrateReport()
    _lib.check(_lib.lib().vmm_ba_calibrate(_ptr(intr0), _ptr(dist0), len(tag_qt), _ptr(tag_qt), _ptr(tag_wh), n_imgs,
                                           _ptr(img_start), _ptr(obs_tag), _ptr(obs_px), C.byref(o), _ptr(intr), _ptr(dist),
                                           _ptr(intr_cov), _ptr(cam_qt), _ptr(cam_cov), _ptr(inl), _ptr(res),
                                           C.byref(rep), device))
    return intr, dist, intr_cov, cam_qt, cam_cov, inl.astype(bool), _result_dicts(res), _struct_dict(rep)


def default_triangulate_options(**kw):
    return _options(_lib.TriangulateOptions, "vmm_ba_default_triangulate_options", kw, "triangulation")


def _known_camera_arrays(cam_qt, cam_cov, start, obs_cam, obs, width, what, n_items=None):
    """Known cameras and a list of items over them as vmm_ba_triangulate and vmm_ba_locate_tags take them: contiguous
    arrays of the C types (obs: `width` numbers per observation; cam_cov may be None), refused when their lengths do
    not fit together.  what: the names of the start array and of its item count, for the error text."""
    cam_qt = np.ascontiguousarray(cam_qt, np.float64).reshape(-1, 7)
    start = np.ascontiguousarray(start, np.int64).reshape(-1)
    obs_cam = np.ascontiguousarray(obs_cam, np.int32).reshape(-1)
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, width)
    if len(obs_cam) != len(obs):
        raise ValueError("observation arrays differ in length")
    n = len(start) - 1 if n_items is None else n_items
    if n < 0 or len(start) != n + 1 or start[-1] != len(obs_cam):
        raise ValueError("%s must have %s + 1 entries and end at the number of observations" % what)
    if cam_cov is not None:
        cam_cov = np.ascontiguousarray(cam_cov, np.float64).reshape(-1, 6, 6)
        if len(cam_cov) != len(cam_qt):
            raise ValueError("cam_cov and cam_qt differ in length")
    return cam_qt, cam_cov, start, obs_cam, obs


def _flags_and_results(n_obs, n_items):
    """The inlier flags (uint8, one per observation) and the result records (one per item) that an entry fills."""
    return np.zeros(n_obs, np.uint8), _results(n_items)


def triangulate(intr, dist, cam_qt, pt_start, obs_cam, obs_uv, cam_cov=None, device=0, **options):
    """Free points (anything that is not a tag) from the cameras of a finished map or of a localisation
    (vmm_ba_triangulate).  cam_qt (n_cams, 7) world->camera.  pt_start (n_pts + 1,): point p owns the observations
    [pt_start[p], pt_start[p + 1]) of obs_cam (n_obs,), strictly increasing within a point, and obs_uv (n_obs, 2).
    cam_cov (n_cams, 6, 6), optional: the cameras' marginal covariances in tangent order.  options: the fields of
    vmm_ba_triangulate_options.  Returns (xyz (n_pts, 3), xyz_cov (n_pts, 3, 3) the part the pixel noise causes,
    xyz_cov_cams (n_pts, 3, 3) the part propagated from cam_cov, camera by camera without their correlations (zeros
    without cam_cov), obs_inlier (n_obs,) bool, results: one dict per point with status, n_obs, n_inlier_obs, trials,
    rms_px, cost)."""
    intr, dist = _model_arrays(intr, dist)
    cam_qt, cam_cov, pt_start, obs_cam, obs_uv = _known_camera_arrays(cam_qt, cam_cov, pt_start, obs_cam, obs_uv, 2,
                                                                      ("pt_start", "n_pts"))
    o = default_triangulate_options(**options)
    n_pts = len(pt_start) - 1
    xyz, cov, cov_cams = np.zeros((n_pts, 3)), np.zeros((n_pts, 3, 3)), np.zeros((n_pts, 3, 3))
    inl, res = _flags_and_results(len(obs_cam), n_pts)
    _lib.check(_lib.lib().vmm_ba_triangulate(_ptr(intr), _ptr(dist), len(cam_qt), _ptr(cam_qt), _ptr(cam_cov), n_pts,
                                             _ptr(pt_start), _ptr(obs_cam), _ptr(obs_uv), C.byref(o), _ptr(xyz), _ptr(cov),
                                             _ptr(cov_cams), _ptr(inl), _ptr(res), device))
    return xyz, cov, cov_cams, inl.astype(bool), _result_dicts(res)


def locate_tags(intr, dist, cam_qt, tag_wh, tag_start, obs_cam, obs_px, cam_cov=None, device=0, **options):
    """Poses of a batch of tags from cameras that are already known (vmm_ba_locate_tags, the dual of engine.localize).
    cam_qt (n_cams, 7) world->camera; tag_wh (n_tags, 2).  tag_start (n_tags + 1,): tag t owns the observations
    [tag_start[t], tag_start[t + 1]) of obs_cam (n_obs,), strictly increasing within a tag, and obs_px (n_obs, 8).
    cam_cov (n_cams, 6, 6), optional: the cameras' marginal covariances in tangent order.  options: the fields of
    vmm_ba_localize_options; min_inlier_tags counts the tag's inlier observations.  Returns (tag_qt (n_tags, 7)
    tag->world, tag_cov (n_tags, 6, 6) the part the pixel noise causes, tag_cov_cams (n_tags, 6, 6) the part propagated
    from cam_cov, camera by camera without their correlations (zeros without cam_cov), obs_inlier (n_obs,) bool, results:
    one dict per tag as engine.localize gives per image)."""
    intr, dist = _model_arrays(intr, dist)
    tag_wh = np.ascontiguousarray(tag_wh, np.float64).reshape(-1, 2)
    n_tags = len(tag_wh)
    cam_qt, cam_cov, tag_start, obs_cam, obs_px = _known_camera_arrays(cam_qt, cam_cov, tag_start, obs_cam, obs_px, 8,
                                                                       ("tag_start", "n_tags"), n_tags)
    o = default_localize_options(**options)
    tag_qt, cov, cov_cams = np.zeros((n_tags, 7)), np.zeros((n_tags, 6, 6)), np.zeros((n_tags, 6, 6))
    inl, res = _flags_and_results(len(obs_cam), n_tags)
    _lib.check(_lib.lib().vmm_ba_locate_tags(_ptr(intr), _ptr(dist), len(cam_qt), _ptr(cam_qt), _ptr(cam_cov), n_tags,
                                             _ptr(tag_wh), _ptr(tag_start), _ptr(obs_cam), _ptr(obs_px), C.byref(o),
                                             _ptr(tag_qt), _ptr(cov), _ptr(cov_cams), _ptr(inl), _ptr(res), device))
    return tag_qt, cov, cov_cams, inl.astype(bool), _result_dicts(res)


def default_predict_options(**kw):
    return _options(_lib.PredictOptions, "vmm_ba_default_predict_options", kw, "prediction")


def predict_localization(intr, dist, tag_qt, tag_wh, cam_qt, image_size, tag_cov=None, device=0, want_visible=False,
                         tag_cov_joint=None, visible_in=None, **options):
    """How well a camera would be localised against a finished map at poses that have no image behind them
    (vmm_ba_predict_localization).  tag_qt (n_tags, 7) tag->world and tag_wh (n_tags, 2): the map.  cam_qt (n_poses, 7)
    world->camera.  image_size: (width, height) in pixels.  tag_cov (n_tags, 6, 6), optional: the tags' marginal
    covariances in tangent order.  options: the other fields of vmm_ba_predict_options.  Returns (cov_px (n_poses, 6, 6)
    the covariance the pixel noise causes, cov_map (n_poses, 6, 6) the part propagated from tag_cov, tag by tag without
    their correlations (zeros without tag_cov), results: one dict per pose with status, n_visible, sigma_pos_m,
    sigma_rot_rad) and, with want_visible, visible (n_poses, n_tags) bool as a fourth.  Occlusion is not modelled.
    tag_cov_joint (n_tags, n_tags, 6, 6) or anything that reshapes to it, instead of tag_cov: the tags' joint covariance
    (BundleAdjuster.tag_joint_covariance); cov_map then holds the part propagated with the correlations between the tags
    (vmm_ba_predict_localization_joint; only the blocks [s, t] with s >= t are read).  visible_in (n_poses, n_tags), only
    with tag_cov_joint: the tags that take part in every pose, instead of the visibility rules."""
    if tag_cov is not None and tag_cov_joint is not None:
        raise ValueError("tag_cov and tag_cov_joint are given both: a map has one covariance")
    if visible_in is not None and tag_cov_joint is None:
        raise ValueError("visible_in needs tag_cov_joint")
    intr, dist = _model_arrays(intr, dist)
    tag_qt = np.ascontiguousarray(tag_qt, np.float64).reshape(-1, 7)
    tag_wh = np.ascontiguousarray(tag_wh, np.float64).reshape(-1, 2)
    cam_qt = np.ascontiguousarray(cam_qt, np.float64).reshape(-1, 7)
    if len(tag_wh) != len(tag_qt):
        raise ValueError("tag_wh and tag_qt differ in length")
    n_tags, n_poses = len(tag_qt), len(cam_qt)
    if tag_cov is not None:
        tag_cov = np.ascontiguousarray(tag_cov, np.float64).reshape(-1, 6, 6)
        if len(tag_cov) != len(tag_qt):
            raise ValueError("tag_cov and tag_qt differ in length")
    if tag_cov_joint is not None:
        tag_cov_joint = np.ascontiguousarray(tag_cov_joint, np.float64)
        if tag_cov_joint.size != 36 * n_tags * n_tags:
            raise ValueError("tag_cov_joint does not have 36 n_tags^2 entries")
        tag_cov_joint = tag_cov_joint.reshape(n_tags, n_tags, 6, 6)
    if visible_in is not None:
        visible_in = np.ascontiguousarray(np.asarray(visible_in) != 0, np.uint8)
        if visible_in.size != n_poses * n_tags:
            raise ValueError("visible_in does not have n_poses x n_tags entries")
        visible_in = visible_in.reshape(n_poses, n_tags)
    o = default_predict_options(image_width=int(image_size[0]), image_height=int(image_size[1]), **options)
    cov_px, cov_map = np.zeros((n_poses, 6, 6)), np.zeros((n_poses, 6, 6))
    visible = np.zeros((n_poses, n_tags), np.uint8) if want_visible else None
    res = np.zeros(n_poses, np.dtype(_lib.PredictResult))
    if tag_cov_joint is None:
        _lib.check(_lib.lib().vmm_ba_predict_localization(_ptr(intr), _ptr(dist), n_tags, _ptr(tag_qt), _ptr(tag_wh),
                                                          _ptr(tag_cov), n_poses, _ptr(cam_qt), C.byref(o), _ptr(cov_px),
                                                          _ptr(cov_map), _ptr(visible), _ptr(res), device))
    else:
        _lib.check(_lib.lib().vmm_ba_predict_localization_joint(_ptr(intr), _ptr(dist), n_tags, _ptr(tag_qt), _ptr(tag_wh),
                                                                _ptr(tag_cov_joint), n_poses, _ptr(cam_qt), _ptr(visible_in),
                                                                C.byref(o), _ptr(cov_px), _ptr(cov_map), _ptr(visible),
                                                                _ptr(res), device))
    out = (cov_px, cov_map, _result_dicts(res))
    return out + (visible.astype(bool),) if want_visible else out


def localization_map_covariance(intr, dist, tag_qt, tag_wh, cam_qt, img_start, obs_tag, obs_inlier, tag_cov_joint, image_size,
                                device=0, **options):
    """The part of a localisation's covariance that the map's own uncertainty causes, with the correlations between the
    tags: one predict_localization call with tag_cov_joint and visible_in built from the localisation's inlier flags.
    cam_qt (n_imgs, 7): the poses engine.localize returned; img_start, obs_tag: its batch; obs_inlier (n_obs,): the flags
    it returned.  An image's selected tags are those of its inlier observations.  Returns (cov_px, cov_map, results,
    visible_in) as predict_localization does; the response is that of the plain least-squares minimiser over the selected
    tags (unit weights, no loss)."""
    cam_qt = np.ascontiguousarray(cam_qt, np.float64).reshape(-1, 7)
    img_start = np.asarray(img_start, np.int64).reshape(-1)
    obs_tag, obs_inlier = np.asarray(obs_tag, np.int64).reshape(-1), np.asarray(obs_inlier).reshape(-1) != 0
    n_tags = len(np.asarray(tag_qt).reshape(-1, 7))
    if len(img_start) != len(cam_qt) + 1 or len(obs_tag) != len(obs_inlier) or (len(img_start) and img_start[-1] != len(obs_tag)):
        raise ValueError("img_start must have n_imgs + 1 entries and end at the number of observations")
    if len(obs_tag) and (obs_tag.min() < 0 or obs_tag.max() >= n_tags):
        raise ValueError("obs_tag outside the map")
    visible_in = np.zeros((len(cam_qt), n_tags), np.uint8)
    img = np.repeat(np.arange(len(cam_qt)), np.diff(img_start))
    visible_in[img[obs_inlier], obs_tag[obs_inlier]] = 1
    cov_px, cov_map, res = predict_localization(intr, dist, tag_qt, tag_wh, cam_qt, image_size, device=device,
                                                tag_cov_joint=tag_cov_joint, visible_in=visible_in, **options)
    return cov_px, cov_map, res, visible_in.astype(bool)


def grid_poses(lo, hi, shape, axes, up):
    """World->camera poses (n, 7) at the nodes of the box lo..hi (3,) with shape = (nx, ny, nz) nodes per dimension (a
    single node sits at lo): one pose per node and per optical-axis direction in `axes` (k, 3) (unit vectors in the
    world, normalised here), the roll fixed by `up` (the image's y axis points away from it).  Node (ix, iy, iz) with
    axis a is pose ((ix ny + iy) nz + iz) k + a.  An axis parallel to `up` is refused."""
    from .pnp import quat_from_R
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    axes = np.asarray(axes, np.float64).reshape(-1, 3)
    up = np.asarray(up, np.float64).reshape(3)
    if any(int(n) < 1 for n in shape) or len(shape) != 3:
        raise ValueError("shape must be three counts of at least 1")
    if not np.linalg.norm(up) > 0.0:
        raise ValueError("up must not be zero")
    frames = []
    for z in axes:
        if not np.linalg.norm(z) > 0.0:
            raise ValueError("an axis must not be zero")
        z = z / np.linalg.norm(z)
        x = np.cross(z, up)   # y = z x x points away from `up`
        if np.linalg.norm(x) <= 1e-9 * np.linalg.norm(up):
            raise ValueError("axis %s is parallel to up" % (tuple(float(v) for v in z),))
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])   # rows: the camera's axes in the world
        frames.append((R, quat_from_R(R)))
    nodes = np.stack(np.meshgrid(*[np.linspace(lo[d], hi[d], int(shape[d])) for d in range(3)], indexing="ij"), axis=-1)
    nodes = nodes.reshape(-1, 3)
    out = np.zeros((len(nodes), len(frames), 7))
    for a, (R, q) in enumerate(frames):
        out[:, a, :4] = q
        out[:, a, 4:] = -(nodes @ R.T)   # t = -R C
    return out.reshape(-1, 7)


def pose_minus(a, b):
    """The tangent step d (6,) with pose_plus(b, d) == a, for two poses (7,) (host numpy, no device call): translation
    is the difference, rotation the axis times the half angle of q_a q_b^-1, its sign chosen so that w >= 0."""
    a, b = np.asarray(a, np.float64).reshape(7), np.asarray(b, np.float64).reshape(7)
    qa, qb = a[:4] / np.linalg.norm(a[:4]), b[:4] / np.linalg.norm(b[:4])
    w1, x1, y1, z1 = qa
    w2, x2, y2, z2 = qb[0], -qb[1], -qb[2], -qb[3]
    z = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
    if z[0] < 0.0:
        z = -z
    s = np.linalg.norm(z[1:])
    d = np.zeros(6)
    d[:3] = a[4:] - b[4:]
    if s > 0.0:
        d[3:] = z[1:] * (np.arctan2(s, z[0]) / s)
    return d


def pose_plus(qt, delta, device=0):
    """Plus(qt, delta) for (n,7) poses and (n,6) tangent steps with the engine's device function
    (Ceres QuaternionParameterization::Plus on q, addition on t; tangent = translation then rotation)."""
    qt = np.ascontiguousarray(qt, np.float64).reshape(-1, 7)
    delta = np.ascontiguousarray(delta, np.float64).reshape(-1, 6)
    out = np.zeros_like(qt)
    _lib.check(_lib.lib().vmm_ba_pose_plus(len(qt), _ptr(qt), _ptr(delta), _ptr(out), device))
    return out


def dense_spd_solve(A, b, device=0):
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    x = np.zeros(len(b))
    info = C.c_int(0)
    _lib.check(_lib.lib().vmm_ba_dense_spd_solve(device, len(b), _ptr(A), _ptr(b), _ptr(x), C.byref(info)))
    return x, info.value


def dense_syrk(Z, device=0):
    Z = np.ascontiguousarray(Z, np.float64)
    k, n = Z.shape
    Cm = np.zeros((n, n))
    _lib.check(_lib.lib().vmm_ba_dense_syrk(device, k, n, _ptr(Z), _ptr(Cm)))
    return Cm
