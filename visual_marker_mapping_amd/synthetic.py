"""Deterministic synthetic scenes via tools/libvmm_scene.so.

Stands in for the detector output (marker_detections.json) and the PnP initial guess the
reference computes with OpenCV (/root/reference/src/TagReconstructor.cpp:156,167-230); neither can
run in this image.  Bench/test input only -- not part of the hot path.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "tools", "libvmm_scene.so")
_LIB = None


class SceneCfg(C.Structure):
    _fields_ = [("n_cams", C.c_int), ("n_tags", C.c_int), ("seed", C.c_uint64),
                ("visibility", C.c_double), ("noise_px", C.c_double), ("outlier_frac", C.c_double),
                ("outlier_px", C.c_double), ("use_distortion", C.c_int), ("cam_rot_deg", C.c_double),
                ("cam_trans_m", C.c_double), ("tag_rot_deg", C.c_double), ("tag_trans_m", C.c_double),
                ("neighbors_min", C.c_int), ("neighbors_max", C.c_int), ("wall_rows", C.c_int)]


def build(force=False):
    src = os.path.join(_ROOT, "tools", "scene_gen.c")
    if force or not os.path.exists(_SO) or (os.path.exists(src)
                                            and os.path.getmtime(_SO) < os.path.getmtime(src)):
        subprocess.check_call(["make", "-C", os.path.join(_ROOT, "tools"), "-s", "all"])
    return _SO


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            build()
        _LIB = C.CDLL(_SO)
        _LIB.vmm_scene_generate.restype = C.c_int
    return _LIB


class SyntheticScene:
    """Arrays of one generated scene.  Poses are rows of (qw,qx,qy,qz,tx,ty,tz)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_obs(self):
        return len(self.obs_cam)

    def by_image(self):
        """The observations grouped by image: (img_start (n_images + 1, int64), order), order a stable sort by obs_cam."""
        start = np.zeros(len(self.cam_gt) + 1, np.int64)
        start[1:] = np.cumsum(np.bincount(self.obs_cam, minlength=len(self.cam_gt)))
        return start, np.argsort(self.obs_cam, kind="stable")


def make_scene(config=2, **overrides):
    """config = index into BASELINE.json configs (1-based); overrides are SceneCfg fields."""
    L = _lib()
    cfg = SceneCfg()
    L.vmm_scene_default_cfg(C.byref(cfg), C.c_int(config))
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    nc, nt = cfg.n_cams, cfg.n_tags
    cap = nc * nt
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    intr, dist = np.zeros(4), np.zeros(5)
    cam_gt, tag_gt = np.zeros((nc, 7)), np.zeros((nt, 7))
    cam_init, tag_init = np.zeros((nc, 7)), np.zeros((nt, 7))
    tag_wh = np.zeros((nt, 2))
    obs_cam, obs_tag = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    obs_px = np.zeros((cap, 8))
    n = L.vmm_scene_generate(C.byref(cfg), dp(intr), dp(dist), dp(cam_gt), dp(tag_gt), dp(tag_wh),
                             dp(cam_init), dp(tag_init), ip(obs_cam), ip(obs_tag), dp(obs_px),
                             C.c_int(cap))
    if n < 0:
        raise RuntimeError("scene buffer too small")
    return SyntheticScene(config=config, intr=intr, dist=dist, cam_gt=cam_gt, tag_gt=tag_gt,
                          cam_init=cam_init, tag_init=tag_init, tag_wh=tag_wh, fixed_tag=0,
                          obs_cam=obs_cam[:n].copy(), obs_tag=obs_tag[:n].copy(),
                          obs_px=obs_px[:n].copy(), noise_px=cfg.noise_px,
                          robustify=bool(cfg.outlier_frac > 0), visibility=cfg.visibility)


def make_rig_scene(config, ext_qt, missing=(), outlier_frac=0.0, outlier_px=(50.0, 200.0), seed=0, intr=None, dist=None,
                   **overrides):
    """A rig of K rigidly mounted cameras moved through make_scene(config, **overrides): the rig poses (world->rig) are
    that scene's cam_gt, the map its tag_gt, and camera c of frame f stands at ext_qt[c] o rig[f] (ext_qt (K, 7),
    rig->camera).  intr (K, 4) / dist (K, 5): one model per camera (default: the scene's for all).
    Tag t is observed in image (f, c) when all four corners have Z > 0.1, project inside 6000 x 4000 with the cost
    functor's projection (pnp.project) and the tag faces the camera; the images of `missing` ((f, c) pairs) are empty.
    Gaussian noise of the scene's noise_px and the planted outliers come from numpy's default_rng(seed): round(
    outlier_frac * n_obs) observations, each with all four corners shifted by one common offset of a length drawn from
    outlier_px = (low, high) in a random direction.
    Returns a SyntheticScene with intr, dist, ext_qt, rig_gt (n_frames, 7), tag_gt, tag_wh, the CSR batch img_start
    (n_frames * K + 1,; image (f, c) is slot f * K + c), obs_tag, obs_px (n_obs, 8), obs_frame, obs_cam and outlier
    (n_obs,) bool, the planted mask."""
    from .pnp import project
    s = make_scene(config, **overrides)
    ext_qt = np.array(ext_qt, np.float64).reshape(-1, 7)
    K, n_frames = len(ext_qt), len(s.cam_gt)
    intr = np.tile(s.intr, (K, 1)) if intr is None else np.array(intr, np.float64).reshape(K, 4)
    dist = np.tile(s.dist, (K, 1)) if dist is None else np.array(dist, np.float64).reshape(K, 5)

    def rot(q):
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])

    sign = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], np.float64)
    tag_R = [rot(q[:4]) for q in s.tag_gt]
    corners = [np.hstack([0.5 * sign * s.tag_wh[t], np.zeros((4, 1))]) @ tag_R[t].T + s.tag_gt[t, 4:]
               for t in range(len(s.tag_gt))]
    missing = {(int(f), int(c)) for f, c in missing}
    start, obs_tag, obs_px, obs_frame, obs_cam = [0], [], [], [], []
    for f in range(n_frames):
        Rf, tf = rot(s.cam_gt[f, :4]), s.cam_gt[f, 4:]
        for c in range(K):
            Rc = rot(ext_qt[c, :4])
            R, t = Rc @ Rf, Rc @ tf + ext_qt[c, 4:]
            for j in range(len(s.tag_gt) if (f, c) not in missing else 0):
                pc = corners[j] @ R.T + t
                if not (pc[:, 2] > 0.1).all():
                    continue
                uv = project(corners[j], R, t, intr[c], dist[c])
                inside = (uv[:, 0] >= 0) & (uv[:, 0] < 6000) & (uv[:, 1] >= 0) & (uv[:, 1] < 4000)
                if not inside.all() or (R @ tag_R[j][:, 2]) @ (R @ s.tag_gt[j, 4:] + t) >= 0:
                    continue
                obs_tag.append(j)
                obs_px.append(uv.reshape(8))
                obs_frame.append(f)
                obs_cam.append(c)
            start.append(len(obs_tag))
    n = len(obs_tag)
    obs_px = np.array(obs_px, np.float64).reshape(n, 8)
    rng = np.random.default_rng(seed)
    obs_px += s.noise_px * rng.standard_normal((n, 8))
    outlier = np.zeros(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        outlier[rng.choice(n, n_out, replace=False)] = True
        length = rng.uniform(outlier_px[0], outlier_px[1], n_out)
        angle = rng.uniform(0.0, 2.0 * np.pi, n_out)
        obs_px[outlier] += np.tile(np.stack([length * np.cos(angle), length * np.sin(angle)], axis=1), (1, 4))
    return SyntheticScene(config=config, intr=intr, dist=dist, ext_qt=ext_qt, rig_gt=s.cam_gt, tag_gt=s.tag_gt,
                          tag_wh=s.tag_wh, img_start=np.array(start, np.int64), obs_tag=np.array(obs_tag, np.int32),
                          obs_px=obs_px, obs_frame=np.array(obs_frame, np.int32), obs_cam=np.array(obs_cam, np.int32),
                          outlier=outlier, noise_px=s.noise_px, n_frames=n_frames, n_rig_cams=K)


def write_project(scene, directory):
    """Writes the scene as a project directory of the reference's mapping step (SURVEY.md 8(d) "emitted
    files"): camera_intrinsics.json and marker_detections.json in the reference's formats (Appendix B),
    plus ground_truth.json and initial_state.json (reconstruction.json layout) for tests."""
    from . import io as _io
    from .tag_reconstructor import Camera, CameraModel, ReconstructedTag, detection_result_from_arrays
    os.makedirs(directory, exist_ok=True)
    model = CameraModel(*[float(v) for v in scene.intr], distortionCoefficients=scene.dist,
                        verticalResolution=4000, horizontalResolution=6000)
    _io.writeCameraModel(model, os.path.join(directory, "camera_intrinsics.json"))
    det = detection_result_from_arrays(scene.obs_cam, scene.obs_tag, scene.obs_px, scene.tag_wh, len(scene.cam_gt))
    _io.writeDetectionResult(det, os.path.join(directory, "marker_detections.json"))
    for name, cams, tags in (("ground_truth.json", scene.cam_gt, scene.tag_gt),
                             ("initial_state.json", scene.cam_init, scene.tag_init)):
        rt = {t: ReconstructedTag(t, "apriltag_36h11", tags[t, :4], tags[t, 4:], scene.tag_wh[t, 0], scene.tag_wh[t, 1])
              for t in range(len(tags))}
        rc = {c: Camera(c, cams[c, :4], cams[c, 4:]) for c in range(len(cams))}
        _io.exportReconstructions(os.path.join(directory, name), rt, rc, model)
    return model, det
