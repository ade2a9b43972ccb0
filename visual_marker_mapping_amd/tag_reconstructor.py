"""Host-side mirror of the reference's TagReconstructor / CameraModel interface for the hot path.

Same names, argument meaning and error behaviour as
/root/reference/include/visual_marker_mapping/{TagReconstructor,CameraModel,Camera,DetectionResults}.h,
so that the parity tests read like tests of the reference class.  The bodies of the hot-path methods
pack the std::map-style state into flat arrays and call libvmm_ba.so (MI355X); nothing here computes
residuals or solves on the CPU.

startReconstruction (the incremental driver) is host logic around the hot
path; its two PnP initialisations (OpenCV in the reference) live in pnp.py.  Callers may also provide
initial poses through setReconstructedTags / setReconstructedCameras and call doBundleAdjustment directly.
"""
import contextlib
import math
import os

import numpy as np

from . import engine as _engine


# ---- plain data types (DetectionResults.h:10-37, Camera.h:9-18, TagReconstructor.h:15-53) -----------


class TagObservation:
    def __init__(self, imageId=-1, tagId=-1, corners=None):
        self.imageId = int(imageId)
        self.tagId = int(tagId)
        # observed tag corners LL, LR, UR, UL as (u, v)
        self.corners = np.zeros((4, 2)) if corners is None else np.asarray(corners, np.float64).reshape(4, 2)


class TagImg:
    def __init__(self, imageId=-1, filename=""):
        self.imageId = int(imageId)
        self.filename = filename


class Tag:
    def __init__(self, tagId, tagType, width, height):
        self.tagId = int(tagId)
        self.tagType = tagType
        self.width = float(width)
        self.height = float(height)


class DetectionResult:
    def __init__(self, images=None, tags=None, tagObservations=None):
        self.images = list(images or [])
        self.tags = list(tags or [])
        self.tagObservations = list(tagObservations or [])


def _quat_to_R(q):
    """Eigen::Quaterniond::toRotationMatrix for q = (w, x, y, z) (no normalisation)."""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


class Camera:
    """World->camera pose; q = (w, x, y, z), default identity (Camera.h:13-14)."""

    def __init__(self, cameraId=-1, q=None, t=None):
        self.cameraId = int(cameraId)
        self.q = np.array([1.0, 0.0, 0.0, 0.0]) if q is None else np.asarray(q, np.float64).reshape(4).copy()
        self.t = np.zeros(3) if t is None else np.asarray(t, np.float64).reshape(3).copy()

    def quat(self):
        return self.q.copy()

    def setQuat(self, quat):
        self.q = np.asarray(quat, np.float64).reshape(4).copy()


class ReconstructedTag:
    """Tag->world pose plus the tag's metric size (TagReconstructor.h:15-53)."""

    def __init__(self, id=-1, tagType="", q=None, t=None, tagWidth=0.0, tagHeight=0.0):
        self.id = int(id)
        self.tagType = tagType
        self.q = np.array([1.0, 0.0, 0.0, 0.0]) if q is None else np.asarray(q, np.float64).reshape(4).copy()
        self.t = np.zeros(3) if t is None else np.asarray(t, np.float64).reshape(3).copy()
        self.tagWidth = float(tagWidth)
        self.tagHeight = float(tagHeight)

    def quat(self):
        return self.q.copy()

    def setQuat(self, quat):
        self.q = np.asarray(quat, np.float64).reshape(4).copy()

    def computeLocalMarkerCorners3D(self):
        w, h = self.tagWidth, self.tagHeight   # TagReconstructor.h:47-50: LL, LR, UR, UL
        return [np.array([-w / 2.0, -h / 2.0, 0.0]), np.array([w / 2.0, -h / 2.0, 0.0]),
                np.array([w / 2.0, h / 2.0, 0.0]), np.array([-w / 2.0, h / 2.0, 0.0])]

    def computeMarkerCorners3D(self):
        R = _quat_to_R(self.q)
        return [R @ p + self.t for p in self.computeLocalMarkerCorners3D()]


class CameraModel:
    """OpenCV pinhole + 5-coefficient distortion (CameraModel.h:12-34)."""

    def __init__(self, fx=0.0, fy=0.0, cx=0.0, cy=0.0, distortionCoefficients=None, verticalResolution=0,
                 horizontalResolution=0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.distortionCoefficients = (np.zeros(5) if distortionCoefficients is None
                                       else np.asarray(distortionCoefficients, np.float64).reshape(5).copy())
        self.verticalResolution = int(verticalResolution)
        self.horizontalResolution = int(horizontalResolution)

    def getK(self):
        """CameraModel::getK, src/CameraModel.cpp:28-36."""
        K = np.eye(3)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = self.fx, self.fy, self.cx, self.cy
        return K

    def projectPoint(self, point3D, device=0):
        """CameraModel::projectPoint, src/CameraModel.cpp:6-26: camera-frame point(s) -> pixel(s), including the
        reference's aliasing at :20-23 (the y tangential term is evaluated with the already distorted x).

        Accepts one point (3,) or a batch (n, 3); evaluated by the device kernel.
        """
        pts = np.asarray(point3D, np.float64)
        single = pts.ndim == 1
        uv = _engine.project_points([self.fx, self.fy, self.cx, self.cy], self.distortionCoefficients,
                                    pts.reshape(-1, 3), device=device)
        return uv[0] if single else uv


# ---- the class whose hot path this package replaces --------------------------------------------------


class TagReconstructor:
    """Mirror of visual_marker_mapping::TagReconstructor (TagReconstructor.h:58-146)."""

    def __init__(self, detection_result, device=0):
        self.originTagId = -1                                  # src/TagReconstructor.cpp:70
        # not in the reference API: ids of tags every bundle adjustment holds constant, like the origin tag (:669-673)
        self.constantTagIds = set()
        self.detectionResults_ = detection_result
        self.reconstructedTags = {}                            # tag id -> ReconstructedTag
        self.reconstructedCameras = {}                         # image id -> Camera
        self.camModel = CameraModel()
        self.device = int(device)
        self.lastSummary = None                                # summary of the last doBundleAdjustment
        self.lastCovariances = None                            # tag id -> 3x3 (last printSummary call)
        self.lastPoseCovariances = None                        # {"tags": {id: 6x6}, "cameras": {id: 6x6}} (computePoseCovariances)
        self.lastInitReport = None                             # report of vmm_ba_initialize (startReconstructionGlobal)
        self.lastLocalizationReport = None                     # image id -> report (computeRelativeCameraPosesFromImgs)
        self.lastSelfCalibrationReport = None                  # report of doBundleAdjustment(refineCameraModel=True)
        self.lastTriangulationDropped = 0                      # observations triangulatePoints dropped (image without a pose)
        self.lastTagLocationReport = None                      # tag id -> report (locateTags)
        self.lastMapCheckReport = None                         # report of checkMap
        self._cached = None                                    # (structure key, BundleAdjuster) of the last call
        self._obs_cache = None                                 # observation list as arrays (see _obs_arrays)
        self._resident = False                                 # device-resident packing (startReconstruction)
        self._oneLaunch = False                                # startReconstruction(oneLaunch=True) while it runs
        self._full = None                                      # the whole detection set as problem arrays

    # -- trivial accessors (src/TagReconstructor.cpp:75-84, 818-842) --
    def getLowestTag(self):
        tags = self.detectionResults_.tags
        m = tags[0].tagId     # the reference dereferences tags[0] unguarded (:77)
        for t in tags:
            if t.tagId < m:
                m = t.tagId
        return m

    def getReconstructedTags(self):
        return dict(self.reconstructedTags)

    def getReconstructedCameras(self):
        return dict(self.reconstructedCameras)

    def setReconstructedTags(self, tags):
        """Not in the reference API: stands in for the PnP initialisation of startReconstruction."""
        self.reconstructedTags = {int(k): v for k, v in dict(tags).items()}

    def setReconstructedCameras(self, cams):
        """Not in the reference API: stands in for the PnP initialisation of startReconstruction."""
        self.reconstructedCameras = {int(k): v for k, v in dict(cams).items()}

    def getCameraModel(self):
        return self.camModel

    def setCameraModel(self, cameraModel):
        self.camModel = cameraModel

    def setOriginTagId(self, originTagId):
        self.originTagId = int(originTagId)

    # -- the camera model as the engine takes and returns it --
    def _model_args(self):
        m = self.camModel
        return [m.fx, m.fy, m.cx, m.cy], m.distortionCoefficients

    def _with_model(self, intr, dist):
        """camModel with the nine numbers replaced; the resolutions stay."""
        return CameraModel(fx=float(intr[0]), fy=float(intr[1]), cx=float(intr[2]), cy=float(intr[3]),
                           distortionCoefficients=dist, verticalResolution=self.camModel.verticalResolution,
                           horizontalResolution=self.camModel.horizontalResolution)

    @staticmethod
    def _model_report(report, intr, dist, cov):
        return dict(report, intrinsics=np.concatenate([intr, dist]), covariance=cov, std=np.sqrt(np.diag(cov)))

    def startReconstruction(self, numThreads=1, deviceResident=True, oneLaunch=False):
        """oneLaunch: every bundle adjustment of the run whose kept family fits goes through engine.solve_small (see
        doBundleAdjustment); the default keeps every call as it was.

        deviceResident: ONE device handle holds every image, tag and observation of the detection result for
        the whole run and each of the N+2 bundle adjustments / prunings only sends an observation mask and the
        poses (vmm_ba_set_observation_mask); False rebuilds a handle whenever the problem structure changes.
        Same results either way (tests/test_gpu_driver.py).

        The incremental driver, src/TagReconstructor.cpp:86-278: origin tag at identity; the image that
        sees the origin tag and the most tags first; then per image: camera pose from the already
        reconstructed tags (PnP+RANSAC), every new tag seen in >= 2 images from its own four corners (PnP),
        robust bundle adjustment (400 iterations), pruning of tags above 2 px; next = the image with the most
        reconstructed tags.  Ends with BA(1500, robust), both prunings, BA(1500, plain, summary).

        The bundle adjustments and the reprojection statistics run on the MI355X through libvmm_ba; the two
        PnP initialisations are host code in pnp.py (OpenCV's role in the reference)."""
        from . import pnp as _pnp
        self._oneLaunch = bool(oneLaunch)
        try:
            with self._resident_frame(deviceResident):
                self._start_reconstruction(numThreads, _pnp)
        finally:
            self._oneLaunch = False

    @contextlib.contextmanager
    def _resident_frame(self, resident=True):
        """The frame of a whole-run driver: the device-resident packing while it runs; afterwards, however it ends,
        the cached handle is released and the full arrays are dropped."""
        self._resident = bool(resident)
        try:
            yield
        finally:
            self._resident = False
            self._drop_cached()
            self._full = None

    def _closing_sequence(self, numThreads):
        """The reference's closing sequence (src/TagReconstructor.cpp:271-277)."""
        print("Starting final bundle adjustment")
        self.doBundleAdjustment(1500, numThreads, True, False)
        self.removeBadMarkers(2.0)
        self.removeBadCameras(2.0)
        self.doBundleAdjustment(1500, numThreads, False, True)

    def _start_reconstruction(self, numThreads, _pnp):
        if self.originTagId == -1:
            self.originTagId = self.getLowestTag()
        intr = (self.camModel.fx, self.camModel.fy, self.camModel.cx, self.camModel.cy)
        dist = tuple(float(v) for v in self.camModel.distortionCoefficients)
        whichImagesObserveTag, tagsInImage, obsOfImage = {}, {}, {}
        for ob in self.detectionResults_.tagObservations:
            whichImagesObserveTag.setdefault(ob.tagId, set()).add(ob.imageId)
            tagsInImage.setdefault(ob.imageId, set()).add(ob.tagId)
            obsOfImage.setdefault(ob.imageId, []).append(ob)
        imageFilenames = {img.imageId: img.filename for img in self.detectionResults_.images}
        tagById = {t.tagId: t for t in self.detectionResults_.tags}

        # the image with the most markers among those that see the origin tag (:117-127)
        maxObservations, curImageId = 0, -1
        for imageId in sorted(whichImagesObserveTag.get(self.originTagId, ())):
            if len(tagsInImage[imageId]) > maxObservations:
                curImageId, maxObservations = imageId, len(tagsInImage[imageId])
        if self.originTagId not in tagById:
            raise RuntimeError("Could not use tag with id %d as origin tag, because it was not detected."
                               % self.originTagId)
        o = tagById[self.originTagId]
        self.reconstructedTags.setdefault(self.originTagId, ReconstructedTag(
            id=self.originTagId, tagType=o.tagType, tagWidth=o.width, tagHeight=o.height))

        while True:
            print("Reconstructing image %d/%d | %s with id: %d" % (
                len(self.reconstructedCameras), len(self.detectionResults_.images),
                imageFilenames.get(curImageId, ""), curImageId))
            pose = self.computeRelativeCameraPoseFromImg(curImageId, intr, dist, obsOfImage.get(curImageId, []))
            if pose is None:
                raise RuntimeError("No reconstructed tags in image found. To reconstruct the image pose "
                                   "already reconstructed markers are needed. This should NOT happen.")
            newCamera = Camera(cameraId=curImageId, q=pose[0], t=pose[1])
            print("   Initialized camera with id %d" % curImageId)
            self.reconstructedCameras.setdefault(curImageId, newCamera)
            cam = self.reconstructedCameras[curImageId]
            Rc, tc = _quat_to_R(cam.q), cam.t
            for ob in obsOfImage.get(curImageId, []):
                if ob.tagId in self.reconstructedTags:
                    continue
                if len(whichImagesObserveTag[ob.tagId]) < 2:
                    print("   Skipping reconstruction of tag %d: Only observed once!" % ob.tagId)
                    continue
                d = tagById[ob.tagId]
                recTag = ReconstructedTag(id=ob.tagId, tagType=d.tagType, tagWidth=d.width, tagHeight=d.height)
                R, t = _pnp.solvePnP(recTag.computeLocalMarkerCorners3D(), ob.corners, intr, dist)   # tag -> camera
                # TMarker2World = extrinsic^-1 * T  (:213-221)
                recTag.setQuat(_pnp.quat_from_R(Rc.T @ R))
                recTag.t = Rc.T @ (t - tc)
                self.reconstructedTags[ob.tagId] = recTag
                print("   Initialized tag with id %d" % ob.tagId)

            self.doBundleAdjustment(400, numThreads, True)
            self.removeBadMarkers(2.0)

            # next: the unreconstructed image with the most reconstructed tags (:236-259)
            maxPairs = 0
            for img in self.detectionResults_.images:
                if img.imageId in self.reconstructedCameras:
                    continue
                n = sum(1 for tid in tagsInImage.get(img.imageId, ()) if tid in self.reconstructedTags)
                if n > maxPairs:
                    maxPairs, curImageId = n, img.imageId
            if maxPairs == 0:
                break
            print("----------------------------------------------------------")

        self._closing_sequence(numThreads)

    def startReconstructionGlobal(self, numThreads=1, **init_options):
        """Not in the reference API: the same map as startReconstruction without its N + 2 dependent bundle
        adjustments.  Origin tag as there (lowest id when -1, at identity); ONE device handle over the whole
        detection result; vmm_ba_initialize places every camera and tag reachable from the origin tag on the device
        (planar pose of every observation, candidate selection by truncated reprojection error, per-pose refinement;
        DESIGN.md section 9) -- these become the reconstructed sets; then the reference's closing sequence
        (src/TagReconstructor.cpp:271-277): BA(1500, robust), both prunings, BA(1500, plain, summary).
        init_options: fields of vmm_ba_init_options.  The report of the initialisation is kept in lastInitReport."""
        with self._resident_frame():
            self._start_reconstruction_global(numThreads, init_options)

    def _start_reconstruction_global(self, numThreads, init_options):
        if self.originTagId == -1:
            self.originTagId = self.getLowestTag()
        tagById = {t.tagId: t for t in self.detectionResults_.tags}
        if self.originTagId not in tagById:
            raise RuntimeError("Could not use tag with id %d as origin tag, because it was not detected."
                               % self.originTagId)
        o = tagById[self.originTagId]
        self.reconstructedTags.setdefault(self.originTagId, ReconstructedTag(
            id=self.originTagId, tagType=o.tagType, tagWidth=o.width, tagHeight=o.height))
        # the resident packing with nothing but the origin tag reconstructed: every other pose is a placeholder that
        # still gives finite residuals (cameras 1 m in front of tags at identity)
        reached = self._initialize_on_device(tagById, init_options)
        imagesOfTag = {}
        for ob in self.detectionResults_.tagObservations:
            imagesOfTag.setdefault(ob.tagId, set()).add(ob.imageId)
        for tid, recTag in reached:
            if tid == self.originTagId:
                continue
            if recTag is not None:
                self.reconstructedTags[tid] = recTag
            elif len(imagesOfTag.get(tid, ())) == 1:
                print("   Skipping reconstruction of tag %d: Only observed once!" % tid)

        self._closing_sequence(numThreads)

    def _initialize_on_device(self, tagById, init_options):
        """The stage startReconstructionGlobal and extendReconstruction share: packs the whole detection result around
        the tags reconstructed so far, runs vmm_ba_initialize on ONE handle, keeps and prints the report, and makes
        every reached image a reconstructed camera.  Returns, in the order of the packed tags, (tag id, the
        ReconstructedTag at its initialised pose -- None when the tag was not reached or is not in the detection
        result's tag list); which of them join the map is the caller's rule."""
        p = self._pack_resident(for_ba=True)
        full = self._full
        with self._handle(p, elimination=_engine.ELIM_AUTO) as ba:
            ba.set_observation_mask(None)
            report, cam_ok, tag_ok = ba.initialize(**init_options)
            cam, tag = ba.get_state()
        self.lastInitReport = report
        print("Initialized %d of %d cameras and %d of %d tags in %d rounds, average reprojection error %g"
              % (report["cams_reached"], len(cam_ok), report["tags_reached"], len(tag_ok), report["rounds"],
                 report["avg_reprojection_px"]))
        if not cam_ok.any():
            raise RuntimeError("No reconstructed tags in image found. To reconstruct the image pose "
                               "already reconstructed markers are needed. This should NOT happen.")
        for r, cid in enumerate(full["cams"].tolist()):
            if cam_ok[r]:
                self.reconstructedCameras[cid] = Camera(cameraId=cid, q=cam[r, :4], t=cam[r, 4:])
        reached = []
        for r, tid in enumerate(full["tags"].tolist()):
            recTag = None
            if tag_ok[r] and tid in tagById:
                d = tagById[tid]
                recTag = ReconstructedTag(id=tid, tagType=d.tagType, q=tag[r, :4], t=tag[r, 4:],
                                          tagWidth=d.width, tagHeight=d.height)
            reached.append((tid, recTag))
        return reached

    def extendReconstruction(self, numThreads=1, **init_options):
        """Not in the reference API: grows a finished map with new images while every tag of the map stays where it
        is, bit for bit.  Precondition: reconstructedTags holds the finished map (io.parseReconstructions),
        detectionResults_ the NEW images.  ONE device handle over the new detection result: its cameras are the new
        images, its tags the map tags the new detections observe plus every tag the detections name that the map lacks
        -- a large map costs nothing beyond what the new images see.  All packed map tags are held constant
        (vmm_ba_set_constant_poses), vmm_ba_initialize grows outward from them, the reached poses become the
        reconstructed sets, and the reference's closing sequence (src/TagReconstructor.cpp:271-277) runs with the
        constants held: BA(1500, robust), both prunings (a map tag is never pruned), BA(1500, plain, summary).
        Afterwards reconstructedTags is the whole map (q, t, width and height untouched) plus the new tags, and
        reconstructedCameras holds the new images' cameras only.  init_options: fields of vmm_ba_init_options; the
        report of the initialisation is kept in lastInitReport."""
        whole_map = dict(self.reconstructedTags)
        observed = {int(ob.tagId) for ob in self.detectionResults_.tagObservations}
        packed_map = {tid: tag for tid, tag in whole_map.items() if tid in observed}
        if not packed_map:
            raise RuntimeError("No reconstructed tags in image found. To reconstruct the image pose "
                               "already reconstructed markers are needed. This should NOT happen.")
        saved_const = set(self.constantTagIds)
        saved_cameras = self.reconstructedCameras
        self.reconstructedTags = dict(packed_map)
        self.reconstructedCameras = {}
        self.constantTagIds = saved_const | set(packed_map)
        done = False
        try:
            with self._resident_frame():
                self._extend_reconstruction(numThreads, init_options)
            done = True
        finally:
            self.constantTagIds = saved_const
            if done:
                # the map tags no new image sees were never packed
                self.reconstructedTags = {**{t: v for t, v in whole_map.items() if t not in packed_map},
                                          **self.reconstructedTags}
            else:
                # a failure part-way leaves the object as it was: the map, and whatever cameras it held
                self.reconstructedTags = whole_map
                self.reconstructedCameras = saved_cameras

    def _extend_reconstruction(self, numThreads, init_options):
        tagById = {t.tagId: t for t in self.detectionResults_.tags}
        # the resident packing with the observed map tags reconstructed (and constant): every other pose is a placeholder
        for tid, recTag in self._initialize_on_device(tagById, init_options):
            if recTag is not None and tid not in self.reconstructedTags:
                self.reconstructedTags[tid] = recTag
        self._closing_sequence(numThreads)

    def computeRelativeCameraPoseFromImg(self, imageId, intr, dist, observations=None):
        """src/TagReconstructor.cpp:280-312: (q, t) of the camera from every correspondence between this
        image's detected corners and the corners of already reconstructed tags, or None without any."""
        from . import pnp as _pnp
        if observations is None:
            observations = [ob for ob in self.detectionResults_.tagObservations if ob.imageId == imageId]
        X, px = [], []
        for ob in observations:
            tag = self.reconstructedTags.get(ob.tagId)
            if tag is None:
                continue
            X.extend(tag.computeMarkerCorners3D())
            px.extend(np.asarray(ob.corners, np.float64).reshape(4, 2))
        print("   Reconstructing camera pose from %d 2d/3d correspondences" % len(px))
        if not px:
            return None
        R, t = _pnp.solvePnPRansac(np.asarray(X), np.asarray(px), intr, dist, seed=int(imageId) & 0x7FFFFFFF)
        return _pnp.quat_from_R(R), t

    def _map_arrays(self):
        """The reconstructed tags in id order: (tag_ids, tag_qt (n, 7), tag_wh (n, 2))."""
        tag_ids = sorted(self.reconstructedTags)
        tags = [self.reconstructedTags[t] for t in tag_ids]
        return (tag_ids, np.array([np.concatenate([t.q, t.t]) for t in tags], np.float64).reshape(-1, 7),
                np.array([[t.tagWidth, t.tagHeight] for t in tags], np.float64).reshape(-1, 2))

    def _joint_for_map(self, ids, joint):
        """The tags' joint covariance (ids, (T, T, 6, 6)) in the order of _map_arrays: (n, n, 6, 6)."""
        ids = [int(t) for t in ids]
        joint = np.asarray(joint, np.float64)
        if joint.size != 36 * len(ids) ** 2 or len(set(ids)) != len(ids):
            raise ValueError("the joint covariance does not have one 6x6 block per pair of its %d tag ids" % len(ids))
        joint = joint.reshape(len(ids), len(ids), 6, 6)
        row = {t: k for k, t in enumerate(ids)}
        missing = [t for t in sorted(self.reconstructedTags) if t not in row]
        if missing:
            raise RuntimeError("The joint covariance does not cover the map: no entry for tag %s."
                               % ", ".join(str(t) for t in missing))
        rows = np.array([row[t] for t in sorted(self.reconstructedTags)], np.int64)
        return np.ascontiguousarray(joint[np.ix_(rows, rows)])

    @staticmethod
    def _item_report(res, pose, cov, order, inl, b, e):
        """One image's or frame's entry of a localisation report: the result's fields, the pose, its covariance and the
        observations [b, e) with their inlier flags."""
        return dict(res, pose=pose.copy(), covariance=cov.copy(), observations=list(order[b:e]), inliers=inl[b:e].copy())

    def _pack_against_map(self, det, imageIds, skipTagIds=()):
        """The flat arrays engine.localize and engine.calibrate take: the reconstructed tags as the map and the
        observations of those tags grouped by image, but for the tags in skipTagIds.  Returns (ids, order, tag_qt, tag_wh,
        img_start, obs_tag, obs_px); order[k] indexes det.tagObservations."""
        if imageIds is None:
            ids = sorted({int(im.imageId) for im in det.images} | {int(ob.imageId) for ob in det.tagObservations})
        else:
            ids = [int(i) for i in imageIds]
        tag_ids, tag_qt, tag_wh = self._map_arrays()
        dense = {t: k for k, t in enumerate(tag_ids)}
        per_img = {i: [] for i in ids}
        for k, ob in enumerate(det.tagObservations):
            if ob.imageId in per_img and ob.tagId in dense and ob.tagId not in skipTagIds:
                per_img[ob.imageId].append(k)
        order = [k for i in ids for k in per_img[i]]
        img_start = np.zeros(len(ids) + 1, np.int64)
        img_start[1:] = np.cumsum([len(per_img[i]) for i in ids])
        obs_tag = np.array([dense[det.tagObservations[k].tagId] for k in order], np.int32)
        obs_px = (np.stack([np.asarray(det.tagObservations[k].corners, np.float64).reshape(8) for k in order])
                  if order else np.zeros((0, 8)))
        return ids, order, tag_qt, tag_wh, img_start, obs_tag, obs_px

    def computeRelativeCameraPosesFromImgs(self, imageIds=None, detectionResult=None, **options):
        """Batch form of computeRelativeCameraPoseFromImg on the device (vmm_ba_localize): every image of
        `detectionResult` (default: the reconstructor's own; `imageIds` restricts it) is localised against the
        reconstructed tags.  Observations of tags that are not reconstructed are dropped.  options: the fields of
        vmm_ba_localize_options.  Returns {imageId: Camera} for the images with status OK; lastLocalizationReport holds
        per image id the status, counts, rms_px, cost, the pose, the 6x6 covariance and the inlier flag of each used
        observation (index into detectionResult.tagObservations)."""
        det = self.detectionResults_ if detectionResult is None else detectionResult
        return self._localize_images(det, imageIds, (), options)

    def _localize_images(self, det, imageIds, skipTagIds, options):
        """computeRelativeCameraPosesFromImgs with the observations of the tags in skipTagIds left out."""
        ids, order, tag_qt, tag_wh, img_start, obs_tag, obs_px = self._pack_against_map(det, imageIds, skipTagIds)
        cam_qt, cam_cov, inl, res = _engine.localize(*self._model_args(), tag_qt, tag_wh, img_start, obs_tag, obs_px,
                                                     device=self.device, **options)
        cams, report = {}, {}
        for n, i in enumerate(ids):
            report[i] = self._item_report(res[n], cam_qt[n], cam_cov[n], order, inl, int(img_start[n]), int(img_start[n + 1]))
            if res[n]["status"] == _engine._lib.LOC_OK:
                cams[i] = Camera(i, cam_qt[n, :4], cam_qt[n, 4:])
        self.lastLocalizationReport = report
        return cams

    def localizationMapCovariances(self, tagJointCovariance, detectionResult=None, **options):
        """The part of every localised image's covariance that the map's own uncertainty causes, with the correlations
        between the tags, for the images of lastLocalizationReport (engine.localization_map_covariance: one
        vmm_ba_predict_localization_joint call whose visible_in holds, per image with status OK, the tags of its inlier
        observations; any other image selects nothing and gets zeros).  tagJointCovariance: (tag ids, (T, T, 6, 6)) as
        computePoseCovariances(jointTags=True)["tag_joint"].  detectionResult: the one that was localised (default: the
        reconstructor's own).  options: the fields of vmm_ba_predict_options.  Adds "map_covariance" (6, 6), "sigma_pos_m"
        and "sigma_rot_rad" (from covariance-of-the-pixels + map_covariance) to every image's report and returns the
        report.  The response is that of the plain least-squares minimiser over the selected tags."""
        det = self.detectionResults_ if detectionResult is None else detectionResult
        report = self.lastLocalizationReport
        ids = sorted(report)
        tag_ids, tag_qt, tag_wh = self._map_arrays()
        dense = {t: k for k, t in enumerate(tag_ids)}
        joint = self._joint_for_map(*tagJointCovariance)
        img_start, obs_tag, inl = [0], [], []
        for i in ids:
            r = report[i]
            ok = r["status"] == _engine._lib.LOC_OK
            obs_tag += [dense[det.tagObservations[k].tagId] for k in r["observations"]]
            inl += [bool(f) and ok for f in r["inliers"]]
            img_start.append(len(obs_tag))
        cam_qt = np.array([report[i]["pose"] for i in ids], np.float64).reshape(-1, 7)
        size = (options.pop("image_width", self.camModel.horizontalResolution),
                options.pop("image_height", self.camModel.verticalResolution))
        _, cov_map, res, _ = _engine.localization_map_covariance(*self._model_args(), tag_qt, tag_wh, cam_qt, img_start, obs_tag, inl,
                                                                 joint, size, device=self.device, **options)
        for n, i in enumerate(ids):
            report[i].update(map_covariance=cov_map[n].copy(), sigma_pos_m=res[n]["sigma_pos_m"],
                             sigma_rot_rad=res[n]["sigma_rot_rad"])
        return report

    def _pack_rig(self, det, frames, cameraModels, extrinsics, loc_options):
        """The flat arrays engine.rig_localize and engine.rig_calibrate take for `frames` (one list of K image ids per
        frame, None where a camera has no image) against the reconstructed tags.  extrinsics None: every image is
        localised on its own under its camera's model (vmm_ba_localize) and engine.rig_extrinsics_start takes the
        extrinsics from the best frame each camera shares with camera 0.  Returns (order, intr, dist, extrinsics,
        tag_qt, tag_wh, img_start, obs_tag, obs_px); order[k] indexes det.tagObservations."""
        K = len(cameraModels)
        if K < 1 or any(len(frame) != K for frame in frames):
            raise ValueError("every frame lists one image id (or None) per camera of the rig")
        slots = [i for frame in frames for i in frame]
        _, order, tag_qt, tag_wh, real_start, obs_tag, obs_px = self._pack_against_map(det, [i for i in slots if i is not None])
        counts = iter(np.diff(real_start))
        img_start = np.zeros(len(slots) + 1, np.int64)
        img_start[1:] = np.cumsum([0 if i is None else next(counts) for i in slots])
        intr = np.array([[m.fx, m.fy, m.cx, m.cy] for m in cameraModels], np.float64)
        dist = np.array([m.distortionCoefficients for m in cameraModels], np.float64).reshape(K, 5)
        n_frames = len(frames)
        if extrinsics is None:
            cam_qt, res = np.zeros((len(slots), 7)), [None] * len(slots)
            for c in range(K):
                own = np.arange(n_frames) * K + c
                idx = np.concatenate([np.arange(img_start[i], img_start[i + 1]) for i in own]
                                     + [np.zeros(0, np.int64)]).astype(np.int64)
                start = np.zeros(n_frames + 1, np.int64)
                start[1:] = np.cumsum(np.diff(img_start)[own])
                q, _, _, r = _engine.localize(intr[c], dist[c], tag_qt, tag_wh, start, obs_tag[idx], obs_px[idx],
                                              device=self.device, **loc_options)
                cam_qt[own] = q
                for f in range(n_frames):
                    res[f * K + c] = r[f]
            extrinsics = _engine.rig_extrinsics_start(K, n_frames, cam_qt, res)
        extrinsics = np.array(extrinsics, np.float64).reshape(K, 7)
        return order, intr, dist, extrinsics, tag_qt, tag_wh, img_start, obs_tag, obs_px

    @staticmethod
    def _rig_frames_report(K, order, img_start, rig_qt, rig_cov, inl, res):
        rigs, report = {}, []
        for f in range(len(res)):
            report.append(TagReconstructor._item_report(res[f], rig_qt[f], rig_cov[f], order, inl, int(img_start[f * K]),
                                                        int(img_start[f * K + K])))
            if res[f]["status"] == _engine._lib.LOC_OK:
                rigs[f] = Camera(f, rig_qt[f, :4], rig_qt[f, 4:])
        return rigs, report

    def computeRigPosesFromFrames(self, frames, cameraModels, extrinsics=None, detectionResult=None, **options):
        """Localises a rig of K rigidly mounted cameras against the reconstructed tags, one pose per frame
        (vmm_ba_rig_localize).  frames: one list of K image ids per frame, None where a camera has no image;
        cameraModels: the K CameraModels; extrinsics (K, 7) rig->camera as (qw, qx, qy, qz, tx, ty, tz), or None: taken
        from the per-image localisation (engine.rig_extrinsics_start; camera 0 is the rig).  options: the fields of
        vmm_ba_localize_options.  Returns {frame index: Camera} (world->rig) for the frames with status OK;
        lastRigLocalizationReport holds `extrinsics` (K, 7) and `frames`: per frame the status, counts, rms_px, cost, the
        pose, the 6x6 covariance and, per used observation (index into detectionResult.tagObservations), the inlier
        flag.  The reference has no such member."""
        det = self.detectionResults_ if detectionResult is None else detectionResult
        order, intr, dist, extrinsics, tag_qt, tag_wh, img_start, obs_tag, obs_px = self._pack_rig(
            det, frames, cameraModels, extrinsics, options)
        rig_qt, rig_cov, inl, res = _engine.rig_localize(intr, dist, extrinsics, tag_qt, tag_wh, img_start, obs_tag, obs_px,
                                                         device=self.device, **options)
        rigs, report = self._rig_frames_report(len(cameraModels), order, img_start, rig_qt, rig_cov, inl, res)
        self.lastRigLocalizationReport = dict(extrinsics=extrinsics, frames=report)
        return rigs

    def calibrateRig(self, frames, cameraModels, extrinsics=None, detectionResult=None, **options):
        """Calibrates the rig against the reconstructed tags (vmm_ba_rig_calibrate): the extrinsics of the cameras and one
        rig pose per frame are refined together from the detections, the tags and the camera models held fixed.
        frames, cameraModels and extrinsics (the start; None: from the per-image localisation) as
        computeRigPosesFromFrames; options: the fields of vmm_ba_rig_calibrate_options (`loc_<field>` for the initial
        localisation's).  Returns the report: the fields of vmm_ba_rig_calibrate_report plus `extrinsics` (K, 7),
        `covariance` (6 K, 6 K), `rigs` ({frame index: Camera} of the localised frames) and `frames` (per frame as
        lastRigLocalizationReport's, the covariance being the joint marginal).  The reference has no such member."""
        det = self.detectionResults_ if detectionResult is None else detectionResult
        loc = {k[4:]: v for k, v in options.items() if k.startswith("loc_")}
        order, intr, dist, extrinsics, tag_qt, tag_wh, img_start, obs_tag, obs_px = self._pack_rig(
            det, frames, cameraModels, extrinsics, loc)
        ext, ext_cov, rig_qt, rig_cov, inl, res, report = _engine.rig_calibrate(
            intr, dist, extrinsics, tag_qt, tag_wh, img_start, obs_tag, obs_px, device=self.device, **options)
        rigs, per_frame = self._rig_frames_report(len(cameraModels), order, img_start, rig_qt, rig_cov, inl, res)
        return dict(report, extrinsics=ext, covariance=ext_cov, rigs=rigs, frames=per_frame)

    def refineCameraModel(self, imageIds=None, detectionResult=None, **options):
        """Calibrates the camera against the reconstructed tags (vmm_ba_calibrate): the nine numbers of the camera model
        and one pose per image are refined together from the detections, the tags held fixed, starting at the current
        camModel.  options: the fields of vmm_ba_calibrate_options (`loc_<field>` for the initial localisation's).
        Sets camModel to the result when some image took part and returns the report: the fields of
        vmm_ba_calibrate_report plus `intrinsics` (9,), `covariance` (9, 9), `std` (9,) and `cameras`
        ({imageId: Camera} of the localised images; one that took no part in the refinement keeps the localisation's
        pose).  The reference has no such member."""
        det = self.detectionResults_ if detectionResult is None else detectionResult
        ids, order, tag_qt, tag_wh, img_start, obs_tag, obs_px = self._pack_against_map(det, imageIds)
        intr, dist, intr_cov, cam_qt, cam_cov, inl, res, report = _engine.calibrate(
            *self._model_args(), tag_qt, tag_wh, img_start, obs_tag, obs_px, device=self.device, **options)
        report = dict(self._model_report(report, intr, dist, intr_cov),
                      cameras={i: Camera(i, cam_qt[n, :4], cam_qt[n, 4:]) for n, i in enumerate(ids)
                               if res[n]["status"] == _engine._lib.LOC_OK})
        if report["status"] != _engine._lib.CAL_NO_IMAGES:
            self.camModel = self._with_model(intr, dist)
        return report

    def _known_cameras(self, cameras, cameraCovariances):
        """The cameras that triangulatePoints and locateTags work from (default: reconstructedCameras) in image id order:
        (cam_ids, dense {imageId: index}, cam_qt (n, 7), cam_cov (n, 6, 6) or None; a camera without an entry in
        cameraCovariances keeps a zero block)."""
        cams = self.reconstructedCameras if cameras is None else {int(k): v for k, v in dict(cameras).items()}
        cam_ids = sorted(cams)
        cam_qt = np.array([np.concatenate([cams[i].q, cams[i].t]) for i in cam_ids], np.float64).reshape(-1, 7)
        cam_cov = None
        if cameraCovariances is not None:
            cam_cov = np.zeros((len(cam_ids), 6, 6))
            for k, i in enumerate(cam_ids):
                if i in cameraCovariances:
                    cam_cov[k] = np.asarray(cameraCovariances[i], np.float64).reshape(6, 6)
        return cam_ids, {i: k for k, i in enumerate(cam_ids)}, cam_qt, cam_cov

    @staticmethod
    def _pack_items(items, dense, what):
        """An item list over known cameras from [(item id, [(imageId, payload), ...]), ...]: every item's observations
        sorted by image id, those of images outside `dense` dropped.  Returns (start, obs_cam, obs_image, payloads,
        n_dropped); an image that appears twice in an item is refused ("<what> <id> is observed twice in one image")."""
        start, obs_cam, obs_image, payloads, dropped = [0], [], [], [], 0
        for item, observations in items:
            kept = sorted(((int(i), p) for i, p in observations), key=lambda e: e[0])
            seen = [i for i, _ in kept]
            if len(set(seen)) != len(seen):
                raise ValueError("%s %r is observed twice in one image" % (what, item))
            for i, p in kept:
                if i not in dense:
                    dropped += 1
                    continue
                obs_cam.append(dense[i])
                obs_image.append(i)
                payloads.append(p)
            start.append(len(obs_cam))
        return np.array(start, np.int64), np.array(obs_cam, np.int32), obs_image, payloads, dropped

    @staticmethod
    def _pack_tracks(tracks, camera_ids):
        """The flat arrays engine.triangulate takes from {pointId: [(imageId, (u, v)), ...]} (_pack_items; camera_ids
        ascending, position = the camera's index).  Returns (point_ids, pt_start, obs_cam, obs_uv, obs_image, n_dropped)."""
        point_ids = list(tracks)
        pt_start, obs_cam, obs_image, uvs, dropped = TagReconstructor._pack_items(
            [(p, tracks[p]) for p in point_ids], {int(c): k for k, c in enumerate(camera_ids)}, "point")
        obs_uv = np.stack([np.asarray(uv, np.float64).reshape(2) for uv in uvs]) if uvs else np.zeros((0, 2))
        return point_ids, pt_start, obs_cam, obs_uv, obs_image, dropped

    def triangulatePoints(self, tracks, cameras=None, cameraCovariances=None, **options):
        """Free points (anything that is not a tag) in the map's frame from pixels in images with a known pose
        (vmm_ba_triangulate): the dual of computeRelativeCameraPosesFromImgs.  tracks: {pointId: [(imageId, (u, v)), ...]}.
        cameras: {imageId: Camera}, default reconstructedCameras (a localisation's result works as well).
        cameraCovariances: {imageId: 6x6} in tangent order (computePoseCovariances()["cameras"], or the covariances of
        lastLocalizationReport); a camera without an entry counts as exact.  options: the fields of
        vmm_ba_triangulate_options.  Observations of images without a pose are dropped (lastTriangulationDropped counts
        them).  Returns {pointId: {"point" (3,), "covariance" (3, 3) from the pixel noise, "covariance_cameras" (3, 3)
        propagated from cameraCovariances camera by camera, "status", "n_obs", "n_inlier_obs", "rms_px",
        "inliers": {imageId: bool}}}.  The reference has no such member."""
        cam_ids, _, cam_qt, cam_cov = self._known_cameras(cameras, cameraCovariances)
        point_ids, pt_start, obs_cam, obs_uv, obs_image, dropped = self._pack_tracks(tracks, cam_ids)
        self.lastTriangulationDropped = dropped
        xyz, cov, cov_cams, inl, res = _engine.triangulate(*self._model_args(), cam_qt, pt_start, obs_cam, obs_uv,
                                                           cam_cov=cam_cov, device=self.device, **options)
        out = {}
        for n, pid in enumerate(point_ids):
            b, e = int(pt_start[n]), int(pt_start[n + 1])
            out[pid] = {"point": xyz[n].copy(), "covariance": cov[n].copy(), "covariance_cameras": cov_cams[n].copy(),
                        "status": res[n]["status"], "n_obs": res[n]["n_obs"], "n_inlier_obs": res[n]["n_inlier_obs"],
                        "rms_px": res[n]["rms_px"], "inliers": {obs_image[k]: bool(inl[k]) for k in range(b, e)}}
        return out

    def triangulateTagCorners(self, tagIds=None, **options):
        """Measures the true shape of the reconstructed tags: the four corners of every tag (default: all; `tagIds`
        restricts them) are triangulated as four free points from the corner pixels of the tag's detections in images
        with a pose, without the rigid rectangle of the declared size that the bundle adjustment assumes.  options: as
        triangulatePoints.  Returns {tagId: {"corners" (4, 3) LL, LR, UR, UL, "width" / "height" (the mean of the two
        opposite sides), "width_ratio" / "height_ratio" (against the declared size), "out_of_plane" (distance of UR from
        the plane through the other three), "model_gap" (largest distance between a triangulated corner and the map's
        computeMarkerCorners3D()), "status" (the worst of the four VMM_BA_TRI_* statuses)}}."""
        ids = sorted(self.reconstructedTags) if tagIds is None else [int(t) for t in tagIds]
        wanted = set(ids)
        tracks = {(t, k): [] for t in ids for k in range(4)}
        for ob in self.detectionResults_.tagObservations:
            if ob.tagId in wanted and ob.imageId in self.reconstructedCameras:
                for k in range(4):
                    tracks[(ob.tagId, k)].append((ob.imageId, ob.corners[k]))
        pts = self.triangulatePoints(tracks, **options)
        out = {}
        for t in ids:
            tag = self.reconstructedTags[t]
            c = np.stack([pts[(t, k)]["point"] for k in range(4)])
            width = 0.5 * (np.linalg.norm(c[1] - c[0]) + np.linalg.norm(c[2] - c[3]))
            height = 0.5 * (np.linalg.norm(c[3] - c[0]) + np.linalg.norm(c[2] - c[1]))
            normal = np.cross(c[1] - c[0], c[3] - c[0])
            nn = np.linalg.norm(normal)
            gap = max(np.linalg.norm(c[k] - m) for k, m in enumerate(tag.computeMarkerCorners3D()))
            out[t] = {"corners": c, "width": float(width), "height": float(height),
                      "width_ratio": float(width / tag.tagWidth) if tag.tagWidth > 0 else 0.0,
                      "height_ratio": float(height / tag.tagHeight) if tag.tagHeight > 0 else 0.0,
                      "out_of_plane": float(abs(np.dot(c[2] - c[0], normal)) / nn) if nn > 0 else 0.0,
                      "model_gap": float(gap), "status": max(pts[(t, k)]["status"] for k in range(4))}
        return out

    def locateTags(self, cameras=None, cameraCovariances=None, tagIds=None, detectionResult=None, **options):
        """Poses of tags from images with a known pose (vmm_ba_locate_tags): the dual of
        computeRelativeCameraPosesFromImgs.  cameras: {imageId: Camera}, default reconstructedCameras (a localisation's
        result works as well).  cameraCovariances: {imageId: 6x6} in tangent order; a camera without an entry counts as
        exact.  tagIds: default every tag the reconstructor or `detectionResult` (default: the reconstructor's own
        detections) knows the size of.  options: the fields of vmm_ba_localize_options; min_inlier_tags counts a tag's
        inlier observations.  Observations in images without a pose are dropped.  Returns {tagId: ReconstructedTag} for
        the tags with status OK; lastTagLocationReport holds per tag id the status, counts, rms_px, cost, the pose, the
        6x6 covariance from the pixel noise (`covariance`), the part propagated from cameraCovariances camera by camera
        (`covariance_cameras`) and the inlier flag of each used observation (index into detectionResult.tagObservations).
        The reference has no such member."""
        det = self.detectionResults_ if detectionResult is None else detectionResult
        _, dense, cam_qt, cam_cov = self._known_cameras(cameras, cameraCovariances)
        known = {int(t.tagId): (t.tagType, t.width, t.height) for t in det.tags}
        known.update({int(i): (t.tagType, t.tagWidth, t.tagHeight) for i, t in self.reconstructedTags.items()})
        ids = sorted(known) if tagIds is None else [int(t) for t in tagIds]
        per_tag = {t: [] for t in ids}
        for k, ob in enumerate(det.tagObservations):
            if ob.tagId in per_tag and ob.imageId in dense:
                per_tag[ob.tagId].append((ob.imageId, k))
        tag_start, obs_cam, _, order, _ = self._pack_items([(t, per_tag[t]) for t in ids], dense, "tag")
        obs_px = (np.stack([np.asarray(det.tagObservations[k].corners, np.float64).reshape(8) for k in order])
                  if order else np.zeros((0, 8)))
        tag_wh = np.array([known[t][1:] for t in ids], np.float64).reshape(-1, 2)
        tag_qt, cov, cov_cams, inl, res = _engine.locate_tags(*self._model_args(), cam_qt, tag_wh, tag_start, obs_cam, obs_px,
                                                              cam_cov=cam_cov, device=self.device, **options)
        tags, report = {}, {}
        for n, t in enumerate(ids):
            report[t] = self._item_report(res[n], tag_qt[n], cov[n], order, inl, int(tag_start[n]), int(tag_start[n + 1]))
            report[t]["covariance_cameras"] = cov_cams[n].copy()
            if res[n]["status"] == _engine._lib.LOC_OK:
                tags[t] = ReconstructedTag(t, known[t][0], tag_qt[n, :4], tag_qt[n, 4:], known[t][1], known[t][2])
        self.lastTagLocationReport = report
        return tags

    def predictLocalizationAccuracy(self, cameras, tagCovariances=None, tagJointCovariance=None, **options):
        """How well a camera would be localised against the reconstructed tags at poses that have no image behind them
        (vmm_ba_predict_localization).  cameras: {id: Camera} or an (n, 7) array of world->camera poses (ids 0..n-1).
        tagCovariances: {tagId: 6x6} in tangent order (computePoseCovariances()["tags"]); a tag without an entry (the
        origin tag) counts as exact.  options: the fields of vmm_ba_predict_options; image_width / image_height default
        to the camera model's horizontalResolution / verticalResolution.  Occlusion is not modelled.  Returns
        {id: {"status", "n_visible", "sigma_pos_m", "sigma_rot_rad", "pose" (7,), "covariance" (6, 6) from the pixel noise,
        "covariance_map" (6, 6) propagated from tagCovariances tag by tag, "visible_tags": [tag ids]}}.  The reference has
        no such member.
        tagJointCovariance: (tag ids, (T, T, 6, 6)) as computePoseCovariances(jointTags=True)["tag_joint"], instead of
        tagCovariances: covariance_map is then propagated with the correlations between the tags
        (vmm_ba_predict_localization_joint).  Its ids must cover the reconstructed tags."""
        if tagJointCovariance is not None:
            if tagCovariances is not None:
                raise ValueError("tagCovariances and tagJointCovariance are given both: a map has one covariance")
            options["tag_cov_joint"] = self._joint_for_map(*tagJointCovariance)
        if isinstance(cameras, dict):
            ids = sorted(int(k) for k in cameras)
            cams = {int(k): v for k, v in cameras.items()}
            cam_qt = np.array([np.concatenate([cams[i].q, cams[i].t]) for i in ids], np.float64).reshape(-1, 7)
        else:
            cam_qt = np.ascontiguousarray(cameras, np.float64).reshape(-1, 7)
            ids = list(range(len(cam_qt)))
        tag_ids, tag_qt, tag_wh = self._map_arrays()
        tag_cov = None
        if tagCovariances is not None:
            tag_cov = np.zeros((len(tag_ids), 6, 6))
            for k, t in enumerate(tag_ids):
                if t in tagCovariances:
                    tag_cov[k] = np.asarray(tagCovariances[t], np.float64).reshape(6, 6)
        size = (options.pop("image_width", self.camModel.horizontalResolution),
                options.pop("image_height", self.camModel.verticalResolution))
        cov_px, cov_map, res, vis = _engine.predict_localization(*self._model_args(), tag_qt, tag_wh, cam_qt, size,
                                                                 tag_cov=tag_cov, device=self.device, want_visible=True,
                                                                 **options)
        return {i: dict(res[n], pose=cam_qt[n].copy(), covariance=cov_px[n].copy(), covariance_map=cov_map[n].copy(),
                        visible_tags=[tag_ids[k] for k in np.flatnonzero(vis[n])]) for n, i in enumerate(ids)}

    def checkMap(self, detectionResult=None, imageIds=None, sigma_px=1.0, chi2_threshold=22.458, min_views=2, rounds=2,
                 **options):
        """Which tags of the map are no longer where the map says?  Fresh images (`detectionResult`, default the
        reconstructor's own detections; `imageIds` restricts them) are localised against the reconstructed tags
        (vmm_ba_localize), then every map tag seen in at least min_views of the images whose localisation is OK is located
        from those cameras (vmm_ba_locate_tags), the localisation's covariances passed on.  Per tag:
        delta = engine.pose_minus(located, map), Sigma = sigma_px^2 (tag_cov + tag_cov_cams), d2 = delta^T Sigma^-1 delta,
        moved = d2 > chi2_threshold (22.458: the 0.999 quantile of chi-square with 6 degrees of freedom), and the largest
        displacement of the tag's four world corners in metres, which is reported and not thresholded.  When a round
        flags something and rounds >= 2, the observations of the flagged tags are dropped from the localisation input,
        the images are localised again, all tags are located again and that round is reported.  options: the fields of
        vmm_ba_localize_options, given to both steps.
        The statistic IGNORES the correlations between cameras (tag_cov_cams is the independent-cameras figure), the map's
        own uncertainty (the map pose is taken as exact), and the fact that an unmoved tag helped localise the cameras it
        is then tested against, which makes its d2 smaller than chi-square says.  Treat the threshold as a ranking
        aid with a known bias towards "not moved", not as a calibrated test.
        Returns and keeps as lastMapCheckReport: {"rounds", "sigma_px", "chi2_threshold", "images": {imageId: status},
        "tags": {tagId: {"status", "n_obs", "n_inlier_obs", "rms_px", "pose", "covariance" (Sigma), "delta",
        "mahalanobis2", "max_corner_displacement", "moved"}}, "skipped": tag ids with fewer than min_views views,
        "moved": the flagged tag ids}."""
        det = self.detectionResults_ if detectionResult is None else detectionResult
        LOC_OK = _engine._lib.LOC_OK
        flagged, report = [], None
        for rnd in range(1, max(int(rounds), 1) + 1):
            cams = self._localize_images(det, imageIds, set(flagged), options)
            loc = self.lastLocalizationReport
            views = {t: 0 for t in self.reconstructedTags}
            for ob in det.tagObservations:
                if ob.imageId in cams and ob.tagId in views:
                    views[ob.tagId] += 1
            checked = sorted(t for t, n in views.items() if n >= min_views)
            self.locateTags(cams, {i: loc[i]["covariance"] for i in cams}, checked, det, **options)
            tags = {}
            for t in checked:
                r, ref = self.lastTagLocationReport[t], self.reconstructedTags[t]
                entry = {k: r[k] for k in ("status", "n_obs", "n_inlier_obs", "rms_px", "pose")}
                sigma = sigma_px * sigma_px * (r["covariance"] + r["covariance_cameras"])
                delta, d2, gap = np.zeros(6), 0.0, 0.0
                if r["status"] == LOC_OK:
                    delta = _engine.pose_minus(r["pose"], np.concatenate([ref.q, ref.t]))
                    d2 = float(delta @ np.linalg.solve(sigma, delta))
                    there = ReconstructedTag(t, ref.tagType, r["pose"][:4], r["pose"][4:], ref.tagWidth, ref.tagHeight)
                    gap = max(float(np.linalg.norm(np.asarray(a) - np.asarray(b)))
                              for a, b in zip(there.computeMarkerCorners3D(), ref.computeMarkerCorners3D()))
                entry.update(covariance=sigma, delta=delta, mahalanobis2=d2, max_corner_displacement=gap,
                             moved=bool(d2 > chi2_threshold))
                tags[t] = entry
            moved = [t for t in checked if tags[t]["moved"]]
            report = {"rounds": rnd, "sigma_px": float(sigma_px), "chi2_threshold": float(chi2_threshold),
                      "images": {i: loc[i]["status"] for i in sorted(loc)}, "tags": tags,
                      "skipped": sorted(t for t in views if t not in tags), "moved": moved}
            if not moved or set(moved) <= set(flagged):
                break
            flagged = sorted(set(flagged) | set(moved))
        self.lastMapCheckReport = report
        return report

    def moveTagIntoOrigin(self, tagId):
        """src/TagReconstructor.cpp:314-338 (applies the same map to tags AND cameras, as the reference does)."""
        if tagId not in self.reconstructedTags:
            raise RuntimeError("Tag with id %d is not reconstructed." % tagId)
        print("Transforming tag with id %d into origin." % tagId)
        q0 = self.reconstructedTags[tagId].quat()
        qinv = np.array([q0[0], -q0[1], -q0[2], -q0[3]]) / float(q0 @ q0)
        t0 = self.reconstructedTags[tagId].t.copy()
        R = _quat_to_R(qinv)
        for tag in self.reconstructedTags.values():
            tag.setQuat(_quat_mul(qinv, tag.quat()))
            tag.t = R @ (tag.t - t0)
        for cam in self.reconstructedCameras.values():
            cam.setQuat(_quat_mul(qinv, cam.quat()))
            cam.t = R @ (cam.t - t0)
        print("Finished transforming Tags")

    # -- packing of the map state into the flat arrays of the C-ABI --
    def _obs_arrays(self):
        """The observation list as arrays (image id, tag id, 8 pixel coordinates), rebuilt only when the list object
        or its length changes: the incremental driver packs the problem three times per image."""
        obs = self.detectionResults_.tagObservations
        key = (id(obs), len(obs))
        if self._obs_cache is None or self._obs_cache[0] != key:
            img = np.fromiter((ob.imageId for ob in obs), np.int64, len(obs))
            tag = np.fromiter((ob.tagId for ob in obs), np.int64, len(obs))
            px = (np.stack([np.asarray(ob.corners, np.float64).reshape(8) for ob in obs]) if len(obs)
                  else np.zeros((0, 8)))
            self._obs_cache = (key, img, tag, px)
        return self._obs_cache[1:]

    def _pack(self, for_ba):
        """Dense problem arrays exactly as doBundleAdjustment assembles the ceres::Problem
        (src/TagReconstructor.cpp:663-724): tags in map (id) order; cameras with >= 1 reconstructed tag
        in map order (for_ba) or all cameras (statistics); observations whose camera and tag are both
        reconstructed, in file order."""
        if self._resident:
            return self._pack_resident(for_ba)
        return self._pack_cold(for_ba)

    def _pack_cold(self, for_ba):
        """_pack without the device-resident variant: the arrays of this step's problem alone."""
        # the cost functor receives the DETECTION tag's width/height but builds the quad from the reconstructed tag's
        # (:713 vs :718); only the quad enters the arithmetic, so tag_wh is the reconstructed tags'
        tag_ids, tag_qt, tag_wh = self._map_arrays()
        ob_img, ob_tag, ob_px = self._obs_arrays()
        tag_arr = np.asarray(tag_ids, np.int64)
        tag_ok = np.isin(ob_tag, tag_arr)
        images_with_tags = set(np.unique(ob_img[tag_ok]).tolist())                            # :679-684
        cam_ids = [cid for cid in sorted(self.reconstructedCameras)
                   if (cid in images_with_tags or not for_ba)]                               # :689-690
        cam_arr = np.asarray(cam_ids, np.int64)
        keep = tag_ok & np.isin(ob_img, cam_arr)                                              # :699-708
        # ids -> dense indices (both id lists are sorted)
        obs_cam = np.searchsorted(cam_arr, ob_img[keep]).astype(np.int32)
        obs_tag = np.searchsorted(tag_arr, ob_tag[keep]).astype(np.int32)
        obs_px = ob_px[keep]
        cam_qt = np.array([np.r_[self.reconstructedCameras[c].q, self.reconstructedCameras[c].t] for c in cam_ids],
                          np.float64).reshape(-1, 7)
        fixed = tag_ids.index(self.originTagId) if self.originTagId in self.reconstructedTags else -1   # :669-673
        intr, dist = self._model_args()
        tag_const = np.isin(tag_arr, np.asarray(sorted(self.constantTagIds), np.int64)).astype(np.uint8)
        return dict(tag_ids=tag_ids, cam_ids=cam_ids, intr=intr, dist=dist,
                    cam_qt=cam_qt, tag_qt=tag_qt, tag_wh=tag_wh, fixed=fixed, tag_const=tag_const,
                    obs_cam=obs_cam, obs_tag=obs_tag, obs_px=np.ascontiguousarray(obs_px, np.float64).reshape(-1, 8),
                    cam_rows=list(range(len(cam_ids))), tag_rows=list(range(len(tag_ids))), mask=None, key=None,
                    n_active=int(len(obs_cam)))

    def _pack_resident(self, for_ba):
        """Device-resident variant used by startReconstruction: the arrays describe EVERY image, tag and
        observation of the detection result (built once), and the step's problem is a mask over the observations
        (camera and tag both reconstructed, :699-708) -- vmm_ba_set_observation_mask.  cam_ids / tag_ids list the
        poses of this step like the cold packing does; cam_rows / tag_rows are their rows in the full arrays.
        Poses that are not reconstructed yet sit at harmless finite defaults; they have no active observation."""
        ob_img, ob_tag, ob_px = self._obs_arrays()
        full = self._full
        if full is None or full["src"] is not self._obs_cache:
            all_cams = np.unique(np.concatenate([ob_img, np.asarray([i.imageId for i in self.detectionResults_.images],
                                                                    np.int64)]))
            det_tags = {t.tagId: t for t in self.detectionResults_.tags}
            all_tags = np.unique(np.concatenate([ob_tag, np.asarray(sorted(det_tags), np.int64)]))
            wh = np.array([[det_tags[t].width, det_tags[t].height] if t in det_tags else [1.0, 1.0]
                           for t in all_tags.tolist()], np.float64).reshape(-1, 2)
            full = dict(src=self._obs_cache, cams=all_cams, tags=all_tags, tag_wh=wh,
                        obs_cam=np.searchsorted(all_cams, ob_img).astype(np.int32),
                        obs_tag=np.searchsorted(all_tags, ob_tag).astype(np.int32),
                        obs_px=np.ascontiguousarray(ob_px, np.float64).reshape(-1, 8))
            self._full = full
        tag_ids = sorted(self.reconstructedTags)
        tag_arr = np.asarray(tag_ids, np.int64)
        rec_cams = np.asarray(sorted(self.reconstructedCameras), np.int64)
        tag_ok = np.isin(ob_tag, tag_arr)
        mask = tag_ok & np.isin(ob_img, rec_cams)
        images_with_tags = set(np.unique(ob_img[mask]).tolist())
        cam_ids = [c for c in rec_cams.tolist() if (c in images_with_tags or not for_ba)]
        cam_rows = np.searchsorted(full["cams"], np.asarray(cam_ids, np.int64)).tolist()
        tag_rows = np.searchsorted(full["tags"], tag_arr).tolist()
        cam_qt = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 1.0]), (len(full["cams"]), 1))   # identity, 1 m in front
        tag_qt = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0.0]), (len(full["tags"]), 1))
        for c, r in zip(cam_ids, cam_rows):
            cam_qt[r] = np.r_[self.reconstructedCameras[c].q, self.reconstructedCameras[c].t]
        tag_wh = full["tag_wh"].copy()
        for t, r in zip(tag_ids, tag_rows):
            tag_qt[r] = np.r_[self.reconstructedTags[t].q, self.reconstructedTags[t].t]
            tag_wh[r] = (self.reconstructedTags[t].tagWidth, self.reconstructedTags[t].tagHeight)
        fixed = (int(np.searchsorted(full["tags"], self.originTagId))
                 if self.originTagId in self.reconstructedTags else -1)
        intr, dist = self._model_args()
        key = ("resident", id(full), fixed, tuple(float(v) for v in intr), tuple(float(v) for v in dist), tag_wh.tobytes())
        # constant tags: rows of the full arrays; only reconstructed ones (the others have no active observation)
        tag_const = np.zeros(len(full["tags"]), np.uint8)
        for t, r in zip(tag_ids, tag_rows):
            if t in self.constantTagIds:
                tag_const[r] = 1
        return dict(tag_ids=tag_ids, cam_ids=cam_ids, cam_rows=cam_rows, tag_rows=tag_rows, intr=intr, dist=dist,
                    cam_qt=cam_qt, tag_qt=tag_qt, tag_wh=tag_wh, fixed=fixed, tag_const=tag_const, obs_cam=full["obs_cam"], obs_tag=full["obs_tag"], obs_px=full["obs_px"],
                    mask=mask, key=key, n_active=int(mask.sum()))

    def _engine_for(self, p, **kw):
        """A device handle for the packed problem.  The handle of the previous call is kept and reused when the
        problem structure (ids, observations, constants) is unchanged -- the usual case for the statistics that
        follow every bundle adjustment of the incremental driver -- so only the 7 doubles per pose travel."""
        if p.get("key") is not None:
            key = (p["key"], tuple(sorted(kw.items())))
        else:
            import hashlib
            h = hashlib.blake2b(digest_size=16)
            for a in (np.asarray(p["cam_ids"], np.int64), np.asarray(p["tag_ids"], np.int64), p["obs_cam"],
                      p["obs_tag"], p["obs_px"], p["tag_wh"], np.asarray(p["intr"], np.float64),
                      np.asarray(p["dist"], np.float64)):
                h.update(np.ascontiguousarray(a).tobytes())
                h.update(b"|")
            key = (h.hexdigest(), int(p["fixed"]), tuple(sorted(kw.items())))
        if self._cached is not None and self._cached[0] == key and not os.environ.get("VMM_BA_NO_HANDLE_CACHE"):
            ba = self._cached[1]
            ba.set_state(p["cam_qt"], p["tag_qt"])
            ba.set_observation_mask(p.get("mask"))
            self._set_constants(ba, p)
            return ba
        self._drop_cached()
        ba = _engine.BundleAdjuster(p["intr"], p["dist"], p["cam_qt"], p["tag_qt"], p["tag_wh"], p["fixed"],
                                    p["obs_cam"], p["obs_tag"], p["obs_px"], device=self.device, **kw)
        if p.get("mask") is not None:
            ba.set_observation_mask(p["mask"])
        self._set_constants(ba, p)
        self._cached = (key, ba)
        return ba

    @contextlib.contextmanager
    def _handle(self, p, **kw):
        """_engine_for(p, **kw) for the length of a block; a call that fails inside it drops the cached handle."""
        ba = self._engine_for(p, **kw)
        try:
            yield ba
        except Exception:
            self._drop_cached()
            raise

    @staticmethod
    def _is_empty(p, observations=True):
        """No camera, no tag or (observations) no active observation in the packed problem."""
        return len(p["cam_ids"]) == 0 or len(p["tag_ids"]) == 0 or (observations and p["n_active"] == 0)

    @staticmethod
    def _set_constants(ba, p):
        """The packed constant-tag flags go to the handle when they differ from what it holds (constantTagIds)."""
        tc = p.get("tag_const")
        want = tc.tobytes() if tc is not None and tc.any() else None
        if ba.constant_poses != (None, want):
            ba.set_constant_poses(None, tc if want is not None else None)

    def _drop_cached(self):
        if self._cached is not None:
            self._cached[1].close()
            self._cached = None

    def close(self):
        """Releases the cached device handle (also done on garbage collection)."""
        self._drop_cached()

    def __del__(self):
        try:
            self._drop_cached()
        except Exception:   # noqa: BLE001 -- interpreter shutdown
            pass

    # -- the hot path --
    def _pack_for_ba(self):
        """The packed problem of a bundle adjustment, or None for an empty one -- Ceres solves that trivially:
        CONVERGENCE, nothing changes."""
        p = self._pack(for_ba=True)
        if self._is_empty(p):
            print("Solution %d" % _engine.CONVERGENCE)
            self.lastSummary = {"termination_type": _engine.CONVERGENCE, "iterations": 1}
            return None
        return p

    def _write_back_cameras(self, p, cam):
        for k, cid in zip(p["cam_rows"], p["cam_ids"]):
            self.reconstructedCameras[cid].q = cam[k, :4].copy()
            self.reconstructedCameras[cid].t = cam[k, 4:].copy()

    def doBundleAdjustment(self, maxNumIterations, ceresThreads=1, robustify=True, printSummary=False,
                           elimination=_engine.ELIM_AUTO, refineCameraModel=False, refine_mask=0x1FF, oneLaunch=False):
        """src/TagReconstructor.cpp:646-743.  Poses are updated in place like the reference's map nodes.

        oneLaunch (or startReconstruction(oneLaunch=True) while it runs): a bundle adjustment whose kept family has at
        most _lib.SMALL_MAX_KEPT poses is solved by engine.solve_small from this step's own arrays -- one launch, no
        handle; one that does not fit, and every printSummary or refineCameraModel request, takes the path below.

        refineCameraModel (not in the reference, which takes the camera model as given): the parameters of refine_mask
        (bit i = parameter i of fx, fy, cx, cy, k1, k2, p1, p2, k3) are refined together with the poses
        (vmm_ba_solve_selfcal); camModel becomes the result and lastSelfCalibrationReport holds the fields of
        vmm_ba_selfcal_report plus `intrinsics` (9,), `covariance` (9, 9) and `std` (9,).  lastSummary is then the
        summary of the last inner solve.  The inner solves run with function_tolerance 1e-14 and parameter_tolerance
        1e-12 instead of the defaults, which stop too early for the outer loop's cost comparisons."""
        if (oneLaunch or self._oneLaunch) and not printSummary and not refineCameraModel \
                and self._bundle_adjust_in_one_launch(maxNumIterations, ceresThreads, robustify, elimination):
            return
        p = self._pack_for_ba()
        if p is None:
            return
        with self._handle(p, elimination=elimination) as ba:
            opts = _engine.default_options(max_num_iterations=int(maxNumIterations), robustify=int(bool(robustify)),
                                           num_threads=int(ceresThreads))
            trace_capacity = int(maxNumIterations) + 2 if printSummary else 0
            if refineCameraModel:
                # the outer loop compares the costs of consecutive solves down to a relative 1e-12: every inner solve
                # has to converge well below Ceres' default stopping rules (a relative cost decrease of 1e-6)
                opts.function_tolerance, opts.parameter_tolerance = 1e-14, 1e-12
                intr, dist, intr_cov, report, summary = ba.solve_selfcal(opts, trace_capacity=trace_capacity,
                                                                         refine_mask=int(refine_mask))
            else:
                summary = ba.solve(opts, trace_capacity=trace_capacity)
            cam, tag = ba.get_state()
            cov = ba.tag_translation_covariance(robustify, opts.huber_a) if printSummary else None   # :744-760
        self._write_back_cameras(p, cam)
        for k, tid in zip(p["tag_rows"], p["tag_ids"]):
            self.reconstructedTags[tid].q = tag[k, :4].copy()
            self.reconstructedTags[tid].t = tag[k, 4:].copy()
        self.lastSummary = summary
        if refineCameraModel:
            self.camModel = self._with_model(intr, dist)
            self.lastSelfCalibrationReport = self._model_report(report, intr, dist, intr_cov)
            self._drop_cached()   # the cached handle is keyed by the model it was created with
            print("Camera model refined: status %d, %d outer iterations (%d accepted), cost %.6e -> %.6e" % (
                report["status"], report["outer_iterations"], report["accepted"], report["initial_cost"],
                report["final_cost"]))
        print("Solution %d" % summary["termination_type"])                                   # :740
        if printSummary:                                                                     # :741-742
            print("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius")
            for it in summary["trace"]:
                print("%4d  %.6e  %9.2e  %9.2e  %9.2e  %9.2e  %9.2e" % (
                    it["iteration"], it["cost"], it["cost_change"], it["gradient_max_norm"], it["step_norm"],
                    it["relative_decrease"], it["trust_region_radius"]))
            print("Cost: initial %.6e final %.6e; iterations %d; time in solver %.4f s" % (
                summary["initial_cost"], summary["final_cost"], summary["iterations"], summary["time_solve_s"]))
            print("Time (s): residual + Jacobian evaluation %.6f, elimination + rank-k update %.6f, linear solver %.6f, "
                  "step + candidate cost %.6f, trust-region control %.6f" % (
                      summary["time_eval_s"], summary["time_eliminate_s"], summary["time_factor_solve_s"],
                      summary["time_step_s"], summary["time_control_s"]))
            # covariance report, :761-782 (Eigen prints a row vector with single spaces, 6 significant digits)
            self.lastCovariances = {}
            avg_diag = np.zeros(3)
            for k, tid in zip(p["tag_rows"], p["tag_ids"]):
                self.lastCovariances[tid] = cov[k].copy()
                diag = np.diag(cov[k])
                std = np.sqrt(diag)
                print("StdDev of tag %d: %s | StdDevNorm: %s" % (
                    tid, " ".join("%.6g" % v for v in std), "%.6g" % math.sqrt(np.linalg.norm(std))))
                avg_diag += diag
            avg_diag /= len(p["tag_ids"])
            print("Marker Position RMS = %.6g" % np.linalg.norm(np.sqrt(avg_diag)))

    def _write_back_poses(self, p, cam, tag):
        self._write_back_cameras(p, cam)
        for k, tid in zip(p["tag_rows"], p["tag_ids"]):
            self.reconstructedTags[tid].q = tag[k, :4].copy()
            self.reconstructedTags[tid].t = tag[k, 4:].copy()

    def _bundle_adjust_in_one_launch(self, maxNumIterations, ceresThreads, robustify, elimination):
        """doBundleAdjustment through engine.solve_small; False (nothing done) when the kept family does not fit."""
        p = self._pack_cold(for_ba=True)
        if self._is_empty(p):
            return False   # the existing path reports the empty problem
        n_cams, n_tags = len(p["cam_ids"]), len(p["tag_ids"])
        elim_cams = n_cams >= n_tags if elimination == _engine.ELIM_AUTO else elimination == _engine.ELIM_CAMERAS
        if (n_tags if elim_cams else n_cams) > _engine._lib.SMALL_MAX_KEPT:
            return False
        opts = _engine.default_options(max_num_iterations=int(maxNumIterations), robustify=int(bool(robustify)),
                                       num_threads=int(ceresThreads))
        problem = (p["intr"], p["dist"], p["cam_qt"], p["tag_qt"], p["tag_wh"], p["fixed"], p["obs_cam"], p["obs_tag"],
                   p["obs_px"])
        tc = p.get("tag_const")
        (cam, tag, summary), = _engine.solve_small([problem], tag_const=[tc] if tc is not None and tc.any() else None,
                                                   options=opts, elimination=elimination, device=self.device)
        self._write_back_poses(p, cam, tag)
        self.lastSummary = summary
        print("Solution %d" % summary["termination_type"])                                   # :740
        return True

    def computePoseCovariances(self, robustify=False, jointTags=False):
        """The 6x6 covariance (tangent order: translation, then rotation) of every reconstructed tag and camera at the
        current poses, no solve: the problem doBundleAdjustment builds (origin tag and constantTagIds constant), then
        one vmm_ba_covariance_blocks call for all marginals.  Fills and returns self.lastPoseCovariances =
        {"tags": {id: 6x6}, "cameras": {id: 6x6}}; the origin tag and the constant tags are zeros.  Not in the
        reference, which asks Ceres for the tags' (t, t) blocks only (src/TagReconstructor.cpp:744-783).
        jointTags: one more call for the tags' cross blocks; "tag_joint": (tag ids, (T, T, 6, 6)) holds the tags' joint
        covariance, block [i, j] that of tag_ids[i] and tag_ids[j] (BundleAdjuster.tag_joint_covariance)."""
        self.lastPoseCovariances = {"tags": {}, "cameras": {}}
        p = self._pack(for_ba=True)
        if self._is_empty(p):
            return self.lastPoseCovariances
        joint = None
        with self._handle(p, elimination=_engine.ELIM_AUTO) as ba:
            cam_cov, tag_cov = ba.pose_covariances(robustify, _engine.default_options().huber_a)
            if jointTags:
                joint = ba.tag_joint_covariance(robustify, _engine.default_options().huber_a)
        self.lastPoseCovariances["tags"] = {t: tag_cov[k].copy() for k, t in zip(p["tag_rows"], p["tag_ids"])}
        self.lastPoseCovariances["cameras"] = {c: cam_cov[k].copy() for k, c in zip(p["cam_rows"], p["cam_ids"])}
        if jointTags:
            rows = np.asarray(list(p["tag_rows"]), np.int64)
            self.lastPoseCovariances["tag_joint"] = ([int(t) for t in p["tag_ids"]], joint[np.ix_(rows, rows)].copy())
        return self.lastPoseCovariances

    def doBundleAdjustment_points(self, maxNumIterations, ceresThreads=1, printSummary=False,
                                  elimination=_engine.ELIM_AUTO):
        """src/TagReconstructor.cpp:457-644 (`#if 0` in the reference): the same bundle adjustment with every
        reconstructed tag replaced by its four world corners as free 3-D points (OpenCVReprojectionError,
        TagReconstructionCostFunction.h:9-84; 3x3 landmark blocks, SPARSE_SCHUR ordering :492,534-535), the origin
        tag's corners constant (:494-497), no loss (:556).  Cameras are written back as at :583-605, tag poses are
        rebuilt from the optimised corners as at :608-639 (with today's corner order, see vmm_ba.h); the corners
        themselves are kept in self.lastPoints (tag id -> 4 x 3).  The corners of the tags in constantTagIds are
        constant too, and those tags' q and t are left as they are, bit for bit."""
        p = self._pack_for_ba()
        if p is None:
            return
        with self._handle(p, elimination=elimination, landmarks=_engine.LANDMARK_POINTS) as ba:
            opts = _engine.default_options(max_num_iterations=int(maxNumIterations), robustify=0,
                                           num_threads=int(ceresThreads))
            summary = ba.solve(opts, trace_capacity=int(maxNumIterations) + 2 if printSummary else 0)
            cam, tag = ba.get_state()
            pts = ba.get_points()
        self._write_back_cameras(p, cam)
        self.lastPoints = {}
        for k, tid in zip(p["tag_rows"], p["tag_ids"]):
            self.lastPoints[tid] = pts[k].copy()
            if tid in self.constantTagIds:
                continue    # its corners did not move: the pose keeps its bits instead of being rebuilt from them
            self.reconstructedTags[tid].q = tag[k, :4].copy()
            self.reconstructedTags[tid].t = tag[k, 4:].copy()
        self.lastSummary = summary
        print("Solution %d" % summary["termination_type"])                                   # :579
        print("Cost: initial %.6e final %.6e; iterations %d; time in solver %.4f s" % (     # :580-581 (FullReport)
            summary["initial_cost"], summary["final_cost"], summary["iterations"], summary["time_solve_s"]))

    # -- reprojection statistics + pruning (src/TagReconstructor.cpp:340-455, 786-816) --
    def _stats(self, per_corner):
        p = self._pack(for_ba=False)
        if self._is_empty(p, observations=False):
            return p, np.zeros(0), np.zeros(0), 0.0, np.zeros((0, 8))
        with self._handle(p, elimination=_engine.ELIM_AUTO) as ba:
            pc, pt, avg, corner = ba.reprojection_stats(per_corner=per_corner)
        return p, pc, pt, avg, corner

    def computeReprojectionErrorPerImg(self):
        """:340-385 -- image id -> mean corner reprojection error; -1.0 for a camera without observations."""
        p, pc, _, _, _ = self._stats(False)
        return {cid: float(pc[k]) for k, cid in zip(p["cam_rows"], p["cam_ids"])}

    def computeReprojectionErrorPerTag(self):
        """:387-428 -- returns (tag id -> mean error, avg).  The reference returns avg through a reference
        parameter; tags without observations do not appear in the map."""
        p, _, pt, avg, _ = self._stats(False)
        return {tid: float(pt[k]) for k, tid in zip(p["tag_rows"], p["tag_ids"]) if not math.isnan(pt[k])}, float(avg)

    def computeReprojectionErrorPerCorner(self):
        """:430-455 -- list of signed (du, dv) per detected corner, observation order."""
        p, _, _, _, corner = self._stats(True)
        if p.get("mask") is not None:
            corner = corner[p["mask"]]   # resident packing: only the observations of this step
        return [corner.reshape(-1, 2)[i].copy() for i in range(corner.size // 2)]

    def removeBadMarkers(self, threshold):
        """:786-802."""
        reperrors, _avg = self.computeReprojectionErrorPerTag()
        for tid in sorted(reperrors):
            if reperrors[tid] > threshold and tid != self.originTagId and tid not in self.constantTagIds:
                print("Removing bad marker with id %d and reprojection error %g" % (tid, reperrors[tid]))
                del self.reconstructedTags[tid]

    def removeBadCameras(self, threshold):
        """:804-816."""
        rep = self.computeReprojectionErrorPerImg()
        for cid in sorted(rep):
            if rep[cid] > threshold or rep[cid] < 0:
                print("Removing bad camera with id %d and reprojection error %g" % (cid, rep[cid]))
                del self.reconstructedCameras[cid]


def detection_result_from_arrays(obs_cam, obs_tag, obs_px, tag_wh, n_cams, tag_type="apriltag_36h11"):
    """Builds a DetectionResult (DetectionResults.h:32-37) from flat arrays; image id = camera index."""
    images = [TagImg(i, "img_%05d.jpg" % i) for i in range(n_cams)]
    tags = [Tag(t, tag_type, tag_wh[t][0], tag_wh[t][1]) for t in range(len(tag_wh))]
    obs = [TagObservation(int(c), int(t), np.asarray(px, np.float64).reshape(4, 2))
           for c, t, px in zip(obs_cam, obs_tag, obs_px)]
    return DetectionResult(images, tags, obs)
