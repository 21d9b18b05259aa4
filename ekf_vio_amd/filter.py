"""Host-side mirror of the reference's `class TightlyCoupledEKF`
(include/ekf_vio/TightlyCoupledEKF.h:25-68) over the C-ABI of libekfvio_hip.so.

Same member names and argument meaning as the reference so that tests read like the
reference's own (test/test_ekf.cpp, test/jacobian_test.cpp, test/analyzeEKFSimulation.cpp).
All arithmetic happens in HIP kernels on the MI355X; this file only marshals buffers.
"""
import ctypes as C

import numpy as np

from . import capi

BASE_STATE_SIZE = 22


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


class TightlyCoupledEKF:
    def __init__(self, max_features=100, device=0, stream=None, predict_mode=capi.PREDICT_STRUCTURED,
                 default_point_depth=0.5, default_point_depth_variance=100.0,
                 default_point_homogenous_variance=1e-5, hooks=False, gate_chi2=0.0, klt_fb_max_px=0.0, distortion=None, output_covariance=False,
                 mask=None, mask_rectify_border=False, equalize=None, klt_photometric=False, ended_export=False, zupt=None,
                 imu_extrinsics=None, camera_model=None, replenish_grid=None, frame_aid=None, **cfg_overrides):
        # hooks=True: this handle lives in libekfvio_hip_hooks.so, the build that also has include/ekfvio_test_hooks.h (tests, profiling scripts)
        self.hooks = bool(hooks)
        self.lib = capi.load(hooks=self.hooks)
        cfg = capi.Config()
        self._chk(self.lib.ekfvio_default_config(C.byref(cfg)))
        cfg.max_features = max_features
        cfg.predict_mode = predict_mode
        cfg.default_point_depth = default_point_depth
        cfg.default_point_depth_variance = default_point_depth_variance
        cfg.default_point_homogenous_variance = default_point_homogenous_variance
        cfg.klt_fb_max_px = klt_fb_max_px  # the tracker's forward-backward check, in pixels of the resized frame (0: off)
        for k, v in cfg_overrides.items():
            if k == "gravity":
                cfg.gravity[0], cfg.gravity[1], cfg.gravity[2] = (float(x) for x in v)
            else:
                setattr(cfg, k, v)
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = self.lib.ekfvio_create(C.byref(cfg), device, C.c_void_p(stream) if stream else None, C.byref(self.h))
        if rc != capi.OK:
            # a failed create releases whatever it had allocated and hands back no handle
            self.h = None
            raise capi.EkfvioError(rc, "ekfvio_create failed (device %d)" % device)
        if gate_chi2:  # a property of the handle, not a field of the configuration (ekfvio_set_gate)
            self.setGate(gate_chi2)
        if distortion is not None:  # likewise a property of the handle (ekfvio_set_distortion)
            self.setDistortion(distortion)
        if camera_model is not None:  # likewise (ekfvio_set_camera_model): (model, D[, P]); behind distortion=, so it wins
            self.setCameraModel(*camera_model)
        if output_covariance:  # likewise (ekfvio_set_output_covariance)
            self.setOutputCovariance(True)
        if mask is not None or mask_rectify_border:  # likewise (ekfvio_set_mask)
            self.setMask(mask, rectify_border=mask_rectify_border)
        if equalize is not None:  # likewise (ekfvio_set_equalize)
            self.setEqualize(*equalize)
        if klt_photometric:  # likewise (ekfvio_set_klt_photometric)
            self.setKltPhotometric(True)
        if ended_export:  # likewise (ekfvio_set_ended_export)
            self.setEndedExport(True)
        if zupt is not None:  # likewise (ekfvio_set_zupt)
            self.setZupt(*zupt)
        if imu_extrinsics is not None:  # likewise (ekfvio_set_imu_extrinsics)
            self.setImuExtrinsics(*imu_extrinsics)
        if replenish_grid is not None:  # likewise (ekfvio_set_replenish_grid): (cells_x, cells_y)
            self.setReplenishGrid(*replenish_grid)
        if frame_aid is not None:  # likewise (ekfvio_set_frame_aid): (H, z, R[, chi2])
            self.setFrameAid(*frame_aid)

    def _chk(self, rc, allow=()):
        if rc != capi.OK and rc not in allow:
            msg = self.lib.ekfvio_last_error(self.h).decode() if getattr(self, "h", None) else ""
            raise capi.EkfvioError(rc, msg)
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.ekfvio_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference members -------------------------------------------------------------
    def initializeBaseState(self):
        self._chk(self.lib.ekfvio_reset(self.h))

    def addNewFeatures(self, new_homogenous_features):
        uv = np.ascontiguousarray(new_homogenous_features, dtype=np.float32).reshape(-1, 2)
        self._chk(self.lib.ekfvio_add_features(self.h, _fp(uv), uv.shape[0]))

    def process(self, dt):
        self._chk(self.lib.ekfvio_process(self.h, float(dt)))

    def numericallyLinearizeProcess(self, dt):
        n = self.dim
        F = np.zeros((n, n), dtype=np.float32)
        self._chk(self.lib.ekfvio_linearize(self.h, float(dt), _fp(F)))
        return F.T.copy()

    def updateWithFeaturePositions(self, measured_positions, estimated_covariance, passed):
        """Returns capi.OK or capi.ENUMERIC (non-positive Cholesky pivot; state still updated)."""
        N = self.num_features
        z = np.ascontiguousarray(measured_positions, dtype=np.float32).reshape(-1, 2)
        R = np.ascontiguousarray(estimated_covariance, dtype=np.float32).reshape(-1, 4)
        p = np.ascontiguousarray(passed, dtype=np.uint8).reshape(-1)
        if not (z.shape[0] == R.shape[0] == p.shape[0]):
            raise capi.EkfvioError(capi.EINVAL, "size mismatch")  # ROS_ASSERT :478
        return self._chk(self.lib.ekfvio_update(self.h, _fp(z), _fp(R), _u8(p), p.shape[0]), allow=(capi.ENUMERIC,))

    def formFeatureMeasurementMap(self, measured):
        m = np.ascontiguousarray(measured, dtype=np.uint8)
        idx = np.zeros(2 * len(m) + 1, dtype=np.int32)
        rows = C.c_int32(0)
        self._chk(self.lib.ekfvio_measurement_map(self.h, _u8(m), len(m), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  C.byref(rows)))
        return idx[:rows.value].copy()

    def previousFeaturePositionVector(self):
        return self.get_state()["last_klt"]

    def getFeatureHomogenousCovariance(self, index):
        cov = np.zeros(4, np.float32)
        self._chk(self.lib.ekfvio_get_feature_cov(self.h, index, _fp(cov)))
        return cov.reshape(2, 2).T.copy()

    def setFeatureHomogenousCovariance(self, index, cov):
        """TightlyCoupledEKF.cpp:668-676; cov is [row, col]."""
        c = np.ascontiguousarray(np.asarray(cov, np.float32).reshape(2, 2).T)  # column-major buffer
        self._chk(self.lib.ekfvio_set_feature_cov(self.h, int(index), _fp(c)))

    def getMetric2PixelMap(self, K):
        """TightlyCoupledEKF.cpp:683-689: diag(K(0,0), K(1,1)) as a dense 2x2."""
        K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        J = np.zeros(4, np.float32)
        self._chk(self.lib.ekfvio_metric2pixel_map(_fp(K), _fp(J)))
        return J.reshape(2, 2).T.copy()

    def getPixel2MetricMap(self, K):
        """TightlyCoupledEKF.cpp:691-697: diag(1/K(0,0), 1/K(1,1))."""
        K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        J = np.zeros(4, np.float32)
        self._chk(self.lib.ekfvio_pixel2metric_map(_fp(K), _fp(J)))
        return J.reshape(2, 2).T.copy()

    def getFeatureDepthVariance(self, index):
        v = C.c_float(0)
        self._chk(self.lib.ekfvio_get_depth_variance(self.h, index, C.byref(v)))
        return float(v.value)

    def imuUpdate(self, gyro, accel):
        """the IMU measurement update alone (no propagation); asynchronous."""
        g = np.ascontiguousarray(gyro, dtype=np.float32)
        a = np.ascontiguousarray(accel, dtype=np.float32)
        self._chk(self.lib.ekfvio_imu_update(self.h, _fp(g), _fp(a)))

    def setImuExtrinsics(self, R_ci=None, p_ci=None):
        """Not in the reference: the IMU in its own frame (ekfvio_set_imu_extrinsics).  R_ci [3, 3] maps IMU coordinates to camera coordinates
        (the rotation of Kalibr's T_cam_imu), p_ci is the IMU's origin in the camera frame in metres (its translation); both None: off.
        Holds from the next IMU update and survives initializeBaseState."""
        if R_ci is None and p_ci is None:
            self._chk(self.lib.ekfvio_set_imu_extrinsics(self.h, None, None))
            return
        R = None if R_ci is None else np.ascontiguousarray(R_ci, dtype=np.float32).reshape(9)
        p = None if p_ci is None else np.ascontiguousarray(p_ci, dtype=np.float32).reshape(3)
        self._chk(self.lib.ekfvio_set_imu_extrinsics(self.h, None if R is None else _fp(R), None if p is None else _fp(p)))

    def imuExtrinsics(self):
        """ekfvio_get_imu_extrinsics: (R_ci [3, 3], p_ci [3], on)."""
        R, p, on = np.zeros(9, np.float32), np.zeros(3, np.float32), C.c_int32(0)
        self._chk(self.lib.ekfvio_get_imu_extrinsics(self.h, _fp(R), _fp(p), C.byref(on)))
        return R.reshape(3, 3), p, bool(on.value)

    def setGravity(self, g):
        """ekfvio_set_gravity: replaces the configuration's gravity vector (world frame, m/s^2) from the next IMU update on."""
        g = np.ascontiguousarray(g, dtype=np.float32).reshape(3)
        self._chk(self.lib.ekfvio_set_gravity(self.h, _fp(g)))

    def gravity(self):
        """ekfvio_get_gravity."""
        g = np.zeros(3, np.float32)
        self._chk(self.lib.ekfvio_get_gravity(self.h, _fp(g)))
        return g

    def setZupt(self, max_flow_px, min_tracks=8, min_ratio=0.75, vel_variance=1e-4, omega_variance=1e-4):
        """Not in the reference: the zero-velocity update (ekfvio_set_zupt).  max_flow_px > 0: a frame of addFrame in which at least min_tracks
        landmarks passed the tracker and at least min_ratio of those moved no more than max_flow_px pixels is taken as standing still, and
        z = 0 on the velocity and the body rate (with these variances) updates the propagated state in front of the camera update; 0: off."""
        self._chk(self.lib.ekfvio_set_zupt(self.h, float(max_flow_px), int(min_tracks), float(min_ratio), float(vel_variance), float(omega_variance)))

    def zuptUpdate(self, vel_variance=1e-4, omega_variance=1e-4):
        """ekfvio_zupt_update: that update alone, unconditional (a caller with its own stop detector); asynchronous."""
        self._chk(self.lib.ekfvio_zupt_update(self.h, float(vel_variance), float(omega_variance)))

    def zupt(self):
        """ekfvio_get_zupt: dict(flow2[n], n_landmarks, n_pass, n_still, applied_last, applied_total) of the most recent frame's decision."""
        cap = max(int(self.cfg.max_features), 1)
        flow2 = np.zeros(cap, np.float32)
        n, npass, nstill, last, total = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._chk(self.lib.ekfvio_get_zupt(self.h, _fp(flow2), C.byref(n), C.byref(npass), C.byref(nstill), C.byref(last), C.byref(total)))
        return dict(flow2=flow2[:n.value].copy(), n_landmarks=int(n.value), n_pass=int(npass.value), n_still=int(nstill.value),
                    applied_last=int(last.value), applied_total=int(total.value))

    @staticmethod
    def _aid_rows(H, z, R):
        """(k, H [k * 22], z [k], R [k * k]) as fp32 for the aiding entry points; R may be given as its diagonal."""
        z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
        k = int(z.shape[0])
        H = np.ascontiguousarray(H, dtype=np.float32).reshape(-1)
        R = np.asarray(R, dtype=np.float32)
        R = np.ascontiguousarray(np.diag(R) if R.ndim == 1 and k > 1 and R.size == k else R, dtype=np.float32).reshape(-1)
        if k == 0 or H.size != k * 22 or R.size != k * k:
            raise capi.EkfvioError(capi.EINVAL, "aiding rows: H must be [k, 22], z [k], R [k, k] or its diagonal")
        return k, H, z, R

    def aidUpdate(self, H, z, R, chi2=0.0):
        """Not in the reference: a linear aiding measurement of the base state, z = H x[0:22] + v, v ~ N(0, R), k = 1..6 rows, Joseph form on
        the device (ekfvio_aid_update): wheel speed, a position or altitude fix, a constraint.  chi2 > 0: rejected where the normalised innovation
        squared exceeds it.  The update alone; asynchronous."""
        k, H, z, R = self._aid_rows(H, z, R)
        self._chk(self.lib.ekfvio_aid_update(self.h, k, _fp(H), _fp(z), _fp(R), float(chi2)))

    def aid(self, stamp, H, z, R, chi2=0.0):
        """ekfvio_aid: propagates to `stamp` (process(dt), whatever use_imu says; the first stamp only sets the time), then aidUpdate."""
        k, H, z, R = self._aid_rows(H, z, R)
        self._chk(self.lib.ekfvio_aid(self.h, float(stamp), k, _fp(H), _fp(z), _fp(R), float(chi2)))

    def setFrameAid(self, H=None, z=None, R=None, chi2=0.0):
        """ekfvio_set_frame_aid: a standing measurement applied in every frame of addFrame behind the tracker, in front of the zero-velocity
        update and the camera update (a nonholonomic constraint, a planar robot).  H None: off."""
        if H is None:
            self._chk(self.lib.ekfvio_set_frame_aid(self.h, 0, None, None, None, 0.0))
            return
        k, H, z, R = self._aid_rows(H, z, R)
        self._chk(self.lib.ekfvio_set_frame_aid(self.h, k, _fp(H), _fp(z), _fp(R), float(chi2)))

    def aid_status(self):
        """ekfvio_get_aid: dict(d2_last, accepted_last, applied_total, rejected_total) of the handle's most recent aiding update; a memcpy
        behind a frame, a wait for the stream behind a bare aid / aidUpdate."""
        d2, acc, ap, rej = C.c_float(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.ekfvio_get_aid(self.h, C.byref(d2), C.byref(acc), C.byref(ap), C.byref(rej)))
        return dict(d2_last=float(d2.value), accepted_last=int(acc.value), applied_total=int(ap.value), rejected_total=int(rej.value))

    def removeFeatures(self, mask=None):
        """Not in the reference, which flags a lost landmark (TightlyCoupledEKF.cpp:528) and keeps it: removes landmarks from the
        state (mean, covariance rows and columns, last KLT results, flags), keeping the order of the rest.  mask: one entry per
        landmark, nonzero = remove; None: the landmarks flagged for deletion.  Returns the number removed."""
        k = C.c_int32(0)
        if mask is None:
            self._chk(self.lib.ekfvio_remove_features(self.h, None, 0, C.byref(k)))
        else:
            m = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8).reshape(-1)
            self._chk(self.lib.ekfvio_remove_features(self.h, _u8(m), m.shape[0], C.byref(k)))
        return int(k.value)

    def landmark_ids(self):
        """Not in the reference, where a landmark's index is its identity: (ids int64[N], born float64[N]) of the landmarks, rows as points()'
        and get_state()'s of the same moment (ekfvio_get_landmark_ids).  An id is never reused during the handle's lifetime, ids rise strictly
        in landmark order, and born is the stamp of the frame a landmark entered in (NaN before any stamp)."""
        N = self.num_features
        ids, born = np.zeros(N, np.int64), np.zeros(N, np.float64)
        self._chk(self.lib.ekfvio_get_landmark_ids(self.h, ids.ctypes.data_as(C.POINTER(C.c_int64)), born.ctypes.data_as(C.POINTER(C.c_double))))
        return ids, born

    def setEndedExport(self, on):
        """Not in the reference: with it on, every removal (removeFeatures, addFrame with remove_lost=1) first writes one record per landmark
        about to leave -- id, born, its row, its camera-frame point and that point's covariance (ekfvio_set_ended_export); ended() reads them."""
        self._chk(self.lib.ekfvio_set_ended_export(self.h, int(on)))

    def ended(self):
        """ekfvio_get_ended: dict(id int64[k], born float64[k], index_before int32[k], xyz float32[k, 3], cov float32[k, 3, 3], count, total) of
        the most recent removal call since the export went on (count 0 with it off).  Each removal overwrites the last one's records."""
        cap = max(int(self.cfg.max_features), 1)
        ids, born, idx = np.zeros(cap, np.int64), np.zeros(cap, np.float64), np.zeros(cap, np.int32)
        xyz, cov = np.zeros((cap, 3), np.float32), np.zeros((cap, 3, 3), np.float32)
        k, total = C.c_int32(0), C.c_int64(0)
        self._chk(self.lib.ekfvio_get_ended(self.h, ids.ctypes.data_as(C.POINTER(C.c_int64)), born.ctypes.data_as(C.POINTER(C.c_double)),
                                            idx.ctypes.data_as(C.POINTER(C.c_int32)), _fp(xyz), _fp(cov), cap, C.byref(k), C.byref(total)))
        k = int(k.value)
        return dict(id=ids[:k].copy(), born=born[:k].copy(), index_before=idx[:k].copy(), xyz=xyz[:k].copy(), cov=cov[:k].copy(), count=k,
                    total=int(total.value))

    def setGate(self, chi2):
        """Not in the reference: the innovation gate (ekfvio_set_gate).  chi2 > 0: a landmark whose squared Mahalanobis distance on
        the propagated state exceeds it is treated as one the tracker failed; 0: off."""
        self._chk(self.lib.ekfvio_set_gate(self.h, float(chi2)))

    def gate(self):
        """ekfvio_get_gate: dict(d2[n], gated[n], n_landmarks, gated_last, gated_total) of the most recent update."""
        cap = max(int(self.cfg.max_features), 1)
        d2, g = np.zeros(cap, np.float32), np.zeros(cap, np.uint8)
        n, last, total = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._chk(self.lib.ekfvio_get_gate(self.h, _fp(d2), _u8(g), C.byref(n), C.byref(last), C.byref(total)))
        return dict(d2=d2[:n.value].copy(), gated=g[:n.value].copy(), n_landmarks=int(n.value), gated_last=int(last.value),
                    gated_total=int(total.value))

    def setKltFb(self, max_px):
        """Not in the reference: the tracker's forward-backward check (ekfvio_set_klt_fb).  max_px > 0: a landmark whose forward
        track, tracked back into the previous frame, ends more than max_px pixels from where it started is treated as one the
        tracker lost; 0: off."""
        self._chk(self.lib.ekfvio_set_klt_fb(self.h, float(max_px)))

    def klt_fb(self):
        """ekfvio_get_klt_fb: dict(err2[n], rejected[n], n_landmarks, rejected_last, rejected_total) of the most recent checked track."""
        cap = max(int(self.cfg.max_features), 1)
        e2, r = np.zeros(cap, np.float32), np.zeros(cap, np.uint8)
        n, last, total = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._chk(self.lib.ekfvio_get_klt_fb(self.h, _fp(e2), _u8(r), C.byref(n), C.byref(last), C.byref(total)))
        return dict(err2=e2[:n.value].copy(), rejected=r[:n.value].copy(), n_landmarks=int(n.value), rejected_last=int(last.value),
                    rejected_total=int(total.value))

    def setDistortion(self, D):
        """Not in the reference, which assumes a pinhole image (Frame.h:31): plumb_bob coefficients (k1, k2, p1, p2[, k3]) of the camera
        (ekfvio_set_distortion).  From the next pushed frame on, frames are rectified on the device between the upload and the pyramid;
        None, () or all zeros: off."""
        d = np.ascontiguousarray([] if D is None else D, dtype=np.float64).reshape(-1)
        self._chk(self.lib.ekfvio_set_distortion(self.h, d.ctypes.data_as(C.POINTER(C.c_double)) if d.size else None, int(d.size)))

    def setCameraModel(self, model, D=None, P=None):
        """Not in the reference: the camera's lens model and, optionally, the rectified camera (ekfvio_set_camera_model).  model:
        capi.CAMERA_PLUMB_BOB / CAMERA_RATIONAL / CAMERA_EQUIDISTANT or CameraInfo.distortion_model's name ("plumb_bob",
        "rational_polynomial", "equidistant", "fisheye"); D: 0, 4 or 5 / 8 / 4 coefficients; P: (fx', cx', fy', cy') of the rectified image
        or None for the raw camera's own K.  From the next pushed frame on frames are rectified through that model onto P, and everything
        behind the rectification takes P for the frame's intrinsics.  The last of setDistortion and setCameraModel wins."""
        m, d, p = _camera_model_args(model, D, P)
        self._chk(self.lib.ekfvio_set_camera_model(self.h, m, d.ctypes.data_as(C.POINTER(C.c_double)) if d.size else None, int(d.size),
                                                   None if p is None else _fp(p)))

    def cameraModel(self):
        """ekfvio_get_camera_model: dict(model, D[count], P (4 floats or None), on) as the handle holds the setting."""
        m, n, has, on = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        d, p = np.zeros(8, np.float64), np.zeros(4, np.float32)
        self._chk(self.lib.ekfvio_get_camera_model(self.h, C.byref(m), d.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n), _fp(p), C.byref(has),
                                                   C.byref(on)))
        return dict(model=int(m.value), D=d[:n.value].copy(), P=p if has.value else None, on=bool(on.value))

    def setMask(self, mask, rectify_border=False):
        """Not in the reference, which passes no mask to cv::FAST: the no-data mask (ekfvio_set_mask).  mask: uint8 [height, width] at the FULL
        frame size, nonzero = scene, or None; rectify_border: the black border that rectification leaves is no-data too.  From the next pushed
        frame on the detector takes no landmark, and the tracker passes none, within the kill-pad window of a no-data pixel; None and False:
        off.  While a mask is set, frames of another size are refused."""
        flags = capi.MASK_RECTIFY_BORDER if rectify_border else 0
        if mask is None:
            self._chk(self.lib.ekfvio_set_mask(self.h, None, 0, 0, 0, flags))
            return
        m = np.asarray(mask)
        if m.ndim != 2:
            raise capi.EkfvioError(capi.EINVAL, "the mask is a 2-D array")
        m = np.ascontiguousarray(m != 0 if m.dtype != np.uint8 else m, dtype=np.uint8)
        self._chk(self.lib.ekfvio_set_mask(self.h, _u8(m), m.shape[1], m.shape[0], m.shape[1], flags))

    def setEqualize(self, clip_limit, tiles_x=8, tiles_y=8):
        """Not in the reference, whose detector has a fixed contrast threshold and whose tracker assumes brightness constancy: clip-limited tile
        histogram equalisation of every pushed frame on the device, between the rectification and the pyramid (ekfvio_set_equalize).
        clip_limit > 0 with tiles in [1, 16]: on from the next pushed frame; clip_limit == 0: off."""
        self._chk(self.lib.ekfvio_set_equalize(self.h, float(clip_limit), int(tiles_x), int(tiles_y)))

    def setKltPhotometric(self, on):
        """Not in the reference, whose tracker assumes brightness constancy: the gain/offset term of the Lucas-Kanade passes
        (ekfvio_set_klt_photometric): span{1, I} is projected out of the template's gradients, once per pyramid level.  On from the next
        track, in the forward pass and in the forward-backward check's backward pass; off by default."""
        self._chk(self.lib.ekfvio_set_klt_photometric(self.h, int(on)))

    def setReplenishGrid(self, cells_x, cells_y):
        """New landmarks spread over the image (ekfvio_set_replenish_grid): from the next replenishment on the strongest free corner of every
        cell of a cells_x x cells_y grid, emptier cells first, instead of the raster first fit.  (0, 0): off; (1, 1): strongest corner first."""
        self._chk(self.lib.ekfvio_set_replenish_grid(self.h, int(cells_x), int(cells_y)))

    def replenishGrid(self):
        """ekfvio_get_replenish_grid: (cells_x, cells_y); (0, 0) = off."""
        cx, cy = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.ekfvio_get_replenish_grid(self.h, C.byref(cx), C.byref(cy)))
        return cx.value, cy.value

    def mask_blocked(self):
        """ekfvio_get_mask: the blocked map B as the device holds it, uint8 [H, W] of level 0 (1 = blocked); shape (0, 0) before the first
        frame pushed with the mask on."""
        w, h = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.ekfvio_get_mask(self.h, None, 0, C.byref(w), C.byref(h)))
        b = np.zeros((h.value, w.value), np.uint8)
        if b.size:
            self._chk(self.lib.ekfvio_get_mask(self.h, _u8(b), b.size, C.byref(w), C.byref(h)))
        return b

    def mask_hits(self):
        """ekfvio_get_mask_hits: dict(masked[n], n_landmarks, masked_last) of the most recent track of the landmarks with the mask on."""
        cap = max(int(self.cfg.max_features), 1)
        m = np.zeros(cap, np.uint8)
        n, last = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.ekfvio_get_mask_hits(self.h, _u8(m), C.byref(n), C.byref(last)))
        return dict(masked=m[:n.value].copy(), n_landmarks=int(n.value), masked_last=int(last.value))

    def setOutputCovariance(self, on):
        """Not in the reference (EKFVIO.cpp:473 "TODO add convariance computation"): with it on, every frame of ekfvio_step_image carries the
        covariances of its odometry and its point cloud with its other outputs (ekfvio_set_output_covariance), and odometry_covariance() /
        points_covariance() cost a memcpy behind a frame.  Such a frame's outputs never go out in front of the update's last GEMM."""
        self._chk(self.lib.ekfvio_set_output_covariance(self.h, int(on)))

    def odometry_covariance(self):
        """ekfvio_get_odometry_covariance: (pose 6x6 over (x, y, z, rotation about X, Y, Z) in the world frame, twist 6x6 over (linear, angular) in
        the body frame), float32, exactly symmetric."""
        c = np.empty((2, 6, 6), np.float32)
        self._chk(self.lib.ekfvio_get_odometry_covariance(self.h, _fp(c[0]), _fp(c[1])))
        return c[0], c[1]

    def points_covariance(self):
        """ekfvio_get_points_covariance: (N, 3, 3) float32, the covariance of the camera-frame point (u/rho, v/rho, 1/rho) of every landmark."""
        cov = np.empty((self.num_features, 3, 3), np.float32)
        self._chk(self.lib.ekfvio_get_points_covariance(self.h, _fp(cov)))
        return cov

    def checkSigma(self):
        a, b = C.c_float(0), C.c_float(0)
        self._chk(self.lib.ekfvio_check_sigma(self.h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    # ---- state access ------------------------------------------------------------------
    @property
    def num_features(self):
        return int(self.lib.ekfvio_num_features(self.h))

    @property
    def dim(self):
        return int(self.lib.ekfvio_dim(self.h))

    @property
    def base_mu(self):
        b = np.zeros(BASE_STATE_SIZE, np.float32)
        self._chk(self.lib.ekfvio_get_base_mu(self.h, _fp(b)))
        return b

    @property
    def Sigma(self):
        n = self.dim
        s = np.zeros((n, n), np.float32)
        self._chk(self.lib.ekfvio_get_sigma(self.h, _fp(s), n))
        return s.T.copy()

    def get_state(self):
        N = self.num_features
        feat = np.zeros((N, 3), np.float32)
        klt = np.zeros((N, 2), np.float32)
        dele = np.zeros(N, np.uint8)
        self._chk(self.lib.ekfvio_get_features(self.h, _fp(feat), _fp(klt), _u8(dele)))
        return dict(base_mu=self.base_mu, feat_mu=feat, last_klt=klt, del_flag=dele, Sigma=self.Sigma)

    def set_state(self, st):
        base = np.ascontiguousarray(st["base_mu"], dtype=np.float32)
        feat = np.ascontiguousarray(st["feat_mu"], dtype=np.float32).reshape(-1, 3)
        N = feat.shape[0]
        klt = np.ascontiguousarray(st["last_klt"], dtype=np.float32).reshape(N, 2)
        dele = np.ascontiguousarray(st["del_flag"], dtype=np.uint8).reshape(N)
        sig = np.ascontiguousarray(np.asarray(st["Sigma"], dtype=np.float32).T)
        n = BASE_STATE_SIZE + 3 * N
        self._chk(self.lib.ekfvio_set_state(self.h, N, _fp(base), _fp(feat), _fp(klt), _u8(dele), _fp(sig), n))

    # ---- device-resident sequences -----------------------------------------------------
    def upload_measurements(self, z, R, passed):
        z = np.ascontiguousarray(z, dtype=np.float32)
        R = np.ascontiguousarray(R, dtype=np.float32)
        p = np.ascontiguousarray(passed, dtype=np.uint8)
        frames = p.shape[0]
        self._chk(self.lib.ekfvio_upload_measurements(self.h, frames, _fp(z), _fp(R), _u8(p)))

    def run_uploaded(self, first, count, dt):
        self._chk(self.lib.ekfvio_run_uploaded(self.h, first, count, float(dt)))

    def synchronize(self):
        """Waits for the handle's stream; returns capi.ENUMERIC once if an asynchronous run met a non-positive pivot."""
        return self._chk(self.lib.ekfvio_synchronize(self.h), allow=(capi.ENUMERIC,))

    # ---- instrumentation ---------------------------------------------------------------
    def profile(self, on):
        self._chk(self.lib.ekfvio_profile_enable(self.h, int(on)))
        if on:
            self._chk(self.lib.ekfvio_profile_reset(self.h))

    def profile_report(self):
        out = {}
        for c in range(self.lib.ekfvio_profile_count()):
            ms, n, fl = C.c_double(0), C.c_int64(0), C.c_double(0)
            self._chk(self.lib.ekfvio_profile_get(self.h, c, C.byref(ms), C.byref(n), C.byref(fl)))
            out[self.lib.ekfvio_profile_name(c).decode()] = dict(ms=ms.value, launches=n.value, flops=fl.value)
        return out

    def profile_update_gemms(self, reps=50):
        """(mean launch duration in us, flops per launch) of the two P-update GEMMs at the shape of the
        most recent update, replayed back to back from a hipGraph between two HIP events."""
        us, fl = C.c_double(0), C.c_double(0)
        self._chk(self.lib.ekfvio_profile_update_gemms(self.h, int(reps), C.byref(us), C.byref(fl)))
        return us.value, fl.value

    # ---- raw kernels -------------------------------------------------------------------
    def test_gemm(self, A, B, C0, alpha=1.0, beta=0.0, transB=True, variant=0):
        """C = beta*C0 + alpha * A @ (B.T if transB else B); arrays are numpy [row, col].  (hooks build)"""
        self._need_hooks()
        A = np.asarray(A, np.float32)
        B = np.asarray(B, np.float32)
        M, K = A.shape
        N = B.shape[0] if transB else B.shape[1]
        Ac, Bc = np.array(A.T, order="C", copy=True), np.array(B.T, order="C", copy=True)  # column-major buffers
        Cc = np.array(np.asarray(C0, np.float32).T, order="C", copy=True)  # never alias the caller's C0
        self._chk(self.lib.ekfvio_test_gemm(self.h, int(transB), M, N, K, alpha, _fp(Ac), M, _fp(Bc), B.shape[0], beta,
                                            _fp(Cc), M, int(variant)))
        return Cc.T.copy()

    def counters(self):
        """ekfvio_get_counters: dict(persistent, schur, recoveries, mode, early_output_frames, t2_updates, graph_steps, prelinearized_steps)."""
        c = (C.c_int64 * 8)()
        self._chk(self.lib.ekfvio_get_counters(self.h, c))
        return dict(persistent=int(c[0]), schur=int(c[1]), recoveries=int(c[2]), mode=int(c[3]), early_output_frames=int(c[4]), t2_updates=int(c[5]),
                    graph_steps=int(c[6]), prelinearized_steps=int(c[7]))

    def _need_hooks(self):
        if not self.hooks:
            raise RuntimeError("this entry point exists only in the hooks build: construct the filter with hooks=True")

    def persistent_sweeps(self):
        """Diagnostic: sweeps of this handle that went out as the single persistent launch so far."""
        return self.counters()["persistent"]

    def sweep_counts(self):
        """Diagnostic: dict(persistent, schur, recoveries, mode) of this handle's Cholesky sweeps."""
        c = self.counters()
        return {k: c[k] for k in ("persistent", "schur", "recoveries", "mode")}

    def sweep_fault(self, spin_limit=0, stall_workgroup=-1):
        """Fault injection for the persistent sweep (ekfvio_test_sweep_fault; hooks build)."""
        self._need_hooks()
        self._chk(self.lib.ekfvio_test_sweep_fault(self.h, int(spin_limit), int(stall_workgroup)))

    def sweep_delay(self, workgroup=-1, point=0, ticks=0):
        """Owner `workgroup` of the persistent sweep (numbered like sweep_fault's stall_workgroup; -1: none) stores its finished tile (point 0)
        or its panel block (point 1) `ticks` of the 100 MHz clock late (ekfvio_test_sweep_delay; hooks build)."""
        self._need_hooks()
        self._chk(self.lib.ekfvio_test_sweep_delay(self.h, int(workgroup), int(point), int(ticks)))

    def fill_update_scratch(self, word):
        """The 32-bit pattern `word` into every element of the float work buffers of process(dt) and the update
        (ekfvio_test_fill_update_scratch; hooks build).  The state, the inputs, the sweep's flags and the integer buffers stay."""
        self._need_hooks()
        self._chk(self.lib.ekfvio_test_fill_update_scratch(self.h, int(word) & 0xFFFFFFFF))

    def test_cholesky_solve(self, S, Crhs):
        """Returns (L, X = Crhs @ inv(S), info).  (hooks build)"""
        self._need_hooks()
        S = np.asarray(S, np.float32)
        Crhs = np.asarray(Crhs, np.float32)
        m, nr = S.shape[0], Crhs.shape[0]
        Sc, Cc = np.array(S.T, order="C", copy=True), np.array(Crhs.T, order="C", copy=True)
        L = np.zeros((m, m), np.float32)
        X = np.zeros((m, nr), np.float32)
        info = C.c_int32(0)
        self._chk(self.lib.ekfvio_test_cholesky_solve(self.h, m, nr, _fp(Sc), _fp(Cc), _fp(L), _fp(X), C.byref(info)))
        return L.T.copy(), X.T.copy(), info.value


class KLTTracker:
    """Host mirror of the reference's `class KLTTracker` (include/ekf_vio/KLTTracker.h:88-90).
    The two most recent frames live on the device inside the filter handle (the reference
    keeps them in EKFVIO::frame_buffer, depth 2)."""

    def __init__(self, ekf):
        self.ekf = ekf
        self.lib = ekf.lib

    def push_frame(self, img, K):
        """Frame(img, K, ...) -> device pyramid; the previous current frame becomes `lf`."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape
        K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        self.ekf._chk(self.lib.ekfvio_klt_push_frame(self.ekf.h, _u8(img), w, h, w, _fp(K)))

    def findNewFeaturePositions(self):
        """(measured_positions[N,2], estimated_uncertainty[N,4], passed[N]) for the filter's
        landmarks, tracked from the previous into the current frame (KLTTracker.cpp:29-95)."""
        N = self.ekf.num_features
        z = np.zeros((N, 2), np.float32)
        R = np.zeros((N, 4), np.float32)
        p = np.zeros(N, np.uint8)
        self.ekf._chk(self.lib.ekfvio_klt_track(self.ekf.h, _fp(z), _fp(R), _u8(p)))
        return z, R, p

    def track_points(self, prev_px, init_px):
        """calcOpticalFlowPyrLK(prev, cur, prev_px, init_px, OPTFLOW_USE_INITIAL_FLOW) in pixels."""
        pp = np.ascontiguousarray(prev_px, dtype=np.float32).reshape(-1, 2)
        ii = np.ascontiguousarray(init_px, dtype=np.float32).reshape(-1, 2)
        out = np.zeros_like(pp)
        st = np.zeros(pp.shape[0], np.uint8)
        self.ekf._chk(self.lib.ekfvio_klt_track_points(self.ekf.h, _fp(pp), _fp(ii), pp.shape[0], _fp(out), _u8(st)))
        return out, st

    def track_points_fb(self, prev_px, init_px):
        """track_points with the forward-backward check (ekfvio_klt_track_points_fb): (out_px, status, back_px, err2, fb_ok).  The
        backward pass runs whatever the handle's threshold; with a threshold of 0, fb_ok is the backward status alone."""
        pp = np.ascontiguousarray(prev_px, dtype=np.float32).reshape(-1, 2)
        ii = np.ascontiguousarray(init_px, dtype=np.float32).reshape(-1, 2)
        out, back = np.zeros_like(pp), np.zeros_like(pp)
        st, ok = np.zeros(pp.shape[0], np.uint8), np.zeros(pp.shape[0], np.uint8)
        e2 = np.zeros(pp.shape[0], np.float32)
        self.ekf._chk(self.lib.ekfvio_klt_track_points_fb(self.ekf.h, _fp(pp), _fp(ii), pp.shape[0], _fp(out), _u8(st), _fp(back), _fp(e2),
                                                          _u8(ok)))
        return out, st, back, e2, ok

    def uncertainty_points(self, ref_px, cur_px):
        """KLTTracker::estimateUncertaintySampleBased (KLTTracker.cpp:111-175) for arbitrary points between the two
        resident frames: cov[n, 2, 2] in px^2."""
        rp = np.ascontiguousarray(ref_px, dtype=np.float32).reshape(-1, 2)
        cp = np.ascontiguousarray(cur_px, dtype=np.float32).reshape(-1, 2)
        cov = np.zeros((rp.shape[0], 4), np.float32)
        self.ekf._chk(self.lib.ekfvio_klt_uncertainty_points(self.ekf.h, _fp(rp), _fp(cp), rp.shape[0], _fp(cov)))
        return cov.reshape(-1, 2, 2)

    def level(self, l):
        w, h = C.c_int32(0), C.c_int32(0)
        self.ekf._chk(self.lib.ekfvio_klt_get_level(self.ekf.h, l, C.byref(w), C.byref(h), None, None))
        img = np.zeros((h.value, w.value), np.uint8)
        der = np.zeros((h.value, w.value, 2), np.int16)
        self.ekf._chk(self.lib.ekfvio_klt_get_level(self.ekf.h, l, C.byref(w), C.byref(h), _u8(img),
                                                    der.ctypes.data_as(C.POINTER(C.c_int16))))
        return img, der

    def padded_level(self, l):
        """Test hook: level l with its border, as the tracker reads it."""
        w, h, b = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self.ekf._chk(self.lib.ekfvio_klt_get_level(self.ekf.h, l, C.byref(w), C.byref(h), None, None))
        self.ekf._chk(self.lib.ekfvio_test_klt_padded_level(self.ekf.h, l, C.byref(b), None, None))
        img = np.zeros((h.value + 2 * b.value, w.value + 2 * b.value), np.uint8)
        der = np.zeros((h.value + 2 * b.value, w.value + 2 * b.value, 2), np.int16)
        self.ekf._chk(self.lib.ekfvio_test_klt_padded_level(self.ekf.h, l, C.byref(b), _u8(img), der.ctypes.data_as(C.POINTER(C.c_int16))))
        return img, der, b.value


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def rotation_error_jacobian(q_wxyz):
    """ekfvio_rotation_error_jacobian: the 3x4 J with dtheta = J dq for q_true = [1, dtheta/2] (x) q (include/ekfvio.h).  A host function: no GPU involved."""
    lib = capi.load()
    q = np.ascontiguousarray(q_wxyz, dtype=np.float32).reshape(4)
    J = np.zeros((3, 4), np.float32)
    rc = lib.ekfvio_rotation_error_jacobian(_fp(q), _fp(J))
    if rc != capi.OK:
        raise capi.EkfvioError(rc, "ekfvio_rotation_error_jacobian")
    return J


def rectify_map(K, D, width, height):
    """ekfvio_rectify_map: the fixed-point map (sx, sy), int32 [height, width] each, that a handle with the coefficients D (k1, k2, p1, p2[, k3])
    rectifies a width x height frame with intrinsics K through; INT32_MIN where no source pixel exists.  A host function: no GPU involved."""
    lib = capi.load()
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    d = np.ascontiguousarray([] if D is None else D, dtype=np.float64).reshape(-1)
    sx, sy = np.zeros((int(height), int(width)), np.int32), np.zeros((int(height), int(width)), np.int32)
    rc = lib.ekfvio_rectify_map(_fp(K), d.ctypes.data_as(C.POINTER(C.c_double)) if d.size else None, int(d.size), int(width), int(height), _ip(sx), _ip(sy))
    if rc != capi.OK:
        raise capi.EkfvioError(rc, "ekfvio_rectify_map")
    return sx, sy


def _camera_model_args(model, D, P):
    """(model as int32, D as float64 [count], P as float32 [4] or None) of the camera-model entry points; a model's name is looked up."""
    if isinstance(model, str):
        if model not in capi.CAMERA_MODELS:
            raise capi.EkfvioError(capi.EINVAL, "unknown camera model %r" % model)
        model = capi.CAMERA_MODELS[model]
    d = np.ascontiguousarray([] if D is None else D, dtype=np.float64).reshape(-1)
    p = None if P is None else np.ascontiguousarray(P, dtype=np.float32).reshape(-1)
    if p is not None and p.size != 4:
        raise capi.EkfvioError(capi.EINVAL, "P is (fx', cx', fy', cy')")
    return int(model), d, p


def rectify_map_model(K, model, D, P, width, height):
    """ekfvio_rectify_map_model: rectify_map for any camera model (TightlyCoupledEKF.setCameraModel's model, D, P).  A host function: no GPU
    involved."""
    lib = capi.load()
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    m, d, p = _camera_model_args(model, D, P)
    sx, sy = np.zeros((int(height), int(width)), np.int32), np.zeros((int(height), int(width)), np.int32)
    rc = lib.ekfvio_rectify_map_model(_fp(K), m, d.ctypes.data_as(C.POINTER(C.c_double)) if d.size else None, int(d.size),
                                      None if p is None else _fp(p), int(width), int(height), _ip(sx), _ip(sy))
    if rc != capi.OK:
        raise capi.EkfvioError(rc, "ekfvio_rectify_map_model")
    return sx, sy


def mask_blocked_model(K, model, D, P, mask, width, height, inverse_image_scale, kill_pad, flags):
    """ekfvio_mask_blocked_model: mask_blocked for any camera model (model, D, P as rectify_map_model takes them).  A host function: no GPU
    involved."""
    lib = capi.load()
    Kp = None if K is None else _fp(np.ascontiguousarray(K, dtype=np.float32).reshape(9))
    m, d, p = _camera_model_args(model, D, P)
    mp, stride = None, 0
    if mask is not None:
        mk = np.asarray(mask)
        if mk.dtype != np.uint8 or mk.ndim != 2 or mk.strides[1] != 1 or mk.shape != (int(height), int(width)):
            mk = np.ascontiguousarray(mk, dtype=np.uint8).reshape(int(height), int(width))
        mp, stride = C.cast(mk.ctypes.data, C.POINTER(C.c_uint8)), int(mk.strides[0])
    s = max(int(inverse_image_scale), 1)
    out = np.zeros((max(int(height) // s, 0), max(int(width) // s, 0)), np.uint8)
    rc = lib.ekfvio_mask_blocked_model(Kp, m, d.ctypes.data_as(C.POINTER(C.c_double)) if d.size else None, int(d.size),
                                       None if p is None else _fp(p), mp, int(width), int(height), stride, int(inverse_image_scale), int(kill_pad),
                                       int(flags), _u8(out) if out.size else None)
    if rc != capi.OK:
        raise capi.EkfvioError(rc, "ekfvio_mask_blocked_model")
    return out


def mask_blocked(K, D, mask, width, height, inverse_image_scale, kill_pad, flags):
    """ekfvio_mask_blocked: the blocked map B (include/ekfvio.h, ekfvio_set_mask), uint8 [height // s, width // s], that a handle with these
    settings holds for width x height frames: K, D as rectify_map takes them, mask uint8 [height, width] or None (any row stride of the array is
    passed on), flags = capi.MASK_RECTIFY_BORDER or 0.  A host function: no GPU involved."""
    lib = capi.load()
    Kp = None if K is None else _fp(np.ascontiguousarray(K, dtype=np.float32).reshape(9))
    d = np.ascontiguousarray([] if D is None else D, dtype=np.float64).reshape(-1)
    mp, stride = None, 0
    if mask is not None:
        m = np.asarray(mask)
        if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1 or m.shape != (int(height), int(width)):
            m = np.ascontiguousarray(m, dtype=np.uint8).reshape(int(height), int(width))
        mp, stride = C.cast(m.ctypes.data, C.POINTER(C.c_uint8)), int(m.strides[0])
    s = max(int(inverse_image_scale), 1)
    out = np.zeros((max(int(height) // s, 0), max(int(width) // s, 0)), np.uint8)
    rc = lib.ekfvio_mask_blocked(Kp, d.ctypes.data_as(C.POINTER(C.c_double)) if d.size else None, int(d.size), mp, int(width), int(height), stride,
                                 int(inverse_image_scale), int(kill_pad), int(flags), _u8(out) if out.size else None)
    if rc != capi.OK:
        raise capi.EkfvioError(rc, "ekfvio_mask_blocked")
    return out


def equalize(image, clip_limit, tiles_x=8, tiles_y=8):
    """ekfvio_equalize: the frame a handle with ekfvio_set_equalize(clip_limit, tiles_x, tiles_y) makes of `image` (uint8 [height, width]; any row
    stride of the array is passed on) before its pyramid, uint8 [height, width].  A host function: no GPU involved."""
    lib = capi.load()
    m = np.asarray(image)
    if m.ndim != 2:
        raise capi.EkfvioError(capi.EINVAL, "the image is a 2-D array")
    if m.dtype != np.uint8 or m.strides[1] != 1 or m.strides[0] < m.shape[1]:
        m = np.ascontiguousarray(m, dtype=np.uint8)
    out = np.zeros(m.shape, np.uint8)
    rc = lib.ekfvio_equalize(C.cast(m.ctypes.data, C.POINTER(C.c_uint8)) if m.size else None, int(m.shape[1]), int(m.shape[0]), int(m.strides[0]),
                             float(clip_limit), int(tiles_x), int(tiles_y), _u8(out) if out.size else None)
    if rc != capi.OK:
        raise capi.EkfvioError(rc, "ekfvio_equalize")
    return out


def klt_project_gradients(Iv, Ix, Iy):
    """ekfvio_klt_project_gradients: (Ix', Iy') of one window's pixels, int32 arrays of Iv's shape, with span{1, Iv} projected out of the two
    gradient images as the tracker does with ekfvio_set_klt_photometric on.  A host function: no GPU involved."""
    lib = capi.load()
    iv, ix, iy = (np.ascontiguousarray(a, dtype=np.int32) for a in (Iv, Ix, Iy))
    if not (iv.shape == ix.shape == iy.shape):
        raise capi.EkfvioError(capi.EINVAL, "Iv, Ix, Iy have one shape")
    ox, oy = np.zeros(iv.shape, np.int32), np.zeros(iv.shape, np.int32)
    rc = lib.ekfvio_klt_project_gradients(_ip(iv) if iv.size else None, _ip(ix) if iv.size else None, _ip(iy) if iv.size else None, int(iv.size),
                                          _ip(ox) if iv.size else None, _ip(oy) if iv.size else None)
    if rc != capi.OK:
        raise capi.EkfvioError(rc, "ekfvio_klt_project_gradients")
    return ox, oy


def replenish_select(kp_xy, score, existing_px_xy, blocked, width, height, radius, kill_pad, cells_x, cells_y, wanted):
    """ekfvio_replenish_select: the pixels (int32 [k, 2], in the order taken) the replenishment's selection takes among the keypoints kp_xy
    (int [n, 2], raster order) with scores `score`, given the rounded pixels of the landmarks in the state and the blocked map (uint8 [h, w]
    or None).  cells_x = cells_y = 0: the raster first fit.  A host function: no GPU involved."""
    lib = capi.load()
    xy = np.ascontiguousarray(kp_xy, dtype=np.int32).reshape(-1, 2)
    sc = np.ascontiguousarray(score, dtype=np.int32).reshape(-1)
    ex = np.ascontiguousarray(existing_px_xy, dtype=np.int32).reshape(-1, 2)
    if xy.shape[0] != sc.shape[0]:
        raise capi.EkfvioError(capi.EINVAL, "one score per keypoint")
    b = None
    if blocked is not None:
        b = np.ascontiguousarray(blocked, dtype=np.uint8)
        if b.shape != (int(height), int(width)):
            raise capi.EkfvioError(capi.EINVAL, "blocked is [height, width]")
    out, k = np.zeros((max(int(wanted), 1), 2), np.int32), C.c_int32(0)
    rc = lib.ekfvio_replenish_select(_ip(xy) if xy.size else None, _ip(sc) if sc.size else None, int(xy.shape[0]), _ip(ex) if ex.size else None,
                                     int(ex.shape[0]), _u8(b) if b is not None else None, int(width), int(height), int(radius), int(kill_pad),
                                     int(cells_x), int(cells_y), int(wanted), _ip(out), C.byref(k))
    if rc != capi.OK:
        raise capi.EkfvioError(rc, "ekfvio_replenish_select")
    return out[:k.value].copy()


class EKFVIO:
    """Host mirror of the step sequence of EKFVIO::addFrame / updateStateWithNewImage
    (include/ekf_vio/EKFVIO.cpp:139-219) without ROS: frames in, odometry + landmark cloud out.
    With replenish=1 in the configuration addFrame also runs replenishFeatures (FAST, EKFVIO.cpp:224-311)
    on the device; otherwise call replenishFeatures() (or addNewFeatures) yourself."""

    def __init__(self, **kw):
        # (distortion=(k1, k2, p1, p2[, k3]): raw frames are rectified on the device, setDistortion below; camera_model=(model, D[, P]): the
        # same for a rational or an equidistant lens and onto a rectified camera P, setCameraModel below; output_covariance=True: every frame's
        # outputs carry their covariances, setOutputCovariance below; mask=uint8 [h, w] and / or mask_rectify_border=True: the no-data mask, setMask below;
        # equalize=(clip_limit, tiles_x, tiles_y): every frame is equalised on the device before its pyramid, setEqualize below;
        # klt_photometric=True: the tracker's gain/offset term, setKltPhotometric below; ended_export=True: every removal hands out the records of
        # the landmarks that leave, setEndedExport below; zupt=(max_flow_px, min_tracks, min_ratio, vel_var, omega_var): the zero-velocity update,
        # setZupt below; imu_extrinsics=(R_ci, p_ci): the IMU in its own frame, setImuExtrinsics below; replenish_grid=(cells_x, cells_y): new
        # landmarks spread over a grid of cells, setReplenishGrid below; frame_aid=(H, z, R[, chi2]): a standing aiding measurement of the base
        # state in every frame, setFrameAid below; gravity_align_samples=K: the first K IMU
        # records that come up for application are not applied but averaged, and their mean accelerometer reading sets the gravity vector:
        # the rig is taken to be AT REST through them, with an accelerometer bias negligible against 9.81; frames meanwhile are processed as
        # without an IMU)
        self.gravity_align_samples = int(kw.pop("gravity_align_samples", 0))
        if self.gravity_align_samples < 0:
            raise capi.EkfvioError(capi.EINVAL, "gravity_align_samples < 0")
        self.tc_ekf = TightlyCoupledEKF(**kw)
        self.tracker = KLTTracker(self.tc_ekf)
        self._imu_queue = []      # (stamp, gyro, accel), kept in stamp order; only used with use_imu = 1
        self._t_filter = None     # the stamp the device state stands at
        self._last_K = None
        self.dropped_imu = 0
        self._align_left = self.gravity_align_samples  # records still to be averaged
        self._align_sum = np.zeros(3, np.float64)

    def reset(self):
        """initializeBaseState, an empty IMU queue, and the gravity alignment starts over (the extrinsics and the gravity set so far stay)."""
        self.tc_ekf.initializeBaseState()
        self._imu_queue = []
        self._t_filter = None  # (ekfvio_reset forgets the filter's clock)
        self._align_left = self.gravity_align_samples
        self._align_sum = np.zeros(3, np.float64)

    def setImuExtrinsics(self, R_ci=None, p_ci=None):
        """TightlyCoupledEKF.setImuExtrinsics: from the next IMU record on the update models the IMU in its own frame."""
        self.tc_ekf.setImuExtrinsics(R_ci, p_ci)

    def setGravity(self, g):
        """TightlyCoupledEKF.setGravity: the gravity vector in the world frame from the next IMU record on."""
        self.tc_ekf.setGravity(g)

    def _apply_imu(self, stamp, g, a):
        """One record, in stamp order: averaged while the gravity alignment runs, else ekfvio_imu."""
        e = self.tc_ekf
        if self._align_left > 0 and e.cfg.use_imu:
            self._align_sum += a.astype(np.float64)
            self._align_left -= 1
            if self._t_filter is None:  # the first message of all only sets the filter's clock (ekfvio_imu), as without the alignment
                e._chk(e.lib.ekfvio_imu(e.h, stamp, _fp(g), _fp(a)))
                self._t_filter = stamp
            if self._align_left == 0:
                mean = np.ascontiguousarray(self._align_sum / self.gravity_align_samples)
                R, _, on = e.imuExtrinsics()
                gvec = np.zeros(3, np.float32)
                mag = float(np.linalg.norm(np.array(list(e.cfg.gravity), np.float32).astype(np.float64)))
                e._chk(e.lib.ekfvio_gravity_from_accel(_fp(np.ascontiguousarray(R.reshape(9))) if on else None,
                                                       mean.ctypes.data_as(C.POINTER(C.c_double)), mag, _fp(gvec)))
                e.setGravity(gvec)
            return
        e._chk(e.lib.ekfvio_imu(e.h, stamp, _fp(g), _fp(a)))
        self._t_filter = stamp

    def addFrame(self, stamp, img, K):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape
        K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
        self._drain_imu(float(stamp))  # IMU records up to this frame's stamp, in stamp order, before the frame itself
        rc = self.tc_ekf.lib.ekfvio_step_image(self.tc_ekf.h, float(stamp), _u8(img), w, h, w, _fp(K))
        # ekfvio_step_image moves the device clock as soon as process(dt) is enqueued; only EINVAL / ECAPACITY refuse the frame
        # before that.  The host's queue clock follows whenever the predict went out, whatever happened behind it, so that a
        # failed frame does not leave IMU records between the two stamps queued for a filter that is already past them.
        if rc not in (capi.EINVAL, capi.ECAPACITY):
            self._t_filter = float(stamp) if self._t_filter is None else max(self._t_filter, float(stamp))
            self._last_K = K.copy()
        return self.tc_ekf._chk(rc, allow=(capi.ENUMERIC,))

    def setDistortion(self, D):
        """The camera's plumb_bob coefficients (TightlyCoupledEKF.setDistortion): from the next frame on addFrame takes raw frames."""
        self.tc_ekf.setDistortion(D)

    def setCameraModel(self, model, D=None, P=None):
        """The camera's lens model and the rectified camera (TightlyCoupledEKF.setCameraModel): from the next frame on addFrame takes raw
        frames of that lens; K stays the raw camera's, and with P the outputs are the rectified camera's."""
        self.tc_ekf.setCameraModel(model, D, P)

    def setMask(self, mask, rectify_border=False):
        """TightlyCoupledEKF.setMask: from the next frame on no landmark is taken or passed within the kill-pad window of a no-data pixel."""
        self.tc_ekf.setMask(mask, rectify_border=rectify_border)

    def setEqualize(self, clip_limit, tiles_x=8, tiles_y=8):
        """TightlyCoupledEKF.setEqualize: from the next frame on the detector and the tracker see the equalised frame (clip_limit 0: off)."""
        self.tc_ekf.setEqualize(clip_limit, tiles_x, tiles_y)

    def setKltPhotometric(self, on):
        """TightlyCoupledEKF.setKltPhotometric: from the next frame on the tracker matches up to a gain and an offset."""
        self.tc_ekf.setKltPhotometric(on)

    def setReplenishGrid(self, cells_x, cells_y):
        """TightlyCoupledEKF.setReplenishGrid: from the next replenishment on new landmarks are spread over a grid of cells ((0, 0): off)."""
        self.tc_ekf.setReplenishGrid(cells_x, cells_y)

    def landmark_ids(self):
        """TightlyCoupledEKF.landmark_ids: (ids int64[N], born float64[N]), rows as points()'; a memcpy behind a frame."""
        return self.tc_ekf.landmark_ids()

    def setEndedExport(self, on):
        """TightlyCoupledEKF.setEndedExport: from the next frame on every removal hands out the records of the landmarks that leave."""
        self.tc_ekf.setEndedExport(on)

    def ended(self):
        """TightlyCoupledEKF.ended: the records of the most recent removal; a consumer that wants every ended track reads it after every frame."""
        return self.tc_ekf.ended()

    def setZupt(self, max_flow_px, min_tracks=8, min_ratio=0.75, vel_variance=1e-4, omega_variance=1e-4):
        """TightlyCoupledEKF.setZupt: from the next frame on a frame whose tracks stand still updates velocity and body rate with z = 0."""
        self.tc_ekf.setZupt(max_flow_px, min_tracks, min_ratio, vel_variance, omega_variance)

    def zuptUpdate(self, vel_variance=1e-4, omega_variance=1e-4):
        """TightlyCoupledEKF.zuptUpdate: the update alone, for a caller with its own stop detector."""
        self.tc_ekf.zuptUpdate(vel_variance, omega_variance)

    def zupt(self):
        """TightlyCoupledEKF.zupt: the most recent frame's decision; a memcpy behind a frame."""
        return self.tc_ekf.zupt()

    def aidUpdate(self, H, z, R, chi2=0.0):
        """TightlyCoupledEKF.aidUpdate: a linear aiding measurement of the base state on the state as it stands."""
        self.tc_ekf.aidUpdate(H, z, R, chi2)

    def aid(self, stamp, H, z, R, chi2=0.0):
        """TightlyCoupledEKF.aid in arrival order: the queued IMU records up to `stamp` first, then process(dt) to the stamp and the update.
        A stamp older than the filter's time is not applied (out-of-order records are not supported) and False is returned."""
        stamp = float(stamp)
        self._drain_imu(stamp)
        if self._t_filter is not None and stamp < self._t_filter:
            return False
        self.tc_ekf.aid(stamp, H, z, R, chi2)
        self._t_filter = stamp
        return True

    def setFrameAid(self, H=None, z=None, R=None, chi2=0.0):
        """TightlyCoupledEKF.setFrameAid: from the next frame on every frame applies the standing measurement; H None: off."""
        self.tc_ekf.setFrameAid(H, z, R, chi2)

    def aid_status(self):
        """TightlyCoupledEKF.aid_status: the most recent aiding update's d2, verdict and counts."""
        return self.tc_ekf.aid_status()

    def setOutputCovariance(self, on):
        """TightlyCoupledEKF.setOutputCovariance: from the next frame on addFrame delivers the covariances with the frame's outputs."""
        self.tc_ekf.setOutputCovariance(on)

    def odometry_covariance(self):
        """The covariances nav_msgs/Odometry asks for: (pose 6x6 in the world frame, twist 6x6 in the body frame); a memcpy behind a frame with
        output_covariance on, a launch and a wait otherwise."""
        return self.tc_ekf.odometry_covariance()

    def points_covariance(self):
        """(N, 3, 3): the covariance of every point of points()."""
        return self.tc_ekf.points_covariance()

    def replenishFeatures(self):
        """EKFVIO::replenishFeatures (EKFVIO.cpp:224-311) on the current frame, on the device: FAST-9/16 with
        non-maximum suppression, occupancy circles, first fit (or, with setReplenishGrid, the grid's rounds), addNewFeatures.  Returns the new
        landmarks' pixels."""
        k = C.c_int32(0)
        px = np.zeros((max(self.tc_ekf.cfg.max_features, 1), 2), np.int32)
        self.tc_ekf._chk(self.tc_ekf.lib.ekfvio_replenish(self.tc_ekf.h, C.byref(k), _ip(px)))
        return px[:k.value].copy()

    def fast(self, threshold=50, nonmax=True):
        """cv::FAST on the current (resized) frame: (xy[n,2], score[n]) in raster order."""
        w, h = C.c_int32(0), C.c_int32(0)
        self.tc_ekf._chk(self.tc_ekf.lib.ekfvio_klt_get_level(self.tc_ekf.h, 0, C.byref(w), C.byref(h), None, None))
        cap = w.value * h.value
        xy, sc, n = np.zeros((cap, 2), np.int32), np.zeros(cap, np.int32), C.c_int32(0)
        self.tc_ekf._chk(self.tc_ekf.lib.ekfvio_fast_detect(self.tc_ekf.h, int(threshold), int(bool(nonmax)), cap, _ip(xy), _ip(sc),
                                                            C.byref(n)))
        k = min(n.value, cap)
        return xy[:k].copy(), sc[:k].copy()

    def imu_callback(self, stamp, gyro, accel):
        """EKFVIO::imu_callback (EKFVIO.cpp:113-115): a logging stub in the reference, and a no-op here unless the filter was
        created with use_imu=1.  Then the record is queued and applied (propagate to its stamp, IMU measurement update) in
        stamp order in front of the next frame whose stamp is not older: IMU messages stamped after an image reach a node
        before that image does.  A record older than the filter's time is dropped and counted (`dropped_imu`)."""
        g = np.ascontiguousarray(gyro, dtype=np.float32)
        a = np.ascontiguousarray(accel, dtype=np.float32)
        if not self.tc_ekf.cfg.use_imu:
            self.tc_ekf._chk(self.tc_ekf.lib.ekfvio_imu(self.tc_ekf.h, float(stamp), _fp(g), _fp(a)))
            return
        stamp = float(stamp)
        if self._t_filter is not None and stamp < self._t_filter:
            self.dropped_imu += 1
            return
        i = len(self._imu_queue)
        while i > 0 and self._imu_queue[i - 1][0] > stamp:
            i -= 1
        self._imu_queue.insert(i, (stamp, g, a))
        if len(self._imu_queue) > 1000:  # the reference's subscriber queue (EKFVIO.cpp:80)
            self._imu_queue.pop(0)
            self.dropped_imu += 1

    def imu_now(self, stamp, gyro, accel):
        """ekfvio_imu directly, for a caller that delivers records in stamp order itself (EKFVIO_EINVAL for an older one)."""
        g = np.ascontiguousarray(gyro, dtype=np.float32)
        a = np.ascontiguousarray(accel, dtype=np.float32)
        self._apply_imu(float(stamp), g, a)

    def _drain_imu(self, until):
        while self._imu_queue and self._imu_queue[0][0] <= until:
            stamp, g, a = self._imu_queue.pop(0)
            if self._t_filter is not None and stamp < self._t_filter:
                self.dropped_imu += 1
                continue
            self._apply_imu(stamp, g, a)

    def insight(self):
        """publishInsight's image (EKFVIO.cpp:379-442): the resized frame as BGR8 [h, w, 3] with a green 22-pixel square
        (cv::drawMarker MARKER_SQUARE) at the pixel of every landmark that is not flagged for deletion."""
        if self._last_K is None:
            raise capi.EkfvioError(capi.ESTATE, "insight() before the first frame")
        grey, _ = self.tracker.level(0)
        h, w = grey.shape
        out = np.repeat(grey[:, :, None], 3, axis=2).copy()
        s = max(int(self.tc_ekf.cfg.inverse_image_scale), 1)
        P = self.tc_ekf.cameraModel()["P"]  # (fx', cx', fy', cy') where set: level 0 is then the rectified camera's image
        fx = np.float32(np.float64(self._last_K[0] if P is None else P[0]) / s)
        fy = np.float32(np.float64(self._last_K[4] if P is None else P[2]) / s)
        st = self.tc_ekf.get_state()
        for (u, v, _), flag in zip(st["feat_mu"], st["del_flag"]):
            if flag:
                continue
            px, py = int(np.rint(np.float32(u) * fx)), int(np.rint(np.float32(v) * fy))
            for d in range(-11, 12):
                for x, y in ((px + d, py - 11), (px + d, py + 11), (px - 11, py + d), (px + 11, py + d)):
                    if 0 <= x < w and 0 <= y < h:
                        out[y, x] = (0, 255, 0)
        return out

    def odometry(self):
        """What publishOdometry sends (EKFVIO.cpp:444-477): position, orientation (w,x,y,z), twist."""
        # (ekfvio_get_odometry's four slices of the base state, taken here from one 22-float read: one array and one pointer conversion
        # per frame instead of four -- the binding's own overhead was ~5 us of a 170 us frame)
        b = np.empty(22, np.float32)
        self.tc_ekf._chk(self.tc_ekf.lib.ekfvio_get_base_mu(self.tc_ekf.h, _fp(b)))
        return dict(position=b[0:3], orientation_wxyz=b[3:7], linear=b[7:10], angular=b[10:13])

    def points(self):
        """publishPoints (EKFVIO.cpp:479-518), formed on the device: (xyz[N,3], intensity[N]) = camera-frame
        (u/rho, v/rho, 1/rho) per landmark and the current frame's byte at the landmark's pixel."""
        N = self.tc_ekf.num_features
        xyz, inten = np.empty((N, 3), np.float32), np.empty(N, np.float32)
        self.tc_ekf._chk(self.tc_ekf.lib.ekfvio_get_points(self.tc_ekf.h, _fp(xyz), _fp(inten)))
        return xyz, inten
