"""Shared by tests/test_frame_twin_cpu.py and tests/test_gpu_frame_twin.py: ONE image sequence that makes every stage of a frame act, the
settings of ekfvio_step_image's stages by name, and the frame loop twice -- fused (ekfvio_step_image does everything) and call by call (a
second handle on which every stage is a call of the public C-ABI, in the order of csrc/frame.hip) -- with a bit-for-bit comparison of
everything a node can read behind a frame.  No tolerance anywhere: the README's promise is that the fused frame "changes when outputs are
published, never what is computed".

Building the sequence and the settings touches no GPU; fused() and call_by_call() do.  Each handle is closed before the next is created
(the persistent sweep is for a device's sole handle, the convention of tests/test_gpu_zupt.py)."""
import ctypes as C
import functools

import numpy as np

from ekf_vio_amd import EKFVIO, capi
from ekf_vio_amd.sim import translated_sequence

import _camera_models as cm
import _equalize as eq
import _imu_extrinsics as ix
import _klt_fb as fb
import _mask as mk
import _rectify as rc

F32 = np.float32
K = rc.kmat(*rc.K_CENTRE)
DX, DY = -3.1, -1.3             # the translated plane's image motion per frame, as the other loop tests'
OBJECT_BOX = (160, 320, 240, 400)  # y0, y1, x0, x1 of the moving object's patch
T0, FRAME_DT = 5.0, 1.0 / 30.0
IMU_PER_FRAME = 10
GATE_CHI2 = 0.01                # (= test_gpu_gate.CHI2; the GPU test asserts it)
ZUPT = (0.25, 8, 0.75, 1e-4, 1e-4)
DETECTOR = dict(fast_threshold=20, min_new_feature_dist=12)

# ---- the sequence: where its segments are ------------------------------------------------------------------------------------------------
STILL = (0, 1, 2)          # the first image three times: the camera stands still
MOVING = tuple(range(3, 12))  # the translated plane, steps 1 .. 9
FLICKER = 6                # ... step 4 at gain 0.8
BLOCK = 7                  # ... step 5 with _klt_fb's foreign block pasted over it
OBJECT = (8, 9, 10)        # ... steps 6 .. 8 with the moving object in front
END = (11, 12)             # step 9 twice: the camera has stopped
FRAMES = 13
SHORT = 8                  # the single-setting and pair cases: still, moving, flicker, block
MOVING_STEPS = 8           # the plane's last position, in steps of (DX, DY)
# The plane starts gently: frame 3 lies FIRST_STEP of a step from the still frames, frame 4 one whole step, frame 5 two, ...  Behind three
# still frames (and two zero-velocity updates) the filter is sure it stands still, and at the gate tests' threshold a whole step rejects
# EVERY landmark, frame after frame: the state empties, refills, and no frame ever both removes and replenishes.  The first step is small
# enough (0.09 pixels) for part of the landmarks to pass the gate, so that frame 4 starts below max_features.  Tuned on the MI355X with
# every setting on: 0.02 rejects 12 of 64 and 21 of 96 landmarks in frame 3, 0.03 rejects 50 of 64 and 71 of 96, 0.04 rejects 64 of 64 and
# 94 of 96, 0.05 and above all of them.
FIRST_STEP = 0.03


def moving_steps(first_step=FIRST_STEP):
    """The plane's position in each frame of MOVING, in steps of (DX, DY)."""
    return (first_step,) + tuple(range(1, MOVING_STEPS + 1))


def paste_moving_object(seq, first, last, box=OBJECT_BOX):
    """Pastes a moving object into the images seq[first .. last], in place: the patch `box` of seq[first - 1], moved by (+3, +1) pixels a
    frame."""
    y0, y1, x0, x1 = box
    patch = seq[first - 1][y0:y1, x0:x1].copy()
    for j, i in enumerate(range(first, last + 1)):
        ox, oy = 3 * (j + 1), j + 1
        img = seq[i].copy()
        img[y0 + oy:y1 + oy, x0 + ox:x1 + ox] = patch
        seq[i] = img
    return seq


def moving_object_sequence(frames=24, first=12, last=17):
    """The loop tests' translated plane (the camera moves sideways: the image moves by (-3.1, -1.3) pixels a frame) with a moving object
    in front of it for frames first .. last: a 160 x 160 patch of frame first - 1 that moves by (+3, +1) pixels a frame, against the
    camera motion.  Returns (images, (y0, y1, x0, x1) of the patch in frame first - 1, first, last)."""
    seq = translated_sequence(fb.image("first"), frames, dx=DX, dy=DY)
    return paste_moving_object(seq, first, last), OBJECT_BOX, first, last


def plane(step):
    """The first image translated by step * (DX, DY) pixels: ekf_vio_amd.sim.translated_sequence's frame `step` for a whole step."""
    return translated_sequence(fb.image("first"), 2, dx=step * DX, dy=step * DY)[1]


@functools.lru_cache(maxsize=None)
def sequence(first_step=FIRST_STEP):
    """uint8 [FRAMES, 480, 640], read-only: STILL, MOVING with FLICKER, BLOCK and OBJECT, END (above)."""
    base = fb.image("first")
    plain = [np.array(base)] * 3 + [plane(s) for s in moving_steps(first_step)] + [plane(MOVING_STEPS)]
    paste_moving_object(plain, OBJECT[0], OBJECT[-1])  # (the patch is frame 7's plain texture, before the block goes in)
    plain[FLICKER] = eq.contrast(plain[FLICKER], 0.8, 0)
    x0, y0, x1, y1 = fb.BLOCK
    blocked = plain[BLOCK].copy()
    blocked[y0:y1, x0:x1] = base[40:40 + (y1 - y0), 60:60 + (x1 - x0)]  # the foreign texture of _klt_fb.image("blocked")
    plain[BLOCK] = blocked
    out = np.ascontiguousarray(np.stack(plain), np.uint8)
    assert out.shape == (FRAMES, 480, 640)
    out.setflags(write=False)
    return out


def stamps(frames=FRAMES):
    return [T0 + i * FRAME_DT for i in range(frames)]


def imu_stamps(i):
    """The stamps (double) of the IMU records between frame i - 1 and frame i."""
    t = stamps(i + 1)
    return [t[i - 1] + (k + 1) * (t[i] - t[i - 1]) / (IMU_PER_FRAME + 1) for k in range(IMU_PER_FRAME)]


def imu_split(record_stamps, frame_stamp, t):
    """The call-by-call path's process(dt) arguments for the records and the frame, with the filter's clock `t` kept in double as
    ekfvio_imu / ekfvio_step_image keep it: (float)(stamp - t_stamp), then t_stamp = stamp.  Returns ([dt per record], dt of the frame)."""
    dts = []
    for s in record_stamps:
        dts.append(F32(np.float64(s) - np.float64(t)))
        t = s
    return dts, F32(np.float64(frame_stamp) - np.float64(t))


def rest_reading(R_ci, gravity):
    """(gyro, accel) an IMU with the rotation R_ci reads on a camera at rest at the identity attitude: no rate, and minus gravity in the
    IMU's frame."""
    a = -(np.asarray(R_ci, np.float64).T @ np.asarray(gravity, np.float64))
    return np.zeros(3, F32), a.astype(F32)


# ---- the settings ------------------------------------------------------------------------------------------------------------------------
def settings(width=640, height=480):
    """Every per-handle setting of the frame loop, as EKFVIO(...) keyword arguments, for width x height frames."""
    return dict(camera_model=(cm.RATIONAL, cm.D_RATIONAL, cm.p4(*cm.P_ZOOM)),
                mask=mk.user_mask("rect", width, height), mask_rectify_border=True,
                equalize=eq.SETTING, klt_photometric=True, klt_fb_max_px=0.5,
                zupt=ZUPT, gate_chi2=GATE_CHI2,
                replenish=1, replenish_grid=(8, 6), remove_lost=1, ended_export=True, output_covariance=True,
                use_imu=1, imu_extrinsics=ix.ext32("generic-p"), **DETECTOR)


SINGLE = {"lens": ("camera_model",), "equalize": ("equalize",), "mask": ("mask", "mask_rectify_border"), "photometric": ("klt_photometric",),
          "forward-backward": ("klt_fb_max_px",), "zupt": ("zupt",), "gate": ("gate_chi2",), "grid": ("replenish_grid",),
          "ended-export": ("ended_export",), "output-covariance": ("output_covariance",)}
PAIRS = {"zupt+gate": ("zupt", "gate_chi2"), "zupt+imu": ("zupt", "use_imu", "imu_extrinsics"),
         "covariance+ended+gate": ("output_covariance", "ended_export", "gate_chi2")}


def subsets(width=640, height=480):
    """name -> settings: "everything", each single setting and each pair -- all with replenish = 1, remove_lost = 1 and DETECTOR."""
    every = settings(width, height)
    out = {"everything": every}
    for name, keys in list(SINGLE.items()) + list(PAIRS.items()):
        out[name] = dict({k: every[k] for k in keys}, replenish=1, remove_lost=1, **DETECTOR)
    return out


# ---- the reference pixel of the zero-velocity decision (include/ekfvio.h), in NumPy ------------------------------------------------------
def frame_intrinsics(K9, P=None, scale=1, use_principal_point=False):
    """(fx, fy, cx, cy) a pushed frame carries: K's, or the rectified camera's P = (fx', cx', fy', cy') where set, divided by the inverse
    image scale in double and narrowed; the principal point is 0 unless the configuration says otherwise (Feature.h's quirk)."""
    K9 = np.asarray(K9, F32).reshape(9)
    fx, cx, fy, cy = (K9[0], K9[2], K9[4], K9[5]) if P is None else (F32(v) for v in np.asarray(P, F32).reshape(4))
    if scale > 1:
        fx, cx, fy, cy = (F32(np.float64(v) / scale) for v in (fx, cx, fy, cy))
    if not use_principal_point:
        cx = cy = F32(0)
    return F32(fx), F32(fy), F32(cx), F32(cy)


def reference_pixels(last_klt, intr):
    """last_klt[2i] * fx + cx, last_klt[2i+1] * fy + cy in fp32: multiply, then add."""
    fx, fy, cx, cy = intr
    lk = np.asarray(last_klt, F32).reshape(-1, 2)
    x = (lk[:, 0] * fx).astype(F32) + cx
    y = (lk[:, 1] * fy).astype(F32) + cy
    return np.ascontiguousarray(np.stack([x, y], axis=1), F32)


# ---- the two loops -----------------------------------------------------------------------------------------------------------------------
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _strided(img, stride):
    """The image as the first columns of a [h, stride] buffer whose slack is 0xFF: what lies there must not be read as image."""
    h, w = img.shape
    buf = np.full((h, stride), 255, np.uint8)
    buf[:, :w] = img
    return buf


def _getters(v):
    """What a node reads behind a frame; the outputs first (behind a fused frame they are fresh: a memcpy), the state after."""
    e = v.tc_ekf
    row = {}
    od = v.odometry()
    for k in ("position", "orientation_wxyz", "linear", "angular"):
        row["odometry." + k] = od[k].copy()
    row["points.xyz"], row["points.intensity"] = v.points()
    row["odometry_covariance.pose"], row["odometry_covariance.twist"] = (c.copy() for c in v.odometry_covariance())
    row["points_covariance"] = v.points_covariance()
    row["landmark_ids"] = v.landmark_ids()[0]  # (born is left out: the call-by-call path has no frame stamp, see born_stamp in csrc/common.h)
    for k, a in e.get_state().items():
        row["state." + k] = a
    en = e.ended()
    for k in ("id", "index_before", "xyz", "cov"):
        row["ended." + k] = en[k]
    g, f, m = e.gate(), e.klt_fb(), e.mask_hits()
    row["gate.d2"], row["gate.gated"] = g["d2"], g["gated"]
    row["gate.counts"] = np.array([g["n_landmarks"], g["gated_last"], g["gated_total"]], np.int64)
    row["klt_fb.err2"], row["klt_fb.rejected"] = f["err2"], f["rejected"]
    row["klt_fb.counts"] = np.array([f["n_landmarks"], f["rejected_last"], f["rejected_total"]], np.int64)
    row["mask_hits.masked"] = m["masked"]
    row["mask_hits.counts"] = np.array([m["n_landmarks"], m["masked_last"]], np.int64)
    row["_counters"] = e.counters()  # (not compared: see compare)
    return row


def _zupt_row(flow2, n_pass, n_still, last, total):
    return {"zupt.flow2": np.ascontiguousarray(flow2, F32), "zupt.counts": np.array([n_pass, n_still, last, total], np.int64)}


def _imu(settings):
    return bool(settings.get("use_imu"))


def fused(seq, settings, max_features, scale=1, stride=None, K9=K):
    """The frames through ekfvio_step_image on one handle with all of `settings`; IMU records through ekfvio_imu.  Returns one row of
    arrays per frame."""
    v = EKFVIO(max_features=max_features, inverse_image_scale=scale, **settings)
    e, rows, t = v.tc_ekf, [], stamps(len(seq))
    try:
        reading = rest_reading(e.imuExtrinsics()[0], e.gravity()) if _imu(settings) else None
        for i, img in enumerate(seq):
            if i > 0 and reading:
                for s in imu_stamps(i):
                    e._chk(e.lib.ekfvio_imu(e.h, float(s), _fp(reading[0]), _fp(reading[1])))
            h, w = img.shape
            buf = _strided(img, stride or w)
            rc_ = e._chk(e.lib.ekfvio_step_image(e.h, float(t[i]), _u8(buf), w, h, buf.shape[1], _fp(K9)), allow=(capi.ENUMERIC,))
            row = _getters(v)
            z = v.zupt()
            row.update(_zupt_row(z["flow2"], z["n_pass"], z["n_still"], z["applied_last"], z["applied_total"]))
            row["return_code"] = np.array([rc_], np.int64)
            rows.append(row)
    finally:
        e.close()
    return rows


def call_by_call(seq, settings, max_features, scale=1, stride=None, K9=K):
    """The same frames on a second handle with the same settings where a setting is a property of the handle; what is a property of the
    frame loop (replenish, remove_lost, the zero-velocity update, the in-frame covariances) is off in its configuration and done here by
    hand, in the order of csrc/frame.hip.  Rows as fused(), plus "_added" / "_removed" per frame."""
    mine = dict(settings)
    do_replenish, do_remove = bool(mine.pop("replenish", 0)), bool(mine.pop("remove_lost", 0))
    zupt = mine.pop("zupt", None)
    mine.pop("output_covariance", None)
    v = EKFVIO(max_features=max_features, inverse_image_scale=scale, hooks=True, replenish=0, remove_lost=0, **mine)
    e, lib, rows, t = v.tc_ekf, v.tc_ekf.lib, [], stamps(len(seq))
    P = settings["camera_model"][2] if "camera_model" in settings else None
    intr = frame_intrinsics(K9, P, scale, bool(e.cfg.use_principal_point))  # (every frame here has the same K: the previous frame's too)
    clock, applied_total = None, 0
    try:
        reading = rest_reading(e.imuExtrinsics()[0], e.gravity()) if _imu(settings) else None
        for i, img in enumerate(seq):
            h, w = img.shape
            buf = _strided(img, stride or w)
            added = removed = 0
            zrow = _zupt_row(np.zeros(0, F32), 0, 0, 0, applied_total)
            if i == 0:
                rc_ = e._chk(lib.ekfvio_step_image(e.h, float(t[0]), _u8(buf), w, h, buf.shape[1], _fp(K9)))
                clock = t[0]
                if do_replenish:
                    added = len(v.replenishFeatures())
                rows.append(dict(_getters(v), **zrow, return_code=np.array([rc_], np.int64), _added=added, _removed=0, _n_before=0))
                continue
            dts, dt_frame = imu_split(imu_stamps(i) if reading else [], t[i], clock)
            for dt in dts:  # 1. the records: process + ekfvio_imu_update
                e.process(float(dt))
                e.imuUpdate(*reading)
            e.process(float(dt_frame))  # 2.
            clock = t[i]
            e._chk(lib.ekfvio_klt_push_frame(e.h, _u8(buf), w, h, buf.shape[1], _fp(K9)))  # 3.
            n_before = e.num_features
            rc_ = capi.OK
            if n_before > 0:
                before = e.get_state()
                zm, R, p = v.tracker.findNewFeaturePositions()  # 4. (the forward-backward and mask reports: _getters below)
                if zupt is not None:  # 5.
                    ref = reference_pixels(before["last_klt"], intr)
                    prev_px, next_px = np.zeros((n_before, 2), F32), np.zeros((n_before, 2), F32)
                    e._chk(lib.ekfvio_test_klt_pixels(e.h, _fp(prev_px), _fp(next_px), n_before))
                    assert prev_px.tobytes() == ref.tobytes(), ("frame %d: the tracker's reference pixels are not last_klt * f + c of the "
                                                                "previous frame's intrinsics" % i, intr)
                    flow2, np_, ns_, st_ = np.zeros(n_before, F32), C.c_int32(0), C.c_int32(0), C.c_int32(0)
                    e._chk(lib.ekfvio_zupt_decide(_fp(ref), _fp(next_px), _u8(p), n_before, zupt[0], zupt[1], zupt[2], _fp(flow2),
                                                  C.byref(np_), C.byref(ns_), C.byref(st_)))
                    if st_.value:
                        e.zuptUpdate(zupt[3], zupt[4])
                    applied_total += int(st_.value != 0)
                    zrow = _zupt_row(flow2, np_.value, ns_.value, int(st_.value != 0), applied_total)
                rc_ = e.updateWithFeaturePositions(zm, R, p)  # 6. (the gate is the handle's)
            gate = e.gate()
            if do_replenish:
                added = len(v.replenishFeatures())  # 7.
            if do_remove:
                # 8. (also behind a frame that began without a landmark, where the fused frame launches no removal: nothing is flagged, so
                # nothing leaves here either, and both report no ended track)
                removed = e.removeFeatures(None)
            row = _getters(v)  # 9.
            # the gate's report is "of the most recent update": read in front of the removal too, it must not have moved
            assert gate["d2"].tobytes() == row["gate.d2"].tobytes() and gate["gated"].tobytes() == row["gate.gated"].tobytes(), i
            row.update(zrow, return_code=np.array([rc_], np.int64), _added=added, _removed=removed, _n_before=n_before)
            rows.append(row)
    finally:
        e.close()
    return rows


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------
def _first_difference(a, b):
    if a.shape != b.shape:
        return "shapes %s (fused) and %s (call by call)" % (a.shape, b.shape)
    fa, fb_ = a.reshape(-1), b.reshape(-1)
    word = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[fa.dtype.itemsize]
    bad = np.nonzero(fa.view(word) != fb_.view(word))[0]
    at = np.unravel_index(int(bad[0]), a.shape)
    return "%d of %d elements differ, the first at %s: fused %r, call by call %r" % (bad.size, fa.size, tuple(int(x) for x in at), fa[bad[0]], fb_[bad[0]])


def compare(rows_fused, rows_twin, what=""):
    """Every recorded array of every frame: dtype, shape and bytes.  Not compared, each for its stated reason:
      - born (never recorded): the call-by-call path has no frame stamp (born_stamp, csrc/common.h);
      - ekfvio_get_counters: the call-by-call update is sized from the host-known row count, the fused frame's for m = 2N
        (tests/test_gpu_klt.py, the device-side row count), so the launch plans legitimately differ; `recoveries` is looked at -- an
        aborted persistent sweep re-runs a replenishing frame "not bit for bit" (csrc/frame.hip) and the message says so."""
    assert len(rows_fused) == len(rows_twin)
    rec = (rows_fused[-1]["_counters"]["recoveries"], rows_twin[-1]["_counters"]["recoveries"])
    note = ""
    if any(rec):
        note = (" -- NOTE: a persistent sweep was aborted and re-run in this loop (recoveries: fused %d, call by call %d): on a shared GPU "
                "the re-run of a replenishing frame is documented as not bit for bit (csrc/frame.hip)" % rec)
    for i, (a, b) in enumerate(zip(rows_fused, rows_twin)):
        keys = sorted(k for k in a if not k.startswith("_"))
        assert keys == sorted(k for k in b if not k.startswith("_")), (i, set(a) ^ set(b))
        for k in keys:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype, (what, i, k, x.dtype, y.dtype)
            if x.shape != y.shape or x.tobytes() != y.tobytes():
                raise AssertionError("%s frame %d, %s: %s%s" % (what, i, k, _first_difference(x, y), note))


def exercised(rows_twin, min_tracks=ZUPT[1]):
    """What the loop made the stages do, counted on the call-by-call handle's reports."""
    later = rows_twin[1:]
    z = [r["zupt.counts"] for r in later]
    return {
        "zupt applied (frames)": sum(int(c[2]) for c in z),
        "zupt refused with n_pass >= min_tracks (frames)": sum(int(c[2] == 0 and c[0] >= min_tracks) for c in z),
        "gated (landmarks)": sum(int(r["gate.counts"][1]) for r in later if r["_n_before"] > 0),
        "forward-backward rejected (landmarks)": sum(int(r["klt_fb.counts"][1]) for r in later if r["_n_before"] > 0),
        "masked (landmarks)": sum(int(r["mask_hits.counts"][1]) for r in later if r["_n_before"] > 0),
        "removed (landmarks)": sum(r["_removed"] for r in later),
        "replenished behind frame 0 (landmarks)": sum(r["_added"] for r in later),
        "frames with a removal and a replenishment": sum(int(r["_removed"] > 0 and r["_added"] > 0) for r in later),
        "ended records": sum(len(r["ended.id"]) for r in later),
        "largest landmark count": max(len(r["landmark_ids"]) for r in rows_twin),
    }
