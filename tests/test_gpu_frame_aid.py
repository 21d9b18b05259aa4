"""The standing aiding measurement of ekfvio_step_image (include/ekfvio.h, ekfvio_set_frame_aid; ekf_vio_amd/csrc/aid.hip, frame.hip) against
a second handle driven call by call, in the manner of tests/_frame_twin.py, whose sequence, getters and comparison these tests use.

Six frames at 64 landmarks -- the camera stands still for three, then the plane moves -- with a nonholonomic-shaped H (the velocity across
the camera's optical axis is zero): the fused frame applies it behind the tracker, in front of the zero-velocity update, the gate and the
camera update.  The second handle does push_frame, process, klt_track, aid_update, (zupt decision and update), update, replenish, remove by
hand.  Everything a node can read behind every frame must match bit for bit, the aiding update's own report included.  Alone, and with the
zero-velocity update, the gate and remove_lost on.  With the setting off the outputs are those of a handle that never heard of it.

Each handle is closed before the next is created (the persistent sweep is for a device's sole handle).
"""
import ctypes as C

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, capi

import _aid as A
import _frame_twin as T

pytestmark = pytest.mark.gpu

F32 = np.float32
N_MAX = 64
FRAMES = 6
# v_x = v_y = 0 in the camera frame: a forward-looking camera on a wheeled vehicle (the node's nhc_variance with the default nhc_R_cv)
NHC = (-A.selection([7, 8]), np.zeros(2, F32), np.array([1e-3, 1e-3], F32))
BASE = dict(replenish=1, **T.DETECTOR)
ALL_ON = dict(BASE, remove_lost=1, zupt=T.ZUPT, gate_chi2=T.GATE_CHI2)


def _aid_row(e):
    s = e.aid_status()
    return {"aid.d2": np.array([s["d2_last"]], F32), "aid.counts": np.array([s["accepted_last"], s["applied_total"], s["rejected_total"]], np.int64)}


def fused(seq, settings, aid, before=None):
    """T.fused with the standing measurement and its report in every row; aid = (H, z, R, chi2) or None."""
    v = EKFVIO(max_features=N_MAX, frame_aid=aid, **settings)
    e, rows, t = v.tc_ekf, [], T.stamps(len(seq))
    try:
        if before:
            before(v)
        for i, img in enumerate(seq):
            h, w = img.shape
            buf = np.ascontiguousarray(img)
            rc_ = e._chk(e.lib.ekfvio_step_image(e.h, float(t[i]), T._u8(buf), w, h, w, T._fp(T.K)), allow=(capi.ENUMERIC,))
            row = T._getters(v)
            z = v.zupt()
            row.update(T._zupt_row(z["flow2"], z["n_pass"], z["n_still"], z["applied_last"], z["applied_total"]))
            row.update(_aid_row(e))
            row["return_code"] = np.array([rc_], np.int64)
            rows.append(row)
    finally:
        e.close()
    return rows


def call_by_call(seq, settings, aid):
    """T.call_by_call with ekfvio_aid_update behind the tracker, in front of the zero-velocity decision."""
    mine = dict(settings)
    do_replenish, do_remove = bool(mine.pop("replenish", 0)), bool(mine.pop("remove_lost", 0))
    zupt = mine.pop("zupt", None)
    v = EKFVIO(max_features=N_MAX, hooks=True, replenish=0, remove_lost=0, **mine)
    e, lib, rows, t = v.tc_ekf, v.tc_ekf.lib, [], T.stamps(len(seq))
    intr = T.frame_intrinsics(T.K, None, 1, bool(e.cfg.use_principal_point))
    clock, applied_total = None, 0
    try:
        for i, img in enumerate(seq):
            h, w = img.shape
            buf = np.ascontiguousarray(img)
            added = removed = 0
            zrow = T._zupt_row(np.zeros(0, F32), 0, 0, 0, applied_total)
            if i == 0:
                rc_ = e._chk(lib.ekfvio_step_image(e.h, float(t[0]), T._u8(buf), w, h, w, T._fp(T.K)))
                clock = t[0]
                if do_replenish:
                    added = len(v.replenishFeatures())
                rows.append(dict(T._getters(v), **zrow, **_aid_row(e), return_code=np.array([rc_], np.int64), _added=added, _removed=0, _n_before=0))
                continue
            e.process(float(F32(np.float64(t[i]) - np.float64(clock))))
            clock = t[i]
            e._chk(lib.ekfvio_klt_push_frame(e.h, T._u8(buf), w, h, w, T._fp(T.K)))
            n_before = e.num_features
            rc_ = capi.OK
            if n_before > 0:
                before = e.get_state()
                zm, R, p = v.tracker.findNewFeaturePositions()
            if aid is not None:  # (landmarks or not, as the fused frame)
                e.aidUpdate(*aid)
            if n_before > 0:
                if zupt is not None:
                    ref = T.reference_pixels(before["last_klt"], intr)
                    prev_px, next_px = np.zeros((n_before, 2), F32), np.zeros((n_before, 2), F32)
                    e._chk(lib.ekfvio_test_klt_pixels(e.h, T._fp(prev_px), T._fp(next_px), n_before))
                    flow2, np_, ns_, st_ = np.zeros(n_before, F32), C.c_int32(0), C.c_int32(0), C.c_int32(0)
                    e._chk(lib.ekfvio_zupt_decide(T._fp(ref), T._fp(next_px), T._u8(p), n_before, zupt[0], zupt[1], zupt[2], T._fp(flow2),
                                                  C.byref(np_), C.byref(ns_), C.byref(st_)))
                    if st_.value:
                        e.zuptUpdate(zupt[3], zupt[4])
                    applied_total += int(st_.value != 0)
                    zrow = T._zupt_row(flow2, np_.value, ns_.value, int(st_.value != 0), applied_total)
                rc_ = e.updateWithFeaturePositions(zm, R, p)
            if do_replenish:
                added = len(v.replenishFeatures())
            if do_remove:
                removed = e.removeFeatures(None)
            row = T._getters(v)
            row.update(zrow, **_aid_row(e), return_code=np.array([rc_], np.int64), _added=added, _removed=removed, _n_before=n_before)
            rows.append(row)
    finally:
        e.close()
    return rows


def sequence():
    return T.sequence()[:FRAMES]


@pytest.mark.parametrize("name,settings,chi2", [("alone", BASE, 0.0), ("zupt+gate+remove_lost", ALL_ON, 0.0), ("gated, alone", BASE, 1.0)],
                         ids=["alone", "all-on", "alone-chi2"])
def test_fused_frame_is_the_call_by_call_paths_bits(name, settings, chi2):
    seq = sequence()
    aid = NHC + (chi2,)
    a = fused(seq, settings, aid)
    b = call_by_call(seq, settings, aid)
    counts = [tuple(int(x) for x in r["aid.counts"]) for r in a]
    print("\nFRAME-AID %s: landmarks %s  aid (accepted, applied, rejected) per frame %s  d2 %s  zupt applied %s  gated %s  removed %s"
          % (name, [len(r["landmark_ids"]) for r in a], counts, ["%.3g" % float(r["aid.d2"][0]) for r in a],
             [int(r["zupt.counts"][2]) for r in a], [int(r["gate.counts"][1]) for r in a], [r["_removed"] for r in b]))
    T.compare(a, b, name)
    # every frame behind the first ran it, and the first did not
    assert counts[0] == (0, 0, 0)
    assert [c[1] + c[2] for c in counts] == list(range(FRAMES))
    assert max(len(r["landmark_ids"]) for r in a) == N_MAX
    if chi2 == 0.0:
        assert counts[-1] == (1, FRAMES - 1, 0)
    else:  # the moving plane contradicts the constraint by more than a gate of 1 allows (d2 = 3.3 behind the last frame): both verdicts occur
        assert counts[-1][1] > 0 and counts[-1][2] > 0, counts
    if "zupt" in settings:
        assert sum(int(r["zupt.counts"][2]) for r in a) > 0  # the zero-velocity update ran behind it in the still frames


def test_the_update_moves_the_state_and_off_is_a_handle_that_never_heard_of_it():
    seq = sequence()
    never = fused(seq, BASE, None)
    on = fused(seq, BASE, NHC + (0.0,))
    # set, then turned off in front of the first frame
    off = fused(seq, BASE, NHC + (0.0,), before=lambda v: v.setFrameAid(None))
    T.compare(off, never, "off against never set")
    assert [tuple(r["aid.counts"]) for r in off] == [(0, 0, 0)] * FRAMES
    # ... and on, the constraint does act: the sideways velocity the moving plane teaches the filter is held down
    last = FRAMES - 1
    assert on[last]["state.Sigma"].tobytes() != never[last]["state.Sigma"].tobytes()
    vx_on, vx_never = abs(float(on[last]["odometry.linear"][0])), abs(float(never[last]["odometry.linear"][0]))
    print("\nFRAME-AID |v_x| behind frame %d: %.4g with the constraint, %.4g without" % (last, vx_on, vx_never))
    assert vx_on < vx_never


def test_the_setting_survives_a_reset_and_the_counts_start_over():
    seq = sequence()[:3]
    v = EKFVIO(max_features=N_MAX, frame_aid=NHC + (0.0,), **BASE)
    try:
        for rnd in range(2):
            for i, img in enumerate(seq):
                assert v.addFrame(3.0 + i / 30.0, np.ascontiguousarray(img), T.K) in (capi.OK, capi.ENUMERIC)
            s = v.aid_status()
            assert (s["accepted_last"], s["applied_total"], s["rejected_total"]) == (1, 2, 0), (rnd, s)
            v.reset()
            assert v.aid_status() == dict(d2_last=0.0, accepted_last=0, applied_total=0, rejected_total=0)
    finally:
        v.tc_ekf.close()


def test_a_frame_without_landmarks_applies_it_too():
    """replenish = 0 and no landmark ever: every frame behind the first is process(dt) and the standing measurement, nothing else.  Against
    a second handle that does ekfvio_process, ekfvio_klt_push_frame and ekfvio_aid_update by hand, bit for bit."""
    seq, t = sequence()[:4], T.stamps(4)
    aid = (NHC[0], np.array([0.1, -0.05], F32), NHC[2], 0.0)  # (a measured value: the mean moves as well)
    rows = {}
    for which in ("fused", "by hand"):
        v = EKFVIO(max_features=N_MAX, replenish=0, frame_aid=aid if which == "fused" else None)
        e, out, clock = v.tc_ekf, [], None
        try:
            for i, img in enumerate(seq):
                buf = np.ascontiguousarray(img)
                h, w = buf.shape
                if which == "fused" or i == 0:
                    e._chk(e.lib.ekfvio_step_image(e.h, float(t[i]), T._u8(buf), w, h, w, T._fp(T.K)))
                else:
                    e.process(float(F32(np.float64(t[i]) - np.float64(clock))))
                    e._chk(e.lib.ekfvio_klt_push_frame(e.h, T._u8(buf), w, h, w, T._fp(T.K)))
                    e.aidUpdate(*aid)
                clock = t[i]
                assert e.num_features == 0 and e.dim == 22
                st, s = e.get_state(), e.aid_status()
                out.append((st["base_mu"].tobytes(), st["Sigma"].tobytes(), F32(s["d2_last"]).tobytes(), s["accepted_last"], s["applied_total"], s["rejected_total"]))
        finally:
            e.close()
        rows[which] = out
    assert rows["fused"] == rows["by hand"]
    assert [r[3:] for r in rows["fused"]] == [(0, 0, 0), (1, 1, 0), (1, 2, 0), (1, 3, 0)]
    assert rows["fused"][1][0] != rows["fused"][0][0]  # the measured velocity reached the mean
