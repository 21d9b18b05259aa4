"""Landmark identities and the tracks that ended (ekfvio_get_landmark_ids, ekfvio_set_ended_export, ekfvio_get_ended) on the device.

The ids and birth stamps travel with the state through the two kernels that move landmarks (add_features_kernel, remove_features_kernel);
the device is held to the pure-Python model of tests/_tracks.py, exactly.  The records of the landmarks a removal takes out are held, bit for
bit, to what ekfvio_get_points and ekfvio_get_points_covariance returned for those rows in front of the removal.

Handles that are compared are run one after the other, each as the device's only live handle (as tests/test_gpu_remove.py does)."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from ekf_vio_amd import EKFVIO, TightlyCoupledEKF, capi
from ekf_vio_amd.sim import Scenario, translated_sequence

from _covout import points_cov32
from _tracks import TrackModel, ended_arrays

pytestmark = pytest.mark.gpu
IMG = os.path.join(os.path.dirname(__file__), "golden", "images")
K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)
KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


def grey(name="640_480_test"):
    return np.asarray(Image.open(os.path.join(IMG, name + "_gray.png")))


def same(a, b):
    """array_equal where NaN equals NaN (birth stamps before any stamp), dtype and shape included."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def compact(st, remove):
    """tests/test_gpu_remove.py's reference, restated: the state with the removed landmarks' entries, rows and columns taken out."""
    keep = ~np.asarray(remove, bool)
    lm = np.nonzero(keep)[0]
    idx = np.concatenate([np.arange(22), (22 + 3 * lm[:, None] + np.arange(3)[None, :]).reshape(-1)]).astype(np.int64)
    return dict(base_mu=st["base_mu"].copy(), feat_mu=st["feat_mu"][keep].copy(), last_klt=st["last_klt"][keep].copy(),
                del_flag=st["del_flag"][keep].copy(), Sigma=np.ascontiguousarray(st["Sigma"][np.ix_(idx, idx)]))


def random_state(N, seed):
    rng = np.random.default_rng(seed)
    n = 22 + 3 * N
    A = rng.standard_normal((n, n))
    S = (A @ A.T / n + np.eye(n)).astype(np.float32)
    S = np.ascontiguousarray((S + S.T) / 2)
    base = rng.standard_normal(22).astype(np.float32)
    base[3:7] = np.array([1, 0, 0, 0], np.float32)
    return dict(base_mu=base, feat_mu=rng.standard_normal((N, 3)).astype(np.float32), last_klt=rng.standard_normal((N, 2)).astype(np.float32),
                del_flag=(rng.random(N) < 0.2).astype(np.uint8), Sigma=S)


def masks(N, seed):
    rng = np.random.default_rng(seed)
    out = {"random": rng.random(N) < 0.3, "none": np.zeros(N, bool), "all": np.ones(N, bool)}
    runs = np.zeros(N, bool)
    for start in range(0, N, max(N // 3, 1)):
        runs[start:start + max(N // 7, 1)] = True
    out["runs"] = runs
    first, last = np.zeros(N, bool), np.zeros(N, bool)
    first[0], last[-1] = True, True
    out["first"], out["last"] = first, last
    return out


def points_of(g):
    xyz = np.empty((g.num_features, 3), np.float32)
    g._chk(g.lib.ekfvio_get_points(g.h, xyz.ctypes.data_as(C.POINTER(C.c_float)), None))
    return xyz


def assert_ids(g, model, what):
    ids, born = g.landmark_ids()
    assert same(ids, model.ids) and same(born, model.born), (what, ids, model.ids, born, model.born)
    assert np.all(np.diff(ids) > 0), what


def assert_ended(e, ended, what):
    eid, eborn, eidx = ended_arrays(ended)
    assert e["count"] == len(ended), (what, e["count"], len(ended))
    assert same(e["id"], eid) and same(e["born"], eborn) and same(e["index_before"], eidx), (what, e, ended)


# ------------------------------------------------------------------ 1. append
def test_append_hands_out_consecutive_ids_and_capacity_refusal_hands_out_none():
    g = TightlyCoupledEKF(max_features=8)
    m = TrackModel()
    rng = np.random.default_rng(0)
    for k in (5, 3):
        g.addNewFeatures(rng.standard_normal((k, 2)).astype(np.float32))
        m.append(k, np.nan)
        assert_ids(g, m, k)
    ids, born = g.landmark_ids()
    assert same(ids, np.arange(8, dtype=np.int64)) and np.all(np.isnan(born)) and born.dtype == np.float64  # no stamp yet
    with pytest.raises(capi.EkfvioError) as err:
        g.addNewFeatures(np.zeros((1, 2), np.float32))
    assert err.value.code == capi.ECAPACITY
    assert_ids(g, m, "after the refused append")
    rm = np.zeros(8, np.uint8)
    rm[2] = 1
    assert g.removeFeatures(rm) == 1
    m.remove(rm)
    g.addNewFeatures(np.zeros((1, 2), np.float32))
    m.append(1, np.nan)
    assert_ids(g, m, "append behind a removal")
    assert g.landmark_ids()[0][-1] == 8  # the refused append took no id
    g.close()


# ------------------------------------------------------------------ 2. compaction against the model
# N = 3: one landmark per scan thread; 257: the first N where scan_keep gives a thread two landmarks; 300: chunks of two throughout
@pytest.mark.parametrize("N", [3, 257, 300])
def test_removal_compacts_ids_and_stamps_as_the_model_does(N):
    g = TightlyCoupledEKF(max_features=N, ended_export=True)
    st = random_state(N, seed=N)
    model = TrackModel()
    total = 0
    for name, mask in masks(N, seed=N + 1).items():
        g.set_state(st)
        model.replace(N, np.nan)
        assert_ids(g, model, (name, "set_state"))
        k = g.removeFeatures(mask.astype(np.uint8))
        ended = model.remove(mask)
        assert k == int(mask.sum()) == len(ended), name
        total += k
        assert_ids(g, model, name)
        e = g.ended()
        assert_ended(e, ended, name)
        assert e["total"] == total, name
        got, want = g.get_state(), compact(st, mask)
        for key in KEYS:
            assert same(got[key], want[key]), (N, name, key)
    g.close()


# ------------------------------------------------------------------ 3. the ended records carry the getters' bits
def spread_pass(N, phase):
    p = np.ones(N, np.uint8)
    p[(np.arange(N) + phase) % 7 == 0] = 0
    return p


def flagged_handle(N, **kw):
    """A handle with a dense Sigma (three simulated updates) and the stride-7 landmarks flagged by a fourth."""
    sc = Scenario(N, seed=N)
    g = TightlyCoupledEKF(max_features=N, **kw)
    g.addNewFeatures(sc.initial_features())
    frames = list(sc.frames(4))
    for z, R, p in frames[:3]:
        g.process(sc.dt)
        assert g.updateWithFeaturePositions(z, R, p) in (capi.OK, capi.ENUMERIC)
    z, R, _ = frames[3]
    g.process(sc.dt)
    assert g.updateWithFeaturePositions(z, R, spread_pass(N, 2)) in (capi.OK, capi.ENUMERIC)
    return g


def test_ended_records_are_the_getters_rows_in_front_of_the_removal():
    N = 40
    g = flagged_handle(N, ended_export=True)
    g.profile(True)
    pre = g.get_state()
    flags = pre["del_flag"].astype(bool)
    assert flags.sum() >= N // 7
    ids, born = g.landmark_ids()
    xyz, cov = points_of(g), g.points_covariance()
    misc = g.profile_report()["update_misc"]["launches"]
    assert g.removeFeatures(None) == int(flags.sum())
    assert g.profile_report()["update_misc"]["launches"] == misc + 1  # the export's one launch
    e = g.ended()
    assert e["count"] == int(flags.sum()) and same(e["index_before"], np.nonzero(flags)[0].astype(np.int32))
    assert same(e["id"], ids[flags]) and same(e["born"], born[flags])
    assert same(e["xyz"], xyz[flags]) and same(e["cov"], cov[flags])
    assert same(e["cov"], points_cov32(pre["feat_mu"], pre["Sigma"])[flags])
    # a removal call that removes nothing reports 0: nothing flagged any more, an explicit mask of zeros
    assert g.removeFeatures(None) == 0 and g.ended()["count"] == 0
    assert g.removeFeatures(np.zeros(g.num_features, np.uint8)) == 0 and g.ended()["count"] == 0
    assert g.ended()["total"] == int(flags.sum())
    g.close()


def test_export_off_launches_nothing_and_reports_nothing():
    N = 40
    g = flagged_handle(N)
    g.profile(True)
    k = int(g.get_state()["del_flag"].sum())
    misc = g.profile_report()["update_misc"]["launches"]
    assert g.removeFeatures(None) == k > 0
    assert g.profile_report()["update_misc"]["launches"] == misc  # ended_tracks_kernel is not in the handle's profile
    e = g.ended()
    assert e["count"] == 0 and e["total"] == 0 and e["id"].shape == (0,)
    g.close()


# ------------------------------------------------------------------ 4. the frame loop against a twin that removes after every frame
def test_frame_loop_ids_and_ended_records_equal_a_twin_and_the_model():
    seq = translated_sequence(grey(), 12, dx=-3.1, dy=-1.3)
    stamps = [3.0 + i / 30.0 for i in range(len(seq))]
    # A: the removal inside the frame, the export on
    a = EKFVIO(max_features=64, replenish=1, remove_lost=1, ended_export=True)
    rows_a = []
    for stamp, img in zip(stamps, seq):
        assert a.addFrame(stamp, img, K) in (capi.OK, capi.ENUMERIC)
        rows_a.append((a.landmark_ids(), a.ended(), a.points()[0].copy()))
    a.tc_ekf.close()
    # B: flags left standing by the frame, read by the test, then removed; the model is driven by what B shows, never by A
    b = EKFVIO(max_features=64, replenish=1, remove_lost=0)
    model = TrackModel()
    n_ended = n_entered_later = 0
    for i, (stamp, img) in enumerate(zip(stamps, seq)):
        n_before = b.tc_ekf.num_features
        assert b.addFrame(stamp, img, K) in (capi.OK, capi.ENUMERIC)
        st = b.tc_ekf.get_state()
        flags = st["del_flag"].astype(bool)
        n_after = b.tc_ekf.num_features
        model.append(n_after - n_before, stamp)
        n_entered_later += (n_after - n_before) if i > 0 else 0
        xyz_before = b.points()[0].copy()
        ended = model.remove(flags)
        n_ended += len(ended)
        assert b.tc_ekf.removeFeatures(None) == len(ended), i
        assert_ids(b.tc_ekf, model, ("B", i))
        (ids_a, born_a), e_a, xyz_a = rows_a[i]
        assert same(ids_a, model.ids) and same(born_a, model.born), ("A", i)
        assert_ended(e_a, ended, ("A", i))
        assert same(e_a["xyz"], xyz_before[flags]), i
        assert same(xyz_a, b.points()[0]), i  # rows of the ids are the rows of the cloud
        assert set(born_a.tolist()) <= set(stamps[:i + 1]), i  # every landmark was born at the stamp of a frame
    b.tc_ekf.close()
    assert n_ended > 0, "no landmark ended: the loop does not exercise the removal"
    assert n_entered_later > 0, "no landmark entered after frame 0: the loop does not exercise the replenishment"


# ------------------------------------------------------------------ 5. frames that cannot change the set (outputs published early)
def test_ids_stand_still_through_frames_that_publish_early():
    seq = translated_sequence(grey(), 5, dx=-3.1, dy=-1.3)
    v = EKFVIO(max_features=32, replenish=1, remove_lost=0)
    assert v.addFrame(1.0, seq[0], K) == capi.OK
    assert v.tc_ekf.num_features == 32  # full: no later frame can add, none removes
    ids0, born0 = v.landmark_ids()
    assert same(ids0, np.arange(32, dtype=np.int64)) and np.all(born0 == 1.0)
    early0 = v.tc_ekf.counters()["early_output_frames"]
    for i, img in enumerate(seq[1:]):
        assert v.addFrame(1.0 + (i + 1) / 30.0, img, K) in (capi.OK, capi.ENUMERIC)
        ids, born = v.landmark_ids()  # (arrived with the frame's outputs)
        assert same(ids, ids0) and same(born, born0), i
    assert v.tc_ekf.counters()["early_output_frames"] > early0  # the early-publication road really ran
    v.tc_ekf.process(0.0)  # (the outputs are stale now: the getter reads the device's arrays)
    ids, born = v.landmark_ids()
    assert same(ids, ids0) and same(born, born0)
    v.tc_ekf.close()


# ------------------------------------------------------------------ 6. lifecycle
def test_lifecycle_reset_set_state_run_uploaded_and_bad_arguments():
    N = 16
    sc = Scenario(N, seed=2)
    g = TightlyCoupledEKF(max_features=N, ended_export=True)
    model = TrackModel()
    g.addNewFeatures(sc.initial_features())
    model.append(N, np.nan)
    assert_ids(g, model, "first append")
    # run_uploaded leaves both arrays alone
    frames = list(sc.frames(4))
    g.upload_measurements(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames]))
    g.run_uploaded(0, 4, sc.dt)
    assert g.synchronize() in (capi.OK, capi.ENUMERIC)
    assert_ids(g, model, "behind run_uploaded")
    # a removal, so that the total is not zero when the reset comes
    rm = np.zeros(N, np.uint8)
    rm[[1, 5]] = 1
    assert g.removeFeatures(rm) == 2
    assert_ended(g.ended(), model.remove(rm), "removal")
    assert g.ended()["total"] == 2
    # cap too small: EINVAL, the count still set
    k, total = C.c_int32(-1), C.c_int64(-1)
    assert g.lib.ekfvio_get_ended(g.h, None, None, None, None, None, 1, C.byref(k), C.byref(total)) == capi.EINVAL
    assert k.value == 2 and total.value == 2
    assert g.lib.ekfvio_get_ended(g.h, None, None, None, None, None, 2, C.byref(k), None) == capi.OK
    # reset: no landmarks, the counter goes on, the export stays on, its report and total start over
    seen_max = model.next_id - 1
    g.initializeBaseState()
    model.reset()
    assert g.num_features == 0 and g.ended()["count"] == 0 and g.ended()["total"] == 0
    g.addNewFeatures(sc.initial_features()[:3])
    model.append(3, np.nan)
    assert_ids(g, model, "append behind reset")
    assert g.landmark_ids()[0].min() > seen_max
    # set_state: five fresh consecutive ids
    g.set_state(random_state(5, seed=9))
    model.replace(5, np.nan)
    assert_ids(g, model, "set_state")
    assert same(g.landmark_ids()[0], np.arange(N + 3, N + 8, dtype=np.int64))
    # the export is still on behind the reset
    assert g.removeFeatures(np.array([0, 0, 1, 0, 0], np.uint8)) == 1
    assert_ended(g.ended(), model.remove([0, 0, 1, 0, 0]), "behind reset")
    # bad arguments
    assert g.lib.ekfvio_set_ended_export(g.h, 2) == capi.EINVAL and g.lib.ekfvio_set_ended_export(g.h, -1) == capi.EINVAL
    assert g.ended()["count"] == 1  # a refused setting changes nothing
    g.close()
