"""Covariances of the published outputs on the device (ekf_vio_amd/csrc/frame.hip), product build, no hooks: both roads of
include/ekfvio.h -- the getters' own launches and the frame's outputs kernel -- against the NumPy float32 restatement (tests/_covout.py)
on the state read back from the same handle, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from ekf_vio_amd import EKFVIO, TightlyCoupledEKF, capi
from ekf_vio_amd.sim import translated_sequence

import _covout as co

pytestmark = pytest.mark.gpu
IMG = os.path.join(os.path.dirname(__file__), "golden", "images")
K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)
KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


def grey(name="640_480_test"):
    return np.asarray(Image.open(os.path.join(IMG, name + "_gray.png")))


def random_state(N, seed):
    """A dense random SPD Sigma, a unit quaternion well away from the identity, rho in [0.2, 2]."""
    rng = np.random.default_rng(seed)
    n = co.BASE + 3 * N
    B = rng.standard_normal((n, n)).astype(np.float32)
    Sigma = B @ B.T / np.float32(n) + np.float32(0.1) * np.eye(n, dtype=np.float32)
    Sigma = np.tril(Sigma) + np.tril(Sigma, -1).T
    base = rng.standard_normal(co.BASE).astype(np.float32)
    base[3:7] = (np.array([0.4, -0.5, 0.6, 0.48]) / np.linalg.norm([0.4, -0.5, 0.6, 0.48])).astype(np.float32)
    feat = np.stack([rng.uniform(-1, 1, N), rng.uniform(-1, 1, N), rng.uniform(0.2, 2.0, N)], axis=1).astype(np.float32)
    return dict(base_mu=base, feat_mu=feat, last_klt=feat[:, :2].copy(), del_flag=np.zeros(N, np.uint8), Sigma=Sigma)


def assert_outputs_are_the_restatement(ekf, where=""):
    """The getters against the restatement on get_state() of the same handle; returns (pose, twist, landmarks)."""
    pose, twist = ekf.odometry_covariance()
    pts = ekf.points_covariance()
    st = ekf.get_state()
    rp, rt, rl = co.covariances32(st["base_mu"], st["feat_mu"], st["Sigma"])
    assert pts.shape == (st["feat_mu"].shape[0], 3, 3), where
    assert np.array_equal(pose, rp), (where, np.abs(pose - rp).max())
    assert np.array_equal(twist, rt), where
    assert np.array_equal(pts, rl), (where, np.abs(pts - rl).max() if pts.size else 0)
    return pose, twist, pts


def test_prior_without_landmarks():
    """N = 0: no landmark; the prior's Sigma is diag [0 x 7, 30 x 9, 0.5 x 6], so the pose covariance is all zeros and the twist's is 30 I."""
    ekf = TightlyCoupledEKF(max_features=4)
    pose, twist, pts = assert_outputs_are_the_restatement(ekf)
    assert not pose.any() and np.array_equal(twist, 30 * np.eye(6, dtype=np.float32)) and pts.shape == (0, 3, 3)
    ekf.close()


@pytest.mark.parametrize("N", [1, 3, 256, 257])
def test_on_demand_road_has_the_bits_of_the_restatement(N):
    """N = 256 is the single workgroup that publishes the host words itself, 257 the first grid that publishes through wait_status."""
    ekf = TightlyCoupledEKF(max_features=257)
    ekf.set_state(random_state(N, N))
    pose, twist, pts = assert_outputs_are_the_restatement(ekf, N)
    assert pose[3:, 3:].any() and np.abs(pose[3:, :3]).min() > 0 and np.abs(pts).min() > 0  # a dense Sigma, an attitude away from the identity
    assert np.array_equal(pose, pose.T) and np.array_equal(pts, pts.transpose(0, 2, 1))
    ekf.close()


def test_only_the_lower_triangle_is_read():
    ekf = TightlyCoupledEKF(max_features=8)
    st = random_state(3, 11)
    ekf.set_state(st)
    before = assert_outputs_are_the_restatement(ekf)
    iu = np.triu_indices(st["Sigma"].shape[0], 1)
    st["Sigma"][iu] += np.float32(0.25) + np.abs(st["Sigma"][iu])  # every element above the diagonal moves, by a lot
    ekf.set_state(st)
    assert not np.array_equal(ekf.get_state()["Sigma"], ekf.get_state()["Sigma"].T)
    after = assert_outputs_are_the_restatement(ekf)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    ekf.close()


def test_getters_are_ordered_behind_the_update():
    """ekfvio_update returns when the sweep's status is known, possibly with the Joseph GEMM still running: the getters, called at once and
    without a synchronize, are enqueued on the handle's stream and must see the updated state."""
    ekf = TightlyCoupledEKF(max_features=8)
    st = random_state(5, 12)
    ekf.set_state(st)
    z = st["feat_mu"][:, :2] + np.float32(0.01)
    R = np.tile(np.array([1e-5, 0, 0, 1e-5], np.float32), (5, 1))
    rc = ekf.updateWithFeaturePositions(z, R, np.ones(5, np.uint8))
    assert rc in (capi.OK, capi.ENUMERIC)
    pose, twist = ekf.odometry_covariance()
    pts = ekf.points_covariance()
    now = ekf.get_state()
    assert not np.array_equal(now["Sigma"], st["Sigma"])
    rp, rt, rl = co.covariances32(now["base_mu"], now["feat_mu"], now["Sigma"])
    assert np.array_equal(pose, rp) and np.array_equal(twist, rt) and np.array_equal(pts, rl)
    ekf.close()


def run_frames(seq, on, **kw):
    v = EKFVIO(replenish=1, output_covariance=on, **kw)
    rows = []
    for i, img in enumerate(seq):
        rc = v.addFrame(2.0 + i / 30.0, img, K)
        pose, twist, pts = assert_outputs_are_the_restatement(v.tc_ekf, (on, i))
        assert pts.shape == (v.tc_ekf.num_features, 3, 3), i
        od = v.odometry()
        xyz, inten = v.points()
        rows.append(dict(rc=rc, N=v.tc_ekf.num_features, pose=pose.copy(), twist=twist.copy(), pts=pts.copy(), xyz=xyz.copy(), inten=inten.copy(),
                         odom=np.concatenate([od[k] for k in ("position", "orientation_wxyz", "linear", "angular")]), state=v.tc_ekf.get_state()))
    early = v.tc_ekf.counters()["early_output_frames"]
    v.tc_ekf.close()
    return rows, early


@pytest.mark.parametrize("max_features,remove_lost", [(48, 0), (48, 1), (160, 0), (160, 1)])
def test_in_frame_road(max_features, remove_lost):
    """Six frames of the motion of tests/test_gpu_frame_outputs.py, whose frames both add and remove landmarks: with the setting on, every
    frame's covariances (written by frame_outputs_kernel with the status word; behind a removal from the buffer the removal wrote, behind a
    replenishment with the new landmarks' prior blocks) are the restatement's on the state read back, and no frame publishes early.  With the
    setting off the same frames give the same state and outputs bit for bit: the setting changes when outputs go out, never what is computed."""
    seq = translated_sequence(grey(), 6, dx=-6.0, dy=-2.5)
    rows_on, early_on = run_frames(seq, True, max_features=max_features, remove_lost=remove_lost)
    rows_off, early_off = run_frames(seq, False, max_features=max_features, remove_lost=remove_lost)
    assert early_on == 0
    if (max_features, remove_lost) == (48, 0):
        assert early_off > 0  # (full from the first frame on, nothing removed: these frames publish in front of the update's last GEMM)
    print("landmarks per frame:", [r["N"] for r in rows_on], "early frames with the setting off:", early_off)
    for i, (a, b) in enumerate(zip(rows_on, rows_off)):
        assert a["rc"] == b["rc"] and a["rc"] in (capi.OK, capi.ENUMERIC) and a["N"] == b["N"], i
        for k in ("pose", "twist", "pts", "xyz", "inten", "odom"):
            assert np.array_equal(a[k], b[k]), (i, k)
        for k in KEYS:
            assert np.array_equal(a["state"][k], b["state"][k]), (i, k)
    assert any(r["N"] > 0 and r["pts"].any() for r in rows_on[1:])
    if (max_features, remove_lost) == (48, 1):  # (48 46 48 46 47 47 in the CPU oracle: frames that remove, frames that add)
        assert len({r["N"] for r in rows_on[1:]}) > 1, "no frame changed the landmark count"


def test_cached_covariances_are_dropped_when_sigma_changes():
    """With the setting on the getters behind a frame are a memcpy of what the frame wrote.  setFeatureHomogenousCovariance changes Sigma and
    nothing else: the next getter must launch again and return the covariance of the NEW state."""
    seq = translated_sequence(grey(), 2, dx=-6.0, dy=-2.5)
    v = EKFVIO(replenish=1, output_covariance=True, max_features=48)
    for i, img in enumerate(seq):
        v.addFrame(2.0 + i / 30.0, img, K)
    cached = assert_outputs_are_the_restatement(v.tc_ekf)[2]
    v.tc_ekf.setFeatureHomogenousCovariance(0, [[0.5, 0.125], [0.125, 0.25]])
    fresh = assert_outputs_are_the_restatement(v.tc_ekf)[2]
    assert not np.array_equal(fresh[0], cached[0]) and np.array_equal(fresh[1:], cached[1:])
    v.tc_ekf.close()


def test_setter_rejects_other_values_and_survives_reset():
    seq = translated_sequence(grey(), 3, dx=-6.0, dy=-2.5)
    v = EKFVIO(replenish=1, max_features=48)
    lib, h = v.tc_ekf.lib, v.tc_ekf.h
    assert lib.ekfvio_set_output_covariance(h, 2) == capi.EINVAL and lib.ekfvio_set_output_covariance(h, -1) == capi.EINVAL
    early = []
    for on in (0, 1):
        assert lib.ekfvio_set_output_covariance(h, on) == capi.OK
        v.tc_ekf.initializeBaseState()  # (the setting is the handle's, like the distortion: it stays)
        before = v.tc_ekf.counters()["early_output_frames"]
        for i, img in enumerate(seq):
            v.addFrame(2.0 + i / 30.0, img, K)
        assert_outputs_are_the_restatement(v.tc_ekf, on)
        early.append(v.tc_ekf.counters()["early_output_frames"] - before)
    assert early[0] > 0 and early[1] == 0, early
    v.tc_ekf.close()
