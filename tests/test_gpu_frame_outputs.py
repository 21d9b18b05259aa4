"""The frame loop's two ways of delivering a frame's results (ekf_vio_amd/csrc/frame.hip), product build, no hooks.

1. EKFVIO_FRAME_OUTPUTS=0: ekfvio_step_image ends in the status word and the landmark count alone (read_status publishes them itself), and
   the getters launch their own kernels behind the frame.  Return codes, landmark counts, outputs and the whole state must equal the
   default's (outputs written by frame_outputs_kernel with the status word) bit for bit, frame by frame.
2. ekfvio_get_points on both sides of its one-workgroup limit: N = 256 is the single workgroup that publishes the host words itself,
   N = 257 the first grid that publishes through wait_status.
"""
import os

import numpy as np
import pytest
from PIL import Image

from ekf_vio_amd import EKFVIO, capi
from ekf_vio_amd.sim import Scenario, translated_sequence

pytestmark = pytest.mark.gpu
IMG = os.path.join(os.path.dirname(__file__), "golden", "images")
K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)
KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")


def grey(name="640_480_test"):
    return np.asarray(Image.open(os.path.join(IMG, name + "_gray.png")))


def cloud_of(feat_mu):
    """publishPoints' (u/rho, v/rho, 1/rho): the reciprocal in double, narrowed, then two float products (tests/test_gpu_loop.py)."""
    zinv = (1.0 / feat_mu[:, 2].astype(np.float64)).astype(np.float32)
    return np.stack([feat_mu[:, 0] * zinv, feat_mu[:, 1] * zinv, zinv], axis=1)


def fresh_landmarks(st):
    """Landmarks no update has measured yet: addNewFeatures leaves their cross-covariances exactly zero (TightlyCoupledEKF.cpp:58-94)."""
    S = st["Sigma"]
    n = S.shape[0]
    off = S - np.diag(np.diag(S))
    return sum(1 for j in range(22, n, 3) if not off[j:j + 3, :].any())


def run_frames(seq, **kw):
    v = EKFVIO(replenish=1, **kw)
    rows, added, removed = [], 0, 0
    for i, img in enumerate(seq):
        n_before = v.tc_ekf.num_features
        rc = v.addFrame(2.0 + i / 30.0, img, K)
        n_after = v.tc_ekf.num_features
        od = v.odometry()
        xyz, inten = v.points()
        st = v.tc_ekf.get_state()
        # in each run the outputs are the state's own numbers
        assert np.array_equal(od["position"], st["base_mu"][0:3]) and np.array_equal(od["orientation_wxyz"], st["base_mu"][3:7]), i
        assert xyz.shape == (n_after, 3) and np.array_equal(xyz, cloud_of(st["feat_mu"])), i
        if i > 0:
            # with cfg.remove_lost the frame's flagged landmarks are gone, so whatever is still unmeasured was added by this frame
            k_new = fresh_landmarks(st) if kw.get("remove_lost") else n_after - n_before
            added += k_new
            removed += n_before + k_new - n_after
        rows.append(dict(rc=rc, N=n_after, position=od["position"].copy(), orientation=od["orientation_wxyz"].copy(),
                         linear=od["linear"].copy(), angular=od["angular"].copy(), xyz=xyz.copy(), inten=inten.copy(), state=st))
    v.tc_ekf.close()
    return rows, added, removed


@pytest.mark.parametrize("max_features,remove_lost", [(48, 0), (48, 1), (160, 0)])
def test_status_word_only_frames_equal_the_default(monkeypatch, max_features, remove_lost):
    """Six frames of the motion that loses landmarks to the kill box (test_add_features_on_dense_sigma_device_count), once with the frame's
    outputs riding with its status word and once with EKFVIO_FRAME_OUTPUTS=0.

    What the CPU oracle (tests/_oracle_node.py, flagged landmarks compacted away behind each frame for remove_lost = 1) gave for this
    motion at 48 landmarks, as (landmarks before, added, flagged, landmarks after) per frame:
      remove_lost=0: (0,48,0,48) (48,0,2,48) (48,0,2,48) (48,0,4,48) (48,0,4,48) (48,0,5,48)
      remove_lost=1: (0,48,0,48) (48,0,2,46) (46,2,0,48) (48,0,2,46) (46,2,1,47) (47,1,1,47)
    With remove_lost = 1 later frames both remove and add.  With remove_lost = 0 the first frame fills all 48 slots and a flagged landmark
    keeps its slot (TightlyCoupledEKF.cpp:528), so NO motion makes a later frame add: there the sequence holds the full, non-replenishing
    frame (status word with no count behind it), and the case with 160 slots -- never full, as in tests/test_gpu_loop.py -- is the one
    that adds landmarks behind the first frame without a removal."""
    seq = translated_sequence(grey(), 6, dx=-6.0, dy=-2.5)
    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("EKFVIO_FRAME_OUTPUTS", mode)  # (Tuning is read in ekfvio_create)
        runs[mode] = run_frames(seq, max_features=max_features, remove_lost=remove_lost)
    (rows1, added1, removed1), (rows0, added0, removed0) = runs["1"], runs["0"]
    for i, (a, b) in enumerate(zip(rows1, rows0)):
        assert a["rc"] == b["rc"] and a["rc"] in (capi.OK, capi.ENUMERIC), (i, a["rc"], b["rc"])
        assert a["N"] == b["N"], (i, a["N"], b["N"])
        for k in ("position", "orientation", "linear", "angular", "xyz", "inten"):
            assert np.array_equal(a[k], b[k]), (i, k)
        for k in KEYS:
            assert np.array_equal(a["state"][k], b["state"][k]), (i, k)
    print("landmarks per frame:", [r["N"] for r in rows0], "added behind the first frame:", added0, "removed:", removed0)
    assert (added1, removed1) == (added0, removed0)
    if (max_features, remove_lost) == (48, 0):
        assert added0 == 0 and removed0 == 0 and all(r["N"] == 48 for r in rows0)  # full from the first frame on (docstring)
    else:
        assert added0 >= 1, "no frame behind the first added landmarks: the test does not exercise what it is named for"
    if remove_lost:
        assert removed0 >= 1, "no frame removed a landmark: the test does not exercise what it is named for"
    else:
        assert removed0 == 0


@pytest.mark.parametrize("N", [256, 257])
def test_get_points_on_both_sides_of_one_workgroup(N):
    """No frame pushed: points() must be the state's own cloud bit for bit, the intensity all zeros."""
    v = EKFVIO(max_features=257)
    v.tc_ekf.addNewFeatures(Scenario(N, seed=5).initial_features())
    assert v.tc_ekf.num_features == N
    xyz, inten = v.points()
    st = v.tc_ekf.get_state()
    assert xyz.shape == (N, 3) and np.array_equal(xyz, cloud_of(st["feat_mu"]))
    assert inten.shape == (N,) and not inten.any()
    v.tc_ekf.close()
