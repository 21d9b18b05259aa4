"""The frame loop with every setting on: the bits of the call-by-call path (tests/_frame_twin.py).

ekfvio_step_image with rectification (rational lens onto a camera P), equalisation, the no-data mask, the photometric term, the
forward-backward check, the zero-velocity update, the gate, the grid replenishment, the removal with the ended-track export, the in-frame
covariances and the IMU -- against a second handle on which each of those stages is a call of the public C-ABI in the order of
csrc/frame.hip: everything a node can read behind every frame, bit for bit, no tolerance.  Then the same with one setting at a time and
with three pairs that share state, so that a red "everything" is located by the cases that stay green.

Each test is at most thirteen 640 x 480 frames on two small handles, one after the other.
"""
import numpy as np
import pytest

import _frame_twin as T
import test_gpu_gate as G

pytestmark = pytest.mark.gpu

# what an "everything" run must make the stages do, each at least once (the counts of T.exercised)
MUST = ("zupt applied (frames)", "zupt refused with n_pass >= min_tracks (frames)", "gated (landmarks)",
        "forward-backward rejected (landmarks)", "masked (landmarks)", "removed (landmarks)", "replenished behind frame 0 (landmarks)",
        "frames with a removal and a replenishment", "ended records")


def run(name, settings, seq, max_features, **kw):
    a = T.fused(seq, settings, max_features, **kw)
    b = T.call_by_call(seq, settings, max_features, **kw)
    counts = T.exercised(b)
    print("\nFRAME-TWIN %s, max_features %d:" % (name, max_features))
    for k, n in counts.items():
        print("    %-50s %d" % (k, n))
    print("    landmarks per frame:", [len(r["landmark_ids"]) for r in b])
    T.compare(a, b, name)
    return counts


def test_the_gate_threshold_is_the_gate_tests():
    assert T.GATE_CHI2 == G.CHI2


@pytest.mark.parametrize("max_features", [64, 96], ids=["one-workgroup", "two-workgroups"])
def test_everything(max_features):
    """max_features = 64: n <= 214, one workgroup in the IMU / zero-velocity gain kernels; 96: n reaches 310 > 256, two workgroups, and
    the removal works above one 256-row block.  The sequence must exercise every stage (MUST).  Measured on an MI355X, at 64 / 96: the
    zero-velocity update applied in 4 / 4 frames (1, 2, 3 and 12) and refused with enough tracks in 8 / 8; 284 / 427 landmarks rejected by
    the gate, 15 / 20 by the forward-backward check, 3 / 3 by the mask; 306 / 455 removed, as many replenished behind frame 0 and as many
    ended records; 8 / 8 frames that both remove and replenish.  Landmarks behind each frame: 64, 64, 64, 14, 50, 14, 50, 14, 50, 14, 50,
    14, 64 and 96, 96, 96, 25, 71, 25, 71, 25, 71, 25, 71, 25, 96 -- behind three still frames the filter is sure it stands still, and
    at the gate tests' threshold it rejects most of what then moves, frame after frame (tests/_frame_twin.py, FIRST_STEP)."""
    counts = run("everything", T.subsets()["everything"], T.sequence(), max_features)
    for k in MUST:
        assert counts[k] >= 1, "the sequence does not exercise: " + k
    if max_features == 96:
        assert 22 + 3 * counts["largest landmark count"] > 256, counts


def test_everything_at_inverse_image_scale_2():
    """P / s in the zero-velocity reference pixel, the mask's s-block OR, the detector on the 320 x 240 level."""
    run("everything, inverse_image_scale = 2", T.subsets()["everything"], T.sequence(), 64, scale=2)


def test_everything_on_a_strided_odd_crop():
    """251 rows of 333 pixels pushed with a stride of 352: tile edges of rectification, equalisation, mask and pyramid that are no
    multiple of 4, 32 or 64, and slack bytes that are no image."""
    seq = T.sequence()[:, :251, :333]
    run("everything on a strided odd crop", T.subsets(333, 251)["everything"], seq, 32, stride=352)


@pytest.mark.parametrize("name", list(T.SINGLE) + list(T.PAIRS))
def test_one_setting_or_one_pair(name):
    """The "everything" run cut to eight frames (still, moving, flicker, block) with one setting, or one pair of settings that share state,
    plus replenish = 1 and remove_lost = 1."""
    run(name, T.subsets()[name], T.sequence()[:T.SHORT], 64)
