"""What the frame twin's sequence (tests/_frame_twin.py) is worth, checked without a GPU: the segments are where the module says, the CPU
oracle's node loses and replenishes landmarks on the plain sequence whatever the new stages do, and the two host-side lines of the
call-by-call path -- the zero-velocity decision's reference pixel and the IMU records' process(dt) arguments -- are the specification's."""
import numpy as np
import pytest

import _equalize as eq
import _frame_twin as T
import _klt_fb as fb
from _oracle_node import OracleNode
from ekf_vio_amd.sim import translated_sequence


def test_sequence_is_deterministic_and_its_segments_are_where_the_module_says():
    T.sequence.cache_clear()
    first = T.sequence().copy()
    T.sequence.cache_clear()
    seq = T.sequence()
    assert seq.dtype == np.uint8 and seq.shape == (T.FRAMES, 480, 640) and seq.tobytes() == first.tobytes() and not seq.flags.writeable
    base = fb.image("first")
    tr = translated_sequence(base, T.MOVING_STEPS + 1, dx=T.DX, dy=T.DY)
    steps = T.moving_steps()
    assert len(steps) == len(T.MOVING) and 0 < steps[0] < 1 and steps[1:] == tuple(range(1, T.MOVING_STEPS + 1))
    for k in range(1, T.MOVING_STEPS + 1):  # a whole step is translated_sequence's frame
        assert T.plane(k).tobytes() == tr[k].tobytes()
    assert sorted(T.STILL + T.MOVING + (T.END[1],)) == list(range(T.FRAMES)) and T.END[0] == T.MOVING[-1]
    assert T.SHORT > T.BLOCK > T.FLICKER > T.MOVING[0] > T.STILL[-1] and T.OBJECT[0] == T.SHORT
    for i in T.STILL:  # "identical" is byte-identical
        assert seq[i].tobytes() == base.tobytes()
    assert seq[T.END[0]].tobytes() == seq[T.END[1]].tobytes() == tr[T.MOVING_STEPS].tobytes()
    y0, y1, x0, x1 = T.OBJECT_BOX
    bx0, by0, bx1, by1 = fb.BLOCK
    for i in T.MOVING:
        want = T.plane(steps[i - T.MOVING[0]])
        assert not np.array_equal(want, base if i == T.MOVING[0] else T.plane(steps[i - T.MOVING[0] - 1]))
        if i == T.FLICKER:
            assert np.array_equal(seq[i], eq.contrast(want, 0.8, 0)) and not np.array_equal(seq[i], want)
        elif i == T.BLOCK:
            outside = np.ones((480, 640), bool)
            outside[by0:by1, bx0:bx1] = False
            assert np.array_equal(seq[i][outside], want[outside])
            assert np.array_equal(seq[i][by0:by1, bx0:bx1], fb.image("blocked_identical")[by0:by1, bx0:bx1])
            assert not np.array_equal(seq[i][by0:by1, bx0:bx1], want[by0:by1, bx0:bx1])
        elif i in T.OBJECT:
            j = i - T.OBJECT[0] + 1
            outside = np.ones((480, 640), bool)
            outside[y0 + j:y1 + j, x0 + 3 * j:x1 + 3 * j] = False
            assert np.array_equal(seq[i][outside], want[outside])
            assert np.array_equal(seq[i][y0 + j:y1 + j, x0 + 3 * j:x1 + 3 * j], T.plane(steps[T.OBJECT[0] - 1 - T.MOVING[0]])[y0:y1, x0:x1])
        else:
            assert np.array_equal(seq[i], want)


def test_moving_object_builder_is_the_gate_tests_sequence():
    seq, box, first, last = T.moving_object_sequence()
    plain = translated_sequence(fb.image("first"), 24, dx=-3.1, dy=-1.3)
    assert (len(seq), box, first, last) == (24, (160, 320, 240, 400), 12, 17)
    for i in range(24):
        assert np.array_equal(seq[i], plain[i]) == (not first <= i <= last), i
    assert np.array_equal(seq[14][163:323, 249:409], plain[11][160:320, 240:400])


def test_settings_by_name():
    every = T.settings()
    subs = T.subsets()
    assert len(T.SINGLE) == 10 and len(T.PAIRS) == 3 and set(subs) == {"everything"} | set(T.SINGLE) | set(T.PAIRS)
    assert set(subs["everything"]) == set(every)
    used = set()
    for name in list(T.SINGLE) + list(T.PAIRS):
        s = subs[name]
        assert s["replenish"] == 1 and s["remove_lost"] == 1 and s["fast_threshold"] == 20 and s["min_new_feature_dist"] == 12
        used |= set(s)
    assert used == set(every)  # no setting of "everything" without a case of its own
    assert every["zupt"] == (0.25, 8, 0.75, 1e-4, 1e-4) and every["klt_fb_max_px"] == 0.5 and every["replenish_grid"] == (8, 6)
    assert T.subsets(333, 251)["everything"]["mask"].shape == (251, 333)


def compact(st, flags):
    """The state without the flagged landmarks (rows and columns of Sigma, order kept)."""
    keep = ~flags
    rows = np.concatenate([np.ones(22, bool), np.repeat(keep, 3)])
    return dict(base_mu=st["base_mu"], feat_mu=st["feat_mu"][keep], last_klt=st["last_klt"][keep], del_flag=st["del_flag"][keep],
                Sigma=st["Sigma"][np.ix_(rows, rows)])


@pytest.mark.parametrize("max_features", [64, 96])
def test_oracle_node_loses_and_replenishes_on_the_plain_sequence(max_features):
    """No lens, no mask, no gate, no forward-backward check, no zero-velocity update: the reference's node with the detector parameters of
    the GPU cases and a removal of the flagged landmarks behind every frame.  The removal and replenishment conditions of the GPU test
    therefore do not hang on a setting's side effect."""
    node = OracleNode(max_features, T.K, **T.DETECTOR)
    lost = added_later = 0
    for i, (stamp, img) in enumerate(zip(T.stamps(), T.sequence())):
        node.add_frame(stamp, img)
        if i > 0:
            p = node.last["passed"]
            added_later += len(node.last["new_px"])
            if i in T.STILL or i == T.END[1]:
                assert int(p.sum()) >= T.ZUPT[1], (i, int(p.sum()))
        st = node.ekf.get_state()
        flags = st["del_flag"].astype(bool)
        lost += int(flags.sum())
        if flags.any():
            node.ekf.set_state(compact(st, flags))
    print("oracle node, max_features %d: lost %d, replenished behind frame 0 %d" % (max_features, lost, added_later))
    assert lost >= 1, "no landmark is lost: the plain sequence does not exercise the removal"
    assert added_later >= 1, "no landmark is added behind frame 0: the plain sequence does not exercise the replenishment"


def test_reference_pixel_line_is_the_oracle_nodes_and_the_headers_with_P_over_s():
    rng = np.random.default_rng(3)
    lk = rng.uniform(-0.8, 0.8, (97, 2)).astype(np.float32)
    node = OracleNode(8, T.K)
    assert T.reference_pixels(lk, T.frame_intrinsics(T.K)).tobytes() == node._px(lk).tobytes()
    node2 = OracleNode(8, T.K, inverse_image_scale=2)
    assert T.reference_pixels(lk, T.frame_intrinsics(T.K, None, 2)).tobytes() == node2._px(lk).tobytes()
    # with P the frame's intrinsics are P's, divided by s in double and narrowed (include/ekfvio.h, ekfvio_set_camera_model), the
    # principal point only where the configuration uses it; the pixel is multiply, then add, each rounded to fp32
    P = T.settings()["camera_model"][2]  # (fx', cx', fy', cy')
    for s in (1, 2, 3):
        for upp in (False, True):
            fx, fy, cx, cy = T.frame_intrinsics(T.K, P, s, upp)
            assert fx == np.float32(np.float64(P[0]) / s) and fy == np.float32(np.float64(P[2]) / s)
            assert (cx, cy) == ((np.float32(np.float64(P[1]) / s), np.float32(np.float64(P[3]) / s)) if upp else (0, 0))
            got = T.reference_pixels(lk, (fx, fy, cx, cy))
            for i in (0, 50, 96):
                assert got[i, 0] == np.float32(np.float32(lk[i, 0] * fx) + cx) and got[i, 1] == np.float32(np.float32(lk[i, 1] * fy) + cy)
            exact = lk.astype(np.float64) * [fx, fy] + [cx, cy]
            assert np.abs(got - exact).max() <= 2 * 2.0 ** -24 * np.abs(exact).max()  # two roundings, nothing fused or reordered


def test_imu_split_reproduces_the_fused_paths_float_dt():
    """ekfvio_imu and ekfvio_step_image form (float)(stamp - t_stamp) with t_stamp a double that takes each stamp in turn."""
    clock = T.stamps()[0]
    for i in range(1, T.FRAMES):
        rec, frame = T.imu_stamps(i), T.stamps()[i]
        assert len(rec) == T.IMU_PER_FRAME and all(a < b for a, b in zip([clock] + rec, rec + [frame]))
        dts, dt_frame = T.imu_split(rec, frame, clock)
        t = float(clock)
        for s, dt in zip(rec + [frame], dts + [dt_frame]):
            assert dt.dtype == np.float32 and dt == np.float32(float(s) - t) and dt > 0
            t = float(s)
        assert abs(sum(float(d) for d in dts) + float(dt_frame) - (frame - clock)) < 1e-7
        clock = frame


def test_compare_names_the_frame_the_array_and_the_first_differing_element():
    def row(v):
        return {"state.Sigma": np.full((3, 3), v, np.float32), "gate.counts": np.array([1, 2, 3], np.int64), "_counters": {"recoveries": 0}}

    a, b = [row(1.0), row(2.0)], [row(1.0), row(2.0)]
    T.compare(a, b, "same")
    b[1]["state.Sigma"][2, 1] = np.nextafter(np.float32(2.0), np.float32(3.0))  # one bit
    with pytest.raises(AssertionError, match=r"case frame 1, state\.Sigma: 1 of 9 elements differ, the first at \(2, 1\)"):
        T.compare(a, b, "case")
    b = [row(1.0), dict(row(2.0), **{"gate.counts": np.array([1, 2], np.int64)})]
    with pytest.raises(AssertionError, match=r"frame 1, gate\.counts: shapes \(3,\) \(fused\) and \(2,\)"):
        T.compare(a, b, "case")
    # -0.0 and 0.0 are different bits; an aborted sweep in either loop is named in the message
    b = [row(1.0), row(2.0)]
    a[0]["state.Sigma"][0, 0], b[0]["state.Sigma"][0, 0] = 0.0, -0.0
    b[1]["_counters"]["recoveries"] = 1
    with pytest.raises(AssertionError, match=r"frame 0, state\.Sigma: .*aborted and re-run in this loop \(recoveries: fused 0, call by call 1\)"):
        T.compare(a, b, "case")
