"""The innovation gate (ekfvio_set_gate / ekfvio_get_gate) on the device.

Not in the reference (its "OUTLIER DETECTION" thresholds are read by nothing).  include/ekfvio.h states the formula and its fp32
association order; `restate` below is that text in NumPy float32, and the device must give its bits.  A rejected landmark takes the
road of one the tracker failed, so a gated update must be, bit for bit, the update with the effective flags.

Inputs separate cleanly: on Scenario(N, seed=0, dt=0.05), on a state the oracle has warmed for two frames, the scenario's own
measurements have d2 <= 5.4e-4 and an offset of +0.05 on both coordinates gives d2 >= 0.074; the threshold of the tests is 0.01.
No case is excluded as too close to call.

Handles that are compared run one after the other, each as the device's only live handle.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
from PIL import Image

from ekf_vio_amd import EKFVIO, TightlyCoupledEKF, capi
from ekf_vio_amd.sim import Scenario
from oracle import OracleFilter

from _frame_twin import moving_object_sequence  # (the builder lives with the frame twin's sequence, which uses it too)

pytestmark = pytest.mark.gpu

CHI2 = 0.01
FLT_MAX = float(np.finfo(np.float32).max)
OFFSET = np.float32(0.05)
KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")
# the update's policy against the fp64 oracle: the constants of tests/test_gpu_parity.py
# (test_teacher_forced_process_bit_exact_and_update_within_fp64_yardstick, its later steps), copied, not new ones
ACC_FACTOR = 4.0
MU_FLOOR = 2e-5
SIG_FLOOR = 2e-6
IMG = os.path.join(os.path.dirname(__file__), "golden", "images")
K = np.array([500.0, 0, 320.0, 0, 500.0, 240.0, 0, 0, 1.0], np.float32)


def relf(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.size(a) else 0.0


@contextlib.contextmanager
def handle(N, **kw):
    g = TightlyCoupledEKF(max_features=N, **kw)
    try:
        yield g
    finally:
        g.close()


def assert_same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


@functools.lru_cache(maxsize=None)
def warmed(N, frames=1):
    """(dt, state of the fp32 oracle behind two teacher-forced frames, the `frames` measurements that follow)."""
    sc = Scenario(N, seed=0, dt=0.05)
    o = OracleFilter(np.float32)
    o.add_new_features(sc.initial_features())
    fr = list(sc.frames(2 + frames))
    for z, R, p in fr[:2]:
        o.process(sc.dt)
        o.update(z, R, p)
    st = o.get_state()
    o.close()
    return sc.dt, st, fr[2:]


def with_outliers(z, which):
    z = z.copy()
    z[which] += OFFSET
    return z


def restate(st, z, R, p, chi2, dtype=np.float32):
    """include/ekfvio.h, "innovation gate", line by line; st: the state behind process(dt).  Returns d2 (-1: not evaluated), accepted, and
    the terms of the fp64 bound."""
    f = dtype
    N = z.shape[0]
    mu = np.concatenate([st["base_mu"], st["feat_mu"].reshape(-1)]).astype(f)
    P = st["Sigma"].astype(f)  # [row, col]
    z, R = z.astype(f), R.astype(f)
    s = 22 + 3 * np.arange(N)
    with np.errstate(all="ignore"):
        y0 = z[:, 0] - mu[s]
        y1 = z[:, 1] - mu[s + 1]
        a = P[s, s] + R[:, 0]
        b = P[s + 1, s] + R[:, 1]  # the lower triangle's element of both
        c = P[s + 1, s + 1] + R[:, 3]
        det = a * c - b * b
        q = ((c * y0) * y0 - ((f(2) * b) * y0) * y1) + (a * y1) * y1
        d2 = q / det
        accept = (det > 0) & (d2 <= f(chi2))
    ev = np.asarray(p).astype(bool)
    amp = (np.abs(c) * y0 * y0 + 2 * np.abs(b * y0 * y1) + np.abs(a) * y1 * y1) / det + d2 * (a * c + b * b) / det
    return np.where(ev, d2, f(-1)), accept & ev, amp


def gate_case(N):
    """The case of tests 2 and 3: every fifth landmark an outlier, a few tracker failures."""
    dt, st, (fr,) = warmed(N)
    z, R, _ = fr
    out = np.zeros(N, bool)
    out[::5] = True
    p = np.ones(N, np.uint8)
    p[[i for i in (1, 7, 10, 33, 215, 640) if i < N]] = 0  # (10, 215, 640: failed outliers -- not evaluated)
    return dt, st, with_outliers(z, out), R, p, out


# ------------------------------------------------------------------ 2. d2 and verdicts, bit for bit
@pytest.mark.parametrize("N", [3, 64, 256, 1024])
def test_d2_and_verdicts_are_the_headers_formula_bit_for_bit(N):
    dt, st, z, R, p, out = gate_case(N)
    with handle(N) as g:
        assert g.gate()["n_landmarks"] == 0  # before the first gated update
        g.set_state(st)
        g.process(dt)
        sp = g.get_state()
        g.setGate(CHI2)
        assert g.updateWithFeaturePositions(z, R, p) in (capi.OK, capi.ENUMERIC)  # (a non-positive pivot at N = 1024: see one_update)
        got = g.gate()
        sg = g.get_state()
    d2, accept, _ = restate(sp, z, R, p, CHI2)
    ev = p.astype(bool)
    assert got["n_landmarks"] == N
    assert np.array_equal(got["d2"].view(np.uint32), d2.view(np.uint32)), np.nonzero(got["d2"] != d2)[0][:8]
    assert np.all(got["d2"][~ev] == -1)
    assert np.array_equal(got["gated"].astype(bool), ev & ~accept)
    # ... and the inputs separate as the module docstring says: the verdicts are the injected outliers, no more, no less
    assert np.array_equal(got["gated"].astype(bool), ev & out), (d2[ev & ~out].max(), d2[ev & out].min())
    assert got["gated_last"] == int((ev & out).sum()) == got["gated_total"] and got["gated_last"] > 0
    # the bookkeeping followed the effective flags (TightlyCoupledEKF.cpp:526-529)
    assert np.array_equal(sg["del_flag"].astype(bool), sp["del_flag"].astype(bool) | ~accept)
    assert np.array_equal(sg["last_klt"], np.where(accept[:, None], z, sp["last_klt"]))
    # against fp64 on the same fp32 inputs: q is at most six rounded operations deep, det four, the quotient one more
    d64, _, amp = restate(sp, z, R, p, CHI2, np.float64)
    err = np.abs(got["d2"].astype(np.float64) - d64)[ev]
    bound = (8 * 2.0 ** -24 * amp)[ev]
    print("N=%d: d2 inliers <= %.3g, outliers >= %.3g, fp32 error used %.3g of the bound" %
          (N, d2[ev & ~out].max(), d2[ev & out].min(), (err / bound).max()))
    assert np.all(err <= bound), (err / bound).max()


# ------------------------------------------------------------------ 3. the update behind the gate is the update with those flags
def one_update(N, mode, st, dt, z, R, p, chi2):
    with handle(N, predict_mode=mode) as g:  # (closed whatever happens: a handle left alive would take the persistent sweep from the next one)
        g.set_state(st)
        g.setGate(chi2)
        g.process(dt)
        sp = g.get_state()
        # (ENUMERIC: a non-positive pivot, carried along by the signed factorisation -- the fp32 sweep meets one on this young state from
        # N = 400 on, gate or no gate; the state is updated all the same, and the comparisons below hold it to the same standard)
        rc = g.updateWithFeaturePositions(z, R, p)
        assert rc in (capi.OK, capi.ENUMERIC)
        return sp, g.get_state(), g.gate(), dict(g.counters(), rc=rc)


@pytest.mark.parametrize("mode", [capi.PREDICT_STRUCTURED, capi.PREDICT_DENSE])
@pytest.mark.parametrize("N", [64, 256, 400, 1024])
def test_gated_update_is_the_update_with_the_effective_flags(N, mode):
    dt, st, z, R, p, out = gate_case(N)
    sp, sa, ga, ca = one_update(N, mode, st, dt, z, R, p, CHI2)
    gated = ga["gated"].astype(bool)
    assert gated.any() and np.array_equal(gated, p.astype(bool) & out)
    eff = (p.astype(bool) & ~gated).astype(np.uint8)
    spb, sb, gb, cb = one_update(N, mode, st, dt, z, R, eff, FLT_MAX)  # same plan: m = 2N, the count on the device
    assert gb["gated_last"] == 0
    assert_same(spb, sp, "propagated state")
    assert_same(sa, sb, ("twin with the effective flags", N, mode))
    assert ca == cb
    # ... and the fp64 oracle's update with those flags, by the yardstick of the teacher-forced parity test
    o32, o64 = OracleFilter(np.float32), OracleFilter(np.float64)
    o32.set_state(sp), o64.set_state(sp)
    o32.update(z, R, eff), o64.update(z, R, eff)
    s32, s64 = o32.get_state(), o64.get_state()
    o32.close(), o64.close()
    assert np.array_equal(sa["del_flag"], s32["del_flag"]) and np.array_equal(sa["last_klt"], s32["last_klt"])
    for key in ("base_mu", "feat_mu"):
        gap, yard = maxabs(sa[key], s64[key]), maxabs(s32[key], s64[key])
        assert gap <= ACC_FACTOR * yard + MU_FLOOR, (N, mode, key, gap, yard)
    if N <= 334:
        gap, yard = relf(sa["Sigma"], s64["Sigma"]), relf(s32["Sigma"], s64["Sigma"])
        print("N=%d mode=%d: Sigma against fp64 %.3g, the fp32 oracle %.3g" % (N, mode, gap, yard))
        assert gap <= ACC_FACTOR * yard + SIG_FLOOR, (N, mode, "Sigma", gap, yard)
        return
    # N > 334: the update's last GEMM forms the lower triangle's tiles and mirrors them (gemm.hip, GemmEpi::sym), and this start state is
    # the ORACLE's, which carries antisymmetric rounding noise.  The tolerance for exactly that situation is written down in
    # tests/test_gpu_shapes.py::test_symmetric_second_joseph_gemm_is_the_full_one_mirrored, copied here: the yardstick on the lower
    # triangle; on the upper triangle that plus the fp64 result's own antisymmetric part.
    S, S64, S32 = (x["Sigma"].astype(np.float64) for x in (sa, s64, s32))
    n = S.shape[0]
    lower = np.tril(np.ones((n, n), dtype=bool))
    upper = ~lower
    nrm = lambda M, msk: float(np.linalg.norm(M[msk]))  # noqa: E731
    print("N=%d mode=%d: lower %.3g against %.3g, upper %.3g, antisymmetric part of fp64 %.3g, norm %.3g" %
          (N, mode, nrm(S - S64, lower), nrm(S32 - S64, lower), nrm(S - S64, upper), nrm(S64 - S64.T, upper), nrm(S64, lower)))
    assert nrm(S - S64, lower) <= ACC_FACTOR * nrm(S32 - S64, lower) + SIG_FLOOR * nrm(S64, lower), (N, mode)
    assert nrm(S - S64, upper) <= nrm(S64 - S64.T, upper) + ACC_FACTOR * nrm(S32 - S64, lower) + SIG_FLOOR * nrm(S64, upper), (N, mode)


# ------------------------------------------------------------------ 4. nothing gated changes nothing
def free_run(N, fr, dt, chi2, st=None, steps=None):
    g = TightlyCoupledEKF(max_features=N)
    try:
        if st is None:
            g.addNewFeatures(Scenario(N, seed=0, dt=0.05).initial_features())
        else:
            g.set_state(st)
        if chi2:
            g.setGate(chi2)
        total = 0
        for z, R, p in fr[:steps]:
            g.process(dt)
            assert g.updateWithFeaturePositions(z, R, p) == capi.OK
            total += g.gate()["gated_last"]
    except BaseException:
        g.close()
        raise
    return g, total


@pytest.mark.parametrize("N", [100, 256])
def test_a_gate_that_rejects_nothing_changes_no_bit(N):
    sc = Scenario(N, seed=0, dt=0.05)
    fr = list(sc.frames(10))  # from the raw prior: all landmarks passed, nothing can exceed FLT_MAX
    a, total = free_run(N, fr, sc.dt, FLT_MAX)
    sa, ca, ga = a.get_state(), a.counters(), a.gate()
    a.close()
    b, _ = free_run(N, fr, sc.dt, 0.0)
    sb, cb, gb = b.get_state(), b.counters(), b.gate()
    b.close()
    assert gb["n_landmarks"] == 0  # a handle that never gated has nothing to report
    assert total == 0 and ga["gated_total"] == 0 and ga["n_landmarks"] == N and np.all(ga["d2"] >= 0)
    assert_same(sa, sb, "gate at FLT_MAX against gate off")
    assert ca == cb


def test_set_gate_zero_goes_back_to_the_ungated_launches():
    N = 128
    dt, st, fr = warmed(N, 7)
    out = np.zeros(N, bool)
    out[::5] = True
    gated_part = [(with_outliers(z, out), R, p) for z, R, p in fr[:3]]
    c, total = free_run(N, gated_part, dt, CHI2, st=st)
    assert total == 3 * int(out.sum())
    try:
        mid, c0 = c.get_state(), c.counters()
        c.setGate(0.0)
        for z, R, p in fr[3:]:
            c.process(dt)
            assert c.updateWithFeaturePositions(z, R, p) == capi.OK
        sc_, c1, gc = c.get_state(), c.counters(), c.gate()
    finally:
        c.close()
    assert gc["gated_total"] == total and gc["gated_last"] == int(out.sum())  # the last GATED update's results stay readable
    d, _ = free_run(N, fr[3:], dt, 0.0, st=mid)
    sd, d1 = d.get_state(), d.counters()
    d.close()
    assert_same(sc_, sd, "steps behind setGate(0) against a handle that never gated")
    for k in ("persistent", "schur", "recoveries", "t2_updates"):
        assert c1[k] - c0[k] == d1[k], (k, c0, c1, d1)
    assert c1["mode"] == d1["mode"]


def test_set_gate_refuses_what_is_not_a_threshold():
    g = TightlyCoupledEKF(max_features=8)
    for bad in (-1.0, float("nan")):
        assert g.lib.ekfvio_set_gate(g.h, bad) == capi.EINVAL
    g.setGate(3.0), g.setGate(0.0)
    g.close()


# ------------------------------------------------------------------ 5. device-resident runs
def per_call(N, st, dt, z, R, p, count, chi2):
    with handle(N) as g:
        g.set_state(st)
        g.setGate(chi2)
        lasts = []
        for i in range(count):
            g.process(dt)
            assert g.updateWithFeaturePositions(z[i], R[i], p[i]) == capi.OK
            lasts.append(g.gate()["gated_last"])
        return g.get_state(), lasts


def test_uploaded_runs_gate_on_the_device_and_leave_the_sequence_alone():
    N, F, count = 96, 20, 19  # 19 = two replays of the 8-step graph, one of the pair graph, one eager step
    dt, st, fr = warmed(N, F)
    z, R, p = (np.stack([f[i] for f in fr]) for i in range(3))
    assert p.all()
    rng = np.random.default_rng(5)
    n_out = {}
    for i in (0, 3, 4, 9, 17):  # outliers in z in some frames, elsewhere each time
        which = rng.choice(N, size=5 + i, replace=False)
        z[i, which] += OFFSET
        n_out[i] = len(which)
    ref1, lasts = per_call(N, st, dt, z, R, p, count, CHI2)
    assert lasts == [n_out.get(i, 0) for i in range(count)]
    ref2, lasts2 = per_call(N, st, dt, z, R, p, count, FLT_MAX)
    assert sum(lasts2) == 0
    with handle(N) as a:
        a.set_state(st)
        a.setGate(CHI2)
        a.upload_measurements(z, R, p)
        a.run_uploaded(0, count, dt)
        assert a.synchronize() == capi.OK
        s1, g1 = a.get_state(), a.gate()
        # another threshold between two runs: the steps are captured again and follow it.  Nothing is rejected now, so the outliers go into
        # the update -- which also shows that the first run left the uploaded pass flags alone
        a.set_state(st)
        a.setGate(FLT_MAX)
        a.run_uploaded(0, count, dt)
        assert a.synchronize() == capi.OK
        s2, g2 = a.get_state(), a.gate()
    assert_same(s1, ref1, "captured replay against process + updateWithFeaturePositions")
    assert g1["gated_total"] == sum(lasts) and g1["gated_last"] == lasts[-1]
    assert g2["gated_last"] == 0 and g2["gated_total"] == sum(lasts)
    assert_same(s2, ref2, "second run, gate at FLT_MAX")
    assert not np.array_equal(s1["Sigma"], s2["Sigma"])
    assert not s2["del_flag"].any() and s1["del_flag"].any()


# ------------------------------------------------------------------ 7. clustered rejections across sweeps
def test_clustered_rejections_give_the_same_bits_under_both_sweeps(monkeypatch):
    """A contiguous run of rejected landmarks plus scattered tracker failures: whole 64-row blocks of the measurement map shift, the shape
    ADVICE.md's finding on gain_tile2<true>'s waits describes.  The persistent sweep must give the per-step sweep's bits.  (It did on an
    idle MI355X before the finding was dealt with, too: a missing wait shows only when the producer is late.  tests/test_gpu_handoff_delay.py
    makes each owner late in turn, with this mask as its case C; that confirmed the finding, and gain_tile2<true> now looks at the flag of
    every row block it gathers from: profiles/handoff_delay.txt.)"""
    N = 256
    dt, st, (fr,) = warmed(N)
    z, R, _ = fr
    out = np.zeros(N, bool)
    out[100:150] = True
    rng = np.random.default_rng(11)
    p = np.ones(N, np.uint8)
    p[rng.choice(N, size=N // 5, replace=False)] = 0
    z = with_outliers(z, out)
    monkeypatch.setenv("EKFVIO_SCHUR", "0")  # the persistent sweep has no Schur tiles: compare like with like
    res = {}
    for mode in ("0", "2"):
        monkeypatch.setenv("EKFVIO_SWEEP", mode)  # (read when the handle is created)
        sp, s, g, c = one_update(N, capi.PREDICT_STRUCTURED, st, dt, z, R, p, CHI2)
        assert np.array_equal(g["gated"].astype(bool), p.astype(bool) & out)
        res[mode] = (s, c)
    assert res["2"][1]["persistent"] == 1 and res["0"][1]["persistent"] == 0, (res["0"][1], res["2"][1])
    assert_same(res["0"][0], res["2"][0], "EKFVIO_SWEEP=0 against EKFVIO_SWEEP=2")


# ------------------------------------------------------------------ 6. image loop
def grey(name="640_480_test"):
    return np.asarray(Image.open(os.path.join(IMG, name + "_gray.png")))


def test_image_loop_gates_a_moving_object_and_removes_it_in_the_same_frame():
    """ekfvio_step_image with the gate and remove_lost = 1 against a gated handle driven call by call (process, push_frame,
    findNewFeaturePositions, updateWithFeaturePositions, removeFeatures()) over the same frames: the same bits behind every frame.  The
    tracker follows the object's texture -- it passes those landmarks -- and the object moves by about (6.1, 2.3) pixels a frame against
    the filter's prediction, where the background's innovations are a fraction of a pixel: the threshold of the other tests lies between."""
    seq, (y0, y1, x0, x1), first, last = moving_object_sequence()
    stamps = [5.0 + i / 30.0 for i in range(len(seq))]
    rows = []
    a = EKFVIO(max_features=160, gate_chi2=CHI2, remove_lost=1)
    try:
        for i, img in enumerate(seq):
            n_before = a.tc_ekf.num_features
            assert a.addFrame(stamps[i], img, K) == capi.OK, i
            if i == 0:
                assert len(a.replenishFeatures()) > 40
            n_after = a.tc_ekf.num_features  # (from the frame's status word: no device work)
            st, od = a.tc_ekf.get_state(), a.odometry()
            assert st["feat_mu"].shape[0] == n_after and not st["del_flag"].any(), i
            assert np.array_equal(od["position"], st["base_mu"][0:3]), i
            rows.append((st, a.tc_ekf.gate(), n_before))
    finally:
        a.tc_ekf.close()
    b = EKFVIO(max_features=160, gate_chi2=CHI2)
    try:
        on_object = 0
        for i, img in enumerate(seq):
            if i == 0:
                assert b.addFrame(stamps[0], img, K) == capi.OK
                b.replenishFeatures()
            else:
                pre = b.tc_ekf.get_state()
                b.tc_ekf.process(float(np.float32(stamps[i] - stamps[i - 1])))
                b.tracker.push_frame(img, K)
                z, R, p = b.tracker.findNewFeaturePositions()
                assert b.tc_ekf.updateWithFeaturePositions(z, R, p) == capi.OK, i
                gb = b.tc_ekf.gate()
                flagged = b.tc_ekf.get_state()["del_flag"].astype(bool)
                assert np.array_equal(flagged, ~p.astype(bool) | gb["gated"].astype(bool)), i
                assert b.tc_ekf.removeFeatures() == int(flagged.sum()), i
                sa, ga, n_before = rows[i]
                assert n_before == len(p) == ga["n_landmarks"], i
                assert np.array_equal(ga["gated"], gb["gated"]) and np.array_equal(ga["d2"].view(np.uint32), gb["d2"].view(np.uint32)), i
                assert ga["gated_last"] == gb["gated_last"] and ga["gated_total"] == gb["gated_total"], i
                if i == first:  # the object appears: the landmarks well inside it were tracked onto it, gated, and are gone
                    px = pre["last_klt"] * np.array([K[0], K[4]], np.float32)
                    inside = (px[:, 0] >= x0 + 30) & (px[:, 0] < x1 - 30) & (px[:, 1] >= y0 + 30) & (px[:, 1] < y1 - 30) & p.astype(bool)
                    on_object = int(inside.sum())
                    assert np.all(gb["gated"][inside] == 1), gb["d2"][inside]
                    assert rows[i][0]["feat_mu"].shape[0] <= n_before - on_object
                if i < first:
                    assert gb["gated_last"] == 0, (i, gb["d2"].max())
            assert_same(rows[i][0], b.tc_ekf.get_state(), ("frame", i))
        assert on_object > 0, "no landmark on the object passed the tracker: the sequence does not exercise the gate"
    finally:
        b.tc_ekf.close()
