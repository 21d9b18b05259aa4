"""One owner for a handle's device and pinned memory (ekf_vio_amd/csrc/mem.h), on the device: what a handle holds, that a grown frame
replaces its buffers, that the lazily allocated blocks are one allocation made once, that the per-frame paths allocate nothing, that the test
hooks and every failed call leave nothing behind.  The counts come from ekfvio_test_mem, the failures from ekfvio_test_mem_fail: an injected
out-of-memory that never reaches the runtime (no test here allocates much, let alone until the device runs out).

Shapes: max_features = 8 and 160 x 120 frames unless a case needs more (the graph path of the device-resident run and the persistent sweep
want 96 landmarks); the ledger cannot go wrong differently at the workload's sizes.
"""
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest

from ekf_vio_amd import EKFVIO, TightlyCoupledEKF, capi
from ekf_vio_amd.sim import Scenario, translated_sequence

pytestmark = pytest.mark.gpu

W, H = 160, 120
BIG_W, BIG_H = 192, 144
K = np.array([100.0, 0, W / 2, 0, 100.0, H / 2, 0, 0, 1.0], np.float32)
KEYS = ("base_mu", "feat_mu", "last_klt", "del_flag", "Sigma")
# ekfvio_test_mem's words
DEV_LIVE, DEV_BYTES, PIN_LIVE, PIN_BYTES, DEV_ACQ, DEV_REL, PIN_ACQ, PIN_REL = range(8)
LIVE = [DEV_LIVE, DEV_BYTES, PIN_LIVE, PIN_BYTES]


@pytest.fixture(autouse=True)
def no_garbage_handles():
    gc.collect()  # a handle some earlier test dropped without close() must not be destroyed in the middle of a count


def lib():
    return capi.load(hooks=True)


def mem(h=None):
    """ekfvio_test_mem of a handle (a TightlyCoupledEKF, a raw pointer) or, with None, of the whole hooks library."""
    out = (C.c_int64 * 8)()
    assert lib().ekfvio_test_mem(getattr(h, "h", h), out) == capi.OK
    m = np.array(list(out), np.int64)
    assert m[DEV_LIVE] == m[DEV_ACQ] - m[DEV_REL] and m[PIN_LIVE] == m[PIN_ACQ] - m[PIN_REL], m
    return m


def fail_nth(h, k):
    assert lib().ekfvio_test_mem_fail(getattr(h, "h", h), int(k)) == capi.OK


def image(w, h):
    """A textured w x h crop of the golden test frame: corners for FAST, texture for the tracker."""
    from PIL import Image
    full = np.asarray(Image.open(os.path.join(os.path.dirname(__file__), "golden", "images", "640_480_test_gray.png")))
    return np.ascontiguousarray(full[120:120 + h, 160:160 + w])


def small(max_features=8, w=W, h=H, **kw):
    return EKFVIO(hooks=True, max_features=max_features, max_image_width=w, max_image_height=h, **kw)


def pyramid(v):
    """Every level of the current frame, as ekfvio_klt_get_level hands it out."""
    out = []
    for l in range(int(v.tc_ekf.cfg.klt_max_pyramid_level) + 1):
        w, h = C.c_int32(0), C.c_int32(0)
        if v.tc_ekf.lib.ekfvio_klt_get_level(v.tc_ekf.h, l, C.byref(w), C.byref(h), None, None) != capi.OK:
            break
        out.append(v.tracker.level(l))
    assert len(out) >= 2
    return out


def same_pyramid(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def clean_grow():
    """A 192 x 144 frame pushed into a handle configured for 160 x 120, and into one configured for 192 x 144 from the start: the counts
    before and after, the pyramids.  Shared by the grow cases (computed once, never modified)."""
    img = image(BIG_W, BIG_H)
    v = small()
    before = mem(v.tc_ekf)
    v.tracker.push_frame(img, K)
    after = mem(v.tc_ekf)
    grown = pyramid(v)
    v.tc_ekf.close()
    ref = small(w=BIG_W, h=BIG_H)
    ref.tracker.push_frame(img, K)
    want = pyramid(ref)
    ref.tc_ekf.close()
    return dict(before=before, after=after, grown=grown, want=want, img=img)


def test_two_handles_hold_the_same_and_destroy_returns_everything():
    base = mem()
    a = small()
    one = mem()
    b = small()
    ma, mb = mem(a.tc_ekf), mem(b.tc_ekf)
    assert ma[DEV_LIVE] > 40 and ma[PIN_LIVE] == 4, ma  # h_info, h_out, h_meas, h_image
    assert np.array_equal(ma[LIVE], mb[LIVE]), (ma, mb)
    assert np.array_equal((one - base)[LIVE], ma[LIVE])  # the library's totals rose by what the handle says it holds
    b.tc_ekf.close()
    assert np.array_equal(mem()[LIVE], one[LIVE])  # ... and are back to what they were before its create
    a.tc_ekf.close()
    assert np.array_equal(mem()[LIVE], base[LIVE])


def test_a_grown_frame_replaces_its_buffers_and_never_adds_to_them():
    g = clean_grow()
    before, after = g["before"], g["after"]
    assert after[DEV_LIVE] == before[DEV_LIVE] and after[PIN_LIVE] == before[PIN_LIVE]
    assert after[DEV_BYTES] > before[DEV_BYTES] and after[PIN_BYTES] > before[PIN_BYTES]
    d = after - before
    assert d[DEV_ACQ] == d[DEV_REL] > 0 and d[PIN_ACQ] == d[PIN_REL] == 1, d  # staging, one frame's planes, the detector's buffers; h_image
    assert g["grown"][0][0].shape == (BIG_H, BIG_W) and np.array_equal(g["grown"][0][0], g["img"])
    assert same_pyramid(g["grown"], g["want"])


def test_lazy_blocks_are_one_allocation_made_once():
    a, b = image(W, H), np.ascontiguousarray(np.roll(image(W, H), (1, -2), axis=(0, 1)))
    v = small()
    t = v.tc_ekf
    t.addNewFeatures(np.array([[x / 100.0, y / 100.0] for x, y in ((40, 40), (80, 60), (120, 80), (60, 90))], np.float32))
    v.tracker.push_frame(a, K)
    v.tracker.push_frame(b, K)
    v.tracker.findNewFeaturePositions()  # (a track without the check: nothing)
    m0 = mem(t)

    def step(what, dev):
        nonlocal m0
        m1 = mem(t)
        assert m1[DEV_LIVE] - m0[DEV_LIVE] == dev and m1[PIN_LIVE] == m0[PIN_LIVE] and m1[DEV_REL] == m0[DEV_REL], (what, m0, m1)
        m0 = m1

    step("track, check off", 0)
    t.setGate(9.0)
    step("first ekfvio_set_gate > 0", 1)
    t.setGate(16.0)
    t.setGate(0.0)
    t.setGate(9.0)
    step("ekfvio_set_gate again", 0)
    t.setKltFb(1.0)
    step("ekfvio_set_klt_fb alone", 0)
    v.tracker.findNewFeaturePositions()
    step("first checked track", 1)
    v.tracker.findNewFeaturePositions()
    step("second checked track", 0)
    t.setDistortion([0.05, 0.0, 0.0, 0.0])
    step("ekfvio_set_distortion alone", 0)
    v.tracker.push_frame(a, K)
    step("first frame with distortion", 3)
    v.tracker.push_frame(b, K)
    step("second frame with distortion", 0)
    assert t.lib.ekfvio_test_sweep_stamps(t.h, 1, None) == capi.OK
    step("ekfvio_test_sweep_stamps(enable)", 1)
    assert t.lib.ekfvio_test_sweep_stamps(t.h, 1, None) == capi.OK
    step("ekfvio_test_sweep_stamps again", 0)
    base = mem()
    t.close()
    assert np.array_equal((base - mem())[LIVE], m0[LIVE])  # destroy released the lazy blocks with the rest


def uploaded(N, frames, seed=5, cap=None, hooks=True):
    sc = Scenario(N, seed=seed)
    g = TightlyCoupledEKF(max_features=cap or N, hooks=hooks)
    g.addNewFeatures(sc.initial_features())
    fr = list(sc.frames(frames))
    return g, sc.dt, np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), np.stack([f[2] for f in fr])


def test_an_upload_is_three_allocations_and_the_next_one_replaces_them():
    g, dt, z, R, p = uploaded(8, 6)
    m0 = mem(g)
    g.upload_measurements(z[:4], R[:4], p[:4])
    m1 = mem(g)
    assert m1[DEV_LIVE] == m0[DEV_LIVE] + 3 and m1[PIN_LIVE] == m0[PIN_LIVE]
    g.upload_measurements(z, R, p)  # another frame count
    m2 = mem(g)
    assert m2[DEV_LIVE] == m1[DEV_LIVE] and m2[DEV_BYTES] > m1[DEV_BYTES] and m2[DEV_ACQ] - m1[DEV_ACQ] == m2[DEV_REL] - m1[DEV_REL] == 3
    g.close()


def test_the_per_frame_paths_allocate_nothing():
    # ekfvio_process + ekfvio_update
    g, dt, z, R, p = uploaded(8, 21)
    g.process(dt)
    g.updateWithFeaturePositions(z[0], R[0], p[0])
    m0, all0 = mem(g), mem()
    for i in range(1, 21):
        g.process(dt)
        assert g.updateWithFeaturePositions(z[i], R[i], p[i]) in (capi.OK, capi.ENUMERIC)
    assert np.array_equal(mem(g), m0) and np.array_equal(mem(), all0)
    g.close()
    # ekfvio_step_image with replenishment on
    seq = translated_sequence(image(W, H), 21)
    v = small(replenish=1, fast_threshold=20)
    v.addFrame(1.0, seq[0], K)
    assert v.tc_ekf.num_features > 0
    m0, all0 = mem(v.tc_ekf), mem()
    for i in range(1, 21):
        v.addFrame(1.0 + i / 30.0, seq[i], K)
    assert np.array_equal(mem(v.tc_ekf), m0) and np.array_equal(mem(), all0)
    v.tc_ekf.close()
    # ekfvio_run_uploaded where its graphs engage (N = 96: tests/test_gpu_resident_run.py)
    g, dt, z, R, p = uploaded(96, 8)
    g.upload_measurements(z, R, p)
    g.run_uploaded(0, 40, dt)  # (captures)
    g.synchronize()
    m0, all0, c0 = mem(g), mem(), g.counters()
    g.run_uploaded(0, 40, dt)
    g.synchronize()
    assert g.counters()["graph_steps"] == c0["graph_steps"] + 40
    assert np.array_equal(mem(g), m0) and np.array_equal(mem(), all0)
    g.close()


def run_scratch_hooks(g):
    rng = np.random.default_rng(11)
    A, B = rng.standard_normal((64, 64)).astype(np.float32), rng.standard_normal((64, 64)).astype(np.float32)
    got = g.test_gemm(A, B, np.zeros((64, 64), np.float32))
    assert np.allclose(got, A @ B.T, rtol=1e-4, atol=1e-3)
    stamps = (C.c_int64 * 80)()
    assert g.lib.ekfvio_test_potrf_stamps(g.h, stamps) == capi.OK
    S = (A @ A.T + 64 * np.eye(64)).astype(np.float32)
    L, X, info = g.test_cholesky_solve(S, B)
    assert info == 0 and np.allclose(X @ S, B, rtol=1e-3, atol=1e-3)


def test_the_hooks_leave_nothing_behind():
    g = TightlyCoupledEKF(max_features=8, hooks=True)
    m0, all0 = mem(g), mem()
    run_scratch_hooks(g)
    assert np.array_equal(mem(g), m0) and np.array_equal(mem()[LIVE], all0[LIVE])
    assert mem()[DEV_ACQ] - all0[DEV_ACQ] == mem()[DEV_REL] - all0[DEV_REL] == 3 + 4 + 5  # their scratch came and went through ledgers of their own
    # the handle's own acquisitions fail: the scratch hooks are not the handle's (the armed failure waits), the hook that does acquire on the
    # handle returns the error, and the counts balance
    fail_nth(g, 1)
    run_scratch_hooks(g)
    assert np.array_equal(mem(g), m0) and np.array_equal(mem()[LIVE], all0[LIVE])
    assert g.lib.ekfvio_test_sweep_stamps(g.h, 1, None) == capi.EDEVICE
    assert g.lib.ekfvio_set_gate(g.h, 9.0) == capi.OK and mem(g)[DEV_LIVE] == m0[DEV_LIVE] + 1  # (the injection fires once)
    fail_nth(g, 1)
    assert g.lib.ekfvio_test_sweep_stamps(g.h, 1, None) == capi.EDEVICE
    assert mem(g)[DEV_LIVE] == m0[DEV_LIVE] + 1 and mem()[DEV_LIVE] == all0[DEV_LIVE] + 1
    assert g.lib.ekfvio_test_sweep_stamps(g.h, 1, None) == capi.OK and mem(g)[DEV_LIVE] == m0[DEV_LIVE] + 2
    g.close()
    assert np.array_equal(mem()[LIVE], (all0 - m0)[LIVE])


def test_a_failed_upload_cannot_be_run():
    g, dt, z, R, p = uploaded(8, 4)
    none = mem(g)
    g.upload_measurements(z, R, p)
    fail_nth(g, 2)
    assert g.lib.ekfvio_upload_measurements(g.h, 4, z.ctypes.data_as(C.POINTER(C.c_float)), R.ctypes.data_as(C.POINTER(C.c_float)),
                                            p.ctypes.data_as(C.POINTER(C.c_uint8))) == capi.EDEVICE
    assert np.array_equal(mem(g)[LIVE], none[LIVE])  # no sequence allocation is live
    c0 = g.counters()
    assert g.lib.ekfvio_run_uploaded(g.h, 0, 4, C.c_float(dt)) == capi.EINVAL
    assert g.counters() == c0  # nothing was enqueued
    g.upload_measurements(z, R, p)
    g.run_uploaded(0, 4, dt)
    rc = g.synchronize()
    got = g.get_state()
    g.close()
    f, dt, z, R, p = uploaded(8, 4)
    f.upload_measurements(z, R, p)
    f.run_uploaded(0, 4, dt)
    assert f.synchronize() == rc
    want = f.get_state()
    f.close()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k


def test_a_failed_grow_leaves_a_usable_handle():
    g = clean_grow()
    d = g["after"] - g["before"]
    A = int(d[DEV_ACQ] + d[PIN_ACQ])  # acquisitions of one 192 x 144 push into a 160 x 120 handle
    assert A > 2
    for k in range(1, A + 1):
        v = small()
        fail_nth(v.tc_ekf, k)
        with pytest.raises(capi.EkfvioError) as e:
            v.tracker.push_frame(g["img"], K)
        assert e.value.code == capi.EDEVICE, k
        v.tracker.push_frame(g["img"], K)
        assert same_pyramid(pyramid(v), g["want"]), k
        assert np.array_equal(mem(v.tc_ekf)[LIVE], g["after"][LIVE]), k
        v.tc_ekf.close()
    # ... and the injection was what failed every time: one more would not have been reached
    v = small()
    fail_nth(v.tc_ekf, A + 1)
    v.tracker.push_frame(g["img"], K)
    v.tc_ekf.close()


def one_step(N=96):
    g, dt, z, R, p = uploaded(N, 1)
    g.process(dt)
    rc = g.updateWithFeaturePositions(z[0], R[0], p[0])
    st, c = g.get_state(), g.counters()
    g.close()
    return rc, st, c


def test_a_failed_create_leaves_nothing():
    before_loop = one_step()
    assert before_loop[2]["persistent"] == 1  # a device's sole handle takes the persistent sweep
    v = small()
    m = mem(v.tc_ekf)
    created = int(m[DEV_ACQ] + m[PIN_ACQ])  # acquisitions of one successful create
    cfg = v.tc_ekf.cfg
    v.tc_ekf.close()
    assert created > 40
    base = mem()
    for k in range(1, created + 1):
        fail_nth(None, k)
        h = C.c_void_p(0xdead)
        rc = lib().ekfvio_create(C.byref(cfg), 0, None, C.byref(h))
        assert rc == capi.EDEVICE and not h.value, k
        assert np.array_equal(mem()[LIVE], base[LIVE]), k
    fail_nth(None, created + 1)  # (one more than a create makes: it succeeds)
    h = C.c_void_p()
    assert lib().ekfvio_create(C.byref(cfg), 0, None, C.byref(h)) == capi.OK and h.value
    assert lib().ekfvio_destroy(h) == capi.OK
    assert np.array_equal(mem()[LIVE], base[LIVE])
    # the live-handle registry came back to balance: the next handle is its device's sole one again, and computes what it computed before
    rc, st, c = one_step()
    assert c["persistent"] == 1, c
    assert rc == before_loop[0]
    for key in KEYS:
        assert np.array_equal(st[key], before_loop[1][key]), key
