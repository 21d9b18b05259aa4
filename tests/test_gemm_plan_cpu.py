"""How ONE GEMM and one process(dt) are launched, checked without a GPU: kernel, tile height, grid, the mean-finishing and linearising
workgroups, the mirrored form and the tile order are integer arithmetic over the switches and a shape (ekf_vio_amd/csrc/plan.h, plan_gemm and
plan_predict; gemm.hip's launch_gemm and ekf_kernels.hip's launch_predict execute the answer).  ekfvio_test_gemm_plan and
ekfvio_test_predict_plan (hooks build) call them with no handle and no HIP call.  Every expected value below was derived by hand from the
launcher this arithmetic was moved out of."""
import ctypes as C

import pytest

import test_plan_cpu as P

CUS = 256  # MI355X
NONE, JOSEPH1, MEAN, MEAN_PARTIAL = 0, 1, 2, 3  # GemmEpiMode of plan.h
FIELDS = ("k16", "bm", "wps", "groups", "threads", "tiles_x", "tiles_y", "tiles", "grid_x", "grid_y", "mean_wg", "lin_blocks", "mean_keep",
          "sym", "sym_w", "order2d", "throughput_regime", "tile_height")
PFIELDS = ("dense", "pre", "lin_inside", "lin_in_front", "ts", "chunks", "book_rides", "grid")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in ("GEMM_ORDER2D", "SYM_JOSEPH", "FUSE_LINEARIZE", "SWEEP", "SWEEP_LA", "T2", "SCHUR", "PERSIST_OVERSUB", "PERSIST_GAIN", "FUSE_SWEEP",
                 "FUSE_GATHER", "LIN_OVERLAP"):
        monkeypatch.delenv("EKFVIO_" + name, raising=False)  # every switch plan_gemm, plan_predict and plan_update read


def gemm(M, N, K, tb=True, lowerB=False, epi=NONE, mean=False, lin_blocks=0, sym=False, variant=0, cus=CUS):
    from ekf_vio_amd import capi
    out = (C.c_int32 * 18)()
    rc = capi.load(hooks=True).ekfvio_test_gemm_plan(cus, M, N, K, int(tb), int(lowerB), epi, int(mean), lin_blocks, int(sym), variant, out)
    assert rc == capi.OK
    return dict(zip(FIELDS, out))


def predict(N, dense=False, pre=False, book=False, cus=CUS):
    from ekf_vio_amd import capi
    out = (C.c_int32 * 8)()
    assert capi.load(hooks=True).ekfvio_test_predict_plan(cus, N, int(dense), int(pre), int(book), out) == capi.OK
    return dict(zip(PFIELDS, out))


def grid(p):
    return (p["grid_x"], p["grid_y"])


# ---------------------------------------------------------------- the latency regime: gemm16_kernel, one wave of workgroups
def test_the_n256_tail_gemm():
    p = gemm(790, 790, 512, epi=MEAN_PARTIAL, mean=True)
    assert (p["k16"], p["bm"], p["wps"], p["threads"]) == (1, 48, 2, 512)
    assert (p["tiles_x"], p["tiles_y"], p["tiles"]) == (17, 13, 221)
    assert grid(p) == (222, 1) and p["mean_wg"] == 1 and (p["lin_blocks"], p["mean_keep"]) == (0, 0)
    p = gemm(790, 790, 512, epi=MEAN_PARTIAL, mean=True, lin_blocks=33)
    assert grid(p) == (255, 1) and (p["lin_blocks"], p["mean_keep"]) == (33, 1)
    p = gemm(790, 790, 512, epi=MEAN_PARTIAL, mean=True, lin_blocks=35)  # 221 + 1 + 35 = 257 > 256: none of them
    assert grid(p) == (222, 1) and (p["lin_blocks"], p["mean_keep"]) == (0, 0)
    p = gemm(790, 791, 512, epi=JOSEPH1)
    assert (p["k16"], p["bm"], p["tiles"]) == (1, 48, 221) and grid(p) == (221, 1) and p["mean_wg"] == 0
    p = gemm(790, 790, 512, epi=MEAN, mean=False)
    assert p["mean_wg"] == 0 and grid(p) == (221, 1)
    assert gemm(790, 790, 512, epi=MEAN, mean=True)["grid_x"] == 222
    # the linearisation rides in the one GEMM of the T2 / Schur tail only, and only with a mean to finish
    assert gemm(790, 790, 512, epi=MEAN, mean=True, lin_blocks=33)["lin_blocks"] == 0
    assert gemm(790, 790, 512, epi=MEAN_PARTIAL, mean=False, lin_blocks=33)["lin_blocks"] == 0


def test_other_latency_regime_shapes():
    p = gemm(322, 322, 256, epi=MEAN_PARTIAL, mean=True)
    assert (p["k16"], p["bm"], p["tiles_x"], p["tiles_y"], p["tiles"]) == (1, 32, 11, 6, 66)
    p = gemm(200, 64, 64, tb=False)
    assert (p["k16"], p["groups"], p["threads"]) == (0, 1, 256) and grid(p) == (4, 1)
    p = gemm(130, 70, 48, tb=True)  # K no multiple of 64
    assert (p["k16"], p["threads"]) == (0, 256) and grid(p) == (3, 2)
    assert gemm(1, 1, 64)["bm"] == 32 and gemm(1, 1, 64)["grid_x"] == 1


# ---------------------------------------------------------------- the throughput regime: gemm_f32_mfma_kernel
def test_the_n1024_joseph_gemms(monkeypatch):
    p = gemm(3094, 3094, 2048, epi=MEAN, mean=True, sym=True)
    assert (p["k16"], p["threads"]) == (0, 256) and grid(p) == (1225, 1)
    assert (p["sym"], p["sym_w"], p["order2d"], p["tiles"]) == (1, 7, 0, 1225)
    assert (p["lin_blocks"], p["mean_keep"], p["mean_wg"]) == (0, 0, 0)  # (gemm16_kernel only; workgroup (0, 0) finishes the mean)
    p = gemm(3094, 3095, 2048, epi=JOSEPH1)
    assert grid(p) == (49, 49) and (p["sym"], p["order2d"], p["tiles"]) == (0, 1, 2401)
    # asked for, not heeded: another epilogue, a product that is not square, A * B
    assert gemm(3094, 3094, 2048, epi=JOSEPH1, sym=True)["sym"] == 0
    assert gemm(3094, 3094, 2048, epi=MEAN_PARTIAL, mean=True, sym=True)["sym"] == 0
    assert gemm(3094, 3030, 2048, epi=MEAN, mean=True, sym=True)["sym"] == 0
    assert gemm(3094, 3094, 2048, sym=True)["sym"] == 0
    assert gemm(3094, 3094, 2048, epi=MEAN, mean=True)["sym"] == 0  # not asked for
    monkeypatch.setenv("EKFVIO_SYM_JOSEPH", "0")
    p = gemm(3094, 3094, 2048, epi=MEAN, mean=True, sym=True)
    assert grid(p) == (49, 49) and (p["sym"], p["sym_w"], p["order2d"], p["tiles"]) == (0, 1, 1, 2401)


def test_order2d(monkeypatch):
    p = gemm(3094, 2048, 2048, lowerB=True)  # the triangular-aware gain GEMM
    assert (p["k16"], p["order2d"]) == (0, 0) and grid(p) == (49, 32)
    on, off = gemm(2048, 1024, 2048), gemm(1984, 1024, 2048)  # two tiles per compute unit: 512 tiles on, 496 off
    assert (on["k16"], on["tiles"], on["order2d"]) == (0, 512, 1) and (off["k16"], off["tiles"], off["order2d"]) == (0, 496, 0)
    ragged = [(2100, 1050, True, (33, 17)), (1050, 2100, True, (17, 33)), (2600, 830, False, (41, 13)), (1601, 1409, True, (26, 23))]
    for M, N, tb, tiles in ragged:  # tests/test_gpu_parity.py, test_throughput_regime_gemm_tile_order_is_a_permutation (K padded to 64 by the hook)
        p = gemm(M, N, 64, tb=tb, variant=1)
        assert (p["k16"], p["threads"], p["order2d"]) == (0, 256, 1) and grid(p) == tiles, (M, N, p)
    monkeypatch.setenv("EKFVIO_GEMM_ORDER2D", "0")
    assert gemm(2048, 1024, 2048)["order2d"] == 0 and gemm(3094, 3095, 2048, epi=JOSEPH1)["order2d"] == 0
    assert not any(gemm(M, N, 64, tb=tb, variant=1)["order2d"] for M, N, tb, _ in ragged)


# ---------------------------------------------------------------- the hooks' variants
def test_variants():
    p = gemm(790, 790, 512, variant=148)
    assert (p["k16"], p["bm"], p["wps"], p["threads"]) == (1, 48, 1, 256) and grid(p) == (221, 1)
    for bm, tx in ((32, 25), (48, 17), (64, 13)):
        p = gemm(790, 790, 512, variant=bm)
        assert (p["k16"], p["bm"], p["wps"], p["threads"]) == (1, bm, 2, 512) and grid(p) == (tx * 13, 1)
    p = gemm(200, 64, 64, tb=False, variant=32)  # gemm16_kernel is A * B^T only
    assert (p["k16"], p["groups"], p["threads"]) == (0, 1, 256)
    assert gemm(130, 70, 48, variant=64)["k16"] == 0  # ... over whole 64-deep K-tiles
    assert gemm(790, 790, 512, variant=40) == gemm(790, 790, 512)  # no such tile height: the production choice
    assert gemm(3094, 3094, 2048, variant=140) == gemm(3094, 3094, 2048)
    p = gemm(790, 790, 512, variant=2)
    assert (p["k16"], p["groups"], p["threads"]) == (0, 2, 512) and grid(p) == (13, 13)
    p = gemm(790, 790, 512, variant=1)
    assert (p["k16"], p["groups"], p["threads"]) == (0, 1, 256) and grid(p) == (13, 13)


# ---------------------------------------------------------------- the planner and the launcher agree (they ask the same function)
def tail_gemm(p, N, cus, lin_blocks):
    """The last GEMM of the update with plan p as launch_update builds it (ekf_kernels.hip, update_tail_gemms): n x n x m_pad, A * B^T."""
    n = 22 + 3 * N
    if p["tail"] == P.TAIL_JOSEPH:
        return n, gemm(n, n, p["m_pad"], epi=MEAN, mean=True, sym=True, cus=cus)
    return n, gemm(n, n, p["m_pad"], epi=MEAN_PARTIAL, mean=True, lin_blocks=lin_blocks, cus=cus)


@pytest.mark.parametrize("cus", [128, 256, 304])
def test_launcher_keeps_exactly_the_linearising_workgroups_the_update_plan_counts_on(cus):
    seen = 0
    for N in P.NS:
        asked = (N + 7) // 8 + 1  # a workgroup per LIN_LM = 8 landmarks and the base block's (plan.h, plan_update)
        for k in range(1, N + 1):
            p = P.plan(N, 2 * k, cus=cus, next_dt=0.05)
            if p["tail"] == P.TAIL_JOSEPH:
                assert p["lin_blocks"] == 0
                continue
            n, g = tail_gemm(p, N, cus, asked)
            assert g["lin_blocks"] == p["lin_blocks"] and p["lin_blocks"] in (0, asked), (N, k, p, g)
            if p["lin_blocks"]:
                assert g["k16"] == 1 and g["grid_x"] == g["tiles"] + 1 + asked <= cus and g["mean_keep"] == 1, (N, k, g)
                seen += 1
            # ... and what the plan does not ask for the launcher does not add
            assert tail_gemm(p, N, cus, 0)[1]["lin_blocks"] == 0
    assert seen


def test_second_joseph_gemm_is_mirrored_exactly_in_the_throughput_regime():
    seen = set()
    for cus in (128, 256, 304):
        for N in P.NS:
            for k in range(1, N + 1):
                p = P.plan(N, 2 * k, cus=cus)
                if p["tail"] != P.TAIL_JOSEPH:
                    continue
                n, g = tail_gemm(p, N, cus, 0)
                assert g["sym"] == g["throughput_regime"] == (0 if g["k16"] else 1), (cus, N, k, g)
                assert g["tiles"] == (g["tiles_x"] * (g["tiles_x"] + 1) // 2 if g["sym"] else g["tiles_x"] * g["tiles_y"])
                seen.add(g["sym"])
    assert seen == {0, 1}


# ---------------------------------------------------------------- process(dt)
def test_predict_plan(monkeypatch):
    p = predict(256)  # 16 x 16 landmark tiles <= 4 x 256
    assert (p["dense"], p["pre"], p["lin_inside"], p["lin_in_front"]) == (0, 0, 1, 0)
    assert (p["ts"], p["chunks"], p["grid"]) == (16, 86, 256 + 1 + 2 * 86)
    assert predict(256, book=True)["grid"] == 256 + 1 + 2 * 86 + 1
    p = predict(1024, book=True)  # 4096 tiles > 1024: linearize_kernel in front, and the bookkeeping with it
    assert (p["lin_inside"], p["lin_in_front"], p["book_rides"]) == (0, 1, 0) and (p["ts"], p["chunks"]) == (64, 342)
    assert p["grid"] == 4096 + 1 + 2 * 342
    assert predict(512)["lin_inside"] == 1 and predict(513)["lin_inside"] == 0  # 32 x 32 = 1024 tiles is the last
    assert predict(256, cus=64)["lin_inside"] == 1 and predict(257, cus=64)["lin_inside"] == 0
    for N in (0, 1, 20, 256, 1024):
        p = predict(N, dense=True, pre=True)  # the dense mode: never inside, never pre
        assert (p["dense"], p["pre"], p["lin_inside"], p["lin_in_front"]) == (1, 0, 0, 1), N
        p = predict(N, pre=True, book=True)  # the previous GEMM linearised: nobody does, the bookkeeping rides
        assert (p["pre"], p["lin_inside"], p["lin_in_front"], p["book_rides"]) == (1, 0, 0, 1), N
        assert p["grid"] == p["ts"] ** 2 + 1 + 2 * p["chunks"] + 1
    monkeypatch.setenv("EKFVIO_FUSE_LINEARIZE", "0")
    for N in (0, 1, 20, 256, 1024):
        p = predict(N)
        assert (p["lin_inside"], p["lin_in_front"]) == (0, 1), N
        assert predict(N, pre=True)["lin_in_front"] == 0
