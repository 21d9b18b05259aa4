"""bench.py's plain run and --dump-outputs: the headline line alone, and the state of the last timed step written as
float32 .npy files (whole below 64 MB, a fixed seeded sample of Sigma above)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CONTRACT_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY_KEYS = ("roofline", "roofline_step", "stage_us_per_step", "pcie_inclusive_steps_per_s", "cpu_baseline", "full_loop", "klt",
                  "other_sizes", "concurrent_sequences_one_gpu")


def _state(N, seed=0):
    rng = np.random.default_rng(seed)
    n = 22 + 3 * N
    return dict(base_mu=rng.standard_normal(22).astype(np.float32), feat_mu=rng.standard_normal((N, 3)).astype(np.float32),
                last_klt=rng.standard_normal((N, 2)).astype(np.float32), del_flag=(rng.random(N) < 0.1).astype(np.uint8),
                Sigma=rng.standard_normal((n, n)).astype(np.float32))


def test_dump_writes_the_whole_state_in_float32(tmp_path):
    st = _state(256)
    names = bench.dump_outputs(str(tmp_path), st)
    assert names == ["Sigma", "base_mu", "del_flag", "feat_mu", "last_klt"]
    for k in names:
        a = np.load(os.path.join(str(tmp_path), k + ".npy"))
        assert a.dtype == np.float32
        assert np.array_equal(a, np.asarray(st[k], np.float32))


def test_dump_of_a_large_sigma_is_a_fixed_sample_under_64_mb(tmp_path):
    st = _state(1400)  # n = 4222: Sigma alone is 71 MB
    a, b = tmp_path / "a", tmp_path / "b"
    names = bench.dump_outputs(str(a), st)
    assert names == ["Sigma_diag", "Sigma_sample", "base_mu", "del_flag", "feat_mu", "last_klt"]
    assert bench.dump_outputs(str(b), st) == names
    total = sum(os.path.getsize(os.path.join(str(a), k + ".npy")) for k in names)
    assert total <= 64 << 20
    for k in names:
        x, y = np.load(os.path.join(str(a), k + ".npy")), np.load(os.path.join(str(b), k + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, y)  # the same positions every time
    assert np.array_equal(np.load(os.path.join(str(a), "Sigma_diag.npy")), np.diagonal(st["Sigma"]))
    sample = np.load(os.path.join(str(a), "Sigma_sample.npy"))
    assert sample.size == bench.DUMP_SIGMA_SAMPLE and np.isin(sample, st["Sigma"]).all()


def test_native_library_loads_from_a_tree_the_benchmark_cannot_write(monkeypatch):
    """capi.load() decides staleness under a lock file it opens for writing next to the library: a benchmark run by a user
    who cannot write into the built tree loads the built library as it is; a missing library and other errors still fail."""
    import errno
    from ekf_vio_amd import capi
    calls = []

    def fake_load(build_if_missing=True, hooks=False):
        calls.append((build_if_missing, hooks))
        if build_if_missing:
            raise PermissionError(errno.EACCES, "Permission denied", ".build.lock")
        return "built library"

    monkeypatch.setattr(capi, "load", fake_load)
    assert bench.load_native(hooks=True) == "built library"
    assert calls == [(True, True), (False, True)]

    def missing(build_if_missing=True, hooks=False):
        if build_if_missing:
            raise PermissionError(errno.EACCES, "Permission denied", ".build.lock")
        raise FileNotFoundError("libekfvio_hip.so not built")

    monkeypatch.setattr(capi, "load", missing)
    with pytest.raises(FileNotFoundError):
        bench.load_native()

    def full_disk(build_if_missing=True, hooks=False):
        raise OSError(errno.ENOSPC, "No space left on device")

    monkeypatch.setattr(capi, "load", full_disk)
    with pytest.raises(OSError):
        bench.load_native()


@pytest.mark.parametrize("warmup,steps", [(20, 300), (5, 20), (20, 428), (20, 429), (5, 110000), (300, 1000), (1000, 50)])
def test_timed_steps_stay_inside_the_valid_part_of_the_sequence(warmup, steps):
    """Exactly --steps timed and --warmup warm-up steps, none of them past VALID_FRAMES (the synthetic camera reaches its
    landmarks near frame 580); a run that fits is one segment over the frames of one uninterrupted run."""
    start, timed, warm = bench.timed_segments(warmup, steps)
    assert sum(timed) == steps and start + sum(warm) == warmup
    assert start + max(timed) <= bench.VALID_FRAMES and start + max(warm + [0]) <= bench.VALID_FRAMES
    assert bench.VALID_FRAMES + 20 + 100 < 580  # the --full profiled and per-call steps that continue from the last timed one
    if warmup + steps <= bench.VALID_FRAMES and warmup <= bench.VALID_FRAMES // 2:
        assert (start, timed, warm) == (warmup, [steps], [])


def test_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_last_step(tmp_path):
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5",
                          "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    for k in CONTRACT_KEYS:
        assert k in r
    assert r["steps"] == 40 and r["warmup"] == 5 and r["unit"] == "steps/s" and r["dtype"] == "f32"
    assert abs(r["ms_per_step"] - 1e3 / r["value"]) < 1e-6 * r["ms_per_step"]
    assert not [k for k in FULL_ONLY_KEYS if k in r]
    assert r["state_finite_and_psd_diag"] and r["dumped_outputs"] == ["Sigma", "base_mu", "del_flag", "feat_mu", "last_klt"]
    n = 22 + 3 * 256
    sig = np.load(str(d / "Sigma.npy"))
    assert sig.dtype == np.float32 and sig.shape == (n, n) and np.isfinite(sig).all()
    assert np.load(str(d / "feat_mu.npy")).shape == (256, 3) and np.load(str(d / "base_mu.npy")).shape == (22,)


@pytest.mark.gpu
def test_a_long_plain_run_stays_finite(tmp_path):
    """--steps far beyond the synthetic sequence's valid part (the camera reaches its landmarks near frame 580): the timed
    steps run in segments from the same warm state, so what the last timed step leaves is a finite, positive-diagonal state."""
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3000", "--warmup", "5",
                          "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["steps"] == 3000 and r["state_finite_and_psd_diag"] and not r["numeric_warning_in_timed_run"]  # (no frame past the valid part)
    assert r["timed_region"]["segments"] > 1
    for k in r["dumped_outputs"]:
        assert np.isfinite(np.load(str(d / (k + ".npy")))).all(), k
    sig = np.load(str(d / "Sigma.npy"))
    assert (np.diagonal(sig) > 0).all()
