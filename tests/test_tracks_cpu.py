"""Landmark identities and the tracks that ended, without a GPU: the pure-Python model the device is held to (tests/_tracks.py) keeps its own
promises, and every layer above the kernels -- header, version script, ctypes prototypes, the two Python classes -- carries the feature."""
import fnmatch
import os
import re

import numpy as np

from _tracks import TrackModel, ended_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ekfvio_get_landmark_ids", "ekfvio_set_ended_export", "ekfvio_get_ended")


def test_model_ids_rise_strictly_and_are_never_reused():
    rng = np.random.default_rng(5)
    m = TrackModel()
    seen, ended_total = set(), 0
    for step in range(300):
        if rng.random() < 0.5:
            k = int(rng.integers(0, 6))
            before = m.next_id
            m.append(k, stamp=0.1 * step)
            assert m.next_id == before + k
            fresh = set(range(before, before + k))
            assert not (fresh & seen)  # never reused, not even an id whose landmark has left
            seen |= fresh
            assert np.array_equal(m.ids[len(m.rows) - k:], np.arange(before, before + k))
            assert np.all(m.born[len(m.rows) - k:] == 0.1 * step)
        else:
            mask = rng.random(len(m.rows)) < 0.3
            ids_before, born_before = m.ids, m.born
            ended = m.remove(mask)
            eid, eborn, eidx = ended_arrays(ended)
            # index_before is the row in front of the removal, in landmark order, and names the very landmark the record carries
            assert np.array_equal(eidx, np.nonzero(mask)[0])
            assert np.array_equal(eid, ids_before[eidx]) and np.array_equal(eborn, born_before[eidx])
            assert np.array_equal(m.ids, ids_before[~mask]) and np.array_equal(m.born, born_before[~mask])
            ended_total += len(ended)
        if step == 150:
            m.reset()
            ended_total = 0
            assert len(m.rows) == 0 and m.next_id == max(seen) + 1  # the counter goes on over a reset
        assert np.all(np.diff(m.ids) > 0)  # strictly increasing in landmark order at all times
        assert m.total_ended == ended_total
    assert len(seen) == m.next_id


def test_model_replace_hands_out_fresh_consecutive_ids():
    m = TrackModel()
    m.append(4, np.nan)
    assert np.all(np.isnan(m.born))
    m.remove([0, 1, 0, 0])
    m.replace(5, 2.5)
    assert np.array_equal(m.ids, np.arange(4, 9)) and np.all(m.born == 2.5) and m.next_id == 9


def test_header_declares_the_entry_points_and_the_map_exports_them():
    hdr = open(os.path.join(ROOT, "include", "ekfvio.h")).read()
    api_marked = set(re.findall(r"^EKFVIO_API [a-z \*]*?\b(ekfvio_[a-z0-9_]+)\s*\(", hdr, re.M))
    vmap = open(os.path.join(ROOT, "ekf_vio_amd", "csrc", "ekfvio.map")).read()
    exported = re.search(r"global:(.*?)local:", vmap, re.S).group(1)
    patterns = [p.strip() for p in exported.replace("\n", " ").split(";") if p.strip()]
    for s in ENTRY_POINTS:
        assert s in api_marked, s
        assert any(fnmatch.fnmatchcase(s, p) for p in patterns), (s, patterns)
    # what the header owes a consumer: the invariant, born's sources, the record and whose bits it carries, the reset rule
    for needle in ("STRICTLY INCREASING", "never reused", "NaN before any stamp", "index_before", "bit for bit", "does NOT start over"):
        assert needle in hdr, needle


def test_capi_has_the_prototypes():
    import ctypes as C
    from ekf_vio_amd import capi
    for s in ENTRY_POINTS:
        assert s in capi.SYMBOLS, s
    lib = capi.load()
    i64p, f64p, i32p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert lib.ekfvio_get_landmark_ids.argtypes == [C.c_void_p, i64p, f64p]
    assert lib.ekfvio_set_ended_export.argtypes == [C.c_void_p, C.c_int32]
    assert lib.ekfvio_get_ended.argtypes == [C.c_void_p, i64p, f64p, i32p, f32p, f32p, C.c_int32, i32p, i64p]
    # a null handle is refused, not dereferenced
    assert lib.ekfvio_get_landmark_ids(None, None, None) == capi.EINVAL
    assert lib.ekfvio_set_ended_export(None, 1) == capi.EINVAL
    assert lib.ekfvio_get_ended(None, None, None, None, None, None, 0, None, None) == capi.EINVAL


def test_python_classes_expose_the_methods():
    import inspect
    from ekf_vio_amd import EKFVIO, TightlyCoupledEKF
    for cls in (TightlyCoupledEKF, EKFVIO):
        for name in ("landmark_ids", "setEndedExport", "ended"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
    p = inspect.signature(TightlyCoupledEKF.__init__).parameters
    assert "ended_export" in p and p["ended_export"].default is False
