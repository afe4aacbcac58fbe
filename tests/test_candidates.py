"""Window selection from candidate positions (preprocess/CreateTensorPileupFromCffi.py:343-397), without a GPU: the numpy statement of the
rule against the fixture the reference's own CreateTensorPileup wrote, the conditions that keep that fixture from being easy, recipe drift,
the rule on random regions against a one-candidate-at-a-time loop, and the new symbols in header, binding and library."""
import ctypes as C
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from tests import util

MODES = (("main", False), ("head_tail", True))


def fixture():
    z = np.load(os.path.join(util.GOLDEN, "pileup_candidates.npz"))
    return z, json.loads(str(z["meta"]))


def maker():
    spec = importlib.util.spec_from_file_location("make_golden_candidates", os.path.join(util.GOLDEN, "make_golden_candidates.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_keeps_its_promises():
    """what tests/golden/make_golden_candidates.py asserts when it writes the fixture, on the committed file: every status of either mode at
    least 8 times, chunks of 1, 32, 33, 34, 35 and >= 100 columns, candidates at every edge of the rule and outside every chunk, windows
    dropped for an empty column at their first, middle and last column, a kept head / tail window that holds one, rescaled windows among
    the kept; and the inputs are the ones the script draws today"""
    mk = maker()
    z, meta = fixture()
    matrix, major, cand, depth = z["matrix"], z["major"], z["cand"], z["depth"]
    assert matrix.dtype == np.int64 and major.dtype == np.int64 and cand.dtype == np.int64 and depth.dtype == np.int32
    kept = {m: z[f"kept_{m}"] for m, _ in MODES}
    windows = {m: z[f"windows_{m}"] for m, _ in MODES}
    counts = mk.conditions(matrix, major, cand, depth, kept, windows)
    assert {m: {str(k): v for k, v in c.items()} for m, c in counts.items()} == meta["status_counts"]
    m2, j2, c2, d2 = mk.make_inputs()
    assert np.array_equal(m2, matrix) and np.array_equal(j2, major) and np.array_equal(c2, cand) and np.array_equal(d2, depth), "recipe drift"
    assert mk.digest(matrix) == meta["matrix_sha"] and mk.digest(cand) == meta["cand_sha"] and mk.digest(depth) == meta["depth_sha"]
    for m, _ in MODES:
        assert mk.digest(kept[m]) == meta["kept_sha"][m] and mk.digest(windows[m]) == meta["windows_sha"][m]
    assert len(matrix) == meta["n_cols"] and len(cand) == meta["n_cand"]


@pytest.mark.parametrize("mode,head_tail", MODES)
def test_rule_reproduces_the_reference(mode, head_tail):
    """statuses, order and windows: exactly what CreateTensorPileup returned"""
    mk = maker()
    z, _ = fixture()
    for region in (z["matrix"], z["matrix"].astype(np.int32)):
        status, windows = syn.select_pileup_windows(region, z["major"], z["cand"], head_tail)
        assert status.dtype == np.uint8 and windows.dtype == np.int32
        kept = np.isin(status, syn.CAND_KEPT)
        assert np.array_equal(z["cand"][kept], z[f"kept_{mode}"]), "kept candidates / their order"
        assert np.array_equal(windows, z[f"windows_{mode}"])
        assert np.array_equal(status, mk.classify(z["matrix"], z["major"], z["cand"], head_tail)[0])
    if not head_tail:
        assert not np.isin(status, (syn.CAND_HEAD, syn.CAND_TAIL)).any()


def test_status_codes_agree_everywhere():
    mk = maker()
    header = open(os.path.join(util.ROOT, "include", "c3hip.h")).read()
    for name, val in (("NO_WINDOW", 0), ("MAIN", 1), ("EMPTY_COLUMN", 2), ("HEAD", 3), ("TAIL", 4)):
        assert f"#define C3_CAND_{name} {val}\n" in header
        assert getattr(syn, f"CAND_{name}") == getattr(_lib, f"CAND_{name}") == getattr(mk, name) == val


def test_rule_on_random_regions():
    """the vectorised statement against the loop over candidates, on regions of 1 - 5 chunks of 1 .. 400 columns with 1 % empty columns"""
    mk = maker()
    rng = np.random.default_rng(21)
    seen = np.zeros(5, np.int64)
    for trial in range(120):
        lens = rng.choice([1, 5, 17, 18, 31, 32, 33, 34, 35, 36, 40, 50, 66, 120, 400], size=rng.integers(1, 6))
        pos0, parts = 5000, []
        for n in lens:
            parts.append(np.arange(pos0, pos0 + n))
            pos0 += n + rng.choice([1, 2, 3, 20, 40])
        major = np.concatenate(parts).astype(np.int64)
        region = rng.integers(1, 50, size=(len(major), 18)).astype(np.int32)
        region[rng.random(len(major)) < 0.01] = 0
        cand = rng.permutation(np.unique(rng.integers(major[0] - 20, major[-1] + 20, size=min(200, len(major) + 5))))
        for ht in (False, True):
            want, _ = mk.classify(region, major, cand, ht)
            status, windows = syn.select_pileup_windows(region, major, cand, ht)
            assert np.array_equal(status, want), (trial, ht)
            st2, chunk, off = syn.select_pileup_starts(region, major, cand, ht)
            assert np.array_equal(st2, status)
            a, _ = syn.pileup_chunks(major)
            for j, i in enumerate(np.flatnonzero(status == syn.CAND_MAIN)[:5]):
                col = a[chunk[i]] + off[i]
                k = int(np.isin(status[:i], syn.CAND_KEPT).sum())
                assert np.array_equal(windows[k], region[col:col + 33])
            if ht:
                seen += np.bincount(status, minlength=5)
    assert (seen >= 100).all(), seen


def test_rule_edge_cases():
    region = np.ones((40, 18), np.int32)
    major = np.arange(100, 140)
    st, w = syn.select_pileup_windows(region, major, np.zeros(0, np.int64))
    assert st.shape == (0,) and w.shape == (0, 33, 18)
    st, w = syn.select_pileup_windows(np.zeros((0, 18), np.int32), np.zeros(0, np.int64), np.array([5, 6]), True)
    assert st.tolist() == [0, 0] and w.shape == (0, 33, 18)
    # 40 columns: main needs pos - 17 >= 100 and pos + 17 <= 139
    st, _ = syn.select_pileup_windows(region, major, np.array([116, 117, 122, 123]))
    assert st.tolist() == [0, 1, 1, 0]
    st, w = syn.select_pileup_windows(region, major, np.array([116, 123, 139, 100]), True)
    assert st.tolist() == [syn.CAND_HEAD, syn.CAND_TAIL, syn.CAND_TAIL, syn.CAND_HEAD]
    assert (w[0, 0] == 0).all() and (w[0, 1] == 1).all() and (w[1] == 1).all()  # 123 + 17 = last + 1: a complete tail window
    assert (w[2, :18] == 1).all() and (w[2, 18:] == 0).all() and (w[3, :17] == 0).all() and (w[3, 17:] == 1).all()  # positions 122 .. 154 / 83 .. 115
    with pytest.raises(ValueError, match="strictly increasing"):
        syn.select_pileup_windows(region, np.r_[major[:-1], major[-2]], np.array([120]))


NEW_SYMBOLS = ("c3_predict_submit_candidates", "c3_predict_pileup_candidates")


def test_new_symbols_in_header_binding_and_library():
    from tests.test_abi import declared_symbols
    declared = declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and name in exported, name
    assert {s for s in exported if s.startswith("c3_")} == set(declared), "nm -D and the header disagree"
    assert b"c3hip 0.5." in _lib.lib().c3_version()


def test_candidate_entries_fail_without_aborting():
    """argument errors that are decided before any device work: non-zero return and a message, the process goes on"""
    L = _lib.lib()
    n = C.c_int64(-1)
    assert L.c3_predict_pileup_candidates(None, None, _lib.DTYPE_I32, 0, None, None, None, 0, 0, None, None, C.byref(n)) != 0
    assert b"null model" in L.c3_last_error()
    assert L.c3_predict_submit_candidates(None, None, _lib.DTYPE_I32, 0, None, None, None, 0, 1, None, None, None, 0) != 0
    assert b"null model" in L.c3_last_error()


def test_python_entry_needs_a_device():
    from clair3_amd.model import Clair3_P
    try:
        has_gpu = _lib.device_count() > 0
    except _lib.C3Error:
        has_gpu = False
    m = Clair3_P(predict=True)
    assert hasattr(m, "predict_candidates") and hasattr(m, "submit_candidates")
    if not has_gpu:  # no handle, no fallback: the numpy rule is synthetic.select_pileup_windows, the rows need the device
        with pytest.raises((_lib.C3Error, TypeError, AttributeError, OSError)):
            m.predict_candidates(np.ones((40, 18), np.int32), np.arange(40), np.array([20]))
