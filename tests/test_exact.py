"""The exact form without a device: its entries in the header and the library, their refusals, the audit tool's comparison
(audit.compare, plain numpy) and its argument handling."""
import os
import re

import numpy as np
import pytest

from clair3_amd import _lib, audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("c3_model_set_exact", "c3_predict_exact", "c3_exact_fetch")


def test_the_header_declares_the_entries_and_the_library_exports_them():
    with open(os.path.join(ROOT, "include", "c3hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(c3_model \*m, ", header, re.M), f"{name} is not declared in include/c3hip.h"
        assert name in _lib.EXPORTS, f"{name} is missing from _lib.EXPORTS"
        assert getattr(_lib.lib(), name) is not None
    assert "double *y_host" in header and "double *host_out, int64_t n_doubles" in header


def test_null_handles_are_refused_with_a_message():
    L = _lib.lib()
    y = np.zeros(90)
    assert L.c3_predict_exact(None, y.ctypes.data, _lib.DTYPE_I8, 1, y.ctypes.data) != 0
    assert "null model" in _lib.last_error() and "c3_predict_exact" in _lib.last_error()
    assert L.c3_exact_fetch(None, b"l4_out", 0, 1, y.ctypes.data, 90) != 0
    assert "null model" in _lib.last_error() and "c3_exact_fetch" in _lib.last_error()
    assert L.c3_model_set_exact(None, 1) != 0 and "null model" in _lib.last_error()


def _rows(n, cols=90, seed=0):
    """n rows of well separated probabilities: every head's arg-max is column 0 of the head, far from a tie"""
    rng = np.random.default_rng(seed)
    y = np.zeros((n, cols))
    for lo, hi in audit.HEAD_SLICES:
        if lo >= cols:
            break
        y[:, lo:hi] = 0.2 / (hi - lo - 1) * (1 + 0.01 * rng.random((n, hi - lo)))
        y[:, lo] = 0.8
    return y


def test_compare_tolerance():
    ye = _rows(6)
    yf = ye.copy()
    yf[1, 5] += 0.99e-4   # just under tol
    yf[4, 30] -= 1.01e-4  # just over: row 4 is the one row over tol, and the worst
    c = audit.compare(ye, yf, tol=1e-4, near_tie=1e-6)
    assert c["windows"] == 6 and c["rows_over_tol"] == 1 and c["worst_window"] == 4
    assert abs(c["max_abs_err"] - 1.01e-4) < 1e-12
    assert c["label_diffs"] == [0, 0, 0, 0] and c["near_ties"] == [0, 0, 0, 0]
    same = audit.compare(ye, ye)
    assert same["max_abs_err"] == 0.0 and same["rows_over_tol"] == 0 and same["head_max_abs_err"] == [0.0] * 4


def test_compare_head_boundaries():
    """columns 0-21-24-57-90: an error in the last column of a head belongs to that head, in the next column to the next"""
    ye = _rows(3)
    for head, (lo, hi) in enumerate(audit.HEAD_SLICES):
        for col, owner in ((lo, head), (hi - 1, head)):
            yf = ye.copy()
            yf[2, col] += 3e-5
            got = audit.compare(ye, yf)["head_max_abs_err"]
            assert [g > 0 for g in got] == [h == owner for h in range(4)], (col, got)
    c24 = audit.compare(_rows(3, 24), _rows(3, 24))
    assert len(c24["head_max_abs_err"]) == len(c24["label_diffs"]) == len(c24["near_ties"]) == 2
    with pytest.raises(ValueError):
        audit.compare(np.zeros((2, 90)), np.zeros((2, 24)))


def test_compare_argmax_flips_and_near_ties():
    ye = _rows(4)
    # window 1, genotype head (21..24): an exact near-tie between columns 21 and 22 (gap 5e-7), the form picks the other one: excused
    ye[1, 21], ye[1, 22] = 0.45, 0.45 - 5e-7
    # window 3, first indel head (24..57): a clear exact gap (2e-5, outside the near-tie), the form flips it: counted
    ye[3, 24], ye[3, 25] = 0.45, 0.45 - 2e-5
    yf = ye.copy()
    yf[1, 21], yf[1, 22] = ye[1, 22], ye[1, 21]
    yf[3, 24], yf[3, 25] = ye[3, 25], ye[3, 24]
    c = audit.compare(ye, yf, tol=1e-4, near_tie=1e-6)
    assert c["near_ties"] == [0, 1, 0, 0] and c["label_diffs"] == [0, 0, 1, 0] and c["rows_over_tol"] == 0
    # the same exact gap excused once near_tie covers it
    assert audit.compare(ye, yf, near_tie=1e-4)["label_diffs"] == [0, 0, 0, 0]


def test_compare_counts_a_non_finite_value_as_over_tol():
    ye = _rows(3)
    for bad in (np.nan, np.inf, -np.inf):
        yf = ye.copy()
        yf[2, 60] = bad
        c = audit.compare(ye, yf)
        assert c["rows_over_tol"] == 1 and c["worst_window"] == 2 and c["max_abs_err"] == np.inf
        assert c["head_max_abs_err"][3] == np.inf and c["head_max_abs_err"][:3] == [0.0] * 3


def test_argument_parsing():
    base = ["--chkpnt_fn", "m.pt", "--tensor_fn", "x.npy"]
    a = audit.parse_args(base)
    assert not a.pileup and a.plan_list == [] and a.tol == 1e-4 and a.near_tie == 1e-6 and a.max_windows is None and a.out is None
    a = audit.parse_args(base + ["--pileup", "--plans", "lstm2; proj2,lstm2 ;all;;lstm2", "--tol", "2e-5", "--max_windows", "64", "--out", "f"])
    assert a.pileup and a.plan_list == ["lstm2", "proj2,lstm2"] and a.tol == 2e-5 and a.max_windows == 64 and a.out == "f"
    assert audit.parse_args(base + ["--plans", "res3a;res2a,res2b"]).plan_list == ["res3a", "res2a,res2b"]
    for bad in (["--tol", "0"], ["--near_tie", "-1"], ["--max_windows", "0"]):
        with pytest.raises(_lib.C3Error):
            audit.parse_args(base + bad)
    with pytest.raises(SystemExit):
        audit.parse_args(["--tensor_fn", "x.npy"])


def test_a_bad_plan_name_is_refused_before_any_device_call():
    """through c3_layer_precision_check: the checkpoint and the tensor file do not even exist"""
    base = ["--chkpnt_fn", "/nonexistent/m.pt", "--tensor_fn", "/nonexistent/x.npy"]
    with pytest.raises(_lib.C3Error, match="unknown layer \"lstm3\""):
        audit.main(base + ["--pileup", "--plans", "lstm2;lstm3"])
    with pytest.raises(_lib.C3Error, match="layer of the pileup network"):
        audit.main(base + ["--plans", "lstm2"])
    with pytest.raises(_lib.C3Error, match="layer of the full-alignment network"):
        audit.main(base + ["--pileup", "--plans", "res3a"])
