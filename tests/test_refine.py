"""Refine mode (c3_model_set_refine, csrc/c3_refine.h), the part that needs no GPU: the rule in numpy (synthetic.refine_gaps / refine_select)
against a plain loop over windows that walks the columns as the kernel does, its hand-made corners, the constants against the headers that
define them, the C ABI, the environment switch and its refusals, and the loud failures without a device.  (The host code -- plan_batch with
the refine section, which batches the mode covers, the accounting of a batch that came home -- is exercised without a device by the
stand-alone program tests/host/refine_host_check.cpp, built with -fsanitize=address,undefined as its head says.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from clair3_amd import _lib, predict, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import util
from tests.test_abi import HEADER, declared_symbols

ENTRIES = ("c3_model_set_refine", "c3_model_refine_stats", "c3_model_refine_reset", "c3_refine_select")
REFINE_H = os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_refine.h")
DECODE_H = os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_decode.h")
F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


def loop_top2(values):
    """refine_top2_gap of csrc/c3_refine.h, value by value"""
    b1, b2, nan = -INF, -INF, False
    for x in values:
        x = F32(x)
        nan |= bool(x != x)
        if x > b1:
            b1, b2 = x, b1
        elif x > b2:
            b2 = x
    with np.errstate(invalid="ignore"):
        return NAN if nan else F32(b1 - b2)


def loop_rule(rows, nout, gap, columns=None):
    """rows_gap_kernel window by window: (gaps (B, 5), selected indices, minimum gaps)"""
    has_cols = rows.shape[1] > nout if columns is None else columns
    gaps, sel, mins = np.full((len(rows), 5), INF, F32), [], np.empty(len(rows), F32)
    for r, row in enumerate(rows):
        g = [INF] * 5
        for h, (lo, hi) in enumerate(syn.head_slices(nout)):
            g[h] = loop_top2(row[lo:hi])
        if has_cols:
            cols, dg = row[nout:], INF
            for b in range(4):
                if int(cols[22]) >> b & 1:
                    continue
                dg = np.fmin(dg, loop_top2([cols[9 + b]] + list(cols[0:9])))
            g[4] = dg
        gaps[r] = g
        if any(v <= F32(gap) for v in g):
            sel.append(r)
        mins[r] = np.fmin.reduce(np.array(g, F32))
    return gaps, np.array(sel, np.int32), mins


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def random_rows(nout, columns, n=97, seed=0):
    """rows whose heads hold probabilities with planted ties and near-ties, decoder columns of the same kind with random early-exit bits"""
    rng = np.random.default_rng(seed)
    rows = rng.random((n, nout + (syn.DECODE_COLS if columns else 0))).astype(F32)
    for r in range(0, n, 5):  # a duplicated maximum in one head
        lo, hi = syn.head_slices(nout)[r % len(syn.head_slices(nout))]
        rows[r, lo + 1] = rows[r, lo] = F32(2.0)
    for r in range(1, n, 7):  # a near-tie of one float32 step
        rows[r, 3] = F32(3.0)
        rows[r, 9] = np.nextafter(F32(3.0), F32(0))
    if columns:
        rows[:, nout + 22] = rng.integers(0, 16, n)
        rows[::11, nout + 22] = 15
        for r in range(2, n, 9):  # the decoder's own near-tie: homo_Ref of base C against class 4
            rows[r, nout + 22] = 0
            rows[r, nout + 10] = rows[r, nout + 3] = F32(5.0)
    return rows


@pytest.mark.parametrize("nout,columns", [(24, False), (24, True), (90, False), (90, True)])
def test_numpy_rule_equals_the_loop_on_random_rows(nout, columns):
    rows = random_rows(nout, columns, seed=nout + columns)
    g = syn.refine_gaps(rows, nout)
    assert g.shape == (len(rows), 5) and g.dtype == F32
    for gap in (0.0, 1e-4, 0.02, 0.3, 2.0):
        lg, lsel, lmin = loop_rule(rows, nout, gap)
        idx, mins = syn.refine_select(rows, nout, gap)
        assert same(g, lg) and same(idx, lsel) and same(mins, lmin), gap
        assert (np.diff(idx) > 0).all()
    assert 0 < len(syn.refine_select(rows, nout, 0.0)[0]) < len(syn.refine_select(rows, nout, 0.02)[0]) < len(rows)
    if columns:  # the decoder columns can be left out of rows that carry them
        assert same(syn.refine_gaps(rows, nout, columns=False), syn.refine_gaps(rows[:, :nout], nout))
        assert np.isinf(syn.refine_gaps(rows, nout, columns=False)[:, 4]).all()
    else:
        assert np.isinf(g[:, 4]).all()
        with pytest.raises(ValueError, match="decoder columns"):
            syn.refine_gaps(rows, nout, columns=True)
    if nout == 24:
        assert np.isinf(g[:, 2:4]).all(), "a 24-column row has two heads"


def corner_rows(nout, columns):
    """(rows, gap, expected selection) of the hand-made corners: every head of every row has the wide gap 0.5 unless the corner says otherwise"""
    gap = F32(1e-4)
    width = nout + (syn.DECODE_COLS if columns else 0)
    names = ["wide", "duplicate", "equal", "next_above", "nan_head", "nan_and_tie"]
    rows = np.zeros((len(names), width), F32)
    for lo, hi in syn.head_slices(nout):
        rows[:, lo] = 0.75
        rows[:, lo + 1] = 0.25
    if columns:  # decoder columns with a wide gap too: class maxima 0.1, homo_Ref 0.9 for every base, nobody on the early exit
        rows[:, nout:nout + 9] = 0.1
        rows[:, nout + 9:nout + 13] = 0.9
    at = {n: i for i, n in enumerate(names)}
    rows[at["duplicate"], 21:24] = [0.5, 0.5, 0.0]
    # head 0 of "equal": b1 = gap over zeros, so b1 - b2 == gap exactly; "next_above": the next float32 above it
    rows[at["equal"], 0:21], rows[at["next_above"], 0:21] = 0, 0
    rows[at["equal"], 2], rows[at["next_above"], 2] = gap, np.nextafter(gap, INF)
    rows[at["nan_head"], 5] = NAN
    rows[at["nan_and_tie"], 5] = NAN
    rows[at["nan_and_tie"], 21:24] = [0.5, 0.5, 0.0]
    expect = {"duplicate", "equal", "nan_and_tie"}
    if columns:
        extra = np.zeros((4, width), F32)
        extra[:] = rows[at["wide"]]
        # all four bases on the early exit, a tie among the class maxima behind it: no decoder gap
        extra[0, nout + 22], extra[0, nout + 9:nout + 13], extra[0, nout:nout + 2] = 15, 0.1, 0.1
        # the same tie with base G not on the early exit: selected through the decoder gap alone
        extra[1] = extra[0]
        extra[1, nout + 22] = 15 - 4
        # homo_Ref of base T ties with class 3 only: the other bases keep their wide gap
        extra[2, nout + 12], extra[2, nout + 2] = 0.5, 0.5
        # ... and that base on the early exit: not selected
        extra[3] = extra[2]
        extra[3, nout + 22] = 8
        rows = np.concatenate([rows, extra])
        names += ["all_early", "one_base_left", "base_t_tie", "base_t_early"]
        expect |= {"one_base_left", "base_t_tie"}
    return rows, gap, names, np.array([i for i, n in enumerate(names) if n in expect], np.int32)


@pytest.mark.parametrize("nout,columns", [(24, False), (24, True), (90, False), (90, True)])
def test_hand_made_corners(nout, columns):
    rows, gap, names, expect = corner_rows(nout, columns)
    at = {n: i for i, n in enumerate(names)}
    g = syn.refine_gaps(rows, nout)
    idx, mins = syn.refine_select(rows, nout, gap)
    assert same(idx, expect), [names[i] for i in idx]
    assert g[at["duplicate"], 1] == 0 and at["duplicate"] in syn.refine_select(rows, nout, 0.0)[0], "a duplicated maximum: gap 0, selected at gap = 0"
    assert g[at["equal"], 0] == gap and g[at["next_above"], 0] == np.nextafter(gap, INF) and g[at["next_above"], 0] > gap
    assert np.isnan(g[at["nan_head"], 0]) and mins[at["nan_head"]] == F32(0.5), "a NaN gap is left out of the minimum and selects nothing"
    assert np.isnan(g[at["nan_and_tie"], 0]) and mins[at["nan_and_tie"]] == 0, "... and hides no tie of another head"
    assert mins[at["wide"]] == F32(0.5)
    if columns:
        assert np.isinf(g[at["all_early"], 4]) and g[at["one_base_left"], 4] == 0
        assert g[at["base_t_tie"], 4] == 0 and g[at["base_t_early"], 4] == F32(0.9) - F32(0.5)
        assert (g[:at["all_early"], 4] == F32(0.9) - F32(0.1)).all()
    lg, lsel, lmin = loop_rule(rows, nout, gap)
    assert same(g, lg) and same(idx, lsel) and same(mins, lmin)
    # the selection at gap = 0 is exactly the rows with a tie
    assert same(syn.refine_select(rows, nout, 0.0)[0], np.array([i for i, n in enumerate(names) if n in ("duplicate", "nan_and_tie", "one_base_left", "base_t_tie")], np.int32))
    # every row with a NaN in every head and no decoder gap: the minimum is what is left
    allnan = np.full((1, nout), NAN, F32)
    assert np.isnan(syn.refine_gaps(allnan, nout)[0, :len(syn.head_slices(nout))]).all() and len(syn.refine_select(allnan, nout, 2.0)[0]) == 0
    assert len(syn.refine_select(np.zeros((0, nout), F32), nout, 1.0)[0]) == 0
    with pytest.raises(ValueError):
        syn.refine_gaps(np.zeros((2, nout + 1), F32), nout)


def test_constants_and_rule_of_the_headers():
    src, dec = open(REFINE_H).read(), open(DECODE_H).read()
    assert int(re.search(r"constexpr int kDecodeCols = (\d+);", dec).group(1)) == syn.DECODE_COLS == Clair3_P.DECODE_COLS
    assert "[22]     early-exit bits" in dec and "[9..12]  homo_Ref probability" in dec, "the decoder columns the rule reads"
    assert "cols[22]" in src and "cols[9 + h]" in src and "cols[c - 1]" in src
    assert "h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57" in src, "the heads of syn.head_slices"
    assert syn.head_slices(90) == [(0, 21), (21, 24), (24, 57), (57, 90)]
    assert int(re.search(r"constexpr size_t kRefineRecordBytes = (\d+);", src).group(1)) == 256
    assert 'section(".c3_refine_text")' in src and src.count("C3_REFINE_TEXT void") == 4, "every kernel of the mode in its own section"
    for word in ("Stated limit", "A NaN gap selects nothing", "ascending"):
        assert word in src, word


def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    comment = src[:src.index("} c3_refine_stats;")].rsplit("/* ----", 1)[1]
    for word in ("DESIGN.md 4", "Errors:", "c3_refine.h", "Off (the default)", "Stated limit", "batches_skipped"):
        assert word in comment, word


def test_stats_struct_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} c3_refine_stats;", src).group(1)
    ctypes_of = {"int64_t": ctypes.c_int64, "float": ctypes.c_float}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for name in names.split(","):
            m = re.fullmatch(r"(\w+)((?:\[\d+\])*)", name.strip())
            t = ctypes_of[ctype]
            for dim in reversed(re.findall(r"\[(\d+)\]", m.group(2))):
                t = t * int(dim)
            want.append((m.group(1), t))
    assert [(n, t) for n, t in _lib.RefineStats._fields_] == want
    assert [n for n, _ in want] == ["batches", "batches_refined", "batches_skipped", "windows", "windows_selected", "windows_changed", "head_selected",
                                    "decoder_selected", "min_gap", "max_abs_diff", "gap"]
    assert ctypes.sizeof(_lib.RefineStats) == 112 and _lib.RefineStats.min_gap.offset == 88


def test_environment_switch(monkeypatch):
    for value, want in ((None, None), ("", None), ("  ", None), ("0", None), ("0.0", None), ("1e-4", 1e-4), (" 0.5 ", 0.5), ("2", 2.0)):
        assert predict.parse_refine_env(value) == want, value
    for value in ("yes", "-1e-4", "nan", "inf", "1e-4,replace"):
        with pytest.raises(_lib.C3Error, match="C3HIP_REFINE"):
            predict.parse_refine_env(value)

    class Model:
        """records what the environment asks of a model"""
        _exact, _handle = False, None

        def __init__(self):
            self.calls = []

        def exact(self, enable=True):
            self._exact = True
            self.calls.append(("exact", enable))

        def refine(self, gap):
            self.calls.append(("refine", gap))

    for name in ("C3HIP_REFINE", "C3HIP_VERIFY", "C3HIP_EXACT", "C3HIP_ANSWER", "C3HIP_VERIFY_REF"):
        monkeypatch.delenv(name, raising=False)
    m = Model()
    assert predict.exact_from_env(m) is False and predict.refine_from_env(m) is False and m.calls == []
    monkeypatch.setenv("C3HIP_REFINE", "0")
    assert predict.exact_from_env(m) is False and predict.refine_from_env(m) is False and m.calls == []
    monkeypatch.setenv("C3HIP_REFINE", "1e-4")
    registered = len(predict._REFINED)
    assert predict.exact_from_env(m) is True, "C3HIP_REFINE implies C3HIP_EXACT=1"
    assert predict.refine_from_env(m) is True and m.calls == [("exact", True), ("refine", 1e-4)]
    assert len(predict._REFINED) == registered + 1 and predict._REFINED[-1] is m, "held for the summary line at exit"
    assert predict.refine_from_env(m) is True and len(predict._REFINED) == registered + 1
    predict._REFINED.remove(m)
    monkeypatch.setenv("C3HIP_VERIFY", "4")
    with pytest.raises(_lib.C3Error, match="C3HIP_REFINE and C3HIP_VERIFY"):
        predict.refine_from_env(Model())
    monkeypatch.setenv("C3HIP_VERIFY", "0")
    assert predict.refine_from_env(Model()) is True
    predict._REFINED.pop()
    monkeypatch.setenv("C3HIP_REFINE", "often")
    for call in (predict.exact_from_env, predict.refine_from_env):
        with pytest.raises(_lib.C3Error, match="C3HIP_REFINE"):
            call(Model())


def test_summary_line():
    class Model:
        def refine_stats(self):
            return dict(batches=7, batches_refined=2, batches_skipped=1, windows=600, windows_selected=3, windows_changed=1, head_selected=[1, 2, 0, 0],
                        decoder_selected=1, min_gap=[2.5e-5, 1e-6, float("inf"), float("inf")], max_abs_diff=3.5e-6, gap=1e-4)

    assert predict.refine_summary(Model()) == ("[clair3_amd] refine: gap=0.0001 batches=7 refined=2 skipped=1 windows=600 selected=3 changed=1 per_head=1/2/0/0 "
                                               "decoder=1 min_gap=2.5e-05/1e-06/inf/inf max_abs_diff=3.5e-06")


def test_null_handle_and_no_device_errors():
    L = _lib.lib()
    st, n = _lib.RefineStats(), ctypes.c_int64(5)
    assert L.c3_model_set_refine(None, 1, 1e-4) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_model_refine_stats(None, ctypes.byref(st)) != 0 and b"null argument" in L.c3_last_error()
    assert L.c3_model_refine_reset(None) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_refine_select(None, None, 24, 0, 1e-4, None, ctypes.byref(n), None) != 0 and b"null model" in L.c3_last_error()
    for cls in (Clair3_P, Clair3_F):
        m = cls(add_indel_length=True, predict=True)
        for call in (m.refine, m.refine_stats, m.refine_reset, lambda: m.refine_select(np.zeros((1, 90), F32), 1e-4)):
            with pytest.raises(_lib.C3Error, match="no device"):
                call()
