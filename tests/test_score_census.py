"""The census of score mode (c3_model_set_score_census, csrc/c3_census.h), the part that needs no GPU: the rule in numpy
(synthetic.score_census) against a plain loop over windows and on the fixtures of score mode, its links to synthetic.focal_scores, the
constants against the header that defines them, the C ABI, evaluate.census_report on a table worked out by hand, and the validation-epoch
hook over a stand-in handle.  (The host code -- plan_batch with the census section, the accumulation -- is exercised without a device by
the stand-alone program tests/host/census_host_check.cpp, built with -fsanitize=address,undefined as its head says.)"""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest

from clair3_amd import _lib, evaluate, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import util
from tests.test_abi import HEADER, declared_symbols
from tests.test_score import CASES, fixture

ENTRIES = ("c3_model_set_score_census", "c3_score_census_read", "c3_score_census_reset")
CENSUS_H = os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_census.h")
ARRAYS = ("rel_windows", "rel_correct", "rel_conf_q32", "rel_skipped", "gap_below")


def same_census(a, b, what=""):
    assert a.windows == b.windows and a.tasks == b.tasks, (what, a.windows, b.windows, a.tasks, b.tasks)
    for t in range(4):
        assert np.array_equal(a.confusion[t], b.confusion[t]), (what, "confusion", t)
    for name in ARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name, getattr(a, name), getattr(b, name))


def loop_census(rows, labels):
    """the rule of csrc/c3_census.h window by window, column by column, as the kernel walks them"""
    heads = syn.head_slices(labels.shape[1])
    out = syn.empty_census(len(heads))._replace(windows=len(rows))
    thr = [np.float32(v) for v in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)]
    ninf = np.float32(-np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(rows)):
            for t, (lo, hi) in enumerate(heads):
                pm, ym, pi, yi = ninf, ninf, 0, 0
                for c in range(lo, hi):
                    pv, yv = np.float32(rows[r, c]), np.float32(labels[r, c])
                    if pv > pm:
                        pm, pi = pv, c - lo
                    if yv > ym:
                        ym, yi = yv, c - lo
                second = ninf
                for c in range(lo, hi):
                    pv = np.float32(rows[r, c])
                    if c - lo != pi and pv > second:
                        second = pv
                out.confusion[t][yi, pi] += 1
                conf = pm
                if np.isfinite(conf) and np.float32(0) <= conf <= np.float32(1):
                    b = min(19, int(np.float32(conf * np.float32(20.0))))
                    out.rel_windows[t, b] += 1
                    out.rel_correct[t, b] += int(pi == yi)
                    out.rel_conf_q32[t, b] += round(float(conf) * 4294967296.0)  # (exact product; round: to nearest, halves to even)
                else:
                    out.rel_skipped[t] += 1
                gap = np.float32(conf - second)
                for k in range(6):
                    out.gap_below[t, k] += int(gap < thr[k])
    return out


def nasty_rows(B, nout, seed):
    """soft-max like rows with the corners sprinkled in: NaN, +-inf, values above 1 and below 0, exact ties, near ties at every threshold"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((B, nout), np.float32)
    labels = np.zeros((B, nout), np.int8)
    for lo, hi in syn.head_slices(nout):
        n = hi - lo
        p = rng.random((B, n)).astype(np.float32) ** 6
        p /= p.sum(1, keepdims=True)
        for r in range(B):
            kind = r % 12
            a, b = rng.choice(n, size=2, replace=False)
            if kind == 1:
                p[r, a] = np.nan
            elif kind == 2:
                p[r] = np.nan
            elif kind == 3:
                p[r, a] = np.inf
            elif kind == 4:
                p[r, a] = -np.inf
            elif kind == 5:
                p[r, a] = 1.5
            elif kind == 6:
                p[r] = -np.abs(p[r]) - 0.25
            elif kind == 7:
                p[r, a] = p[r, b] = p[r].max()
            elif kind == 8:
                p[r, a] = 0.5
                p[r, b] = np.float32(0.5) - np.float32(10.0 ** -rng.integers(1, 8))
            elif kind == 9:
                p[r] = 0.0
                p[r, a] = 1.0
        rows[:, lo:hi] = p
        labels[np.arange(B), lo + np.where(rng.random(B) < 0.5, np.nan_to_num(p, nan=-1).argmax(1), rng.integers(0, n, size=B))] = 1
    return rows, labels


# ------------------------------------------------------------------------------------------------ the rule
def test_constants_are_the_headers():
    src = open(CENSUS_H).read()
    assert int(re.search(r"constexpr int kScoreCensusBins = (\d+);", src).group(1)) == syn.CENSUS_BINS == 20
    assert int(re.search(r"constexpr int kScoreCensusGaps = (\d+);", src).group(1)) == len(syn.CENSUS_GAP_THR) == 6
    assert float(re.search(r"constexpr double kScoreCensusConfUnit = ([\d.]+);", src).group(1)) == syn.CENSUS_CONF_UNIT == 2.0 ** 32
    thr = re.search(r"thr\[kScoreCensusGaps\] = \{([^}]*)\}", src).group(1)
    assert [np.float32(v.strip().rstrip("f")) for v in thr.split(",")] == list(syn.CENSUS_GAP_THR) and syn.CENSUS_GAP_THR.dtype == np.float32
    off = re.search(r"kScoreCensusCellOff\[4\] = \{([^}]*)\}", src).group(1)
    assert tuple(int(v) for v in off.split(",")) == syn.CENSUS_CELL_OFF == tuple(int(v) for v in np.cumsum([0] + [k * k for k in syn.HEAD_SIZES])[:4])
    assert int(re.search(r"constexpr int kScoreCensusCells = (\d+);", src).group(1)) == sum(k * k for k in syn.HEAD_SIZES) == 2628
    for place in (open(HEADER).read(), syn.score_census.__doc__):
        assert "c3_census.h" in place, "the header and the numpy rule cite the place of the definitions"


@pytest.mark.parametrize("nout", [90, 24])
def test_rule_against_a_loop(nout):
    rows, labels = nasty_rows(96, nout, seed=7100 + nout)
    got, want = syn.score_census(rows, labels), loop_census(rows, labels)
    same_census(got, want, f"nout={nout}")
    assert got.tasks == (4 if nout == 90 else 2) and got.windows == 96
    for t in range(got.tasks):
        assert got.confusion[t].sum() == 96 and got.rel_windows[t].sum() + got.rel_skipped[t] == 96
        assert got.rel_skipped[t] >= 4 * 8 and (np.diff(got.gap_below[t]) >= 0).all() and got.gap_below[t, 0] >= 8, "the corners occur"
    for t in range(got.tasks, 4):
        assert not got.confusion[t].any() and not got.rel_windows[t].any() and not got.gap_below[t].any() and got.rel_skipped[t] == 0
    # rows wider than the labels: the first columns count; float32 labels of the same values: the same census
    wide = np.concatenate([rows, np.full((len(rows), 31), np.nan, np.float32)], axis=1)
    same_census(syn.score_census(wide, labels), got)
    same_census(syn.score_census(rows, labels.astype(np.float32)), got)
    # integers: the census of a batch is the sum of the censuses of its parts
    parts = [syn.score_census(rows[i:i + 37], labels[i:i + 37]) for i in range(0, 96, 37)]
    assert sum(p.windows for p in parts) == 96
    for name in ARRAYS:
        assert np.array_equal(sum(getattr(p, name) for p in parts), getattr(got, name)), name
    assert all(np.array_equal(sum(p.confusion[t] for p in parts), got.confusion[t]) for t in range(4))
    empty = syn.score_census(rows[:0], labels[:0])
    assert empty.windows == 0 and empty.tasks == got.tasks and not any(c.any() for c in empty.confusion)
    with pytest.raises(ValueError):
        syn.score_census(rows[:, :20], labels)
    with pytest.raises(ValueError):
        syn.score_census(rows[:5], labels)


def test_handmade_corners():
    """make_golden_score.py handmade_rows: the same treatment in every task"""
    f = fixture("handmade")
    rows, labels = f["rows"], f["labels"]
    got = syn.score_census(rows, labels)
    same_census(got, loop_census(rows, labels), "handmade")
    one = [syn.score_census(rows[i:i + 1], labels[i:i + 1]) for i in range(len(rows))]
    for t, k in enumerate(syn.HEAD_SIZES):
        truth = labels[:, syn.head_slices(90)[t][0]:syn.head_slices(90)[t][1]].argmax(1)
        # p = 1 at the true class: the last bin, the whole unit, a gap of 1
        assert one[0].rel_windows[t, 19] == 1 and one[0].rel_correct[t, 19] == 1 and one[0].rel_conf_q32[t, 19] == 2 ** 32 and not one[0].gap_below[t].any()
        # a NaN row: index 0, no confidence, no gap
        assert one[3].confusion[t][truth[3], 0] == 1 and one[3].rel_skipped[t] == 1 and not one[3].rel_windows[t].any() and not one[3].gap_below[t].any()
        # one NaN beside the true class: counted like any window
        assert one[4].rel_windows[t].sum() == 1 and one[4].rel_skipped[t] == 0
        # ties at columns 1 and 2: the lower index is the prediction, the gap is 0 -- below every threshold
        for row, tr, ok in ((5, 1, 1), (6, 2, 0)):
            assert one[row].confusion[t][tr, 1] == 1 and (one[row].gap_below[t] == 1).all(), (row, t)
            assert one[row].rel_windows[t, 8] == 1 and one[row].rel_correct[t, 8] == ok  # (0.4f * 20.0f = 8.0f)
            assert one[row].rel_conf_q32[t, 8] == round(float(np.float32(0.4)) * 2 ** 32)
        # +inf beside the true class is the prediction: no bin, an infinite gap counts nowhere
        assert one[7].rel_skipped[t] == 1 and not one[7].gap_below[t].any() and one[7].confusion[t][truth[7], (truth[7] + 1) % k] == 1
        # -inf at the true class: never the prediction
        assert one[8].confusion[t][truth[8]].sum() == 1 and one[8].confusion[t][truth[8], truth[8]] == 0 and one[8].rel_windows[t].sum() == 1
        # just above 1: outside [0, 1]
        assert one[9].rel_skipped[t] == 1 and one[9].confusion[t][truth[9], truth[9]] == 1
        assert got.rel_skipped[t] == 3 and got.rel_windows[t].sum() == len(rows) - 3


@pytest.mark.parametrize("case", CASES)
def test_links_to_the_score_record(case):
    """the trace of a confusion table is the record's count of correct windows, its sum the windows"""
    f = fixture(case)
    for labels in (f["labels"], (0.75 * f["labels"] + 0.25 / 4).astype(np.float32)):  # hard, and soft float32 labels
        c, r = syn.score_census(f["rows"], labels), syn.focal_scores(f["rows"], labels)
        assert c.windows == r["windows"] and c.tasks == r["tasks"] == (2 if f["labels"].shape[1] == 24 else 4)
        for t in range(c.tasks):
            assert np.trace(c.confusion[t]) == r["correct"][t] and c.confusion[t].sum() == c.windows, (case, t)
            assert c.rel_correct[t].sum() <= r["correct"][t] and c.rel_windows[t].sum() + c.rel_skipped[t] == c.windows
        same_census(c, loop_census(f["rows"], labels), case)
    # soft labels that move the label's arg-max move the truth
    soft = f["labels"].astype(np.float32) * 0.4
    soft[:, 0] += 0.5
    assert syn.score_census(f["rows"], soft).confusion[0][0].sum() == len(soft)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    assert src.index("} c3_score_census;") > src.index("int c3_score_rows("), "behind c3_score_rows"
    comment = src[:src.index("} c3_score_census;")].rsplit("/* ----", 1)[1]
    assert "DESIGN.md 4" in comment and "Errors:" in comment and "c3_census.h" in comment and "Off (the default)" in comment


def test_census_struct_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} c3_score_census;", src).group(1)
    ctypes_of = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
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
    assert [(n, t) for n, t in _lib.ScoreCensus._fields_] == want
    assert ctypes.sizeof(_lib.ScoreCensus) == 23184
    assert _lib.ScoreCensus.confusion.offset == 16 and _lib.ScoreCensus.gap_below.offset == 23184 - 4 * 6 * 8


def test_null_handle_and_no_device_errors():
    L = _lib.lib()
    rec = _lib.ScoreCensus()
    assert L.c3_model_set_score_census(None, 1) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_score_census_read(None, ctypes.byref(rec)) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_score_census_reset(None) != 0 and b"null model" in L.c3_last_error()
    for cls in (Clair3_P, Clair3_F):
        m = cls(add_indel_length=True, predict=True)
        for call in (m.score_census, m.census, m.census_reset):
            with pytest.raises(_lib.C3Error, match="no device"):
                call()


# ------------------------------------------------------------------------------------------------ the report
def hand_census():
    """one task of three classes; class 2 has no window but is predicted once.  Two occupied bins: [0.5, 0.55) with 4 windows of confidence
    0.5, two of them correct; [0.95, 1] with 8 windows of confidence 15/16, six of them correct"""
    c = syn.empty_census(1)._replace(windows=12)
    c.confusion[0] = np.array([[5, 1, 0], [2, 3, 1], [0, 0, 0]], np.int64)
    c.rel_windows[0, 10], c.rel_correct[0, 10], c.rel_conf_q32[0, 10] = 4, 2, 4 * 2 ** 31
    c.rel_windows[0, 19], c.rel_correct[0, 19], c.rel_conf_q32[0, 19] = 8, 6, 8 * 15 * 2 ** 28
    c.gap_below[0] = [0, 1, 2, 3, 5, 8]
    return c


def test_report_on_a_hand_written_table():
    rep = evaluate.census_report(hand_census())
    assert rep["windows"] == 12 and len(rep["tasks"]) == 1
    t = rep["tasks"][0]
    assert t["name"] == syn.HEAD_NAMES[0] and t["accuracy"] == 8 / 12
    assert list(t["support"]) == [6, 6, 0]
    assert np.allclose(t["precision"], [5 / 7, 3 / 4, 0.0], rtol=1e-15)
    assert np.allclose(t["recall"][:2], [5 / 6, 3 / 6], rtol=1e-15) and np.isnan(t["recall"][2]), "no window of class 2: a zero denominator is nan"
    assert np.allclose(t["f1"], [10 / 13, 6 / 10, 0.0], rtol=1e-15)
    assert abs(t["macro_f1"] - (10 / 13 + 6 / 10) / 2) < 1e-15, "the mean over the classes with support"
    assert abs(t["ece"] - (4 / 12 * abs(0.5 - 0.5) + 8 / 12 * abs(6 / 8 - 15 / 16))) < 1e-15 and t["ece"] == 0.125
    assert t["binned"] == 12 and t["skipped"] == 0
    assert t["gap_below"] == {"1e-06": 0, "1e-05": 1, "0.0001": 2, "0.001": 3, "0.01": 5, "0.1": 8}
    # nothing at all: every ratio is nan, nothing raises
    nothing = evaluate.census_report(syn.empty_census(2))
    assert len(nothing["tasks"]) == 2 and all(np.isnan(x["accuracy"]) and np.isnan(x["ece"]) and np.isnan(x["macro_f1"]) for x in nothing["tasks"])
    assert np.isnan(nothing["tasks"][1]["precision"]).all()
    plain = evaluate.report_json(rep)
    assert plain["tasks"][0]["recall"][2] is None and plain["tasks"][0]["support"] == [6, 6, 0]
    lines = evaluate.format_census_report(rep)
    assert "ECE 0.125000" in lines[0] and len(lines) == 1 + 3


# ------------------------------------------------------------------------------------------------ the validation epoch
class StandIn:
    """a handle built on the numpy rules: 'windows' are window numbers, their rows the recorded ones"""

    def __init__(self, rows):
        self.rows, self.output_size = rows, rows.shape[1]
        self.on, self.total, self.resets = False, syn.score_census(rows[:3], np.ones((3, rows.shape[1]), np.int8)), 0  # (stale counts)

    def score(self, x, labels, class_weights=None, gamma=2.0):
        r = syn.focal_scores(self.rows[np.asarray(x)], labels, gamma=gamma, class_weights=class_weights)
        if self.on:
            c = syn.score_census(self.rows[np.asarray(x)], labels)
            self.total = self.total._replace(windows=self.total.windows + c.windows, confusion=[a + b for a, b in zip(self.total.confusion, c.confusion)],
                                             **{n: getattr(self.total, n) + getattr(c, n) for n in ARRAYS})
        task = r["loss_sum"] / max(1, r["windows"])
        return types.SimpleNamespace(loss=float(sum(float(v) for v in task)), task_loss=task, windows=r["windows"])

    def score_census(self, enable=True):
        self.on = enable
        return self

    def census(self):
        return self.total

    def census_reset(self):
        self.total, self.resets = syn.empty_census(len(syn.head_slices(self.output_size))), self.resets + 1
        return self


@pytest.mark.parametrize("case", ["pileup_realistic", "fa_realistic"])
def test_validation_epoch_hook_over_a_stand_in(case, monkeypatch):
    f = fixture(case)
    rows, labels = f["rows"], f["labels"]
    loader = [(np.arange(i, min(i + 7, len(labels))), labels[i:i + 7]) for i in range(0, len(labels), 7)]
    plain = evaluate.run_validation_epoch(StandIn(rows), loader, class_weights=f["weights"])
    h, out = StandIn(rows), io.StringIO()
    got = evaluate.run_validation_epoch_with_census(h, loader, class_weights=f["weights"], out=out)
    assert got == plain, "the value of the epoch is unchanged"
    assert h.on and h.resets == 1
    same_census(h.census(), syn.score_census(rows, labels), "the epoch's census starts from zero")
    lines = out.getvalue().splitlines()
    rep = evaluate.census_report(syn.score_census(rows, labels))
    assert len(lines) == len(rep["tasks"]) == (2 if rows.shape[1] == 24 else 4)
    for line, t in zip(lines, rep["tasks"]):
        assert line.startswith(f"[clair3_amd] validation: task={t['name']} windows={len(rows)} accuracy={t['accuracy']:.6f} macro_f1=")
        assert f" ece={t['ece']:.6f} below_1e-4={t['gap_below']['0.0001']}" in line
    # the switch
    for value, want in (("", False), ("0", False), ("1", True), (" 1 ", True)):
        monkeypatch.setenv("C3HIP_SCORE_CENSUS", value)
        assert evaluate.census_from_env() is want
    monkeypatch.delenv("C3HIP_SCORE_CENSUS")
    assert evaluate.census_from_env() is False
    monkeypatch.setenv("C3HIP_SCORE_CENSUS", "yes")
    with pytest.raises(ValueError, match="C3HIP_SCORE_CENSUS"):
        evaluate.census_from_env()
