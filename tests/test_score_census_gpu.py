"""The census of score mode on the device (csrc/c3_census.h; needs an MI355X): rows_census_kernel counts the confusion, reliability and
gap tables of a scored batch from the rows it is answered with, and the handle adds the batch's table to its totals when the batch is
waited for.  Every comparison is exact: the tables are integers, and the numpy rule (synthetic.score_census) is applied to the very rows
the library returned.

  1  c3_score_rows on the hand-made rows;
  2  the reference fixtures' windows through a forward pass, with and without rows; two tasks: the other tables stay zero;
  3  chunking, slots and lanes do not change the totals (a child process: C3HIP_PREDICT_CHUNK is read once per process);
  4  a workgroup takes a second group of windows;
  5  the range guard, both policies: counted once, on the rows that answer;
  6  off means off; the launch is profiled under its own name; errors.
Nothing of the reference checkout is read."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from tests import util
from tests.test_calibration import recipe_state_dict
from tests.test_parity_gpu import make_model
from tests.test_score import fixture
from tests.test_score_census import ARRAYS, same_census
from tests.test_score_gpu import NETS, _clean_env, make_labels, net

pytestmark = pytest.mark.gpu


def fresh(name):
    kind, ch, indel = NETS[name]
    return make_model(kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=811))


def census_of(m, call):
    """the census of what ``call`` scores on m, from zero"""
    m.score_census(True).census_reset()
    r = call()
    return r, m.census()


def links(c, r, what):
    """a census and the record of the same batch"""
    assert c.windows == r.windows, what
    for t in range(c.tasks):
        assert np.trace(c.confusion[t]) == r.correct[t] and c.confusion[t].sum() == r.windows, (what, t)
        assert c.rel_windows[t].sum() + c.rel_skipped[t] == r.windows, (what, t)


# ------------------------------------------------------------------------------------------------ 1: given rows
def test_score_rows_on_the_hand_made_rows(monkeypatch):
    _clean_env(monkeypatch)
    m = fresh("pileup_4")
    f = fixture("handmade")
    rows, labels = f["rows"], f["labels"]
    r, c = census_of(m, lambda: m.score_rows(rows, labels))
    same_census(c, syn.score_census(rows, labels), "hand-made rows")
    links(c, r, "hand-made rows")
    assert c.tasks == 4 and list(c.rel_skipped) == [3] * 4 and (c.gap_below[:, 0] >= 2).all()
    assert m.describe().endswith(" score=gamma:2,weights:0,census:1"), m.describe()
    # float32 labels, rows wider than the outputs, and an empty batch: the totals add up
    wide = np.concatenate([rows, np.full((len(rows), 31), np.nan, np.float32)], axis=1)
    m.score_rows(wide, labels.astype(np.float32))
    m.score_rows(rows[:0], labels[:0])
    twice = m.census()
    assert twice.windows == 2 * len(rows) and all(np.array_equal(twice.confusion[t], 2 * c.confusion[t]) for t in range(4))
    for name in ARRAYS:
        assert np.array_equal(getattr(twice, name), 2 * getattr(c, name)), name
    assert m.census_reset().census().windows == 0 and not m.census().rel_conf_q32.any()


# ------------------------------------------------------------------------------------------------ 2: the reference fixtures
@pytest.mark.parametrize("case", ["pileup_realistic", "pileup_indel_heads", "fa_realistic", "fa_no_indel_heads"])
def test_reference_fixtures(case, monkeypatch, golden_manifest):
    _clean_env(monkeypatch)
    meta, f = golden_manifest[case], fixture(case)
    sd, x = util.case_inputs(meta)
    m = make_model(meta["kind"], meta["channels"], meta["add_indel_length"], sd, depth=meta.get("depth"))
    labels = f["labels"]
    r, c = census_of(m, lambda: m.score(x, labels, rows=True))
    want = syn.score_census(r.rows, labels)
    same_census(c, want, case)
    links(c, r, case)
    assert c.tasks == (4 if meta["add_indel_length"] else 2) and c.windows == len(x)
    for t in range(c.tasks, 4):  # a 24-column model: the tables of the other two tasks stay zero
        assert not c.confusion[t].any() and not c.rel_windows[t].any() and not c.rel_conf_q32[t].any() and not c.gap_below[t].any() and c.rel_skipped[t] == 0
    # without rows: the same record, the same census
    r2, c2 = census_of(m, lambda: m.score(x, labels))
    assert r2.rows is None and np.array_equal(r2.correct, r.correct) and r2.loss_sum.tobytes() == r.loss_sum.tobytes()
    same_census(c2, want, f"{case} without rows")
    # soft float32 labels through the ring
    soft = (0.75 * labels + 0.25 / 4).astype(np.float32)
    soft[::2, 0] += 0.9
    r3, c3 = census_of(m, lambda: m.wait_score(m.submit_score(x, soft, slot=2, rows=True)))
    same_census(c3, syn.score_census(r3.rows, soft), f"{case} soft labels")
    links(c3, r3, f"{case} soft labels")


# ------------------------------------------------------------------------------------------------ 3: chunking, slots, lanes
CHILD = r"""
import json, sys
import numpy as np
from clair3_amd import synthetic as syn
from tests.test_parity_gpu import make_model
from tests.test_score_census import ARRAYS
from tests.test_score_gpu import make_labels

kind, ch, indel = syn.FULL_ALIGNMENT, 8, True
m = make_model(kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=811))
x = syn.make_windows(kind, 20, seed=812, channels=ch)
labels = make_labels(m.predict_numpy(x), 821)
m.score_census(True)

def flat(c):
    return dict(windows=c.windows, tasks=c.tasks, confusion=[a.tolist() for a in c.confusion], **{n: getattr(c, n).tolist() for n in ARRAYS})

out = {}
whole = m.wait_score(m.submit_score(x, labels, slot=0, rows=True))  # one batch of the ring
out["whole"], out["rule"] = flat(m.census()), flat(syn.score_census(whole.rows, labels))
m.census_reset()
cut = m.score(x, labels, rows=True)  # chunks of 8 and 12 windows
out["cut"], out["cut_rows_equal"], out["cut_correct"] = flat(m.census()), bool(np.array_equal(cut.rows, whole.rows)), [cut.correct.tolist(), whole.correct.tolist()]
m.census_reset()
tickets = [m.submit_score(x[a:b], labels[a:b], slot=s) for s, (a, b) in zip((3, 1, 2), ((0, 7), (7, 14), (14, 20)))]  # three lanes, in flight together
for t in reversed(tickets):
    m.wait_score(t)
out["three"] = flat(m.census())
out["describe"] = m.describe()
print("RESULT " + json.dumps(out))
"""


def test_chunks_slots_and_lanes_do_not_change_the_totals(monkeypatch):
    _clean_env(monkeypatch)
    env = dict(os.environ, C3HIP_PREDICT_CHUNK="8", PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=util.ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert out["whole"]["windows"] == 20 and out["whole"]["tasks"] == 4
    assert out["whole"] == out["rule"], "one batch: the numpy rule on its rows"
    assert out["cut_rows_equal"] and out["cut_correct"][0] == out["cut_correct"][1]
    assert out["cut"] == out["whole"], "two chunks (C3HIP_PREDICT_CHUNK=8): the totals of one call"
    assert out["three"] == out["whole"], "three submits on three slots and lanes, waited for in another order"
    assert "ring_lanes=1" not in out["describe"]


# ------------------------------------------------------------------------------------------------ 4: a second group
def test_a_workgroup_takes_a_second_group(monkeypatch):
    """24-column rows, one window beyond 256 workgroups x 64 windows: the first workgroup walks on to a second group of one window"""
    _clean_env(monkeypatch)
    m = fresh("pileup_2")
    n = 256 * 64 + 1
    rng = np.random.default_rng(822)
    rows = rng.random((n, 24)).astype(np.float32) ** 8
    rows /= rows.sum(1, keepdims=True)
    rows[-1] = 0.0
    rows[-1, [3, 22]] = 1.0  # the last window
    rows[5, :21] = np.nan
    labels = make_labels(rows, 823)
    labels[-1] = 0
    labels[-1, [20, 21]] = 1
    r, c = census_of(m, lambda: m.score_rows(rows, labels, window_loss=False))
    head = syn.score_census(rows[:-1], labels[:-1])
    assert c.confusion[0][20, 3] == head.confusion[0][20, 3] + 1 and c.confusion[1][0, 1] == head.confusion[1][0, 1] + 1, "the window of the second group was counted"
    same_census(c, syn.score_census(rows, labels), f"B={n}")
    links(c, r, f"B={n}")
    assert c.tasks == 2 and not c.confusion[2].any() and not c.confusion[3].any()


# ------------------------------------------------------------------------------------------------ 5: the range guard
@pytest.mark.parametrize("policy", [None, "recalibrate"])
def test_range_guard_counts_once_on_the_rows_that_answer(policy, monkeypatch, capfd):
    from clair3_amd.model import Clair3_F
    _clean_env(monkeypatch)
    sd = recipe_state_dict()
    x7 = syn.make_fa_windows(7, seed=63)

    def handle():
        m = Clair3_F(add_indel_length=True, predict=True, input_channels=8).to("cuda:0")
        if policy is not None:
            m.range_policy(policy)
        m.load_state_dict(sd)
        return m
    s7 = handle().predict_numpy(x7)  # what the guard answers this batch with
    assert np.isfinite(s7).all()
    labels = make_labels(s7, 818)
    want = syn.score_census(s7, labels)
    for rows in (True, False):
        m = handle()
        m.score_census(True)
        capfd.readouterr()
        r = m.score(x7, labels, rows=rows)
        assert "libc3hip: activations beyond" in capfd.readouterr().err, "the batch tripped the guard"
        c = m.census()
        assert c.windows == 7, "counted once"
        same_census(c, want, f"range guard policy={policy} rows={rows}")
        links(c, r, f"range guard policy={policy} rows={rows}")
        if policy is None:
            assert "precision=fp32-range-guard" in m.describe()
        else:
            assert "range_guard=recalibrate,recalibrations:1" in m.describe() and "precision=fp16x3" in m.describe()


# ------------------------------------------------------------------------------------------------ 6: off means off; errors
def _profiled(m, x, labels):
    m.profile(True)
    m.profile_reset()
    try:
        r = m.score(x, labels, window_loss=True, rows=True)
        return r, {p["name"]: p["launches"] for p in m.profile_read()}
    finally:
        m.profile_reset()  # (the handle may be one the score tests share: leave no records on it)
        m.profile(False)


@pytest.mark.parametrize("name,tag", [("pileup_2", "p.census"), ("fa_4", "fa.census")])
def test_off_means_off(name, tag, monkeypatch):
    m, x, y = net(name, monkeypatch)  # (a handle of the score tests: score mode on or off, the census never on)
    labels = make_labels(y[:65], 824)
    never, prof_never = _profiled(m, x[:65], labels)
    assert m.describe().endswith(" score=gamma:2,weights:0"), m.describe()
    assert not [n for n in prof_never if "census" in n], prof_never
    rec = _lib.ScoreCensus()
    assert _lib.lib().c3_score_census_read(m._handle, C.byref(rec)) != 0 and "never enabled" in _lib.last_error()
    assert _lib.lib().c3_score_census_reset(m._handle) != 0 and "never enabled" in _lib.last_error()
    h = fresh(name)
    on, prof_on = _profiled(h.score_census(True), x[:65], labels)
    assert h.describe() == m.describe() + ",census:1"
    assert prof_on.pop(tag) == 1 and prof_on == prof_never, "one more launch, under its own name"
    off, prof_off = _profiled(h.score_census(False), x[:65], labels)
    assert h.describe() == m.describe() and prof_off == prof_never
    for other in (on, off):
        assert other.rows.tobytes() == never.rows.tobytes() and other.window_loss.tobytes() == never.window_loss.tobytes()
        assert other.loss_sum.tobytes() == never.loss_sum.tobytes() and np.array_equal(other.correct, never.correct) and other.nonfinite == never.nonfinite
    assert np.array_equal(never.rows, y[:65])
    same_census(h.census(), syn.score_census(on.rows, labels), "only the batch scored while the census was on")


def test_errors(monkeypatch):
    _clean_env(monkeypatch)
    L = _lib.lib()
    m = fresh("pileup_2")
    rec = _lib.ScoreCensus()
    assert L.c3_model_set_score_census(m._handle, 1) != 0 and "c3_model_set_score first" in _lib.last_error()
    assert L.c3_score_census_read(m._handle, C.byref(rec)) != 0 and "score mode is off" in _lib.last_error()
    m.score_mode()
    x = syn.make_windows(syn.PILEUP, 3, seed=825, channels=18)
    labels = np.zeros((3, 24), np.int8)
    labels[:, [0, 21]] = 1
    t = m.submit_score(x, labels, slot=1)
    assert L.c3_model_set_score_census(m._handle, 1) != 0 and "in flight" in _lib.last_error()
    m.wait_score(t)
    assert "census" not in m.describe()
    m.score_census(True)
    assert L.c3_score_census_read(m._handle, None) != 0 and "out" in _lib.last_error()
    assert m.census().windows == 0, "the batch that was in flight while the census was off is not in it"
    with pytest.raises(_lib.C3Error, match="True or False"):
        m.score_census(1)
    m.score_mode(enable=False)
    assert "score" not in m.describe()
    with pytest.raises(_lib.C3Error, match="score mode is off"):
        m.census()
