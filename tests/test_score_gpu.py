"""Score mode on the device (csrc/c3_score.h; needs an MI355X): the focal loss and arg-max accuracy of labelled windows, evaluated by
rows_score_kernel / rows_score_final_kernel on the rows of a batch where they are.

  1  own rows: the windows' values against synthetic.focal_scores on the library's OWN float32 rows of the same call, the record's sums
     and counts -- both networks, 2 and 4 tasks, batches of 1, 3, 65, 257 windows and one beyond the block cap, int8 and float32 labels,
     with and without class weights, gamma 2 and 0;
  2  the reference fixtures (tests/golden/score_*.npz): per window within the first-order propagation of the measured row difference;
  3  the rows of a scored batch are the predict rows; without rows the record and the values are the same bits;
  4  c3_score_rows on the hand-made rows;
  5  the record does not depend on lanes, slots or on who computed the rows;
  6  the range guard, both policies: scored on the rows the batch is answered with;
  7  errors; off means off.
Nothing of the reference checkout is read."""
import ctypes as C

import numpy as np
import pytest

from clair3_amd import _lib, evaluate, synthetic as syn
from tests import util
from tests.test_calibration import recipe_state_dict
from tests.test_parity_gpu import make_model
from tests.test_score import EPOCH_BATCH, REF_F32, _loader, fixture

pytestmark = pytest.mark.gpu

NETS = {"pileup_2": (syn.PILEUP, 18, False), "pileup_4": (syn.PILEUP, 18, True), "fa_2": (syn.FULL_ALIGNMENT, 8, False), "fa_4": (syn.FULL_ALIGNMENT, 8, True)}
SIZES = (1, 3, 65, 257)  # less than one group of 64 windows, a ragged block, more than one block partial, a ragged last block
_cache = {}


def _clean_env(monkeypatch):
    for k in ("C3HIP_FP32", "C3HIP_AUTO_FP32", "C3HIP_VERIFY", "C3HIP_RING_LANES", "C3HIP_PACK_ROWS", "C3HIP_RANGE_GUARD"):
        monkeypatch.delenv(k, raising=False)


def net(name, monkeypatch):
    """(handle, 257 windows, their rows by predict_numpy): built once per network"""
    _clean_env(monkeypatch)
    if name not in _cache:
        kind, ch, indel = NETS[name]
        m = make_model(kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=811))
        x = syn.make_windows(kind, max(SIZES), seed=812, channels=ch)
        _cache[name] = (m, x, m.predict_numpy(x))
    return _cache[name]


def make_labels(y, seed, soft=False):
    """one-hot per task: half of the windows carry the row's arg-max, half a random class; soft: float32, mass spread over the task"""
    rng = np.random.default_rng(seed)
    B, nout = y.shape
    labels = np.zeros((B, nout), np.float32 if soft else np.int8)
    for lo, hi in syn.head_slices(nout):
        cls = np.where(rng.random(B) < 0.5, y[:, lo:hi].argmax(1), rng.integers(0, hi - lo, size=B))
        labels[np.arange(B), lo + cls] = 1
        if soft:
            labels[:, lo:hi] = 0.8 * labels[:, lo:hi] + 0.2 * rng.random((B, hi - lo)).astype(np.float32)
    return labels


def assert_own_rows(r, rows, labels, gamma, weights, what):
    """a ScoreResult against the numpy rule on the rows the same call returned"""
    want = syn.focal_scores(rows, labels, gamma=gamma, class_weights=weights)
    L, W = r.window_loss.astype(np.float64), want["window_loss"]
    assert r.window_loss.dtype == np.float32 and L.shape == W.shape
    assert np.array_equal(np.isnan(L), np.isnan(W)), what
    ok = ~np.isnan(W)
    err, bound = np.abs(L[ok] - W[ok]), 2.0 ** -23 * np.abs(W[ok]) + 1e-30  # one float32 rounding of a double result, slack for the double log
    print(f"{what}: values: worst |d| / bound {float((err / bound).max()) if err.size else 0:.3f}; sums device {list(r.loss_sum)} numpy {list(want['loss_sum'])} "
          f"correct {list(r.correct)} nonfinite {r.nonfinite}")
    assert (err <= bound).all(), what
    B = len(rows)
    for t in range(want["tasks"]):
        if np.isnan(want["loss_sum"][t]):
            assert np.isnan(r.loss_sum[t]), what
        else:
            assert abs(r.loss_sum[t] - want["loss_sum"][t]) <= B * 2.0 ** -52 * abs(want["loss_sum"][t]), (what, t, r.loss_sum[t], want["loss_sum"][t])
    assert list(r.correct) == list(want["correct"]) and r.nonfinite == want["nonfinite"] and r.windows == B, what


# ------------------------------------------------------------------------------------------------ 1: own rows
@pytest.mark.parametrize("name", list(NETS))
def test_own_rows(name, monkeypatch):
    m, x, y = net(name, monkeypatch)
    nout = m.output_size
    weights = evaluate.class_weights(np.random.default_rng(813).integers(1, 6000, size=nout))
    for n in SIZES:
        for soft in (False, True):
            labels = make_labels(y[:n], 814 + n, soft)
            for w in (None, weights):
                for gamma in (2.0, 0.0):
                    r = m.score(x[:n], labels, class_weights=w, gamma=gamma, window_loss=True, rows=True)
                    assert np.array_equal(r.rows, y[:n]), "the rows of a scored batch are the predict rows"
                    assert_own_rows(r, r.rows, labels, gamma, w, f"{name} B={n} soft={soft} weights={w is not None} gamma={gamma}")
    assert f" score=gamma:0,weights:1" in m.describe(), m.describe()
    assert 0 < r.accuracy.min() and r.accuracy.max() < 1, "the labels make both outcomes occur"


def test_a_block_scores_a_second_group(monkeypatch):
    """a pileup batch beyond 1024 workgroups x 64 windows: the grid-stride loop under the block cap"""
    m, x, y = net("pileup_2", monkeypatch)
    n = 1024 * 64 + 70
    idx = np.arange(n) % len(x)
    labels = make_labels(y[idx], 815)
    r = m.wait_score(m.submit_score(x[idx], labels, slot=1, window_loss=True, rows=True))
    assert np.array_equal(r.rows, y[idx])
    assert_own_rows(r, r.rows, labels, 2.0, None, f"pileup B={n}")


# ------------------------------------------------------------------------------------------------ 2: the reference fixtures
@pytest.mark.parametrize("case", ["pileup_realistic", "pileup_indel_heads", "fa_realistic", "fa_no_indel_heads"])
def test_reference_fixtures(case, monkeypatch, golden_manifest):
    _clean_env(monkeypatch)
    meta, f = golden_manifest[case], fixture(case)
    sd, x = util.case_inputs(meta)
    m = make_model(meta["kind"], meta["channels"], meta["add_indel_length"], sd, depth=meta.get("depth"))
    y_ref, labels = f["rows"], f["labels"]
    for tag, w in (("", None), ("_w", f["weights"])):
        r = m.score(x, labels, class_weights=w, window_loss=True, rows=True)
        lo_c, hi_c = np.float32(1e-9), np.float32(1.0)
        pl, pr = np.clip(r.rows[:, :y_ref.shape[1]], lo_c, hi_c).astype(np.float64), np.clip(y_ref, lo_c, hi_c).astype(np.float64)
        pt, dp = np.minimum(pl, pr), np.abs(pl - pr)
        yy = labels.astype(np.float64) ** 2
        on = yy > 0
        assert (dp[on] <= 0.05 * pt[on]).all(), f"{case}: the first-order bound needs |dp| <= 0.05 p at the labelled columns (worst {float((dp[on] / pt[on]).max()):.3e})"
        ww = np.ones(y_ref.shape[1]) if w is None else w.astype(np.float64)
        terms = ww[None, :] * yy * (2 * np.abs(np.log(pt)) + 1 / pt) * dp
        bound = 1.05 * np.stack([terms[:, lo:hi].sum(1) for lo, hi in syn.head_slices(y_ref.shape[1])], axis=1)
        # L_lib: the window's UNROUNDED value, read as the record's sum of a batch of that one window (c3_score_rows on the rows of this call).
        # The float32 value the batch reports is that double rounded once -- checked exactly -- and is not what the bound is applied to: where
        # a labelled probability equals the reference's bit for bit the bound is 0, which no value rounded to float32 can meet against a
        # double (measured: 18 of 96 values of pileup_realistic, by at most 1.9e-7 = 2^-24 |L|).  What remains beside the propagated row
        # difference is the double arithmetic itself, log and three products on either side: 4 units in the last place of a double
        unrounded = np.stack([m.score_rows(r.rows[i:i + 1], labels[i:i + 1], class_weights=w).loss_sum for i in range(len(x))])
        assert np.array_equal(unrounded.astype(np.float32), r.window_loss), f"{case}{tag}: the reported values are the doubles rounded once"
        bound = bound + 2.0 ** -50 * np.abs(f["loss_f64" + tag])
        err = np.abs(unrounded - f["loss_f64" + tag])
        over = err > bound
        print(f"{case}{tag}: max |dY| {float(np.abs(r.rows.astype(np.float64) - y_ref).max()):.3e}; per window |L_lib - L_ref64| max {float(err.max()):.3e}, "
              f"bound min {float(bound.min()):.3e} max {float(bound.max()):.3e}, windows x tasks over the bound {int(over.sum())} of {over.size}, "
              f"worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, worst excess {float((err - bound).max()):.3e}")
        assert not over.any(), f"{case}{tag}: {int(over.sum())} values beyond the propagated row difference"
        # the epoch value over batches of 7 windows: the sum of those bounds as the epoch weighs them, plus the float32 bound of the recorded value
        got = evaluate.run_validation_epoch(m, [(x[idx], lab) for idx, lab in _loader(labels)], class_weights=w)
        batches = [bound[i:i + EPOCH_BATCH] for i in range(0, len(bound), EPOCH_BATCH)]
        eb = sum(float(b.sum()) / len(b) for b in batches) / len(batches)
        ref = float(f["epoch_ref" + tag])
        tol = eb + (REF_F32 + (np.log2(EPOCH_BATCH) + 8) * 2.0 ** -24) * abs(ref)
        print(f"{case}{tag}: epoch {got:.9g} recorded {ref:.9g} |d| {abs(got - ref):.3e} bound {tol:.3e}")
        assert abs(got - ref) <= tol


# ------------------------------------------------------------------------------------------------ 3: with and without rows
@pytest.mark.parametrize("name", ["pileup_4", "fa_2"])
def test_without_rows_the_same_bits(name, monkeypatch):
    m, x, y = net(name, monkeypatch)
    labels = make_labels(y, 816)
    for n in (65, 257):
        a = m.score(x[:n], labels[:n], window_loss=True, rows=True)
        b = m.score(x[:n], labels[:n], window_loss=True, rows=False)
        c = m.score(x[:n], labels[:n])
        assert b.rows is None and c.rows is None and c.window_loss is None
        assert np.array_equal(a.window_loss, b.window_loss)
        for other in (b, c):
            assert np.array_equal(a.loss_sum, other.loss_sum) and np.array_equal(a.correct, other.correct) and a.nonfinite == other.nonfinite == 0
            assert a.loss == other.loss and a.windows == other.windows == n
    # the blocking call of two chunks or more (256 full-alignment / 4096 pileup windows) adds the chunks' records up in chunk order: the same
    # values and counts as ONE batch of the ring, sums within the rounding of the order
    n = 9000 if NETS[name][0] == syn.PILEUP else 600
    idx = np.arange(n) % len(x)
    cut = m.score(x[idx], labels[idx], window_loss=True, rows=True)
    whole = m.wait_score(m.submit_score(x[idx], labels[idx], slot=3, window_loss=True, rows=True))
    assert np.array_equal(cut.rows, whole.rows) and np.array_equal(cut.window_loss, whole.window_loss) and np.array_equal(cut.correct, whole.correct)
    assert cut.windows == whole.windows == n and np.allclose(cut.loss_sum, whole.loss_sum, rtol=n * 2.0 ** -52, atol=0)
    assert_own_rows(cut, cut.rows, labels[idx], 2.0, None, f"{name} blocking call of {n} windows")


# ------------------------------------------------------------------------------------------------ 4: given rows
def test_score_rows_on_the_hand_made_rows(monkeypatch):
    m, _, _ = net("pileup_4", monkeypatch)
    f = fixture("handmade")
    rows, labels = f["rows"], f["labels"]
    for tag, w in (("", None), ("_w", f["weights"])):
        r = m.score_rows(rows, labels, class_weights=w)
        assert_own_rows(r, rows, labels, 2.0, w, f"hand-made rows{tag}")
        L = r.window_loss
        top = np.float32(-np.log(np.float64(np.float32(1e-9))) * (1.0 - np.float64(np.float32(1e-9))) ** 2)
        if w is None:
            assert abs(float(top) - 20.7233) < 1e-4 and (L[[1, 2, 8, 10]] == top).all(), "p = 0, 1e-12, -inf and the clamp itself"
        assert (L[0] == 0).all() and (L[9] == 0).all(), "p = 1 and p just above 1: a zero term"
        assert np.isnan(L[3]).all() and np.isnan(L[4]).all() and np.isnan(r.loss_sum).all(), "a NaN is not hidden"
        assert r.nonfinite == 4 and r.windows == len(rows)
        close_to_ref = np.abs(L.astype(np.float64) - f["loss_ref" + tag])
        ok = ~np.isnan(f["loss_ref" + tag])
        assert (close_to_ref[ok] <= (REF_F32 + 2.0 ** -24) * np.abs(f["loss_ref" + tag][ok])).all(), "the reference's float32 values"
    # ties: rows 5 and 6 hold their maximum twice; the lowest index counts
    for row, want in ((5, 1), (6, 0)):
        one = m.score_rows(rows[row:row + 1], labels[row:row + 1])
        assert list(one.correct) == [want] * 4 and one.windows == 1
    # rows wider than the model's outputs: the first columns count; float32 labels of the same values: the same record
    wide = np.concatenate([rows, np.full((len(rows), 31), np.nan, np.float32)], axis=1)
    a, b, c = m.score_rows(rows, labels), m.score_rows(wide, labels), m.score_rows(rows, labels.astype(np.float32))
    for other in (b, c):
        assert np.array_equal(a.window_loss, other.window_loss, equal_nan=True) and np.array_equal(a.correct, other.correct) and a.nonfinite == other.nonfinite
    empty = m.score_rows(rows[:0], labels[:0])
    assert empty.windows == 0 and (empty.loss_sum == 0).all() and empty.loss == 0.0


# ------------------------------------------------------------------------------------------------ 5: the record is stable
def _same_record(a, b, what):
    assert a.loss_sum.tobytes() == b.loss_sum.tobytes() and np.array_equal(a.correct, b.correct) and a.nonfinite == b.nonfinite and a.windows == b.windows, what
    if a.window_loss is not None and b.window_loss is not None:
        assert a.window_loss.tobytes() == b.window_loss.tobytes(), what


@pytest.mark.parametrize("name", ["pileup_2", "fa_4"])
def test_record_across_lanes_slots_and_forms(name, monkeypatch):
    m, x, y = net(name, monkeypatch)
    kind, ch, indel = NETS[name]
    labels = make_labels(y, 817)
    n = 130
    base = m.score(x[:n], labels[:n], window_loss=True, rows=True)
    # four batches in flight in the four slots (dealt to the ring's lanes in submit order): each the record of the blocking call
    tickets = [m.submit_score(x[:n], labels[:n], slot=s, window_loss=True) for s in range(4)]
    for s, t in enumerate(tickets):
        _same_record(base, m.wait_score(t), f"{name} slot {s}")
    # one lane
    monkeypatch.setenv("C3HIP_RING_LANES", "1")
    one = make_model(kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=811))
    assert "ring_lanes=1" in one.describe() and "ring_lanes=1" not in m.describe()
    tickets = [one.submit_score(x[:n], labels[:n], slot=s, window_loss=True) for s in range(2)]
    for s, t in enumerate(tickets):
        _same_record(base, one.wait_score(t), f"{name} one lane, slot {s}")
    # the fp32 forms' rows, scored where they are and handed over as rows
    monkeypatch.setenv("C3HIP_FP32", "1")
    f32 = make_model(kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=811))
    r = f32.score(x[:n], labels[:n], window_loss=True, rows=True)
    assert "on_fp32=1" in f32.describe()
    _same_record(r, m.score_rows(r.rows, labels[:n]), f"{name} fp32 forms against c3_score_rows")
    _same_record(base, m.score_rows(base.rows, labels[:n]), f"{name} product forms against c3_score_rows")


# ------------------------------------------------------------------------------------------------ 6: the range guard
@pytest.mark.parametrize("policy", [None, "recalibrate"])
def test_range_guard_scores_the_rows_that_answer(policy, monkeypatch, capfd):
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
    plain = handle()
    s7 = plain.predict_numpy(x7)  # what the guard answers this batch with
    assert np.isfinite(s7).all()
    labels = make_labels(s7, 818)
    for rows in (True, False):
        m = handle()
        capfd.readouterr()
        r = m.score(x7, labels, window_loss=True, rows=rows)
        assert "libc3hip: activations beyond" in capfd.readouterr().err, "the batch tripped the guard"
        if rows:
            assert np.array_equal(r.rows, s7)
        assert_own_rows(r, s7, labels, 2.0, None, f"range guard policy={policy} rows={rows}")
        assert r.nonfinite == 0
        if policy is None:
            assert m.range_status()[1] and "precision=fp32-range-guard" in m.describe()
        else:
            assert "range_guard=recalibrate,recalibrations:1" in m.describe() and "precision=fp16x3" in m.describe()


# ------------------------------------------------------------------------------------------------ 7: errors; off means off
def test_errors(monkeypatch):
    m, x, y = net("pileup_2", monkeypatch)
    kind, ch, indel = NETS["pileup_2"]
    fresh = make_model(kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=811))
    L, rec = _lib.lib(), _lib.ScoreResult()
    labels = make_labels(y[:3], 819)
    rows = np.ascontiguousarray(y[:3])
    wl = np.zeros((3, 2), np.float32)
    x3 = np.ascontiguousarray(x[:3])
    for rc in (L.c3_score_rows(fresh._handle, rows.ctypes.data, 24, 3, labels.ctypes.data, _lib.DTYPE_I8, C.byref(rec), wl.ctypes.data),
               L.c3_score(fresh._handle, x3.ctypes.data, _lib.DTYPE_I8, 3, labels.ctypes.data, _lib.DTYPE_I8, None, None, C.byref(rec)),
               L.c3_score_submit(fresh._handle, x3.ctypes.data, _lib.DTYPE_I8, 3, labels.ctypes.data, _lib.DTYPE_I8, None, None, 0)):
        assert rc != 0 and "score mode is off" in _lib.last_error() and "c3_model_set_score" in _lib.last_error()
    assert L.c3_score_wait(fresh._handle, 0, C.byref(rec)) != 0 and "nothing in flight" in _lib.last_error()
    assert L.c3_model_set_score(fresh._handle, 1, -1.0, None) != 0 and "gamma" in _lib.last_error()
    assert L.c3_model_set_score(fresh._handle, 1, float("nan"), None) != 0 and "gamma" in _lib.last_error()
    bad = np.ones(24, np.float32)
    bad[5] = np.inf
    assert L.c3_model_set_score(fresh._handle, 1, 2.0, bad.ctypes.data) != 0 and "class weight 5" in _lib.last_error()
    assert "score=" not in fresh.describe()
    assert L.c3_model_set_score(fresh._handle, 1, 2.0, None) == 0 and fresh.describe().endswith(" score=gamma:2,weights:0")
    for dt in (_lib.DTYPE_I32, _lib.DTYPE_I64, 9):
        assert L.c3_score_rows(fresh._handle, rows.ctypes.data, 24, 3, labels.ctypes.data, dt, C.byref(rec), None) != 0
        assert "labels must be int8 or float32" in _lib.last_error()
    assert L.c3_score_rows(fresh._handle, rows.ctypes.data, 23, 3, labels.ctypes.data, _lib.DTYPE_I8, C.byref(rec), None) != 0 and "shorter" in _lib.last_error()
    # a slot that holds an unscored batch is not a scored one; c3_predict_wait completes a scored batch as well
    t = fresh.submit(x3, slot=2)
    assert L.c3_score_wait(fresh._handle, 2, C.byref(rec)) != 0 and "not scored" in _lib.last_error()
    assert np.array_equal(fresh.wait(t), y[:3])
    slot, yy, _ = fresh.submit_score(x3, labels, slot=2, rows=True)
    assert np.array_equal(fresh.wait((slot, yy)), y[:3])
    with pytest.raises(_lib.C3Error, match="labels must be"):
        fresh.score(x3, labels[:, :20])
    with pytest.raises(_lib.C3Error, match="label dtype"):
        fresh.score(x3, labels.astype(np.int32))
    assert L.c3_model_set_score(fresh._handle, 0, 0.0, None) == 0 and "score=" not in fresh.describe()


def test_off_means_off(monkeypatch, golden_manifest):
    """without c3_model_set_score: describe(), the rows of a golden case and what the default-off tests of verify mode read are what they were"""
    _clean_env(monkeypatch)
    for case in ("pileup_realistic", "fa_no_indel_heads"):
        meta = golden_manifest[case]
        sd, x = util.case_inputs(meta)
        m = make_model(meta["kind"], meta["channels"], meta["add_indel_length"], sd, depth=meta.get("depth"))
        m.profile(True)
        y = m.predict_numpy(x)
        util.assert_rows_match(y, util.golden_y(case), what=case)
        assert "score" not in m.describe()
        names = [r["name"] for r in m.profile_read()]
        assert names and not [n for n in names if "score" in n], names
        st = m.verify_stats()
        assert st["every"] == 0 and st["batches_submitted"] == 0 and st["batches_checked"] == 0 and st["worst_batch"] == -1, st
        assert m.describe().split()[-1].startswith("chunks=" if meta["kind"] == syn.PILEUP else "pack_rows="), m.describe()


def test_score_launches_are_profiled(monkeypatch):
    """the two launches carry their tags (p.score / fa.score); the windows' values of a profiled batch are the unprofiled ones"""
    for name, tag in (("pileup_2", "p.score"), ("fa_2", "fa.score")):
        m, x, y = net(name, monkeypatch)
        labels = make_labels(y[:65], 820)
        base = m.score(x[:65], labels, window_loss=True)
        m.profile(True)
        try:
            r = m.score(x[:65], labels, window_loss=True)
            recs = {p["name"]: p for p in m.profile_read()}
        finally:
            m.profile(False)
        assert tag in recs and recs[tag]["launches"] == 1 and recs[tag]["total_ms"] > 0, sorted(recs)
        _same_record(base, r, name)
