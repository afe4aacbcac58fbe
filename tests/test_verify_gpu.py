"""Verify mode on the device (csrc/c3_verify.h; need an MI355X): a batch of the submit / wait ring also runs on the fp32-MFMA forms from
the same staged input and rows_compare_kernel compares the two sets of rows where they are.

  1  report mode changes no row, and the selection rule counts what it says;
  2  the record is the truth: recomputed in numpy from the rows of two more handles (C3HIP_FP32=0 and =1), no tolerance;
  3  the policy acts on exactly what it measured;
  4  range guard, keep mode, profiling, reload, three slots in flight;
  5  off means off.
Every weight set and window comes from clair3_amd/synthetic.py."""
import numpy as np
import pytest

from clair3_amd import _lib, predict, synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model

pytestmark = pytest.mark.gpu

# the batch of tests/diag/sensitive_window.py: synthetic._trained_like pileup weights with the +-8 LSTM entries, window 549 of 920
SENSITIVE_SEED = 925999917


def _env(monkeypatch, fp32=None):
    for k in ("C3HIP_FP32", "C3HIP_AUTO_FP32", "C3HIP_VERIFY", "C3HIP_VERIFY_TOL", "C3HIP_KEEP_ACTIVATIONS", "C3HIP_PACK_ROWS"):
        monkeypatch.delenv(k, raising=False)
    if fp32 is not None:
        monkeypatch.setenv("C3HIP_FP32", str(fp32))


def _model(monkeypatch, kind, ch, indel, sd, fp32=None, decode=False, **kw):
    """a handle created under C3HIP_FP32=<fp32> (None: the library's own decision)"""
    _env(monkeypatch, fp32)
    m = make_model(kind, ch, indel, sd, **kw)
    if decode:
        m.decode_columns(True)
    return m


def np_record(y16, y32, nout, tol, near_tie):
    """What the device reports for rows y16 against the reference rows y32, in numpy float32: the rule of tests.util.label_mismatches with
    the fp32 rows as the reference; the decoder columns behind nout are not compared."""
    a, r = np.ascontiguousarray(y16[:, :nout], np.float32), np.ascontiguousarray(y32[:, :nout], np.float32)
    d = np.abs(a - r)
    assert d.dtype == np.float32
    rec = dict(windows_checked=len(a), max_abs_diff=np.float32(d.max() if d.size else 0), head_max_abs_diff=[np.float32(0)] * 4,
               rows_over_tol=int((d.max(1) > np.float32(tol)).sum()) if d.size else 0, label_diffs=[0] * 4, near_ties=[0] * 4,
               worst_row=int(d.max(1).argmax()) if d.size else 0)
    for k, (lo, hi) in enumerate(util.HEAD_SLICES):
        if lo >= nout or not d.size:
            break
        rec["head_max_abs_diff"][k] = np.float32(d[:, lo:hi].max())
        differ = a[:, lo:hi].argmax(1) != r[:, lo:hi].argmax(1)
        top = np.sort(r[:, lo:hi], axis=1)
        wide = (top[:, -1] - top[:, -2]) > np.float32(near_tie)
        rec["label_diffs"][k], rec["near_ties"][k] = int((differ & wide).sum()), int((differ & ~wide).sum())
    return rec


def assert_record(st, rec, what):
    """floats as floats, counts as integers, no tolerance"""
    print(f"{what}: device max_abs_diff {st['max_abs_diff']:.3e} per head {[f'{v:.2e}' for v in st['head_max_abs_diff']]} worst row {st['worst_row']} "
          f"over tol {st['rows_over_tol']} labels {st['label_diffs']} near ties {st['near_ties']} windows {st['windows_checked']}")
    assert np.float32(st["max_abs_diff"]) == rec["max_abs_diff"], (what, st["max_abs_diff"], rec["max_abs_diff"])
    assert [np.float32(v) for v in st["head_max_abs_diff"]] == rec["head_max_abs_diff"], (what, st["head_max_abs_diff"], rec["head_max_abs_diff"])
    for key in ("windows_checked", "rows_over_tol", "label_diffs", "near_ties", "worst_row"):
        assert st[key] == rec[key], (what, key, st[key], rec[key])


# ------------------------------------------------------------------------------------------------ 1: report mode changes no row
def _tile(x, n):
    return np.concatenate([x] * (n // len(x) + 1))[:n]


REPORT_CASES = {
    # name: (kind, channels, indel heads, dtype, decoder columns, batch sizes: the first above the lane's micro-batch cap (16384 / 2048), the last one window)
    "pileup_i8": (syn.PILEUP, 18, False, np.int8, False, (16500, 300, 1025, 1)),
    "pileup_i32": (syn.PILEUP, 18, True, np.int32, False, (16500, 77, 1025, 1)),
    "pileup_i8_decode": (syn.PILEUP, 18, True, np.int8, True, (16500, 129, 1025, 1)),
    "fa_c8": (syn.FULL_ALIGNMENT, 8, True, np.int8, False, (2100, 77, 300, 1)),
    "fa_c9": (syn.FULL_ALIGNMENT, 9, True, np.int8, False, (2100, 130, 17, 1)),
}


@pytest.mark.parametrize("name", list(REPORT_CASES))
def test_report_mode_changes_no_row(name, monkeypatch):
    kind, ch, indel, dtype, decode, sizes = REPORT_CASES[name]
    m = _model(monkeypatch, kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=701), decode=decode)
    if kind == syn.PILEUP:
        base = syn.make_pileup_windows(600, seed=702, dtype=np.dtype(dtype))
    else:
        base = syn.make_fa_windows(160, seed=702, channels=ch)
    batches = [_tile(base[i:], n) for i, n in enumerate(sizes)]

    def run():
        return [m.wait(m.submit(x, slot=i % 2)) for i, x in enumerate(batches)]

    off = run()
    assert "verify" not in m.describe()
    assert all(y.shape == (len(x), m.row_size) and np.isfinite(y).all() for x, y in zip(batches, off))
    for every in (1, 3):
        m.verify(every=every)
        m.verify_reset()
        rows = run()
        st = m.verify_stats()
        for i, (a, b) in enumerate(zip(off, rows)):
            assert np.array_equal(a, b), f"{name} every={every}: batch {i} ({len(a)} windows) is not bit-identical to the run without verify mode"
        selected = [i for i in range(len(batches)) if i % every == 0]
        assert st["batches_submitted"] == len(batches) and st["batches_checked"] == len(selected) and st["batches_skipped"] == 0, st
        assert st["windows_checked"] == sum(len(batches[i]) for i in selected), st
        assert st["every"] == every and st["policy"] == "report" and st["escalations"] == 0
        assert "precision=fp16x3" in m.describe() and f"verify=every:{every},policy:report" in m.describe(), m.describe()
        print(f"{name} every={every}: {st}")
    m.verify(every=0)
    assert all(np.array_equal(a, b) for a, b in zip(off, run()))
    assert m.verify_stats()["batches_submitted"] == len(batches), "verify mode off: nothing is numbered"


# ------------------------------------------------------------------------------------------------ 2: the record is the truth
def _three_handles(monkeypatch, kind, ch, indel, sd, **kw):
    """(the handle under verify, forced to the fp16x3 kernels; a plain fp16x3 handle; a handle on the fp32 forms): same weights"""
    return (_model(monkeypatch, kind, ch, indel, sd, fp32=0, **kw), _model(monkeypatch, kind, ch, indel, sd, fp32=0, **kw),
            _model(monkeypatch, kind, ch, indel, sd, fp32=1, **kw))


def _check_truth(what, mv, m16, m32, call, nout):
    """call(model) -> rows.  Under two settings: the project's gates, and a tol / near_tie pair inside the fp16x3 noise so that the counts count"""
    y16, y32 = call(m16), call(m32)
    assert "on_fp32=0" in m16.describe() and "on_fp32=1" in m32.describe()
    assert y16.shape == y32.shape and len(y16) > 0
    for tol, near_tie in ((1e-4, util.NEAR_TIE), (2e-7, 1e-3)):
        mv.verify(every=1, tol=tol, near_tie=near_tie)
        mv.verify_reset()
        y = call(mv)
        assert np.array_equal(y, y16), f"{what}: report mode returns the fp16x3 rows"
        st = mv.verify_stats()
        assert st["batches_checked"] == 1 and st["batches_skipped"] == 0 and st["worst_batch"] == 0, st
        rec = np_record(y16, y32, nout, tol, near_tie)
        assert_record(st, rec, f"{what} tol={tol:g}")
        if near_tie == util.NEAR_TIE:  # the same count as the suite's own helper gives
            assert sum(rec["label_diffs"]) == len(util.label_mismatches(y16[:, :nout], y32[:, :nout]))
    return y16, y32


@pytest.mark.parametrize("kind,ch,indel,decode", [(syn.PILEUP, 18, True, False), (syn.PILEUP, 18, False, True), (syn.FULL_ALIGNMENT, 8, True, True)])
def test_record_ordinary_weights(kind, ch, indel, decode, monkeypatch):
    sd = syn.make_state_dict(kind, ch, indel, seed=711)
    mv, m16, m32 = _three_handles(monkeypatch, kind, ch, indel, sd, decode=decode)
    x = syn.make_windows(kind, 777 if kind == syn.PILEUP else 203, seed=712, channels=ch)
    y16, y32 = _check_truth(f"ordinary {kind}", mv, m16, m32, lambda m: m.predict_numpy(x), 90 if indel else 24)
    assert float(np.abs(y16 - y32)[:, :90 if indel else 24].max()) < util.PROB_TOL


def test_record_trained_like_pileup_on_fp16x3(monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=SENSITIVE_SEED, peaked=False, trained_like=True)
    x = syn.make_pileup_windows(920, seed=SENSITIVE_SEED, recipe="realistic")
    mv, m16, m32 = _three_handles(monkeypatch, syn.PILEUP, 18, True, sd)
    assert "precision=fp16x3" in mv.describe() and "precision=fp32-forced" in m32.describe()
    _check_truth("trained-like pileup", mv, m16, m32, lambda m: m.predict_numpy(x), 90)


def test_record_region_with_deep_windows(monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=721)
    region, _ = syn.make_pileup_region(9000, seed=722, depth=300)
    rng = np.random.default_rng(723)
    starts = rng.integers(0, len(region) - 33, size=1300).astype(np.int32)
    depths = rng.choice(np.array([40, 216, 217, 400, 3000], np.int32), size=len(starts)).astype(np.int32)
    assert int((depths > 1.5 * 144).sum()) > 300
    mv, m16, m32 = _three_handles(monkeypatch, syn.PILEUP, 18, False, sd)
    y16, _ = _check_truth("region with depths", mv, m16, m32, lambda m: m.predict_region(region, starts, depths=depths), 24)
    assert f"rescaled={int((depths > 216).sum())} " in mv.describe(), mv.describe()
    x = syn.rescale_deep_windows(np.stack([region[s:s + 33] for s in starts]), depths)
    assert np.array_equal(y16, m16.predict_numpy(x)), "the rows are those of the host-rescaled windows"


def test_record_candidates_only_kept_rows(monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=731)
    region, major = syn.make_pileup_region(30000, 5, seed=732, empty_fraction=0.01, depth=260)
    rng = np.random.default_rng(733)
    cand = np.unique(rng.integers(major[0] - 30, major[-1] + 30, size=1700))[:1500]
    depths = rng.choice(np.array([40, 150, 217, 400], np.int32), size=len(cand)).astype(np.int32)
    want_status, windows = syn.select_pileup_windows(region, major, cand, True)
    kept = len(windows)
    assert 0 < kept < len(cand) - 100, "candidates are dropped"
    mv, m16, m32 = _three_handles(monkeypatch, syn.PILEUP, 18, False, sd)

    def call(m):
        rows, status = m.predict_candidates(region, major, cand, depths=depths, head_tail=True)
        assert np.array_equal(status, want_status) and len(rows) == kept
        return rows
    _check_truth("candidates", mv, m16, m32, call, 24)
    assert mv.verify_stats()["windows_checked"] == kept
    # a candidate call with nothing to launch is numbered, selected and skipped
    mv.verify_reset()
    rows, status = mv.predict_candidates(region[:10], major[:10], cand[:5])
    st = mv.verify_stats()
    assert len(rows) == 0 and (st["batches_submitted"], st["batches_checked"], st["batches_skipped"]) == (1, 0, 1), st


@pytest.mark.parametrize("packed_here", [False, True])
def test_record_full_alignment_rows(packed_here, monkeypatch):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 9, True, seed=741)
    x = syn.make_fa_windows(190, seed=742, channels=9)
    rows, firsts, counts = syn.pack_fa_rows(x)
    mv, m16, m32 = _three_handles(monkeypatch, syn.FULL_ALIGNMENT, 9, True, sd)
    if packed_here:  # C3HIP_PACK_ROWS=1: the windows are packed while they are staged
        _env(monkeypatch, 0)
        monkeypatch.setenv("C3HIP_PACK_ROWS", "1")
        mv = make_model(syn.FULL_ALIGNMENT, 9, True, sd)
        monkeypatch.delenv("C3HIP_PACK_ROWS")
        assert "pack_rows=1" in mv.describe() and "precision=fp16x3" in mv.describe()
        y16, _ = _check_truth("rows packed here", mv, m16, m32, lambda m: m.predict_numpy(x), 90)
        assert "rows_windows=190" in mv.describe(), mv.describe()
    else:
        y16, _ = _check_truth("rows handed over", mv, m16, m32, lambda m: m.predict_rows(rows, counts, firsts), 90)
    assert np.array_equal(y16, m16.predict_numpy(x))


# ------------------------------------------------------------------------------------------------ 3: the policy acts on exactly what it measured
# seeds tried in this order for the trained-like weights and windows; the first whose max |d| on the fp16x3 kernels exceeds the ordinary weight
# set's is used and printed.  Seed 925999917 comes first: tests/diag/sensitive_window.py, the window the |w| >= 4 rule exists for.
POLICY_SEEDS = (SENSITIVE_SEED, 7, 11, 13, 17)


def _device_max(monkeypatch, sd, x):
    m = _model(monkeypatch, syn.PILEUP, 18, True, sd, fp32=0)
    m.verify(every=1)
    y = m.predict_numpy(x)
    st = m.verify_stats()
    assert st["batches_checked"] == 1
    return y, st


@pytest.fixture(scope="module")
def sensitive():
    """(weights, windows, d = the device's own max_abs_diff of a report run, fp16x3 rows, fp32 rows)"""
    mp = pytest.MonkeyPatch()
    try:
        sd0 = syn.make_state_dict(syn.PILEUP, 18, True, seed=711)
        _, st0 = _device_max(mp, sd0, syn.make_pileup_windows(920, seed=712))
        for seed in POLICY_SEEDS:
            sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=seed, peaked=False, trained_like=True)
            x = syn.make_pileup_windows(920, seed=seed, recipe="realistic")
            y16, st = _device_max(mp, sd, x)
            print(f"seed {seed}: max_abs_diff {st['max_abs_diff']:.3e} (ordinary weights: {st0['max_abs_diff']:.3e})")
            if st["max_abs_diff"] > st0["max_abs_diff"]:
                y32 = _model(mp, syn.PILEUP, 18, True, sd, fp32=1).predict_numpy(x)
                assert np.float32(np.abs(y16 - y32).max()) == np.float32(st["max_abs_diff"])
                return sd, x, np.float32(st["max_abs_diff"]), y16, y32
        pytest.fail("no trained-like weight set differs more between the two forms than the ordinary one")
    finally:
        mp.undo()


# near_tie = 1: every top-2 gap of a row of probabilities is at most 1, so every arg-max difference is excused and the batch escalates on tol
# alone -- the two runs below differ in nothing but tol = d / 2 against 2 d
def test_escalate_below_the_measured_difference(sensitive, monkeypatch, capfd):
    sd, x, d, y16, y32 = sensitive
    m = _model(monkeypatch, syn.PILEUP, 18, True, sd, fp32=0)
    m.verify(every=1, tol=float(d) / 2, near_tie=1.0, escalate=True)
    capfd.readouterr()
    y = m.predict_numpy(x)
    assert np.array_equal(y, y32) and not np.array_equal(y, y16), "the batch comes back as the C3HIP_FP32=1 handle's rows, bit for bit"
    st = m.verify_stats()
    assert "precision=fp32-verify" in m.describe() and "on_fp32=1" in m.describe(), m.describe()
    assert st["escalations"] == 1 and st["batches_checked"] == 1 and st["rows_over_tol"] >= 1 and st["batches_skipped"] == 0, st
    err = capfd.readouterr().err
    assert err.count("libc3hip: verify mode") == 1 and "continues on fp32" in err, err
    assert m.range_status()[1]
    y2 = m.predict_numpy(x[:300])  # the next batch: the handle is on the fp32 forms, nothing to compare
    st = m.verify_stats()
    assert np.array_equal(y2, y32[:300]) and st["batches_skipped"] == 1 and st["batches_checked"] == 1 and st["escalations"] == 1, st
    assert "libc3hip" not in capfd.readouterr().err
    m.load_state_dict(sd)  # a reload starts afresh: what C3HIP_FP32 chose, totals zero, the setting stays
    assert "precision=fp16x3" in m.describe() and m.verify_stats()["escalations"] == 0 and m.verify_stats()["policy"] == "escalate"


def test_no_escalation_above_the_measured_difference(sensitive, monkeypatch, capfd):
    sd, x, d, y16, y32 = sensitive
    m = _model(monkeypatch, syn.PILEUP, 18, True, sd, fp32=0)
    m.verify(every=1, tol=2 * float(d), near_tie=1.0, escalate=True)
    y = m.predict_numpy(x)
    st = m.verify_stats()
    assert np.array_equal(y, y16), "nothing escalates: the rows are the fp16x3 ones"
    assert st["escalations"] == 0 and st["rows_over_tol"] == 0 and st["batches_checked"] == 1 and np.float32(st["max_abs_diff"]) == d, st
    assert "precision=fp16x3" in m.describe() and "libc3hip" not in capfd.readouterr().err


@pytest.mark.parametrize("factor,escalates", [(0.5, True), (2.0, False)])
def test_policy_with_rows_left_on_the_device(sensitive, factor, escalates, monkeypatch):
    import torch
    sd, x, d, y16, y32 = sensitive
    m = _model(monkeypatch, syn.PILEUP, 18, True, sd, fp32=0)
    m.verify(every=1, tol=float(d) * factor, near_tie=1.0, escalate=True)
    y_dev = torch.full((len(x), 90), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert m.wait(m.submit_dev(x, y_dev.data_ptr(), slot=1)) is None
    y = y_dev.cpu().numpy()
    st = m.verify_stats()
    assert st["batches_checked"] == 1 and st["windows_checked"] == len(x) and np.float32(st["max_abs_diff"]) == d, st
    assert np.array_equal(y, y32 if escalates else y16), "the rows on the device are replaced exactly when the batch escalates"
    assert st["escalations"] == int(escalates) and ("precision=fp32-verify" in m.describe()) == escalates


def test_ordinary_models_never_escalate_on_the_golden_inputs(monkeypatch, capfd):
    """the project's own 1e-4 gate on those cases, as the device measures it"""
    _env(monkeypatch)
    for name, meta in sorted(util.manifest().items()):
        sd, x = util.case_inputs(meta)
        m = make_model(meta["kind"], meta["channels"], meta["add_indel_length"], sd, depth=meta.get("depth"))
        m.verify(every=1, escalate=True)
        y = m.predict_numpy(x)
        st = m.verify_stats()
        print(f"{name}: {m.describe().split('verify=')[1]}")
        assert st["escalations"] == 0 and "fp32-verify" not in m.describe(), (name, st)
        assert st["batches_checked"] + st["batches_skipped"] == st["batches_submitted"] >= 1, (name, st)
        assert (st["batches_checked"] > 0) == ("on_fp32=0" in m.describe()), (name, st, m.describe())
        assert st["rows_over_tol"] == 0 and sum(st["label_diffs"]) == 0 and st["max_abs_diff"] <= util.PROB_TOL, (name, st)
        util.assert_rows_match(y, util.golden_y(name), what=name)
    assert "verify mode" not in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------ 4: interplay
def _overflowing_weights():
    """the weight set of tests/test_parity_gpu.py's range-guard tests: a stage at ~1e7 that the fp16 pieces of its readers cannot hold"""
    sd = {k: np.array(v, copy=True) for k, v in syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=61).items()}
    for k in ("conv3.conv.weight", "conv3.conv.bias", "conv3.bn.running_mean"):
        sd[k] *= 4.0e6
    for k in ("res_block2.0.conv1.weight", "res_block2.0.conv2.weight"):
        sd[k] /= 2.0e3
    sd["conv5.conv.weight"] /= 4.0e6
    return sd


def test_range_guard_keeps_priority(monkeypatch, capfd):
    sd = _overflowing_weights()
    x = syn.make_fa_windows(5, seed=62)
    want = _model(monkeypatch, syn.FULL_ALIGNMENT, 8, True, sd, fp32=1).predict_numpy(x)
    m = _model(monkeypatch, syn.FULL_ALIGNMENT, 8, True, sd)
    m.verify(every=1, escalate=True)
    capfd.readouterr()
    y = m.predict_numpy(x)
    st = m.verify_stats()
    assert np.array_equal(y, want), "answered by the guard's re-run on the fp32 forms"
    assert (st["batches_submitted"], st["batches_checked"], st["batches_skipped"], st["escalations"]) == (1, 0, 1, 0), st
    err = capfd.readouterr().err
    assert "precision=fp32-range-guard" in m.describe() and "beyond the range of the fp16x3 kernels" in err and "verify mode" not in err


def test_keep_activations_and_profiling_are_left_alone(monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=751)
    x = syn.make_pileup_windows(40, seed=752)
    plain, kept = _model(monkeypatch, syn.PILEUP, 18, False, sd, keep=True), _model(monkeypatch, syn.PILEUP, 18, False, sd, keep=True)
    kept.verify(every=1)
    y0, y1 = plain.predict_numpy(x), kept.predict_numpy(x)
    st = kept.verify_stats()
    assert np.array_equal(y0, y1) and (st["batches_checked"], st["batches_skipped"]) == (0, 1), st
    for name, shape in (("lstm1_out", (40, 33, 256)), ("lstm2_out", (40, 33, 320)), ("l4_out", (40, 128))):
        assert np.array_equal(plain.debug_fetch(name, shape), kept.debug_fetch(name, shape)), f"{name}: the fp16x3 pass's activations"
    # profiling: the same launches as a handle that never heard of verify mode
    a, b = _model(monkeypatch, syn.PILEUP, 18, False, sd), _model(monkeypatch, syn.PILEUP, 18, False, sd)
    b.verify(every=1)
    for m in (a, b):
        m.profile(True)
        m.predict_numpy(x)
    st = b.verify_stats()
    assert (st["batches_checked"], st["batches_skipped"]) == (0, 1), st
    assert [(r["name"], r["launches"]) for r in a.profile_read()] == [(r["name"], r["launches"]) for r in b.profile_read()]
    # taps: the same
    b.profile(False)
    b.tap("lstm2_out")
    b.predict_numpy(x)
    assert b.verify_stats()["batches_skipped"] == 2
    b.tap("")
    b.predict_numpy(x)
    st = b.verify_stats()
    assert (st["batches_submitted"], st["batches_checked"], st["batches_skipped"]) == (3, 1, 2), st
    assert "lstm1=fused-f16x3" in b.describe() and "lstm2=f16x3" in b.describe(), "describe() reports the product pass, not the second one"


def test_reload_resets_the_totals_and_keeps_the_setting(monkeypatch):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=761)
    m = _model(monkeypatch, syn.FULL_ALIGNMENT, 8, True, sd)
    m.verify(every=2, tol=3e-5)
    x = syn.make_fa_windows(30, seed=762)
    for _ in range(3):
        m.predict_numpy(x)
    st = m.verify_stats()
    assert (st["batches_submitted"], st["batches_checked"], st["windows_checked"]) == (3, 2, 60) and st["max_abs_diff"] > 0 and st["worst_batch"] in (0, 2), st
    m.load_state_dict(sd)
    st = m.verify_stats()
    assert (st["batches_submitted"], st["batches_checked"], st["windows_checked"], st["worst_batch"]) == (0, 0, 0, -1) and st["max_abs_diff"] == 0, st
    assert st["every"] == 2 and np.float32(st["tol"]) == np.float32(3e-5)
    m.predict_numpy(x)
    assert m.verify_stats()["batches_checked"] == 1


@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_three_slots_in_flight_match_blocking_calls(kind, monkeypatch):
    ch, indel = (18, False) if kind == syn.PILEUP else (8, True)
    sd = syn.make_state_dict(kind, ch, indel, seed=771)
    sizes = (300, 256, 17, 500, 64, 256, 129) if kind == syn.PILEUP else (100, 64, 17, 130, 64, 90, 33)
    batches = [syn.make_windows(kind, n, seed=772 + i, channels=ch) for i, n in enumerate(sizes)]
    ring, blocking = _model(monkeypatch, kind, ch, indel, sd), _model(monkeypatch, kind, ch, indel, sd)
    for m in (ring, blocking):
        m.verify(every=2, tol=1e-6)
    want = [blocking.predict_numpy(x) for x in batches]
    got, tickets = [], []
    for i, x in enumerate(batches):
        if len(tickets) == 3:
            got.append(ring.wait(tickets.pop(0)))
        tickets.append(ring.submit(x, slot=i % 3))
    got += [ring.wait(t) for t in tickets]
    for i, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a, b), f"batch {i}"
    sr, sb = ring.verify_stats(), blocking.verify_stats()
    assert sr == sb, (sr, sb)
    assert sr["batches_checked"] == 4 and sr["windows_checked"] == sum(sizes[0::2]) and sr["max_abs_diff"] > 0, sr


# ------------------------------------------------------------------------------------------------ 5: off means off, and the environment
def test_off_means_off(monkeypatch):
    for kind, ch, indel in ((syn.PILEUP, 18, False), (syn.FULL_ALIGNMENT, 8, True)):
        m = _model(monkeypatch, kind, ch, indel, syn.make_state_dict(kind, ch, indel, seed=781))
        m.profile(True)
        m.predict_numpy(syn.make_windows(kind, 50, seed=782, channels=ch))
        assert "verify" not in m.describe()
        names = [r["name"] for r in m.profile_read()]
        assert names and not [n for n in names if "verify" in n or "compare" in n or "shadow" in n], names
        st = m.verify_stats()
        assert st["every"] == 0 and st["batches_submitted"] == 0 and st["batches_checked"] == 0 and st["worst_batch"] == -1, st
        assert m.describe().split()[-1].startswith("chunks=" if kind == syn.PILEUP else "pack_rows="), m.describe()


def test_environment_switches_it_on_where_the_model_is_built(monkeypatch):
    _env(monkeypatch)
    monkeypatch.setattr(predict, "_VERIFIED", [])
    monkeypatch.setattr("atexit.register", lambda fn: None)
    monkeypatch.setenv("C3HIP_VERIFY", "2,escalate")
    monkeypatch.setenv("C3HIP_VERIFY_TOL", "5e-5")
    m = predict.build_model(pileup=True, add_indel_length=False)
    m.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, False, seed=791))
    st = m.verify_stats()
    assert st["every"] == 2 and st["policy"] == "escalate" and np.float32(st["tol"]) == np.float32(5e-5) and np.float32(st["near_tie"]) == np.float32(util.NEAR_TIE)
    x = syn.make_pileup_windows(64, seed=792)
    for _ in range(3):
        m.predict_numpy(x)
    line = predict.verify_summary(m)
    print(line)
    assert line.startswith("[clair3_amd] verify: precision=fp16x3 every=2 policy=escalate") and "submitted=3 checked=2 skipped=0 windows=128" in line
    assert "escalations=0" in line and predict._VERIFIED == [m]


# ------------------------------------------------------------------------------------------------ 3b: escalation on labels alone
# The second condition of the policy: an arg-max difference outside near-ties escalates although no row is beyond tol.  The batch is built to
# have such differences: the zygosity head's class 1 gets class 0's weights moved by a few units in the last place (and class 2 is taken out of
# the race), so the two probabilities sit within rounding of each other, on either side of it -- which side is decided by the rounding of the
# forms.  tol = 1 is never exceeded by a difference of two probabilities; near_tie = 0 excuses only exact ties of the fp32 rows.
TIE_ULPS = (2, 1, 4, 8, 16)  # tried in this order; the first that gives a label difference outside exact ties is used and printed
# (on an MI355X the first does: 176 label differences, 82 exact ties, no row beyond tol, max |d| 4.1e-7 over 920 windows)


def _nearly_tied_zygosity(sd, ulps, seed):
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    w, b = sd["Y_genotype_logits.weight"], sd["Y_genotype_logits.bias"]
    moved = w[0].copy().view(np.int32) + np.random.default_rng(seed).integers(-ulps, ulps + 1, size=w.shape[1]).astype(np.int32)
    w[1] = moved.view(np.float32)
    b[1], b[2] = b[0], b[0] - 30.0
    return sd


def test_escalate_on_label_differences_alone(monkeypatch, capfd):
    base = syn.make_state_dict(syn.PILEUP, 18, False, seed=801)
    x = syn.make_pileup_windows(920, seed=802)
    for ulps in TIE_ULPS:
        sd = _nearly_tied_zygosity(base, ulps, 803)
        m = _model(monkeypatch, syn.PILEUP, 18, False, sd, fp32=0)
        m.verify(every=1, tol=1.0, near_tie=0.0)
        y16 = m.predict_numpy(x)
        st = m.verify_stats()
        with capfd.disabled():
            print(f"{ulps} ulps: labels {st['label_diffs']} exact ties {st['near_ties']} rows over tol {st['rows_over_tol']} max_abs_diff {st['max_abs_diff']:.3e}")
        if sum(st["label_diffs"]) > 0:
            break
    else:
        pytest.fail("no weight set gives an arg-max difference outside exact ties")
    assert st["rows_over_tol"] == 0 and st["escalations"] == 0 and "precision=fp16x3" in m.describe(), "report mode only counts"
    y32 = _model(monkeypatch, syn.PILEUP, 18, False, sd, fp32=1).predict_numpy(x)
    rec = np_record(y16, y32, 24, 1.0, 0.0)
    assert_record(st, rec, "nearly tied zygosity")
    assert float(np.abs(y16 - y32).max()) < util.PROB_TOL, "the rows agree within the project's gate: only labels differ"
    # escalate: the labels alone switch the handle
    m = _model(monkeypatch, syn.PILEUP, 18, False, sd, fp32=0)
    m.verify(every=1, tol=1.0, near_tie=0.0, escalate=True)
    capfd.readouterr()
    y = m.predict_numpy(x)
    st = m.verify_stats()
    assert np.array_equal(y, y32) and not np.array_equal(y, y16)
    assert st["escalations"] == 1 and st["rows_over_tol"] == 0 and st["label_diffs"] == rec["label_diffs"], st
    assert "precision=fp32-verify" in m.describe(), m.describe()
    err = capfd.readouterr().err
    assert err.count("libc3hip: verify mode") == 1 and " 0 rows beyond" in err, err
    # every difference excused (near_tie = 1) and none beyond tol: nothing escalates
    m = _model(monkeypatch, syn.PILEUP, 18, False, sd, fp32=0)
    m.verify(every=1, tol=1.0, near_tie=1.0, escalate=True)
    y = m.predict_numpy(x)
    st = m.verify_stats()
    assert np.array_equal(y, y16) and st["escalations"] == 0 and sum(st["label_diffs"]) == 0 and sum(st["near_ties"]) == sum(rec["label_diffs"]) + sum(rec["near_ties"]), st
    assert "precision=fp16x3" in m.describe()


# ------------------------------------------------------------------------------------------------ the drop-in: a worker process
def _worker(ref, job_dir, lst, ck, vcf, env_extra):
    """the reference's own stage-B worker command on libc3hip (tests/refloop.run_worker), stdout and stderr apart"""
    import os
    import subprocess
    import sys
    from tests import refloop
    cmd = [sys.executable, "-m", "clair3_amd.run_reference", "--ref", ref, "CallVariantsFromCffi", "--chkpnt_fn", ck, "--bam_fn", "unused.bam",
           "--call_fn", vcf, "--sampleName", "SAMPLE", "--platform", "ont", "--use_gpu", "True", "--cpu_threads", "2", "--threads", "4",
           "--output_tensor_can_fn_list", lst, "--gpu_id", "0", "--pileup"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("C3HIP_")}
    env["PYTHONPATH"] = os.pathsep.join([refloop.ROOT, refloop.STUBS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env.update(env_extra)
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=job_dir)


def test_worker_process_leaves_one_summary_line_on_stderr(tmp_path):
    """callvar.install() takes no new argument: C3HIP_VERIFY in the worker's environment is all.  One line on stderr at exit (not one per
    decode process), stdout and the VCF as without it"""
    import os
    from tests import refloop
    ref = refloop.reference_root()
    if ref is None:
        pytest.skip("no reference modules (oracle/_ref is staged by the build)")
    d = str(tmp_path)
    sizes = [1300, 41]  # two batches of the loop from the first file, one from the second
    lst = refloop.write_job(d, syn.PILEUP, sizes, channels=18)
    ck = os.path.join(d, "model")
    refloop.write_checkpoint(ck + ".pt", syn.PILEUP, 18, False)
    plain = _worker(ref, d, lst, ck, os.path.join(d, "plain.vcf"), {})
    assert plain.returncode == 0, (plain.stdout + plain.stderr)[-3000:]
    ver = _worker(ref, d, lst, ck, os.path.join(d, "verify.vcf"), {"C3HIP_VERIFY": "2", "C3HIP_VERIFY_TOL": "1e-4"})
    assert ver.returncode == 0, (ver.stdout + ver.stderr)[-3000:]
    print(ver.stderr[-2000:])
    summary = [ln for ln in ver.stderr.splitlines() if "[clair3_amd] verify" in ln]
    assert len(summary) == 1 and summary[0].startswith("[clair3_amd] verify: precision=fp16x3 every=2 policy=report"), ver.stderr[-3000:]
    assert " checked=0 " not in summary[0] and "skipped=0 " in summary[0] and "escalations=0" in summary[0], summary[0]
    assert "verify" not in plain.stderr and "verify" not in plain.stdout
    assert "verify" not in ver.stdout, "stdout is the loop's own"
    assert len(ver.stdout.splitlines()) == len(plain.stdout.splitlines()) and len(ver.stderr.splitlines()) == len(plain.stderr.splitlines()) + 1
    assert f"Total processed positions : {sum(sizes)}" in ver.stdout + ver.stderr
    a, b = refloop.vcf_records(os.path.join(d, "plain.vcf")), refloop.vcf_records(os.path.join(d, "verify.vcf"))
    assert len(a) >= sum(sizes) // 2 and a == b, "the VCF is character for character the one without verify mode"
