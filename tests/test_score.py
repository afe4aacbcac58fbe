"""Score mode (c3_model_set_score, csrc/c3_score.h), the part that needs no GPU: the rule in numpy (synthetic.focal_scores) against the
fixtures of tests/golden/make_golden_score.py -- the reference's own FocalLoss and _run_epoch(train=False) on committed reference rows --
the class weights, the validation epoch over a stand-in handle, the rebinding of clair3.Train._run_epoch where the reference checkout is
readable, and the C ABI.  (The host code of a scored batch -- plan_batch, the labels fill, the record reader -- is exercised without a
device by the stand-alone program tests/host/score_host_check.cpp, built with -fsanitize=address,undefined as its head says.)"""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

from clair3_amd import _lib, evaluate, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import util
from tests.test_abi import HEADER, _has_gpu, declared_symbols

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
CASES = ("pileup_realistic", "pileup_indel_heads", "fa_realistic", "fa_no_indel_heads", "handmade")
ENTRIES = ("c3_model_set_score", "c3_score_submit", "c3_score_wait", "c3_score", "c3_score_rows")
EPOCH_BATCH = 7  # make_golden_score.py EPOCH_BATCH
# the float32 rounding of the reference's own chain, relative per window: 6 roundings per term (log, the negated product with y, 1 - p, the
# square, its product with y, the product of the two -- a 7th with weights is covered by terms that are zero for one-hot labels), at most 32
# additions, and the double rounding of the comparison
REF_F32 = (6 + 32 + 2) * 2.0 ** -24


def fixture(case):
    f = dict(np.load(os.path.join(util.GOLDEN, f"score_{case}.npz")))
    f["rows"] = f["rows"] if case == "handmade" else util.golden_y(case)
    return f


def close(a, b, rel, what):
    """|a - b| <= rel * |b| element-wise; NaN exactly where b has NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN in other places"
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok])
    worst = float((err / np.maximum(np.abs(b[ok]), 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst relative difference {worst:.3e} (bound {rel:.3e})")
    assert (err <= rel * np.abs(b[ok])).all(), f"{what}: worst relative difference {worst:.3e} > {rel:.3e}"


@pytest.mark.parametrize("case", CASES)
def test_numpy_rule_reproduces_the_float64_fixture(case):
    f = fixture(case)
    for tag, w in (("", None), ("_w", f["weights"])):
        r = syn.focal_scores(f["rows"], f["labels"], gamma=2.0, class_weights=w)
        close(r["window_loss"], f["loss_f64" + tag], 1e-12, f"{case}{tag} float64")
        assert r["windows"] == len(f["rows"]) and r["tasks"] == f["loss_f64"].shape[1]
        with np.errstate(invalid="ignore"):
            close(r["loss_sum"], r["window_loss"].sum(0), len(f["rows"]) * 2.0 ** -52, f"{case}{tag} sums")


@pytest.mark.parametrize("case", CASES)
def test_numpy_rule_reproduces_the_reference_loss(case):
    f = fixture(case)
    for tag, w in (("", None), ("_w", f["weights"])):
        r = syn.focal_scores(f["rows"], f["labels"], gamma=2.0, class_weights=w)
        assert f["loss_ref" + tag].dtype == np.float32
        close(r["window_loss"], f["loss_ref" + tag], REF_F32, f"{case}{tag} reference float32")


def test_handmade_corners():
    """the clamp rule, the non-finite count and the lowest-index rule on the hand-made rows (make_golden_score.py handmade_rows)"""
    f = fixture("handmade")
    r = syn.focal_scores(f["rows"], f["labels"])
    L = r["window_loss"]
    top = -np.log(np.float64(np.float32(1e-9))) * (1.0 - np.float64(np.float32(1e-9))) ** 2
    assert abs(top - 20.7233) < 1e-4
    assert (L[0] == 0).all(), "p = 1 at the true class: a zero term"
    for row in (1, 2, 8, 10):  # p = 0, 1e-12, -inf, 1e-9f at the true class
        assert np.allclose(L[row], top, rtol=1e-15), (row, L[row])
    assert np.isnan(L[3]).all() and np.isnan(L[4]).all(), "a NaN anywhere in the task's columns reaches the window's value"
    assert (L[9] == 0).all(), "p just above 1 clamps to 1"
    assert np.isfinite(L[7]).all()
    assert r["nonfinite"] == 4, "rows 3, 4 (NaN), 7 (+inf), 8 (-inf)"
    # ties: rows 5 and 6 hold 0.4 at columns 1 and 2 of every task; the label sits on 1 (correct) and on 2 (not)
    per_row = [syn.focal_scores(f["rows"][i:i + 1], f["labels"][i:i + 1])["correct"] for i in range(len(L))]
    assert (per_row[5] == 1).all() and (per_row[6] == 0).all()
    assert (per_row[0] == 1).all() and (per_row[3] == 0).sum() + (per_row[3] == 1).sum() == 4
    assert (r["correct"] == np.sum(per_row, axis=0)).all()


def test_numpy_rule_general_in_y_and_gamma():
    """soft labels enter twice; gamma 0 leaves the squared-label cross entropy; float32 and int8 labels of the same values agree"""
    f = fixture("fa_realistic")
    rows, hard = f["rows"], f["labels"]
    soft = (0.75 * hard + 0.25 / 4).astype(np.float32)
    q = np.clip(rows, np.float32(1e-9), np.float32(1.0)).astype(np.float64)
    y = soft.astype(np.float64)
    for gamma in (0.0, 1.5, 2.0):
        want = np.stack([(y * y * -np.log(q) * (1 - q) ** gamma)[:, lo:hi].sum(1) for lo, hi in util.HEAD_SLICES], axis=1)
        close(syn.focal_scores(rows, soft, gamma=gamma)["window_loss"], want, 1e-12, f"soft labels gamma={gamma}")
    a, b = syn.focal_scores(rows, hard), syn.focal_scores(rows, hard.astype(np.float32))
    assert np.array_equal(a["window_loss"], b["window_loss"]) and np.array_equal(a["correct"], b["correct"])
    with pytest.raises(ValueError):
        syn.focal_scores(rows[:, :50], hard)
    with pytest.raises(ValueError):
        syn.focal_scores(rows, hard, class_weights=np.ones(24))
    empty = syn.focal_scores(rows[:0], hard[:0])
    assert empty["windows"] == 0 and (empty["loss_sum"] == 0).all() and empty["nonfinite"] == 0


@pytest.mark.parametrize("case", CASES)
def test_class_weights_are_the_reference_weights(case):
    f = fixture(case)
    w = evaluate.class_weights(f["eln"])
    assert w.dtype == np.float32 and w.shape == f["weights"].shape
    close(w, f["weights"], 2.0 ** -23, f"{case} class weights")
    for lo, hi in syn.head_slices(len(w)):
        assert abs(float(w[lo:hi].astype(np.float64).sum()) - (hi - lo)) < 1e-4
    if len(f["eln"]) == 90:
        assert np.array_equal(evaluate.class_weights(f["eln"], tasks=2), w[:24])


class StandIn:
    """a handle built on the numpy rule: 'windows' are window numbers, their rows the recorded ones"""

    def __init__(self, rows):
        self.rows, self.output_size, self.calls = rows, rows.shape[1], 0

    def score(self, x, labels, class_weights=None, gamma=2.0):
        self.calls += 1
        r = syn.focal_scores(self.rows[np.asarray(x)], labels, gamma=gamma, class_weights=class_weights)
        task = r["loss_sum"] / max(1, r["windows"])
        return types.SimpleNamespace(loss=float(sum(float(v) for v in task)), task_loss=task, windows=r["windows"])


def _loader(labels, batch=EPOCH_BATCH):
    return [(np.arange(i, min(i + batch, len(labels))), labels[i:i + batch]) for i in range(0, len(labels), batch)]


@pytest.mark.parametrize("case", CASES)
def test_validation_epoch_over_a_stand_in(case):
    f = fixture(case)
    bound = REF_F32 + (np.log2(EPOCH_BATCH) + 8) * 2.0 ** -24  # ... plus torch's float32 batch mean, the sum over tasks and the epoch's mean
    for tag, w in (("", None), ("_w", f["weights"])):
        h = StandIn(f["rows"])
        got = evaluate.run_validation_epoch(h, _loader(f["labels"]), class_weights=w)
        assert h.calls == -(-len(f["rows"]) // EPOCH_BATCH)
        close(np.array([got]), np.array([float(f["epoch_ref" + tag])]), bound, f"{case}{tag} epoch")
    # float labels and labels wider than the model's outputs are taken as the reference takes them
    wide = np.concatenate([f["labels"].astype(np.float32), np.ones((len(f["labels"]), 3), np.float32)], axis=1)
    a = evaluate.run_validation_epoch(StandIn(f["rows"]), _loader(wide))
    b = evaluate.run_validation_epoch(StandIn(f["rows"]), _loader(f["labels"]))
    assert a == b or (np.isnan(a) and np.isnan(b))
    assert evaluate.run_validation_epoch(StandIn(f["rows"]), []) == 0.0


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "clair3")), reason="needs the reference checkout")
def test_rebound_run_epoch_returns_the_reference_value(monkeypatch):
    torch = pytest.importorskip("torch")
    for name in ("h5py", "hdf5plugin", "tables"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    monkeypatch.syspath_prepend(REF)
    import clair3.Train as train
    from shared import param_p
    f = fixture("pileup_indel_heads")
    rows, labels = f["rows"], f["labels"]

    class Recorded(torch.nn.Module):
        def forward(self, idx):
            r = torch.from_numpy(rows)[idx.long()]
            return [r[:, lo:hi] for lo, hi in util.HEAD_SLICES]

    loader = _loader(labels, batch=8)
    assert len(loader) == 2
    bound = REF_F32 + (np.log2(8) + 8) * 2.0 ** -24
    original = evaluate.install(handle_factory=lambda module: StandIn(rows))
    try:
        assert train._run_epoch is not original
        for e in (None, f["eln"]):
            funcs = [train.FocalLoss(param_p.label_shape_cum, t, e) for t in range(4)]
            want = original(Recorded(), loader, None, funcs, param_p.label_shape[:4], "cpu", train=False)
            got = train._run_epoch(Recorded(), loader, None, funcs, param_p.label_shape[:4], "cpu", train=False)
            close(np.array([got]), np.array([want]), bound, f"rebound _run_epoch weights={e is not None}")
            # a distributed pass goes to the reference's function (which would need a process group to reduce: it never gets that far
            # with an empty loader)
            assert train._run_epoch(Recorded(), [], None, funcs, param_p.label_shape[:4], "cpu", train=False, distributed=True) == 0.0
        g, w = evaluate.loss_setting(funcs)
        assert g == 2.0 and np.array_equal(w, f["weights"])
    finally:
        evaluate.uninstall()
    assert train._run_epoch is original


def test_handle_for_strips_the_module_prefix():
    """the state dict of a (possibly wrapped) torch module reaches load_state_dict without the ``module.`` prefix; without a device the
    handle's creation fails loudly, which is how far a GPU-less host gets"""
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=3)

    class Clair3_P_:  # named like the reference's class
        add_indel_length = True

        def state_dict(self):
            return {"module." + k: v for k, v in sd.items()}
    Clair3_P_.__name__ = "Clair3_P"
    if _has_gpu():
        m = evaluate.handle_for(Clair3_P_())
        assert m.output_size == 90 and m.input_channels == 18
    else:
        with pytest.raises(_lib.C3Error):
            evaluate.handle_for(Clair3_P_())
    with pytest.raises(TypeError):
        evaluate.handle_for(types.SimpleNamespace(state_dict=lambda: sd))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    comment = src[:src.index("} c3_score_result;")].rsplit("/* ----", 1)[1]
    assert "DESIGN.md 4" in comment and "Train.py:87-107" in comment and "nonfinite" in comment


def test_result_struct_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} c3_score_result;", src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, name = decl.split(None, 1)
            fields.append((ctype, name.strip()))
    ctypes_of = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    want = []
    for ctype, name in fields:
        m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
        want.append((m.group(1), ctypes_of[ctype] * int(m.group(2))) if m else (name, ctypes_of[ctype]))
    assert [(n, t) for n, t in _lib.ScoreResult._fields_] == want
    assert ctypes.sizeof(_lib.ScoreResult) == 8 + 4 + 4 + 32 + 32 + 8


def test_null_handle_and_python_argument_errors():
    L = _lib.lib()
    rec = _lib.ScoreResult()
    assert L.c3_model_set_score(None, 1, 2.0, None) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_score_submit(None, None, 0, 0, None, 0, None, None, 0) != 0
    assert L.c3_score_wait(None, 0, ctypes.byref(rec)) != 0
    assert L.c3_score(None, None, 0, 0, None, 0, None, None, ctypes.byref(rec)) != 0
    assert L.c3_score_rows(None, None, 24, 0, None, 0, ctypes.byref(rec), None) != 0
    for cls in (Clair3_P, Clair3_F):
        m = cls(add_indel_length=True, predict=True)
        with pytest.raises(_lib.C3Error, match="no device"):
            m.score(np.zeros((1, 33, 18), np.int8), np.zeros((1, 90), np.int8))
        with pytest.raises(_lib.C3Error, match="no device"):
            m.score_rows(np.zeros((1, 90), np.float32), np.zeros((1, 90), np.int8))
