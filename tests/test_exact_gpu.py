"""The exact form (c3_predict_exact, c3_exact_fetch: both networks in fp64 on the device) against the C oracle, and the audit tool.

The yardstick is always oracle.oracle, never a form of the library.  Bounds, with y_o and the layer dumps d of the oracle (debug=True):
    rows    |y64 - y_o| <= 2**-25 + 1e-9
    layers  |a64 - a_o| <= 2**-24 |a_o| + 1e-9 max(1, max |a_o|)
The first term is the rounding of the oracle's own float32 output and dumps.  The 1e-9 is derived, not measured: fp64 sums of at most
10 560 terms give 1.2e-12 relative; the worst amplification this suite knows is about 500 x (the sensitive window turns the 2.4e-7 of
fp16x3 into 1.25e-4); an order of magnitude to spare.  Every test prints its measured maxima before it asserts."""
import json

import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P

pytestmark = pytest.mark.gpu

ROW_BOUND = 2.0 ** -25 + 1e-9
SENSITIVE_SEED, SENSITIVE_WINDOW = 925999917, 549


def make(kind, ch, indel, sd, depth=None, exact=True):
    m = (Clair3_P if kind == syn.PILEUP else Clair3_F)(add_indel_length=indel, predict=True, input_channels=ch)
    if depth:
        m.set_geometry(depth, 33)
    m.to("cuda:0")
    m.load_state_dict(sd)
    return m.exact(True) if exact else m


def check_rows(y64, y_o, what):
    assert y64.dtype == np.float64 and y64.shape == y_o.shape and np.isfinite(y64).all(), what
    err = float(np.abs(y64 - y_o.astype(np.float64)).max())
    print(f"{what}: rows max |y64 - y_o| = {err:.3e} (bound {ROW_BOUND:.3e})")
    assert err <= ROW_BOUND, f"{what}: rows {err:.3e} > {ROW_BOUND:.3e}"
    return err


def check_layer(a64, a_o, what):
    a_o = a_o.astype(np.float64)
    assert a64.shape == a_o.shape and np.isfinite(a64).all(), what
    bound = 2.0 ** -24 * np.abs(a_o) + 1e-9 * max(1.0, float(np.abs(a_o).max()))
    excess = np.abs(a64 - a_o) - bound
    err = float(np.abs(a64 - a_o).max())
    print(f"{what}: max |a64 - a_o| = {err:.3e}, max |a_o| = {float(np.abs(a_o).max()):.3e}, worst excess over the bound {float(excess.max()):.3e}")
    assert (excess <= 0).all(), f"{what}: {int((excess > 0).sum())} values beyond the bound, worst by {float(excess.max()):.3e}"


@pytest.fixture(scope="module")
def oracle_mod():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def fa_case(oracle_mod):
    """case (a) of the full-alignment test, shared with the batch / chunk test: ordinary weights, C = 8, depth 89, B = 3"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=61)
    x = syn.make_fa_windows(3, seed=62)
    y_o, d = oracle_mod.fa_forward(sd, x, True, debug=True)
    return dict(sd=sd, x=x, y_o=y_o, d=d, ch=8, depth=None)


@pytest.fixture(scope="module")
def pileup_case(oracle_mod):
    """case (a) of the pileup test, shared with the batch / chunk test: int32 windows, add_indel_length, B = 5"""
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=61)
    x = syn.make_pileup_windows(5, seed=63, dtype=np.int32)
    y_o, d = oracle_mod.pileup_forward(sd, x, True, debug=True)
    return dict(sd=sd, x=x, y_o=y_o, d=d, indel=True)


# ------------------------------------------------------------------------------------------------ 1: full alignment
@pytest.mark.parametrize("case", ["ordinary_c8_d89_b3", "trained_like_c9_d55_b2"])
def test_full_alignment_rows_and_layers(case, fa_case, oracle_mod):
    if case == "ordinary_c8_d89_b3":  # M = B Ho Wo is odd in every layer: every layer has an edge tile
        c = fa_case
    else:  # unaligned 9-byte pixels, even-sized stride-2 stages, top and bottom padding of the 3-bin level
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 9, True, seed=64, trained_like=True)
        x = syn.make_fa_windows(2, seed=65, channels=9, depth=55)
        y_o, d = oracle_mod.fa_forward(sd, x, True, debug=True)
        c = dict(sd=sd, x=x, y_o=y_o, d=d, ch=9, depth=55)
    m = make(syn.FULL_ALIGNMENT, c["ch"], True, c["sd"], depth=c["depth"])
    y64 = m.predict_exact(c["x"])
    check_rows(y64, c["y_o"], case)
    for name in [f"act{i}" for i in range(9)] + ["spp", "l4_out"]:
        check_layer(m.exact_fetch(name, 0, c["d"][name].shape), c["d"][name], f"{case} {name}")


# ------------------------------------------------------------------------------------------------ 2: pileup
@pytest.mark.parametrize("case", ["int32_indel_b5", "int8_b17"])
def test_pileup_rows_and_layers(case, pileup_case, oracle_mod):
    if case == "int32_indel_b5":  # the 16-window tile is part-filled
        c = pileup_case
    else:  # one full tile and one with a single window; rows 24 wide
        sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=66)
        x = syn.make_pileup_windows(17, seed=67, dtype=np.int8)
        y_o, d = oracle_mod.pileup_forward(sd, x, False, debug=True)
        c = dict(sd=sd, x=x, y_o=y_o, d=d, indel=False)
    m = make(syn.PILEUP, 18, c["indel"], c["sd"])
    y64 = m.predict_exact(c["x"])
    assert y64.shape[1] == (90 if c["indel"] else 24)
    check_rows(y64, c["y_o"], case)
    for name in ("lstm1_out", "lstm2_out", "l4_out"):
        check_layer(m.exact_fetch(name, 0, c["d"][name].shape), c["d"][name], f"{case} {name}")


# ------------------------------------------------------------------------------------------------ 3: the sensitive recurrence
def test_the_sensitive_recurrence(oracle_mod, monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=SENSITIVE_SEED, peaked=False, trained_like=True)
    x = syn.make_pileup_windows(920, seed=SENSITIVE_SEED, recipe="realistic")
    lo = SENSITIVE_WINDOW - SENSITIVE_WINDOW % 16
    xs = np.ascontiguousarray(x[lo:lo + 16])
    y_o = oracle_mod.pileup_forward(sd, xs, True)
    for k in ("C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_AUTO_FP32"):
        monkeypatch.delenv(k, raising=False)
    y64 = None
    for fp32 in ("0", "1"):
        monkeypatch.setenv("C3HIP_FP32", fp32)
        m = make(syn.PILEUP, 18, True, sd)
        y = m.predict_exact(xs)
        check_rows(y, y_o, f"sensitive tile, exact rows of the C3HIP_FP32={fp32} handle")
        assert y64 is None or np.array_equal(y, y64), "the exact rows do not depend on the handle's precision"
        y64 = y
        dist = float(np.abs(m.predict_numpy(xs).astype(np.float64) - y64).max())
        print(f"sensitive tile: C3HIP_FP32={fp32} ({m.describe().split('precision=')[1].split()[0]}) max |y - y64| = {dist:.3e}")
        assert dist <= 1e-3, "the project's sanity bound (the line prints the distance; it is not the gate of the forms)"


# ------------------------------------------------------------------------------------------------ 4: independent of batch and chunk
@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_rows_do_not_depend_on_batch_or_chunk(kind, pileup_case, fa_case, monkeypatch):
    c = pileup_case if kind == syn.PILEUP else fa_case
    x = c["x"]
    monkeypatch.delenv("C3HIP_EXACT_CHUNK", raising=False)
    m = make(kind, x.shape[-1], True, c["sd"])
    y = m.predict_exact(x)
    name = "lstm2_out" if kind == syn.PILEUP else "act4"
    shape = c["d"][name].shape[1:]
    whole = m.exact_fetch(name, 0, (len(x),) + shape)
    alone = m.predict_exact(x[2:3])
    assert np.array_equal(alone[0], y[2]), "window 2 alone against window 2 inside the batch"
    monkeypatch.setenv("C3HIP_EXACT_CHUNK", "2")
    cut = m.predict_exact(x)
    assert np.array_equal(cut, y), "C3HIP_EXACT_CHUNK=2 against the uncut call"
    # the cut call's LAST pass: window 4 of 5 (passes of 2, 2, 1) / window 2 of 3 (passes of 2, 1)
    last = m.exact_fetch(name, 0, (1,) + shape)
    assert np.array_equal(last[0], whole[len(x) - 1]), "exact_fetch after the cut call returns the last pass's windows"
    with pytest.raises(_lib.C3Error, match="the last pass had 1"):
        m.exact_fetch(name, 0, (2,) + shape)


# ------------------------------------------------------------------------------------------------ 5: nothing else moves
def test_nothing_else_moves(pileup_case, monkeypatch):
    for k in ("C3HIP_EXACT", "C3HIP_EXACT_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    x = pileup_case["x"]
    m = make(syn.PILEUP, 18, True, pileup_case["sd"], exact=False)
    y0 = m.predict_numpy(x)
    d0 = m.describe()
    assert "exact" not in d0
    with pytest.raises(_lib.C3Error, match="c3_model_set_exact"):  # a handle that never enabled it
        m.predict_exact(x)
    assert np.array_equal(m.predict_numpy(x), y0) and m.describe() == d0, "... predicts as before afterwards"
    m.exact(True)
    assert np.array_equal(m.predict_numpy(x), y0), "predict_numpy before and after exact(True)"
    assert m.describe() == d0 + " exact=1", "describe() differs only by ' exact=1'"
    # what an exact call leaves alone: verify totals, the range flag, a tap, what describe() reports
    m.verify(every=1)
    assert np.array_equal(m.predict_numpy(x), y0)
    m.tap("lstm2_out")  # (a tapped batch is not verified: the totals stay those of the batch before)
    assert np.array_equal(m.predict_numpy(x), y0)
    d1, r1, v1, t1 = m.describe(), m.range_status(), m.verify_stats(), m.tap_fetch("lstm2_out", 0, (5, 33, 320))
    assert v1["batches_checked"] == 1 and v1["windows_checked"] == 5
    m.predict_exact(x)
    assert m.describe() == d1 and m.range_status() == r1 and m.verify_stats() == v1
    assert np.array_equal(m.tap_fetch("lstm2_out", 0, (5, 33, 320)), t1), "a tap set before the exact call"
    assert np.array_equal(m.predict_numpy(x), y0), "predict_numpy after a predict_exact"


# ------------------------------------------------------------------------------------------------ 6: errors
def test_errors(fa_case, pileup_case):
    f = make(syn.FULL_ALIGNMENT, 8, True, fa_case["sd"])
    x = fa_case["x"]
    y = np.full((3, 90), -1.0)
    assert _lib.lib().c3_predict_exact(f._handle, x.astype(np.int32).ctypes.data, _lib.DTYPE_I32, 3, y.ctypes.data) != 0
    assert "int8" in _lib.last_error() and (y == -1.0).all()
    assert _lib.lib().c3_predict_exact(f._handle, None, _lib.DTYPE_I8, 3, y.ctypes.data) != 0 and "null buffer" in _lib.last_error()
    assert _lib.lib().c3_predict_exact(f._handle, x.ctypes.data, _lib.DTYPE_I8, 0, y.ctypes.data) == 0 and (y == -1.0).all(), "batch == 0 writes nothing"
    assert _lib.lib().c3_predict_exact(f._handle, None, _lib.DTYPE_I8, 0, None) == 0
    with pytest.raises(_lib.C3Error, match="unknown tensor"):
        f.exact_fetch("lstm1_out", 0, (1, 33, 256))
    p = make(syn.PILEUP, 18, True, pileup_case["sd"])
    xp = pileup_case["x"]
    want = p.predict_numpy(xp)
    ticket = p.submit(xp, slot=1)
    with pytest.raises(_lib.C3Error, match="in flight"):
        p.predict_exact(xp)
    with pytest.raises(_lib.C3Error, match="in flight"):
        p.exact(False)
    assert np.array_equal(p.wait(ticket), want), "the slot can still be waited"
    check_rows(p.predict_exact(xp), pileup_case["y_o"], "after the refusals")


# ------------------------------------------------------------------------------------------------ 7: the tool end to end
@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_the_audit_tool_end_to_end(kind, tmp_path, monkeypatch, capsys):
    import torch
    from clair3_amd import audit
    for k in ("C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_EXACT", "C3HIP_EXACT_CHUNK", "C3HIP_CALIBRATION", "C3HIP_VERIFY"):
        monkeypatch.delenv(k, raising=False)
    pileup = kind == syn.PILEUP
    ch = 18 if pileup else 8
    sd = syn.make_state_dict(kind, ch, True, seed=71)
    x = syn.make_windows(kind, 8, seed=72)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(tmp_path / "m.pt"))
    np.save(str(tmp_path / "x.npy"), x)
    plan = "lstm2" if pileup else "res3a"
    rows = {}
    argv = ["--chkpnt_fn", str(tmp_path / "m.pt"), "--tensor_fn", str(tmp_path / "x.npy"), "--plans", plan, "--out", str(tmp_path / "audit.jsonl")]
    assert audit.main(argv + (["--pileup"] if pileup else []), rows_out=rows) == 0
    printed = capsys.readouterr().out
    with open(tmp_path / "audit.jsonl") as f:
        text = f.read()
    assert text == printed[-len(text):]
    lines = [json.loads(line) for line in text.splitlines()]
    print(text)
    assert [line["form"] for line in lines] == ["exact", "none", "all", plan]
    for line in lines:
        flat = [v for val in line.values() if not isinstance(val, str) for v in (val if isinstance(val, list) else [val])]
        assert np.isfinite(np.array(flat, dtype=np.float64)).all(), line
        assert line["windows"] == 8 and len(line["head_max_abs_err"]) == 4
        assert line["max_abs_err"] <= 1e-4 and line["rows_over_tol"] == 0, f"{line['form']} beyond the 1e-4 gate on ordinary weights"
    assert lines[0]["max_abs_err"] == 0.0 and lines[0]["precision"] == "fp64" and lines[1]["precision"] == "fp16x3"
    monkeypatch.setenv("C3HIP_FP32", "1")
    fp32 = make(kind, ch, True, sd, exact=False)
    assert np.array_equal(rows["all"], fp32.predict_numpy(x)), "the `all` line's rows are a C3HIP_FP32=1 handle's, bit for bit"
