"""Calibration of the full-alignment channel exponents on the device (c3_model_calibrate and the entries around it; needs an MI355X): the
census kernel against numpy and the fp64 oracle, the rule on the handle's own census, and the calibrated fp16x3 path on the suite's
out-of-range recipe -- rows, layers, every entry, verify mode, portability -- against the oracle and against the uncalibrated handle."""
import ctypes

import numpy as np
import pytest

from clair3_amd import _lib, calibrate as cal, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import util
from tests.test_calibration import recipe_state_dict, rule_numpy

pytestmark = pytest.mark.gpu

LAYER_TOL = 2e-5  # the suite's layer gate: max |a - oracle| relative to max(1, max |oracle|) of the tensor


def make_fa(sd, channels=8, depth=None, keep=False, lowering=None):
    m = Clair3_F(add_indel_length=True, predict=True, input_channels=channels)
    if depth:
        m.set_geometry(depth, 33)
    if keep:
        m.keep_activations(True)
    m.to("cuda:0")
    if lowering is not None:
        m.set_calibration(lowering)  # before the load: it packs with it
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def oracle_mod():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def recipe(oracle_mod):
    """the suite's out-of-range recipe (tests/test_parity_gpu.py), its sample (seed 62), an unseen batch (seed 63) and the oracle on both"""
    sd = recipe_state_dict()
    x5, x7 = syn.make_fa_windows(5, seed=62), syn.make_fa_windows(7, seed=63)
    y5, d5 = oracle_mod.fa_forward(sd, x5, True, debug=True)
    y7 = oracle_mod.fa_forward(sd, x7, True)
    return dict(sd=sd, x5=x5, x7=x7, y5=y5, d5=d5, y7=y7)


@pytest.fixture(scope="module")
def calibrated(recipe):
    """a handle calibrated on the sample; the tests that share it only predict with it"""
    m = make_fa(recipe["sd"])
    summary = m.calibrate(recipe["x5"])
    return m, summary


def census_numpy(acts):
    out = np.zeros((9, 256), np.float32)
    for l, a in enumerate(acts):
        out[l, :a.shape[-1]] = np.abs(a).reshape(-1, a.shape[-1]).max(0)
    return out


def solve_numpy(state, cap=10):
    """the rule of include/c3hip.h on a handle's own census and k0, group by group"""
    a, k0 = cal.group_maxima(state["census"]), state["k0"].astype(np.int64)
    low = np.concatenate([rule_numpy(np.ldexp(a[at:at + n], k0[at:at + n]), cap) for _, at, n, _ in cal.GROUPS]).astype(np.int64)
    return np.minimum(low, k0 + 40).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 1, 2: the census
@pytest.mark.parametrize("windows, channels, depth", [(3, 8, None), (3, 9, None), (3, 8, 55), (12, 8, None)])
def test_census_is_the_exact_maximum(windows, channels, depth, oracle_mod, monkeypatch):
    """3 windows: 2295 / 621 / 180 rows at C = 8 -- odd, and at the last stage fewer than one workgroup's stride; 12 windows: more
    workgroups than the grid is capped at, so that every workgroup strides"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, channels, True, seed=7)
    x = syn.make_fa_windows(windows, seed=8, channels=channels, depth=depth or syn.FA_DEPTH_ONT)
    _, d = oracle_mod.fa_forward(sd, x, True, debug=True)
    m = make_fa(sd, channels, depth)
    m.calibrate(x, apply=False)
    state = m.calibration()
    assert state["windows"] == windows
    monkeypatch.setenv("C3HIP_FP32", "1")
    ref = make_fa(sd, channels, depth, keep=True)  # the fp32 forms, every layer kept: debug_fetch returns the checkpoint's units
    monkeypatch.delenv("C3HIP_FP32")
    ref.predict_numpy(x)
    acts = [ref.debug_fetch(f"act{l}", d[f"act{l}"].shape) for l in range(9)]
    assert np.array_equal(state["census"], census_numpy(acts))
    want = census_numpy([d[f"act{l}"] for l in range(9)]).astype(np.float64)
    for l in range(9):
        err = float(np.abs(state["census"][l] - want[l]).max()) / max(1.0, float(want[l].max()))
        print(f"layer {l}: census against the oracle {err:.3e}")
        assert err < LAYER_TOL, f"layer {l}"


def test_census_accumulates_and_resets():
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7)
    x = syn.make_fa_windows(7, seed=63)
    m = make_fa(sd)
    m.calibrate(x, apply=False)
    whole = m.calibration()
    assert whole["windows"] == 7 and whole["census"].max() > 0
    for cut in (3, 4):
        m.calibration_reset()
        zero = m.calibration()
        assert zero["windows"] == 0 and not zero["census"].any()
        m.calibrate(x[:cut], apply=False)
        m.calibrate(x[cut:], apply=False)
        parts = m.calibration()
        assert parts["windows"] == 7 and np.array_equal(parts["census"], whole["census"]), cut
    m.calibrate(x[:2], apply=False)  # windows seen before add nothing to the maxima, only to the count
    again = m.calibration()
    assert again["windows"] == 9 and np.array_equal(again["census"], whole["census"])


# ------------------------------------------------------------------------------------------------ 3: an ordinary model
def test_ordinary_model_is_left_as_it_is():
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7)
    x = syn.make_fa_windows(8, seed=8)
    fresh = make_fa(sd)
    y0 = fresh.predict_numpy(x)
    m = make_fa(sd)
    assert np.array_equal(m.predict_numpy(x), y0)
    before = (m.describe(), m.range_status(), m.layer_precision())
    m.calibrate(x, apply=False)  # the census pass leaves what the handle runs and reports alone
    assert (m.describe(), m.range_status(), m.layer_precision()) == before and "calibration=" not in before[0]
    assert np.array_equal(m.predict_numpy(x), y0)
    s = m.calibrate(x)
    assert not s["lowering"].any() and s["lowered"] == 0 and s["applied"]
    assert all(g["lowered"] == 0 and g["shift"] == 0 and g["max_before"] == g["max_after"] < 64 for g in s["groups"]), s["groups"]
    state = m.calibration()
    assert np.array_equal(state["k0"], state["k"]) and not state["lowering"].any()
    assert np.array_equal(m.predict_numpy(x), y0), "an all-zero lowering packs the bytes of a handle without one"
    text = m.describe()
    assert "calibration=cap:10,windows:16,lowered:0" in text and "conv_stack=planes-f16x3" in text
    assert "precision=fp16x3" in text and m.range_status() == (0, False)


# ------------------------------------------------------------------------------------------------ 4: the suite's recipe
def test_recipe_runs_calibrated_on_the_product_path(recipe, calibrated, oracle_mod, capfd, monkeypatch):
    m, s = calibrated
    groups = {g["name"]: g for g in s["groups"]}
    figures = [cal.summary_text(s)]  # (shown at the end, past capfd)
    assert groups["stage1"]["max_before"] > 16000 and groups["inner1"]["max_before"] > 16000, "the recipe is beyond the guard without it"
    assert all(g["max_after"] < 1024 for g in s["groups"])
    assert (groups["stage1"]["lowered"], groups["stage1"]["shift"], groups["inner1"]["lowered"], groups["inner1"]["shift"]) == (128, 13, 128, 3)
    assert all(groups[n]["lowered"] == 0 for n in ("stage0", "inner0", "stage2", "inner2"))
    state = m.calibration()
    assert np.array_equal(state["lowering"], solve_numpy(state)), "the handle's lowering is the rule on the handle's own census"
    assert np.array_equal(state["k"], state["k0"].astype(np.int64) - state["lowering"])
    capfd.readouterr()
    errs = {}
    for name, x, y_o in (("sample", recipe["x5"], recipe["y5"]), ("unseen", recipe["x7"], recipe["y7"])):
        y = m.predict_numpy(x)
        errs[name] = float(np.abs(y.astype(np.float64) - y_o).max())
        figures.append(f"calibrated fp16x3 rows, {name} batch: max |dY| against the oracle = {errs[name]:.3e}")
    # beside them, the fp32 forms on the same weights (what the guard falls back to)
    monkeypatch.setenv("C3HIP_FP32", "1")
    f32 = make_fa(recipe["sd"])
    monkeypatch.delenv("C3HIP_FP32")
    for name, x, y_o in (("sample", recipe["x5"], recipe["y5"]), ("unseen", recipe["x7"], recipe["y7"])):
        figures.append(f"fp32 forms, {name} batch: max |dY| against the oracle = {float(np.abs(f32.predict_numpy(x).astype(np.float64) - y_o).max()):.3e}")
    text = m.describe()
    figures.append(text)
    with capfd.disabled():
        print("\n" + "\n".join(figures))
    assert "continues on fp32" not in capfd.readouterr().err
    assert m.range_status() == (0, False)
    assert "conv_stack=planes-f16x3" in text and "precision=fp16x3" in text and "calibration=cap:10,windows:5,lowered:256" in text
    for name, x, y_o in (("sample", recipe["x5"], recipe["y5"]), ("unseen", recipe["x7"], recipe["y7"])):
        util.assert_rows_match(m.predict_numpy(x), y_o, tol=util.PROB_TOL, what=f"calibrated, {name} batch")


def test_recipe_layers_calibrated(recipe, calibrated):
    keep = make_fa(recipe["sd"], keep=True, lowering=calibrated[0].calibration()["lowering"])
    keep.predict_numpy(recipe["x5"])
    assert "conv_stack=planes-f16x3" in keep.describe() and keep.range_status() == (0, False)
    worst = {}
    for l in range(9):
        ref = recipe["d5"][f"act{l}"]
        a = keep.debug_fetch(f"act{l}", ref.shape)
        assert np.isfinite(a).all(), l
        worst[l] = float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))
    print("calibrated fp16x3 layers against the oracle: " + " ".join(f"act{l}={e:.2e}" for l, e in worst.items()))
    assert all(e < LAYER_TOL for e in worst.values()), worst


# ------------------------------------------------------------------------------------------------ 5: one hot channel
def test_a_single_hot_channel_moves_alone(oracle_mod, capfd):
    sd = recipe_state_dict(hot_channel=5)
    x5, x7 = syn.make_fa_windows(5, seed=62), syn.make_fa_windows(7, seed=63)
    m = make_fa(sd)
    s = m.calibrate(x5)
    assert np.flatnonzero(s["lowering"]).tolist() == [128 + 5], "channel 5 of stage 2: one of 896 entries"
    stage = {g["name"]: g for g in s["groups"]}["stage1"]
    assert stage["max_before"] > 16000 and stage["max_after"] < 1024 and stage["shift"] == 0
    capfd.readouterr()
    for name, x in (("sample", x5), ("unseen", x7)):
        err = util.assert_rows_match(m.predict_numpy(x), oracle_mod.fa_forward(sd, x, True), tol=util.PROB_TOL, what=f"hot channel, {name} batch")
        with capfd.disabled():
            print(f"hot channel, {name} batch: max |dY| against the oracle = {err:.3e}")
    assert "continues on fp32" not in capfd.readouterr().err and m.range_status() == (0, False)
    assert "lowered:1" in m.describe()


# ------------------------------------------------------------------------------------------------ 6: portability
def test_a_lowering_travels(recipe, calibrated, tmp_path, monkeypatch, capfd):
    import torch
    from clair3_amd.predict import build_model
    a = calibrated[0]
    lowering = a.calibration()["lowering"]
    ya = a.predict_numpy(recipe["x7"])
    b = make_fa(recipe["sd"], lowering=lowering)
    assert np.array_equal(b.predict_numpy(recipe["x7"]), ya), "set on a fresh handle before its load"
    assert np.array_equal(b.calibration()["k"], a.calibration()["k"]) and "calibration=cap:0,windows:0,lowered:256" in b.describe()
    # the census is in the checkpoint's units whatever exponents the handle runs with: on the lowered handle, bit for bit the first one
    b.calibrate(recipe["x5"], apply=False)
    assert np.array_equal(b.calibration()["census"], a.calibration()["census"]) and b.calibration()["windows"] == 5
    b.calibrate(recipe["x5"], cap_log2=12, apply=False)  # a solve that is not applied leaves what describe() says of the lowering in force
    assert "calibration=cap:0,windows:0,lowered:256" in b.describe() and "calibration=cap:10,windows:5,lowered:256" in a.describe()
    # ... through a file and the environment, where the drop-in builds its model from a checkpoint file
    path = str(tmp_path / "recipe.calibration.json")
    a.save_calibration(path)
    saved = cal.read_file(path)
    assert (saved["channels"], saved["depth"], saved["cap_log2"], saved["windows"]) == (8, 89, 10, 5) and np.array_equal(saved["lowering"], lowering)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in recipe["sd"].items()}, str(tmp_path / "recipe.pt"))
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7).items()}, str(tmp_path / "other.pt"))
    monkeypatch.setenv("C3HIP_CALIBRATION", path)
    c = build_model(pileup=False, add_indel_length=True, device="cuda:0", chkpnt_fn=str(tmp_path / "recipe.pt"))
    assert np.array_equal(c.predict_numpy(recipe["x7"]), ya) and "calibration=cap:10,windows:5,lowered:256" in c.describe()
    with pytest.raises(_lib.C3Error, match="another checkpoint"):
        build_model(pileup=False, add_indel_length=True, device="cuda:0", chkpnt_fn=str(tmp_path / "other.pt"))
    monkeypatch.setenv("C3HIP_CALIBRATION", str(tmp_path / "typo.json"))
    with pytest.raises(_lib.C3Error, match="typo.json"):
        build_model(pileup=False, add_indel_length=True, device="cuda:0", chkpnt_fn=str(tmp_path / "recipe.pt"))
    monkeypatch.delenv("C3HIP_CALIBRATION")
    # ... and off again: the uncalibrated handle's rows, bit for bit (on this recipe: the range guard's)
    plain = make_fa(recipe["sd"])
    y_plain = plain.predict_numpy(recipe["x7"])
    assert plain.range_status()[1], "uncalibrated, the recipe meets the range guard"
    b.set_calibration(None)
    b.load_state_dict(recipe["sd"])
    assert np.array_equal(b.predict_numpy(recipe["x7"]), y_plain) and "calibration=" not in b.describe()
    assert np.array_equal(b.calibration()["k"], b.calibration()["k0"])
    assert "continues on fp32" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------ 7, 8: every entry, verify mode
def test_every_entry_runs_the_calibrated_weights(recipe, calibrated):
    import torch
    m = calibrated[0]
    x = recipe["x7"]
    y = m.predict_numpy(x)
    t0, t1 = m.submit(x[:4], slot=0), m.submit(x[4:], slot=1)
    assert np.array_equal(np.concatenate([m.wait(t0), m.wait(t1)]), y), "two slots of submit / wait"
    yd = m(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y), "the device-resident entry"
    assert m.range_status() == (0, False)


def test_verify_mode_agrees_with_the_fp32_forms_on_the_calibrated_weights(recipe, calibrated):
    m = make_fa(recipe["sd"], lowering=calibrated[0].calibration()["lowering"])
    m.verify(every=1)
    for x in (recipe["x5"], recipe["x7"]):
        m.predict_numpy(x)
    st = m.verify_stats()
    print(f"verify mode on the calibrated recipe: {st}")
    assert st["batches_checked"] == 2 and st["windows_checked"] == 12 and st["batches_skipped"] == 0
    assert st["rows_over_tol"] == 0 and sum(st["label_diffs"]) == 0
    assert "precision=fp16x3" in m.describe() and m.range_status() == (0, False)


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals(recipe):
    p = Clair3_P(add_indel_length=False, predict=True, input_channels=18).to("cuda:0")
    p.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, False, seed=7))
    xp = syn.make_windows(syn.PILEUP, 4, seed=8)
    for call in (lambda: p.calibrate(xp), p.calibration, p.calibration_reset, lambda: p.set_calibration(np.zeros(896, np.uint8)),
                 lambda: p.load_calibration("unread.json")):
        with pytest.raises(_lib.C3Error, match="full-alignment"):
            call()
    m = make_fa(syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7))
    low = np.zeros(896, np.uint8)
    assert _lib.lib().c3_model_calibration_solve(m._handle, 10, low.ctypes.data) != 0 and "no census yet" in _lib.last_error()
    x = recipe["x5"]
    ticket = m.submit(x, slot=1)
    n = ctypes.c_int64(0)
    for call in (lambda: m.calibrate(x), m.calibration, m.calibration_reset, lambda: m.set_calibration(low)):
        with pytest.raises(_lib.C3Error, match="in flight"):
            call()
    assert _lib.lib().c3_model_calibration_solve(m._handle, 10, low.ctypes.data) != 0 and "in flight" in _lib.last_error()
    assert _lib.lib().c3_model_calibration_census(m._handle, None, ctypes.byref(n)) != 0 and "in flight" in _lib.last_error()
    y = m.wait(ticket)
    assert np.array_equal(y, m.predict_numpy(x)) and m.calibration()["windows"] == 0 and "calibration=" not in m.describe()
    with pytest.raises(_lib.C3Error, match="cap_log2"):
        m.calibrate(x, cap_log2=14)
    with pytest.raises(_lib.C3Error, match="896"):
        m.set_calibration(np.zeros(10, np.uint8))
