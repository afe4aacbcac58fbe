"""The per-layer precision plan on the device (c3_model_set_layer_precision; needs an MI355X): named layers on their fp32-MFMA forms, the
rest on fp16x3, at the smallest shapes that cross the tile edges.  An empty plan changes nothing, ``all`` is the C3HIP_FP32=1 handle,
layers upstream of the first named layer are bit-identical to a handle without a plan, every tapped layer stays within the suite's layer
gate (2e-5 of max(1, range) against the fp64 oracle, tests/test_product_layers_gpu.py) and rows within 2e-5 of the oracle's."""
import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model
from tests.test_product_layers_gpu import FA_TAPS, P_TAPS, Oracle, _gx2, tapped

pytestmark = pytest.mark.gpu

ENV = ("C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_AUTO_FP32", "C3HIP_CONV1_FUSED", "C3HIP_SPP_FUSED", "C3HIP_HALF_TILES",
       "C3HIP_WINO", "C3HIP_KEEP_ACTIVATIONS")
LAYER_GATE = 2e-5
CACHE = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def cached(key, make):
    if key not in CACHE:
        CACHE[key] = make()
    return CACHE[key]


def model(kind, ch, sd, monkeypatch, env=None, plan=None, taps=None, depth=None):
    """a handle created under `env` (the switches are read in c3_model_create), with a plan and taps"""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        m = make_model(kind, ch, True, sd, depth=depth)
    finally:
        for k in env or {}:
            monkeypatch.delenv(k)
    if plan is not None:
        m.layer_precision(plan)
    if taps:
        m.tap(taps)
    return m


def run(m, x):
    """one forward pass over the whole batch through the ring"""
    return m.wait(m.submit(x, slot=0))


def split22(x):
    """a value as the two fp16 pieces of a plane activation hold it"""
    h0 = x.astype(np.float16)
    h1 = (x - h0.astype(np.float32)).astype(np.float16)
    return h0.astype(np.float32) + h1.astype(np.float32)


# ------------------------------------------------------------------------------------------ pileup
P_ORDER = ("lstm1", "proj2", "lstm2", "l4")  # the layer that writes P_TAPS[i]
# (batch, window dtype, C3HIP_HALF_TILES): 8-window tiles (one, and three with a ragged last one), 16-window tiles (two and three, ragged)
P_CASES = [(1, np.int8, "1"), (17, np.int8, "1"), (17, np.int8, "0"), (40, np.int32, "1"), (40, np.int8, "0")]


def p_pool():
    def make():
        sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=51)
        x = syn.make_pileup_windows(40, seed=52)
        orc = Oracle(syn.PILEUP, sd, x, True)
        y, d = orc(np.arange(40))
        d = dict(d)
        d["gx2"] = _gx2(sd, d["lstm1_out"])
        return sd, x, y, d
    return cached("p_pool", make)


def p_taps(m, n, d):
    return {k: tapped(m, k, np.arange(n), d[k].shape[1:]) for k in P_TAPS}


def p_reference(case, fp32, monkeypatch):
    """rows and taps of the handle without a plan (fp32: of the C3HIP_FP32=1 handle) for one case"""
    n, dt, half = case
    sd, x, _, d = p_pool()

    def make():
        env = {"C3HIP_HALF_TILES": half}
        if fp32:
            env["C3HIP_FP32"] = "1"
        m = model(syn.PILEUP, 18, sd, monkeypatch, env, taps=P_TAPS)
        y = run(m, x[:n].astype(dt))
        return y, p_taps(m, n, d), m.describe()
    return cached(("p_ref", n, np.dtype(dt).name, half, fp32), make)


def fa_pool(weights, ch, depth):
    def make():
        seed = {"plain": 41, "peaked": 43, "trained_like": 141}[weights]
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, True, seed=seed, peaked=weights != "plain", trained_like=weights == "trained_like")
        x = syn.make_fa_windows(3, seed=seed + 1, channels=ch, depth=depth)
        y, d = Oracle(syn.FULL_ALIGNMENT, sd, x, True)(np.arange(3))
        return sd, x, y, d
    return cached(("fa_pool", weights, ch, depth), make)


# ------------------------------------------------------------------------------------------ 1. the empty plan
@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_empty_plan_changes_nothing(kind, monkeypatch):
    if kind == syn.PILEUP:
        sd, x, _, _ = p_pool()
        x, ch, plan = x[:17], 18, "lstm1,l4"
    else:
        sd, x, _, _ = fa_pool("plain", 8, 89)
        ch, plan = 8, "res2a,res3b"
    m = model(kind, ch, sd, monkeypatch)
    y0, d0 = run(m, x), m.describe()
    assert "fp32_layers" not in d0 and m.layer_precision() == ()
    m.layer_precision("")
    assert np.array_equal(run(m, x), y0) and m.describe() == d0
    m.layer_precision(plan)
    y1, d1 = run(m, x), m.describe()
    assert f" fp32_layers={plan}" in d1 and m.layer_precision() == tuple(plan.split(",")) and "on_fp32=0" in d1 and "precision=fp16x3" in d1, d1
    assert not np.array_equal(y1, y0), "the plan ran the forms of the empty plan"
    m.layer_precision(())
    assert np.array_equal(run(m, x), y0) and m.describe() == d0 and m.layer_precision() == ()
    assert np.array_equal(m.predict_numpy(x), y0)


# ------------------------------------------------------------------------------------------ 2. `all`
@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_all_is_the_fp32_handle(kind, monkeypatch):
    if kind == syn.PILEUP:
        sd, x, _, _ = p_pool()
        x, ch = x[:17], 18
    else:
        sd, x, _, _ = fa_pool("plain", 8, 89)
        ch = 8
    m32 = model(kind, ch, sd, monkeypatch, {"C3HIP_FP32": "1"})
    y32, d32 = run(m32, x), m32.describe()
    m = model(kind, ch, sd, monkeypatch, plan="all")
    y, d = run(m, x), m.describe()
    assert np.array_equal(y, y32), float(np.abs(y - y32).max())
    if kind == syn.PILEUP:
        assert "lstm1=fused-fp32-mfma proj2=fp32-mfma lstm2=fp32-mfma" in d and "lstm1=fused-fp32-mfma proj2=fp32-mfma lstm2=fp32-mfma" in d32, (d, d32)
        assert m.layer_precision() == P_ORDER
    else:
        assert "conv_stack=fp32-mfma" in d and "conv_stack=fp32-mfma" in d32, (d, d32)
        assert m.layer_precision() == ("conv1", "res1a", "res1b", "conv3", "res2a", "res2b", "conv5", "res3a", "res3b", "l4")
    # ... and C3HIP_FP32=1 wins over a plan: the whole handle is on fp32 whatever the plan names
    mw = model(kind, ch, sd, monkeypatch, {"C3HIP_FP32": "1", "C3HIP_FP32_LAYERS": "l4"})
    assert np.array_equal(run(mw, x), y32) and "on_fp32=1" in mw.describe()


# ------------------------------------------------------------------------------------------ 3. pileup, each single name
P_FORM = {"lstm1": "lstm1=fused-fp32-mfma-planes ", "proj2": "proj2=fp32-mfma ", "lstm2": "lstm2=fp32-mfma ", "l4": None}


@pytest.mark.parametrize("name", P_ORDER)
def test_pileup_single_layer(name, monkeypatch):
    sd, x, y_o, d = p_pool()
    at = P_ORDER.index(name)
    for case in P_CASES:
        n, dt, half = case
        y_plain, t_plain, d_plain = p_reference(case, False, monkeypatch)
        m = model(syn.PILEUP, 18, sd, monkeypatch, {"C3HIP_HALF_TILES": half}, plan=name, taps=P_TAPS)
        y = run(m, x[:n].astype(dt))
        form, what = m.describe(), f"plan {name} n={n} {np.dtype(dt).name} half_tiles={half}"
        assert f" fp32_layers={name}" in form and "on_fp32=0" in form and "precision=fp16x3" in form, form
        # the named layer on its fp32 form, every other layer on the form (and tile shape) the handle without a plan takes
        for k in ("lstm1", "proj2", "lstm2"):
            mine, plain = form.split(f" {k}=")[1].split()[0], d_plain.split(f" {k}=")[1].split()[0]
            if k == name:
                assert P_FORM[k] == f"{k}={mine} " and "fp32" not in plain, (what, form, d_plain)
            else:
                assert mine == plain, (what, k, form, d_plain)
        t = p_taps(m, n, d)
        for k in P_TAPS[:at]:
            assert np.array_equal(t[k], t_plain[k]), (what, k, "upstream of the named layer")
        assert not np.array_equal(t[P_TAPS[at]], t_plain[P_TAPS[at]]), (what, "the named layer ran its product form")
        err = {k: float(np.abs(t[k] - d[k][:n]).max()) / max(1.0, float(np.abs(d[k][:n]).max())) for k in P_TAPS}
        err["y"] = util.assert_rows_match(y, y_o[:n], tol=2e-5, what=what)
        print(f"{what}: " + " ".join(f"{k}={v * 1e6:.2f}e-6" for k, v in err.items()))
        for k, v in err.items():
            assert v <= LAYER_GATE, (what, k, v)
        if name == "lstm1":  # the fp32 recurrence, handed over as the two fp16 pieces the product projection reads
            t32 = p_reference(case, True, monkeypatch)[1]
            assert np.array_equal(t["lstm1_out"], split22(t32["lstm1_out"])), what


# ------------------------------------------------------------------------------------------ 4. the recurrences of the sensitive window
SENSITIVE = (925999917, 549)  # tests/test_parity_gpu.py test_precision_escalates_without_a_switch
RECURRENT = "lstm1,proj2,lstm2"


def sensitive_tile():
    def make():
        from oracle import oracle
        seed, w = SENSITIVE
        sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=seed, peaked=False, trained_like=True)
        x = syn.make_pileup_windows(920, seed=seed, recipe="realistic")
        lo = w - w % 16
        xs = x[lo:lo + 16]
        return sd, xs, oracle.pileup_forward(sd, xs, True)
    return cached("sensitive", make)


def sensitive_plan_rows(monkeypatch):
    sd, xs, _ = sensitive_tile()

    def make():
        m = model(syn.PILEUP, 18, sd, monkeypatch, {"C3HIP_FP32": "0"}, plan=RECURRENT, taps=P_TAPS)
        y = run(m, xs)
        shapes = {"lstm1_out": (33, 256), "gx2": (33, 1280), "lstm2_out": (33, 320)}
        return y, {k: tapped(m, k, np.arange(16), s) for k, s in shapes.items()}, m.describe()
    return cached("sensitive_plan", make)


def test_recurrent_plan_on_the_sensitive_window(monkeypatch):
    sd, xs, y_o = sensitive_tile()
    y, t, form = sensitive_plan_rows(monkeypatch)
    assert f" fp32_layers={RECURRENT}" in form and "on_fp32=0" in form and "precision=fp16x3" in form, form
    assert "lstm1=fused-fp32-mfma proj2=fp32-mfma lstm2=fp32-mfma" in form, form
    m32 = model(syn.PILEUP, 18, sd, monkeypatch, {"C3HIP_FP32": "1"}, taps=P_TAPS)
    y32 = run(m32, xs)
    for k in t:  # the same kernels on the same inputs
        assert np.array_equal(t[k], tapped(m32, k, np.arange(16), t[k].shape[1:])), k
    err, err32 = float(np.abs(y - y_o).max()), float(np.abs(y32 - y_o).max())
    print(f"sensitive tile: plan {RECURRENT} |Y - exact| = {err:.3e}, all-fp32 handle {err32:.3e}, |plan - fp32| = {np.abs(y - y32).max():.3e}")
    assert err <= 1e-4, err


# ------------------------------------------------------------------------------------------ 5. full alignment
FA_ORDER = ("conv1", "res1a", "res1b", "conv3", "res2a", "res2b", "conv5", "res3a", "res3b", "l4")
FA_PLANS = ("conv1", "res1b", "conv3", "res2a", "res3b", "l4", "res2a,res2b")
# (weights, channels, depth, batch): M = 765 B (not a multiple of 128); the 9-channel window; 28 x 9 images whose pooling is never fused
FA_CASES = [("plain", 8, 89, 1), ("plain", 8, 89, 3), ("trained_like", 9, 89, 3), ("peaked", 9, 55, 3)]


def fa_switches(plan):
    """the fusion switches a plan implies"""
    env = {}
    if set(plan.split(",")) & {"conv1", "res1a", "res1b"}:
        env["C3HIP_CONV1_FUSED"] = "0"
    if "res3b" in plan.split(","):
        env["C3HIP_SPP_FUSED"] = "0"
    return env


def fa_taps(m, n, d, env, depth):
    names = list(FA_TAPS)
    if env.get("C3HIP_CONV1_FUSED") != "0":
        names.remove("act0")  # computed inside res1a / res1b
    if env.get("C3HIP_SPP_FUSED") != "0" and depth == 89:
        names.remove("act8")  # pooled inside res3b
    return {k: tapped(m, k, np.arange(n), d[k].shape[1:]) for k in names}


@pytest.mark.parametrize("weights,ch,depth,n", FA_CASES)
def test_full_alignment_plans(weights, ch, depth, n, monkeypatch):
    sd, x, y_o, d = fa_pool(weights, ch, depth)
    x, y_o = x[:n], y_o[:n]
    d = {k: v[:n] for k, v in d.items()}
    plain = {}
    for plan in FA_PLANS:
        env = fa_switches(plan)
        key = tuple(sorted(env.items()))
        if key not in plain:  # the handle without a plan under the fusion switches the plan implies
            mp = model(syn.FULL_ALIGNMENT, ch, sd, monkeypatch, env, taps=FA_TAPS, depth=depth)
            yp = run(mp, x)
            plain[key] = (yp, fa_taps(mp, n, d, env, depth), mp.describe())
        y_plain, t_plain, d_plain = plain[key]
        m = model(syn.FULL_ALIGNMENT, ch, sd, monkeypatch, plan=plan, taps=FA_TAPS, depth=depth)  # (no switch set: the plan implies them)
        y = run(m, x)
        form, what = m.describe(), f"{weights} C={ch} depth={depth} n={n} plan {plan}"
        assert f" fp32_layers={plan}" in form and "on_fp32=0" in form and "conv_stack=planes-f16x3" in form and "precision=fp16x3" in form, form
        t = fa_taps(m, n, d, env, depth)
        assert set(t) == set(t_plain)
        first = min(FA_ORDER.index(p) for p in plan.split(","))
        upstream = [k for k in t if k.startswith("act") and int(k[3:]) < first] + (["spp"] if first == 9 else [])
        for k in upstream:
            assert np.array_equal(t[k], t_plain[k]), (what, k, "upstream of the first named layer")
        out = "l4_out" if first == 9 else f"act{first}"
        assert not np.array_equal(t[out], t_plain[out]), (what, "the named layer ran its product form")
        # the stride-1 layers: f where the plan names one, the plain handle's form everywhere else
        s1, s1_plain = form.split("stride1=")[1].split()[0], d_plain.split("stride1=")[1].split()[0]
        for i, k in enumerate(("res1a", "res1b", "res2a", "res2b", "res3a", "res3b")):
            assert s1[i] == ("f" if k in plan.split(",") else s1_plain[i]), (what, form, d_plain)
        assert ("conv3=fp32-mfma" in form) == ("conv3" in plan.split(",")), form
        whole, chan = util.layer_errors(lambda k: t[k], d, list(t), sd)
        whole["y"] = util.assert_rows_match(y, y_o, tol=2e-5, what=what)
        print(f"{what}: " + " ".join(f"{k}={whole[k] * 1e6:.2f}" + (f"/{chan[k] * 1e6:.2f}" if k in chan else "") for k in whole) + " (x1e-6)")
        for k in t:
            assert whole[k] <= LAYER_GATE, (what, k, whole[k])


# ------------------------------------------------------------------------------------------ 6. rows do not depend on the batch
@pytest.mark.parametrize("kind,plan", [(syn.PILEUP, "lstm1"), (syn.PILEUP, "proj2,l4"), (syn.FULL_ALIGNMENT, "res2a,res2b"),
                                       (syn.FULL_ALIGNMENT, "conv1,res3b")])
def test_batch_slot_and_entry_independence(kind, plan, monkeypatch):
    import torch
    if kind == syn.PILEUP:
        sd, x, _, _ = p_pool()
        x, ch = x[:17], 18
    else:
        sd, x, _, _ = fa_pool("plain", 8, 89)
        ch = 8
    m = model(kind, ch, sd, monkeypatch, plan=plan)
    y = run(m, x)
    for k in (0, len(x) // 2, len(x) - 1):  # a window alone
        assert np.array_equal(m.predict_numpy(x[k:k + 1])[0], y[k]), (plan, k)
    ta, tb = m.submit(x[:2], slot=0), m.submit(x[1:], slot=1)  # two slots in flight (two lanes)
    ya, yb = m.wait(ta), m.wait(tb)
    assert np.array_equal(ya, y[:2]) and np.array_equal(yb, y[1:]), plan
    xd = torch.from_numpy(x).cuda()
    yd = m(xd)  # device resident
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y), plan
    assert np.array_equal(m.forward(xd, checked=True).cpu().numpy(), y) and m.range_status() == (0, False)
    assert f" fp32_layers={plan}" in m.describe()


# ------------------------------------------------------------------------------------------ 7. the range guard
def test_range_guard_moves_a_plan_handle_to_fp32(monkeypatch, capfd):
    """the weights of tests/test_parity_gpu.py test_activations_beyond_the_fp16_range_fall_back_to_fp32"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=61)
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    for k in ("conv3.conv.weight", "conv3.conv.bias", "conv3.bn.running_mean"):
        sd[k] *= 4.0e6
    for k in ("res_block2.0.conv1.weight", "res_block2.0.conv2.weight"):
        sd[k] /= 2.0e3
    sd["conv5.conv.weight"] /= 4.0e6
    x = syn.make_fa_windows(5, seed=62)
    y32 = run(model(syn.FULL_ALIGNMENT, 8, sd, monkeypatch, {"C3HIP_FP32": "1"}), x)
    assert np.isfinite(y32).all()
    for plan in ("res2a", "conv3"):  # the overflowing stage read by an fp32 layer / written by one: the flag is raised either way
        m = model(syn.FULL_ALIGNMENT, 8, sd, monkeypatch, plan=plan)
        y = m.predict_numpy(x)
        form = m.describe()
        assert "precision=fp32-range-guard" in form and "on_fp32=1" in form and "conv_stack=fp32-mfma" in form, (plan, form)
        assert np.array_equal(y, y32), plan
        assert np.array_equal(m.predict_numpy(x), y32) and m.range_status()[1]
        assert "continues on fp32" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------ 8. verify mode
@pytest.mark.parametrize("kind,plan", [(syn.PILEUP, "lstm1"), (syn.FULL_ALIGNMENT, "res2a")])
def test_verify_mode_on_a_plan_handle(kind, plan, monkeypatch):
    if kind == syn.PILEUP:
        sd, x, _, _ = p_pool()
        x, ch = x[:17], 18
    else:
        sd, x, _, _ = fa_pool("plain", 8, 89)
        ch = 8
    m = model(kind, ch, sd, monkeypatch, plan=plan)
    y0, d0 = run(m, x), m.describe()
    m.verify(every=1, layers=True)
    y1 = run(m, x)
    assert np.array_equal(y1, y0), "verify mode changed the plan's rows"
    assert m.describe().split(" verify=")[0] == d0, (m.describe(), d0)
    st = m.verify_stats()
    assert st["batches_checked"] == 1 and st["batches_skipped"] == 0 and st["windows_checked"] == len(x), st
    assert st["rows_over_tol"] == 0 and sum(st["label_diffs"]) == 0, st  # the plan's rows against the all-fp32 forms, at verify mode's own 1e-4
    table = {e["name"]: e for e in m.verify_layers()}
    print("\n".join(f"  {k}: {e['status']} rel={e['rel']:.3e}" for k, e in table.items()))
    want = P_TAPS if kind == syn.PILEUP else tuple(f"act{l}" for l in range(1, 8)) + ("spp", "l4_out")
    for k in want:
        assert table[k]["status"] == "compared" and table[k]["windows"] == len(x) and np.isfinite(table[k]["rel"]), (k, table[k])
    assert np.array_equal(run(m, x), y0) and m.verify_stats()["batches_checked"] == 2


# ------------------------------------------------------------------------------------------ 9. errors and the environment
def test_errors_leave_the_plan_unchanged(monkeypatch):
    sd, x, _, _ = p_pool()
    m = model(syn.PILEUP, 18, sd, monkeypatch, plan="lstm2")
    for bad, why in (("lstm2,conv3", '"conv3" is a layer of the full-alignment network'), ("lstm9", 'unknown layer "lstm9"'), ("lstm2,,l4", "empty entry")):
        with pytest.raises(_lib.C3Error, match=why):
            m.layer_precision(bad)
        assert _lib.lib().c3_model_set_layer_precision(m._handle, bad.encode()) != 0 and why.encode() in _lib.lib().c3_last_error()
        assert m.layer_precision() == ("lstm2",)
    t = m.submit(x[:17], slot=0)
    with pytest.raises(_lib.C3Error, match="in flight"):
        m.layer_precision("l4")
    y = m.wait(t)
    assert m.layer_precision() == ("lstm2",) and " fp32_layers=lstm2" in m.describe() and "lstm2=fp32-mfma" in m.describe()
    m.load_state_dict(sd)  # the plan belongs to the handle: a load keeps it
    assert m.layer_precision() == ("lstm2",) and np.array_equal(run(m, x[:17]), y)
    m.layer_precision(["l4", "lstm2", "l4"])  # naming a layer twice is accepted; reported in network order
    assert m.layer_precision() == ("lstm2", "l4")


def test_environment_sets_the_initial_plan(monkeypatch):
    sd, x, _, _ = p_pool()
    m = model(syn.PILEUP, 18, sd, monkeypatch, {"C3HIP_FP32_LAYERS": "lstm2"})
    assert m.layer_precision() == ("lstm2",) and " fp32_layers=lstm2" in m.describe()
    y = run(m, x[:17])
    assert "lstm2=fp32-mfma" in m.describe() and "lstm1=fused-f16x3" in m.describe()
    assert np.array_equal(y, run(model(syn.PILEUP, 18, sd, monkeypatch, plan="lstm2"), x[:17]))
    # with C3HIP_FP32=0 an explicit plan still applies
    m0 = model(syn.PILEUP, 18, sd, monkeypatch, {"C3HIP_FP32": "0", "C3HIP_FP32_LAYERS": "lstm2"})
    assert np.array_equal(run(m0, x[:17]), y) and "lstm2=fp32-mfma" in m0.describe()
    for var in ("C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS"):
        for bad in ("lstm2,res2a", "lstm2,,l4", "everything"):
            with pytest.raises(_lib.C3Error, match=var):
                model(syn.PILEUP, 18, sd, monkeypatch, {var: bad})
    with pytest.raises(_lib.C3Error, match="C3HIP_FP32_LAYERS.*lstm2"):
        model(syn.FULL_ALIGNMENT, 8, fa_pool("plain", 8, 89)[0], monkeypatch, {"C3HIP_FP32_LAYERS": "lstm2"})


def test_load_time_rule_escalates_the_named_layers(monkeypatch):
    sd, xs, y_o = sensitive_tile()
    y_plan = sensitive_plan_rows(monkeypatch)[0]
    m = model(syn.PILEUP, 18, sd, monkeypatch, {"C3HIP_AUTO_FP32_LAYERS": RECURRENT})
    assert f"precision=fp32-auto({RECURRENT}) " in m.describe() and "on_fp32=0" in m.describe(), m.describe()
    assert m.range_status() == (0, False) and m.layer_precision() == tuple(RECURRENT.split(","))
    y = run(m, xs)
    assert np.array_equal(y, y_plan) and float(np.abs(y - y_o).max()) <= 1e-4
    assert "lstm1=fused-fp32-mfma proj2=fp32-mfma lstm2=fp32-mfma" in m.describe() and f" fp32_layers={RECURRENT}" in m.describe(), m.describe()
    # weights the rule does not fire on: nothing is escalated, and a reload decides again
    sd_plain = syn.make_state_dict(syn.PILEUP, 18, True, seed=SENSITIVE[0])
    m.load_state_dict(sd_plain)
    assert "precision=fp16x3" in m.describe() and "fp32_layers" not in m.describe() and m.layer_precision() == ()
    m.load_state_dict(sd)
    assert f"precision=fp32-auto({RECURRENT}) " in m.describe() and np.array_equal(run(m, xs), y_plan)
    # unset: the whole handle, as before
    mu = model(syn.PILEUP, 18, sd, monkeypatch)
    run(mu, xs)
    du = mu.describe()
    assert "precision=fp32-auto " in du and "on_fp32=1" in du and "lstm_wmax=8 " in du and "fp32_layers" not in du, du
    assert mu.range_status() == (0, True)
    # C3HIP_FP32=0 switches the rule off, the variable with it
    mo = model(syn.PILEUP, 18, sd, monkeypatch, {"C3HIP_FP32": "0", "C3HIP_AUTO_FP32_LAYERS": RECURRENT})
    assert "precision=fp16x3" in mo.describe() and "fp32_layers" not in mo.describe()
