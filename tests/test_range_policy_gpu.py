"""The range-guard policy on the device (c3_model_set_range_policy; needs an MI355X): a handle that meets the range guard on the suite's
out-of-range recipe recalibrates from the batch that tripped it and stays on the fp16x3 kernels -- through the blocking call, the ring and
its lanes, rows input and the reference's worker command -- and a handle without the policy does what it always did."""
import os

import numpy as np
import pytest

from clair3_amd import _lib, predict, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import refloop, util
from tests.test_calibration import recipe_state_dict

pytestmark = pytest.mark.gpu

HEALED = "recalibrated from this batch"
STICKY = "continues on fp32"


def make_fa(sd, policy=None, max_recalibrations=4):
    m = Clair3_F(add_indel_length=True, predict=True, input_channels=8).to("cuda:0")
    if policy is not None:
        m.range_policy(policy, max_recalibrations)  # before the load: the library keeps the tensors it is given
    m.load_state_dict(sd)
    return m


def guard_lines(err):
    return [line for line in err.splitlines() if line.startswith("libc3hip: activations beyond")]


@pytest.fixture(scope="module")
def recipe():
    """the suite's out-of-range recipe (tests/test_calibration.py), the two batches the calibration suite trips the guard with, the fp64
    oracle on both and what a sticky handle answers: computed once, read by every test"""
    from oracle import oracle
    sd = recipe_state_dict()
    x5, x7 = syn.make_fa_windows(5, seed=62), syn.make_fa_windows(7, seed=63)
    sticky = make_fa(sd)
    return dict(sd=sd, x5=x5, x7=x7, y5=oracle.fa_forward(sd, x5, True), y7=oracle.fa_forward(sd, x7, True),
                s7=sticky.predict_numpy(x7), s5=sticky.predict_numpy(x5))


def healed_handle(recipe, capfd):
    """a handle under the policy after the one blocking call that trips it; (handle, rows of that call, its stderr)"""
    m = make_fa(recipe["sd"], "recalibrate")
    capfd.readouterr()
    y = m.predict_numpy(recipe["x7"])
    return m, y, capfd.readouterr().err


def assert_healed(m, err, windows=7):
    assert m.range_status() == (0, False)
    text = m.describe()
    for part in ("precision=fp16x3", "conv_stack=planes-f16x3", f"calibration=cap:10,windows:{windows},lowered:", "range_guard=recalibrate,recalibrations:1"):
        assert part in text, (part, text)
    assert "fell_back" not in text
    assert HEALED in err and STICKY not in err and len(guard_lines(err)) == 1, err
    assert f"census of {windows} windows); this handle stays on the fp16x3 kernels" in err
    st = m.range_stats()
    assert (st["trips"], st["recalibrations"], st["fell_back"], st["census_windows"], st["cap_log2"]) == (1, 1, "", windows, 10), st
    assert st["channels_lowered"] > 0


def assert_on_the_product_path_within_tolerance(m, recipe, capfd, what):
    """test 4's assertions: rows against the oracle, a bounded number of recalibrations, no fall-back, the handle on fp16x3"""
    st = m.range_stats()
    assert 1 <= st["recalibrations"] <= 2 and st["fell_back"] == "", st
    assert "precision=fp16x3" in m.describe() and not m.range_status()[1], what
    assert STICKY not in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------ 1: the default
def test_default_is_untouched(recipe, capfd):
    m = make_fa(recipe["sd"])
    capfd.readouterr()
    y = m.predict_numpy(recipe["x7"])
    err = capfd.readouterr().err
    assert STICKY in err and HEALED not in err and "(range guard:" not in err
    assert m.range_status()[1] and "range_guard=" not in m.describe() and "precision=fp32-range-guard" in m.describe()
    assert np.array_equal(y, recipe["s7"])
    st = m.range_stats()
    assert (st["policy"], st["trips"], st["recalibrations"], st["reruns"], st["fell_back"]) == ("sticky", 0, 0, 0, "")


# ------------------------------------------------------------------------------------------------ 2: heals
def test_a_trip_recalibrates_and_the_handle_stays_on_fp16x3(recipe, capfd):
    m, y, err = healed_handle(recipe, capfd)
    assert np.array_equal(y, recipe["s7"]), "the rows that answer the batch are the fp32 re-run's, bit for bit the sticky guard's"
    assert_healed(m, err)
    y2 = m.predict_numpy(recipe["x7"])
    e = util.assert_rows_match(y2, recipe["y7"], tol=util.PROB_TOL, what="healed handle, the batch again")
    print(f"healed handle, x7 again on the product path: max |dY| against the oracle = {e:.3e}")
    assert not guard_lines(capfd.readouterr().err), "no new trip"
    assert m.range_stats()["trips"] == 1 and m.range_status() == (0, False) and "conv_stack=planes-f16x3" in m.describe()


# ------------------------------------------------------------------------------------------------ 3: the state of the offline tool
def test_same_state_as_the_offline_calibration(recipe, capfd, tmp_path):
    healed, _, _ = healed_handle(recipe, capfd)
    offline = make_fa(recipe["sd"])
    offline.calibrate(recipe["x7"])
    a, b = healed.calibration(), offline.calibration()
    assert np.array_equal(a["lowering"], b["lowering"]) and np.array_equal(a["k"], b["k"]) and np.array_equal(a["k0"], b["k0"])
    assert np.array_equal(a["census"], b["census"]) and a["windows"] == b["windows"] == 7
    # what was learned online travels as a calibration file
    path = str(tmp_path / "online.calibration.json")
    healed.save_calibration(path)
    fresh = make_fa(recipe["sd"])
    fresh.load_calibration(path)
    assert np.array_equal(fresh.calibration()["k"], a["k"]) and "calibration=cap:10,windows:7,lowered:" in fresh.describe()
    capfd.readouterr()
    ya, yb = healed.predict_numpy(recipe["x5"]), offline.predict_numpy(recipe["x5"])
    if healed.range_stats()["trips"] == 1 and not offline.range_status()[1]:  # neither tripped on the batch the census did not see
        assert np.array_equal(ya, yb) and np.array_equal(fresh.predict_numpy(recipe["x5"]), ya)
        assert not guard_lines(capfd.readouterr().err)
    else:
        util.assert_rows_match(ya, recipe["y5"], tol=util.PROB_TOL, what="healed handle, x5")
        assert_on_the_product_path_within_tolerance(healed, recipe, capfd, "healed handle, x5")


# ------------------------------------------------------------------------------------------------ 4: the ring and its lanes
@pytest.mark.parametrize("lanes", [None, "1"])
def test_three_batches_in_flight_across_a_recalibration(lanes, recipe, capfd, monkeypatch):
    if lanes:
        monkeypatch.setenv("C3HIP_RING_LANES", lanes)
    m = make_fa(recipe["sd"], "recalibrate")
    assert f"ring_lanes={lanes or 3}" in m.describe()
    capfd.readouterr()
    tickets = [m.submit(x, slot=k) for k, x in enumerate((recipe["x5"], recipe["x7"], recipe["x5"]))]
    rows = [m.wait(t) for t in tickets]
    for k, (y, want) in enumerate(zip(rows, (recipe["y5"], recipe["y7"], recipe["y5"]))):
        e = util.assert_rows_match(y, want, tol=util.PROB_TOL, what=f"slot {k}")
        print(f"lanes={lanes or 3} slot {k}: max |dY| against the oracle = {e:.3e}")
    assert np.array_equal(rows[0], recipe["s5"]), "the batch that tripped is answered by its fp32 re-run"
    st = m.range_stats()
    print(f"lanes={lanes or 3}: {st}")
    assert st["reruns"] >= 1, "the batches in flight across the recalibration ran again on the new weights"
    assert_on_the_product_path_within_tolerance(m, recipe, capfd, f"lanes={lanes}")


# ------------------------------------------------------------------------------------------------ 5: rows input
def test_a_rows_batch_expands_again_for_the_census(recipe, capfd):
    rows, firsts, counts = predict.pack_rows(recipe["x7"])
    sticky = make_fa(recipe["sd"])
    want = sticky.wait(sticky.submit_rows(rows, counts, firsts, slot=0))
    assert np.array_equal(want, recipe["s7"])
    m = make_fa(recipe["sd"], "recalibrate")
    capfd.readouterr()
    y = m.wait(m.submit_rows(rows, counts, firsts, slot=0))
    err = capfd.readouterr().err
    assert np.array_equal(y, want)
    assert_healed(m, err)
    assert np.array_equal(m.calibration()["census"], healed_handle(recipe, capfd)[0].calibration()["census"]), "the census of the dense windows"
    capfd.readouterr()
    y2 = m.wait(m.submit_rows(rows, counts, firsts, slot=1))
    util.assert_rows_match(y2, recipe["y7"], tol=util.PROB_TOL, what="healed handle, rows again")
    assert not guard_lines(capfd.readouterr().err) and m.range_stats()["trips"] == 1 and "rows_windows=7" in m.describe()


def test_the_checked_device_entry_recalibrates_and_the_unchecked_one_stays_outside(recipe, capfd):
    import torch
    xd = torch.from_numpy(recipe["x7"]).cuda()
    m = make_fa(recipe["sd"], "recalibrate")
    capfd.readouterr()
    y = m.forward(xd, checked=True).cpu().numpy()  # c3_predict_device_checked: synchronises, reads the flag, recalibrates
    err = capfd.readouterr().err
    assert np.array_equal(y, recipe["s7"])
    assert_healed(m, err)
    util.assert_rows_match(m.forward(xd, checked=True).cpu().numpy(), recipe["y7"], tol=util.PROB_TOL, what="the checked entry on the healed handle")
    assert m.range_stats()["trips"] == 1 and not guard_lines(capfd.readouterr().err)
    plain = make_fa(recipe["sd"], "recalibrate")
    plain(xd)  # c3_predict_device: asynchronous, unchecked, unchanged
    torch.cuda.synchronize()
    assert plain.range_status() == (1, False) and plain.range_stats()["trips"] == 0 and "calibration=" not in plain.describe()
    assert not guard_lines(capfd.readouterr().err)


# ------------------------------------------------------------------------------------------------ 6: bounded
def test_an_allowance_of_zero_is_the_sticky_guard(recipe, capfd):
    sticky = make_fa(recipe["sd"])
    capfd.readouterr()
    want = sticky.predict_numpy(recipe["x7"])
    sticky_err = guard_lines(capfd.readouterr().err)
    m = make_fa(recipe["sd"], "recalibrate", 0)
    y = m.predict_numpy(recipe["x7"])
    assert guard_lines(capfd.readouterr().err) == sticky_err and len(sticky_err) == 1
    assert np.array_equal(y, want) and m.range_status() == sticky.range_status() and m.range_status()[1]
    assert "precision=fp32-range-guard" in m.describe() and m.range_stats()["recalibrations"] == 0


def test_a_census_that_is_not_finite_falls_back(recipe, capfd):
    sd = {k: np.array(v, copy=True) for k, v in recipe["sd"].items()}
    sd["conv5.conv.bias"][0] = np.inf
    want = make_fa(sd).predict_numpy(recipe["x7"])
    m = make_fa(sd, "recalibrate")
    capfd.readouterr()
    y = m.predict_numpy(recipe["x7"])
    err = capfd.readouterr().err
    assert np.array_equal(y, want, equal_nan=True)
    st = m.range_stats()
    assert "census not finite" in st["fell_back"] and (st["trips"], st["recalibrations"]) == (1, 0), st
    assert STICKY in err and "census not finite" in err and HEALED not in err
    text = m.describe()
    assert "precision=fp32-range-guard" in text and "range_guard=recalibrate,recalibrations:0,fell_back" in text and m.range_status()[1]
    assert np.array_equal(m.predict_numpy(recipe["x7"]), want, equal_nan=True), "later batches: the sticky behaviour"
    assert not guard_lines(capfd.readouterr().err) and m.range_stats()["trips"] == 1


@pytest.fixture(scope="module")
def heat(recipe):
    """Three levels of heat, each beyond what a census of the one before leaves room for at cap 2^13 (16000 / 8192 = 1.95x): two all-zero
    windows, x7, two windows of 127 everywhere.  On the fp64 oracle, with the rule in numpy: calibrated on the zeros at cap 13, x7 reaches
    25956 (the guard flags 16000); after a recalibration on x7 at that cap, the 127s reach 27525 and x5 9478.  With the oracle and the sticky
    handle's rows for the 127s"""
    from oracle import oracle
    zeros, hot = np.zeros_like(recipe["x7"][:2]), np.full_like(recipe["x7"][:2], 127)
    return dict(zeros=zeros, hot=hot, y_hot=oracle.fa_forward(recipe["sd"], hot, True), s_hot=make_fa(recipe["sd"]).predict_numpy(hot))


def calibrated_on_zeros_at_cap_13(recipe, heat, max_recalibrations):
    """a handle calibrated ahead of time on the coolest batch at cap 13, THEN put under the policy: it starts from that lowering and solves at its cap"""
    m = make_fa(recipe["sd"])
    m.calibrate(heat["zeros"], cap_log2=13)
    assert "calibration=cap:13,windows:2,lowered:" in m.describe()
    m.range_policy("recalibrate", max_recalibrations)  # (a loaded handle: created anew, the lowering and its origin travel)
    assert "calibration=cap:13,windows:2,lowered:" in m.describe() and "range_guard=recalibrate,recalibrations:0" in m.describe()
    return m


def test_a_hotter_batch_trips_again_and_the_lowering_never_goes_up(recipe, heat, capfd):
    m = calibrated_on_zeros_at_cap_13(recipe, heat, 4)
    l0 = m.calibration()["lowering"]
    capfd.readouterr()
    assert np.array_equal(m.predict_numpy(recipe["x7"]), recipe["s7"])
    st, l1 = m.range_stats(), m.calibration()["lowering"]
    assert (st["trips"], st["recalibrations"], st["cap_log2"], st["census_windows"], st["fell_back"]) == (1, 1, 13, 7, ""), st
    assert "calibration=cap:13,windows:7,lowered:" in m.describe(), "solved at the cap of the lowering in force"
    assert (l1 >= l0).all() and st["channels_lowered"] == int((l1 != l0).sum()) > 0
    util.assert_rows_match(m.predict_numpy(recipe["x7"]), recipe["y7"], tol=util.PROB_TOL, what="x7 after the first recalibration")
    assert m.range_stats()["trips"] == 1
    assert np.array_equal(m.predict_numpy(heat["hot"]), heat["s_hot"]), "a further trip: answered by the fp32 rows again"
    st, l2 = m.range_stats(), m.calibration()["lowering"]
    assert (st["trips"], st["recalibrations"], st["census_windows"], st["fell_back"]) == (2, 2, 9, ""), st
    assert (l2 >= l1).all() and st["channels_lowered"] == int((l2 != l1).sum()) > 0
    for name, x, want in (("the 127s", heat["hot"], heat["y_hot"]), ("x7", recipe["x7"], recipe["y7"]), ("x5", recipe["x5"], recipe["y5"])):
        e = util.assert_rows_match(m.predict_numpy(x), want, tol=util.PROB_TOL, what=f"{name} after the second recalibration")
        print(f"{name} after two recalibrations at cap 13: max |dY| against the oracle = {e:.3e}")
    err = capfd.readouterr().err
    assert len(guard_lines(err)) == 2 and err.count(HEALED) == 2 and STICKY not in err
    assert m.range_stats()["trips"] == 2 and m.range_status() == (0, False) and "recalibrations:2" in m.describe()


def test_the_allowance_bounds_the_recalibrations(recipe, heat, capfd):
    m = calibrated_on_zeros_at_cap_13(recipe, heat, 1)
    capfd.readouterr()
    assert np.array_equal(m.predict_numpy(recipe["x7"]), recipe["s7"])
    assert HEALED in capfd.readouterr().err and m.range_stats()["recalibrations"] == 1
    y = m.predict_numpy(heat["hot"])
    err = capfd.readouterr().err
    st = m.range_stats()
    assert (st["trips"], st["recalibrations"], st["max_recalibrations"]) == (2, 1, 1) and "allowance" in st["fell_back"], st
    assert np.array_equal(y, heat["s_hot"]) and STICKY in err and "allowance" in err and HEALED not in err
    assert m.range_status()[1] and "precision=fp32-range-guard" in m.describe() and "recalibrations:1,fell_back" in m.describe()


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals(recipe, capfd):
    L = _lib.lib()
    p = Clair3_P(add_indel_length=False, predict=True, input_channels=18).to("cuda:0")
    with pytest.raises(_lib.C3Error, match="full-alignment.*LSTM"):
        p.range_policy("recalibrate")
    p.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, False, seed=7))
    with pytest.raises(_lib.C3Error, match="full-alignment.*LSTM"):
        p.range_policy("recalibrate")
    assert p.range_policy("sticky").range_policy() == ("sticky", 0)
    m = make_fa(recipe["sd"], "recalibrate")
    ticket = m.submit(recipe["x5"], slot=1)
    for policy in ("sticky", "recalibrate"):
        with pytest.raises(_lib.C3Error, match="in flight"):
            m.range_policy(policy)
    m.wait(ticket)
    assert m.range_policy() == ("recalibrate", 4)
    for bad in ("fp32", "", 1):
        with pytest.raises(_lib.C3Error, match="sticky"):
            m.range_policy(bad)
    with pytest.raises(_lib.C3Error, match="max_recalibrations"):
        m.range_policy("recalibrate", -1)
    assert L.c3_model_set_range_policy(m._handle, 7, 4) != 0 and "unknown policy" in _lib.last_error()
    assert L.c3_model_set_range_policy(m._handle, _lib.RANGE_RECALIBRATE, -1) != 0 and "max_recalibrations" in _lib.last_error()
    # a loaded handle that kept no tensors: the C ABI refuses, the Python layer loads again from the state dict it holds
    plain = make_fa(recipe["sd"])
    assert L.c3_model_set_range_policy(plain._handle, _lib.RANGE_RECALIBRATE, 4) != 0 and "before c3_model_load" in _lib.last_error()
    assert L.c3_model_set_range_policy(plain._handle, _lib.RANGE_STICKY, 0) == 0
    plain.range_policy("recalibrate", 2)
    assert plain.range_policy() == ("recalibrate", 2)
    capfd.readouterr()
    assert np.array_equal(plain.predict_numpy(recipe["x7"]), recipe["s7"]) and HEALED in capfd.readouterr().err
    # back to sticky drops the copy: from then on the C ABI refuses again
    plain.range_policy("sticky")
    assert "range_guard=" not in plain.describe()
    assert L.c3_model_set_range_policy(plain._handle, _lib.RANGE_RECALIBRATE, 4) != 0 and "before c3_model_load" in _lib.last_error()


def test_the_environment_sets_the_policy_where_the_handle_is_created(recipe, capfd, monkeypatch):
    monkeypatch.setenv("C3HIP_RANGE_GUARD", "recalibrate:3")
    m = make_fa(recipe["sd"])
    assert m.range_policy() == ("recalibrate", 3)
    capfd.readouterr()
    assert np.array_equal(m.predict_numpy(recipe["x7"]), recipe["s7"]) and HEALED in capfd.readouterr().err
    p = Clair3_P(add_indel_length=False, predict=True, input_channels=18).to("cuda:0")
    assert p.range_policy() == ("sticky", 0) and "range_guard=" not in p.describe(), "a pileup handle ignores it"
    monkeypatch.setenv("C3HIP_RANGE_GUARD", "recalibrate:many")
    with pytest.raises(_lib.C3Error, match="C3HIP_RANGE_GUARD=recalibrate:many"):
        Clair3_F(add_indel_length=True, predict=True, input_channels=8).to("cuda:0")


def test_the_policy_and_what_was_learned_travel_with_the_object(recipe, capfd):
    m, _, _ = healed_handle(recipe, capfd)
    k = m.calibration()["k"]
    m._create(m._device)  # what .to(another device) does
    assert m.range_policy() == ("recalibrate", 4) and np.array_equal(m.calibration()["k"], k)
    text = m.describe()
    assert "calibration=cap:10,windows:7,lowered:" in text and "range_guard=recalibrate,recalibrations:0" in text
    capfd.readouterr()
    util.assert_rows_match(m.predict_numpy(recipe["x7"]), recipe["y7"], tol=util.PROB_TOL, what="the handle created anew")
    assert not guard_lines(capfd.readouterr().err) and m.range_stats()["trips"] == 0


# ------------------------------------------------------------------------------------------------ 8: bystanders
def test_an_ordinary_checkpoint_does_not_notice_the_policy():
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7)
    x = syn.make_fa_windows(8, seed=8)
    a, b = make_fa(sd), make_fa(sd, "recalibrate")
    assert np.array_equal(a.predict_numpy(x), b.predict_numpy(x))
    ta, tb = a.wait(a.submit(x, slot=2)), b.wait(b.submit(x, slot=2))
    assert np.array_equal(ta, tb)
    st = b.range_stats()
    assert all(st[k] == 0 for k in ("trips", "recalibrations", "reruns", "census_windows", "channels_lowered", "cap_log2")) and st["fell_back"] == "", st
    assert b.describe() == a.describe() + " range_guard=recalibrate,recalibrations:0" and b.range_status() == (0, False)
    assert b.calibration()["lowering"] is None


def test_verify_mode_beside_the_policy(recipe, capfd):
    m = make_fa(recipe["sd"], "recalibrate")
    m.verify(every=1)
    ticket = m.submit(recipe["x7"], slot=0)
    before = m.verify_stats()
    assert before["batches_submitted"] == 1
    y = m.wait(ticket)
    assert np.array_equal(y, recipe["s7"]) and HEALED in capfd.readouterr().err
    st = m.verify_stats()  # a repack is no load: the totals from before the trip are still there; the guard kept priority
    assert (st["batches_submitted"], st["batches_skipped"], st["batches_checked"], st["every"]) == (1, 1, 0, 1), st
    for _ in range(2):  # the calibrated product rows against the fp32 forms on the same packed weights
        m.predict_numpy(recipe["x7"])
    st = m.verify_stats()
    print(f"verify mode on the healed handle: {st}")
    assert (st["batches_submitted"], st["batches_skipped"], st["batches_checked"], st["windows_checked"]) == (3, 1, 2, 14), st
    assert st["rows_over_tol"] == 0 and sum(st["label_diffs"]) == 0
    assert "precision=fp16x3" in m.describe() and m.range_stats()["trips"] == 1


# ------------------------------------------------------------------------------------------------ 9: the worker command
def test_the_worker_command_heals_and_prints_the_same_calls(recipe, tmp_path):
    import torch
    ref = refloop.reference_root()
    if ref is None:
        pytest.skip("no reference modules: run tools/stage_reference.sh in the build container (oracle/_ref travels with the snapshot)")
    d = str(tmp_path)
    lst = refloop.write_job(d, syn.FULL_ALIGNMENT, [200, 100], channels=8)
    ck = os.path.join(d, "recipe")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in recipe["sd"].items()}, ck + ".pt")
    outs = {}
    for name, env in (("healed", {"C3HIP_RANGE_GUARD": "recalibrate"}), ("fp32", {"C3HIP_FP32": "1"})):
        vcf = os.path.join(d, name + ".vcf")
        rc, out = refloop.run_worker(ref, lst, ck, vcf, False, True, hip=True, extra_env=env)
        assert rc == 0, out[-3000:]
        assert "Total processed positions : 300" in out, out[-3000:]
        outs[name] = (vcf, out)
    t = refloop.compare_vcfs(outs["healed"][0], outs["fp32"][0])
    print({k: v for k, v in t.items() if k != "call_differs"})
    assert t["records_a"] == t["records_b"] > 0 and not t["only_a"] and not t["only_b"] and not t["call_differs"], t
    out = outs["healed"][1]
    line = [ln for ln in out.splitlines() if ln.startswith("[clair3_amd] range guard:")]
    print("\n".join(line))
    assert len(line) == 1 and "precision=fp16x3" in line[0] and "fell_back=no" in line[0], out[-3000:]
    assert HEALED in out and STICKY not in out
    assert "[clair3_amd] range guard:" not in outs["fp32"][1]
