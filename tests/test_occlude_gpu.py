"""Occlusion mode on the device (needs an MI355X): c3_occlude, c3_occlude_rows, c3_occlude_reduce, both networks.

Yardsticks: a second, plain handle that is handed the variants built in numpy (synthetic.occlude_variants -> predict_numpy) and the windows
themselves (predict_rows / predict_numpy), and the numpy rule synthetic.occlude_records applied to the rows the same call returned -- never
the mode measured against itself.  Every comparison is bitwise: a window's row does not depend on the batch it travels in (DESIGN.md 2;
test_projection_kernels_are_bit_identical, test_lstm_tile_shapes_are_bit_identical and test_stride2_convolution_forms_are_bit_identical
hold it for the form switches), and the record holds only counts, comparisons and single float32 subtractions.  Full-alignment windows are
those of tests/test_jackknife_gpu.py: counts forced to 0, 1, 2, 17 (an interior all-zero row) and the full depth, and a natural one."""
import os
import re

import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import util
from tests.test_calibration import recipe_state_dict
from tests.test_jackknife import random_rows, same, same_drops
from tests.test_jackknife_gpu import CASES, forced, make_fa
from tests.test_occlude import corner_rows, same_records

pytestmark = pytest.mark.gpu

F32 = np.float32
P = syn.NO_OF_POSITIONS
_made = {}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("C3HIP_OCCLUDE_CHUNK", "C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_PACK_ROWS", "C3HIP_REFINE", "C3HIP_VERIFY", "C3HIP_EXACT", "C3HIP_RANGE_GUARD"):
        monkeypatch.delenv(k, raising=False)


def microbatches():
    """(full alignment, pileup) dense windows per micro-batch, read from c3_model.h max_microbatch"""
    src = open(os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_model.h")).read()
    m = re.search(r"max_microbatch\(const c3_model \*m\) \{ return m->kind == C3_KIND_PILEUP \? (\d+) : (\d+); \}", src)
    return int(m.group(2)), int(m.group(1))


def make_p(sd, indel=True, columns=False):
    m = Clair3_P(add_indel_length=indel, predict=True).to("cuda:0")
    m.load_state_dict(sd)
    return m.decode_columns(columns)


# ---- the full-alignment cases: weights, windows as rows, handles and calls, made once and left unchanged ----
def fa_case(name):
    if ("fa", name) not in _made:
        ch, depth, indel, seed = CASES[name]
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, indel, seed=seed)
        x = syn.make_fa_windows(6, seed=seed + 100, channels=ch, depth=depth)
        natural = int((x[5] != 0).any(axis=(1, 2)).sum())
        rows, counts = forced(x, [0, 1, 2, 17, depth, natural])
        _made["fa", name] = dict(ch=ch, depth=depth, indel=indel, sd=sd, rows=rows, counts=counts, nout=90 if indel else 24, handles={}, calls={})
    return _made["fa", name]


def fa_handles(c, columns):
    """(the handle under test, a plain handle that never runs the mode), per case and row width"""
    if columns not in c["handles"]:
        c["handles"][columns] = tuple(make_fa(c["sd"], c["ch"], c["depth"], c["indel"], columns) for _ in range(2))
    return c["handles"][columns]


def fa_call(c, columns, band):
    if (columns, band) not in c["calls"]:
        c["calls"][columns, band] = fa_handles(c, columns)[0].occlude_rows(c["rows"], c["counts"], band=band, drops=True, variant_rows=True)
    return c["calls"][columns, band]


FA_PARAMS = [(n, col, band) for n in CASES for col in (False, True) for band in (1, 5)]


# ---- the pileup cases ----
def p_case(dtype, indel):
    key = ("p", np.dtype(dtype).name, indel)
    if key not in _made:
        sd = syn.make_state_dict(syn.PILEUP, 18, indel, seed=41 + indel)
        x = np.concatenate([np.zeros((1, P, 18), dtype), syn.make_pileup_windows(1, seed=51, recipe="uniform", dtype=dtype),
                            syn.make_pileup_windows(3, seed=52, dtype=dtype)])
        if np.dtype(dtype) == np.int32:
            deep = syn.make_pileup_windows(1, seed=53, dtype=np.int32, depth=400)
            assert np.abs(deep).max() > 127, "counts that leave int8"
            x = np.concatenate([x, deep])
        x[2, :, 7] = 0  # a channel that is zero throughout a window
        columns = indel  # (rows with the decoder columns on the model with indel heads, without on the other)
        _made[key] = dict(sd=sd, x=np.ascontiguousarray(x), indel=indel, nout=90 if indel else 24, columns=columns,
                          handles=tuple(make_p(sd, indel, columns) for _ in range(2)), calls={})
    return _made[key]


def p_call(c, band):
    if band not in c["calls"]:
        c["calls"][band] = c["handles"][0].occlude(c["x"], band=band, drops=True, variant_rows=True)
    return c["calls"][band]


P_PARAMS = [(dt, indel, band) for dt in (np.int8, np.int32) for indel in (False, True) for band in (1, 5, P)]


def check_records(r, nout, reducer):
    """3: records and drops are the numpy rule's on the returned rows; the reduction alone gives the same"""
    rec, drops = syn.occlude_records(r["base_rows"], r["variant_rows"], r["channels"], r["bands"], nout)
    assert same_records(r["rows"], rec), {k: (r["rows"][k].tolist(), rec[k].tolist()) for k in rec.dtype.names if not same(r["rows"][k], rec[k])}
    assert same(r["drops"], drops) and not rec["nonfinite"].any() and (rec["variants"] == r["channels"] + r["bands"]).all()
    alone = reducer.occlude_reduce(r["base_rows"], r["variant_rows"], r["channels"], r["bands"], drops=True)
    assert same_records(alone["rows"], rec) and same(alone["drops"], drops)
    return rec


# ------------------------------------------------------------------------------------------------ 1: full-alignment rows
@pytest.mark.parametrize("name,columns,band", FA_PARAMS)
def test_full_alignment_rows_are_those_of_a_plain_handle(name, columns, band):
    c = fa_case(name)
    m, plain = fa_handles(c, columns)
    r = fa_call(c, columns, band)
    B, K = len(c["counts"]), c["ch"] + -(-P // band)
    assert (r["channels"], r["bands"], r["band"]) == (c["ch"], -(-P // band), band)
    assert r["variant_rows"].shape == (B * K, m.row_size) and r["drops"].shape == (B, K, 4) and r["rows"].dtype == syn.OCCLUDE_DTYPE
    assert same(r["counts"], c["counts"]) and not r["on_fp32"] and r["passes"] == 1
    x = syn.pad_fa_rows(c["rows"], c["counts"], depth=c["depth"])
    want_v = plain.predict_numpy(syn.occlude_variants(x, "both", band))
    assert same(r["variant_rows"], want_v), "the variants the device built are the numpy rule's, their rows a plain handle's"
    assert same(r["base_rows"], plain.predict_rows(c["rows"], c["counts"]))
    assert not same(want_v[4 * K], want_v[4 * K + 1]), "the variants differ from each other"
    assert all(same(want_v[k], r["base_rows"][0]) for k in range(K)), "a window without reads: every variant is the zero window"
    # dense windows: the run is found on the host, its first row is the run's own; explicit firsts at the centred places
    d = m.occlude(x, band=band, drops=True, variant_rows=True)
    firsts = ((c["depth"] - c["counts"]) // 2).astype(np.int32)
    e = m.occlude_rows(c["rows"], c["counts"], firsts, band=band, drops=True, variant_rows=True)
    for got in (d, e):
        assert same(got["counts"], c["counts"]) and same_records(got["rows"], r["rows"]) and same(got["base_rows"], r["base_rows"])
        assert same(got["variant_rows"], r["variant_rows"]) and same(got["drops"], r["drops"])
    # runs that do not sit in the centre: at the top and at the bottom of the window
    firsts = np.where(np.arange(B) % 2, c["depth"] - c["counts"], 0).astype(np.int32)
    e = m.occlude_rows(c["rows"], c["counts"], firsts, band=band, variant_rows=True)
    xf = syn.pad_fa_rows(c["rows"], c["counts"], firsts, depth=c["depth"])
    assert same(e["variant_rows"], plain.predict_numpy(syn.occlude_variants(xf, "both", band)))
    assert same(e["base_rows"], plain.predict_rows(c["rows"], c["counts"], firsts)) and "drops" not in e
    if band == 5:  # one group alone, and band = P: the band variant is the zero window
        only = m.occlude_rows(c["rows"], c["counts"], what="bands", band=P, variant_rows=True)
        zero = plain.predict_numpy(np.zeros((1,) + x.shape[1:], np.int8))[0]
        assert (only["channels"], only["bands"]) == (0, 1) and all(same(v, zero) for v in only["variant_rows"])
        assert (only["rows"]["lean"][:, 0] == -1).all() and not only["rows"]["flips"][:, 0].any()
        chans = m.occlude_rows(c["rows"], c["counts"], what="channels", band=7, variant_rows=True)
        assert (chans["channels"], chans["bands"]) == (c["ch"], 0)
        assert same(chans["variant_rows"], r["variant_rows"].reshape(B, K, -1)[:, :c["ch"]].reshape(B * c["ch"], -1))


# ------------------------------------------------------------------------------------------------ 2: pileup rows
@pytest.mark.parametrize("dtype,indel,band", P_PARAMS)
def test_pileup_rows_are_those_of_a_plain_handle(dtype, indel, band):
    c = p_case(dtype, indel)
    m, plain = c["handles"]
    r = p_call(c, band)
    x = c["x"]
    B, K = len(x), 18 + -(-P // band)
    assert (r["channels"], r["bands"], r["band"]) == (18, -(-P // band), band) and "counts" not in r
    assert r["variant_rows"].shape == (B * K, m.row_size) and r["drops"].shape == (B, K, 4) and not r["on_fp32"] and r["passes"] == 1
    variants = syn.occlude_variants(x, "both", band)
    assert variants.dtype == x.dtype
    want_v = plain.predict_numpy(variants)
    assert same(r["variant_rows"], want_v), "the variants the device built are the numpy rule's, their rows a plain handle's"
    assert same(r["base_rows"], plain.predict_numpy(x))
    v = r["variant_rows"].reshape(B, K, -1)
    assert same(v[2, 7], r["base_rows"][2]), "a channel that is zero throughout the window: the variant's row is the base row bit for bit"
    assert all(same(v[0, k], r["base_rows"][0]) for k in range(K)), "the all-zero window"
    assert not same(v[1, 0], v[1, 1]) and not same(v[3, 18], r["base_rows"][3])
    if band == P:
        assert all(same(v[b, 18], r["base_rows"][0]) for b in range(B)), "band = P: the band variant is the zero window"


# ------------------------------------------------------------------------------------------------ 3: records and drops
@pytest.mark.parametrize("name,columns,band", FA_PARAMS)
def test_full_alignment_records_equal_the_numpy_rule_on_the_same_rows(name, columns, band):
    c = fa_case(name)
    rec = check_records(fa_call(c, columns, band), c["nout"], fa_handles(c, columns)[1])
    assert rec["max_delta"][0] == 0 and (rec["lean"][0, :, :len(syn.head_slices(c["nout"]))] == 0).all(), "no reads: every drop is +0, the first member leans"
    assert rec["max_delta"][1:].min() > 0, "setting a channel or a column of a window that holds a read to zero moves the row"
    assert bool(rec["decision_flips"].any()) <= columns


@pytest.mark.parametrize("dtype,indel,band", P_PARAMS)
def test_pileup_records_equal_the_numpy_rule_on_the_same_rows(dtype, indel, band):
    c = p_case(dtype, indel)
    rec = check_records(p_call(c, band), c["nout"], c["handles"][1])
    assert rec["max_delta"][0] == 0 and rec["max_delta"][1:].min() > 0


@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
@pytest.mark.parametrize("indel", [False, True])
def test_reduce_on_hand_made_rows(kind, indel):
    nout = 90 if indel else 24
    if kind == syn.PILEUP:
        m = Clair3_P(add_indel_length=indel, predict=True).to("cuda:0")  # (the reduction needs no weights)
    else:
        m = make_fa(syn.make_state_dict(kind, 8, indel, seed=3), indel=indel)
    for columns in (False, True):
        for channels, bands in ((3, 2), (0, 4), (4, 0)):
            names, base, var = corner_rows(nout, columns, channels, bands)
            got = m.occlude_reduce(base, var, channels, bands, drops=True)
            rec, drops = syn.occlude_records(base, var, channels, bands, nout)
            bad = [names[i] for i in range(len(names)) if got["rows"][i].tobytes() != rec[i].tobytes()]
            assert same_records(got["rows"], rec), (columns, channels, bands, bad)
            assert same_drops(got["drops"], drops) and np.isnan(drops).any(), columns
            assert got["rows"]["flips"].sum() > 0 and got["rows"]["nonfinite"].sum() > 0
            assert "drops" not in m.occlude_reduce(base, var, channels, bands)
        # more variants than lanes (the stride loop), and the shipped K: 70 + 3, 18 + 33, 8 + 33
        rng = np.random.default_rng(nout + columns)
        for channels, bands in ((70, 3), (18, 33), (8, 33), (0, 0)):
            base, var = random_rows(5, nout, columns, rng), random_rows(5 * (channels + bands), nout, columns, rng)
            got = m.occlude_reduce(base, var, channels, bands, drops=True)
            rec, drops = syn.occlude_records(base, var, channels, bands, nout)
            assert same_records(got["rows"], rec) and same(got["drops"], drops), (columns, channels, bands)
    empty = m.occlude_reduce(np.zeros((0, nout), F32), np.zeros((0, nout), F32), 8, 33, drops=True)
    assert len(empty["rows"]) == 0 and empty["drops"].shape == (0, 41, 4)
    with pytest.raises(_lib.C3Error, match="rows of"):
        m.occlude_reduce(np.zeros((1, nout + 1), F32), np.zeros((2, nout + 1), F32), 1, 1)
    with pytest.raises(_lib.C3Error, match="group sizes"):
        m.occlude_reduce(np.zeros((1, nout), F32), np.zeros((0, nout), F32), -1, 1)


# ------------------------------------------------------------------------------------------------ 4: the cuts
def test_full_alignment_passes_and_micro_batches_do_not_show(monkeypatch):
    """52 windows at band 1 are 52 + 52 * 41 = 2184 dense windows: as one pass a micro-batch of 2048 ends inside a window's variants"""
    micro, K = microbatches()[0], 8 + P
    n = -(-micro // (K + 1)) + 3
    assert n * (K + 1) > micro and (micro - n) % K != 0, "the boundary falls inside a window's variants"
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=31)
    m = make_fa(sd, columns=True)
    x = syn.make_fa_windows(n, seed=5, recipe="uniform")
    rows, counts = x.reshape(n * 89, P, 8), np.full(n, 89, np.int32)
    results = {}
    for chunk, passes in (("0", 1), ("5", -(-n // 5)), ("1", n)):
        monkeypatch.setenv("C3HIP_OCCLUDE_CHUNK", chunk)
        r = results[chunk] = m.occlude_rows(rows, counts, drops=True, variant_rows=True)
        assert r["passes"] == passes and len(r["variant_rows"]) == n * K
    monkeypatch.delenv("C3HIP_OCCLUDE_CHUNK")
    assert m.occlude_rows(rows, counts)["passes"] == -(-n // 64), "the default pass: 64 full-alignment windows"
    for chunk in ("5", "1"):
        for key in ("base_rows", "variant_rows", "drops"):
            assert same(results[chunk][key], results["0"][key]), (chunk, key)
        assert same_records(results[chunk]["rows"], results["0"]["rows"]), chunk
    # the rows on either side of the micro-batch boundary (dense window `micro` = variant micro - n) against a plain batch
    w = (micro - n) // K
    v = syn.occlude_variants(x[w:w + 2])
    assert w * K < micro - n < (w + 1) * K and same(results["0"]["variant_rows"][w * K:(w + 2) * K], m.predict_numpy(v))
    rec, drops = syn.occlude_records(results["0"]["base_rows"], results["0"]["variant_rows"], 8, P, 90)
    assert same_records(results["0"]["rows"], rec) and same(results["0"]["drops"], drops)
    # staged once, whatever the cut: the occupied rows and 32 bytes of table per dense window
    assert results["0"]["bytes_staged"] == results["1"]["bytes_staged"] == n * 89 * P * 8 + n * (K + 1) * 32


def test_pileup_passes_and_micro_batches_do_not_show(monkeypatch):
    """320 windows at band 1 are 320 + 320 * 51 = 16640 dense windows: as one pass they cross the micro-batch of 16384"""
    micro, K = microbatches()[1], 18 + P
    n = -(-micro // (K + 1)) + 4
    assert n * (K + 1) > micro and (micro - n) % K != 0
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=43)
    m = make_p(sd, False)
    x = syn.make_pileup_windows(n, seed=6)
    monkeypatch.setenv("C3HIP_OCCLUDE_CHUNK", "0")
    one = m.occlude(x, drops=True, variant_rows=True)
    monkeypatch.setenv("C3HIP_OCCLUDE_CHUNK", "64")
    cut = m.occlude(x, drops=True, variant_rows=True)
    monkeypatch.delenv("C3HIP_OCCLUDE_CHUNK")
    assert one["passes"] == 1 and cut["passes"] == -(-n // 64) and m.occlude(x)["passes"] == -(-n // 256), "the default pass: 256 pileup windows"
    for key in ("base_rows", "variant_rows", "drops"):
        assert same(one[key], cut[key]), key
    assert same_records(one["rows"], cut["rows"])
    w = (micro - n) // K
    assert same(one["variant_rows"][w * K:(w + 2) * K], m.predict_numpy(syn.occlude_variants(x[w:w + 2])))
    assert same(one["base_rows"], m.predict_numpy(x))
    rec, drops = syn.occlude_records(one["base_rows"], one["variant_rows"], 18, P, 24)
    assert same_records(one["rows"], rec) and same(one["drops"], drops)
    assert one["bytes_staged"] == x.nbytes + n * (K + 1) * 32


# ------------------------------------------------------------------------------------------------ 5: the handle is left as it was
def state(m):
    return m.describe(), m.verify_stats(), m.refine_stats(), m.range_status(), m.layer_precision()


@pytest.mark.parametrize("kind", [syn.FULL_ALIGNMENT, syn.PILEUP])
def test_the_handle_is_left_as_it_was(kind):
    if kind == syn.FULL_ALIGNMENT:
        c = fa_case("c8_d89_indel")
        sd, rows, counts = c["sd"], c["rows"], c["counts"]
        x = syn.make_fa_windows(7, seed=9)
        used, fresh = make_fa(sd), make_fa(sd)
        for m in (used, fresh):
            m.predict_rows(rows, counts)  # (rows_windows= of the last call)
        run = lambda m: m.occlude_rows(rows, counts, band=5, drops=True, variant_rows=True)  # noqa: E731
    else:
        c = p_case(np.int8, True)
        sd, x = c["sd"], syn.make_pileup_windows(7, seed=9)
        used, fresh = make_p(sd), make_p(sd)
        for m in (used, fresh):
            m.predict_numpy(c["x"])
        run = lambda m: m.occlude(c["x"], band=5, drops=True, variant_rows=True)  # noqa: E731
    before = state(used)
    assert kind == syn.PILEUP or "rows_windows=6" in before[0]
    r = run(used)
    assert state(used) == before == state(fresh)
    assert same(used.predict_numpy(x), fresh.predict_numpy(x)) and state(used) == state(fresh)
    tickets = [[m.submit(x[k:k + 3], slot=k) for k in range(3)] for m in (used, fresh)]
    # refused while a submit is pending on any slot, and nothing of the pending batches is disturbed
    with pytest.raises(_lib.C3Error, match="a prediction is in flight: call c3_predict_wait first"):
        run(used)
    with pytest.raises(_lib.C3Error, match="in flight"):
        used.occlude(x)
    got = [[m.wait(t) for t in ts] for m, ts in zip((used, fresh), tickets)]
    assert all(same(a, b) for a, b in zip(*got)) and all(same(got[0][k], fresh.predict_numpy(x[k:k + 3])) for k in range(3))
    after_wait = state(used)
    again = run(used)  # works after the wait, gives what it gave, and again leaves the handle as it was
    assert all(same(again[k], r[k]) for k in ("base_rows", "variant_rows", "drops")) and same_records(again["rows"], r["rows"])
    assert state(used) == after_wait


# ------------------------------------------------------------------------------------------------ 6: the forms
def test_full_alignment_runs_on_the_forms_the_handle_is_on(monkeypatch):
    c = fa_case("c8_d89_indel")
    sd, rows, counts = c["sd"], c["rows"], c["counts"]
    variants = syn.occlude_variants(syn.pad_fa_rows(rows, counts), "both", 5)
    monkeypatch.setenv("C3HIP_FP32", "1")
    f32 = make_fa(sd)
    monkeypatch.delenv("C3HIP_FP32")
    plan = make_fa(sd)
    plan.layer_precision("conv3,res2a")
    product = fa_call(c, False, 5)
    for m, name in ((f32, "fp32-forced"), (plan, "fp32_layers=conv3,res2a")):
        before = m.describe()
        r = m.occlude_rows(rows, counts, band=5, variant_rows=True)
        assert m.describe() == before and name in before and not r["on_fp32"]
        assert same(r["base_rows"], m.predict_rows(rows, counts)) and same(r["variant_rows"], m.predict_numpy(variants))
        assert not same(r["variant_rows"], product["variant_rows"]), "other forms, other bits"
        assert same_records(r["rows"], syn.occlude_records(r["base_rows"], r["variant_rows"], 8, 7, 90)[0])


def test_pileup_runs_on_the_forms_the_handle_is_on(monkeypatch):
    for dtype in (np.int8, np.int32):
        c = p_case(dtype, True)
        sd, x = c["sd"], c["x"]
        variants = syn.occlude_variants(x, "both", 5)
        monkeypatch.setenv("C3HIP_FP32", "1")
        f32 = make_p(sd, True, c["columns"])
        monkeypatch.delenv("C3HIP_FP32")
        plan = make_p(sd, True, c["columns"])
        plan.layer_precision("lstm2")
        product = p_call(c, 5)
        for m, name in ((f32, "fp32-forced"), (plan, "fp32_layers=lstm2")):
            before = m.describe()
            r = m.occlude(x, band=5, variant_rows=True)
            assert m.describe() == before and name in before and not r["on_fp32"]
            assert same(r["base_rows"], m.predict_numpy(x)) and same(r["variant_rows"], m.predict_numpy(variants))
            assert not same(r["variant_rows"], product["variant_rows"]), "other forms, other bits"
            assert same_records(r["rows"], syn.occlude_records(r["base_rows"], r["variant_rows"], 18, 7, 90)[0])


# ------------------------------------------------------------------------------------------------ 7: the range guard
def test_range_guard_runs_the_pass_again_on_fp32_for_this_call_alone(monkeypatch, capfd):
    sd = recipe_state_dict()
    x = syn.make_fa_windows(3, seed=62)
    rows, _, counts = syn.pack_fa_rows(x)
    m, never = make_fa(sd), make_fa(sd)
    monkeypatch.setenv("C3HIP_FP32", "1")
    f32 = make_fa(sd)
    monkeypatch.delenv("C3HIP_FP32")
    before = m.describe()
    r = m.occlude_rows(rows, counts, band=5, drops=True, variant_rows=True)
    assert r["on_fp32"], "the checkpoint's activations leave the range of the fp16x3 kernels"
    assert same(r["base_rows"], f32.predict_rows(rows, counts)) and same(r["variant_rows"], f32.predict_numpy(syn.occlude_variants(x, "both", 5)))
    rec, drops = syn.occlude_records(r["base_rows"], r["variant_rows"], 8, 7, 90)
    assert same_records(r["rows"], rec) and same(r["drops"], drops) and not rec["nonfinite"].any()
    assert m.range_status() == (0, False) and m.describe() == before and "precision=fp16x3" in before
    assert "continues on fp32" not in capfd.readouterr().err, "the handle stays on its forms and says nothing"
    # the handle's next ordinary batch trips its own guard exactly as on a handle that never ran the call
    y, y_never = m.predict_numpy(x), never.predict_numpy(x)
    assert same(y, y_never) and same(y, f32.predict_numpy(x))
    assert m.range_status() == never.range_status() and m.range_status()[1] and m.describe() == never.describe()
    assert capfd.readouterr().err.count("continues on fp32") == 2
    assert not m.occlude_rows(rows, counts, band=5)["on_fp32"], "a handle that is on the fp32 forms has no guard to meet"


# ------------------------------------------------------------------------------------------------ 8: refusals that need the device
def test_refusals_and_the_empty_call():
    c = fa_case("c8_d89_indel")
    sd, rows, counts = c["sd"], c["rows"], c["counts"]
    L = _lib.lib()
    rec = np.zeros(len(counts), syn.OCCLUDE_DTYPE)
    pc = p_case(np.int8, True)
    p = pc["handles"][0]
    assert L.c3_occlude_rows(p._handle, rows.ctypes.data, None, counts.ctypes.data, len(counts), 3, 1, None, rec.ctypes.data, None, None, None) != 0
    assert "full-alignment input" in _lib.last_error()
    with pytest.raises(_lib.C3Error, match="unsupported window dtype"):
        p.occlude(pc["x"].astype(np.float32))
    assert L.c3_occlude(p._handle, pc["x"].ctypes.data, _lib.DTYPE_F32, 1, 3, 1, None, rec.ctypes.data, None, None, None) != 0 and "int8 or int32" in _lib.last_error()
    for empty, x in ((Clair3_F(add_indel_length=True, predict=True).to("cuda:0"), np.zeros((1, 89, P, 8), np.int8)),
                     (Clair3_P(add_indel_length=True, predict=True).to("cuda:0"), pc["x"])):
        with pytest.raises(_lib.C3Error, match="no weights"):
            empty.occlude(x)
    m = make_fa(sd)
    before = m.describe()
    assert L.c3_occlude(m._handle, rows.ctypes.data, _lib.DTYPE_I32, 1, 3, 1, None, rec.ctypes.data, None, None, None) != 0 and "must be int8" in _lib.last_error()
    bad = counts.copy()
    bad[2] = -1
    with pytest.raises(_lib.C3Error, match="window 2: negative row_count"):
        m.occlude_rows(rows, bad)
    with pytest.raises(_lib.C3Error, match="counts add up"):
        m.occlude_rows(rows[:-1], counts)
    firsts = np.zeros(len(counts), np.int32)
    firsts[3] = 89 - 16
    with pytest.raises(_lib.C3Error, match=r"window 3: rows \[73, 90\) reach beyond the depth"):
        m.occlude_rows(rows, counts, firsts)
    firsts[3] = -1
    with pytest.raises(_lib.C3Error, match="window 3: negative row_first"):
        m.occlude_rows(rows, counts, firsts)
    for h, args in ((m, (rows.ctypes.data, _lib.DTYPE_I8, 1)), (p, (pc["x"].ctypes.data, _lib.DTYPE_I8, 1))):
        for what in (0, 4):
            assert L.c3_occlude(h._handle, *args, what, 1, None, rec.ctypes.data, None, None, None) != 0 and "unknown `what`" in _lib.last_error()
        for band in (0, P + 1):
            assert L.c3_occlude(h._handle, *args, 3, band, None, rec.ctypes.data, None, None, None) != 0 and "outside 1 .. 33" in _lib.last_error()
        assert L.c3_occlude(h._handle, *args, 3, 1, None, None, None, None, None) != 0 and "null buffer" in _lib.last_error()
    with pytest.raises(_lib.C3Error, match="window shape"):
        m.occlude(np.zeros((1, 89, P, 9), np.int8))
    # the empty call launches nothing
    none = m.occlude_rows(rows[:0], counts[:0], drops=True, variant_rows=True)
    assert len(none["rows"]) == 0 and none["passes"] == 0 and none["drops"].shape == (0, 41, 4) and none["variant_rows"].shape == (0, 90)
    none = p.occlude(pc["x"][:0], band=5, drops=True, variant_rows=True)
    assert len(none["rows"]) == 0 and none["passes"] == 0 and none["drops"].shape == (0, 25, 4) and none["variant_rows"].shape == (0, p.row_size)
    assert m.describe() == before
    # a handle that answers from the exact form
    m.exact(True)
    m.answer("exact")
    with pytest.raises(_lib.C3Error, match="answers from the exact form"):
        m.occlude_rows(rows, counts)
    m.answer("product")
    assert same_records(m.occlude_rows(rows, counts, band=5)["rows"], fa_call(c, False, 5)["rows"])


# ------------------------------------------------------------------------------------------------ 9: the tool
@pytest.mark.parametrize("kind", [syn.FULL_ALIGNMENT, syn.PILEUP])
def test_the_tool_prints_the_report_of_the_same_windows(kind, tmp_path, capsys):
    import json
    import torch
    from clair3_amd import occlude
    if kind == syn.FULL_ALIGNMENT:
        c = fa_case("c8_d89_indel")
        x, handle, extra = syn.pad_fa_rows(c["rows"], c["counts"]), fa_handles(c, True)[0], []
    else:
        c = p_case(np.int32, True)
        x, handle, extra = c["x"], c["handles"][0], ["--pileup"]
        assert handle.row_size == 90 + syn.DECODE_COLS
    np.save(str(tmp_path / "x.npy"), x)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in c["sd"].items()}, str(tmp_path / "m.pt"))
    out = str(tmp_path / "lines.json")
    assert occlude.main(["--chkpnt_fn", str(tmp_path / "m.pt"), "--tensor_fn", str(tmp_path / "x.npy"), "--band", "5", "--head", "1", "--out", out] + extra) == 0
    printed = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    want = occlude.report(handle.occlude(x, band=5, drops=True, variant_rows=True), 90, 1)
    assert printed == json.loads(json.dumps(want)) == [json.loads(line) for line in open(out)]
    C = x.shape[-1]
    assert len(printed) == C + 7 + 1 and [line.get("channel") for line in printed[:C]] == list(range(C)) and printed[C]["columns"] == [0, 5]
    assert printed[-1]["windows"] == len(x) and printed[-1]["variants"] == len(x) * (C + 7) and printed[-1]["head"] == 1
