"""The exact form on the submit / wait ring (needs an MI355X): c3_model_set_answer, c3_model_set_verify_reference, C3_VERIFY_REPLACE.

Yardsticks: ``predict_exact`` of the same handle (the blocking entry, itself held to the fp64 oracle by tests/test_exact_gpu.py) and the C
oracle (oracle.oracle) -- never a path of this file measured against itself.  Bounds:
    float32 exact rows against predict_exact(windows).astype(float32)   bitwise (the rule is ONE rounding, round to nearest even)
    float32 exact rows against the oracle's rows                        ROW_BOUND + 2**-25 (tests/test_exact_gpu.py's bound and the second
                                                                        rounding: half a float32 ulp of a probability <= 1)
    verify mode's double maximum against numpy on the returned rows     bitwise (a maximum of correctly rounded differences)
The windows of depths, regions, candidates and rows are materialised on the host by synthetic.rescale_deep_windows,
synthetic.select_pileup_windows and synthetic.pad_fa_rows.
    a layer's max_abs_diff against numpy on tap_fetch and exact_fetch       bitwise the float32 rounding of the double maximum"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from clair3_amd import _lib, audit, decode, predict, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_BOUND = 2.0 ** -25 + 1e-9          # tests/test_exact_gpu.py
F32_BOUND = ROW_BOUND + 2.0 ** -25     # ... and the rounding of the exact row to float32
SENSITIVE_SEED, SENSITIVE_WINDOW = 925999917, 549
ENV = ("C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_AUTO_FP32", "C3HIP_EXACT", "C3HIP_EXACT_CHUNK", "C3HIP_VERIFY",
       "C3HIP_VERIFY_TOL", "C3HIP_VERIFY_LAYERS", "C3HIP_VERIFY_REF", "C3HIP_ANSWER", "C3HIP_RING_LANES", "C3HIP_PACK_ROWS", "C3HIP_CALIBRATION",
       "C3HIP_RANGE_GUARD")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def make(kind, ch, indel, sd, depth=None, exact=True):
    m = (Clair3_P if kind == syn.PILEUP else Clair3_F)(add_indel_length=indel, predict=True, input_channels=ch)
    if depth:
        m.set_geometry(depth, 33)
    m.to("cuda:0")
    m.load_state_dict(sd)
    return m.exact(True) if exact else m


def f32(y64):
    return y64.astype(np.float32)


def precision(m):
    return m.describe().split("precision=")[1].split()[0]


@pytest.fixture(scope="module")
def oracle_mod():
    from oracle import oracle
    return oracle


CASES = {  # name: kind, channels, depth, indel, windows, dtype, seeds
    "fa_c8_d89_b3": (syn.FULL_ALIGNMENT, 8, None, True, 3, np.int8, 61, 62),     # odd M in every layer
    "fa_c9_d55_b2": (syn.FULL_ALIGNMENT, 9, 55, True, 2, np.int8, 64, 65),       # unaligned 9-byte pixels
    "pileup_i32_indel_b5": (syn.PILEUP, 18, None, True, 5, np.int32, 61, 63),    # a part-filled tile, rows 90 wide
    "pileup_i8_b17": (syn.PILEUP, 18, None, False, 17, np.int8, 66, 67),         # one full 16-window tile plus one window
}
_cases = {}


def case(name, oracle_mod):
    """weights, windows and the oracle's rows of a case, made once and left unchanged"""
    if name not in _cases:
        kind, ch, depth, indel, n, dtype, s_sd, s_x = CASES[name]
        sd = syn.make_state_dict(kind, ch, indel, seed=s_sd, trained_like=name == "fa_c9_d55_b2")
        if kind == syn.PILEUP:
            x = syn.make_pileup_windows(n, seed=s_x, dtype=dtype)
            y_o = oracle_mod.pileup_forward(sd, x, indel)
        else:
            x = syn.make_fa_windows(n, seed=s_x, channels=ch, depth=depth or 89)
            y_o = oracle_mod.fa_forward(sd, x, indel)
        _cases[name] = dict(kind=kind, ch=ch, depth=depth, indel=indel, sd=sd, x=x, y_o=y_o)
    return _cases[name]


def check_oracle(y, y_o, what):
    err = float(np.abs(y.astype(np.float64) - y_o.astype(np.float64)).max())
    print(f"{what}: max |y - y_oracle| = {err:.3e} (bound {F32_BOUND:.3e})")
    assert err <= F32_BOUND, what


# ------------------------------------------------------------------------------------------------ 1: the answer form, every input kind
@pytest.mark.parametrize("name", list(CASES))
def test_answer_exact_sliced_windows(name, oracle_mod):
    c = case(name, oracle_mod)
    x = c["x"]
    plain = make(c["kind"], c["ch"], c["indel"], c["sd"], c["depth"], exact=False)
    y_product, d_product = plain.predict_numpy(x), plain.describe()
    m = make(c["kind"], c["ch"], c["indel"], c["sd"], c["depth"])
    want = f32(m.predict_exact(x))
    assert precision(m) == precision(plain)
    m.answer("exact")
    y = m.predict_numpy(x)
    assert y.dtype == np.float32 and np.array_equal(y, want), f"{name}: predict_numpy is the float32 rounding of the exact rows, bit for bit"
    check_oracle(y, c["y_o"], name)
    assert precision(m) == "exact" and m.describe().endswith(" exact=1")
    half = len(x) // 2
    t0, t1 = m.submit(x[:half + 1], slot=1), m.submit(x[half:], slot=3)
    assert np.array_equal(m.wait(t1), want[half:]) and np.array_equal(m.wait(t0), want[:half + 1]), f"{name}: two slots of the ring"
    # decoder columns are computed from those rows
    m.decode_columns(True)
    wide = m.predict_numpy(x)
    assert wide.shape == (len(x), m.output_size + m.DECODE_COLS) and np.array_equal(wide[:, :m.output_size], want)
    assert np.array_equal(wide, decode.decode_columns(m, want)), f"{name}: the decoder columns are c3_decode_columns of the float32 exact rows"
    m.decode_columns(False)
    # the range flag is neither raised nor read, and a reload that keeps the exact form keeps the answer form
    assert m.range_status()[0] == 0
    m.load_state_dict(c["sd"])
    assert precision(m) == "exact" and np.array_equal(m.predict_numpy(x), want), f"{name}: after a reload"
    # ... and set back, the handle is one that never had it set
    m.answer("product")
    assert np.array_equal(m.predict_numpy(x), y_product), f"{name}: product rows after answer('product')"
    assert m.describe() == d_product + " exact=1"


def test_answer_exact_pileup_depths_region_candidates(oracle_mod, monkeypatch):
    c = case("pileup_i32_indel_b5", oracle_mod)
    monkeypatch.setenv("C3HIP_EXACT_CHUNK", "4")  # 9 windows and more: every batch below crosses a chunk boundary
    m = make(syn.PILEUP, 18, True, c["sd"])
    # depths: two windows deeper than 1.5 x 144
    x = syn.make_pileup_windows(9, seed=901, dtype=np.int32)
    depths = np.array([100, 300, 0, 216, 217, 144, 1000, 150, 215], np.int32)
    xr = syn.rescale_deep_windows(x, depths)
    assert (xr != x).any(axis=(1, 2)).sum() >= 2
    want_d, want_x = f32(m.predict_exact(xr)), f32(m.predict_exact(x))
    # a region with starts; candidates with a head window, a tail window and a dropped candidate
    region, major = syn.make_pileup_region(400, n_chunks=2, seed=902, empty_runs=((120, 1),))
    starts = np.array([0, 7, 33, 34, 150, 199, 250, 300, 367], np.int32)
    a, b = syn.pileup_chunks(major)
    cand = np.r_[major[a[0]] + 3, major[a[0] + 30:a[0] + 34], major[110], major[b[0] - 2], major[a[1] + 40:a[1] + 44], major[-1] + 5].astype(np.int64)
    status, windows = syn.select_pileup_windows(region, major, cand, head_tail=True)
    assert (status == syn.CAND_HEAD).any() and (status == syn.CAND_TAIL).any() and (status == syn.CAND_EMPTY_COLUMN).any()
    assert (status == syn.CAND_NO_WINDOW).any() and 4 < len(windows) < len(cand)
    want_r = f32(m.predict_exact(np.stack([region[s:s + 33] for s in starts])))
    want_c = f32(m.predict_exact(windows))
    cdepths = np.where(np.arange(len(cand)) % 3 == 0, 400, 20).astype(np.int32)
    kept = np.isin(status, syn.CAND_KEPT)
    want_cd = f32(m.predict_exact(syn.rescale_deep_windows(windows, cdepths[kept])))
    m.answer("exact")
    assert np.array_equal(m.predict_numpy(x), want_x), "9 sliced windows in chunks of 4"
    assert np.array_equal(m.predict_numpy(x, depths=depths), want_d), "windows with depths: the rescaled windows through the exact form"
    assert np.array_equal(m.predict_region(region, starts), want_r), "a region with starts"
    assert np.array_equal(m.predict_region(region.astype(np.int64), starts, depths=depths),
                          f32(m.predict_exact(syn.rescale_deep_windows(np.stack([region[s:s + 33] for s in starts]), depths)))), "an int64 region with depths"
    rows, st = m.predict_candidates(region, major, cand, head_tail=True)
    assert np.array_equal(st, status) and np.array_equal(rows, want_c), "candidates: head, tail, dropped"
    rows, st = m.predict_candidates(region, major, cand, depths=cdepths, head_tail=True)
    assert np.array_equal(st, status) and np.array_equal(rows, want_cd), "candidates with depths"
    rows, st = m.predict_candidates(region, major, cand[-1:], head_tail=True)
    assert len(rows) == 0 and list(st) == [syn.CAND_NO_WINDOW], "a batch with nothing kept"
    with pytest.raises(_lib.C3Error, match="int8 region"):
        m.predict_region(region.astype(np.int8), starts)
    assert np.array_equal(m.predict_numpy(x), want_x), "... which leaves the handle usable"
    check_oracle(m.predict_numpy(c["x"]), c["y_o"], "pileup int32, chunks of 4")


def test_answer_exact_full_alignment_rows_and_parts(oracle_mod):
    c = case("fa_c8_d89_b3", oracle_mod)
    m = make(syn.FULL_ALIGNMENT, 8, True, c["sd"])
    x = syn.make_fa_windows(7, seed=903)
    x[2] = 0                                            # a window with zero reads
    x[5] = syn.make_fa_windows(1, seed=904, recipe="uniform")[0]  # ... and one with all 89 rows occupied
    x[5, 0, 0, 0], x[5, 88, 0, 0] = 1, 1
    rows, firsts, counts = syn.pack_fa_rows(x)
    assert counts[2] == 0 and counts[5] == 89 and np.array_equal(syn.pad_fa_rows(rows, counts, firsts), x)
    want = f32(m.predict_exact(x))
    m.answer("exact")
    assert np.array_equal(m.predict_rows(rows, counts, firsts), want), "occupied rows: the expanded windows through the exact form"
    got = m.predict_parts([x[:1], x[1:5], x[5:]])
    assert [len(g) for g in got] == [1, 4, 2] and np.array_equal(np.concatenate(got), want), "three parts of 1, 4 and 2 windows"
    mine = [(x[:1].copy(), np.full((1, 90), np.nan, np.float32)), (x[1:5].copy(), np.full((4, 90), np.nan, np.float32)),
            (x[5:].copy(), np.full((2, 90), np.nan, np.float32))]
    out = m.wait(m.submit_parts(mine, slot=2))
    assert np.array_equal(np.concatenate(out), want)
    check_oracle(m.predict_numpy(c["x"]), c["y_o"], "full alignment through the ring")


# ------------------------------------------------------------------------------------------------ 2: independent of travel
@pytest.mark.parametrize("name", ["pileup_i32_indel_b5", "fa_c8_d89_b3"])
def test_a_row_does_not_depend_on_batch_chunk_or_lane(name, oracle_mod, monkeypatch):
    c = case(name, oracle_mod)
    x9 = np.concatenate([c["x"]] * 3)[:9] if len(c["x"]) < 9 else c["x"][:9]
    x9 = np.ascontiguousarray(x9)
    x9[8] = x9[0]  # the same window as batch member 0 and 8
    m = make(c["kind"], c["ch"], c["indel"], c["sd"], c["depth"]).answer("exact")
    monkeypatch.setenv("C3HIP_EXACT_CHUNK", "4")
    cut = m.predict_numpy(x9)
    assert np.array_equal(cut[0], cut[8]), "member 0 (first pass) and member 8 (third pass, alone)"
    monkeypatch.setenv("C3HIP_EXACT_CHUNK", "1024")
    whole = m.predict_numpy(x9)
    assert np.array_equal(whole, cut), "chunks of 4 against one pass"
    # three small batches back to back: the lanes are in use, the one workspace is handed from pass to pass
    monkeypatch.setenv("C3HIP_EXACT_CHUNK", "4")
    t = [m.submit(x9[k:k + 5], slot=k) for k in range(3)]
    for k in (2, 0, 1):
        assert np.array_equal(m.wait(t[k]), whole[k:k + 5]), f"batch {k} of three in flight"
    assert np.array_equal(m.predict_numpy(x9[8:]), whole[:1]), "alone in a batch"


# ------------------------------------------------------------------------------------------------ 3: verify against exact, report policy
def sensitive_tile():
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=SENSITIVE_SEED, peaked=False, trained_like=True)
    x = syn.make_pileup_windows(920, seed=SENSITIVE_SEED, recipe="realistic")
    lo = SENSITIVE_WINDOW - SENSITIVE_WINDOW % 16
    return sd, np.ascontiguousarray(x[lo:lo + 16])


def host_compare(y, e64, tol, near_tie=1e-6):
    """the comparison of verify mode against the exact rows, in numpy: per-row maxima (double), rows over tol, label differences per head"""
    d = np.abs(y.astype(np.float64) - e64)
    per_row = d.max(axis=1)
    labels, bad = [], per_row > np.float64(np.float32(tol))
    for lo, hi in syn.head_slices(y.shape[1]):
        top2 = np.sort(e64[:, lo:hi], axis=1)[:, -2:]
        differs = (y[:, lo:hi].argmax(1) != e64[:, lo:hi].argmax(1)) & (top2[:, 1] - top2[:, 0] > np.float64(np.float32(near_tie)))
        labels.append(int(differs.sum()))
        bad = bad | differs
    return d, per_row, labels, bad


def tol_between(per_row):
    """halfway between two distinct per-row maxima, so that some rows but not all lie beyond it (as float32: what the ABI takes)"""
    u = np.unique(per_row)
    assert len(u) >= 2, "the batch has at least two distinct per-row maxima"
    k = len(u) // 2
    tol = float(np.float32((u[k - 1] + u[k]) / 2))
    assert u[k - 1] < tol < u[k], "float32 separates the two maxima"
    return tol


def verify_cases(oracle_mod):
    sd, xs = sensitive_tile()
    c = case("fa_c8_d89_b3", oracle_mod)
    return (("sensitive_tile", syn.PILEUP, 18, sd, xs, None), ("fa_c8_d89_b3", syn.FULL_ALIGNMENT, 8, c["sd"], c["x"], None))


@pytest.mark.parametrize("which", [0, 1])
def test_verify_against_exact_report(which, oracle_mod, monkeypatch):
    monkeypatch.setenv("C3HIP_FP32", "0")  # the product forms whatever the weights look like: the comparison is about them
    name, kind, ch, sd, x, depth = verify_cases(oracle_mod)[which]
    m = make(kind, ch, True, sd, depth)
    y0, e64 = m.predict_numpy(x), m.predict_exact(x)
    d, per_row, _, _ = host_compare(y0, e64, 1e-4)
    tol = tol_between(per_row)
    _, _, labels, _ = host_compare(y0, e64, tol)
    m.verify(every=1, tol=tol, reference="exact")
    assert m.describe().endswith(",ref:exact exact=1") and "policy:report" in m.describe()
    y = m.predict_numpy(x)
    assert np.array_equal(y, y0), f"{name}: the rows are those of a run without verify mode"
    st, ex = m.verify_stats(), m.verify_extra()
    print(f"{name}: max |y - exact| = {ex['max_abs_diff_f64']:.6e} (host {d.max():.6e}), rows over {tol:.3e}: {st['rows_over_tol']} of {len(x)}")
    assert ex["reference"] == "exact" and ex["max_abs_diff_f64"] == float(d.max()), "the double maximum, bit for bit"
    assert np.float32(st["max_abs_diff"]) == np.float32(d.max()), "... and its float32 rounding"
    heads = syn.head_slices(y.shape[1])
    assert [np.float32(v) for v in st["head_max_abs_diff"][:len(heads)]] == [np.float32(d[:, lo:hi].max()) for lo, hi in heads]
    assert st["batches_checked"] == 1 and st["windows_checked"] == len(x) and st["worst_row"] == int(per_row.argmax())
    assert st["rows_over_tol"] == int((per_row > np.float64(np.float32(tol))).sum()) and 0 < st["rows_over_tol"] < len(x)
    assert st["label_diffs"][:len(heads)] == labels
    assert ex["rows_replaced"] == 0 and precision(m) == "fp16x3"
    # back on the fp32 reference the totals start again and the text loses its last word
    m.verify(every=1, reference="fp32")
    assert ",ref:" not in m.describe() and m.verify_extra()["reference"] == "fp32"


# ------------------------------------------------------------------------------------------------ 4: replace
@pytest.mark.parametrize("which", [0, 1])
def test_replace_repairs_only_the_rows_that_are_wrong(which, oracle_mod, monkeypatch):
    import torch
    monkeypatch.setenv("C3HIP_FP32", "0")
    name, kind, ch, sd, x, depth = verify_cases(oracle_mod)[which]
    m = make(kind, ch, True, sd, depth)
    y0, e64 = m.predict_numpy(x), m.predict_exact(x)
    _, per_row, _, _ = host_compare(y0, e64, 1e-4)
    tol = tol_between(per_row)
    _, _, _, bad = host_compare(y0, e64, tol)
    assert bad.any() and not bad.all(), "some rows but not all are beyond tol"
    want = np.where(bad[:, None], f32(e64), y0)
    m.verify(every=2, tol=tol, reference="exact", replace=True)
    y = m.predict_numpy(x)
    print(f"{name}: tol {tol:.3e}: rows {np.flatnonzero(bad).tolist()} of {len(x)} replaced")
    assert np.array_equal(y[bad], f32(e64)[bad]), "exactly the host-predicted rows are the float32 exact rows"
    assert np.array_equal(y[~bad], y0[~bad]), "... and all others the product rows, bit for bit"
    ex, st = m.verify_extra(), m.verify_stats()
    assert ex["rows_replaced"] == int(bad.sum()) and ex["batches_with_replacements"] == 1 and st["policy"] == "replace" and st["escalations"] == 0
    assert precision(m) == "fp16x3" and "policy:replace" in m.describe()
    assert np.array_equal(m.predict_numpy(x), y0), "the next, unselected batch is an ordinary one"
    assert m.verify_extra()["rows_replaced"] == int(bad.sum())
    # decoder columns follow the rows as they are returned
    m.decode_columns(True)
    m.verify_reset()
    wide = m.predict_numpy(x)
    assert np.array_equal(wide, decode.decode_columns(m, want)), "decoder columns of repaired and untouched rows"
    m.decode_columns(False)
    # rows left on the device
    m.verify_reset()
    y_dev = torch.full((len(x), y0.shape[1]), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert m.wait(m.submit_dev(x, y_dev.data_ptr(), slot=1)) is None
    torch.cuda.synchronize()
    assert np.array_equal(y_dev.cpu().numpy(), want), "rows left on the device are repaired there"
    assert m.verify_extra()["rows_replaced"] == int(bad.sum())
    # parts: the repaired rows take the parts' way back
    m.verify_reset()
    got = m.predict_parts([x[:1], x[1:]])
    assert np.array_equal(np.concatenate(got), want)
    # once with the fp32 forms as the reference: replaced rows are those of a C3HIP_FP32=1 handle
    monkeypatch.setenv("C3HIP_FP32", "1")
    y32 = make(kind, ch, True, sd, depth, exact=False).predict_numpy(x)
    monkeypatch.setenv("C3HIP_FP32", "0")
    d32 = np.abs(y0 - y32).max(axis=1)  # (float32 arithmetic, as the fp32 comparison states it)
    if len(np.unique(d32)) >= 2:
        u = np.unique(d32)
        tol32 = float(np.float32((np.float64(u[len(u) // 2 - 1]) + np.float64(u[len(u) // 2])) / 2))
        bad32 = d32 > np.float32(tol32)
        for lo, hi in syn.head_slices(y0.shape[1]):
            top2 = np.sort(y32[:, lo:hi], axis=1)[:, -2:]
            bad32 |= (y0[:, lo:hi].argmax(1) != y32[:, lo:hi].argmax(1)) & (top2[:, 1] - top2[:, 0] > np.float32(1e-6))
        assert bad32.any() and not bad32.all()
        m.verify(every=1, tol=tol32, reference="fp32", replace=True)
        m.verify_reset()
        y = m.predict_numpy(x)
        assert np.array_equal(y[bad32], y32[bad32]) and np.array_equal(y[~bad32], y0[~bad32]), "fp32 reference: replaced rows are the fp32 handle's"
        assert m.verify_extra() == dict(reference="fp32", rows_replaced=int(bad32.sum()), batches_with_replacements=1, max_abs_diff_f64=0.0)


def test_escalate_against_exact_answers_with_the_exact_rows(monkeypatch, capfd):
    monkeypatch.setenv("C3HIP_FP32", "0")
    sd, x = sensitive_tile()
    m = make(syn.PILEUP, 18, True, sd)
    y0, e64 = m.predict_numpy(x), m.predict_exact(x)
    _, per_row, _, _ = host_compare(y0, e64, 1e-4)
    m.verify(every=1, tol=tol_between(per_row), escalate=True, reference="exact")
    assert np.array_equal(m.predict_numpy(x), f32(e64)), "the tripping batch is answered with the float32 exact rows"
    assert precision(m) == "fp32-verify" and m.verify_stats()["escalations"] == 1
    assert "differ from the exact form" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------ 5: layers against exact
@pytest.mark.parametrize("name", ["pileup_i32_indel_b5", "fa_c8_d89_b3"])
def test_layer_records_against_the_exact_layers(name, oracle_mod, monkeypatch):
    monkeypatch.setenv("C3HIP_FP32", "0")
    monkeypatch.setenv("C3HIP_EXACT_CHUNK", "2")  # the exact layers of a batch exist two windows at a time: 3 (2) passes per batch
    c = case(name, oracle_mod)
    x, B = c["x"], len(c["x"])
    m = make(c["kind"], c["ch"], True, c["sd"], c["depth"])
    y0 = m.predict_numpy(x)
    m.verify(every=1, layers=True, reference="exact")
    assert np.array_equal(m.predict_numpy(x), y0)
    assert m.describe().endswith(",layers:1,ref:exact exact=1")
    layers = m.verify_layers()
    if c["kind"] == syn.PILEUP:
        names = {"lstm1_out": 33 * 256, "gx2": 33 * 1280, "lstm2_out": 33 * 320, "l4_out": 128}
    else:
        hw, names = [(45, 17)] * 3 + [(23, 9)] * 3 + [(12, 5)] * 3, {}
        for i, ((h, w), ch) in enumerate(zip(hw, [64] * 3 + [128] * 3 + [256] * 3)):
            names[f"act{i}"] = h * w * ch
        names.update(spp=14 * 256, l4_out=256)
    assert [e["name"] for e in layers] == list(names)
    # the host's side: the product layers of a tapped run, the exact layers window by window (a pass of one: every window is a last pass)
    m.verify(every=0, reference="exact")
    compared = [e["name"] for e in layers if e["status"] == "compared"]
    assert len(compared) >= 3 and all(e["status"] in ("compared", "fused") for e in layers)
    m.tap(",".join(compared))
    assert np.array_equal(m.predict_numpy(x), y0)
    taps = {n: m.tap_fetch(n, 0, (B, names[n])) for n in compared}
    m.tap("")
    monkeypatch.setenv("C3HIP_EXACT_CHUNK", "1")
    m.predict_exact(x[:1])
    want = {n: 0.0 for n in compared}
    for b in range(B):
        m.predict_exact(x[b:b + 1])
        for n in compared:
            want[n] = max(want[n], float(np.abs(taps[n][b].astype(np.float64) - m.exact_fetch(n, 0, (1, names[n]))[0]).max()))
    for e in layers:
        if e["status"] == "fused":
            assert e["name"] in ("act0", "act8"), "only what the product form computes inside a fused kernel"
            continue
        print(f"{name} {e['name']}: max |a - exact| = {e['max_abs_diff']:.6e} (host {want[e['name']]:.6e}), max |exact| = {e['ref_max_abs']:.4g}")
        assert np.float32(e["max_abs_diff"]) == np.float32(want[e["name"]]), e["name"]
        assert e["batches"] == 1 and e["windows"] == B


# ------------------------------------------------------------------------------------------------ 6: refusals leave the handle usable
def test_refusals_leave_the_handle_usable(oracle_mod):
    c = case("pileup_i32_indel_b5", oracle_mod)
    x = c["x"]
    m = make(syn.PILEUP, 18, True, c["sd"], exact=False)
    y0, d0 = m.predict_numpy(x), m.describe()
    with pytest.raises(_lib.C3Error, match="c3_model_set_exact"):
        m.answer("exact")
    with pytest.raises(_lib.C3Error, match="c3_model_set_exact"):
        m.verify(every=1, reference="exact")
    assert m._answer == "product" and m._verify_ref == "fp32" and m._verify is None
    assert np.array_equal(m.predict_numpy(x), y0) and m.describe() == d0, "without the exact form: refused, nothing changed"
    m.exact(True)
    ticket = m.submit(x, slot=1)
    with pytest.raises(_lib.C3Error, match="in flight"):
        m.answer("exact")
    with pytest.raises(_lib.C3Error, match="in flight"):
        m.verify(every=1, reference="exact")
    assert np.array_equal(m.wait(ticket), y0), "while a submit is pending: refused, the slot can still be waited"
    assert np.array_equal(m.predict_numpy(x), y0) and m.describe() == d0 + " exact=1"
    m.answer("exact")
    with pytest.raises(_lib.C3Error, match="answers from the exact form"):
        m.exact(False)
    want = f32(m.predict_exact(x))
    assert np.array_equal(m.predict_numpy(x), want) and m._exact
    # verify mode skips the batches of an exact-answer handle, as it does on a handle on the fp32 forms
    m.verify(every=1)
    assert np.array_equal(m.predict_numpy(x), want)
    st = m.verify_stats()
    assert (st["batches_submitted"], st["batches_checked"], st["batches_skipped"]) == (1, 0, 1)
    m.verify(every=0)
    m.answer("product")
    m.exact(False)
    assert np.array_equal(m.predict_numpy(x), y0)
    m.exact(True)
    # the device-resident entry stays the product forms on an exact-answer handle
    import torch
    m.verify(every=0, reference="fp32")
    m.answer("exact")
    xt = torch.from_numpy(x).to("cuda:0")
    assert np.array_equal(m.forward(xt).cpu().numpy(), y0), "c3_predict_device is what it was"


# ------------------------------------------------------------------------------------------------ 7: through the builder, and a server
def test_through_the_builder(oracle_mod, tmp_path, monkeypatch):
    from tests import refloop
    c = case("pileup_i32_indel_b5", oracle_mod)
    ck = str(tmp_path / "model")
    sd = refloop.write_checkpoint(ck + ".pt", syn.PILEUP, 18, True)
    monkeypatch.setattr(predict, "_VERIFIED", [])
    monkeypatch.setattr("atexit.register", lambda fn: None)
    x = c["x"]
    want = f32(make(syn.PILEUP, 18, True, sd).predict_exact(x))
    monkeypatch.setenv("C3HIP_ANSWER", "exact")
    m = predict.build_model(True, True, chkpnt_fn=ck)
    assert precision(m) == "exact" and m._exact and np.array_equal(m.predict_numpy(x), want)
    monkeypatch.delenv("C3HIP_ANSWER")
    monkeypatch.setenv("C3HIP_VERIFY", "2,replace")
    monkeypatch.setenv("C3HIP_VERIFY_REF", "exact")
    m = predict.build_model(True, True, chkpnt_fn=ck)
    st = m.verify_stats()
    assert (st["every"], st["policy"]) == (2, "replace") and m.verify_extra()["reference"] == "exact" and m._exact
    assert "policy:replace" in m.describe() and m.describe().endswith(",ref:exact exact=1") and precision(m) in ("fp16x3", "fp32-auto")
    m.predict_numpy(x)
    line = predict.verify_summary(m)
    assert "submitted=1 checked=" in line and line.endswith(f" ref=exact replaced={m.verify_extra()['rows_replaced']}")


def test_a_server_answers_from_the_exact_form(oracle_mod, tmp_path):
    from clair3_amd import client
    from tests import refloop
    c = case("pileup_i32_indel_b5", oracle_mod)
    ck = str(tmp_path / "model")
    sd = refloop.write_checkpoint(ck + ".pt", syn.PILEUP, 18, True)
    want = f32(make(syn.PILEUP, 18, True, sd).predict_exact(c["x"]))
    sock, log = str(tmp_path / "c3.sock"), open(str(tmp_path / "serve.log"), "w+")
    env = {k: v for k, v in os.environ.items() if k != "C3HIP_SERVER"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, refloop.STUBS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env["C3HIP_ANSWER"] = "exact"
    cmd = [sys.executable, "-m", "clair3_amd.serve", "--socket", sock, "--model", f"pileup={ck}", "--add_indel_length"]
    proc = subprocess.Popen(cmd, env=env, stdout=log, stderr=subprocess.STDOUT, cwd=str(tmp_path))
    try:
        end = time.monotonic() + 120
        while True:
            if proc.poll() is not None:
                log.seek(0)
                pytest.fail(f"the server ended with status {proc.returncode}\n{log.read()[-3000:]}")
            try:
                hello = client.control(sock, "hello", timeout=5)
                break
            except client.ServerError:
                assert time.monotonic() < end, "the server did not come up"
                time.sleep(0.05)
        assert hello["models"]["pileup"]["answer"] == "exact" and hello["models"]["pileup"]["verify_reference"] == "fp32"
        remote = client.RemoteModel(sock, "pileup", add_indel_length=True, timeout=60)
        rows = remote.predict_numpy(c["x"])
        remote.close()
        assert np.array_equal(rows, want), "one request through the server: bit for bit the exact-answer rows"
        assert client.control(sock, "stats")["answer"] == {"pileup": "exact"}
        client.control(sock, "shutdown", timeout=10)
        proc.wait(timeout=30)
    finally:
        if proc.poll() is None:
            proc.terminate()
            try:
                proc.wait(timeout=20)
            except subprocess.TimeoutExpired:
                proc.kill()
                proc.wait()
        log.close()


# ------------------------------------------------------------------------------------------------ 8: score mode on an exact-answer handle
def test_score_mode_scores_the_exact_rows(oracle_mod):
    c = case("pileup_i32_indel_b5", oracle_mod)
    x = c["x"]
    m = make(syn.PILEUP, 18, True, c["sd"]).answer("exact")
    want = f32(m.predict_exact(x))
    rng = np.random.default_rng(905)
    labels = np.zeros((len(x), 90), np.int8)
    for lo, hi in syn.head_slices(90):
        labels[np.arange(len(x)), lo + np.where(rng.random(len(x)) < 0.5, want[:, lo:hi].argmax(1), rng.integers(0, hi - lo, size=len(x)))] = 1
    r = m.score(x, labels, window_loss=True, rows=True)
    assert np.array_equal(r.rows, want), "the rows of a scored batch are the float32 exact rows"
    ref = syn.focal_scores(want, labels, gamma=2.0)
    L, W = r.window_loss.astype(np.float64), ref["window_loss"]
    bound = 2.0 ** -23 * np.abs(W) + 1e-30  # tests/test_score_gpu.py: one float32 rounding of a double result
    print(f"score on exact rows: worst |d| / bound {float((np.abs(L - W) / bound).max()):.3f}")
    assert (np.abs(L - W) <= bound).all()
    for t in range(ref["tasks"]):
        assert abs(r.loss_sum[t] - ref["loss_sum"][t]) <= len(x) * 2.0 ** -52 * abs(ref["loss_sum"][t])
    assert list(r.correct) == list(ref["correct"]) and r.windows == len(x)
    without = m.score(x, labels)  # the rows stay on the device
    assert list(without.loss_sum) == list(r.loss_sum) and list(without.correct) == list(r.correct)


# ------------------------------------------------------------------------------------------------ 9: the audit tool through the ring
def test_audit_on_ring_reproduces_the_blocking_table(oracle_mod, monkeypatch):
    monkeypatch.setenv("C3HIP_FP32", "0")
    sd, x = sensitive_tile()
    m = make(syn.PILEUP, 18, True, sd)
    blocking = audit.audit(m, x, ["lstm2"])
    ring = audit.audit_on_ring(m, x, ["lstm2"])
    assert [line["form"] for line in ring] == ["none", "all", "lstm2"] == [line["form"] for line in blocking[1:]]
    for b, r in zip(blocking[1:], ring):
        print(r)
        assert r["max_abs_err"] == b["max_abs_err"], f"{r['form']}: the maxima are those of the blocking tool, bit for bit (the rows are the same rows)"
        assert (r["rows_over_tol"], r["label_diffs"], r["near_ties"], r["windows"]) == (b["rows_over_tol"], b["label_diffs"], b["near_ties"], b["windows"])
        assert [np.float32(v) for v in r["head_max_abs_err"]] == [np.float32(v) for v in b["head_max_abs_err"]]
        assert r["batches_checked"] == 1 and r["batches_skipped"] == 0
    assert m._verify_ref == "fp32" and m.verify_stats()["every"] == 0 and m.layer_precision() == ()
