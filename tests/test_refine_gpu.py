"""Refine mode on the submit / wait ring (needs an MI355X): c3_model_set_refine, c3_model_refine_stats, c3_refine_select.

Yardsticks: ``predict_exact`` of the same handle (the blocking entry, held to the fp64 oracle by tests/test_exact_gpu.py), a second handle
WITHOUT refine mode, and the numpy rule synthetic.refine_gaps / refine_select -- never a refine path measured against itself.  Every
comparison is bitwise: a refined row is ONE rounding of the exact row, an unrefined row is the product row, the selection and the totals are
integers, minima and maxima of float32 values.  The shapes are those of tests/test_exact_ring_gpu.py CASES plus one pileup batch of
256 * 4 + 1 windows (17 workgroups of the selection: the compaction across workgroups)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from clair3_amd import _lib, decode, predict, synthetic as syn
from tests import util
from tests.test_exact_ring_gpu import CASES, ENV, f32, make
from tests.test_refine import corner_rows, random_rows

pytestmark = pytest.mark.gpu

F32 = np.float32
BIG = "pileup_i8_b1025"
SHAPES = dict(CASES)
SHAPES[BIG] = (syn.PILEUP, 18, None, False, 256 * 4 + 1, np.int8, 66, 68)
_cases = {}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV + ("C3HIP_REFINE", "C3HIP_PREDICT_CHUNK"):
        monkeypatch.delenv(k, raising=False)


def case(name):
    """weights and windows of a case, made once and left unchanged"""
    if name not in _cases:
        kind, ch, depth, indel, n, dtype, s_sd, s_x = SHAPES[name]
        sd = syn.make_state_dict(kind, ch, indel, seed=s_sd, trained_like=name == "fa_c9_d55_b2")
        x = syn.make_pileup_windows(n, seed=s_x, dtype=dtype) if kind == syn.PILEUP else syn.make_fa_windows(n, seed=s_x, channels=ch, depth=depth or 89)
        _cases[name] = dict(kind=kind, ch=ch, depth=depth, indel=indel, sd=sd, x=x, nout=90 if indel else 24)
    return _cases[name]


def handle(c, columns=False):
    """a handle of the case with the exact form loaded and refine mode off"""
    return make(c["kind"], c["ch"], c["indel"], c["sd"], c["depth"]).decode_columns(columns)


def kth_gap(rows, nout, k):
    """the k-th smallest per-window minimum gap of ``rows`` (float32): a gap that selects some windows and leaves others"""
    mins = syn.refine_select(rows, nout, 0.0)[1]
    return float(np.sort(mins)[k])


def expected_stats(y_plain, want, nout, gap, sel):
    """refine_stats() of ONE refined batch, from numpy: the plain handle's rows, the exact float32 rows, the numpy rule's selection"""
    g = syn.refine_gaps(y_plain, nout)
    with np.errstate(invalid="ignore"):
        below = g <= F32(gap)
    changed = np.zeros(len(sel), bool)
    for lo, hi in syn.head_slices(nout):
        changed |= y_plain[sel, lo:hi].argmax(1) != want[sel, lo:hi].argmax(1)
    return dict(batches=1, batches_refined=int(len(sel) > 0), batches_skipped=0, windows=len(y_plain), windows_selected=len(sel), windows_changed=int(changed.sum()),
                head_selected=[int(v) for v in below[:, :4].sum(0)], decoder_selected=int(below[:, 4].sum()),
                min_gap=[float(v) for v in np.fmin.reduce(g[:, :4], axis=0)],
                max_abs_diff=float(np.abs(want[sel] - y_plain[sel, :nout]).max()) if len(sel) else 0.0, gap=float(F32(gap)))


# ------------------------------------------------------------------------------------------------ 1: the selection alone
@pytest.mark.parametrize("name", ["pileup_i8_b17", "pileup_i32_indel_b5"])
def test_refine_select_equals_the_numpy_rule(name):
    c = case(name)
    nout = c["nout"]
    m = make(c["kind"], c["ch"], c["indel"], c["sd"], c["depth"], exact=False)  # (the selection needs neither the mode nor the exact form)
    for columns in (False, True):
        rows, gap, names, expect = corner_rows(nout, columns)
        idx, mins = m.refine_select(rows, gap)
        want_idx, want_mins = syn.refine_select(rows, nout, gap)
        assert np.array_equal(idx, expect) and np.array_equal(idx, want_idx), (columns, [names[i] for i in idx])
        assert np.array_equal(mins, want_mins, equal_nan=True), columns
        rows = random_rows(nout, columns, n=64 * 3 + 5, seed=7)
        for gap in (0.0, 1e-4, 0.02, 2.0):
            idx, mins = m.refine_select(rows, gap)
            want_idx, want_mins = syn.refine_select(rows, nout, gap)
            assert idx.dtype == np.int32 and np.array_equal(idx, want_idx) and (np.diff(idx) > 0).all(), (columns, gap)
            assert np.array_equal(mins, want_mins, equal_nan=True), (columns, gap)
    assert len(m.refine_select(np.zeros((0, nout), F32), 1e-4)[0]) == 0
    with pytest.raises(_lib.C3Error, match="gap must be"):
        m.refine_select(np.zeros((1, nout), F32), -1.0)
    with pytest.raises(_lib.C3Error, match="rows of 25 floats"):
        m.refine_select(np.zeros((1, 25), F32), 1e-4)


def test_refine_select_on_product_rows_across_workgroups():
    c = case(BIG)
    m = handle(c, columns=True)
    y = m.predict_numpy(c["x"])
    for k in (0, len(y) // 3, len(y) - 1):
        gap = kth_gap(y, 24, k)
        idx, mins = m.refine_select(y, gap)
        want_idx, want_mins = syn.refine_select(y, 24, gap)
        assert np.array_equal(idx, want_idx) and np.array_equal(mins, want_mins) and len(idx) >= k + 1, k
    assert len(set(idx // 64)) == 17, "every workgroup of the selection holds a selected window"


# ------------------------------------------------------------------------------------------------ 2: per case, a gap chosen from the data
@pytest.mark.parametrize("columns", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_selected_rows_are_exact_rows_and_the_rest_product_rows(name, columns):
    c = case(name)
    x, nout = c["x"], c["nout"]
    plain = handle(c, columns)
    y_plain = plain.predict_numpy(x)
    gap = kth_gap(y_plain, nout, len(x) // 3)
    sel = syn.refine_select(y_plain, nout, gap)[0]
    rest = np.setdiff1d(np.arange(len(x)), sel)
    assert 0 < len(sel) < len(x), f"{name}: the gap {gap:.3g} selects {len(sel)} of {len(x)} windows"
    m = handle(c, columns).refine(gap)
    want = f32(m.predict_exact(x))
    want_sel = f32(m.predict_exact(np.ascontiguousarray(x[sel])))
    y = m.predict_numpy(x)
    st = m.refine_stats()
    print(f"{name} columns={columns}: gap {gap:.3e} selects {len(sel)} of {len(x)}; {st}")
    assert y.shape == y_plain.shape and y.dtype == F32
    assert np.array_equal(y[sel, :nout], want_sel) and np.array_equal(y[sel, :nout], want[sel]), f"{name}: selected rows are the exact float32 rows"
    assert np.array_equal(y[rest], y_plain[rest]), f"{name}: every other row is the product row, decoder columns included"
    if columns:
        assert np.array_equal(y[sel], decode.decode_columns(m, want[sel])), f"{name}: the columns of a refined row come from its refined probabilities"
    exp = expected_stats(y_plain, want, nout, gap, sel)
    assert {k: st[k] for k in exp} == exp, (st, exp)
    assert f" refine=gap:{F32(gap):g},windows:{len(x)},selected:{len(sel)},changed:{exp['windows_changed']}" in m.describe() + " "
    # the totals add up over batches and start again on request
    assert np.array_equal(m.predict_numpy(x), y)
    st = m.refine_stats()
    assert st["batches"] == 2 and st["windows_selected"] == 2 * len(sel) and st["head_selected"] == [2 * v for v in exp["head_selected"]]
    assert m.refine_reset().refine_stats()["batches"] == 0 and m.refine_stats()["min_gap"] == [float("inf")] * 4


# ------------------------------------------------------------------------------------------------ 3: the edges of gap
@pytest.mark.parametrize("name", ["fa_c9_d55_b2", "pileup_i32_indel_b5"])
def test_gap_two_answers_every_row_exactly_and_gap_zero_none(name):
    c = case(name)
    x, nout = c["x"], c["nout"]
    plain = handle(c, columns=True)
    y_plain, d_plain = plain.predict_numpy(x), plain.describe()
    m = handle(c, columns=True).refine(2.0)
    want = f32(m.predict_exact(x))
    y = m.predict_numpy(x)
    assert np.array_equal(y[:, :nout], want) and np.array_equal(y, decode.decode_columns(m, want)), "gap = 2: every row is the exact-answer row"
    st = m.refine_stats()
    assert st["windows_selected"] == len(x) and st["batches_refined"] == 1
    m.refine(0.0)
    m.refine_reset()
    assert syn.refine_select(y_plain, nout, 0.0)[0].size == 0, "these rows hold no exact tie"
    assert np.array_equal(m.predict_numpy(x), y_plain)
    st, d = m.refine_stats(), m.describe()
    assert (st["batches"], st["batches_refined"], st["batches_skipped"], st["windows"], st["windows_selected"]) == (1, 0, 0, len(x), 0), st
    field = f" refine=gap:0,windows:{len(x)},selected:0,changed:0"
    assert d.endswith(field) and d[:-len(field)] == d_plain, (d, d_plain)


# ------------------------------------------------------------------------------------------------ 4: the label claim
@pytest.mark.parametrize("kind,ch,seeds", [(syn.FULL_ALIGNMENT, 8, (71, 72)), (syn.PILEUP, 18, (73, 74))])
def test_every_label_is_the_exact_label_at_the_default_gap(kind, ch, seeds):
    sd = syn.make_state_dict(kind, ch, True, seed=seeds[0])
    x = syn.make_windows(kind, 64, seed=seeds[1], channels=ch)
    plain = make(kind, ch, True, sd)
    m = make(kind, ch, True, sd).refine()
    gap = m.refine_stats()["gap"]
    assert gap == float(F32(1e-4)), "the default gap is verify mode's tol"
    want = f32(m.predict_exact(x))
    err = float(np.abs(plain.predict_numpy(x).astype(np.float64) - want.astype(np.float64)).max())
    print(f"{kind}: max |product - exact| = {err:.3e} (gap / 2 = {gap / 2:.3e})")
    assert err < gap / 2, "the precondition of the argument: the forms' row error lies far below the gap"
    y = m.predict_numpy(x)
    st = m.refine_stats()
    print(f"{kind}: {st}")
    for lo, hi in syn.head_slices(90):
        assert np.array_equal(y[:, lo:hi].argmax(1), want[:, lo:hi].argmax(1)), (kind, lo)


# ------------------------------------------------------------------------------------------------ 5: the ring
def test_slots_lanes_parts_and_rows_on_the_device(monkeypatch):
    import torch
    c = case("pileup_i8_b17")
    x, nout = c["x"], c["nout"]
    plain = handle(c, columns=True)
    y_plain = plain.predict_numpy(x)
    gap = kth_gap(y_plain, nout, 4)
    sel = syn.refine_select(y_plain, nout, gap)[0]
    assert len(sel) == 5, "five selected windows"
    monkeypatch.setenv("C3HIP_EXACT_CHUNK", "2")  # ... in passes of 2, 2 and 1
    m = handle(c, columns=True).refine(gap)
    y = m.predict_numpy(x)
    want = f32(m.predict_exact(x))
    assert np.array_equal(y[sel, :nout], want[sel]) and not np.array_equal(y[sel], y_plain[sel]), "five selected windows through passes of two"
    assert np.array_equal(np.delete(y, sel, 0), np.delete(y_plain, sel, 0))
    assert "ring_lanes=2" in m.describe()
    # two slots in flight on different lanes, waited for in the other order
    t1, t3 = m.submit(x[:9], slot=1), m.submit(x[9:], slot=3)
    assert np.array_equal(m.wait(t3), y[9:]) and np.array_equal(m.wait(t1), y[:9]), "two slots in flight"
    # three parts, one of them without a selected window or empty
    parts = [x[:1], x[1:1], x[1:12], x[12:]]
    got = m.wait(m.submit_parts(parts, slot=2))
    assert [len(g) for g in got] == [1, 0, 11, 5] and np.array_equal(np.concatenate(got), y), "a batch of parts"
    assert np.array_equal(np.concatenate(m.predict_parts([x[:7], x[7:8], x[8:]])), y)
    # rows that stay on the device
    m.refine_reset()
    y_dev = torch.full((len(x), y.shape[1]), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert m.wait(m.submit_dev(x, y_dev.data_ptr(), slot=1)) is None
    torch.cuda.synchronize()
    assert np.array_equal(y_dev.cpu().numpy(), y), "submit_dev: the refined rows are in the caller's device tensor"
    st = m.refine_stats()
    assert (st["batches"], st["batches_refined"], st["windows_selected"]) == (1, 1, 5), st


CHILD = r"""
import json
import numpy as np
from clair3_amd import synthetic as syn
from tests.test_refine_gpu import case, handle, kth_gap

c = case("pileup_i8_b17")
x = np.concatenate([c["x"], c["x"][::-1]])[:20]
plain = handle(c, columns=True)
y_plain = np.concatenate([plain.predict_numpy(x[:10]), plain.predict_numpy(x[10:])])
gap = kth_gap(y_plain, 24, 6)
m = handle(c, columns=True).refine(gap)
whole = m.wait(m.submit(x, slot=0))  # one batch of the ring
one = m.refine_stats()
m.refine_reset()
cut = m.predict_numpy(x)  # chunks of 8 and 12 windows
two = m.refine_stats()
sel = syn.refine_select(y_plain, 24, gap)[0]
print("RESULT " + json.dumps(dict(equal=bool(np.array_equal(cut, whole)), one=one, two=two, selected=len(sel),
                                  rest_equal=bool(np.array_equal(np.delete(cut, sel, 0), np.delete(y_plain, sel, 0))))))
"""


def test_a_blocking_call_beyond_one_chunk():
    """a child process: C3HIP_PREDICT_CHUNK is read once per process"""
    env = dict(os.environ, C3HIP_PREDICT_CHUNK="8", PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=util.ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert out["equal"] and out["rest_equal"], "two chunks (C3HIP_PREDICT_CHUNK=8): the rows of one batch"
    assert out["one"]["batches"] == 1 and out["two"]["batches"] >= 2, "the blocking call travelled as chunks"
    assert out["selected"] >= 7 and out["one"]["windows_selected"] == out["two"]["windows_selected"] == out["selected"]
    for k in ("windows", "windows_changed", "head_selected", "decoder_selected", "min_gap", "max_abs_diff"):
        assert out["one"][k] == out["two"][k], k


# ------------------------------------------------------------------------------------------------ 6: precedence and refusals
def test_precedence_and_refusals():
    c = case("pileup_i32_indel_b5")
    x, nout = c["x"], c["nout"]
    plain = handle(c)
    depths = np.array([100, 300, 0, 217, 1000], np.int32)
    region, _ = syn.make_pileup_region(400, n_chunks=2, seed=902, empty_runs=((120, 1),))
    starts = np.array([0, 7, 33, 150, 367], np.int32)
    y_depth, y_region = plain.predict_numpy(x, depths=depths), plain.predict_region(region, starts)
    m = handle(c).refine(2.0)  # (every window of a batch the mode covers would be answered exactly)
    want = f32(m.predict_exact(x))
    assert np.array_equal(m.predict_numpy(x, depths=depths), y_depth), "a batch with depths is answered as without the mode"
    assert np.array_equal(m.predict_region(region, starts), y_region), "... and so is a region batch"
    st = m.refine_stats()
    assert (st["batches"], st["batches_skipped"], st["batches_refined"], st["windows"]) == (2, 2, 0, 0), st
    # an exact-answer handle and a scored batch count as skipped too
    m.answer("exact")
    assert np.array_equal(m.predict_numpy(x), want) and m.refine_stats()["batches_skipped"] == 3
    m.answer("product")
    labels = np.zeros((len(x), nout), np.int8)
    labels[:, [0, 21, 24, 57]] = 1
    m.score(x, labels)
    st = m.refine_stats()
    assert (st["batches"], st["batches_skipped"], st["batches_refined"]) == (4, 4, 0), st
    m.score_mode(enable=False)
    # the two owners of the same rows refuse each other, and each names the other
    with pytest.raises(_lib.C3Error, match="refine"):
        m.verify(every=1)
    rc = _lib.lib().c3_model_set_verify(m._handle, 1, 1e-4, 1e-6, _lib.VERIFY_REPORT)
    assert rc != 0 and "refine mode is on" in _lib.last_error()
    m.verify(every=0)  # (switching verify mode off is no conflict)
    other = handle(c)
    other.verify(every=2)
    with pytest.raises(_lib.C3Error, match="verify mode is on"):
        other.refine()
    assert other._refine is None and " refine=" not in other.describe()
    other.verify(every=0)
    assert " refine=" in other.refine().describe()
    for bad in (-1e-4, float("nan"), float("inf"), "wide"):
        with pytest.raises(_lib.C3Error, match="gap must be"):
            other.refine(bad)
    with pytest.raises(_lib.C3Error, match="refine mode"):
        other.exact(False)
    # without the exact form: the message of c3_model_set_answer
    bare = make(c["kind"], c["ch"], c["indel"], c["sd"], c["depth"], exact=False)
    with pytest.raises(_lib.C3Error, match=r"the exact form was not enabled at the last load: c3_model_set_exact\(m, 1\), then c3_model_load"):
        bare.refine()
    assert bare._refine is None and np.array_equal(bare.predict_numpy(x), plain.predict_numpy(x))
    # a reload keeps the mode and starts the totals again; switched off, the handle is the parent's
    assert np.array_equal(m.predict_numpy(x), want) and m.refine_stats()["batches_refined"] == 1
    m.load_state_dict(c["sd"])
    assert m.refine_stats()["batches"] == 0 and " refine=gap:2," in m.describe()
    assert np.array_equal(m.predict_numpy(x), want), "after a reload"
    m._create(m._device)  # (what .to(another device) does: a handle created anew takes the mode along)
    assert np.array_equal(m.predict_numpy(x), want) and " refine=gap:2," in m.describe()
    m.refine(enable=False)
    y_plain, d_plain = plain.predict_numpy(x), plain.describe()
    assert np.array_equal(m.predict_numpy(x), y_plain) and m.describe() == d_plain, (m.describe(), d_plain)
    assert m.refine_stats()["batches"] == 1, "the totals stay readable"


# ------------------------------------------------------------------------------------------------ 7: the drop-in: a worker process
def test_worker_process_leaves_one_summary_line_on_stderr(tmp_path):
    import re
    from tests import refloop
    from tests.test_verify_gpu import _worker
    ref = refloop.reference_root()
    if ref is None:
        pytest.skip("no reference modules (oracle/_ref is staged by the build)")
    d = str(tmp_path)
    sizes = [1300, 41]
    lst = refloop.write_job(d, syn.PILEUP, sizes, channels=18)
    ck = os.path.join(d, "model")
    refloop.write_checkpoint(ck + ".pt", syn.PILEUP, 18, False)
    plain = _worker(ref, d, lst, ck, os.path.join(d, "plain.vcf"), {})
    assert plain.returncode == 0, (plain.stdout + plain.stderr)[-3000:]
    ref_run = _worker(ref, d, lst, ck, os.path.join(d, "refine.vcf"), {"C3HIP_REFINE": "1e-4"})
    assert ref_run.returncode == 0, (ref_run.stdout + ref_run.stderr)[-3000:]
    summary = [ln for ln in ref_run.stderr.splitlines() if "[clair3_amd] refine" in ln]
    print(summary)
    assert len(summary) == 1 and summary[0].startswith("[clair3_amd] refine: gap=0.0001 batches="), ref_run.stderr[-3000:]
    fields = dict(re.findall(r"(\w+)=(\S+)", summary[0]))
    assert int(fields["windows"]) == sum(sizes) and int(fields["skipped"]) == 0, summary[0]
    assert "refine" not in plain.stderr and "refine" not in plain.stdout and "refine" not in ref_run.stdout
    assert len(ref_run.stdout.splitlines()) == len(plain.stdout.splitlines()) and len(ref_run.stderr.splitlines()) == len(plain.stderr.splitlines()) + 1
    a, b = refloop.vcf_records(os.path.join(d, "plain.vcf")), refloop.vcf_records(os.path.join(d, "refine.vcf"))
    assert len(a) == len(b) >= sum(sizes) // 2
    differ = sum(1 for ra, rb in zip(a, b) if ra != rb)
    print(f"{differ} of {len(a)} records differ; the line counts {fields['selected']} selected windows")
    assert differ <= int(fields["selected"]), "only records of selected windows can differ"
