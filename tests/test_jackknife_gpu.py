"""Jackknife mode on the device (needs an MI355X): c3_jackknife_rows, c3_jackknife, c3_jackknife_reduce.

Yardsticks: a second, plain handle that is handed the variants built in numpy (synthetic.leave_one_out -> predict_numpy) and the windows
themselves (predict_rows), and the numpy rule synthetic.jackknife_records applied to the rows the same call returned -- never a jackknife
path measured against itself.  Every comparison is bitwise: a window's row does not depend on the batch it travels in, and
the record holds only counts, comparisons and single float32 subtractions.  Windows come from syn.make_fa_windows with their counts forced
to 0, 1, 2, 17 and the full depth (an interior all-zero row inside the run of 17)."""
import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests.test_calibration import recipe_state_dict
from tests.test_jackknife import corner_rows, same, same_drops, same_records

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = {"c8_d89_indel": (8, 89, True, 31), "c9_d89": (9, 89, False, 32), "c8_d55": (8, 55, True, 33)}
_made = {}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("C3HIP_JACKKNIFE_CHUNK", "C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_PACK_ROWS", "C3HIP_REFINE", "C3HIP_VERIFY", "C3HIP_EXACT", "C3HIP_RANGE_GUARD"):
        monkeypatch.delenv(k, raising=False)


def make_fa(sd, channels=8, depth=89, indel=True, columns=False):
    m = Clair3_F(add_indel_length=indel, predict=True, input_channels=channels)
    m.set_geometry(depth, 33)
    m.to("cuda:0")
    m.load_state_dict(sd)
    return m.decode_columns(columns)


def forced(x, counts):
    """(rows, counts): window b of ``x`` cut or repeated to counts[b] reads, row 5 of a run of 17 zeroed"""
    out = []
    for b, n in enumerate(counts):
        run = x[b][(x[b] != 0).any(axis=(1, 2))]
        run = np.resize(run, (n,) + run.shape[1:]) if n else run[:0]
        if n == 17:
            run[5] = 0
        out.append(run)
    return np.concatenate(out), np.asarray(counts, np.int32)


def case(name):
    """weights, windows as rows, and the reference of a case on a plain handle, made once and left unchanged"""
    if name not in _made:
        ch, depth, indel, seed = CASES[name]
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, indel, seed=seed)
        x = syn.make_fa_windows(6, seed=seed + 100, channels=ch, depth=depth)
        natural = int((x[5] != 0).any(axis=(1, 2)).sum())
        rows, counts = forced(x, [0, 1, 2, 17, depth, natural])
        _made[name] = dict(ch=ch, depth=depth, indel=indel, sd=sd, rows=rows, counts=counts, nout=90 if indel else 24, handles={}, calls={}, want={})
    return _made[name]


def handles(c, columns):
    """(the handle under test, a plain handle that never runs the call), per case and row width"""
    if columns not in c["handles"]:
        c["handles"][columns] = tuple(make_fa(c["sd"], c["ch"], c["depth"], c["indel"], columns) for _ in range(2))
    return c["handles"][columns]


def call(c, columns, layout):
    if (columns, layout) not in c["calls"]:
        c["calls"][columns, layout] = handles(c, columns)[0].jackknife_rows(c["rows"], c["counts"], layout=layout, drops=True, variant_rows=True)
    return c["calls"][columns, layout]


PARAMS = [(n, col, lay) for n in CASES for col in (False, True) for lay in syn.JACKKNIFE_LAYOUTS]


# ------------------------------------------------------------------------------------------------ 1: the rows
@pytest.mark.parametrize("name,columns,layout", PARAMS)
def test_variant_rows_and_base_rows_are_those_of_a_plain_handle(name, columns, layout):
    c = case(name)
    m, plain = handles(c, columns)
    r = call(c, columns, layout)
    total = int(c["counts"].sum())
    assert r["variant_rows"].shape == (total, m.row_size) and r["drops"].shape == (total, 4) and r["rows"].dtype == syn.JACKKNIFE_DTYPE
    assert same(r["counts"], c["counts"]) and not r["on_fp32"] and r["passes"] == 1
    want_v = plain.predict_numpy(syn.leave_one_out(c["rows"], c["counts"], depth=c["depth"], layout=layout))
    assert same(r["variant_rows"], want_v), "the variants the device built are the numpy rule's, their rows a plain handle's"
    assert same(r["base_rows"], plain.predict_rows(c["rows"], c["counts"]))
    assert not same(want_v[4], want_v[5]), "the variants differ from each other"
    # dense windows: the run is found on the host, its first row is the run's own
    x = syn.pad_fa_rows(c["rows"], c["counts"], depth=c["depth"])
    d = m.jackknife(x, layout=layout, drops=True, variant_rows=True)
    firsts = ((c["depth"] - c["counts"]) // 2).astype(np.int32)
    e = m.jackknife_rows(c["rows"], c["counts"], firsts, layout=layout, drops=True, variant_rows=True)
    for got in (d, e):
        assert same(got["counts"], c["counts"]) and same_records(got["rows"], r["rows"]) and same(got["base_rows"], r["base_rows"])
        assert same(got["variant_rows"], r["variant_rows"]) and same(got["drops"], r["drops"])
    # runs that do not sit in the centre: at the top and at the bottom of the window
    firsts = np.where(np.arange(len(c["counts"])) % 2, c["depth"] - c["counts"], 0).astype(np.int32)
    e = m.jackknife_rows(c["rows"], c["counts"], firsts, layout=layout, variant_rows=True)
    assert same(e["variant_rows"], plain.predict_numpy(syn.leave_one_out(c["rows"], c["counts"], firsts, depth=c["depth"], layout=layout)))
    assert same(e["base_rows"], plain.predict_rows(c["rows"], c["counts"], firsts)) and "drops" not in e


# ------------------------------------------------------------------------------------------------ 2: the records
@pytest.mark.parametrize("name,columns,layout", PARAMS)
def test_records_equal_the_numpy_rule_on_the_same_rows(name, columns, layout):
    c = case(name)
    r = call(c, columns, layout)
    rec, drops = syn.jackknife_records(r["base_rows"], r["variant_rows"], r["counts"], c["nout"])
    assert same_records(r["rows"], rec), {k: (r["rows"][k].tolist(), rec[k].tolist()) for k in rec.dtype.names if not same(r["rows"][k], rec[k])}
    assert same(r["drops"], drops)
    assert r["rows"]["reads"].tolist() == c["counts"].tolist() and (r["rows"]["lean_read"][0] == -1).all() and not r["rows"]["nonfinite"].any()
    assert r["rows"]["max_delta"][1:].min() > 0, "taking a read away moves the row"
    # the reduction alone on the same rows gives the same records
    alone = handles(c, columns)[1].jackknife_reduce(r["base_rows"], r["variant_rows"], r["counts"], drops=True)
    assert same_records(alone["rows"], rec) and same(alone["drops"], drops)


# ------------------------------------------------------------------------------------------------ 3: hand-made rows
@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
@pytest.mark.parametrize("indel", [False, True])
def test_reduce_on_hand_made_rows(kind, indel):
    nout = 90 if indel else 24
    if kind == syn.PILEUP:
        m = Clair3_P(add_indel_length=indel, predict=True).to("cuda:0")  # (the reduction needs no weights)
    else:
        m = make_fa(syn.make_state_dict(kind, 8, indel, seed=3), indel=indel)
    for columns in (False, True):
        names, base, var, counts = corner_rows(nout, columns)
        got = m.jackknife_reduce(base, var, counts, drops=True)
        rec, drops = syn.jackknife_records(base, var, counts, nout)
        bad = [names[i] for i in range(len(names)) if got["rows"][i].tobytes() != rec[i].tobytes()]
        assert same_records(got["rows"], rec), (columns, bad)
        assert same_drops(got["drops"], drops) and np.isnan(drops).any(), columns
        assert got["rows"]["flips"].sum() > 0 and got["rows"]["nonfinite"].sum() > 0
        assert "drops" not in m.jackknife_reduce(base, var, counts)
    empty = m.jackknife_reduce(np.zeros((0, nout), F32), np.zeros((0, nout), F32), np.zeros(0, np.int32), drops=True)
    assert len(empty["rows"]) == 0 and empty["drops"].shape == (0, 4)
    with pytest.raises(_lib.C3Error, match="rows of"):
        m.jackknife_reduce(np.zeros((1, nout + 1), F32), np.zeros((1, nout + 1), F32), np.ones(1, np.int32))
    with pytest.raises(_lib.C3Error, match="negative row_count"):
        m.jackknife_reduce(np.zeros((1, nout), F32), np.zeros((0, nout), F32), np.array([-1], np.int32))


# ------------------------------------------------------------------------------------------------ 4: the cuts
def test_passes_and_micro_batches_do_not_show(monkeypatch):
    """24 windows of 89 reads are 24 + 2136 dense windows: as one pass a micro-batch of 2048 ends inside a window's variants"""
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=31)
    m = make_fa(sd, columns=True)
    x = syn.make_fa_windows(24, seed=5, recipe="uniform")
    rows, counts = x.reshape(24 * 89, 33, 8), np.full(24, 89, np.int32)
    results = {}
    for chunk, passes in (("0", 1), ("5", 5), ("1", 24)):
        monkeypatch.setenv("C3HIP_JACKKNIFE_CHUNK", chunk)
        r = results[chunk] = m.jackknife_rows(rows, counts, drops=True, variant_rows=True)
        assert r["passes"] == passes and len(r["variant_rows"]) == 24 * 89
    monkeypatch.delenv("C3HIP_JACKKNIFE_CHUNK")
    assert m.jackknife_rows(rows, counts)["passes"] == 1, "24 windows fit the default pass of 64"
    for chunk in ("5", "1"):
        for key in ("base_rows", "variant_rows", "drops"):
            assert same(results[chunk][key], results["0"][key]), (chunk, key)
        assert same_records(results[chunk]["rows"], results["0"]["rows"]), chunk
    # the rows on either side of the micro-batch boundary (dense window 2048 = variant 2024) against a plain batch
    v = syn.leave_one_out(rows[22 * 89:], counts[22:])[2000 - 22 * 89:2050 - 22 * 89]
    assert same(results["0"]["variant_rows"][2000:2050], m.predict_numpy(v))
    rec, drops = syn.jackknife_records(results["0"]["base_rows"], results["0"]["variant_rows"], counts, 90)
    assert same_records(results["0"]["rows"], rec) and same(results["0"]["drops"], drops)
    assert results["0"]["bytes_staged"] < results["1"]["bytes_staged"] < 24 * 89 * 33 * 8 + 24 * 90 * 24 + 24 * 1024


# ------------------------------------------------------------------------------------------------ 5: the handle is left as it was
def state(m):
    return m.describe(), m.verify_stats(), m.refine_stats(), m.range_status(), m.layer_precision()


def test_the_handle_is_left_as_it_was():
    c = case("c8_d89_indel")
    sd, rows, counts = c["sd"], c["rows"], c["counts"]
    x = syn.make_fa_windows(7, seed=9)
    used, fresh = make_fa(sd), make_fa(sd)
    for m in (used, fresh):
        m.predict_rows(rows, counts)  # (rows_windows= of the last call)
    before = state(used)
    assert "rows_windows=6" in before[0]
    r = used.jackknife_rows(rows, counts, drops=True, variant_rows=True)
    assert state(used) == before == state(fresh)
    assert same(used.predict_numpy(x), fresh.predict_numpy(x)) and state(used) == state(fresh)
    tickets = [[m.submit(x[k:k + 3], slot=k) for k in range(3)] for m in (used, fresh)]
    # refused while a submit is pending on any slot, and nothing of the pending batches is disturbed
    with pytest.raises(_lib.C3Error, match="a prediction is in flight: call c3_predict_wait first"):
        used.jackknife_rows(rows, counts)
    with pytest.raises(_lib.C3Error, match="in flight"):
        used.jackknife(x)
    got = [[m.wait(t) for t in ts] for m, ts in zip((used, fresh), tickets)]
    assert all(same(a, b) for a, b in zip(*got)) and all(same(got[0][k], fresh.predict_numpy(x[k:k + 3])) for k in range(3))
    again = used.jackknife_rows(rows, counts, drops=True, variant_rows=True)  # works after the wait, and gives what it gave
    assert all(same(again[k], r[k]) for k in ("base_rows", "variant_rows", "drops")) and same_records(again["rows"], r["rows"])


def test_it_runs_on_the_forms_the_handle_is_on(monkeypatch):
    c = case("c8_d89_indel")
    sd, rows, counts = c["sd"], c["rows"], c["counts"]
    variants = syn.leave_one_out(rows, counts)
    monkeypatch.setenv("C3HIP_FP32", "1")
    f32 = make_fa(sd)
    monkeypatch.delenv("C3HIP_FP32")
    plan = make_fa(sd)
    plan.layer_precision("conv3,res2a")
    product = call(c, False, "recentre")
    for m, name in ((f32, "fp32-forced"), (plan, "fp32_layers=conv3,res2a")):
        before = m.describe()
        r = m.jackknife_rows(rows, counts, variant_rows=True)
        assert m.describe() == before and name in before and not r["on_fp32"]
        assert same(r["base_rows"], m.predict_rows(rows, counts)) and same(r["variant_rows"], m.predict_numpy(variants))
        assert not same(r["variant_rows"], product["variant_rows"]), "other forms, other bits"
        assert same_records(r["rows"], syn.jackknife_records(r["base_rows"], r["variant_rows"], counts, 90)[0])


# ------------------------------------------------------------------------------------------------ 6: the range guard
def test_range_guard_runs_the_pass_again_on_fp32_for_this_call_alone(monkeypatch, capfd):
    sd = recipe_state_dict()
    x = syn.make_fa_windows(3, seed=62)
    rows, _, counts = syn.pack_fa_rows(x)
    m, never = make_fa(sd), make_fa(sd)
    monkeypatch.setenv("C3HIP_FP32", "1")
    f32 = make_fa(sd)
    monkeypatch.delenv("C3HIP_FP32")
    before = m.describe()
    r = m.jackknife_rows(rows, counts, drops=True, variant_rows=True)
    assert r["on_fp32"], "the checkpoint's activations leave the range of the fp16x3 kernels"
    assert same(r["base_rows"], f32.predict_rows(rows, counts)) and same(r["variant_rows"], f32.predict_numpy(syn.leave_one_out(rows, counts)))
    rec, drops = syn.jackknife_records(r["base_rows"], r["variant_rows"], counts, 90)
    assert same_records(r["rows"], rec) and same(r["drops"], drops) and not rec["nonfinite"].any()
    assert m.range_status() == (0, False) and m.describe() == before and "precision=fp16x3" in before
    assert "continues on fp32" not in capfd.readouterr().err, "the handle stays on its forms and says nothing"
    # the handle's next ordinary batch trips its own guard exactly as on a handle that never ran the call
    y, y_never = m.predict_numpy(x), never.predict_numpy(x)
    assert same(y, y_never) and same(y, f32.predict_numpy(x))
    assert m.range_status() == never.range_status() and m.range_status()[1] and m.describe() == never.describe()
    assert capfd.readouterr().err.count("continues on fp32") == 2
    assert not m.jackknife_rows(rows, counts)["on_fp32"], "a handle that is on the fp32 forms has no guard to meet"


# ------------------------------------------------------------------------------------------------ 7: refusals that need the device
def test_refusals():
    c = case("c8_d89_indel")
    sd, rows, counts = c["sd"], c["rows"], c["counts"]
    L = _lib.lib()
    rec = np.zeros(len(counts), syn.JACKKNIFE_DTYPE)
    p = Clair3_P(add_indel_length=True, predict=True)
    p.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, True, seed=1))
    assert L.c3_jackknife_rows(p._handle, rows.ctypes.data, None, counts.ctypes.data, len(counts), 0, None, rec.ctypes.data, None, None, None) != 0
    assert "counts, not reads" in _lib.last_error()
    assert L.c3_jackknife(p._handle, rows.ctypes.data, _lib.DTYPE_I8, 1, 0, None, rec.ctypes.data, None, None, None) != 0 and "counts, not reads" in _lib.last_error()
    empty = Clair3_F(add_indel_length=True, predict=True).to("cuda:0")
    with pytest.raises(_lib.C3Error, match="no weights"):
        empty.jackknife_rows(rows, counts)
    m = make_fa(sd)
    before = m.describe()
    bad = counts.copy()
    bad[2] = -1
    with pytest.raises(_lib.C3Error, match="window 2: negative row_count"):
        m.jackknife_rows(rows, bad)
    with pytest.raises(_lib.C3Error, match="counts add up"):
        m.jackknife_rows(rows[:-1], counts)
    firsts = np.zeros(len(counts), np.int32)
    firsts[3] = 89 - 16
    with pytest.raises(_lib.C3Error, match=r"window 3: rows \[73, 90\) reach beyond the depth"):
        m.jackknife_rows(rows, counts, firsts)
    firsts[3] = -1
    with pytest.raises(_lib.C3Error, match="window 3: negative row_first"):
        m.jackknife_rows(rows, counts, firsts)
    assert L.c3_jackknife_rows(m._handle, rows.ctypes.data, None, counts.ctypes.data, len(counts), 2, None, rec.ctypes.data, None, None, None) != 0
    assert "unknown layout 2" in _lib.last_error()
    assert L.c3_jackknife_rows(m._handle, rows.ctypes.data, None, counts.ctypes.data, len(counts), 0, None, None, None, None, None) != 0
    assert "null buffer" in _lib.last_error()
    with pytest.raises(_lib.C3Error, match="window shape"):
        m.jackknife(np.zeros((1, 89, 33, 9), np.int8))
    none = m.jackknife_rows(rows[:0], counts[:0], drops=True, variant_rows=True)
    assert len(none["rows"]) == 0 and none["passes"] == 0 and none["drops"].shape == (0, 4) and none["variant_rows"].shape == (0, 90)
    assert m.describe() == before
    # a handle that answers from the exact form
    m.exact(True)
    m.answer("exact")
    with pytest.raises(_lib.C3Error, match="answers from the exact form"):
        m.jackknife_rows(rows, counts)
    m.answer("product")
    assert same_records(m.jackknife_rows(rows, counts)["rows"], call(c, False, "recentre")["rows"])


# ------------------------------------------------------------------------------------------------ 8: the tool
def test_the_tool_prints_the_report_of_the_same_windows(tmp_path, capsys):
    import json
    import torch
    from clair3_amd import jackknife
    c = case("c8_d89_indel")
    x = syn.pad_fa_rows(c["rows"], c["counts"])
    np.save(str(tmp_path / "x.npy"), x)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in c["sd"].items()}, str(tmp_path / "m.pt"))
    out = str(tmp_path / "lines.json")
    assert jackknife.main(["--chkpnt_fn", str(tmp_path / "m.pt"), "--tensor_fn", str(tmp_path / "x.npy"), "--layout", "in_place", "--top", "4", "--out", out]) == 0
    printed = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    want = jackknife.report(handles(c, True)[0].jackknife(x, layout="in_place"), 90, 1e-4, 4)
    assert printed == json.loads(json.dumps(want)) == [json.loads(line) for line in open(out)]
    assert printed[-1]["windows"] == 6 and printed[-1]["variants"] == int(c["counts"].sum()) and sum(map(sum, printed[-1]["near_tie_table"])) == 6
