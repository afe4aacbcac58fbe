"""Subsample mode on the device (needs an MI355X): c3_subsample_rows, c3_subsample, c3_subsample_reduce.

Yardsticks: a second, plain handle that is handed the variants built in numpy (synthetic.subsample_variants -> predict_numpy) and the
windows themselves (predict_rows), the masks of the numpy rule (synthetic.subsample_masks), and synthetic.subsample_records applied to the
rows the same call returned -- never a subsample path measured against itself.  Every comparison is bitwise: a window's row does not depend
on the batch it travels in, and the records hold only counts, comparisons and copied float bits.  Windows come from
syn.make_fa_windows with their counts forced to 0, 1, 2, 17, the full depth and the window's own (an interior all-zero row inside the run of
17); with depths (1, 2, 16, 60) and three replicates a call builds at most 42 dense windows."""
import numpy as np
import pytest

from clair3_amd import _lib, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests.test_calibration import recipe_state_dict
from tests.test_jackknife_gpu import CASES, forced, make_fa
from tests.test_subsample import CORNER_DEPTHS, CORNER_R, corner_rows, same, same_records

pytestmark = pytest.mark.gpu

F32 = np.float32
DEPTHS, R, SEED = (1, 2, 16, 60), 3, 20261020
_made = {}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("C3HIP_SUBSAMPLE_CHUNK", "C3HIP_JACKKNIFE_CHUNK", "C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_PACK_ROWS", "C3HIP_REFINE", "C3HIP_VERIFY",
              "C3HIP_EXACT", "C3HIP_RANGE_GUARD"):
        monkeypatch.delenv(k, raising=False)


def case(name):
    """weights and windows as rows of a case, made once and left unchanged"""
    if name not in _made:
        ch, depth, indel, seed = CASES[name]
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, indel, seed=seed)
        x = syn.make_fa_windows(6, seed=seed + 100, channels=ch, depth=depth)
        natural = int((x[5] != 0).any(axis=(1, 2)).sum())
        rows, counts = forced(x, [0, 1, 2, 17, depth, natural])
        _made[name] = dict(ch=ch, depth=depth, indel=indel, sd=sd, rows=rows, counts=counts, nout=90 if indel else 24, handles={}, calls={})
    return _made[name]


def handles(c, columns):
    """(the handle under test, a plain handle that never runs the call), per case and row width"""
    if columns not in c["handles"]:
        c["handles"][columns] = tuple(make_fa(c["sd"], c["ch"], c["depth"], c["indel"], columns) for _ in range(2))
    return c["handles"][columns]


def call(c, columns, layout):
    if (columns, layout) not in c["calls"]:
        c["calls"][columns, layout] = handles(c, columns)[0].subsample_rows(c["rows"], c["counts"], depths=DEPTHS, replicates=R, seed=SEED, layout=layout,
                                                                            masks=True, variant_rows=True)
    return c["calls"][columns, layout]


def same_call(a, b, keys=("base_rows", "variant_rows", "masks")):
    return all(same(a[k], b[k]) for k in keys) and same_records(a["levels"], b["levels"]) and same_records(a["rows"], b["rows"])


PARAMS = [(n, col, lay) for n in CASES for col in (False, True) for lay in syn.JACKKNIFE_LAYOUTS]


# ------------------------------------------------------------------------------------------------ 1: masks and rows
@pytest.mark.parametrize("name,columns,layout", PARAMS)
def test_masks_and_rows_are_the_rule_s_and_a_plain_handle_s(name, columns, layout):
    c = case(name)
    m, plain = handles(c, columns)
    r = call(c, columns, layout)
    kw = dict(depths=DEPTHS, replicates=R, seed=SEED, layout=layout, masks=True, variant_rows=True)
    total = int(syn.subsample_variant_counts(c["counts"], DEPTHS, R).sum())
    assert 0 < total and total + len(c["counts"]) <= 72 and r["variants"] == total
    assert r["variant_rows"].shape == (total, m.row_size) and r["masks"].shape == (total, 2) and r["masks"].dtype == np.uint64
    assert r["levels"].shape == (6, len(DEPTHS)) and r["levels"].dtype == syn.SUBSAMPLE_LEVEL_DTYPE and r["rows"].dtype == syn.SUBSAMPLE_WINDOW_DTYPE
    assert same(r["counts"], c["counts"]) and not r["on_fp32"] and r["passes"] == 1
    assert same(r["masks"], syn.subsample_masks(c["counts"], DEPTHS, R, SEED, c["depth"])), "the subsets the device drew are the numpy rule's"
    want_v = plain.predict_numpy(syn.subsample_variants(c["rows"], c["counts"], None, DEPTHS, R, SEED, c["depth"], layout))
    assert same(r["variant_rows"], want_v), "the variants the device built are the numpy rule's, their rows a plain handle's"
    assert same(r["base_rows"], plain.predict_rows(c["rows"], c["counts"]))
    assert not same(want_v[0], want_v[-1]), "the variants differ from each other"
    # dense windows: the run is found on the host, its first row is the run's own; explicit centred firsts
    x = syn.pad_fa_rows(c["rows"], c["counts"], depth=c["depth"])
    d = m.subsample(x, **kw)
    firsts = ((c["depth"] - c["counts"]) // 2).astype(np.int32)
    e = m.subsample_rows(c["rows"], c["counts"], firsts, **kw)
    for got in (d, e):
        assert same(got["counts"], c["counts"]) and same_call(got, r)
    # runs that do not sit in the centre: at the top and at the bottom of the window
    firsts = np.where(np.arange(len(c["counts"])) % 2, c["depth"] - c["counts"], 0).astype(np.int32)
    e = m.subsample_rows(c["rows"], c["counts"], firsts, depths=DEPTHS, replicates=R, seed=SEED, layout=layout, variant_rows=True)
    assert same(e["variant_rows"], plain.predict_numpy(syn.subsample_variants(c["rows"], c["counts"], firsts, DEPTHS, R, SEED, c["depth"], layout)))
    assert same(e["base_rows"], plain.predict_rows(c["rows"], c["counts"], firsts)) and "masks" not in e
    if layout == "recentre":
        assert same(e["variant_rows"], r["variant_rows"]), "a recentred variant does not see where the base run sat"
    # another seed draws other subsets
    other = m.subsample_rows(c["rows"], c["counts"], depths=DEPTHS, replicates=R, seed=SEED + 1, layout=layout, masks=True)
    assert same(other["masks"], syn.subsample_masks(c["counts"], DEPTHS, R, SEED + 1, c["depth"])) and not same(other["masks"], r["masks"])


# ------------------------------------------------------------------------------------------------ 2: the records
@pytest.mark.parametrize("name,columns,layout", PARAMS)
def test_records_equal_the_numpy_rule_on_the_same_rows(name, columns, layout):
    c = case(name)
    r = call(c, columns, layout)
    lev, win = syn.subsample_records(r["base_rows"], r["variant_rows"], r["counts"], DEPTHS, R, c["nout"])
    assert same_records(r["levels"], lev), {k: (r["levels"][k].tolist(), lev[k].tolist()) for k in lev.dtype.names if not same(r["levels"][k], lev[k])}
    assert same_records(r["rows"], win), {k: (r["rows"][k].tolist(), win[k].tolist()) for k in win.dtype.names if not same(r["rows"][k], win[k])}
    assert r["rows"]["reads"].tolist() == c["counts"].tolist() and not r["levels"]["nonfinite"].any()
    assert r["rows"]["levels_run"][:5].tolist() == [0, 0, 1, 3, 4 if c["depth"] > 60 else 3] and r["levels"]["run"].sum() == r["variants"]
    assert (r["levels"]["keep"] == np.minimum(c["counts"][:, None], np.array(DEPTHS)[None, :])).all()
    # the reduction alone on the same rows gives the same records
    alone = handles(c, columns)[1].subsample_reduce(r["base_rows"], r["variant_rows"], r["counts"], DEPTHS, R)
    assert same_records(alone["levels"], lev) and same_records(alone["rows"], win)


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
        got = m.subsample_reduce(base, var, counts, CORNER_DEPTHS, CORNER_R)
        lev, win = syn.subsample_records(base, var, counts, CORNER_DEPTHS, CORNER_R, nout)
        bad = [names[i] for i in range(len(names)) if got["levels"][i].tobytes() != lev[i].tobytes() or got["rows"][i].tobytes() != win[i].tobytes()]
        assert same_records(got["levels"], lev) and same_records(got["rows"], win), (columns, bad)
        assert got["levels"]["flips"].sum() > 0 and got["levels"]["nonfinite"].sum() > 0 and got["rows"]["hold_level"].max() == len(CORNER_DEPTHS)
    # 32 replicates, 8 levels: every lane of the half wave holds a variant
    rng = np.random.default_rng(nout)
    counts, depths = np.array([100, 3, 0, 9], np.int32), (1, 2, 3, 5, 8, 13, 21, 34)
    total = int(syn.subsample_variant_counts(counts, depths, 32).sum())
    base, var = rng.random((4, nout)).astype(F32), rng.random((total, nout)).astype(F32)
    got = m.subsample_reduce(base, var, counts, depths, 32)
    lev, win = syn.subsample_records(base, var, counts, depths, 32, nout)
    assert same_records(got["levels"], lev) and same_records(got["rows"], win) and win["levels_run"].tolist() == [8, 2, 0, 5]
    empty = m.subsample_reduce(np.zeros((0, nout), F32), np.zeros((0, nout), F32), np.zeros(0, np.int32))
    assert len(empty["rows"]) == 0 and empty["levels"].shape == (0, 4)
    with pytest.raises(_lib.C3Error, match="rows of"):
        m.subsample_reduce(np.zeros((1, nout + 1), F32), np.zeros((0, nout + 1), F32), np.ones(1, np.int32))
    with pytest.raises(_lib.C3Error, match="negative row_count"):
        m.subsample_reduce(np.zeros((1, nout), F32), np.zeros((0, nout), F32), np.array([-1], np.int32))


# ------------------------------------------------------------------------------------------------ 4: the cut
@pytest.mark.parametrize("name", ["c8_d89_indel", "c9_d89"])
def test_the_cut_into_passes_does_not_show(name, monkeypatch):
    c = case(name)
    m = handles(c, True)[0]
    whole = call(c, True, "recentre")
    for chunk, passes in (("1", 6), ("2", 3), ("0", 1)):
        monkeypatch.setenv("C3HIP_SUBSAMPLE_CHUNK", chunk)
        r = m.subsample_rows(c["rows"], c["counts"], depths=DEPTHS, replicates=R, seed=SEED, masks=True, variant_rows=True)
        assert r["passes"] == passes and same_call(r, whole), chunk
    monkeypatch.delenv("C3HIP_SUBSAMPLE_CHUNK")
    # a window's subsets are those of its index in the CALL: the last two windows alone are windows 0 and 1 of another call
    tail = m.subsample_rows(c["rows"][-int(c["counts"][4:].sum()):], c["counts"][4:], depths=DEPTHS, replicates=R, seed=SEED, masks=True)
    assert same(tail["masks"], syn.subsample_masks(c["counts"][4:], DEPTHS, R, SEED, c["depth"]))
    assert not same(tail["masks"], whole["masks"][-len(tail["masks"]):])


# ------------------------------------------------------------------------------------------------ 5: the handle is left as it was
def state(m):
    return m.describe(), m.verify_stats(), m.refine_stats(), m.range_status(), m.layer_precision()


def test_the_handle_is_left_as_it_was():
    c = case("c8_d89_indel")
    sd, rows, counts = c["sd"], c["rows"], c["counts"]
    kw = dict(depths=DEPTHS, replicates=R, seed=SEED, masks=True, variant_rows=True)
    x = syn.make_fa_windows(7, seed=9)
    used, fresh = make_fa(sd), make_fa(sd)
    for m in (used, fresh):
        m.predict_rows(rows, counts)  # (rows_windows= of the last call)
    y_before = used.predict_numpy(x)
    fresh.predict_numpy(x)
    before = state(used)
    r = used.subsample_rows(rows, counts, **kw)
    assert state(used) == before == state(fresh)
    assert same(used.predict_numpy(x), y_before) and same(y_before, fresh.predict_numpy(x)) and state(used) == state(fresh)
    tickets = [[m.submit(x[k:k + 3], slot=k) for k in range(3)] for m in (used, fresh)]
    # refused while a submit is pending on any slot, and nothing of the pending batches is disturbed
    with pytest.raises(_lib.C3Error, match="a prediction is in flight: call c3_predict_wait first"):
        used.subsample_rows(rows, counts)
    with pytest.raises(_lib.C3Error, match="in flight"):
        used.subsample(x)
    got = [[m.wait(t) for t in ts] for m, ts in zip((used, fresh), tickets)]
    assert all(same(a, b) for a, b in zip(*got)) and all(same(got[0][k], y_before[k:k + 3]) for k in range(3))
    again = used.subsample_rows(rows, counts, **kw)  # works after the wait, and gives what it gave
    assert same_call(again, r) and same_call(r, call(c, False, "recentre"))


# ------------------------------------------------------------------------------------------------ 6: the range guard
def test_range_guard_runs_the_pass_again_on_fp32_for_this_call_alone(monkeypatch, capfd):
    sd = recipe_state_dict()
    x = syn.make_fa_windows(3, seed=62)
    rows, _, counts = syn.pack_fa_rows(x)
    depths = (2, int(counts.min()) - 1)
    m, never = make_fa(sd), make_fa(sd)
    monkeypatch.setenv("C3HIP_FP32", "1")
    f32 = make_fa(sd)
    monkeypatch.delenv("C3HIP_FP32")
    before, precision = m.describe(), m.layer_precision()
    r = m.subsample_rows(rows, counts, depths=depths, replicates=2, seed=5, masks=True, variant_rows=True)
    assert r["on_fp32"], "the checkpoint's activations leave the range of the fp16x3 kernels"
    assert r["variants"] == 12 and same(r["masks"], syn.subsample_masks(counts, depths, 2, 5, 89))
    assert same(r["base_rows"], f32.predict_rows(rows, counts))
    assert same(r["variant_rows"], f32.predict_numpy(syn.subsample_variants(rows, counts, None, depths, 2, 5)))
    lev, win = syn.subsample_records(r["base_rows"], r["variant_rows"], counts, depths, 2, 90)
    assert same_records(r["levels"], lev) and same_records(r["rows"], win) and not lev["nonfinite"].any()
    assert m.range_status() == (0, False) and m.describe() == before and "precision=fp16x3" in before and m.layer_precision() == precision
    assert "continues on fp32" not in capfd.readouterr().err, "the handle stays on its forms and says nothing"
    # the handle's next ordinary batch trips its own guard exactly as on a handle that never ran the call
    y, y_never = m.predict_numpy(x), never.predict_numpy(x)
    assert same(y, y_never) and same(y, f32.predict_numpy(x))
    assert m.range_status() == never.range_status() and m.range_status()[1] and m.describe() == never.describe()
    assert not m.subsample_rows(rows, counts, depths=depths, replicates=2)["on_fp32"], "a handle that is on the fp32 forms has no guard to meet"


# ------------------------------------------------------------------------------------------------ 7: refusals that need the device
def test_refusals():
    c = case("c8_d89_indel")
    sd, rows, counts = c["sd"], c["rows"], c["counts"]
    L = _lib.lib()
    rec, lev = np.zeros(len(counts), syn.SUBSAMPLE_WINDOW_DTYPE), np.zeros((len(counts), 2), syn.SUBSAMPLE_LEVEL_DTYPE)
    depths = np.array([2, 4], np.int32)
    tail = (depths.ctypes.data, 2, 3, 0, 0, None, rec.ctypes.data, lev.ctypes.data, None, None, None)
    p = Clair3_P(add_indel_length=True, predict=True)
    p.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, True, seed=1))
    assert L.c3_subsample_rows(p._handle, rows.ctypes.data, None, counts.ctypes.data, len(counts), *tail) != 0 and "counts, not reads" in _lib.last_error()
    assert L.c3_subsample(p._handle, rows.ctypes.data, _lib.DTYPE_I8, 1, *tail) != 0 and "counts, not reads" in _lib.last_error()
    empty = Clair3_F(add_indel_length=True, predict=True).to("cuda:0")
    with pytest.raises(_lib.C3Error, match="no weights"):
        empty.subsample_rows(rows, counts)
    m = make_fa(sd)
    before = m.describe()
    bad = counts.copy()
    bad[2] = -1
    with pytest.raises(_lib.C3Error, match="window 2: negative row_count"):
        m.subsample_rows(rows, bad)
    with pytest.raises(_lib.C3Error, match="counts add up"):
        m.subsample_rows(rows[:-1], counts)
    firsts = np.zeros(len(counts), np.int32)
    firsts[3] = 89 - 16
    with pytest.raises(_lib.C3Error, match=r"window 3: rows \[73, 90\) reach beyond the depth"):
        m.subsample_rows(rows, counts, firsts)
    firsts[3] = -1
    with pytest.raises(_lib.C3Error, match="window 3: negative row_first"):
        m.subsample_rows(rows, counts, firsts)
    head = (m._handle, rows.ctypes.data, None, counts.ctypes.data, len(counts))
    for args, word in (((depths.ctypes.data, 2, 3, 0, 2), "unknown layout 2"), ((depths.ctypes.data, 0, 3, 0, 0), "0 levels"), ((depths.ctypes.data, 9, 3, 0, 0), "9 levels"),
                       ((depths[::-1].copy().ctypes.data, 2, 3, 0, 0), "strictly increasing"), ((depths.ctypes.data, 2, 33, 0, 0), "33 replicates"),
                       ((None, 2, 3, 0, 0), "null buffer: depths")):
        assert L.c3_subsample_rows(*head, *args, None, rec.ctypes.data, lev.ctypes.data, None, None, None) != 0 and word in _lib.last_error(), word
    assert L.c3_subsample_rows(*head, depths.ctypes.data, 2, 3, 0, 0, None, None, lev.ctypes.data, None, None, None) != 0 and "null buffer" in _lib.last_error()
    assert L.c3_subsample_rows(*head, depths.ctypes.data, 2, 3, 0, 0, None, rec.ctypes.data, None, None, None, None) != 0 and "null buffer" in _lib.last_error()
    with pytest.raises(_lib.C3Error, match="window shape"):
        m.subsample(np.zeros((1, 89, 33, 9), np.int8))
    none = m.subsample_rows(rows[:0], counts[:0], masks=True, variant_rows=True)
    assert len(none["rows"]) == 0 and none["passes"] == 0 and none["masks"].shape == (0, 2) and none["variant_rows"].shape == (0, 90)
    assert m.describe() == before
    # a handle that answers from the exact form
    m.exact(True)
    m.answer("exact")
    with pytest.raises(_lib.C3Error, match="answers from the exact form"):
        m.subsample_rows(rows, counts)
    m.answer("product")
    got = m.subsample_rows(rows, counts, depths=DEPTHS, replicates=R, seed=SEED)
    assert same_records(got["levels"], call(c, False, "recentre")["levels"]) and same_records(got["rows"], call(c, False, "recentre")["rows"])


# ------------------------------------------------------------------------------------------------ 8: the tool
def test_the_tool_prints_the_report_of_the_same_windows(tmp_path, capsys):
    import json
    import torch
    from clair3_amd import subsample
    c = case("c8_d89_indel")
    x = syn.pad_fa_rows(c["rows"], c["counts"])
    np.save(str(tmp_path / "x.npy"), x)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in c["sd"].items()}, str(tmp_path / "m.pt"))
    out = str(tmp_path / "lines.json")
    assert subsample.main(["--chkpnt_fn", str(tmp_path / "m.pt"), "--tensor_fn", str(tmp_path / "x.npy"), "--depths", "1,2,16,60", "--replicates", "3",
                           "--seed", str(SEED), "--layout", "in_place", "--top", "4", "--out", out]) == 0
    printed = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    want = subsample.report(handles(c, True)[0].subsample(x, depths=DEPTHS, replicates=R, seed=SEED, layout="in_place"), 90, DEPTHS, 4)
    assert printed == json.loads(json.dumps(want)) == [json.loads(line) for line in open(out)]
    assert printed[-1]["windows"] == 6 and printed[-1]["variants"] == int(syn.subsample_variant_counts(c["counts"], DEPTHS, R).sum())
    assert printed[-1]["windows_run"] == [int((c["counts"] > d).sum()) for d in DEPTHS] and printed[-1]["windows_run"][0] == 4 and sum(printed[-1]["hold_level_genotype"]) == 6
