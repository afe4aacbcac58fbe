"""Jackknife mode (c3_jackknife_rows, csrc/c3_jackknife.h), the part that needs no GPU: the numpy rule (synthetic.leave_one_out /
jackknife_records) against plain loops that walk rows and columns as the kernels do, its hand-made corners (shared with
tests/test_jackknife_gpu.py, which runs them through the device), the record against the header and the binding, the refusals that need no
device and the tool's argument errors.  (The host's table builder -- the pass cut, the order of the entries, src / first / skip -- is
exercised without a device by the stand-alone program tests/host/jackknife_host_check.cpp, built with -fsanitize=address,undefined as its
head says.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from clair3_amd import _lib, jackknife, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import util
from tests.test_abi import HEADER, declared_symbols

ENTRIES = ("c3_jackknife_rows", "c3_jackknife", "c3_jackknife_reduce")
JACKKNIFE_H = os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_jackknife.h")
VARIANTS_H = os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_variants.h")  # what the mode shares with subsample and occlusion mode
F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_drops(a, b):
    """drops: bitwise equal where they are numbers, a NaN where the other holds a NaN (the sign and payload of a NaN that a subtraction
    returns are the machine's, not the rule's; a record never holds one)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and same(np.where(np.isnan(a), F32(0), a), np.where(np.isnan(b), F32(0), b))


def same_records(a, b):
    """every field: integers equal, floats bitwise equal"""
    return a.dtype == b.dtype == syn.JACKKNIFE_DTYPE and all(same(a[name], b[name]) for name in syn.JACKKNIFE_DTYPE.names)


# ---- leave_one_out against a loop over windows, reads and rows ----
def loop_leave_one_out(rows, counts, firsts, depth, layout):
    out, at = [], 0
    for b, n in enumerate(counts):
        base_first = (depth - n) // 2 if firsts is None else firsts[b]
        for j in range(n):
            w = np.zeros((depth,) + rows.shape[1:], rows.dtype)
            first = base_first if layout == "in_place" else (depth - (n - 1)) // 2
            k = first
            for i in range(n):
                if i != j:
                    w[k] = rows[at + i]
                    k += 1
            out.append(w)
        at += n
    return np.stack(out) if out else np.zeros((0, depth) + rows.shape[1:], rows.dtype)


@pytest.mark.parametrize("depth,channels", [(89, 8), (89, 9), (55, 8)])
@pytest.mark.parametrize("layout", syn.JACKKNIFE_LAYOUTS)
def test_leave_one_out_against_a_loop(depth, channels, layout):
    rng = np.random.default_rng(depth * 10 + channels)
    counts = np.array([0, 1, 2, depth, 5, 0, 7], np.int64)
    rows = rng.integers(-100, 101, size=(int(counts.sum()), 33, channels)).astype(np.int8)
    rows[(rows == 0).all(axis=(1, 2))] = 1
    rows[int(counts[:4].sum()) + 2] = 0  # an interior all-zero row inside the run of five: a read like any other
    got = syn.leave_one_out(rows, counts, depth=depth, layout=layout)
    assert got.shape == (int(counts.sum()), depth, 33, channels) and got.dtype == np.int8
    assert same(got, loop_leave_one_out(rows, counts, None, depth, layout))
    # the variant of the single read is the all-zero window; the variant without the zero row still holds the other four
    assert not got[0].any() and (got[int(counts[:4].sum()) + 2] != 0).any(axis=(1, 2)).sum() == 4
    firsts = np.array([3, depth - 1, 0, 0, depth - 5, depth, 1], np.int64)  # explicit firsts, runs at both ends
    got = syn.leave_one_out(rows, counts, firsts, depth=depth, layout=layout)
    assert same(got, loop_leave_one_out(rows, counts, firsts, depth, layout))
    if layout == "in_place":  # the rows that stay start where the base run starts
        assert (got[1] != 0).any(axis=(1, 2)).nonzero()[0][0] == 0 and (got[int(counts[:4].sum())] != 0).any(axis=(1, 2)).nonzero()[0][0] == depth - 5
    with pytest.raises(ValueError):
        syn.leave_one_out(rows, counts, depth=depth, layout="centre")
    with pytest.raises(ValueError):
        syn.leave_one_out(rows[:-1], counts, depth=depth)


# ---- jackknife_records against a loop that walks the columns as jackknife_reduce_kernel does ----
def loop_argmax(v, lo, hi):
    best, at = -INF, lo
    for c in range(lo, hi):
        if v[c] > best:
            best, at = v[c], c
    return at


def loop_records(base, var, counts, nout, columns=None):
    has_cols = base.shape[1] > nout if columns is None else columns
    heads = syn.head_slices(nout)
    rec = np.zeros(len(base), syn.JACKKNIFE_DTYPE)
    drops = np.zeros((len(var), 4), F32)
    at = 0
    with np.errstate(invalid="ignore"):
        for b, n in enumerate(counts):
            y = base[b]
            t = [loop_argmax(y, lo, hi) for lo, hi in heads]
            best = [None] * len(heads)
            rec["reads"][b] = n
            rec["lean_read"][b] = -1
            delta = F32(0)
            for j in range(n):
                v = var[at + j]
                finite, d = True, F32(0)
                for c in range(nout):
                    finite &= bool(np.isfinite(v[c]))
                    a = np.abs(F32(v[c] - y[c]))
                    if a > d:
                        d = a
                rec["nonfinite"][b] += not finite
                if finite and d > delta:
                    delta = d
                for h, (lo, hi) in enumerate(heads):
                    rec["flips"][b, h] += loop_argmax(v, lo, hi) != t[h]
                    drop = F32(y[t[h]] - v[t[h]])
                    drops[at + j, h] = drop
                    if finite and drop == drop and (best[h] is None or drop > best[h][0]):
                        best[h] = (drop, j)
                if has_cols:
                    for k in range(4):
                        rec["decision_flips"][b, k] += bool(v[nout + 23 + k] != y[nout + 23 + k])
            for h in range(len(heads)):
                if best[h] is not None:
                    rec["lean_read"][b, h], rec["lean_drop"][b, h] = best[h][1], best[h][0] + F32(0)
            rec["max_delta"][b] = delta
            at += n
    return rec, drops


def random_rows(n, nout, columns, rng):
    """softmax-like rows per head, decoder columns (decisions 0 .. 9 in columns 23 .. 26) behind them where asked for"""
    y = np.zeros((n, nout + (syn.DECODE_COLS if columns else 0)), F32)
    for lo, hi in syn.head_slices(nout):
        e = np.exp(rng.normal(size=(n, hi - lo)) * 2).astype(F32)
        y[:, lo:hi] = e / e.sum(axis=1, keepdims=True)
    if columns:
        y[:, nout:nout + 23] = rng.random((n, 23)).astype(F32)
        y[:, nout + 23:nout + 27] = rng.integers(0, 3, size=(n, 4)).astype(F32)
    return y


def corner_rows(nout, columns):
    """Hand-made windows where flips, ties and NaNs are certain: (names, base rows, variant rows, counts).  One window per corner."""
    width = nout + (syn.DECODE_COLS if columns else 0)
    heads = syn.head_slices(nout)

    def row(tops=None, top=0.9, rest=0.001):
        r = np.full(width, rest, F32)
        for h, (lo, hi) in enumerate(heads):
            r[lo + (tops[h] if tops else 0)] = top
        if columns:
            r[nout:] = 0
            r[nout:nout + 9] = F32(0.05) * np.arange(1, 10, dtype=F32)  # class maxima far from each other and from homo_Ref's: no decoder tie
            r[nout + 9:nout + 13] = 0.9
            r[nout + 23:nout + 27] = (1, 2, 0, 5)
        return r

    names, base, var, counts = [], [], [], []

    def add(name, y, variants):
        names.append(name), base.append(y), var.extend(variants), counts.append(len(variants))

    zero = [0] * len(heads)
    # an exact tie in the base row: the arg-max is the lower index; a variant that keeps the tie does not flip, one that breaks it upward does
    y = row(zero, top=0.5)
    y[7] = 0.5
    up = y.copy()
    up[0], up[7] = 0.4, 0.6
    down = y.copy()
    down[0], down[7] = 0.6, 0.4
    add("base_tie", y, [y.copy(), up, down])
    # two reads with the same largest drop: the lowest j
    y = row(zero)
    v = [row(zero, top=t) for t in (0.8, 0.5, 0.5, 0.7)]
    add("drop_tie", y, v)
    # every drop negative: the largest is the least negative
    add("all_negative", row(zero, top=0.5), [row(zero, top=t) for t in (0.9, 0.6, 0.7)])
    # a NaN variant with what would be the largest drop is left out of lean_read and max_delta but counts in nonfinite (and flips by the rule)
    nan_v = row(zero, top=0.1)
    nan_v[heads[-1][0] + 1] = NAN
    add("nan_variant", row(zero), [row(zero, top=0.85), nan_v, row(zero, top=0.8)])
    inf_v = row([1] * len(heads))
    inf_v[1] = INF
    add("inf_variant", row(zero), [inf_v, row([1] * len(heads), top=0.7)])
    # all variants NaN: no lean read, max_delta 0
    allnan = np.full(width, NAN, F32)
    add("all_nan", row([2] * len(heads)), [allnan.copy(), allnan.copy()])
    add("no_reads", row(zero), [])
    # a variant equal to the base: drop +0, no flip, delta 0 -- and -0 against +0 is a tie (the lower j leans)
    add("equal_to_base", row(zero), [row(zero)])
    y = row(zero, top=0.0, rest=-1.0)
    neg0 = y.copy()
    y[[lo for lo, _ in heads]] = F32(-0.0)
    add("zero_drops", y, [neg0, y.copy()])
    # a NaN base row: no drop is a number
    add("nan_base", allnan.copy(), [row(zero), row([1] * len(heads))])
    # flips in every head but the first, and a different decoder decision for reference bases A and T
    fl = row([0] + [2] * (len(heads) - 1), top=0.6)
    if columns:
        fl[nout + 23], fl[nout + 26] = 0, 9
    add("flips", row(zero), [fl, row(zero, top=0.95), fl.copy()])
    # more variants than lanes: the largest drop sits at j = 70, a flip at j = 64
    many = [row(zero, top=F32(0.9) - F32(0.001) * F32(j % 7)) for j in range(80)]
    many[70] = row(zero, top=0.2)
    many[64] = row([1] * len(heads), top=0.9)
    many[64][[lo for lo, _ in heads]] = 0.85
    add("many_reads", row(zero), many)
    return names, np.stack(base), np.stack(var), np.array(counts, np.int32)


@pytest.mark.parametrize("nout", [90, 24])
@pytest.mark.parametrize("columns", [False, True])
def test_records_against_a_loop(nout, columns):
    rng = np.random.default_rng(nout + columns)
    counts = np.array([5, 0, 1, 89, 17, 2], np.int32)
    base, var = random_rows(len(counts), nout, columns, rng), random_rows(int(counts.sum()), nout, columns, rng)
    var[10:60] = base[3] + (var[10:60] - base[3]) * F32(0.01)  # variants close to their base row, as real ones are
    rec, drops = syn.jackknife_records(base, var, counts, nout)
    lrec, ldrops = loop_records(base, var, counts, nout)
    assert same_records(rec, lrec) and same(drops, ldrops)
    assert rec["flips"].sum() > 0 and (rec["lean_read"][1] == -1).all() and rec["reads"][1] == 0 and rec[1]["max_delta"] == 0
    if columns:
        assert rec["decision_flips"].sum() > 0
        ignored, _ = syn.jackknife_records(base, var, counts, nout, columns=False)
        assert not ignored["decision_flips"].any() and same(ignored["flips"], rec["flips"])
    else:
        assert not rec["decision_flips"].any()
    if nout == 24:
        assert not rec["flips"][:, 2:].any() and (rec["lean_read"][:, 2:] == -1).all() and not drops[:, 2:].any()
    with pytest.raises(ValueError):
        syn.jackknife_records(base, var[:-1], counts, nout)
    with pytest.raises(ValueError):
        syn.jackknife_records(base[:, :-1], var[:, :-1], counts, nout)


@pytest.mark.parametrize("nout", [90, 24])
@pytest.mark.parametrize("columns", [False, True])
def test_records_of_the_hand_made_corners(nout, columns):
    names, base, var, counts = corner_rows(nout, columns)
    rec, drops = syn.jackknife_records(base, var, counts, nout)
    lrec, ldrops = loop_records(base, var, counts, nout)
    assert same_records(rec, lrec) and same(drops, ldrops)
    at = {n: i for i, n in enumerate(names)}
    heads = len(syn.head_slices(nout))
    r = rec[at["base_tie"]]
    assert r["flips"][0] == 1 and r["lean_read"][0] == 1 and r["lean_drop"][0] == F32(0.5) - F32(0.4)
    r = rec[at["drop_tie"]]
    assert (r["lean_read"][:heads] == 1).all() and (r["lean_drop"][:heads] == F32(0.9) - F32(0.5)).all() and not r["flips"].any()
    r = rec[at["all_negative"]]
    assert (r["lean_read"][:heads] == 1).all() and (r["lean_drop"][:heads] == F32(0.5) - F32(0.6)).all() and (r["lean_drop"][:heads] < 0).all()
    r = rec[at["nan_variant"]]
    assert r["nonfinite"] == 1 and (r["lean_read"][:heads] == 2).all() and r["max_delta"] == F32(0.9) - F32(0.8)
    r = rec[at["inf_variant"]]
    assert r["nonfinite"] == 1 and (r["lean_read"][:heads] == 1).all() and (r["flips"][:heads] == 2).all()
    r = rec[at["all_nan"]]
    assert r["nonfinite"] == 2 and (r["lean_read"] == -1).all() and not r["lean_drop"].any() and r["max_delta"] == 0 and (r["flips"][:heads] == 2).all()
    r = rec[at["no_reads"]]
    assert r["reads"] == 0 and r["nonfinite"] == 0 and (r["lean_read"] == -1).all() and not r["decision_flips"].any()
    assert not r["flips"].any() and not r["lean_drop"].any() and r["max_delta"] == 0
    r = rec[at["equal_to_base"]]
    assert (r["lean_read"][:heads] == 0).all() and same(r["lean_drop"], np.zeros(4, F32)) and r["max_delta"] == 0 and not r["flips"].any()
    r = rec[at["zero_drops"]]
    assert (r["lean_read"][:heads] == 0).all() and same(r["lean_drop"], np.zeros(4, F32)), "-0 and +0 are a tie and reported as +0"
    r = rec[at["nan_base"]]
    assert r["nonfinite"] == 0 and (r["lean_read"] == -1).all() and r["max_delta"] == 0
    r = rec[at["flips"]]
    assert r["flips"][0] == 0 and (r["flips"][1:heads] == 2).all()
    assert list(r["decision_flips"]) == ([2, 0, 0, 2] if columns else [0, 0, 0, 0])
    r = rec[at["many_reads"]]
    assert r["reads"] == 80 and (r["lean_read"][:heads] == 70).all() and (r["flips"][:heads] == 1).all()
    if nout == 24:
        assert (rec["lean_read"][:, 2:] == -1).all() and not rec["flips"][:, 2:].any()


# ---- the header, the binding and the numpy dtype are one record ----
def test_record_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct c3_jackknife_window \{([^}]*)\} c3_jackknife_window;", src).group(1)
    ctypes_of = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "int64_t": ctypes.c_int64}

    def fields(body):
        want = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            ctype, names = decl.split(None, 1)
            for name in names.split(","):
                m = re.fullmatch(r"(\w+)((?:\[\d+\])*)", name.strip())
                t = ctypes_of[ctype]
                for dim in reversed(re.findall(r"\[(\d+)\]", m.group(2))):
                    t = t * int(dim)
                want.append((m.group(1), t))
        return want

    assert list(_lib.JackknifeWindow._fields_) == fields(body)
    assert ctypes.sizeof(_lib.JackknifeWindow) == 80 == syn.JACKKNIFE_DTYPE.itemsize
    for name, _ in _lib.JackknifeWindow._fields_:
        assert getattr(_lib.JackknifeWindow, name).offset == syn.JACKKNIFE_DTYPE.fields[name][1], name
    assert [_lib.JackknifeWindow.flips.offset, _lib.JackknifeWindow.lean_read.offset, _lib.JackknifeWindow.lean_drop.offset,
            _lib.JackknifeWindow.max_delta.offset] == [8, 40, 56, 72]
    info = re.search(r"typedef struct \{([^}]*)\} c3_jackknife_info;", src).group(1)
    assert list(_lib.JackknifeInfo._fields_) == fields(info) and ctypes.sizeof(_lib.JackknifeInfo) == 48
    for name, value in (("C3_JACKKNIFE_RECENTRE", 0), ("C3_JACKKNIFE_IN_PLACE", 1)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == value
    assert _lib.JACKKNIFE_LAYOUT == {"recentre": 0, "in_place": 1} and syn.JACKKNIFE_LAYOUTS == ("recentre", "in_place")


def test_definitions_of_the_kernel_header():
    src = open(JACKKNIFE_H).read()
    assert 'section(".c3_jackknife_text")' in src and src.count("C3_JACKKNIFE_TEXT void") == 2, "both kernels of the mode in their own section"
    assert "h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57" in src, "the heads of syn.head_slices"
    assert "p.nout + 23 + k" in src, "the decoder's first decision per reference base"
    assert "(depth - (n - 1)) / 2" in src and "C3_JACKKNIFE_IN_PLACE ? f" in src, "the two layouts"
    assert "static_assert(sizeof(JackknifeEntry) == 24" in src and 'variant_chunk_env("C3HIP_JACKKNIFE_CHUNK", 64)' in src
    assert "e ? atoll(e) : dflt" in open(VARIANTS_H).read(), "the switch is read in one place, with the mode's default"
    for word in ("a NaN never", "lowest j on ties", "an interior all-zero row of the run is a read too", "left out", "atomic"):
        assert word in src, word
    assert "atomicAdd" not in src and "atomicMax" not in src and "hipMemset(" not in src


def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    comment = src[src.index("/* ---- jackknife mode"):src.index("int c3_jackknife_rows(")]
    for word in ("DESIGN.md 4", "c3_jackknife.h", "Refused before anything is queued", "C3HIP_JACKKNIFE_CHUNK", "on_fp32", "bit for bit c3_predict_rows",
                 "a NaN"):
        assert word in comment, word


# ---- refusals that need no device ----
def test_null_handle_and_no_device_errors():
    L = _lib.lib()
    rec, cnt = _lib.JackknifeWindow(), (ctypes.c_int32 * 1)(1)
    assert L.c3_jackknife_rows(None, None, None, cnt, 1, 0, None, ctypes.byref(rec), None, None, None) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_jackknife(None, None, _lib.DTYPE_I8, 1, 0, None, ctypes.byref(rec), None, None, None) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_jackknife_reduce(None, None, None, 90, cnt, 1, ctypes.byref(rec), None) != 0 and b"null model" in L.c3_last_error()
    rows, counts = np.zeros((2, 33, 8), np.int8), np.array([2], np.int32)
    f = Clair3_F(add_indel_length=True, predict=True)
    for call in (lambda: f.jackknife_rows(rows, counts), lambda: f.jackknife(np.zeros((1, 89, 33, 8), np.int8)),
                 lambda: f.jackknife_reduce(np.zeros((1, 90), F32), np.zeros((2, 90), F32), counts)):
        with pytest.raises(_lib.C3Error, match="no device"):
            call()
    with pytest.raises(_lib.C3Error, match="no device"):
        Clair3_P(add_indel_length=True, predict=True).jackknife_reduce(np.zeros((1, 90), F32), np.zeros((2, 90), F32), counts)
    for call in (lambda: f.jackknife_rows(rows, counts, layout="centre"), lambda: f.jackknife(np.zeros((1, 89, 33, 8), np.int8), layout=1)):
        with pytest.raises(_lib.C3Error, match="layout must be"):
            call()
    assert not hasattr(Clair3_P, "jackknife") and not hasattr(Clair3_P, "jackknife_rows"), "the pileup network's windows are counts, not reads"


# ---- the tool ----
def test_the_tool_refuses_bad_arguments_before_any_device_call(monkeypatch):
    from clair3_amd import predict
    monkeypatch.setattr(predict, "build_model", lambda *a, **k: pytest.fail("a device call before the arguments were checked"))
    base = ["--chkpnt_fn", "m.pt", "--tensor_fn", "x.npy"]
    for extra, match in ((["--layout", "centre"], "--layout"), (["--gap", "-1"], "--gap"), (["--gap", "nan"], "--gap"), (["--gap", "inf"], "--gap"),
                         (["--top", "-1"], "--top"), (["--max_windows", "0"], "--max_windows")):
        with pytest.raises(_lib.C3Error, match=match):
            jackknife.main(base + extra)
    with pytest.raises(SystemExit):
        jackknife.parse_args(["--tensor_fn", "x.npy"])
    args = jackknife.parse_args(base)
    assert args.layout == "recentre" and args.gap == 1e-4 and args.top == 20


def test_the_report_of_the_tool():
    nout = 90
    names, base, var, counts = corner_rows(nout, True)
    rec, _ = syn.jackknife_records(base, var, counts, nout)
    lines = jackknife.report(dict(rows=rec, base_rows=base, counts=counts), nout, gap=1e-4, top=3)
    total, listed = lines[-1], lines[:-1]
    assert len(listed) == 3 and all(rec["flips"][line["window"]].any() or rec["decision_flips"][line["window"]].any() for line in listed)
    # most flips first: the all-NaN variants (8 head flips + 8 decision flips), then the NaN base row (4 + 8), then "flips" (6 + 4)
    assert [line["window"] for line in listed] == [names.index(n) for n in ("all_nan", "nan_base", "flips")]
    assert listed[0]["flips"] == [2, 2, 2, 2] and listed[0]["reads"] == 2 and listed[2]["decision_flips"] == [2, 0, 0, 2] and listed[1]["lean_read"] == [-1] * 4
    flips = (rec["flips"] > 0).any(axis=1) | (rec["decision_flips"] > 0).any(axis=1)
    near = np.zeros(len(rec), bool)
    near[syn.refine_select(base, nout, 1e-4)[0]] = True
    assert near[names.index("base_tie")] and not near[names.index("flips")]
    assert total["windows"] == len(rec) and total["variants"] == int(counts.sum()) and total["windows_head_flip"] == int((rec["flips"] > 0).any(axis=1).sum())
    assert total["near_tie_table"] == [[int((~near & ~flips).sum()), int((~near & flips).sum())], [int((near & ~flips).sum()), int((near & flips).sum())]]
    assert sum(map(sum, total["near_tie_table"])) == len(rec) and total["nonfinite"] == int(rec["nonfinite"].sum())
    assert len(jackknife.report(dict(rows=rec, base_rows=base, counts=counts), nout, top=0)) == 1
