"""Occlusion mode (c3_occlude, csrc/c3_occlude.h), the part that needs no GPU: the numpy rule (synthetic.occlude_variants /
occlude_records) against plain loops that walk windows, reads, positions and channels -- and rows and columns as the kernels do --, its
hand-made corners (shared with tests/test_occlude_gpu.py, which runs them through the device), the record against the header and the
binding, the refusals that need no device, the tool's argument errors and its report.  (The host's plan -- the pass cut, the layout, the
table of every pass -- is exercised without a device by the stand-alone program tests/host/occlude_host_check.cpp, built with
-fsanitize=address,undefined as its head says.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from clair3_amd import _lib, occlude, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import util
from tests.test_abi import HEADER, declared_symbols
from tests.test_jackknife import corner_rows as jackknife_corner_rows, loop_argmax, random_rows, same, same_drops

ENTRIES = ("c3_occlude", "c3_occlude_rows", "c3_occlude_reduce")
OCCLUDE_H = os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_occlude.h")
F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
WHATS = ("channels", "bands", "both")


def same_records(a, b):
    """every field: integers equal, floats bitwise equal"""
    return a.dtype == b.dtype == syn.OCCLUDE_DTYPE and all(same(a[name], b[name]) for name in syn.OCCLUDE_DTYPE.names)


# ---- occlude_variants against a loop over windows, reads, positions and channels ----
def loop_variants(x, what, band):
    """x (B, R, P, C) -- R reads, 1 for a pileup window"""
    B, R, P, C = x.shape
    out = []
    for b in range(B):
        masks = []
        if what in ("channels", "both"):
            masks += [("c", c) for c in range(C)]
        if what in ("bands", "both"):
            masks += [("b", k) for k in range(-(-P // band))]
        for kind, k in masks:
            w = np.zeros((R, P, C), x.dtype)
            for r in range(R):
                for p in range(P):
                    for c in range(C):
                        gone = c == k if kind == "c" else k * band <= p < min(P, (k + 1) * band)
                        w[r, p, c] = 0 if gone else x[b, r, p, c]
            out.append(w)
    return np.stack(out)


@pytest.mark.parametrize("P,C", [(33, 8), (33, 9), (33, 18), (5, 3)])
@pytest.mark.parametrize("what", WHATS)
def test_variants_against_a_loop(P, C, what):
    rng = np.random.default_rng(P * 100 + C)
    fa = rng.integers(1, 101, size=(3, 4, P, C)).astype(np.int8)  # no zero anywhere: what is zero in a variant was set to zero
    fa[1, :, :, 2] = 0  # a channel that is already zero
    fa[2] = 0           # the zero window
    pile = rng.integers(1, 300, size=(2, P, C)).astype(np.int32)
    for band in sorted({1, 2, 5, P}):
        nc, nb = syn.occlude_groups(P, C, what, band)
        K = nc + nb
        assert (nc, nb) == (C if what != "bands" else 0, -(-P // band) if what != "channels" else 0)
        got = syn.occlude_variants(fa, what, band)
        assert got.shape == (3 * K, 4, P, C) and got.dtype == np.int8 and same(got, loop_variants(fa, what, band))
        gp = syn.occlude_variants(pile, what, band)
        assert gp.shape == (2 * K, P, C) and gp.dtype == np.int32 and same(gp, loop_variants(pile[:, None], what, band)[:, 0])
        v = got.reshape(3, K, 4, P, C)
        assert not v[2].any(), "every variant of the zero window is the zero window"
        if nc:
            assert same(v[1, 2], fa[1]), "a channel that is already zero gives a variant equal to the window"
            assert not v[0, 1, :, :, 1].any() and (np.delete(v[0, 1], 1, axis=2) != 0).all()
        if nb:
            last = v[0, K - 1]  # the ragged last band: 33 = 6 * 5 + 3
            first_col = (nb - 1) * band
            assert not last[:, first_col:].any() and (last[:, :first_col] != 0).all() and P - first_col == (P - 1) % band + 1
            if band == P:
                assert nb == 1 and not v[0, K - 1].any(), "band = P: the one band variant is the zero window"
    for bad in (0, P + 1, -1, 1.5, True):
        with pytest.raises(ValueError):
            syn.occlude_variants(fa, what, bad)
    with pytest.raises(ValueError):
        syn.occlude_variants(fa, "columns", 1)
    with pytest.raises(ValueError):
        syn.occlude_variants(np.zeros((P, C), np.int8))


# ---- occlude_records against a loop that walks the columns as occlude_reduce_kernel does ----
def loop_records(base, var, channels, bands, nout):
    K = channels + bands
    has_cols = base.shape[1] > nout
    heads = syn.head_slices(nout)
    rec = np.zeros(len(base), syn.OCCLUDE_DTYPE)
    drops = np.zeros((len(base), K, 4), F32)
    with np.errstate(invalid="ignore"):
        for b in range(len(base)):
            y = base[b]
            t = [loop_argmax(y, lo, hi) for lo, hi in heads]
            best = [[None] * len(heads) for _ in range(2)]
            rec["variants"][b] = K
            rec["lean"][b] = -1
            delta = F32(0)
            for j in range(K):
                g, idx = (0, j) if j < channels else (1, j - channels)
                v = var[b * K + j]
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
                    rec["flips"][b, g, h] += loop_argmax(v, lo, hi) != t[h]
                    drop = F32(y[t[h]] - v[t[h]])
                    drops[b, j, h] = drop
                    if finite and drop == drop and (best[g][h] is None or drop > best[g][h][0]):
                        best[g][h] = (drop, idx)
                if has_cols:
                    for r in range(4):
                        rec["decision_flips"][b, g, r] += bool(v[nout + 23 + r] != y[nout + 23 + r])
            for g in range(2):
                for h in range(len(heads)):
                    if best[g][h] is not None:
                        rec["lean"][b, g, h], rec["lean_drop"][b, g, h] = best[g][h][1], best[g][h][0] + F32(0)
            rec["max_delta"][b] = delta
    return rec, drops


def corner_rows(nout, columns, channels, bands):
    """Hand-made windows where flips, ties and NaNs are certain, every window with channels + bands variants: (names, base rows, variant
    rows).  The corners are those of tests/test_jackknife.py corner_rows -- ties, -0 against +0, negative drops, a NaN and an infinity in a
    variant, a NaN base row --, every window's variants dealt out over the K members round robin, so that they fall into both groups, and
    from the second round on moved towards the base row by a power of two, so that the first occurrence holds the largest drop."""
    names, base, var, counts = jackknife_corner_rows(nout, columns)
    K = channels + bands
    keep = [i for i, n in enumerate(counts) if 0 < n <= max(K, 1)]
    at = np.r_[0, np.cumsum(counts)]
    out = []
    for i in keep:
        mine = var[at[i]:at[i + 1]]
        for j in range(K):
            v = mine[j % len(mine)].copy()
            if j >= len(mine) and np.isfinite(v).all() and np.isfinite(base[i]).all():
                v[:nout] = base[i, :nout] + (v[:nout] - base[i, :nout]) * F32(0.5)
            out.append(v)
    width = base.shape[1]
    return [names[i] for i in keep], base[keep], np.stack(out) if out else np.zeros((0, width), F32)


@pytest.mark.parametrize("nout", [90, 24])
@pytest.mark.parametrize("columns", [False, True])
def test_records_against_a_loop(nout, columns):
    rng = np.random.default_rng(nout + columns)
    for channels, bands in ((8, 33), (18, 7), (0, 33), (9, 0), (70, 3), (0, 0)):
        K, B = channels + bands, 4
        base, var = random_rows(B, nout, columns, rng), random_rows(B * K, nout, columns, rng)
        if K:
            var[K:2 * K] = base[1] + (var[K:2 * K] - base[1]) * F32(0.01)  # variants close to their base row, as real ones are
        rec, drops = syn.occlude_records(base, var, channels, bands, nout)
        lrec, ldrops = loop_records(base, var, channels, bands, nout)
        assert same_records(rec, lrec) and same(drops, ldrops) and drops.shape == (B, K, 4)
        assert (rec["variants"] == K).all()
        if not channels:  # a group that was not asked for
            assert not rec["flips"][:, 0].any() and (rec["lean"][:, 0] == -1).all() and not rec["lean_drop"][:, 0].any() and not rec["decision_flips"][:, 0].any()
        if not bands:
            assert not rec["flips"][:, 1].any() and (rec["lean"][:, 1] == -1).all() and not rec["lean_drop"][:, 1].any()
        if K:
            assert rec["flips"].sum() > 0 and rec["max_delta"].min() > 0
            assert bool(rec["decision_flips"].any()) == columns
        if channels:
            assert (rec["lean"][:, 0, :2] >= 0).all() and (rec["lean"][:, 0] < channels).all()
        if bands:
            assert (rec["lean"][:, 1, :2] >= 0).all() and (rec["lean"][:, 1] < bands).all()
        if nout == 24:
            assert not rec["flips"][:, :, 2:].any() and (rec["lean"][:, :, 2:] == -1).all() and not drops[:, :, 2:].any()
    with pytest.raises(ValueError):
        syn.occlude_records(base, var[:-1] if len(var) else np.zeros((1, base.shape[1]), F32), 9, 0, nout)
    with pytest.raises(ValueError):
        syn.occlude_records(base[:, :-1], var[:, :-1], 0, 0, nout)
    with pytest.raises(ValueError):
        syn.occlude_records(base, var, -1, 1, nout)


@pytest.mark.parametrize("nout", [90, 24])
@pytest.mark.parametrize("columns", [False, True])
@pytest.mark.parametrize("channels,bands", [(3, 2), (0, 4), (4, 0)])
def test_records_of_the_hand_made_corners(nout, columns, channels, bands):
    names, base, var = corner_rows(nout, columns, channels, bands)
    K = channels + bands
    assert {"base_tie", "drop_tie", "all_negative", "nan_variant", "inf_variant", "all_nan", "zero_drops", "nan_base", "flips"} <= set(names)
    rec, drops = syn.occlude_records(base, var, channels, bands, nout)
    lrec, ldrops = loop_records(base, var, channels, bands, nout)
    assert same_records(rec, lrec) and same_drops(drops, ldrops) and np.isnan(drops).any()
    at = {n: i for i, n in enumerate(names)}
    heads = len(syn.head_slices(nout))
    groups = [g for g, n in enumerate((channels, bands)) if n]
    off = [0, channels]
    for g in range(2):
        if g not in groups:
            assert not rec["flips"][:, g].any() and (rec["lean"][:, g] == -1).all() and not rec["lean_drop"][:, g].any() and not rec["decision_flips"][:, g].any()
    # member j of the window holds the corner's variant j % n: which member of a group is the first to hold variant `k` of a corner with n
    # variants
    def first_in(g, n, k):
        size = (channels, bands)[g]
        hits = [i for i in range(size) if (off[g] + i) % n == k]
        return hits[0] if hits else None

    r = rec[at["drop_tie"]]  # variants 1 and 2 of 4 share the largest drop: the lowest index of the group that holds either
    for g in groups:
        want = min(i for i in (first_in(g, 4, 1), first_in(g, 4, 2)) if i is not None) if any(first_in(g, 4, k) is not None for k in (1, 2)) else None
        if want is not None and K <= 4:
            assert (r["lean"][g, :heads] == want).all() and (r["lean_drop"][g, :heads] == F32(0.9) - F32(0.5)).all()
    assert not r["flips"].any()
    r = rec[at["all_negative"]]
    for g in groups:
        assert (r["lean_drop"][g, :heads] < 0).all() and (r["lean"][g, :heads] >= 0).all(), "every drop negative: the largest is the least negative"
    r = rec[at["nan_variant"]]
    assert r["nonfinite"] == sum(1 for j in range(K) if j % 3 == 1) and r["max_delta"] == F32(0.9) - F32(0.8)
    for g in groups:
        assert all(((off[g] + int(i)) % 3) != 1 for i in r["lean"][g, :heads]), "a non-finite variant never leans"
    r = rec[at["all_nan"]]
    assert r["nonfinite"] == K and (r["lean"] == -1).all() and not r["lean_drop"].any() and r["max_delta"] == 0
    assert r["flips"][:, :heads].sum() == K * heads
    r = rec[at["zero_drops"]]  # -0 and +0 are a tie and reported as +0: the first member of every group
    for g in groups:
        assert (r["lean"][g, :heads] == 0).all() and same(r["lean_drop"][g], np.zeros(4, F32))
    r = rec[at["nan_base"]]
    assert r["nonfinite"] == 0 and (r["lean"] == -1).all() and r["max_delta"] == 0
    r = rec[at["flips"]]
    assert r["flips"][:, 0].sum() == 0 and r["flips"][:, 1:heads].sum() > 0
    assert bool(r["decision_flips"].any()) == columns
    if nout == 24:
        assert (rec["lean"][:, :, 2:] == -1).all() and not rec["flips"][:, :, 2:].any()


# ---- the header, the binding and the numpy dtype are one record ----
def test_record_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct c3_occlude_window \{([^}]*)\} c3_occlude_window;", src).group(1)
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

    assert list(_lib.OccludeWindow._fields_) == fields(body)
    assert [n for n, _ in fields(body)] == ["variants", "nonfinite", "flips", "decision_flips", "lean", "lean_drop", "max_delta", "reserved"]
    assert ctypes.sizeof(_lib.OccludeWindow) == 144 == syn.OCCLUDE_DTYPE.itemsize
    for name, _ in _lib.OccludeWindow._fields_:
        assert getattr(_lib.OccludeWindow, name).offset == syn.OCCLUDE_DTYPE.fields[name][1], name
    assert [getattr(_lib.OccludeWindow, n).offset for n in ("variants", "nonfinite", "flips", "decision_flips", "lean", "lean_drop", "max_delta", "reserved")] \
        == [0, 4, 8, 40, 72, 104, 136, 140]
    assert syn.OCCLUDE_DTYPE["flips"].shape == (2, 4) and syn.OCCLUDE_DTYPE["lean_drop"].base == np.dtype("<f4")
    info = re.search(r"typedef struct \{([^}]*)\} c3_occlude_info;", src).group(1)
    assert list(_lib.OccludeInfo._fields_) == fields(info) and ctypes.sizeof(_lib.OccludeInfo) == 48
    for name, value in (("C3_OCCLUDE_CHANNELS", 1), ("C3_OCCLUDE_BANDS", 2)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == value
    assert _lib.OCCLUDE_WHAT == {"channels": 1, "bands": 2, "both": 3} == syn.OCCLUDE_WHAT


def test_definitions_of_the_kernel_header():
    src = open(OCCLUDE_H).read()
    assert 'section(".c3_occlude_text")' in src and src.count("C3_OCCLUDE_TEXT void") == 3, "every kernel of the mode in its own section"
    assert "behind `.c3_subsample_text`" in src
    assert "h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57" in src, "the heads of syn.head_slices"
    assert "p.nout + 23 + r" in src, "the decoder's first decision per reference base"
    assert "fa && m->C == 8" in src, "the cell form is chosen on C == 8, not on row_bytes % 8"
    assert "static_assert(sizeof(OccludeEntry) == 32" in src and "static_assert(sizeof(c3_occlude_window) == 144" in src
    assert "C3_KIND_PILEUP ? 256 : 64" in src and "C3HIP_OCCLUDE_CHUNK" in src
    assert "jackknife_key(drop)" in src and "jackknife_unkey(" in src
    for word in ("a NaN never", "lowest index on ties", "still has K variants", "left", "atomic", "nb = ceil(P / band)"):
        assert word in src, word
    assert "atomicAdd" not in src and "atomicMax" not in src and "hipMemset(" not in src
    model_hip = open(os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_model.hip")).read()
    assert model_hip.index('#include "c3_subsample.h"') < model_hip.index('#include "c3_occlude.h"')


def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    comment = src[src.index("/* ---- occlusion mode"):src.index("int c3_occlude(")]
    for word in ("DESIGN.md 4", "c3_occlude.h", "Refused before anything is queued", "C3HIP_OCCLUDE_CHUNK", "on_fp32", "bit for bit c3_predict",
                 "a NaN", "nb = ceil(P / band)", "b * K .. b * K + K - 1"):
        assert word in comment, word
    L = _lib.lib()
    assert len(L.c3_occlude.argtypes) == 11 and len(L.c3_occlude_rows.argtypes) == 12 and len(L.c3_occlude_reduce.argtypes) == 9
    assert L.c3_occlude.argtypes[3] is ctypes.c_int64 and L.c3_occlude_rows.argtypes[4] is ctypes.c_int64 and L.c3_occlude_reduce.argtypes[6] is ctypes.c_int64
    assert L.c3_occlude.argtypes[-1] is L.c3_occlude_rows.argtypes[-1] and L.c3_occlude.argtypes[-1]._type_ is _lib.OccludeInfo


# ---- refusals that need no device ----
def test_null_handle_and_no_device_errors():
    L = _lib.lib()
    rec, cnt = _lib.OccludeWindow(), (ctypes.c_int32 * 1)(1)
    assert L.c3_occlude(None, None, _lib.DTYPE_I8, 1, 3, 1, None, ctypes.byref(rec), None, None, None) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_occlude_rows(None, None, None, cnt, 1, 3, 1, None, ctypes.byref(rec), None, None, None) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_occlude_reduce(None, None, None, 90, 8, 33, 1, ctypes.byref(rec), None) != 0 and b"null model" in L.c3_last_error()
    rows, counts = np.zeros((2, 33, 8), np.int8), np.array([2], np.int32)
    f, p = Clair3_F(add_indel_length=True, predict=True), Clair3_P(add_indel_length=True, predict=True)
    for call in (lambda: f.occlude_rows(rows, counts), lambda: f.occlude(np.zeros((1, 89, 33, 8), np.int8)), lambda: p.occlude(np.zeros((1, 33, 18), np.int8)),
                 lambda: f.occlude_reduce(np.zeros((1, 90), F32), np.zeros((41, 90), F32), 8, 33),
                 lambda: p.occlude_reduce(np.zeros((1, 90), F32), np.zeros((51, 90), F32), 18, 33)):
        with pytest.raises(_lib.C3Error, match="no device"):
            call()
    for call in (lambda: f.occlude_rows(rows, counts, what="columns"), lambda: p.occlude(np.zeros((1, 33, 18), np.int8), what=3)):
        with pytest.raises(_lib.C3Error, match="what must be"):
            call()
    for band in (0, 34, -1, 2.0, True):
        with pytest.raises(_lib.C3Error, match="band must be"):
            f.occlude(np.zeros((1, 89, 33, 8), np.int8), band=band)
        with pytest.raises(_lib.C3Error, match="band must be"):
            p.occlude(np.zeros((1, 33, 18), np.int8), band=band)
    assert not hasattr(Clair3_P, "occlude_rows"), "occupied rows are full-alignment input"


# ---- the tool ----
def test_the_tool_refuses_bad_arguments_before_any_device_call(monkeypatch):
    from clair3_amd import predict
    monkeypatch.setattr(predict, "build_model", lambda *a, **k: pytest.fail("a device call before the arguments were checked"))
    base = ["--chkpnt_fn", "m.pt", "--tensor_fn", "x.npy"]
    for extra, match in ((["--what", "columns"], "--what"), (["--band", "0"], "--band"), (["--band", "34"], "--band"), (["--head", "4"], "--head"),
                         (["--head", "-1"], "--head"), (["--max_windows", "0"], "--max_windows")):
        with pytest.raises(_lib.C3Error, match=match):
            occlude.main(base + extra)
    with pytest.raises(SystemExit):
        occlude.parse_args(["--tensor_fn", "x.npy"])
    with pytest.raises(SystemExit):
        occlude.parse_args(base + ["--band", "two"])
    args = occlude.parse_args(base)
    assert args.what == "both" and args.band == 1 and args.head == 0 and not args.pileup


def test_the_report_of_the_tool():
    nout, channels, bands, band = 90, 3, 2, 20
    names, base, var = corner_rows(nout, True, channels, bands)
    rec, drops = syn.occlude_records(base, var, channels, bands, nout)
    result = dict(rows=rec, base_rows=base, drops=drops, variant_rows=var, channels=channels, bands=bands, band=band)
    for head in range(4):
        lines = occlude.report(result, nout, head)
        total, members = lines[-1], lines[:-1]
        assert [m.get("channel") for m in members[:channels]] == [0, 1, 2] and [m.get("band") for m in members[channels:]] == [0, 1]
        assert [m["columns"] for m in members[channels:]] == [[0, 20], [20, 33]]
        for j, m in enumerate(members):
            g, k = (0, j) if j < channels else (1, j - channels)
            d = drops[:, j, head]
            d = d[~np.isnan(d)].astype(np.float64)
            assert m["mean_drop"] == float(d.mean()) and m["max_drop"] == float(d.max()) and m["lean"] == int((rec["lean"][:, g, head] == k).sum())
        for g, sl in ((0, slice(0, channels)), (1, slice(channels, None))):
            assert sum(m["flips"] for m in members[sl]) == int(rec["flips"][:, g, head].sum()), "the members' flips add up to the records'"
        assert total["windows"] == len(rec) and total["variants"] == len(var) and total["head"] == head and total["band"] == band
        assert total["windows_head_flip"] == [int((rec["flips"][:, g, head] > 0).sum()) for g in range(2)]
        assert total["nonfinite"] == int(rec["nonfinite"].sum()) and total["channels"] == channels and total["bands"] == bands
    without = occlude.report({k: v for k, v in result.items() if k != "variant_rows"}, nout, 0)
    assert all("flips" not in m for m in without[:-1]) and without[-1] == occlude.report(result, nout, 0)[-1]
    with pytest.raises(_lib.C3Error, match="head 2"):
        occlude.report(dict(result, base_rows=base[:, :24]), 24, 2)
