"""Subsample mode (c3_subsample_rows, csrc/c3_subsample.h), the part that needs no GPU: the counter hash against its known answers, the numpy
rule (synthetic.subsample_keys / subsample_masks / subsample_variants / subsample_records) against plain loops that sort, build windows row
by row and walk columns as the kernels do, its hand-made corners (shared with tests/test_subsample_gpu.py, which runs them through the
device), the records against the header and the binding, the refusals that need no device and the tool.  (The host's planner -- the pass
cut, the staged table, the host's own selection -- is exercised without a device by the stand-alone program
tests/host/subsample_host_check.cpp, built with -fsanitize=address,undefined as its head says.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from clair3_amd import _lib, subsample, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import util
from tests.test_abi import HEADER, declared_symbols

ENTRIES = ("c3_subsample_rows", "c3_subsample", "c3_subsample_reduce")
SUBSAMPLE_H = os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_subsample.h")
F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
M64 = (1 << 64) - 1
GOLD, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_records(a, b):
    """every field of level or window records: integers equal, floats bitwise equal"""
    return a.dtype == b.dtype and a.shape == b.shape and all(same(a[name], b[name]) for name in a.dtype.names)


# ---- the hash ----
def py_mix(z):
    z ^= z >> 30
    z = z * MUL1 & M64
    z ^= z >> 27
    z = z * MUL2 & M64
    return z ^ z >> 31


def py_key(seed, w, r, j, depth, R):
    return py_mix((seed + GOLD * (1 + (w * R + r) * depth + j)) & M64)


def test_known_answers_of_the_hash():
    assert [int(k) for k in syn.subsample_keys(0, 0, 0, 3, 89, 8)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [py_key(0, 0, 0, j, 89, 8) for j in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # any window, replicate and seed, the wrap of the counter and of the seed included
    for seed, w, r, depth, R in ((0, 5, 2, 89, 3), (M64, 7, 31, 55, 32), (0xDEADBEEFCAFEF00D, (1 << 40) + 3, 1, 128, 2)):
        got = syn.subsample_keys(seed, w, r, 9, depth, R)
        assert got.dtype == np.uint64 and [int(k) for k in got] == [py_key(seed, w, r, j, depth, R) for j in range(9)]
    assert len(syn.subsample_keys(1, 0, 0, 0, 89, 1)) == 0


def test_the_header_states_the_same_hash():
    src = open(SUBSAMPLE_H).read()
    for word in ("0x9E3779B97F4A7C15ull * (1 + (w * R + r) * depth + j)", "z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;", "z ^= z >> 27; z *= 0x94D049BB133111EBull;",
                 "z ^= z >> 31;"):
        assert word in src, word


# ---- masks against a plain-Python loop that sorts (key, j) ----
COUNTS = [0, 1, 2, 17, 89, 5]
DEPTHS = (1, 2, 16, 60, 200)


def loop_masks(counts, depths, R, seed, depth):
    """[(window, level, replicate, kept reads in read order)] in the rule's order"""
    out = []
    for w, n in enumerate(counts):
        for l, d in enumerate(depths):
            k = min(n, d)
            if k == n:
                continue
            for r in range(R):
                ranked = sorted((py_key(seed, w, r, j, depth, R), j) for j in range(n))
                out.append((w, l, r, sorted(j for _, j in ranked[:k])))
    return out


def bits_of(mask):
    return int(mask[0]) | int(mask[1]) << 64


def test_masks_against_a_loop():
    R, seed, depth = 3, 12345, 89
    masks = syn.subsample_masks(COUNTS, DEPTHS, R, seed, depth)
    want = loop_masks(COUNTS, DEPTHS, R, seed, depth)
    assert masks.shape == (len(want), 2) and masks.dtype == np.uint64
    assert same(syn.subsample_variant_counts(COUNTS, DEPTHS, R), np.array([0, 0, 3, 9, 12, 6], np.int64)) and len(want) == 30
    by_replicate = {}
    for mask, (w, l, r, kept) in zip(masks, want):
        bits = bits_of(mask)
        assert bits == sum(1 << j for j in kept), (w, l, r)
        assert bin(bits).count("1") == min(COUNTS[w], DEPTHS[l]) < COUNTS[w], "popcount == keep, and a level with k == n is not run"
        assert bits >> COUNTS[w] == 0
        by_replicate.setdefault((w, r), []).append(bits)
    for chain in by_replicate.values():  # nested across levels
        assert all(a & b == a for a, b in zip(chain, chain[1:]))
    assert any(bits_of(m) >> 64 for m in masks), "reads beyond the 64th are kept too"
    assert not same(masks, syn.subsample_masks(COUNTS, DEPTHS, R, seed + 1, depth)), "another seed, other subsets"
    assert not same(masks[3:6], masks[6:9][:, :]) and len({bits_of(m) for m in masks[3:6]}) > 1, "replicates differ"
    # the window index is the call's: the masks of a window do not depend on the windows behind it, and do depend on its place
    assert same(syn.subsample_masks(COUNTS[:4], DEPTHS, R, seed, depth), masks[:12])
    assert not same(syn.subsample_masks(COUNTS[3:4], DEPTHS, R, seed, depth), masks[3:12])
    for bad in (dict(depths=()), dict(depths=(2, 2)), dict(depths=(0, 1)), dict(depths=tuple(range(1, 10))), dict(replicates=0), dict(replicates=33)):
        with pytest.raises(ValueError):
            syn.subsample_masks(COUNTS, bad.get("depths", DEPTHS), bad.get("replicates", R), seed, depth)


def test_the_lowest_read_wins_equal_keys():
    keys = np.array([7, 3, 3, 9, 3], np.uint64)
    assert syn.subsample_rank(keys, 1).tolist() == [False, True, False, False, False]
    assert syn.subsample_rank(keys, 2).tolist() == [False, True, True, False, False]
    assert syn.subsample_rank(keys, 4).tolist() == [True, True, True, False, True]
    assert not syn.subsample_rank(keys, 0).any() and syn.subsample_rank(keys, 5).all()
    big = np.array([M64, 1 << 63, (1 << 63) - 1], np.uint64)  # unsigned order
    assert syn.subsample_rank(big, 1).tolist() == [False, False, True]


# ---- variants against a loop that builds each dense window row by row ----
def loop_variants(rows, counts, firsts, depths, R, seed, depth, layout):
    out, starts = [], np.r_[0, np.cumsum(counts)]
    for w, l, r, kept in loop_masks(counts, depths, R, seed, depth):
        n, k = counts[w], len(kept)
        base_first = (depth - n) // 2 if firsts is None else firsts[w]
        x = np.zeros((depth,) + rows.shape[1:], rows.dtype)
        at = base_first if layout == "in_place" else (depth - k) // 2
        for j in kept:
            x[at] = rows[starts[w] + j]
            at += 1
        out.append(x)
    return np.stack(out) if out else np.zeros((0, depth) + rows.shape[1:], rows.dtype)


@pytest.mark.parametrize("depth,channels", [(89, 8), (89, 9), (55, 8)])
@pytest.mark.parametrize("layout", syn.JACKKNIFE_LAYOUTS)
def test_variants_against_a_loop(depth, channels, layout):
    rng = np.random.default_rng(depth * 10 + channels)
    counts = [0, 1, 2, 17, depth, 5]
    rows = rng.integers(-100, 101, size=(sum(counts), 33, channels)).astype(np.int8)
    rows[(rows == 0).all(axis=(1, 2))] = 1
    rows[3 + 5] = 0  # an interior all-zero row inside the run of 17: a read like any other
    R, seed, depths = 3, 99, (1, 2, 16, 60)
    got = syn.subsample_variants(rows, counts, None, depths, R, seed, depth, layout)
    want = loop_variants(rows, counts, None, depths, R, seed, depth, layout)
    assert got.dtype == np.int8 and got.shape == want.shape == (int(syn.subsample_variant_counts(counts, depths, R).sum()), depth, 33, channels)
    assert same(got, want)
    firsts = [3, depth - 1, 0, depth - 17, 0, depth - 5]  # explicit firsts, runs at the top and at the bottom of the window
    got = syn.subsample_variants(rows, counts, firsts, depths, R, seed, depth, layout)
    assert same(got, loop_variants(rows, counts, firsts, depths, R, seed, depth, layout))
    occupied = (got != 0).any(axis=(2, 3))
    if layout == "in_place":  # the kept rows start where the base run starts: window 2 (first 0), level 0 keeps one read
        assert occupied[0].nonzero()[0].tolist() == [0]
    else:
        assert occupied[0].nonzero()[0].tolist() == [(depth - 1) // 2]
    with pytest.raises(ValueError):
        syn.subsample_variants(rows, counts, None, depths, R, seed, depth, "centre")
    with pytest.raises(ValueError):
        syn.subsample_variants(rows[:-1], counts, None, depths, R, seed, depth)


# ---- subsample_records against a loop that walks the columns as subsample_reduce_kernel does ----
def loop_argmax(v, lo, hi):
    best, at = -INF, lo
    for c in range(lo, hi):
        if v[c] > best:
            best, at = v[c], c
    return at


def loop_records(base, var, counts, depths, R, nout):
    cols = base.shape[1] > nout
    heads = syn.head_slices(nout)
    L = len(depths)
    lev = np.zeros((len(base), L), syn.SUBSAMPLE_LEVEL_DTYPE)
    win = np.zeros(len(base), syn.SUBSAMPLE_WINDOW_DTYPE)
    at = 0
    with np.errstate(invalid="ignore"):
        for b, n in enumerate(counts):
            y = base[b]
            t = [loop_argmax(y, lo, hi) for lo, hi in heads]
            flipped = [[False] * L for _ in range(5)]
            win["reads"][b] = n
            for l, d in enumerate(depths):
                k = min(n, d)
                lev["keep"][b, l] = k
                best = [None] * len(heads)
                if k < n:
                    lev["run"][b, l] = R
                    win["levels_run"][b] += 1
                    for r in range(R):
                        v = var[at + r]
                        finite = all(bool(np.isfinite(v[c])) for c in range(nout))
                        lev["nonfinite"][b, l] += not finite
                        for h, (lo, hi) in enumerate(heads):
                            lev["flips"][b, l, h] += loop_argmax(v, lo, hi) != t[h]
                            if finite and (best[h] is None or v[t[h]] < best[h]):
                                best[h] = v[t[h]]
                        if cols:
                            lev["decision_flips"][b, l] += any(bool(v[nout + 23 + q] != y[nout + 23 + q]) for q in range(4))
                    at += R
                for h in range(len(heads)):
                    lev["min_kept"][b, l, h] = y[t[h]] if best[h] is None else best[h]
                    flipped[h][l] = lev["flips"][b, l, h] > 0
                flipped[4][l] = lev["decision_flips"][b, l] > 0
            for h in range(5):  # the lowest l such that nothing flips at l or deeper
                hold = next(l for l in range(L + 1) if not any(flipped[h][l:]))
                if h < 4:
                    win["hold_level"][b, h] = hold
                else:
                    win["hold_decision"][b] = hold
    return lev, win


def random_rows(n, nout, columns, rng):
    y = np.zeros((n, nout + (syn.DECODE_COLS if columns else 0)), F32)
    for lo, hi in syn.head_slices(nout):
        e = np.exp(rng.normal(size=(n, hi - lo)) * 2).astype(F32)
        y[:, lo:hi] = e / e.sum(axis=1, keepdims=True)
    if columns:
        y[:, nout:nout + 23] = rng.random((n, 23)).astype(F32)
        y[:, nout + 23:nout + 27] = rng.integers(0, 3, size=(n, 4)).astype(F32)
    return y


CORNER_DEPTHS, CORNER_R = (2, 4, 8), 3


def corner_rows(nout, columns):
    """Hand-made windows where flips, ties and NaNs are certain: (names, base rows, variant rows, counts) for CORNER_DEPTHS / CORNER_R.
    One window per corner; its variants are given level by level (only the levels below its count), CORNER_R rows each."""
    width = nout + (syn.DECODE_COLS if columns else 0)
    heads = syn.head_slices(nout)
    nh = len(heads)

    def row(tops=None, top=0.9, rest=0.001):
        r = np.full(width, rest, F32)
        for h, (lo, hi) in enumerate(heads):
            r[lo + (tops[h] if tops else 0)] = top
        if columns:
            r[nout:] = 0
            r[nout:nout + 9] = F32(0.05) * np.arange(1, 10, dtype=F32)
            r[nout + 9:nout + 13] = 0.9
            r[nout + 23:nout + 27] = (1, 2, 0, 5)
        return r

    names, base, var, counts = [], [], [], []

    def add(name, n, y, levels):
        assert len(levels) == sum(d < n for d in CORNER_DEPTHS) and all(len(v) == CORNER_R for v in levels), name
        names.append(name), base.append(y), counts.append(n)
        for v in levels:
            var.extend(v)

    zero, one = [0] * nh, [1] * nh
    allnan = np.full(width, NAN, F32)
    stay = lambda top=0.9: row(zero, top=top)  # noqa: E731
    # nothing flips at any level: every hold 0; min_kept is the smallest called probability of the level
    add("stable", 20, stay(), [[stay(0.5), stay(0.4), stay(0.6)], [stay(0.7), stay(0.8), stay(0.75)], [stay(0.85), stay(0.9), stay(0.88)]])
    # a flip only at the shallowest level: holds from level 1 on
    add("flip_shallowest", 20, stay(), [[row(one), stay(0.6), stay(0.6)], [stay(0.8)] * 3, [stay()] * 3])
    # a flip at the deepest level: hold_level == L, whatever the shallower levels do
    add("flip_deepest", 9, stay(), [[stay()] * 3, [stay()] * 3, [stay(), stay(), row(one)]])
    # a flip at the middle level alone, and the deepest level not run (count 8): holds from level 2 on
    add("flip_middle_short", 8, stay(), [[stay()] * 3, [stay(), row(one), row(one)]])
    # a NaN base row: t is the head's first column, no comparison holds, min_kept of a level without variants is the NaN itself
    add("nan_base", 3, allnan.copy(), [[stay(0.3), stay(0.2), stay(0.25)]])
    # all variants NaN: they flip by the rule, none is finite, min_kept is the base row's own value
    add("all_nan", 5, row([2] * nh), [[allnan.copy()] * 3, [allnan.copy()] * 3])
    # an inf in a variant: non-finite, counted in flips, left out of min_kept although its called probability is the smallest
    inf_v = row(one, top=0.95)
    inf_v[0] = F32(0.01)
    inf_v[1] = INF
    add("inf_variant", 3, stay(), [[inf_v, stay(0.6), stay(0.7)]])
    # a tie in a head: base arg-max is the lower index; a variant that keeps the tie does not flip, one that breaks it upward does
    y = row(zero, top=0.5)
    y[7] = 0.5
    up = y.copy()
    up[0], up[7] = 0.4, 0.6
    add("base_tie", 5, y, [[y.copy(), up, y.copy()], [y.copy()] * 3])
    # -0 against +0 in the called column: equal by `<`, the lowest replicate's bits stay
    z = row(zero, top=0.0, rest=-1.0)
    nz = z.copy()
    nz[[lo for lo, _ in heads]] = F32(-0.0)
    add("zero_tie", 3, z, [[nz, z.copy(), nz.copy()]])
    add("zero_tie_other_order", 3, z, [[z.copy(), nz, nz.copy()]])
    # decoder decisions alone differ (columns): a decision flip at levels 0 and 1, none at 2; two columns in one variant count once
    d1, d2 = stay(), stay()
    if columns:
        d1[nout + 23], d1[nout + 26] = 0, 9
        d2[nout + 24] = 7
    add("decision_only", 20, stay(), [[d1, stay(), d1.copy()], [stay(), d2, stay()], [stay()] * 3])
    add("no_reads", 0, stay(), [])
    add("one_read", 1, stay(), [])
    add("count_equals_shallowest", 2, stay(), [])
    # flips in every head but the first
    fl = row([0] + [2] * (nh - 1), top=0.6)
    add("other_heads", 5, stay(), [[fl, stay(), fl.copy()], [stay()] * 3])
    return names, np.stack(base), np.stack(var), np.array(counts, np.int32)


@pytest.mark.parametrize("nout", [90, 24])
@pytest.mark.parametrize("columns", [False, True])
def test_records_against_a_loop(nout, columns):
    rng = np.random.default_rng(nout + columns)
    counts = np.array([5, 0, 1, 89, 17, 2, 61], np.int32)
    depths, R = (1, 2, 16, 60, 200), 5
    total = int(syn.subsample_variant_counts(counts, depths, R).sum())
    base, var = random_rows(len(counts), nout, columns, rng), random_rows(total, nout, columns, rng)
    var[40:70] = base[3] + (var[40:70] - base[3]) * F32(0.01)  # variants close to their base row, as real ones are
    lev, win = syn.subsample_records(base, var, counts, depths, R, nout)
    llev, lwin = loop_records(base, var, counts, depths, R, nout)
    assert same_records(lev, llev) and same_records(win, lwin)
    assert lev["flips"].sum() > 0 and win["reads"].tolist() == counts.tolist() and win["levels_run"].tolist() == [2, 0, 0, 4, 3, 1, 4]
    assert not lev["run"][:, 4].any() and (lev["keep"][:, 4] == counts).all(), "a target depth above every count is never run"
    assert (lev["decision_flips"].sum() > 0) == columns
    if nout == 24:
        assert not lev["flips"][:, :, 2:].any() and not lev["min_kept"][:, :, 2:].any() and not win["hold_level"][:, 2:].any()
    with pytest.raises(ValueError):
        syn.subsample_records(base, var[:-1], counts, depths, R, nout)
    with pytest.raises(ValueError):
        syn.subsample_records(base[:, :-1], var[:, :-1], counts, depths, R, nout)


@pytest.mark.parametrize("nout", [90, 24])
@pytest.mark.parametrize("columns", [False, True])
def test_records_of_the_hand_made_corners(nout, columns):
    names, base, var, counts = corner_rows(nout, columns)
    lev, win = syn.subsample_records(base, var, counts, CORNER_DEPTHS, CORNER_R, nout)
    llev, lwin = loop_records(base, var, counts, CORNER_DEPTHS, CORNER_R, nout)
    assert same_records(lev, llev) and same_records(win, lwin)
    at = {n: i for i, n in enumerate(names)}
    nh, L = len(syn.head_slices(nout)), len(CORNER_DEPTHS)
    i = at["stable"]
    assert not win["hold_level"][i].any() and win["hold_decision"][i] == 0 and win["levels_run"][i] == 3 and lev["run"][i].tolist() == [3, 3, 3]
    assert (lev["min_kept"][i, :, :nh] == np.array([0.4, 0.7, 0.85], F32)[:, None]).all() and lev["keep"][i].tolist() == [2, 4, 8]
    i = at["flip_shallowest"]
    assert (win["hold_level"][i, :nh] == 1).all() and lev["flips"][i, 0, 0] == 1 and not lev["flips"][i, 1:].any()
    i = at["flip_deepest"]
    assert (win["hold_level"][i, :nh] == L).all() and lev["flips"][i, :, 0].tolist() == [0, 0, 1]
    i = at["flip_middle_short"]
    assert (win["hold_level"][i, :nh] == 2).all() and lev["run"][i].tolist() == [3, 3, 0] and lev["keep"][i, 2] == 8 and win["levels_run"][i] == 2
    assert (lev["min_kept"][i, 2, :nh] == F32(0.9)).all(), "a level that did not run reports the base row's own value"
    i = at["nan_base"]
    assert lev["nonfinite"][i].sum() == 0 and (lev["min_kept"][i, 0, :nh] == F32(0.2)).all() and np.isnan(lev["min_kept"][i, 1:, :nh]).all()
    assert same(lev["min_kept"][i, 1, :nh], base[i][[lo for lo, _ in syn.head_slices(nout)]]), "the NaN's own bits"
    i = at["all_nan"]
    assert lev["nonfinite"][i].tolist() == [3, 3, 0] and (lev["flips"][i, :2, :nh] == 3).all() and (lev["min_kept"][i, :, :nh] == F32(0.9)).all()
    assert (win["hold_level"][i, :nh] == 2).all()
    i = at["inf_variant"]
    assert lev["nonfinite"][i, 0] == 1 and (lev["flips"][i, 0, :nh] == 1).all() and (lev["min_kept"][i, 0, :nh] == F32(0.6)).all()
    i = at["base_tie"]
    assert lev["flips"][i, 0, 0] == 1 and lev["flips"][i, 1, 0] == 0 and win["hold_level"][i, 0] == 1 and lev["min_kept"][i, 0, 0] == F32(0.4)
    i, j = at["zero_tie"], at["zero_tie_other_order"]
    assert np.signbit(lev["min_kept"][i, 0, :nh]).all() and not np.signbit(lev["min_kept"][j, 0, :nh]).any() and not lev["flips"][[i, j]].any()
    i = at["decision_only"]
    assert lev["decision_flips"][i].tolist() == ([2, 1, 0] if columns else [0, 0, 0]) and win["hold_decision"][i] == (2 if columns else 0)
    assert not win["hold_level"][i].any()
    for name, n in (("no_reads", 0), ("one_read", 1), ("count_equals_shallowest", 2)):
        i = at[name]
        assert win["reads"][i] == n and win["levels_run"][i] == 0 and not win["hold_level"][i].any() and not lev["run"][i].any()
        assert lev["keep"][i].tolist() == [n] * 3 and (lev["min_kept"][i, :, :nh] == F32(0.9)).all()
    i = at["other_heads"]
    assert win["hold_level"][i, 0] == 0 and (win["hold_level"][i, 1:nh] == 1).all() and (lev["flips"][i, 0, 1:nh] == 2).all()
    assert not win["reserved"].any()
    if nout == 24:
        assert not win["hold_level"][:, 2:].any() and not lev["min_kept"][:, :, 2:].any()


# ---- the header, the binding and the numpy dtypes are one record ----
def header_fields(body):
    ctypes_of = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "int64_t": ctypes.c_int64}
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


def test_records_match_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, struct, dtype, size in (("c3_subsample_level", _lib.SubsampleLevel, syn.SUBSAMPLE_LEVEL_DTYPE, 48),
                                      ("c3_subsample_window", _lib.SubsampleWindow, syn.SUBSAMPLE_WINDOW_DTYPE, 32)):
        body = re.search(rf"typedef struct {name} \{{([^}}]*)\}} {name};", src).group(1)
        assert list(struct._fields_) == header_fields(body), name
        assert ctypes.sizeof(struct) == size == dtype.itemsize, name
        for field, _ in struct._fields_:
            assert getattr(struct, field).offset == dtype.fields[field][1], (name, field)
    assert [_lib.SubsampleLevel.flips.offset, _lib.SubsampleLevel.min_kept.offset] == [16, 32]
    assert [_lib.SubsampleWindow.hold_level.offset, _lib.SubsampleWindow.hold_decision.offset] == [8, 24]
    info = re.search(r"typedef struct \{([^}]*)\} c3_subsample_info;", src).group(1)
    assert list(_lib.SubsampleInfo._fields_) == header_fields(info) and ctypes.sizeof(_lib.SubsampleInfo) == 48


def test_definitions_of_the_kernel_header():
    src = open(SUBSAMPLE_H).read()
    assert 'section(".c3_subsample_text")' in src and src.count("C3_SUBSAMPLE_TEXT void") == 2, "both kernels of the mode in their own section"
    assert "behind `.c3_jackknife_text`" in src
    assert "h == 0 ? 0 : h == 1 ? 21 : h == 2 ? 24 : 57" in src, "the heads of syn.head_slices"
    assert "p.nout + 23 + q" in src, "the decoder's first decision per reference base"
    assert "(depth - k) / 2" in src and "C3_JACKKNIFE_IN_PLACE ? f" in src, "the two layouts"
    variants = open(os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_variants.h")).read()  # what the mode shares with the other two
    assert "static_assert(sizeof(SubsampleEntry) == 32" in src and 'variant_chunk_env("C3HIP_SUBSAMPLE_CHUNK", 64)' in src
    assert "e ? atoll(e) : dflt" in variants
    assert "kSubsampleMaxDepth = 128" in src and "kSubsampleMaxLevels = 8, kSubsampleMaxReplicates = 32" in src
    for word in ("a NaN never", "lowest j first on equal keys", "an interior all-zero row of\n// the run is a read too", "NOT RUN", "NESTED", "atomic"):
        assert word in src, word
    assert "atomicAdd" not in src and "atomicMax" not in src and "hipMemset(" not in src
    jk = open(os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_jackknife.h")).read()
    assert "subsample" not in jk, "the mode adds nothing to c3_jackknife.h"
    hip = open(os.path.join(util.ROOT, "clair3_amd", "csrc", "c3_model.hip")).read()
    assert hip.index('#include "c3_jackknife.h"') < hip.index('#include "c3_subsample.h"') and "hipFree(m->variant_dev)" in hip
    assert "subsample_dev" not in hip and "hipMalloc(&m->variant_dev" in variants, "one buffer for the three modes, freed with the handle"


def test_entries_are_declared_bound_and_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared_symbols() and name in _lib.EXPORTS and hasattr(lib, name), name
    src = open(HEADER).read()
    comment = src[src.index("/* ---- subsample mode"):src.index("int c3_subsample_rows(")]
    for word in ("DESIGN.md 4", "c3_subsample.h", "Refused before anything is queued", "C3HIP_SUBSAMPLE_CHUNK", "on_fp32", "bit for bit c3_predict_rows",
                 "a NaN", "0x9E3779B97F4A7C15", "nested"):
        assert word in comment, word


# ---- refusals that need no device ----
def test_null_handle_and_no_device_errors():
    L = _lib.lib()
    rec, lev, cnt = _lib.SubsampleWindow(), (_lib.SubsampleLevel * 2)(), (ctypes.c_int32 * 1)(1)
    depths = (ctypes.c_int32 * 2)(1, 2)
    out = (ctypes.byref(rec), lev, None, None, None)
    assert L.c3_subsample_rows(None, None, None, cnt, 1, depths, 2, 3, 0, 0, None, *out) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_subsample(None, None, _lib.DTYPE_I8, 1, depths, 2, 3, 0, 0, None, *out) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_subsample_reduce(None, None, None, 90, cnt, 1, depths, 2, 3, ctypes.byref(rec), lev) != 0 and b"null model" in L.c3_last_error()
    rows, counts = np.zeros((2, 33, 8), np.int8), np.array([2], np.int32)
    x = np.zeros((1, 89, 33, 8), np.int8)
    f = Clair3_F(add_indel_length=True, predict=True)
    for call in (lambda: f.subsample_rows(rows, counts), lambda: f.subsample(x),
                 lambda: f.subsample_reduce(np.zeros((1, 90), F32), np.zeros((0, 90), F32), counts)):
        with pytest.raises(_lib.C3Error, match="no device"):
            call()
    with pytest.raises(_lib.C3Error, match="no device"):
        Clair3_P(add_indel_length=True, predict=True).subsample_reduce(np.zeros((1, 90), F32), np.zeros((0, 90), F32), counts)
    # the plan is refused before the handle is looked at
    for call in (lambda: f.subsample_rows(rows, counts, layout="centre"), lambda: f.subsample(x, layout=1)):
        with pytest.raises(_lib.C3Error, match="layout must be"):
            call()
    for kw, match in ((dict(depths=()), "levels"), (dict(depths=tuple(range(1, 10))), "levels"), (dict(depths=(2, 2)), "strictly increasing"),
                      (dict(depths=(0, 5)), "strictly increasing"), (dict(depths=(5, 3)), "strictly increasing"), (dict(depths="ab"), "depths must be"),
                      (dict(replicates=0), "replicates"), (dict(replicates=33), "replicates"), (dict(replicates=2.5), "replicates"),
                      (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed")):
        for call in (lambda: f.subsample_rows(rows, counts, **kw), lambda: f.subsample(x, **kw)):
            with pytest.raises(_lib.C3Error, match=match):
                call()
        if "seed" not in kw:
            with pytest.raises(_lib.C3Error, match=match):
                f.subsample_reduce(np.zeros((1, 90), F32), np.zeros((0, 90), F32), counts, **kw)
    assert not hasattr(Clair3_P, "subsample") and not hasattr(Clair3_P, "subsample_rows"), "the pileup network's windows are counts, not reads"
    assert hasattr(Clair3_P, "subsample_reduce")


# ---- the tool ----
def test_the_tool_refuses_bad_arguments_before_any_device_call(monkeypatch):
    from clair3_amd import predict
    monkeypatch.setattr(predict, "build_model", lambda *a, **k: pytest.fail("a device call before the arguments were checked"))
    base = ["--chkpnt_fn", "m.pt", "--tensor_fn", "x.npy"]
    for extra, match in ((["--layout", "centre"], "--layout"), (["--depths", "10,x"], "--depths"), (["--depths", "10,10"], "--depths"),
                         (["--depths", "0,3"], "--depths"), (["--depths", "1,2,3,4,5,6,7,8,9"], "--depths"), (["--depths", ""], "--depths"),
                         (["--replicates", "0"], "--replicates"), (["--replicates", "33"], "--replicates"), (["--seed", "-1"], "--seed"),
                         (["--top", "-1"], "--top"), (["--max_windows", "0"], "--max_windows")):
        with pytest.raises(_lib.C3Error, match=match):
            subsample.main(base + extra)
    with pytest.raises(SystemExit):
        subsample.parse_args(["--tensor_fn", "x.npy"])
    args = subsample.parse_args(base)
    assert args.layout == "recentre" and args.depths == (10, 20, 30, 40) and args.replicates == 8 and args.seed == 0 and args.top == 20


def test_the_report_of_the_tool():
    nout = 90
    names, base, var, counts = corner_rows(nout, True)
    lev, win = syn.subsample_records(base, var, counts, CORNER_DEPTHS, CORNER_R, nout)
    lines = subsample.report(dict(levels=lev, rows=win, counts=counts), nout, CORNER_DEPTHS, top=4)
    total, listed = lines[-1], lines[:-1]
    assert len(listed) == 4
    # the windows that hold latest first: flip_deepest (3), then those that hold from level 2 on in window order
    assert [line["window"] for line in listed] == [names.index(n) for n in ("flip_deepest", "flip_middle_short", "all_nan", "decision_only")]
    assert listed[0]["hold_level"] == [3, 3, 3, 3] and listed[0]["hold_depth"] is None and listed[0]["reads"] == 9
    assert listed[1]["hold_depth"] == 8 and [l["depth"] for l in listed[1]["levels"]] == [2, 4] and listed[1]["levels"][1]["flips"] == [2, 2, 2, 2]
    assert listed[3]["hold_decision"] == 2 and listed[3]["hold_level"] == [0, 0, 0, 0] and [l["decision_flips"] for l in listed[3]["levels"]] == [2, 1, 0]
    run = lev["run"] > 0
    assert total["windows"] == len(win) and total["variants"] == len(var) and total["depths"] == [2, 4, 8]
    assert total["windows_run"] == run.sum(axis=0).tolist() and total["windows_run"][0] > total["windows_run"][2] > 0
    assert total["windows_head_flip"] == (lev["flips"] > 0).any(axis=2).sum(axis=0).tolist()
    # level 0: all_nan and nan_base (a NaN compares != to anything) and decision_only; level 1: all_nan and decision_only
    assert total["windows_decision_flip"] == [3, 2, 0] and total["nonfinite"] == int(lev["nonfinite"].sum())
    assert total["hold_level_genotype"] == [int((win["hold_level"][:, 1] == l).sum()) for l in range(4)] and sum(total["hold_level_genotype"]) == len(win)
    assert len(subsample.report(dict(levels=lev, rows=win, counts=counts), nout, CORNER_DEPTHS, top=0)) == 1
