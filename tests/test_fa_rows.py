"""Full-alignment windows as their occupied read rows, the parts that need no GPU (csrc/c3_expand.h, include/c3hip.h c3_pack_rows): the
padding rule in numpy against the tensor the reference's own generator padded (tests/golden/make_golden_fa_rows.py), its inverse, and the
host code of the library against both."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from clair3_amd import _lib, predict, synthetic as syn
from tests import util

MIN_GAP = 1e-5  # make_golden_fa_rows.py: the smallest top-two gap of a head the fixture accepts


def fixture(name="fa_rows"):
    z = np.load(os.path.join(util.GOLDEN, f"{name}.npz"))
    return z, json.loads(str(z["meta"]))


def top_two_gap(y):
    gap = np.inf
    for lo, hi in util.HEAD_SLICES:
        s = np.sort(y[:, lo:hi], axis=1)
        gap = min(gap, float((s[:, -1] - s[:, -2]).min()))
    return gap


def fixture_sets():
    """(what, rows, counts, padded tensor of the reference generator, depth)"""
    z8, _ = fixture("fa_rows")
    z9, _ = fixture("fa_rows_dwell")
    return [("C=8", z8["rows"], z8["counts"], z8["x"], 89), ("C=9", z9["rows"], z9["counts"], z9["x"], 89),
            ("depth 55", z8["rows55"], z8["counts55"], z8["x55"], 55)]


def odd_windows(channels=8, depth=89, seed=77):
    """dense windows the centred rule does not describe: interior zero rows, off-centre runs, runs that touch row 0 and row depth - 1, an
    all-zero window, a single row at either end"""
    x = syn.make_fa_windows(9, seed=seed, recipe="uniform", channels=channels, depth=depth)
    x[0, 5:9] = 0                       # interior zero rows inside a full window
    x[1, :7] = 0                        # run [7, depth): touches the last row
    x[2, depth - 11:] = 0               # run [0, depth - 11): touches row 0
    x[3, :20] = 0
    x[3, 31:] = 0                       # an off-centre run with ...
    x[3, 24:27] = 0                     # ... interior zero rows
    x[4] = 0                            # no read at all
    x[5, 1:] = 0                        # one row, the first
    x[6, :depth - 1] = 0                # one row, the last
    x[7, :, :, :] = np.where(np.arange(depth)[:, None, None] % 2 == 0, x[7], 0)  # every other row empty
    x[8, :40] = 0
    x[8, 41:] = 0
    x[8, 40, :, :] = 0
    x[8, 40, 32, channels - 1] = -1     # one non-zero byte, the last of its row
    return x


# ------------------------------------------------------------------------------------------------ 1: the rule in numpy
def test_fixture_conditions():
    for name in ("fa_rows", "fa_rows_dwell"):
        z, meta = fixture(name)
        counts = z["counts"]
        assert len(counts) <= 32 and {0, 1, 88, 89} <= set(counts.tolist())
        pads = 89 - counts[(counts > 0) & (counts < 89)]
        assert (pads % 2 == 1).any() and (pads % 2 == 0).any()
        assert z["x"].shape == (len(counts), 89, 33, meta["channels"]) and z["x"].dtype == np.int8 and z["rows"].dtype == np.int8
        assert np.isfinite(z["y_ref"]).all() and top_two_gap(z["y_ref"]) >= MIN_GAP
        assert os.path.getsize(os.path.join(util.GOLDEN, f"{name}.npz")) <= os.path.getsize(os.path.join(util.GOLDEN, "fa_baseline_256.npz"))
    z, _ = fixture()
    assert {0, 1, 54, 55} <= set(z["counts55"].tolist()) and z["x55"].shape == (len(z["counts55"]), 55, 33, 8)


def test_padding_rule_equals_the_reference_generator():
    for what, rows, counts, x, depth in fixture_sets():
        assert int(counts.sum()) == len(rows), what
        padded = syn.pad_fa_rows(rows, counts, depth=depth)
        assert padded.dtype == np.int8 and np.array_equal(padded, x), f"{what}: pad_fa_rows differs from the reference generator's tensor"
        r, firsts, c = syn.pack_fa_rows(padded)
        assert np.array_equal(r, rows) and np.array_equal(c, counts), what
        centred = np.where(counts > 0, (depth - counts) // 2, 0)
        assert np.array_equal(firsts, centred), what


def test_explicit_firsts_round_trip():
    for channels, depth in ((8, 89), (9, 89), (8, 55)):
        x = odd_windows(channels, depth)
        rows, firsts, counts = syn.pack_fa_rows(x)
        assert counts[4] == 0 and firsts[4] == 0 and counts[0] == depth and counts[3] == 11 and firsts[3] == 20
        assert firsts[1] + counts[1] == depth and firsts[2] == 0 and counts[5] == 1 and firsts[6] == depth - 1 and counts[8] == 1
        assert np.array_equal(syn.pad_fa_rows(rows, counts, firsts, depth=depth), x)
        assert not np.array_equal(syn.pad_fa_rows(rows, counts, depth=depth), x)  # (the centred rule is another statement)
    with pytest.raises(ValueError):
        syn.pad_fa_rows(np.zeros((3, 33, 8), np.int8), [2, 2])
    with pytest.raises(ValueError):
        syn.pad_fa_rows(np.zeros((3, 33, 8), np.int8), [3], firsts=[87])


# ------------------------------------------------------------------------------------------------ 2: c3_pack_rows
def _c_pack(x, offset=0, rows_out=True):
    """c3_pack_rows through ctypes on a copy of x that starts `offset` bytes into a guarded buffer; returns (rows, firsts, counts, n)"""
    b, depth, positions, channels = x.shape
    guard = 64
    src = np.full(guard + offset + x.nbytes + guard, 0x5B, dtype=np.uint8)
    src[guard + offset:guard + offset + x.nbytes] = x.reshape(-1).view(np.uint8)
    before = src.copy()
    out = np.full(guard + offset + x.nbytes + guard, 0x5B, dtype=np.uint8)
    firsts = np.full(b + 2, -7, dtype=np.int32)
    counts = np.full(b + 2, -7, dtype=np.int32)
    n = _lib.lib().c3_pack_rows(depth, positions, channels, src.ctypes.data + guard + offset, b,
                                out.ctypes.data + guard + offset if rows_out else None, firsts[1:].ctypes.data, counts[1:].ctypes.data)
    assert n >= 0, _lib.last_error()
    assert np.array_equal(src, before), "c3_pack_rows wrote the caller's windows"
    assert firsts[0] == firsts[-1] == counts[0] == counts[-1] == -7
    nb = n * positions * channels
    assert (out[:guard + offset] == 0x5B).all() and (out[guard + offset + (nb if rows_out else 0):] == 0x5B).all()
    rows = out[guard + offset:guard + offset + nb].view(np.int8).reshape(n, positions, channels).copy()
    return rows, firsts[1:-1].copy(), counts[1:-1].copy(), n


def test_c_pack_rows_equals_the_numpy_rule():
    cases = [(what, x) for what, _, _, x, _ in fixture_sets()]
    cases += [(f"odd C={c} depth={d}", odd_windows(c, d)) for c, d in ((8, 89), (9, 89), (8, 55))]
    cases += [("realistic", syn.make_fa_windows(40, seed=5)), ("uniform", syn.make_fa_windows(6, seed=6, recipe="uniform")),
              ("realistic dwell", syn.make_fa_windows(12, seed=7, channels=9)), ("none", np.zeros((0, 89, 33, 8), np.int8))]
    for what, x in cases:
        want_rows, want_firsts, want_counts = syn.pack_fa_rows(x)
        for offset in (0, 1, 3, 7):
            rows, firsts, counts, n = _c_pack(x, offset)
            assert n == len(want_rows) and np.array_equal(counts, want_counts) and np.array_equal(firsts, want_firsts), (what, offset)
            assert np.array_equal(rows, want_rows), (what, offset)
        _, firsts, counts, n = _c_pack(x, 5, rows_out=False)
        assert n == len(want_rows) and np.array_equal(counts, want_counts) and np.array_equal(firsts, want_firsts), what
        r, f, c = predict.pack_rows(x)
        assert np.array_equal(r, want_rows) and np.array_equal(f, want_firsts) and np.array_equal(c, want_counts), what
        assert np.array_equal(syn.pad_fa_rows(r, c, f, depth=x.shape[1]), x), what


def test_c_pack_rows_refuses_bad_arguments():
    L = _lib.lib()
    c = np.zeros(1, np.int32)
    assert L.c3_pack_rows(0, 33, 8, None, 0, None, None, None) < 0 and b"geometry" in L.c3_last_error()
    assert L.c3_pack_rows(89, 33, 8, None, -1, None, None, None) < 0 and b"negative" in L.c3_last_error()
    assert L.c3_pack_rows(89, 33, 8, None, 1, None, c.ctypes.data, c.ctypes.data) < 0 and b"null" in L.c3_last_error()
    assert L.c3_pack_rows(89, 33, 8, None, 0, None, None, None) == 0
    with pytest.raises(_lib.C3Error):
        predict.pack_rows(np.zeros((1, 89, 33, 8), np.int32))


# ------------------------------------------------------------------------------------------------ 3: the ABI
NEW = ("c3_predict_submit_rows", "c3_predict_rows", "c3_pack_rows")


def test_header_binding_and_library_agree_on_the_new_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(util.ROOT, "include", "c3hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(c3_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert sorted(declared) == sorted(_lib.EXPORTS)
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    dyn = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True) if nm else None
    if dyn is not None and dyn.returncode == 0:  # (binutils at hand: the dynamic symbol table itself)
        exported = {line.split()[-1] for line in dyn.stdout.splitlines() if line.strip()}
        assert set(_lib.EXPORTS) <= exported, sorted(set(_lib.EXPORTS) - exported)
    assert _lib.lib().c3_predict_rows(None, None, None, None, 0, None) != 0 and b"null model" in _lib.lib().c3_last_error()
    assert _lib.lib().c3_predict_submit_rows(None, None, None, None, 0, None, 0) != 0
