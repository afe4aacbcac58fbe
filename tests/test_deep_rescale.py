"""The rescaling rule for pileup windows of very deep coverage (clair3/CallVariantsFromCffi.py:278-285, clair3/utils.py:104-111), without
a GPU: the numpy statement of the rule against the fixture the reference's own statement wrote and against numpy's in-place
division on random pairs, the spec itself (two roundings, not the exact rational), the depth parser, the synthetic depths, and the new
symbols in header, binding and library."""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

from clair3_amd import _lib, predict, synthetic as syn
from tests import util

# (x, depth) pairs for which trunc(x / (depth / 144)) in doubles is one below the exact trunc(x * 144 / depth)
PLANTED = ((217, 248, 125, 126), (250, 300, 119, 120), (294, 336, 125, 126))


def fixture(name="pileup_deep_rescaled"):
    z = np.load(os.path.join(util.GOLDEN, f"{name}.npz"))
    return z, json.loads(str(z["meta"]))


def maker():
    spec = importlib.util.spec_from_file_location("make_golden_deep", os.path.join(util.GOLDEN, "make_golden_deep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def numpy_in_place(x, depths, max_depth=144):
    """the reference's loop, word for word, on a copy"""
    X = np.array(x, dtype=np.int32, copy=True)
    for alt_idx in range(len(X)):
        depth = int(depths[alt_idx])
        if depth > 0 and depth > max_depth * 1.5:
            scale_factor = depth / max_depth
            X[alt_idx] = X[alt_idx] / scale_factor
    return X


def test_fixture_keeps_its_promises():
    """the conditions tests/golden/make_golden_deep.py asserts when it writes the fixture, on the committed files: enough windows that tell
    the two formulas apart, a third rescaled, a quarter not, every depth class present, no near-tie in any head of any window; and the
    inputs are the ones the script draws today (recipe drift)"""
    mk = maker()
    z, meta = fixture()
    x, depth, xr, y = z["x"], z["depth"], z["x_rescaled"], z["y_ref"]
    assert x.dtype == np.int32 and depth.dtype == np.int32 and xr.dtype == np.int32 and y.dtype == np.float32
    assert x.shape == (64, 33, 18) and y.shape == (64, 90)
    differ, n_deep, gap = mk.conditions(x, depth, xr, y)
    assert (differ, n_deep) == (meta["windows_telling_formulas_apart"], meta["rescaled"]) and gap >= 1e-5
    x2, depth2, planted = mk.make_inputs()
    assert np.array_equal(x2, x) and np.array_equal(depth2, depth) and [list(p) for p in planted] == meta["planted"]
    assert mk.digest(x) == meta["x_sha"] and mk.digest(xr) == meta["x_rescaled_sha"] and mk.digest(y) == meta["y_sha"]
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=meta["weight_seed"])
    assert mk.sd_digest(sd) == meta["sd_sha"]
    z24, meta24 = fixture("pileup_deep_rescaled_noindel")
    assert z24["y_ref"].shape == (64, 24) and meta24["x_rescaled_sha"] == meta["x_rescaled_sha"]
    mk.conditions(x, depth, xr, z24["y_ref"])


def test_rule_equals_the_fixture_and_numpy_in_place():
    z, meta = fixture()
    got = syn.rescale_deep_windows(z["x"], z["depth"])
    assert got.dtype == np.int32 and np.array_equal(got, z["x_rescaled"])
    assert np.array_equal(numpy_in_place(z["x"], z["depth"]), z["x_rescaled"])
    # 10^5 random (x, depth) pairs, the planted ones among them, one pair per "window" of a single count
    rng = np.random.default_rng(11)
    depth = rng.integers(-50, 6000, size=100000).astype(np.int32)
    depth[:2000] = rng.integers(200, 240, size=2000)  # around the threshold
    depth[2000:2100] = 30000
    x = (rng.integers(-1, 2, size=depth.size) * rng.integers(0, np.maximum(np.abs(depth), 1) + 1)).astype(np.int32)
    for i, (px, pd, _, _) in enumerate(PLANTED):
        x[3000 + 2 * i], depth[3000 + 2 * i] = px, pd
        x[3001 + 2 * i], depth[3001 + 2 * i] = -px, pd
    got = syn.rescale_deep_windows(x.reshape(-1, 1, 1), depth)
    assert np.array_equal(got, numpy_in_place(x.reshape(-1, 1, 1), depth))
    deep = (depth > 0) & (depth > 216)
    assert np.array_equal(got.ravel()[~deep], x[~deep]) and deep.sum() > 50000
    # another max_depth moves the threshold with it
    assert np.array_equal(syn.rescale_deep_windows(x.reshape(-1, 1, 1), depth, max_depth=89), numpy_in_place(x.reshape(-1, 1, 1), depth, 89))
    x0 = z["x"].copy()
    syn.rescale_deep_windows(x0, z["depth"])
    assert np.array_equal(x0, z["x"]), "the input must not be modified"
    with pytest.raises(TypeError):
        syn.rescale_deep_windows(z["x"].astype(np.int8), z["depth"])
    with pytest.raises(ValueError):
        syn.rescale_deep_windows(z["x"], z["depth"][:3])


def test_the_rule_is_not_the_exact_rational():
    """guards the spec: two roundings in double, then towards zero -- one below the exact quotient on these pairs, for either sign"""
    mk = maker()
    for px, pd, want, exact in PLANTED:
        for sign in (1, -1):
            got = syn.rescale_deep_windows(np.full((1, 33, 18), sign * px, np.int32), np.array([pd], np.int32))
            assert (got == sign * want).all(), (px, pd, got[0, 0, 0])
            assert int(mk.exact_rational(np.array([sign * px]), pd)[0]) == sign * exact
    z, meta = fixture()
    hit = 0
    for i, pd, px in meta["planted"]:
        sel = np.abs(z["x"][i]) == px
        assert sel.sum() >= 5 and z["depth"][i] == pd
        hit += bool((z["x_rescaled"][i][sel] != mk.exact_rational(z["x"][i][sel], pd)).all())
    assert hit >= 8


def test_thresholds():
    w = np.full((6, 33, 18), 200, np.int32)
    d = np.array([216, 217, 0, -500, 218, 30000], np.int32)
    got = syn.rescale_deep_windows(w, d)
    assert [int(v) for v in got[:, 0, 0]] == [200, int(200 / (217 / 144)), 200, 200, int(200 / (218 / 144)), 0]


def test_depths_from_alt_info():
    got = predict.depths_from_alt_info(["500-XA 3 R 497 ", "0-", "217-I 2", "30000-XT 1-2 "])
    assert got.dtype == np.int32 and got.tolist() == [500, 0, 217, 30000]
    assert predict.depths_from_alt_info([]).shape == (0,)
    with pytest.raises(_lib.C3Error, match="alt_info 1 "):
        predict.depths_from_alt_info(["12-", "XA 3", "7-"])
    with pytest.raises(_lib.C3Error, match="alt_info 0 "):
        predict.depths_from_alt_info([""])


def test_synthetic_depths_leave_the_windows_alone():
    for depth in (None, 500, 3000):
        a = syn.make_pileup_windows(24, seed=5, dtype=np.int32, depth=depth)
        b, d = syn.make_pileup_windows(24, seed=5, dtype=np.int32, depth=depth, return_depth=True)
        assert np.array_equal(a, b) and d.dtype == np.int32 and d.shape == (24,)
        # the drawn depth is the reads of both strands at every position: the negated reference-base channels say so
        assert np.array_equal(-(b[:, :, 0:4].clip(max=0).sum(2) + b[:, :, 9:13].clip(max=0).sum(2)), np.repeat(d[:, None], 33, 1))
    with pytest.raises(ValueError):
        syn.make_pileup_windows(4, recipe="uniform", return_depth=True)


NEW_SYMBOLS = ("c3_model_set_max_depth", "c3_predict_depth", "c3_predict_submit_depth", "c3_predict_pileup_region_depth",
               "c3_predict_submit_region")


def test_new_symbols_in_header_binding_and_library():
    from tests.test_abi import declared_symbols
    declared = declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and name in exported, name
    assert b"c3hip 0.5." in _lib.lib().c3_version()


def test_depth_entries_fail_without_aborting():
    """argument errors that are decided before any device work: non-zero return and a message, the process goes on"""
    L = _lib.lib()
    assert L.c3_model_set_max_depth(None, 144) != 0 and b"null model" in L.c3_last_error()
    assert L.c3_predict_depth(None, None, _lib.DTYPE_I32, 0, None, None) != 0
    assert L.c3_predict_submit_depth(None, None, _lib.DTYPE_I32, 0, None, None, 0) != 0
    assert L.c3_predict_pileup_region_depth(None, None, _lib.DTYPE_I32, 0, None, 0, None, None) != 0
    assert L.c3_predict_submit_region(None, None, _lib.DTYPE_I32, 0, None, 0, None, None, 0) != 0
