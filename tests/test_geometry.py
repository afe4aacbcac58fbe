"""Full-alignment windows of other geometries than 89 x 33 and 55 x 33, without a GPU: the fp64 oracle -- what the device sweep of
tests/test_geometry_gpu.py is held to -- against the rows of the REAL reference module at nine (depth, positions) shapes
(tests/golden/fa_geometry.npz, written by tests/golden/make_golden_geometry.py), the shapes the oracle refuses, and the window recipe's
stream: make_fa_windows(positions=) draws for the default call what it drew before it took the argument."""
import hashlib
import json
import os

import numpy as np
import pytest

from clair3_amd import synthetic as syn
from oracle import oracle
from tests import util

# (depth, positions) -> stages behind conv1 / conv3 / conv5; 14 pyramid bins iff each final extent is 3 or >= 5
SHAPES = [(90, 34), (64, 33), (144, 33), (41, 20), (33, 23), (17, 17), (18, 24), (55, 41), (23, 35)]
DWELL = [(90, 34), (41, 20)]
REFUSED = [(89, 31), (25, 33), (3, 3)]  # 11, 11 and 3 bins
ENTRIES = [(d, p, 8) for d, p in SHAPES] + [(d, p, 9) for d, p in DWELL]


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def fixture():
    z = np.load(os.path.join(util.GOLDEN, "fa_geometry.npz"))
    return z, json.loads(str(z["meta"]))


def fixture_windows(meta, depth, positions, channels):
    """the windows of one entry as make_golden_geometry.py drew them: the uniform ones first"""
    seed = meta["input_seed"] + 1000 * depth + 10 * positions + channels
    k = meta["per_recipe"]
    return np.concatenate([syn.make_fa_windows(k, seed=seed, recipe="uniform", channels=channels, depth=depth, positions=positions),
                           syn.make_fa_windows(k, seed=seed + 1, recipe="realistic", channels=channels, depth=depth, positions=positions)])


def stages(depth, positions):
    out, h, w = [], depth, positions
    for _ in range(3):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def test_default_window_stream_is_unchanged():
    """digests taken before make_fa_windows took ``positions``: every golden and every seeded test rests on the default call's stream"""
    assert _digest(syn.make_fa_windows(5, seed=7)) == "e0d956399dcf406a"
    assert _digest(syn.make_fa_windows(4, seed=8, channels=9, depth=55)) == "1a5de40536068f9a"
    assert _digest(syn.make_fa_windows(3, seed=9, recipe="uniform")) == "6a5cfba8df3661c5"
    assert np.array_equal(syn.make_fa_windows(3, seed=7, positions=33), syn.make_fa_windows(3, seed=7))
    x = syn.make_fa_windows(4, seed=11, channels=9, depth=41, positions=20)
    assert x.shape == (4, 41, 20, 9) and x.dtype == np.int8 and (x != 0).any(axis=(1, 3)).all(axis=1).any()
    # windows of any width go through the rows transport helpers as they are
    rows, firsts, counts = syn.pack_fa_rows(x)
    assert rows.shape[1:] == (20, 9) and np.array_equal(syn.pad_fa_rows(rows, counts, firsts, depth=41), x)


def test_fixture_covers_the_shapes():
    z, meta = fixture()
    assert [(e["depth"], e["positions"], e["channels"]) for e in meta["entries"]] == ENTRIES
    assert [tuple(r) for r in meta["refused"]] == REFUSED
    for d, p in SHAPES:  # 14 bins: each final extent is 3 or at least 5
        assert all(e == 3 or e >= 5 for e in stages(d, p)[2]), (d, p)
    for d, p in REFUSED:
        assert not all(e == 3 or e >= 5 for e in stages(d, p)[2]), (d, p)
    # what the shapes are for: even extents at conv1's input and further down, windows under a 128-pixel tile, windows wider than 34
    assert stages(90, 34) == [(45, 17), (23, 9), (12, 5)] and stages(64, 33)[2] == (8, 5) and stages(144, 33)[2] == (18, 5)
    assert stages(41, 20) == [(21, 10), (11, 5), (6, 3)] and stages(17, 17) == [(9, 9), (5, 5), (3, 3)]
    assert stages(55, 41)[0][1] > 17 and stages(23, 35)[0][1] == 18 and stages(23, 34)[0][1] == 17


@pytest.mark.parametrize("depth,positions,channels", ENTRIES)
def test_oracle_matches_reference_at_shape(depth, positions, channels):
    z, meta = fixture()
    entry = meta["entries"][ENTRIES.index((depth, positions, channels))]
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, channels, True, seed=meta["weight_seed"])
    x = fixture_windows(meta, depth, positions, channels)
    assert _digest(x) == entry["x_sha"] and x.shape == (2 * meta["per_recipe"], depth, positions, channels)
    y_ref = z[f"y_{depth}x{positions}_c{channels}"]
    assert _digest(y_ref) == entry["y_sha"]
    y, d = oracle.fa_forward(sd, x, True, debug=True)
    # the gate of the 89- and 55-row pins (test_oracle_golden.py): fp64 restatement against the fp32 reference
    err = util.assert_rows_match(y, y_ref, tol=1e-5, what=f"{depth}x{positions} C={channels}")
    print(f"{depth} x {positions}, C = {channels}: max|dY| oracle vs reference = {err:.2e}")
    assert err < 1e-5
    for l, (h, w) in zip((0, 3, 6, 8), stages(depth, positions) + stages(depth, positions)[2:]):
        assert d[f"act{l}"].shape[1:3] == (h, w), (l, d[f"act{l}"].shape)
    assert d["spp"].shape == (len(x), 14 * 256)


@pytest.mark.parametrize("depth,positions", REFUSED)
def test_oracle_refuses(depth, positions):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=101)
    x = syn.make_fa_windows(1, seed=1, recipe="uniform", depth=depth, positions=positions)
    with pytest.raises(RuntimeError, match="rc=-2"):
        oracle.fa_forward(sd, x, True)
