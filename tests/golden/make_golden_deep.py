#!/usr/bin/env python3
"""Golden rows of the REAL reference pileup module on windows of very deep coverage, rescaled the way its in-process loops
rescale them before the model call (clair3/CallVariantsFromCffi.py:278-285, clair3/utils.py:104-111).

Run in the build container only (needs the reference checkout, like make_golden.py):

    python tests/golden/make_golden_deep.py

It builds seeded weights (clair3_amd/synthetic.py make_state_dict), draws int32 windows whose depths spread over everything
the rule distinguishes (<= 216: untouched; 217, 218: just above 1.5 x 144; 300 .. 6000; 30000; 0 and a negative depth: untouched),
plants counts for which the rule's two roundings differ from the exact rational x * 144 / depth, applies the rule with the
reference's own statement -- ``X[i] = X[i] / scale_factor`` on the int32 array -- runs the reference Clair3_P in fp32 on the CPU
with one thread and stores the unscaled windows, the depths, the rescaled windows, the rows, seeds and digests in
tests/golden/pileup_deep_rescaled.npz (90 columns) and the rows of a model without indel heads on the same windows in
pileup_deep_rescaled_noindel.npz.  The conditions a label comparison on the fixture rests on are asserted here and again by
tests/test_deep_rescale.py (conditions()).
"""
import hashlib
import json
import os
import sys

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from clair3_amd import synthetic as syn  # noqa: E402

MAX_DEPTH = 144  # shared/param_p.py:15
INPUT_SEED = 7001
# depth each window is drawn at and declares (the leading integer of its alt_info); None = a depth with a planted pair, see below
DEPTHS = [30, 60, 100, 144, 150, 180, 200, 210, 215, 216, 216, 216,            # not rescaled: 216 = 1.5 x 144 is not "deeper than"
          217, 217, 218, 218, 220, 250, 300, 300, 400, 500, 500, 650, 800, 1000, 1000, 1500, 2000, 3000, 3000, 4500, 6000, 6000, 30000, 30000,
          0, 0, -1, -300,                                                         # declared depths the rule leaves alone, whatever the counts
          90, 120, 160, 190, 205, 212,                                            # more ordinary coverage
          None, None, None, None, None, None, None, None, None, None, None, None,  # planted pairs
          350, 700, 1200, 2500, 5000, 216]
MIN_GAP = 1e-5  # smallest distance between a head's top two reference probabilities the fixture accepts
HEAD_SLICES = ((0, 21), (21, 24), (24, 57), (57, 90))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def sd_digest(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


def exact_rational(x, depth, max_depth=MAX_DEPTH):
    """trunc(x * max_depth / depth) in integers: what the rule is NOT"""
    x = np.asarray(x, dtype=np.int64)
    q = np.abs(x) * max_depth // depth
    return (np.sign(x) * q).astype(np.int32)


def two_roundings(x, depth, max_depth=MAX_DEPTH):
    """the reference's statement on an int32 array"""
    X = np.array(x, dtype=np.int32).reshape(1, -1)
    X[0] = X[0] / (int(depth) / max_depth)
    return X[0]


def planted_pairs(n, lo=230, hi=3000):
    """n (depth, x) pairs, depths spread over [lo, hi], 0 < x <= depth / 2 (a strand's count), where the two formulas differ"""
    found = []
    for depth in range(lo, hi + 1):
        xs = np.arange(1, depth // 2 + 1, dtype=np.int32)
        bad = xs[two_roundings(xs, depth) != exact_rational(xs, depth)]
        if len(bad):
            found.append((depth, int(bad[-1])))
    assert len(found) >= n, f"only {len(found)} depths in [{lo}, {hi}] have such a count"
    pick = np.linspace(0, len(found) - 1, n).round().astype(int)
    return [found[i] for i in pick]


def make_inputs():
    """(x int32 [B, 33, 18], depth int32 [B], planted [(window, depth, x)])"""
    n_plant = sum(d is None for d in DEPTHS)
    pairs = planted_pairs(n_plant)
    xs, depths, planted = [], [], []
    for i, d in enumerate(DEPTHS):
        pair = None
        if d is None:
            pair = pairs[len(planted)]
            d = pair[0]
        drawn = d if d > 0 else 400  # (windows that declare 0 / a negative depth carry deep counts: the rule must still leave them alone)
        w = syn.make_pileup_windows(1, seed=INPUT_SEED + i, dtype=np.int32, depth=drawn)[0]
        if pair is not None:
            # the planted count on both strands of the centre position and its neighbours, as a base count and (negated) as the reference base
            for pos, ch, sign in ((16, 1, 1), (16, 10, 1), (15, 0, -1), (17, 9, -1), (14, 4, 1)):
                w[pos, ch] = sign * pair[1]
            planted.append((i, pair[0], pair[1]))
        xs.append(w)
        depths.append(d)
    return np.stack(xs).astype(np.int32), np.array(depths, dtype=np.int32), planted


def reference_rescale(x, depth):
    """clair3/CallVariantsFromCffi.py:279-285 on a copy"""
    X = x.copy()
    for alt_idx in range(len(X)):
        d = int(depth[alt_idx])
        if d > 0 and d > MAX_DEPTH * 1.5:
            scale_factor = d / MAX_DEPTH
            X[alt_idx] = X[alt_idx] / scale_factor
    return X


def top_two_gap(y):
    gap = np.inf
    for lo, hi in HEAD_SLICES:
        if lo >= y.shape[1]:
            break
        s = np.sort(y[:, lo:hi], axis=1)
        gap = min(gap, float((s[:, -1] - s[:, -2]).min()))
    return gap


def conditions(x, depth, x_rescaled, y_ref):
    """what the fixture promises; returns (windows with a count where the two formulas differ, rescaled windows, smallest top-two gap)"""
    deep = (depth > 0) & (depth > 1.5 * MAX_DEPTH)
    differ = 0
    for i in np.nonzero(deep)[0]:
        differ += bool((x_rescaled[i].ravel() != exact_rational(x[i].ravel(), int(depth[i]))).any())
    n = len(x)
    assert differ >= 8, f"{differ} windows carry a count that tells the two formulas apart (8 needed)"
    assert 3 * int(deep.sum()) >= n, f"{int(deep.sum())} of {n} windows rescaled (a third needed)"
    assert 4 * int((~deep).sum()) >= n, f"{int((~deep).sum())} of {n} windows not rescaled (a quarter needed)"
    assert np.array_equal(x_rescaled[~deep], x[~deep])
    assert {0, 217, 218, 30000} <= set(depth.tolist()) and (depth < 0).any() and (depth <= 216).any() and ((depth >= 300) & (depth <= 6000)).any()
    assert np.isfinite(y_ref).all()
    gap = top_two_gap(y_ref)
    assert gap >= MIN_GAP, f"top-two gap {gap:.2e} below {MIN_GAP}"
    return differ, int(deep.sum()), gap


def reference_rows(sd, indel, x):
    import torch
    sys.path.insert(0, REF)
    from clair3.model import Clair3_P
    torch.set_num_threads(1)
    m = Clair3_P(add_indel_length=indel, predict=True, input_channels=18)
    m.eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    with torch.inference_mode():
        return m(torch.from_numpy(x)).detach().cpu().numpy().astype(np.float32), torch.__version__


def main():
    x, depth, planted = make_inputs()
    x_rescaled = reference_rescale(x, depth)
    for name, indel, first_seed in (("pileup_deep_rescaled", True, 7100), ("pileup_deep_rescaled_noindel", False, 7200)):
        for seed in range(first_seed, first_seed + 20):  # re-draw the weights while a head's top two are a near-tie somewhere
            sd = syn.make_state_dict(syn.PILEUP, 18, indel, seed=seed)
            y, torch_version = reference_rows(sd, indel, x_rescaled)
            gap = top_two_gap(y)
            print(f"{name}: weight seed {seed}: smallest top-two gap {gap:.2e}")
            if gap >= MIN_GAP and np.isfinite(y).all():
                break
        else:
            raise SystemExit("no weight seed without a near-tie")
        differ, n_deep, gap = conditions(x, depth, x_rescaled, y)
        meta = dict(kind=syn.PILEUP, channels=18, add_indel_length=indel, weight_seed=seed, input_seed=INPUT_SEED, max_depth=MAX_DEPTH,
                    batch=len(x), rescaled=n_deep, windows_telling_formulas_apart=differ, top_two_gap=gap, planted=planted,
                    x_sha=digest(x), depth_sha=digest(depth), x_rescaled_sha=digest(x_rescaled), sd_sha=sd_digest(sd), y_sha=digest(y),
                    torch=torch_version)
        out = dict(y_ref=y, meta=np.array(json.dumps(meta)))
        if indel:  # the windows travel once
            out.update(x=x, depth=depth, x_rescaled=x_rescaled)
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {len(x)} windows, {n_deep} rescaled, {differ} tell the formulas apart, gap {gap:.2e}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
