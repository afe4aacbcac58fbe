"""Shared helpers of the test-suite: rebuild golden cases from their seeds, compare probability rows."""
import json
import os

import numpy as np

from clair3_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# parity gate of BASELINE.json: probabilities within 1e-4 (fp32), genotype / zygosity labels identical
PROB_TOL = 1e-4
# arg-max labels may legitimately differ only when the reference's own top-2 are closer than this (the reference
# moves its own probabilities by 1-2 ulp = 1.2e-7 with thread count or batch size, so "identical labels" is only meaningful outside ~1e-6)
NEAR_TIE = 1e-6
HEAD_SLICES = ((0, 21), (21, 24), (24, 57), (57, 90))


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def case_inputs(meta):
    sd = syn.make_state_dict(meta["kind"], meta["channels"], meta["add_indel_length"], seed=meta["weight_seed"],
                             peaked=meta["peaked"], trained_like=meta.get("trained_like", False))
    if meta["kind"] == syn.PILEUP:
        x = syn.make_pileup_windows(meta["batch"], meta["input_seed"], meta["recipe"], dtype=np.dtype(meta["x_dtype"]),
                                    channels=meta["channels"])
    else:
        x = syn.make_fa_windows(meta["batch"], meta["input_seed"], meta["recipe"], channels=meta["channels"],
                                depth=meta.get("depth") or syn.FA_DEPTH_ONT)
    return sd, x


def golden_y(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))["y_ref"]


def label_mismatches(y, y_ref):
    """Per head: windows whose arg-max differs although the reference top-2 gap exceeds NEAR_TIE."""
    bad = []
    for lo, hi in HEAD_SLICES:
        if lo >= y_ref.shape[1]:
            break
        a, r = y[:, lo:hi], y_ref[:, lo:hi]
        diff = np.nonzero(a.argmax(1) != r.argmax(1))[0]
        for i in diff:
            top2 = np.sort(r[i])[-2:]
            if top2[1] - top2[0] > NEAR_TIE:
                bad.append((lo, int(i)))
    return bad


def assert_rows_match(y, y_ref, tol=PROB_TOL, what=""):
    assert y.shape == y_ref.shape, f"{what}: shape {y.shape} vs {y_ref.shape}"
    assert y.dtype == np.float32
    assert np.isfinite(y).all(), f"{what}: non-finite probabilities"
    err = float(np.abs(y.astype(np.float64) - y_ref.astype(np.float64)).max())
    assert err <= tol, f"{what}: max |dY| = {err:.3e} > {tol}"
    bad = label_mismatches(y, y_ref)
    assert not bad, f"{what}: arg-max label differs outside near-ties at (head_start, window) {bad[:8]}"
    return err


def layer_errors(get, d, names, sd):
    """Full-alignment layer outputs against the oracle's.  get(name) -> the library's tensor of the same windows as d[name].
    Per tensor: max |a - d| relative to the tensor's range (at least 1).  Per channel (act0 .. act8, spp): the worst CHANNEL relative
    to that channel's own scale (a channel whose values are 1e-3 of the tensor's is invisible in the first number and is what the
    next layer's large weights amplify).  A channel's scale is what its BatchNorm gives it, |gamma| + |beta| (the larger of the two
    producers behind a residual add; spp pools act8's channels) -- its observed range if that is larger: a channel the ReLU leaves
    almost dead on the windows at hand is the clipped tail of a sum of that scale, and so is its rounding noise.  l4_out has
    no per-channel number (no BatchNorm behind it)."""
    whole, chan = {}, {}
    for name in names:
        a, ref = get(name), d[name]
        assert a.shape == ref.shape, (name, a.shape, ref.shape)
        assert np.isfinite(a).all(), name
        C = ref.shape[-1] if name.startswith("act") else 256
        err = np.abs(a.astype(np.float64) - ref).reshape(-1, C).max(0)
        rng = np.abs(ref).reshape(-1, C).max(0)
        whole[name] = float(err.max()) / max(1.0, float(rng.max()))
        if name == "l4_out":
            continue
        l = 8 if name == "spp" else int(name[3:])
        mag = lambda k: np.abs(sd[syn.FA_CONV_LAYERS[k][1] + ".weight"]) + np.abs(sd[syn.FA_CONV_LAYERS[k][1] + ".bias"])
        scale = np.maximum(rng, np.maximum(mag(l), mag(l - 2)) if l % 3 == 2 else mag(l))
        chan[name] = float((err / np.maximum(scale, 1e-30)).max())
    return whole, chan
