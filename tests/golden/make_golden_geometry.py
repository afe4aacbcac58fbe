#!/usr/bin/env python3
"""Golden rows for full-alignment windows of other geometries than 89 x 33 and 55 x 33: the REAL reference module on windows of nine
(depth, positions) shapes, so that the fp64 oracle -- what every device test of those shapes is held to -- is itself pinned there.

Run in the build container only (needs the reference checkout, like make_golden.py):

    python tests/golden/make_golden_geometry.py

Per shape (and per channel count: 8 everywhere, 9 with the dwell channel at 90 x 34 and 41 x 20) three windows of the ``uniform`` and three
of the ``realistic`` recipe (clair3_amd/synthetic.py make_fa_windows(depth=, positions=)) go through the reference Clair3_F in fp32 on the
CPU with one thread.  Stored in tests/golden/fa_geometry.npz: the float32 rows ``y_<depth>x<positions>_c<channels>`` (6 x 90, the uniform
windows first) and a ``meta`` JSON with the seeds and digests the inputs are rebuilt from -- no weights, no windows.  All nine shapes
pool into 14 pyramid bins (a stage-3 extent of 3, or of at least 5, in both directions: clair3/model.py PyramidPolling); the three shapes
of REFUSED pool into 11, 11 and 3 and the reference's own L4 turns them down, which is asserted here and recorded.
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

SHAPES = [(90, 34), (64, 33), (144, 33), (41, 20), (33, 23), (17, 17), (18, 24), (55, 41), (23, 35)]
DWELL = [(90, 34), (41, 20)]  # the shapes that also run with 9 channels
REFUSED = [(89, 31), (25, 33), (3, 3)]
WEIGHT_SEED, INPUT_SEED, PER_RECIPE = 101, 8400, 3


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def sd_digest(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


def key(depth, positions, channels):
    return f"y_{depth}x{positions}_c{channels}"


def windows(depth, positions, channels, input_seed=INPUT_SEED, per_recipe=PER_RECIPE):
    """the windows of one entry: ``per_recipe`` uniform ones, then as many realistic ones; the seed follows the shape"""
    seed = input_seed + 1000 * depth + 10 * positions + channels
    return np.concatenate([syn.make_fa_windows(per_recipe, seed=seed, recipe="uniform", channels=channels, depth=depth, positions=positions),
                           syn.make_fa_windows(per_recipe, seed=seed + 1, recipe="realistic", channels=channels, depth=depth, positions=positions)])


def reference_model(sd, channels):
    import torch
    sys.path.insert(0, REF)
    from clair3.model import Clair3_F
    torch.set_num_threads(1)
    m = Clair3_F(add_indel_length=True, predict=True, input_channels=channels)
    m.eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m, torch


def main():
    out, entries = {}, []
    for channels in (8, 9):
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, channels, True, seed=WEIGHT_SEED)
        m, torch = reference_model(sd, channels)
        for depth, positions in SHAPES if channels == 8 else DWELL:
            x = windows(depth, positions, channels)
            with torch.inference_mode():
                y = m(torch.from_numpy(x)).detach().cpu().numpy().astype(np.float32)
            assert y.shape == (2 * PER_RECIPE, 90) and np.isfinite(y).all()
            out[key(depth, positions, channels)] = y
            entries.append(dict(depth=depth, positions=positions, channels=channels, x_sha=digest(x), sd_sha=sd_digest(sd), y_sha=digest(y)))
            print(f"{depth} x {positions}, C = {channels}: y{y.shape}  argmax21={y[:, :21].argmax(1).tolist()}")
        if channels == 8:
            for depth, positions in REFUSED:  # the reference's own L4 (14 x 256 inputs) cannot take what these shapes pool into
                x = syn.make_fa_windows(1, seed=INPUT_SEED, recipe="uniform", depth=depth, positions=positions)
                try:
                    with torch.inference_mode():
                        m(torch.from_numpy(x))
                except RuntimeError as e:
                    print(f"{depth} x {positions}: refused by the reference ({str(e).splitlines()[0][:80]})")
                else:
                    raise SystemExit(f"{depth} x {positions}: the reference takes it")
    meta = dict(kind=syn.FULL_ALIGNMENT, add_indel_length=True, weight_seed=WEIGHT_SEED, input_seed=INPUT_SEED, per_recipe=PER_RECIPE,
                entries=entries, refused=REFUSED, torch=torch.__version__)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "fa_geometry.npz")
    np.savez_compressed(path, **out)
    print(f"fa_geometry.npz: {len(entries)} entries, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
