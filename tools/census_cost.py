"""Cost of score mode's census while on (profiles/score_census.txt): scored batches at B = 256 full alignment and B = 1024 pileup, census
off against on, same handle alternating -- the launches by HIP events (c3_profile_read) and the ring host to host.

    python tools/census_cost.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clair3_amd import synthetic as syn  # noqa: E402
from clair3_amd.model import Clair3_F, Clair3_P  # noqa: E402

RING, BATCHES, PASSES = 3, 240, 3


def labels_for(y, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros(y.shape, np.int8)
    for lo, hi in syn.head_slices(y.shape[1]):
        cls = np.where(rng.random(len(y)) < 0.5, y[:, lo:hi].argmax(1), rng.integers(0, hi - lo, size=len(y)))
        lab[np.arange(len(y)), lo + cls] = 1
    return lab


def ring(m, x, lab, n):
    t0 = time.perf_counter()
    pending = []
    for i in range(n):
        if len(pending) == RING:
            m.wait_score(pending.pop(0))
        pending.append(m.submit_score(x, lab, slot=i % RING))
    for t in pending:
        m.wait_score(t)
    return time.perf_counter() - t0


for name, cls, kind, ch, B in (("full alignment", Clair3_F, syn.FULL_ALIGNMENT, 8, 256), ("pileup", Clair3_P, syn.PILEUP, 18, 1024)):
    m = cls(add_indel_length=True, predict=True, input_channels=ch).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(kind, ch, True, seed=7))
    x = syn.make_windows(kind, B, seed=8, channels=ch)
    lab = labels_for(m.predict_numpy(x), 9)
    m.score_mode()
    ring(m, x, lab, 30)  # warm-up
    # HIP events around the launches of one batch (c3_profile_read), 20 batches each
    for on in (False, True):
        m.score_census(on)
        m.profile(True)
        m.profile_reset()
        for _ in range(20):
            m.score(x, lab)
        recs = {r["name"]: r for r in m.profile_read()}
        m.profile(False)
        tags = {k: (v["total_ms"] * 1e3 / v["launches"], v["launches"]) for k, v in recs.items() if "score" in k or "census" in k}
        total = sum(v["total_ms"] for v in recs.values()) * 1e3 / 20
        print(f"{name} B={B} census={'on' if on else 'off'}: " + "  ".join(f"{k} {us:.1f} us x {n}" for k, (us, n) in sorted(tags.items()))
              + f"  (all launches of the profiled pass: {total:.0f} us per batch)", flush=True)
    # the ring, host to host, scored without rows: off, on, off, on ...
    for p in range(PASSES):
        out = []
        for on in (False, True):
            m.score_census(on)
            dt = ring(m, x, lab, BATCHES)
            out.append((dt / BATCHES * 1e6, B * BATCHES / dt / 1e3))
        print(f"{name} B={B} ring pass {p}: off {out[0][0]:.1f} us/batch ({out[0][1]:.0f} k windows/s)   on {out[1][0]:.1f} us/batch ({out[1][1]:.0f} k windows/s)"
              f"   added {out[1][0] - out[0][0]:+.1f} us/batch", flush=True)
    c = m.census()
    print(f"{name}: census windows {c.windows} (sum of confusion[0] {int(c.confusion[0].sum())})", flush=True)
