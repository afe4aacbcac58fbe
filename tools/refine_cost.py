"""Cost of refine mode (profiles/refine_mode.txt): B = 256 full alignment and B = 1024 pileup, one handle alternating off and on at the
default gap -- the two selection launches by HIP events (c3_profile_read), the ring host to host, the windows the batches select, and one
refining wait at a gap chosen so that a few windows are selected.

    python tools/refine_cost.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clair3_amd import synthetic as syn  # noqa: E402
from clair3_amd.model import Clair3_F, Clair3_P  # noqa: E402

RING, BATCHES, PASSES = 3, 240, 3


def ring(m, x, n):
    t0 = time.perf_counter()
    pending = []
    for i in range(n):
        if len(pending) == RING:
            m.wait(pending.pop(0))
        pending.append(m.submit(x, slot=i % RING))
    for t in pending:
        m.wait(t)
    return time.perf_counter() - t0


def blocking_us(m, x, n=20):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        m.predict_numpy(x)
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


for name, cls, kind, ch, B in (("full alignment", Clair3_F, syn.FULL_ALIGNMENT, 8, 256), ("pileup", Clair3_P, syn.PILEUP, 18, 1024)):
    m = cls(add_indel_length=True, predict=True, input_channels=ch).to("cuda:0")
    m.load_state_dict(syn.make_state_dict(kind, ch, True, seed=7))
    m.exact(True)
    x = syn.make_windows(kind, B, seed=8, channels=ch)
    y = m.predict_numpy(x)
    mins = np.sort(syn.refine_select(y, 90, 0.0)[1])
    ring(m, x, 30)  # warm-up
    # HIP events around the launches of one batch (c3_profile_read), 20 batches; the refine scope holds the two selection launches
    for on in (False, True):
        m.refine(enable=on)
        m.profile(True)
        m.profile_reset()
        for _ in range(20):
            m.predict_numpy(x)
        recs = {r["name"]: r for r in m.profile_read()}
        m.profile(False)
        tags = {k: (v["total_ms"] * 1e3 / v["launches"], v["launches"]) for k, v in recs.items() if "refine" in k}
        total = sum(v["total_ms"] for v in recs.values()) * 1e3 / 20
        print(f"{name} B={B} refine={'on' if on else 'off'}: " + "  ".join(f"{k} {us:.1f} us x {n}" for k, (us, n) in sorted(tags.items()))
              + f"  (all launches of the profiled pass: {total:.0f} us per batch)", flush=True)
    # the ring host to host, off and on alternating on the same handle
    for p in range(PASSES):
        row = []
        for on in (False, True):
            m.refine(enable=on)
            m.refine_reset()
            dt = ring(m, x, BATCHES)
            row.append(f"{'on ' if on else 'off'} {dt / BATCHES * 1e6:7.1f} us per batch ({B * BATCHES / dt / 1e3:6.0f} k windows/s)")
        st = m.refine_stats()
        print(f"{name} B={B} ring pass {p}: " + "   ".join(row) + f"   on: {st['windows_selected']} of {st['windows']} windows selected, smallest gaps "
              + "/".join(f"{g:.3g}" for g in st["min_gap"]), flush=True)
    # one refining wait: the blocking call of one batch, the mode off, on with nothing selected, on with k windows selected
    m.refine(enable=False)
    line = f"{name} B={B} blocking call: off {blocking_us(m, x):.0f} us"
    for k in (0, 1, 4, 16):
        gap = float(mins[k - 1]) if k else float(np.float32(mins[0]) / 2)
        m.refine(gap)
        m.refine_reset()
        us = blocking_us(m, x)
        st = m.refine_stats()
        line += f"   {st['windows_selected'] // st['batches']} selected {us:.0f} us"
    print(line, flush=True)
