#!/usr/bin/env python3
"""The forms of full alignment's FC chain (C3HIP_FA_TAIL: split | w4 | w8 | w16, clair3_amd/csrc/c3_tail.h) against each other in one
process on one MI355X: one handle per form on the same weights (the switch is read when a handle is created), the device-resident step
time with one batch in flight, the forms alternating (median of RUNS runs of STEPS steps each per batch size), then the HIP-event times
of the chain's launches.  Where `split` stops losing is where run_tail's `auto` goes back to it (c3_model.h fa_tail_max_batch).
usage: fa_tail_ab.py [RUNS=7] [STEPS=100] [BATCH ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
for k in ("C3HIP_FA_TAIL", "C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_AUTO_FP32"):
    os.environ.pop(k, None)
import torch  # noqa: E402
from clair3_amd import synthetic as syn  # noqa: E402
from tests.test_parity_gpu import make_model  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
BATCHES = [int(a) for a in sys.argv[3:]] or [256, 512, 1000, 2048]
FORMS = ("split", "w4", "w8", "w16", "auto")

sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=41)
models = {}
for f in FORMS:
    os.environ["C3HIP_FA_TAIL"] = f
    models[f] = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
del os.environ["C3HIP_FA_TAIL"]

for batch in BATCHES:
    xd = torch.from_numpy(syn.make_fa_windows(batch, seed=42)).cuda()
    rows = {f: models[f](xd).float().cpu().numpy() for f in FORMS}
    same = all(np.array_equal(rows[f], rows["split"]) for f in FORMS)
    print(f"== B = {batch}, device resident, one batch in flight; {RUNS} runs of {STEPS} steps per form, forms alternating; rows of every form "
          f"equal to split's: {same}", flush=True)
    ms = {f: [] for f in FORMS}
    for r in range(RUNS + 1):  # (the first round warms up and is dropped)
        for f in FORMS:
            m = models[f]
            m(xd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                m(xd)
            torch.cuda.synchronize()
            if r:
                ms[f].append((time.perf_counter() - t0) * 1e3 / STEPS)
    base = float(np.median(ms["split"]))
    for f in FORMS:
        med = float(np.median(ms[f]))
        form = models[f].describe().split(" fa_tail=")[1].split()[0]
        print(f"{f:6s} {form:10s} median {med * 1e3:8.1f} us/step  (min {min(ms[f]) * 1e3:.1f}, max {max(ms[f]) * 1e3:.1f})  "
              f"{batch / med:9.1f} k windows/s  x{med / base:.4f}   all: " + " ".join(f"{v * 1e3:.1f}" for v in ms[f]), flush=True)
    for f in FORMS:  # HIP events around every launch (one stream)
        m = models[f]
        m.profile(True)
        m.profile_reset()
        for _ in range(20):
            m(xd)
        torch.cuda.synchronize()
        recs = m.profile_read()
        m.profile(False)
        print(f"{f:6s} " + " ".join(f"{r['name']}={r['total_ms'] * 1e3 / max(1, r['launches']):.1f}" for r in recs if r["name"] in ("fa.l4", "fa.tail")) + " (us)",
              flush=True)
