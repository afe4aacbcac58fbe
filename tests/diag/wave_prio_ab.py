#!/usr/bin/env python3
"""The wave priority schemes of the convolution kernels (C3HIP_WAVE_PRIO=0/1, clair3_amd/csrc/c3_conv3.h wave_prio_masks) against each other in
one process on one MI355X: one handle with the switch off and one with it on, on the same weights (the switch is read when a handle is
created), the device-resident step time with one batch in flight, the handles alternating (median of RUNS runs of STEPS steps each per
batch size), then the HIP-event times of the convolution launches.
usage: wave_prio_ab.py [RUNS=7] [STEPS=100] [BATCH ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
for k in ("C3HIP_WAVE_PRIO", "C3HIP_FA_TAIL", "C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_AUTO_FP32"):
    os.environ.pop(k, None)
import torch  # noqa: E402
from clair3_amd import synthetic as syn  # noqa: E402
from tests.test_parity_gpu import make_model  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
BATCHES = [int(a) for a in sys.argv[3:]] or [256, 305, 1000]
FORMS = ("0", "1")

sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=41)
models = {}
for f in FORMS:
    os.environ["C3HIP_WAVE_PRIO"] = f
    models[f] = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
del os.environ["C3HIP_WAVE_PRIO"]

for batch in BATCHES:
    xd = torch.from_numpy(syn.make_fa_windows(batch, seed=42)).cuda()
    rows = {f: models[f](xd).float().cpu().numpy() for f in FORMS}
    same = all(np.array_equal(rows[f], rows["0"]) for f in FORMS)
    print(f"== B = {batch}, device resident, one batch in flight; {RUNS} runs of {STEPS} steps per handle, handles alternating; rows equal: {same}",
          flush=True)
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
    base = float(np.median(ms["0"]))
    for f in FORMS:
        med = float(np.median(ms[f]))
        field = models[f].describe().split(" wave_prio=")[1].split()[0]
        print(f"C3HIP_WAVE_PRIO={f} wave_prio={field}: median {med * 1e3:8.1f} us/step  (min {min(ms[f]) * 1e3:.1f}, max {max(ms[f]) * 1e3:.1f})  "
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
        print(f"C3HIP_WAVE_PRIO={f} " + " ".join(f"{r['name']}={r['total_ms'] * 1e3 / max(1, r['launches']):.1f}" for r in recs if r["name"].startswith("fa.")) + " (us)",
              flush=True)
