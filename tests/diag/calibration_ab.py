#!/usr/bin/env python3
"""What calibrating the channel exponents (model.calibrate, c3_model_calibrate) buys on a checkpoint whose activations leave the fp16 range, in
one process on one MI355X: the suite's out-of-range recipe (tests/test_calibration.py recipe_state_dict) at B = 256 on three handles --
uncalibrated (the range guard has moved it to the fp32 forms), calibrated on a sample of 64 other windows, and the ordinary seed-61
checkpoint the recipe was made from -- device-resident step time with the handles alternating (median of RUNS runs of STEPS steps each, one
batch in flight), and the rows of the first two against each other.  usage: calibration_ab.py [RUNS=9] [STEPS=100]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
for k in ("C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_CALIBRATION", "C3HIP_VERIFY"):
    os.environ.pop(k, None)
import torch  # noqa: E402
from clair3_amd import calibrate as cal, synthetic as syn  # noqa: E402
from tests.test_calibration import recipe_state_dict  # noqa: E402
from tests.test_parity_gpu import make_model  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
B = 256

sd = recipe_state_dict()
x = syn.make_fa_windows(B, seed=63)
xd = torch.from_numpy(x).cuda()

guard = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
y_guard = guard.forward(xd, checked=True).cpu().numpy()  # the checked entry notices, re-runs on fp32 and stays there
calibrated = make_model(syn.FULL_ALIGNMENT, 8, True, sd)
print(cal.summary_text(calibrated.calibrate(syn.make_fa_windows(64, seed=62))))
y_cal = calibrated.forward(xd, checked=True).cpu().numpy()
ordinary = make_model(syn.FULL_ALIGNMENT, 8, True, syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=61))
ordinary.forward(xd, checked=True)
handles = (("uncalibrated (fp32, range guard)", guard), ("calibrated", calibrated), ("ordinary seed 61", ordinary))
for name, m in handles:
    print(f"{name:34s} range_status={m.range_status()}  {m.describe()}")
print(f"rows of the {B} windows, calibrated fp16x3 against the fp32 forms on the same checkpoint: max |dY| = {np.abs(y_cal - y_guard).max():.3e}, "
      f"labels differing = {int(sum((y_cal[:, lo:hi].argmax(1) != y_guard[:, lo:hi].argmax(1)).sum() for lo, hi in ((0, 21), (21, 24), (24, 57), (57, 90))))}")

print(f"== full alignment step time, B = {B}, device resident, one batch in flight; {RUNS} runs of {STEPS} steps per handle, handles alternating")
ms = {name: [] for name, _ in handles}
for r in range(RUNS + 1):  # (the first round warms every handle's kernels up and is dropped)
    for name, m in handles:
        m(xd)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            m(xd)
        torch.cuda.synchronize()
        if r:
            ms[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
base = float(np.median(ms["ordinary seed 61"]))
for name, m in handles:
    med = float(np.median(ms[name]))
    print(f"{name:34s} median {med * 1e3:8.1f} us/step  (min {min(ms[name]) * 1e3:.1f}, max {max(ms[name]) * 1e3:.1f})  "
          f"{B / med:7.1f} k windows/s  x{med / base:.3f} of ordinary")
for name, m in handles:
    print(f"{name:34s} range_status={m.range_status()}")
