#!/usr/bin/env python3
"""What the range-guard policy "recalibrate" (model.range_policy, c3_model_set_range_policy) buys on the suite's out-of-range recipe
(tests/test_calibration.py recipe_state_dict), in one process on one MI355X at B = 256:
  (a) the handle healed online by the batch that tripped it against a handle calibrated offline on the same batch (model.calibrate),
  (b) ... against a sticky handle (no policy: the range guard has moved it to the fp32 forms) -- this tree's and, with PARENT given, the one
      of another checkout of the project (its package is loaded beside this one under another name, its library beside this one),
      device-resident step time, the handles alternating (median of RUNS runs of STEPS steps each, one batch in flight),
  (c) the wall time of the one c3_predict_wait that trips: recalibrating (fp32 re-run + census + solve + repack) against sticky (fp32 re-run),
      on fresh handles, the two kinds alternating.
usage: range_guard_ab.py [RUNS=7] [STEPS=100] [PARENT=<path of a checkout with a built library>]"""
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
for k in ("C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_CALIBRATION", "C3HIP_VERIFY", "C3HIP_RANGE_GUARD"):
    os.environ.pop(k, None)
import torch  # noqa: E402
from clair3_amd import synthetic as syn  # noqa: E402
from clair3_amd.model import Clair3_F  # noqa: E402
from tests.test_calibration import recipe_state_dict  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
PARENT = sys.argv[3] if len(sys.argv) > 3 else None
B = 256


def parent_class(path):
    """Clair3_F of another checkout, its package loaded as clair3_parent (its ctypes binding opens its own lib/libc3hip.so)"""
    pkg = os.path.join(path, "clair3_amd")
    spec = importlib.util.spec_from_file_location("clair3_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["clair3_parent"] = mod
    spec.loader.exec_module(mod)
    from clair3_parent import _lib as plib, model as pmodel
    print(f"parent: {plib.LIB_PATH}: {plib.lib().c3_version().decode()}")
    return pmodel.Clair3_F


def make(sd, cls=Clair3_F, policy=None):
    m = cls(add_indel_length=True, predict=True, input_channels=8).to("cuda:0")
    if policy:
        m.range_policy(policy)
    m.load_state_dict(sd)
    return m


sd = recipe_state_dict()
x = syn.make_fa_windows(B, seed=63)
xd = torch.from_numpy(x).cuda()

# ---- (c) first: fresh handles, the one wait that trips
print(f"== (c) the c3_predict_wait that trips, B = {B}: submit, then the wall time of wait; fresh handle each time, kinds alternating")
waits = {"recalibrate": [], "sticky": []}
for r in range(RUNS + 1):  # (the first round pays the process's first launches and is dropped)
    for kind in ("recalibrate", "sticky"):
        m = make(sd, policy="recalibrate" if kind == "recalibrate" else None)
        t = m.submit(x, slot=0)
        t0 = time.perf_counter()
        m.wait(t)
        el = (time.perf_counter() - t0) * 1e3
        if r:
            waits[kind].append(el)
        del m
for kind, v in waits.items():
    print(f"{kind:12s} wait: median {np.median(v):8.2f} ms  (min {min(v):.2f}, max {max(v):.2f})  runs: " + " ".join(f"{e:.2f}" for e in v))
print(f"   -> the recalibrating wait costs {np.median(waits['recalibrate']) - np.median(waits['sticky']):.2f} ms more than the sticky one, once")

# ---- (a), (b): the handles
healed = make(sd, policy="recalibrate")
y_healed_trip = healed.forward(xd, checked=True).cpu().numpy()  # the checked entry notices, recalibrates from these windows and stays on fp16x3
offline = make(sd)
offline.calibrate(x)
sticky = make(sd)
y_sticky = sticky.forward(xd, checked=True).cpu().numpy()
handles = [("healed online (recalibrate)", healed), ("calibrated offline, same batch", offline), ("sticky (fp32, this tree)", sticky)]
if PARENT:
    try:
        parent = make(sd, cls=parent_class(PARENT))
        y_parent = parent.forward(xd, checked=True).cpu().numpy()
        handles.append(("sticky (fp32, parent commit)", parent))
        print(f"rows of the trip, parent's sticky handle against this tree's: array_equal = {np.array_equal(y_parent, y_sticky)}")
    except Exception as e:  # noqa: BLE001
        print(f"parent checkout not usable ({e!r}): measured without it")
print(f"rows that answer the batch that tripped, healed against sticky: array_equal = {np.array_equal(y_healed_trip, y_sticky)}")
a, b = healed.calibration(), offline.calibration()
print(f"healed against offline: lowering equal = {np.array_equal(a['lowering'], b['lowering'])}, k equal = {np.array_equal(a['k'], b['k'])}, "
      f"census equal = {np.array_equal(a['census'], b['census'])}")
ya, yb = healed(xd).cpu().numpy(), offline(xd).cpu().numpy()
print(f"rows of the {B} windows on the product path, healed against offline: array_equal = {np.array_equal(ya, yb)}; against the fp32 forms: "
      f"max |dY| = {np.abs(ya - y_sticky).max():.3e}")
print(f"range stats of the healed handle: {healed.range_stats()}")
for name, m in handles:
    print(f"{name:32s} range_status={m.range_status()}  {m.describe()}")

print(f"== (a), (b) full alignment step time, B = {B}, device resident, one batch in flight; {RUNS} runs of {STEPS} steps per handle, handles alternating")
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
base = float(np.median(ms["calibrated offline, same batch"]))
for name, m in handles:
    med = float(np.median(ms[name]))
    print(f"{name:32s} median {med * 1e3:8.1f} us/step  (min {min(ms[name]) * 1e3:.1f}, max {max(ms[name]) * 1e3:.1f})  "
          f"{B / med:7.1f} k windows/s  x{med / base:.3f} of offline   runs: " + " ".join(f"{e * 1e3:.1f}" for e in ms[name]))
lo, hi = min(ms["calibrated offline, same batch"]), max(ms["calibrated offline, same batch"])
med = float(np.median(ms["healed online (recalibrate)"]))
print(f"   -> healed median {med * 1e3:.1f} us lies {'INSIDE' if lo <= med <= hi else 'OUTSIDE'} the run-to-run spread of the offline handle "
      f"[{lo * 1e3:.1f}, {hi * 1e3:.1f}] us")
for name, m in handles:
    print(f"{name:32s} range_status={m.range_status()}")
