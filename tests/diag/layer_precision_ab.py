#!/usr/bin/env python3
"""What a per-layer precision plan (c3_model_set_layer_precision) buys and costs, in one process on one MI355X: the sensitive pileup window's
error per plan (the table of profiles/r06_a_precision_escalation.txt, per plan), then the device-resident step time of the pileup network
at B = 1024 and of the full-alignment network at B = 256 with the plans alternating on one handle (median of RUNS runs of STEPS steps
each, one batch in flight) and the per-layer HIP-event times of c3_profile_read.  usage: layer_precision_ab.py [RUNS=9] [STEPS=100]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
for k in ("C3HIP_FP32", "C3HIP_FP32_LAYERS", "C3HIP_AUTO_FP32_LAYERS", "C3HIP_AUTO_FP32"):
    os.environ.pop(k, None)
import torch  # noqa: E402
from clair3_amd import synthetic as syn  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.test_parity_gpu import make_model  # noqa: E402
from tests.test_product_layers_gpu import _gx2  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100


def sensitive_window():
    seed, w = 925999917, 549
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=seed, peaked=False, trained_like=True)
    x = syn.make_pileup_windows(920, seed=seed, recipe="realistic")
    lo = w - w % 16
    xs, k = x[lo:lo + 16], w - lo
    y_o, d = oracle.pileup_forward(sd, xs, True, debug=True)
    d = dict(d)
    d["gx2"] = _gx2(sd, d["lstm1_out"])
    shapes = {"lstm1_out": (33, 256), "gx2": (33, 1280), "lstm2_out": (33, 320), "l4_out": (128,)}
    print(f"== sensitive window: trained-like weights seed {seed}, window {w} in its 16-window tile; errors against the fp64 oracle "
          f"(tile = all 16 windows, window = the sensitive one)")
    os.environ["C3HIP_FP32"] = "0"  # the load-time rule would move the whole handle: the plans are explicit here
    m = make_model(syn.PILEUP, 18, True, sd).tap(tuple(shapes))
    del os.environ["C3HIP_FP32"]
    for plan in ("", "lstm2", "proj2,lstm2", "lstm1,proj2,lstm2", "all"):
        m.layer_precision(plan)
        y = m.wait(m.submit(xs, slot=0))
        layers = "  ".join(f"{name} {np.abs(m.tap_fetch(name, 0, (16,) + s) - d[name]).max():.2e}" for name, s in shapes.items())
        print(f"plan {plan or 'none':18s} |Y - exact| tile {np.abs(y - y_o).max():.3e} window {np.abs(y[k] - y_o[k]).max():.3e}   {layers}")
    print(f"   ({m.describe()})")


def step_times(kind, ch, batch, plans, seed):
    sd = syn.make_state_dict(kind, ch, True, seed=seed)
    x = syn.make_windows(kind, batch, seed=seed + 1, channels=ch)
    m = make_model(kind, ch, True, sd)
    xd = torch.from_numpy(x).cuda()
    print(f"== {kind} step time, B = {batch}, device resident, one batch in flight; {RUNS} runs of {STEPS} steps per plan, plans alternating")
    ms = {p: [] for p in plans}
    forms = {}
    for r in range(RUNS + 1):  # (the first round warms every plan's kernels up and is dropped)
        for p in plans:
            m.layer_precision(p)
            m(xd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                m(xd)
            torch.cuda.synchronize()
            if r:
                ms[p].append((time.perf_counter() - t0) * 1e3 / STEPS)
            forms[p] = m.describe()
    base = float(np.median(ms[plans[0]]))
    for p in plans:
        med = float(np.median(ms[p]))
        print(f"plan {p or 'none':18s} median {med * 1e3:8.1f} us/step  (min {min(ms[p]) * 1e3:.1f}, max {max(ms[p]) * 1e3:.1f})  "
              f"{batch / med / 1e3:7.3f} M windows/s  x{med / base:.3f}")
    for p in plans:  # per layer: HIP events around every launch (the profiler serialises nothing else: one stream)
        m.layer_precision(p)
        m.profile(True)
        m.profile_reset()
        for _ in range(20):
            m(xd)
        torch.cuda.synchronize()
        recs = m.profile_read()
        m.profile(False)
        print(f"plan {p or 'none':18s} " + " ".join(f"{r['name']}={r['total_ms'] * 1e3 / max(1, r['launches']):.1f}" for r in recs) + " (us)")
    for p in plans:
        print(f"   plan {p or 'none'}: {forms[p]}")


sensitive_window()
step_times(syn.PILEUP, 18, 1024, ("", "lstm2", "proj2,lstm2", "lstm1,proj2,lstm2", "all"), 51)
step_times(syn.FULL_ALIGNMENT, 8, 256, ("", "res3a", "res2a,res2b", "all"), 41)
