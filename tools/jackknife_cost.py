"""Cost of jackknife mode (profiles/jackknife_mode.txt): 256 full-alignment windows of realistic read counts, C = 8, indel heads, one handle --
variants per second through c3_jackknife_rows next to windows per second of c3_predict_rows over the same number of dense windows, the two
alternated, three pairs; the device time of the two new launches per pass; the bytes staged against the host-built alternative
(synthetic.leave_one_out + predict_numpy), which is timed in the same job.

    python tools/jackknife_cost.py [windows]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clair3_amd import synthetic as syn  # noqa: E402
from clair3_amd.model import Clair3_F  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
PAIRS = 3

m = Clair3_F(add_indel_length=True, predict=True, input_channels=8).to("cuda:0")
m.load_state_dict(syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7))
m.decode_columns(True)
x = syn.make_fa_windows(B, seed=8)
rows, firsts, counts = syn.pack_fa_rows(x)
variants = int(counts.sum())
dense = B + variants
print(f"{B} windows, {variants} reads (mean {variants / B:.1f} a window), {dense} dense windows a call; rows of {m.row_size} floats", flush=True)

# the same number of dense windows as plain rows batches: the call's own windows repeated
reps = -(-dense // B)
plain_rows, plain_counts = np.concatenate([rows] * reps), np.concatenate([counts] * reps)
keep = dense
plain_counts = plain_counts[:keep]
plain_rows = plain_rows[:int(plain_counts.sum())]

r = m.jackknife_rows(rows, counts)  # warm-up: workspace, buffers, the kernels' load
m.predict_rows(plain_rows, plain_counts)
for p in range(PAIRS):
    t0 = time.perf_counter()
    r = m.jackknife_rows(rows, counts)
    t1 = time.perf_counter()
    m.predict_rows(plain_rows, plain_counts)
    t2 = time.perf_counter()
    print(f"pair {p}: jackknife_rows {t1 - t0:.4f} s = {variants / (t1 - t0) / 1e3:.0f} k variants/s ({dense / (t1 - t0) / 1e3:.0f} k dense windows/s), "
          f"{r['passes']} passes, expand {r['expand_us'] / r['passes']:.1f} us and reduce {r['reduce_us'] / r['passes']:.1f} us per pass, "
          f"{r['bytes_staged']} bytes staged   |   predict_rows of {keep} windows {t2 - t1:.4f} s = {keep / (t2 - t1) / 1e3:.0f} k windows/s "
          f"({int(plain_counts.sum()) * 33 * 8} bytes of rows)", flush=True)

# the host-built alternative: every variant dense, built in numpy and shipped
t0 = time.perf_counter()
v = syn.leave_one_out(rows, counts)
t1 = time.perf_counter()
y = m.predict_numpy(v)
t2 = time.perf_counter()
y = m.predict_numpy(v)
t3 = time.perf_counter()
print(f"host-built: leave_one_out {t1 - t0:.3f} s, predict_numpy of {len(v)} dense windows {t3 - t2:.4f} s (first call {t2 - t1:.4f} s) = "
      f"{len(v) / (t3 - t2) / 1e3:.0f} k variants/s shipping {v.nbytes} bytes; with the build {len(v) / (t3 - t2 + t1 - t0) / 1e3:.1f} k variants/s", flush=True)
print(f"bytes: device path {r['bytes_staged']} against {v.nbytes + x.nbytes} host-built = 1 : {(v.nbytes + x.nbytes) / r['bytes_staged']:.1f}", flush=True)
full = m.jackknife_rows(rows, counts, variant_rows=True)
print(f"variant rows bit-identical to the host-built ones: {np.array_equal(full['variant_rows'].view(np.uint32), y.view(np.uint32))}", flush=True)
rec = full["rows"]
flips = (rec["flips"] > 0).any(axis=1) | (rec["decision_flips"] > 0).any(axis=1)
near = np.zeros(B, bool)
near[syn.refine_select(full["base_rows"], 90, 1e-4)[0]] = True
print(f"synthetic weights: {int(flips.sum())} of {B} windows have a variant that flips a label; within 1e-4 of a tie {int(near.sum())}, of which "
      f"{int((near & flips).sum())} flip; largest max_delta {float(rec['max_delta'].max()):.3g}", flush=True)
