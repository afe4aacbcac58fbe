"""Cost of subsample mode (profiles/subsample_mode.txt): 256 full-alignment windows of realistic read counts, C = 8, indel heads, one handle, the
default plan (depths 10, 20, 30, 40; 8 replicates) -- variants per second through c3_subsample_rows next to the SAME variants built on the
host (synthetic.subsample_variants) and pushed through the plain handle as dense windows (predict_numpy), the two alternated, three pairs;
the device time of the two new launches per pass; the bytes staged by either path.

    python tools/subsample_cost.py [windows]
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
DEPTHS, R, SEED = (10, 20, 30, 40), 8, 0

m = Clair3_F(add_indel_length=True, predict=True, input_channels=8).to("cuda:0")
m.load_state_dict(syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7))
m.decode_columns(True)
x = syn.make_fa_windows(B, seed=8)
rows, firsts, counts = syn.pack_fa_rows(x)
variants = int(syn.subsample_variant_counts(counts, DEPTHS, R).sum())
print(f"{B} windows, {int(counts.sum())} reads (mean {counts.mean():.1f} a window), {variants} variants, {B + variants} dense windows a call; "
      f"rows of {m.row_size} floats", flush=True)

t0 = time.perf_counter()
v = syn.subsample_variants(rows, counts, None, DEPTHS, R, SEED)
t_build = time.perf_counter() - t0
dense = np.concatenate([x, v])  # what a caller without the mode ships: the windows and every variant, dense

r = m.subsample_rows(rows, counts, depths=DEPTHS, replicates=R, seed=SEED)  # warm-up: workspace, buffers, the kernels' load
y = m.predict_numpy(dense)
for p in range(PAIRS):
    t0 = time.perf_counter()
    r = m.subsample_rows(rows, counts, depths=DEPTHS, replicates=R, seed=SEED)
    t1 = time.perf_counter()
    y = m.predict_numpy(dense)
    t2 = time.perf_counter()
    print(f"pair {p}: subsample_rows {t1 - t0:.4f} s = {variants / (t1 - t0) / 1e3:.0f} k variants/s, {r['passes']} passes, "
          f"expand {r['expand_us'] / r['passes']:.1f} us and reduce {r['reduce_us'] / r['passes']:.1f} us per pass, {r['bytes_staged']} bytes staged   |   "
          f"predict_numpy of the {len(dense)} dense windows {t2 - t1:.4f} s = {variants / (t2 - t1) / 1e3:.0f} k variants/s "
          f"({dense.nbytes} bytes shipped)", flush=True)
print(f"host build of the variants (numpy, not part of the pairs): {t_build:.3f} s; bytes: device path {r['bytes_staged']} against {dense.nbytes} = "
      f"1 : {dense.nbytes / r['bytes_staged']:.1f}", flush=True)
full = m.subsample_rows(rows, counts, depths=DEPTHS, replicates=R, seed=SEED, masks=True, variant_rows=True)
print(f"variant rows bit-identical to the host-built ones: {np.array_equal(full['variant_rows'].view(np.uint32), y[B:].view(np.uint32))}; "
      f"masks equal the numpy rule's: {np.array_equal(full['masks'], syn.subsample_masks(counts, DEPTHS, R, SEED, 89))}", flush=True)
lev, win = full["levels"], full["rows"]
print(f"synthetic weights: windows run per level {(lev['run'] > 0).sum(axis=0).tolist()}, with a head flip {(lev['flips'] > 0).any(axis=2).sum(axis=0).tolist()}, "
      f"with a decision flip {(lev['decision_flips'] > 0).sum(axis=0).tolist()}; hold_level of the genotype head "
      f"{[int((win['hold_level'][:, 1] == l).sum()) for l in range(len(DEPTHS) + 1)]}", flush=True)
