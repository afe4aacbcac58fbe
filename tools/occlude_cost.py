"""Cost of occlusion mode (profiles/occlude_mode.txt): 256 realistic full-alignment windows (C = 8, indel heads, K = 41 variants a window at
band 1) and 1024 realistic pileup windows (int8, K = 51), one handle each, decoder columns on -- wall time and variants per second of the
call next to the same variants built on the host (synthetic.occlude_variants) and pushed through predict_numpy on the same handle, the two
alternated, three pairs; the device time of the two new launches; the bytes staged against the bytes of the host-built alternative; and the
pass sizes (C3HIP_OCCLUDE_CHUNK) that were tried.

    python tools/occlude_cost.py [fa_windows [pileup_windows]]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clair3_amd import synthetic as syn  # noqa: E402
from clair3_amd.model import Clair3_F, Clair3_P  # noqa: E402

B_FA = int(sys.argv[1]) if len(sys.argv) > 1 else 256
B_P = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
PAIRS = 3


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def one_kind(name, m, x, chunks):
    os.environ.pop("C3HIP_OCCLUDE_CHUNK", None)
    r = m.occlude(x)  # warm-up: workspace, buffers, the kernels' load
    K = r["channels"] + r["bands"]
    variants, dense = len(x) * K, len(x) * (K + 1)
    print(f"== {name}: {len(x)} windows, K = {K}, {variants} variants, {dense} dense windows a call; rows of {m.row_size} floats", flush=True)
    t0 = time.perf_counter()
    v = syn.occlude_variants(x)
    build = time.perf_counter() - t0
    m.predict_numpy(v)
    for p in range(PAIRS):
        t0 = time.perf_counter()
        r = m.occlude(x)
        t1 = time.perf_counter()
        y = m.predict_numpy(v)
        t2 = time.perf_counter()
        print(f"pair {p}: occlude {1e3 * (t1 - t0):.2f} ms = {variants / (t1 - t0) / 1e3:.0f} k variants/s, {r['passes']} passes, expand "
              f"{r['expand_us']:.1f} us and reduce {r['reduce_us']:.1f} us a call, {r['bytes_staged']} bytes staged   |   predict_numpy of the {variants} "
              f"host-built variants {1e3 * (t2 - t1):.2f} ms = {variants / (t2 - t1) / 1e3:.0f} k variants/s shipping {v.nbytes} bytes", flush=True)
    print(f"host-built: occlude_variants {build:.3f} s; with the build {variants / (build + t2 - t1) / 1e3:.1f} k variants/s", flush=True)
    print(f"bytes: device path {r['bytes_staged']} against {v.nbytes + x.nbytes} host-built = 1 : {(v.nbytes + x.nbytes) / r['bytes_staged']:.1f}", flush=True)
    full = m.occlude(x, drops=True, variant_rows=True)
    rec, drops = syn.occlude_records(full["base_rows"], full["variant_rows"], full["channels"], full["bands"], m.output_size)
    print(f"variant rows bit-identical to the host-built ones: {same(full['variant_rows'], y)}; records and drops equal the numpy rule: "
          f"{all(np.array_equal(full['rows'][k], rec[k]) for k in rec.dtype.names) and same(full['drops'], drops)}", flush=True)
    # the pass size: the same call under other cuts, best of three
    for chunk in chunks:
        os.environ["C3HIP_OCCLUDE_CHUNK"] = str(chunk)
        m.occlude(x)
        best, passes = None, 0
        for _ in range(3):
            t0 = time.perf_counter()
            passes = m.occlude(x)["passes"]
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print(f"C3HIP_OCCLUDE_CHUNK={chunk}: {passes} passes, best of three {1e3 * best:.2f} ms = {variants / best / 1e3:.0f} k variants/s", flush=True)
    os.environ.pop("C3HIP_OCCLUDE_CHUNK", None)
    rec = full["rows"]
    heads = len(syn.head_slices(m.output_size))
    print(f"synthetic weights: windows with a head flip by a channel {int((rec['flips'][:, 0] > 0).any(axis=1).sum())}, by a band "
          f"{int((rec['flips'][:, 1] > 0).any(axis=1).sum())} of {len(x)}; the channel most often the lean of head 0: "
          f"{int(np.bincount(np.clip(rec['lean'][:, 0, 0], 0, None)).argmax())}, the band: {int(np.bincount(np.clip(rec['lean'][:, 1, 0], 0, None)).argmax())}; "
          f"largest max_delta {float(rec['max_delta'].max()):.3g} ({heads} heads)", flush=True)


f = Clair3_F(add_indel_length=True, predict=True, input_channels=8).to("cuda:0")
f.load_state_dict(syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7))
f.decode_columns(True)
one_kind("full alignment", f, syn.make_fa_windows(B_FA, seed=8), (16, 32, 48, 64, 128, 0))

p = Clair3_P(add_indel_length=True, predict=True).to("cuda:0")
p.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, True, seed=7))
p.decode_columns(True)
one_kind("pileup", p, syn.make_pileup_windows(B_P, seed=8), (64, 128, 256, 315, 512, 0))
