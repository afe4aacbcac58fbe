"""Cost of gVCF mode (profiles/gvcf_blocks.txt): sites per second host to host of Context.blocks_from_counts and blocks_from_region at 1 M
and 5 M sites on three depth shapes (depth 0 everywhere: one block; constant 30; Poisson(30) with binomial reference counts), median of 5
calls after a warm-up, a host clock around calls that end in a device-to-host copy; the sequential C rule (c3_gvcf_blocks_host) on one
core on the same inputs; and the reference's own loop (make_gvcf_online of preprocess/utils.py, Python math, writing into memory) on a
200 k-site slice where the reference is staged.  Every device answer is compared with the C rule's.

    python tools/gvcf_cost.py                 the table
    python tools/gvcf_cost.py --trace SITES   three calls on Poisson(30) at SITES sites and nothing else: the run to put behind
                                              rocprofv3 --kernel-trace --stats
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clair3_amd import gvcf  # noqa: E402
from clair3_amd import synthetic as syn  # noqa: E402

REPEATS = 5
SLICE = 200_000


def shape(name, n, seed=11):
    rng = np.random.default_rng(seed)
    if name == "depth 0":
        t = np.zeros(n, np.int64)
        a = t.copy()
    elif name == "constant 30":
        t = np.full(n, 30, np.int64)
        a = t.copy()
    else:
        t = rng.poisson(30, size=n).astype(np.int64)
        a = rng.binomial(t, 0.98).astype(np.int64)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n)
    return a, t, ref


def region_of(a, t, ref):
    """a region matrix with these counts: the difference on one alternative base"""
    n = len(t)
    up = ref & 0xDF
    r = np.select([up == ord("C"), up == ord("G"), up == ord("T")], [1, 2, 3], 0)
    m = np.zeros((n, 18), np.int32)
    rows = np.arange(n)
    k = (r + 1) % 4
    m[rows, k] = t - a
    m[rows, r] = -((a + 1) // 2 + (t - a))
    m[rows, 9 + r] = -(a // 2)
    return m, rows.astype(np.int64)


def median_time(fn):
    fn()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def reference_loop(a, t, ref):
    """seconds of the reference's own make_gvcf_online over the sites (None where the reference is not staged)"""
    sys.path.insert(0, os.path.join(ROOT))
    from tests import gvcf_cases as gc
    import tempfile
    with gc.reference_utils() as U:
        if U is None:
            return None
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            gc.run_producer_loop(U.variantInfoCalculator, tmp, a, t, ref, 1)
            return time.perf_counter() - t0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        n = int(sys.argv[2])
        a, t, ref = shape("Poisson(30)", n)
        with gvcf.Context() as c:
            for _ in range(3):
                b = c.blocks_from_counts(a, t, ref, 1)
        print(f"{n} sites, {len(b)} records")
        return
    with gvcf.Context() as c:
        for n in (1_000_000, 5_000_000):
            for name in ("depth 0", "constant 30", "Poisson(30)"):
                a, t, ref = shape(name, n)
                m, major = region_of(a, t, ref)
                host = [None]

                def run_host():
                    host[0] = gvcf.blocks_host(a, t, ref, 1)
                t_host = median_time(run_host)
                got = [None]

                def run_counts():
                    got[0] = c.blocks_from_counts(a, t, ref, 1)
                t_counts = median_time(run_counts)
                same = len(got[0]) == len(host[0]) and got[0].tobytes() == host[0].tobytes()

                def run_region():
                    got[0] = c.blocks_from_region(m, major, ref, 0, n, 1)
                t_region = median_time(run_region)
                same = same and got[0].tobytes() == host[0].tobytes()
                print(f"{n:>8} sites  {name:<12} records {len(host[0]):>8}  counts form {t_counts * 1e3:8.2f} ms {n / t_counts / 1e6:8.1f} M sites/s   "
                      f"region form {t_region * 1e3:8.2f} ms {n / t_region / 1e6:8.1f} M sites/s   C rule, one core {t_host * 1e3:8.2f} ms "
                      f"{n / t_host / 1e6:8.1f} M sites/s   identical: {same}", flush=True)
                if not same:
                    raise SystemExit("the device records differ from the C rule's")
    for name in ("depth 0", "constant 30", "Poisson(30)"):
        a, t, ref = shape(name, SLICE)
        s = reference_loop(a, t, ref)
        print(f"reference make_gvcf_online, {SLICE} sites, {name:<12} " + ("not staged" if s is None else f"{s:8.2f} s  {SLICE / s / 1e6:8.3f} M sites/s"), flush=True)


if __name__ == "__main__":
    main()
