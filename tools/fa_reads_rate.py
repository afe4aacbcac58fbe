"""Rates of full alignment from reads (profiles/fa_reads.txt): what the device form (c3_fa_reads + c3_fa_reads_result) and the host form
(c3_fa_reads_host, one core of the same box) make of synthetic read sets, host to host, and what the chained predict is worth.

    timeout -k 10 900 python tools/fa_reads_rate.py [--quick]

One job for the GPU box, under a limit of its own.  It needs a GPU and fails without one.

Shapes: 10 k and 100 k candidates, one every 10 sites, at depth 30 and 150 (matrix_depth 89), reads of 5 000 bases
(synthetic.make_read_set defaults: 1 % substitutions, 0.4 % insertions and deletions each, 3 % variant sites; make_read_extras: qualities,
60 % of the reads phased).  A set of 100 k sites is generated and, for 100 k candidates, laid end to end 10 times
(synthetic.tile_read_set), so reads that reach over a seam double the depth there.  Per shape, a host clock around calls that end with the
result in host arrays (median of 3 after a warm-up; the host form once at 100 k candidates):
  windows/s of both forms; "device, held" is c3_fa_reads alone: rows stay on the device (what a caller of the chained entry pays), the
  counts, centre depths and text come back;
  the context's per-kernel times of the last device call (device events around each launch group);
  windows/s of c3_predict_fa_reads against c3_fa_reads_result followed by c3_predict_rows on the same held result: the same rows, with and
  without the windows travelling to the host and back.
Every device answer is compared with the host form's.  The reference's own loop (src/clair3_full_alignment_dwell.c over htslib) cannot be
built where this runs, so the host form on one core is the yardstick.  --quick: one tiny shape, for a rehearsal without timing value.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clair3_amd import fa_reads as fa  # noqa: E402
from clair3_amd import pileup_reads as pr  # noqa: E402
from clair3_amd import synthetic as syn  # noqa: E402

KEYS = ("rows", "counts", "depths", "text")


def timed(fn, repeats):
    if repeats > 1:
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    quick = "--quick" in sys.argv
    from clair3_amd.model import Clair3_F
    m = Clair3_F(add_indel_length=True, predict=True, input_channels=8)
    m.to("cuda:0")
    m.eval()
    m.load_state_dict(syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=7))
    shapes = [("tiny", 5_000, 1, 30, 1000)] if quick else [("10 k candidates, depth 30", 100_000, 1, 30, 5000), ("100 k candidates, depth 30", 100_000, 10, 30, 5000),
                                                           ("10 k candidates, depth 150", 100_000, 1, 150, 5000), ("100 k candidates, depth 150", 100_000, 10, 150, 5000)]
    dev, host = fa.Context(0), fa.Context(None)
    for name, base, copies, depth, read_len in shapes:
        t0 = time.perf_counter()
        rs0 = syn.tile_read_set(syn.make_read_set(base, depth, read_len, seed=71), copies)
        ex0 = syn.make_read_extras(rs0, 72)
        rs, ex = syn.sort_read_set(rs0), syn.sort_read_extras(rs0, ex0)
        reads, extras = pr.ReadSet.from_dict(rs), fa.ReadExtras.from_dict(ex)
        centres = np.arange(rs["start"], rs["end"], 10, dtype=np.int64)
        args = (reads, extras, centres, rs["ref_bytes"], rs["ref_first"])
        print(f"\n== {name}: {len(centres)} candidates over {rs['end'] - rs['start']} sites, {len(reads)} reads, {len(rs['cigar'])} CIGAR ops "
              f"(made in {time.perf_counter() - t0:.1f} s)", flush=True)
        big = len(centres) > 20_000
        t0 = time.perf_counter()
        want = host.run(*args).fetch()
        host_once = time.perf_counter() - t0
        got = dev.run(*args).fetch()
        for k in KEYS:
            assert np.array_equal(got[k], want[k]) if k != "text" else got[k] == want[k], f"{name}: {k} differs between the forms"
        s = dev.stats()
        assert not s["fell_back"]
        print(f"   {len(want['rows'])} rows, {s['deep_windows']} windows deeper than 89, {len(want['text'])} bytes of text; both forms equal", flush=True)
        del got
        for label, ctx, repeats, fetch in (("device", dev, 3, True), ("device, held", dev, 3, False), ("host, one core", host, 1 if big else 3, True)):
            if label.startswith("host") and big:
                med = lo = hi = host_once
            else:
                med, lo, hi = timed((lambda: ctx.run(*args).fetch()) if fetch else (lambda: ctx.run(*args)), repeats)
            print(f"   {label:15s} {med * 1e3:9.1f} ms (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})   {len(centres) / med / 1e3:9.1f} k windows/s", flush=True)
        dev.run(*args)
        print("   device call by part, ms: " + ", ".join(f"{k} {v:.2f}" for k, v in dev.stats()["kernel_ms"].items()), flush=True)
        chained = lambda: m.predict_reads(dev)  # noqa: E731

        def round_trip():
            f = dev.fetch()
            return m.predict_rows(f["rows"], f["counts"])
        a, b = chained(), round_trip()
        assert a.tobytes() == b.tobytes()
        for label, fn in (("chained", chained), ("fetch + rows", round_trip), ("chained", chained), ("fetch + rows", round_trip)):
            med, lo, hi = timed(fn, 3)
            print(f"   {label:15s} {med * 1e3:9.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})   {len(a) / med / 1e3:9.1f} k windows/s", flush=True)
        del want
    return 0


if __name__ == "__main__":
    sys.exit(main())
