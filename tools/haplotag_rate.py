"""Rates of haplotagging the reads (profiles/haplotag.txt): what the device form (c3_fa_haplotag + c3_fa_haplotag_result) and the host form
(c3_fa_haplotag_host, one core of the same box) make of synthetic read sets, host to host, and what the chained call c3_fa_reads_phased
is worth against c3_fa_haplotag_host followed by c3_fa_reads.

    timeout -k 10 600 python tools/haplotag_rate.py [--quick]

One job for the GPU box, under a limit of its own.  It needs a GPU and fails without one.

Shapes: 100 k sites at depth 30 and 150, reads of 5 000 bases (synthetic.make_read_set defaults), one het SNP per 1 000 and per 100 bases
(synthetic.make_phased_variants; phase sets of 20 000 bases), candidates every 10 sites for the chained call (matrix_depth 89).  Per shape,
a host clock around calls that end with the tags (or the windows' counts, depths and text) in host arrays, median of 3 after a warm-up:
  reads/s and pairs/s of both forms of the tag step, and the context's per-part times of the last device call;
  the chained device call against the host tags followed by the device window call: the same windows, with and without the tags
  being computed on one core and travelling to the device.
Every device answer is compared with the host form's.  The reference's own loop (src/clair3_full_alignment_dwell.c over htslib) cannot be
built where this runs, so the host form on one core is the yardstick.  No rate is a pass condition.  --quick: one tiny shape, for a
rehearsal without timing value.
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


def timed(fn, repeats=3):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    quick = "--quick" in sys.argv
    shapes = [(5_000, 30, 1000, 0.01)] if quick else [(100_000, depth, 5000, rate) for depth in (30, 150) for rate in (0.001, 0.01)]
    dev, host = fa.Context(0), fa.Context(None)
    for n_sites, depth, read_len, rate in shapes:
        t0 = time.perf_counter()
        rs0 = syn.make_read_set(n_sites, depth, read_len, seed=81)
        ex0 = syn.make_read_extras(rs0, 82)
        rs, ex = syn.sort_read_set(rs0), syn.sort_read_extras(rs0, ex0)
        v = syn.make_phased_variants(rs, 83, rate=rate, set_span=20_000)
        reads, variants = pr.ReadSet.from_dict(rs), fa.PhasedVariants.from_dict(v)
        ref, ref_first = rs["ref_bytes"], rs["ref_first"]
        print(f"\n== depth {depth}, one het SNP per {round(1 / rate)} bases: {len(reads)} reads of {read_len} bases, {len(rs['cigar'])} CIGAR ops, "
              f"{len(variants)} variants (made in {time.perf_counter() - t0:.1f} s)", flush=True)
        want = host.haplotag(reads, variants, ref, ref_first, path="host")
        want_pairs = host.haplotag_pairs()
        got = dev.haplotag(reads, variants, ref, ref_first, path="device")
        got_pairs = dev.haplotag_pairs()
        assert np.array_equal(got, want) and all(np.array_equal(a, b) for a, b in zip(got_pairs, want_pairs)), "the forms differ"
        n_pairs = len(want_pairs[1])
        s = host.haplotag_stats()
        print(f"   {n_pairs} pairs, {s['pairs_allele0']} with allele 0; tags 0 / 1 / 2: {s['reads_hap']}; both forms equal", flush=True)
        for label, ctx, path in (("device", dev, "device"), ("host, one core", host, "host")):
            med, lo, hi = timed(lambda: ctx.haplotag(reads, variants, ref, ref_first, path=path))
            print(f"   {label:28s} {med * 1e3:9.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})   {len(reads) / med / 1e3:9.1f} k reads/s "
                  f"{n_pairs / med / 1e6:8.2f} M pairs/s", flush=True)
        dev.haplotag(reads, variants, ref, ref_first, path="device")
        print("   device call by part, ms: " + ", ".join(f"{k} {x:.3f}" for k, x in dev.haplotag_stats()["kernel_ms"].items()), flush=True)
        # the chained call
        centres = np.arange(rs["start"], rs["end"], 10, dtype=np.int64)
        bare = fa.ReadExtras.from_dict({k: a for k, a in ex.items() if k != "haplotype"})

        def chained():
            return dev.run(reads, bare, centres, ref, ref_first, path="device", variants=variants)

        def host_tags_then_device():
            tags = host.haplotag(reads, variants, ref, ref_first, path="host")
            return dev.run(reads, fa.ReadExtras.from_dict(dict(ex, haplotype=tags)), centres, ref, ref_first, path="device")
        a = chained().fetch()
        b = host_tags_then_device().fetch()
        assert all(np.array_equal(a[k], b[k]) if k != "text" else a[k] == b[k] for k in ("rows", "counts", "depths", "text")), "the chains differ"
        assert not dev.stats()["fell_back"]
        print(f"   {len(centres)} candidates, {len(a['rows'])} rows; both chains equal", flush=True)
        for label, fn in (("chained (c3_fa_reads_phased)", chained), ("host tags + c3_fa_reads", host_tags_then_device)) * 2:
            med, lo, hi = timed(fn)
            print(f"   {label:28s} {med * 1e3:9.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})   {len(centres) / med / 1e3:9.1f} k windows/s", flush=True)
        chained()
        print("   chained call, tag step by part, ms: " + ", ".join(f"{k} {x:.3f}" for k, x in dev.haplotag_stats()["kernel_ms"].items()), flush=True)
        print("   chained call, window step by part, ms: " + ", ".join(f"{k} {x:.2f}" for k, x in dev.stats()["kernel_ms"].items()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
