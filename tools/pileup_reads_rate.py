"""Rates of pileup from reads (profiles/pileup_reads.txt): what the device form (c3_pileup_reads + c3_pileup_result) and the host form
(c3_pileup_reads_host, one core of the same box) make of synthetic read sets, host to host, and what the chained entry is worth.

    timeout -k 10 540 python tools/pileup_reads_rate.py [--quick]

One job for the GPU box, under a limit of its own: about 25 s of run time on one MI355X (three read sets are made, 4 s; every timed
call ends in a synchronise), plus the start of the interpreter and the library.  It needs a GPU and fails without one.

Shapes: 1 M and 5 M sites at depth 30 and 1 M sites at depth 150, reads of 5 000 bases (synthetic.make_read_set defaults: 1 % substitutions,
0.4 % insertions and deletions each, 3 % variant sites).  A set of 250 k sites is generated and laid end to end 4 or 20 times
(synthetic.tile_read_set), so reads that reach over a seam double the depth there; nothing else is special about the seams.
Per shape, median of 5 calls after a warm-up (3 for the host form), a host clock around calls that end with the result in host arrays:
  sites/s and read-bases/s of both forms (read-bases: M, =, X, I, S bases of all reads, kept or not); "device, held" is c3_pileup_reads
  alone: the matrix, major and the count pair stay on the device (what a caller of the chained entry pays), the text is built;
  the context's per-kernel times of the last device call (device events around each launch group);
  windows/s of c3_predict_pileup_reads against c3_pileup_result followed by c3_predict_pileup_candidates on the same held result: the
  same rows, with and without the region matrix travelling to the host and back.
Every device answer is compared with the host form's.  The reference's own loop (src/clair3_pileup.c over htslib) cannot be built where
this runs, so the host form on one core is the yardstick; the form that privatises a tile of positions in LDS was not built, so there is
no number for it.  --quick: one tiny shape, for a rehearsal without timing value.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clair3_amd import pileup_reads as pr  # noqa: E402
from clair3_amd import synthetic as syn  # noqa: E402

CFG = dict(min_snp_af=0.08, min_indel_af=0.15)
KEYS = ("counts", "major", "cand_pos", "cand_depth", "n_ref", "n_total", "text")


def median_time(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def read_bases(rs):
    op, n = rs["cigar"] & 15, rs["cigar"] >> 4
    return int(n[np.isin(op, (0, 1, 4, 7, 8))].sum())


def main():
    quick = "--quick" in sys.argv
    from clair3_amd.model import Clair3_P
    m = Clair3_P(add_indel_length=False, predict=True, input_channels=18)
    m.to("cuda:0")
    m.eval()
    m.load_state_dict(syn.make_state_dict(syn.PILEUP, 18, False, seed=7))
    shapes = [("tiny", 20_000, 1, 30, 1000)] if quick else [("1 M sites, depth 30", 250_000, 4, 30, 5000), ("5 M sites, depth 30", 250_000, 20, 30, 5000),
                                                             ("1 M sites, depth 150", 250_000, 4, 150, 5000)]
    dev, host = pr.Context(0), pr.Context(None)
    for name, base, copies, depth, read_len in shapes:
        t0 = time.perf_counter()
        rs = syn.tile_read_set(syn.make_read_set(base, depth, read_len, seed=61), copies)
        reads = pr.ReadSet.from_dict(rs)
        n_sites, bases = rs["end"] - rs["start"], read_bases(rs)
        args = (reads, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"])
        print(f"\n== {name}: {n_sites} sites, {len(reads)} reads, {len(rs['cigar'])} CIGAR ops, {bases} read bases (made in {time.perf_counter() - t0:.1f} s)")
        want = host.run(*args, **CFG).fetch()
        got = dev.run(*args, **CFG).fetch()
        for k in KEYS:
            assert np.array_equal(got[k], want[k]) if k != "text" else got[k] == want[k], f"{name}: {k} differs between the forms"
        s = dev.stats()
        assert not s["fell_back"]
        print(f"   {len(want['major'])} columns, {len(want['cand_pos'])} candidates, {s['events']} indel events, {len(want['text'])} bytes of text; both forms equal")
        for label, ctx, repeats, fetch in (("device", dev, 5, True), ("device, held", dev, 5, False), ("host, one core", host, 3, True)):
            med, lo, hi = median_time((lambda: ctx.run(*args, **CFG).fetch()) if fetch else (lambda: ctx.run(*args, **CFG)), repeats)
            print(f"   {label:15s} {med * 1e3:9.1f} ms (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})   {n_sites / med / 1e6:8.2f} M sites/s   {bases / med / 1e6:9.1f} M read-bases/s")
        dev.run(*args, **CFG)
        ms = dev.stats()["kernel_ms"]
        print("   device call by part, ms: " + ", ".join(f"{k} {v:.2f}" for k, v in ms.items()))
        # the chained entry against the host round trip, on the held result
        r = dev.fetch()
        chained = lambda: m.predict_reads(dev)  # noqa: E731
        def round_trip():
            f = dev.fetch()
            return m.predict_candidates(f["counts"], f["major"], f["cand_pos"], depths=f["cand_depth"])
        rows_a, status_a = chained()
        rows_b, status_b = round_trip()
        assert rows_a.tobytes() == rows_b.tobytes() and np.array_equal(status_a, status_b)
        for label, fn in (("chained", chained), ("fetch + candidates", round_trip), ("chained", chained), ("fetch + candidates", round_trip)):
            med, lo, hi = median_time(fn, 5)
            print(f"   {label:19s} {med * 1e3:8.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})   {len(rows_a)} windows of {len(r['cand_pos'])} candidates   {len(rows_a) / med / 1e6:.3f} M windows/s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
