"""Rates of the 9-channel windows with the dwell channel (profiles/fa_dwell.txt): what the dwell device call (c3_fa_reads_dwell +
c3_fa_reads_result) adds over the 8-channel device call of the same reads on the same box, what the host form (c3_fa_reads_dwell_host, one
core) makes of them, and the chained predict of a 9-channel model, host to host.

    timeout -k 10 900 python tools/dwell_rate.py [--quick]

One job for the GPU box, under a limit of its own.  It needs a GPU and fails without one.

Shapes: 100 k sites at depth 30 and 150, reads of 5 000 bases (synthetic.make_read_set defaults) with move tables of about 2.2 entries a
base (synthetic.make_read_moves), 10 k candidates (every tenth site) and 100 k (every site), matrix_depth 89.  Per shape, a host clock
around calls that end with rows, counts, depths and text in host arrays, median of 5 after a warm-up, the two device forms alternating:
  the dwell device call and the 8-channel device call (code of before the dwell channel: the yardstick), windows/s of both;
  c3_fa_reads_dwell_host on one core (the run that is compared is the warm-up; one timed run at 100 k candidates, three at 10 k);
  the chained predict of the 10 k shapes: the dwell call and c3_predict_fa_reads on a 9-channel model, nothing fetched but the rows y;
  the context's per-part times of the last dwell call, "moves_staged" and "dwell_table" among them, and the table kernel's share.
Every device answer is compared with the host form's.  No rate is a pass condition.  --quick: one tiny shape, for a rehearsal without
timing value.
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


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def line(label, t, n_cand):
    med = float(np.median(t))
    print(f"   {label:34s} {med * 1e3:10.2f} ms (min {min(t) * 1e3:.2f}, max {max(t) * 1e3:.2f}, {len(t)} runs)   {n_cand / med / 1e3:9.1f} k windows/s", flush=True)
    return med


def main():
    quick = "--quick" in sys.argv
    shapes = [(3_000, 30, 1000, (10,))] if quick else [(100_000, depth, 5000, (10, 1)) for depth in (30, 150)]
    dev, host = fa.Context(0), fa.Context(None)
    import torch  # noqa: F401  (the model's device)
    from clair3_amd.model import Clair3_F
    m = Clair3_F(add_indel_length=True, predict=True, input_channels=9)
    m.set_geometry(89, 33)
    m = m.to("cuda:0")
    m.eval()
    m.load_state_dict(syn.make_state_dict(syn.FULL_ALIGNMENT, 9, True, seed=7))
    for n_sites, depth, read_len, strides in shapes:
        t0 = time.perf_counter()
        rs0 = syn.make_read_set(n_sites, depth, read_len, seed=81)
        ex0 = syn.make_read_extras(rs0, 82)
        mv0 = syn.make_read_moves(rs0, ex0, 84)
        rs, ex, mv = syn.sort_read_set(rs0), syn.sort_read_extras(rs0, ex0), syn.sort_read_moves(rs0, mv0)
        reads, extras, moves = pr.ReadSet.from_dict(rs), fa.ReadExtras.from_dict(ex), fa.ReadMoves.from_dict(mv)
        ref, ref_first = rs["ref_bytes"], rs["ref_first"]
        print(f"\n== depth {depth}: {len(reads)} reads of {read_len} bases, {len(rs['cigar'])} CIGAR ops, {len(ex['qual'])} bases, "
              f"{len(mv['mv'])} move-table bytes ({len(mv['mv']) / max(len(ex['qual']), 1):.2f} a base; made in {time.perf_counter() - t0:.1f} s)", flush=True)
        for stride in strides:
            centres = np.arange(rs["start"], rs["end"], stride, dtype=np.int64)
            n = len(centres)

            def dwell():
                return dev.run(reads, extras, centres, ref, ref_first, path="device", moves=moves).fetch()

            def plain():
                return dev.run(reads, extras, centres, ref, ref_first, path="device").fetch()

            def on_host():
                return host.run(reads, extras, centres, ref, ref_first, path="host", moves=moves).fetch()

            t0 = time.perf_counter()
            want = on_host()
            warm = time.perf_counter() - t0
            got, got8 = dwell(), plain()
            assert all(np.array_equal(got[k], want[k]) if k != "text" else got[k] == want[k] for k in ("rows", "counts", "depths", "text")), "the forms differ"
            assert np.array_equal(got["rows"][:, :, :8], got8["rows"]) and not dev.stats()["fell_back"]
            print(f" - {n} candidates, {len(got['rows'])} rows of 297 bytes; device and host forms equal, channels 0 .. 7 equal to the 8-channel call's", flush=True)
            dwell(), plain()
            t9, t8 = [], []
            for _ in range(5):  # alternating: both see the same box in the same minute
                t9.append(clock(dwell)), t8.append(clock(plain))
            med9 = line("dwell device call (9 channels)", t9, n)
            med8 = line("8-channel device call (yardstick)", t8, n)
            t_host = [clock(on_host) for _ in range(1 if n > 20_000 else 3)] if not quick else [warm]
            med_h = line("c3_fa_reads_dwell_host, one core", t_host, n)
            print(f"   dwell call / 8-channel call {med9 / med8:.2f}; host form / dwell call {med_h / med9:.2f}", flush=True)
            dwell()
            parts = dev.stats()["kernel_ms"]
            print("   dwell call by part, ms: " + ", ".join(f"{k} {x:.2f}" for k, x in parts.items()), flush=True)
            print(f"   fa_dwell_kernel: {parts['dwell_table']:.2f} ms, {100 * parts['dwell_table'] / (med9 * 1e3):.1f} % of the call; staging the tables: "
                  f"{parts['moves_staged']:.2f} ms, {100 * parts['moves_staged'] / (med9 * 1e3):.1f} %", flush=True)
            if n <= 20_000:
                def chained():
                    dev.run(reads, extras, centres, ref, ref_first, path="device", moves=moves)
                    return m.predict_reads(dev)

                y = chained()
                assert np.array_equal(y.view(np.uint32), m.predict_rows(got["rows"], got["counts"]).view(np.uint32)), "the chained rows differ"
                chained()
                line("dwell call + chained predict", [clock(chained) for _ in range(5)], n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
