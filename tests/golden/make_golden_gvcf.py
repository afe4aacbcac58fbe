#!/usr/bin/env python3
"""Golden non-variant gVCF records of the REAL reference class: preprocess/utils.py variantInfoCalculator (reference_likelihood,
make_gvcf_online, write_to_gvcf_batch, write_to_gvcf, write_empty_pileup), driven the way the pileup producer drives it
(preprocess/CreateTensorPileupFromCffi.py:399-441).

Run in the build container only (needs the reference checkout, like make_golden_candidates.py):

    python tests/golden/make_golden_gvcf.py

The reference's own class runs, not a transcription of it.  cffi is not installed here: a stand-in ``cffi`` module whose FFI().verify
raises is put into sys.modules, so mathcalculator takes its own Python definitions (speedUp = False) -- the only well-defined path
anyway, since the inline C getMyMaxItem reads one element past its array.  The class is run twice in fresh processes, once with mpmath
importable (preprocess/utils.py then computes with mpmath's 53-bit numbers) and once with it masked (Python's math); the two results
must agree before anything is written.

tests/golden/gvcf_blocks.npz holds
  (a) the site table: gq, binned_gq, validPL and the three PLs for every n_ref <= n_total <= 300 at base_err 0.001 / bin 5, and for
      n_total <= 64 at base_err 0.01 / bin 10 (pair (n_total, n_ref) at n_total * (n_total + 1) / 2 + n_ref);
  (b) a region of a few thousand sites (make_region) with the per-site items the reference made of it, its lines with bp_resolution
      off and on, and the records parsed back from those lines;
  (c) a contig-end case (the last sites of the contig: END == contig_len - 1 prints contig_len) and an all-zero region
      (write_empty_pileup).
conditions() counts the cases that keep (b) from being easy; it is asserted here and again in tests/test_gvcf.py on the committed file.
"""
import io
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gvcf_blocks.npz")

CTG = "chrG"
CONTIG_LEN = 60000
REGION_SEED = 2511
REGION_FIRST = 20001
TABLES = ((0.001, 5, 300), (0.01, 10, 64))
MIN_PER_CONDITION = 8
LONG_BLOCK = 600


def make_region():
    """(n_ref, n_total int64, ref bytes): segments laid end to end so that every branch of make_gvcf_online fires (conditions())"""
    rng = np.random.default_rng(REGION_SEED)
    nr, nt, ref = [], [], []

    def add(total, refc, bases=None):
        total, refc = np.atleast_1d(total).astype(np.int64), np.atleast_1d(refc).astype(np.int64)
        nt.extend(total.tolist()), nr.extend(refc.tolist())
        ref.extend(bases if bases is not None else rng.choice(list(b"ACGT"), size=len(total)).tolist())

    def flat(n, d, bases=None):
        add(np.full(n, d), np.full(n, d), bases)

    for k in range(9):
        flat(LONG_BLOCK + 5 + 7 * k, 30 + k)             # a long block at gq 50
        flat(3, 40 + 2 * k + 12)                         # an upward DP break: f(30 + k) < 52 + 2k
        flat(4, 31 + k)                                  # and a downward one behind it
        flat(2, 30), flat(2, 39), flat(2, 30)            # a maximum absorbed: f(30) = 39
        flat(2, 30), flat(2, 24), flat(2, 30)            # a minimum absorbed: f(24) = 32 >= 30
        flat(2, 22)                                      # a minimum that breaks: f(22) = 29 < 30
        add(np.full(3 + k % 3, 20), np.full(3 + k % 3, 2))   # a ./. run: written item by item
        flat(5, 30)
        flat(2 + k, 0)                                   # a depth-0 run
        flat(3, 3), flat(2, 6), flat(2, 30)              # other gq bins
        flat(4 + k % 2, 30, [ord("N")] * (4 + k % 2))    # an N run: a break by N status in front and behind, a block whose first item is N
        flat(3, 30)
        flat(3, 30, [ord("a"), ord("c"), ord("g")])      # lower case: printed as N, not an N for the break
        flat(3, 30, [ord("R"), ord("Y"), ord("N")])      # IUPAC, then N: a break by N status inside a stretch of binned_gq 1
        flat(2, 1, [ord("n"), ord("A")])
        add(np.full(2, 20), np.full(2, 2), [ord("N"), ord("N")])  # ./. by the counts, N by the base: one block, not items
        n = 40
        total = rng.poisson(30, size=n)
        add(total, rng.binomial(total, 0.97))
        total = rng.poisson(6, size=n)
        add(total, rng.binomial(total, 0.8))
    return np.array(nr, np.int64), np.array(nt, np.int64), bytes(ref)


def conditions(z):
    """how often each case occurs in fixture (b), from what the file holds: the per-site items the reference made (item_gq, item_binned,
    item_gt), the counts, the raw bytes, and the records of its lines"""
    total, raw = z["b_n_total"].astype(np.int64), bytes(z["b_ref"].tobytes())
    binned, gt = z["b_item_binned"], z["b_item_gt"]
    n = len(total)
    c = dict(break_bin=0, break_gt=0, break_n=0, dp_break_down=0, dp_break_up=0, dp_absorb_down=0, dp_absorb_up=0, per_site_run=0,
             lower_case=0, iupac=0, first_n_block=0, depth0_run=0, long_block=0)
    f = lambda x: int(np.ceil(x + x * 0.3))
    s = 0
    starts = [0]
    mn = mx = int(total[0])
    for i in range(1, n):
        d = int(total[i])
        new = True
        if binned[i] != binned[s]:
            c["break_bin"] += 1
        elif gt[i] != gt[s]:
            c["break_gt"] += 1
        elif (raw[i] == ord("N")) != (raw[i - 1] == ord("N")):
            c["break_n"] += 1
        elif d < mn:
            if mx > f(d):
                c["dp_break_down"] += 1
            else:
                c["dp_absorb_down"] += 1
                mn, new = d, False
        elif d > mx:
            if d <= f(mn):
                c["dp_absorb_up"] += 1
                mx, new = d, False
            else:
                c["dp_break_up"] += 1
        else:
            new = False
        if new:
            s, mn, mx = i, d, d
            starts.append(i)
    lines = 0
    for s, e in zip(starts, starts[1:] + [n]):
        acgt = raw[s] in b"ACGT"
        c["per_site_run"] += int(not gt[s] and acgt)
        c["first_n_block"] += int(not acgt)
        lines += e - s if not gt[s] and acgt else 1
    c["lower_case"] = sum(1 for b in raw if b in b"acgtn")
    c["iupac"] = sum(1 for b in raw if b in b"RYSWKMBDHV")
    zero = np.r_[0, (total == 0).astype(np.int8), 0]
    c["depth0_run"] = int(((np.diff(zero) == 1)).sum())
    rec = z["b_records"]
    c["long_block"] = int(((rec["end"] - rec["pos"] + 1) > LONG_BLOCK).sum())
    assert lines == len(rec), "the replay and the reference's lines disagree on the blocks"
    return c


def parse_lines(text):
    """the records of write_to_gvcf lines, as (pos, end, min_dp, gq, pl[3], ref, gt) -- END as printed"""
    dt = np.dtype([("pos", "<i8"), ("end", "<i8"), ("min_dp", "<i4"), ("gq", "<i4"), ("pl", "<i4", (3,)), ("ref", "u1"), ("gt", "u1")])
    out = []
    for line in text.splitlines():
        f = line.split("\t")
        assert f[2] == "." and f[4] == "<NON_REF>" and f[5] == "0" and f[6] == "." and f[8] == "GT:GQ:MIN_DP:PL", line
        gt, gq, dp, pl = f[9].split(":")
        out.append((int(f[1]), int(f[7][4:]), int(dp), int(gq), tuple(int(x) for x in pl.split(",")), ord(f[3]), int(gt == "0/0")))
    return np.array(out, dtype=dt)


# ------------------------------------------------------------------------------------------ the worker: one fresh process per math library
def worker(mode, path):
    if mode == "plain":
        sys.modules["mpmath"] = None  # import mpmath -> ImportError: preprocess/utils.py falls back to math
    cffi = types.ModuleType("cffi")

    class FFI:
        def cdef(self, *_a, **_k):
            pass

        def verify(self, *_a, **_k):
            raise RuntimeError("no cffi here: the Python definitions run")

    cffi.FFI = FFI
    sys.modules["cffi"] = cffi
    sys.path.insert(0, REF)
    import preprocess.utils as U
    assert U.use_mpmath == (mode == "mpmath")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "ref.fa")
        open(fa, "w").write(f">{CTG}\n")
        open(fa + ".fai", "w").write(f"{CTG}\t{CONTIG_LEN}\t{len(CTG) + 2}\t60\t61\n")

        def calc(base_err=0.001, bin_size=5, bp=False):
            keep, sys.stdout = sys.stdout, io.StringIO()
            try:
                c = U.variantInfoCalculator("PIPE", fa, base_err, bin_size, CTG, bp_resolution=bp, sample_name="S")
            finally:
                sys.stdout = keep
            assert c.variantMath.speedUp is False
            c.vcf_writer = io.StringIO()
            return c

        def run(c, n_ref, n_total, ref, first):
            """the producer's loop (:419-437)"""
            items = []
            for i in range(len(n_total)):
                info = {"chr": CTG, "pos": first + i, "ref": chr(ref[i]), "n_total": int(n_total[i]), "n_ref": int(n_ref[i])}
                it = c.reference_likelihood(info)
                items.append((int(it["gq"]), int(it["binned_gq"]), int(it["gt"] == "0/0")) + tuple(int(x) for x in it["pl"]))
                c.make_gvcf_online(info)
            if len(c.current_block) != 0:
                c.write_to_gvcf_batch(c.current_block, c.cur_min_DP, c.cur_raw_gq)
            return c.vcf_writer.getvalue(), np.array(items, np.int32)

        for t, (base_err, bin_size, depth) in enumerate(TABLES):
            c = calc(base_err, bin_size)
            rows = []
            for nt in range(depth + 1):
                for nr in range(nt + 1):
                    it = c.reference_likelihood({"chr": CTG, "pos": 1, "ref": "A", "n_total": nt, "n_ref": nr})
                    rows.append((int(it["gq"]), int(it["binned_gq"]), int(it["gt"] == "0/0")) + tuple(int(x) for x in it["pl"]))
            out[f"a_table{t}"] = np.array(rows, np.int32)
        n_ref, n_total, ref = make_region()
        out["b_n_ref"], out["b_n_total"], out["b_ref"] = n_ref, n_total, np.frombuffer(ref, np.uint8)
        text, items = run(calc(), n_ref, n_total, ref, REGION_FIRST)
        out["b_text"], out["b_items"] = np.frombuffer(text.encode(), np.uint8), items
        text_bp, _ = run(calc(bp=True), n_ref, n_total, ref, REGION_FIRST)
        out["b_text_bp"] = np.frombuffer(text_bp.encode(), np.uint8)
        # (c) the contig's last sites: the last block ends at contig_len - 1 and prints contig_len
        k = 700
        first = CONTIG_LEN - k
        text_end, _ = run(calc(), n_ref[:k], n_total[:k], ref[:k], first)
        out["c_end_text"], out["c_end_first"], out["c_end_sites"] = np.frombuffer(text_end.encode(), np.uint8), np.int64(first), np.int64(k)
        c = calc()
        c.write_empty_pileup(CTG, 5001, 5001 + 400)
        out["c_empty_text"], out["c_empty_first"], out["c_empty_sites"] = np.frombuffer(c.vcf_writer.getvalue().encode(), np.uint8), np.int64(5001), np.int64(400)
    np.savez(path, **out)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        got = {}
        for mode in ("mpmath", "plain"):
            path = os.path.join(tmp, mode + ".npz")
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker", mode, path])
            got[mode] = dict(np.load(path))
    a, b = got["mpmath"], got["plain"]
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), f"{k}: the reference under mpmath and under math disagree"
    z = dict(a)
    items = z.pop("b_items")
    z["b_item_gq"], z["b_item_binned"], z["b_item_gt"], z["b_item_pl"] = items[:, 0], items[:, 1], items[:, 2].astype(np.uint8), items[:, 3:6]
    z["b_records"] = parse_lines(z["b_text"].tobytes().decode())
    z["meta"] = np.frombuffer(json.dumps({"ctg": CTG, "contig_len": CONTIG_LEN, "region_first": REGION_FIRST, "region_seed": REGION_SEED,
                                          "tables": [list(t) for t in TABLES]}).encode(), np.uint8)
    counts = conditions(z)
    print(json.dumps(counts))
    low = {k: v for k, v in counts.items() if v < MIN_PER_CONDITION}
    assert not low, f"conditions that occur fewer than {MIN_PER_CONDITION} times: {low}"
    np.savez_compressed(OUT, **z)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(z['b_n_total'])} sites, {len(z['b_records'])} records")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3])
    else:
        main()
