#!/usr/bin/env python3
"""Golden full-alignment windows of the REAL reference functions preprocess/CreateTensorFullAlignment.py sorted_by_hap_read_name and
generate_tensor, for read sets in BAM's own encoding (tests/test_fa_reads.py holds c3_fa_reads_host to them).

Run in the build container only (needs the reference checkout, like make_golden_pileup_reads.py), never where the GPU tests run:

    python tests/golden/make_golden_fa_reads.py

Three small read sets come from clair3_amd.synthetic.make_read_set / make_read_extras (depth about 30, reads of 60 - 160 bases, all three
haplotypes, ACGT bases only, no N ops, no D directly followed by I and no I followed by D), put into coordinate order.  The plain per-read
walker below -- it does not use the library -- renders every flanking position into the Position objects of the reference's pileup_dict
(read names, (base, indel) pairs, quality characters), and the reference's own functions are imported and run, not transcribed.
tests/golden/fa_reads.npz holds, per set k: the read arrays, extras and reference, the candidates (k_centres), the rows of every window
(k_rows, k_counts: generate_tensor's tensor is the occupied rows, in its order) and its alt-info string (k_alt).

The Python path and the C function (calculate_clair3_full_alignment, the rule of csrc/c3_fa_rule.h) differ on the following, which is kept
out of the fixture; the C function is the rule:
  - windows with more reads than matrix_depth (random.sample against rand()): the depth stays below 89;
  - non-ACGT bases and N ops: none are generated;
  - the allele fraction is computed in double here and in float32 there: main() asserts that both give the same integer on every
    (count, depth) pair that occurs;
  - a read that carries an indel at the centre AND a non-reference base there: the Python path keys an insertion by base + string and
    counts the base only for reads without an indel (alt_dict), the C function keys by the string and counts every base (acgt_count).
    Positions where such a read exists are not used as candidates (centres() drops them).
conditions() counts what keeps the sets from being easy; it is asserted when the file is written.
"""
import os
import sys
import types
from collections import defaultdict

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "fa_reads.npz")
sys.path.insert(0, ROOT)

from clair3_amd import synthetic as syn  # noqa: E402

MIN_PER_CONDITION = 8
MIN_MQ = 5
SETS = (dict(n_sites=110, depth=30, seed=8101), dict(n_sites=100, depth=31, seed=8102), dict(n_sites=90, depth=29, seed=8103))
READ_FIELDS = ("pos", "flag", "mapq", "cigar_first", "cigar", "seq_first", "seq")
EXTRA_FIELDS = ("qual_first", "qual", "haplotype", "name_key")


def make_set(n_sites, depth, seed):
    start = 2000
    hot_at = [(start + 10 + 9 * k, 2, 1 + k % 3) for k in range(8)] + [(start + 14 + 9 * k, 3, 1 + k % 2) for k in range(8)]
    rs0 = syn.make_read_set(n_sites, depth, (60, 160), seed, start=start, ins=0.02, dele=0.008, hot=0.04, hot_at=hot_at, min_mq=MIN_MQ)
    ex0 = syn.make_read_extras(rs0, seed + 1, phased=0.6, duplicate_names=0.03)
    return syn.sort_read_set(rs0), syn.sort_read_extras(rs0, ex0)


def walk(rs, ex):
    """{position: [(read, base, indel, quality)]} over the span of the kept reads, in read order; per read (first, behind)"""
    cols, spans, kept, seen = defaultdict(list), [], [], set()
    for r in range(len(rs["pos"])):
        flag, mapq = int(rs["flag"][r]), int(rs["mapq"][r])
        ops = [(int(c) & 15, int(c) >> 4) for c in rs["cigar"][int(rs["cigar_first"][r]):int(rs["cigar_first"][r + 1])]]
        packed = rs["seq"][int(rs["seq_first"][r]):int(rs["seq_first"][r + 1])]
        bases = "".join(syn.NT16[b >> 4] + syn.NT16[b & 15] for b in packed)
        qual = ex["qual"][int(ex["qual_first"][r]):int(ex["qual_first"][r + 1])]
        first = int(rs["pos"][r])
        spans.append((first, first + sum(n for op, n in ops if op in (0, 2, 3, 7, 8))))
        ok = not (flag & syn.FA_DROP_FLAGS or mapq < MIN_MQ)
        if ok:
            ok = int(ex["name_key"][r]) not in seen
            seen.add(int(ex["name_key"][r]))
        kept.append(ok)
        if not ok:
            continue
        case = str.lower if flag & 16 else str.upper
        p, q = first, 0
        for k, (op, n) in enumerate(ops):
            if op in (1, 4):
                q += n
            if op not in (0, 2, 7, 8):
                continue
            for i in range(n):
                base = case(bases[q + i]) if op != 2 else ("#" if flag & 16 else "*")
                indel = ""
                if i == n - 1:
                    rest = [x for x in ops[k + 1:] if x[0] != 6]
                    if rest and rest[0][0] == 1:
                        q_ins = q + (n if op != 2 else 0)
                        indel = "+" + case(bases[q_ins:q_ins + rest[0][1]])
                    elif rest and rest[0][0] == 2:
                        at = p + i + 1 - rs["ref_first"]
                        indel = "-" + case(bytes(rs["ref_bytes"][at:at + rest[0][1]]).decode())
                cols[p + i].append((r, base, indel, int(qual[q + i]) if op != 2 else 0))
            p += n
            if op != 2:
                q += n
    return cols, spans, kept


def centres(rs, cols):
    """the positions of the region, without those where a read carries an indel and a non-reference base (the docstring says why)"""
    ref = bytes(rs["ref_bytes"]).decode()
    out = []
    for c in range(rs["start"], rs["end"]):
        rb = ref[c - rs["ref_first"]]
        if all(not (indel and base.upper() != rb and base not in "*#") for _, base, indel, _ in cols.get(c, ())):
            out.append(c)
    return np.array(out, np.int64)


def reference_windows(rs, ex, cols, cand):
    cffi = types.ModuleType("cffi")

    class FFI:
        def cdef(self, *_a, **_k):
            pass

        def verify(self, *_a, **_k):
            raise RuntimeError("no cffi here: the Python definitions run")

    cffi.FFI = FFI
    sys.modules.setdefault("cffi", cffi)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from preprocess.CreateTensorFullAlignment import Position, generate_tensor, sorted_by_hap_read_name
    ref = bytes(rs["ref_bytes"]).decode()
    pileup_dict = {}
    flank = set()
    for c in cand:
        flank.update(range(int(c) - 16, int(c) + 17))
    for p in sorted(flank):
        e = cols.get(p, ())
        pileup_dict[p] = Position(pos=p, ref_base=ref[p - rs["ref_first"]], read_name_list=["r%06d" % r for r, _, _, _ in e],
                                  base_list=[[b, i] for _, b, i, _ in e], raw_base_quality="".join(chr(q + 33) for _, _, _, q in e),
                                  raw_mapping_quality="".join(chr(int(rs["mapq"][r]) + 33) for r, _, _, _ in e))
    hap_dict = defaultdict(int, {"r%06d" % r: int(ex["haplotype"][r]) for r in range(len(rs["pos"]))})
    rows, counts, alts = [], [], []
    for c in cand:
        c = int(c)
        names = sorted_by_hap_read_name(c, defaultdict(int), pileup_dict, hap_dict, "ont")
        assert len(names) < 89, "a window as deep as matrix_depth"
        text, alt = generate_tensor("c", c, names, pileup_dict, ref[c - 16 - rs["ref_first"]:c + 17 - rs["ref_first"]], ref, rs["ref_first"], "ont", {}, False)
        counts.append(len(names))
        if text is None:
            alts.append("")
            continue
        rows.append(np.array(text.split("\t")[3].split(" "), np.int64).astype(np.int8).reshape(len(names), 33, 8))
        alts.append(alt)
    return (np.concatenate(rows) if rows else np.zeros((0, 33, 8), np.int8)), np.array(counts, np.int32), np.array(alts)


def conditions(rs, ex, cols, spans, kept, cand):
    names = ("fewer_reads_than_depth", "ins_at_centre", "ins_string_on_several_reads", "ins_past_column_32", "ins_at_column_32",
             "overlapping_ins_spans_in_a_row", "del_starting_at_centre", "deleted_centre", "read_starting_in_window", "read_ending_in_window",
             "three_haplotypes_in_window", "filtered_read", "soft_clipped_read")
    n = dict.fromkeys(names, 0)
    for c in cand:
        c = int(c)
        at = cols.get(c, ())
        reads = {r for p in range(c - 16, c + 17) for r, _, _, _ in cols.get(p, ())}
        n["fewer_reads_than_depth"] += len(reads) < 89
        ins = [i for _, b, i, _ in at if i.startswith("+") and b not in "*#"]
        n["ins_at_centre"] += bool(ins)
        n["ins_string_on_several_reads"] += any(ins.count(s.upper()) + ins.count(s.lower()) >= 2 for s in ins)
        n["del_starting_at_centre"] += any(i.startswith("-") for _, _, i, _ in at)
        n["deleted_centre"] += any(b in "*#" for _, b, _, _ in at)
        n["read_starting_in_window"] += any(c - 16 < spans[r][0] <= c + 16 for r in reads)
        n["read_ending_in_window"] += any(c - 16 < spans[r][1] <= c + 16 for r in reads)
        n["three_haplotypes_in_window"] += len({int(ex["haplotype"][r]) for r in reads}) == 3
        per_read = defaultdict(list)
        for col in range(33):
            for r, b, i, _ in cols.get(c - 16 + col, ()):
                if i.startswith("+") and b not in "*#":
                    per_read[r].append((col, len(i) - 1))
                    n["ins_past_column_32"] += col < 32 and col + len(i) - 1 > 33
                    n["ins_at_column_32"] += col == 32
        n["overlapping_ins_spans_in_a_row"] += any(a[0] + a[1] > b[0] for v in per_read.values() for a, b in zip(v, v[1:]))
    n["filtered_read"] = sum(not k for k in kept)
    for r in range(len(rs["pos"])):
        ops = [int(x) & 15 for x in rs["cigar"][int(rs["cigar_first"][r]):int(rs["cigar_first"][r + 1])]]
        n["soft_clipped_read"] += kept[r] and 4 in ops
    return n


def af_pairs_agree(alts):
    """every (count, depth) pair of the fixture gives one integer in double and in float32"""
    for alt in alts:
        if not alt:
            continue
        depth, _, rest = str(alt).partition("-")
        for v in rest.split(" ")[1::2]:
            count, depth_i = int(v), int(depth)
            d = int(100 * min(count / max(1, float(depth_i)), 1.0))
            x = np.float32(count) / np.float32(depth_i)
            f = int(np.float32(100) * x) if x < 1.0 else 100
            assert d == f, f"count {count} depth {depth_i}: double {d}, float32 {f} -- choose another seed"


def main():
    out, total = {}, {}
    for k, spec in enumerate(SETS):
        rs, ex = make_set(**spec)
        codes = np.concatenate([rs["seq"] >> 4, rs["seq"] & 15])
        assert np.isin(codes, [0, 1, 2, 4, 8]).all(), "a non-ACGT read base"
        cols, spans, kept = walk(rs, ex)
        cand = centres(rs, cols)
        rows, counts, alts = reference_windows(rs, ex, cols, cand)
        af_pairs_agree(alts)
        for name in READ_FIELDS:
            out[f"{k}_{name}"] = rs[name]
        for name in EXTRA_FIELDS:
            out[f"{k}_{name}"] = ex[name]
        out[f"{k}_ref"], out[f"{k}_ref_first"], out[f"{k}_centres"] = rs["ref_bytes"], rs["ref_first"], cand
        out[f"{k}_rows"], out[f"{k}_counts"], out[f"{k}_alt"] = rows, counts, alts
        for name, v in conditions(rs, ex, cols, spans, kept, cand).items():
            total[name] = total.get(name, 0) + int(v)
        print(f"set {k}: {len(rs['pos'])} reads, {len(cand)} candidates of {spec['n_sites']} sites, {len(rows)} rows")
    print(total)
    short = {name: v for name, v in total.items() if v < MIN_PER_CONDITION}
    assert not short, f"conditions that occur fewer than {MIN_PER_CONDITION} times: {short}"
    np.savez_compressed(OUT, n_sets=len(SETS), min_mq=MIN_MQ, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
