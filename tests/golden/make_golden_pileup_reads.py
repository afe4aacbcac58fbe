#!/usr/bin/env python3
"""Golden pileup columns of the REAL reference function preprocess/CreateTensorPileup.py generate_tensor, for read sets in BAM's own
encoding (tests/test_pileup_reads.py holds c3_pileup_reads_host to them).

Run in the build container only (needs the reference checkout, like make_golden_gvcf.py), never where the GPU tests run:

    python tests/golden/make_golden_pileup_reads.py

Three small read sets come from clair3_amd.synthetic.make_read_set (at most 400 sites, depth about 30, reads of 150 - 600 bases, no
non-ACGT read bases, no N ops, no D directly followed by I).  Every column's mpileup base string is rendered by the plain per-read walker
below -- it does not use the library -- and handed to the reference's own generate_tensor, which is imported and run, not transcribed.
tests/golden/pileup_reads.npz holds, per set k: the read arrays and the reference (k_pos .. k_seq, k_ref, k_ref_first, k_start, k_end),
the 18 channels of every column (k_channels, k_major), generate_tensor's depth (k_depth) and the X, I, D entries of its alt_dict per column
as one string "KEY count;KEY count" with the keys sorted (k_alleles).  conditions() counts what keeps the sets from being easy; it is
asserted here when the file is written.

generate_tensor and calculate_clair3_pileup agree on the 18 channels and on the X / I / D allele counts for such inputs; they differ in
candidate flags, R and (under N ops or non-ACGT bases) depth, which the numpy mirror of the tests holds instead.
"""
import os
import sys
import types

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "pileup_reads.npz")
sys.path.insert(0, ROOT)

from clair3_amd import synthetic as syn  # noqa: E402

MIN_PER_CONDITION = 8
DROP = 0x4 | 0x100 | 0x800 | 0x200 | 0x400
MIN_MQ = 5
SETS = (dict(n_sites=400, depth=31, seed=7101), dict(n_sites=320, depth=30, seed=7102), dict(n_sites=260, depth=32, seed=7103))
FIELDS = ("pos", "flag", "mapq", "cigar_first", "cigar", "seq_first", "seq")


def make_set(n_sites, depth, seed):
    """variant sites by hand at both ends of the region (deletions from start - 1, deletions that cross end) and inside it; three narrow gaps"""
    start = 2000
    end = start + n_sites
    hot_at = [(start - 1, 3, 2), (end - 3, 3, 2), (end - 1, 3, 1)] + [(start + 90 + 20 * k, 2, 1 + k % 3) for k in range(6)]
    hot_at += [(start + 100 + 20 * k, 3, 1 + k % 2) for k in range(6)]
    gap_at = [(start + 30, start + 36), (start + 80, start + 84), (start + 130, start + 133)]
    return syn.make_read_set(n_sites, depth, (150, 600), seed, start=start, hot=0.04, hot_at=hot_at, gap_at=gap_at, min_mq=MIN_MQ)


# ------------------------------------------------------------------------------------------ the walker: reads -> mpileup base strings
def walk(rs):
    """{position: [one string per kept read that spans it]} over the whole span of the reads, and per read (first, last) spanned position"""
    cols, spans = {}, []
    for r in range(len(rs["pos"])):
        flag, mapq = int(rs["flag"][r]), int(rs["mapq"][r])
        ops = [(int(c) & 15, int(c) >> 4) for c in rs["cigar"][int(rs["cigar_first"][r]):int(rs["cigar_first"][r + 1])]]
        packed = rs["seq"][int(rs["seq_first"][r]):int(rs["seq_first"][r + 1])]
        bases = "".join(syn.NT16[b >> 4] + syn.NT16[b & 15] for b in packed)
        first = int(rs["pos"][r])
        last = first + sum(n for op, n in ops if op in (0, 2, 3, 7, 8)) - 1
        spans.append((first, last))
        if flag & DROP or mapq < MIN_MQ:
            continue
        case = str.lower if flag & 16 else str.upper
        p, q = first, 0
        for k, (op, n) in enumerate(ops):
            if op in (1, 4):
                q += n
            if op == 3:
                p += n
            if op not in (0, 2, 7, 8):
                continue
            for i in range(n):
                s = ("^" + chr(min(mapq, 93) + 33)) if p + i == first else ""
                s += case(bases[q + i]) if op != 2 else ("#" if flag & 16 else "*")
                if i == n - 1:
                    rest = [x for x in ops[k + 1:] if x[0] != 6]
                    if rest and rest[0][0] == 1:
                        total = 0
                        for o2, n2 in rest:
                            if o2 != 1:
                                break
                            total += n2
                        q_ins = q + (n if op != 2 else 0)
                        s += "+%d%s" % (total, case(bases[q_ins:q_ins + total]))
                    elif rest and rest[0][0] == 2:
                        at = p + i + 1 - rs["ref_first"]
                        s += "-%d%s" % (rest[0][1], case(bytes(rs["ref_bytes"][at:at + rest[0][1]]).decode()))
                if p + i == last:
                    s += "$"
                cols.setdefault(p + i, []).append(s)
            p += n
            if op != 2:
                q += n
    return cols, spans


def reference_columns(rs):
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
    from preprocess.CreateTensorPileup import generate_tensor
    cols, spans = walk(rs)
    ref = bytes(rs["ref_bytes"]).decode()
    major, channels, depth, alleles = [], [], [], []
    for p in sorted(cols):
        if not rs["start"] <= p < rs["end"]:
            continue
        tensor, alt_dict, _af, d, _pass, _list, _mdl = generate_tensor(
            pos=p, pileup_bases="".join(cols[p]), reference_sequence=ref, reference_start=rs["ref_first"], reference_base=ref[p - rs["ref_first"]],
            minimum_af_for_candidate=0.0, minimum_snp_af_for_candidate=0.0, minimum_indel_af_for_candidate=0.0, platform="ont", fast_mode=False,
            call_snp_only=False)
        major.append(p), channels.append(tensor), depth.append(d)
        alleles.append(";".join(f"{k} {v}" for k, v in sorted(alt_dict.items()) if k[0] in "XID"))
    return np.array(major, np.int64), np.array(channels, np.int32).reshape(-1, 18), np.array(depth, np.int32), np.array(alleles), cols, spans


def conditions(rs, cols, spans, major):
    """how often each hard case occurs in one set"""
    start, end = rs["start"], rs["end"]
    c = dict.fromkeys(("two_ins_strings_one_length_one_strand", "ins_string_on_both_strands", "two_del_lengths", "del_crossing_end", "del_from_start_minus_1",
                       "read_crossing_start", "read_outside", "filtered_read", "soft_clipped_read", "coverage_gap"), 0)
    for p in range(start - 1, end):
        ins, dels = {}, set()
        for s in cols.get(p, ()):
            if "+" in s[2 if s[0] == "^" else 0:]:
                body = s.split("+", 1)[1] if s[0] != "^" else s[2:].split("+", 1)[1]
                bases = body.lstrip("0123456789").rstrip("$")
                ins.setdefault((len(bases), bases.isupper()), set()).add(bases)
            elif "-" in s[2 if s[0] == "^" else 0:]:
                body = (s[2:] if s[0] == "^" else s).split("-", 1)[1]
                n = int(body[:len(body) - len(body.lstrip("0123456789"))])
                dels.add(n)
                if p == start - 1:
                    c["del_from_start_minus_1"] += 1
                if start <= p and p + n >= end:
                    c["del_crossing_end"] += 1
        if p < start:
            continue
        c["two_ins_strings_one_length_one_strand"] += any(len(v) >= 2 for v in ins.values())
        fwd = set().union(*[v for (n, up), v in ins.items() if up] or [set()])
        rev = {b.upper() for (n, up), v in ins.items() if not up for b in v}
        c["ins_string_on_both_strands"] += bool(fwd & rev)
        c["two_del_lengths"] += len(dels) >= 2
    for r, (first, last) in enumerate(spans):
        kept = not (int(rs["flag"][r]) & DROP or int(rs["mapq"][r]) < MIN_MQ)
        c["filtered_read"] += not kept
        c["read_crossing_start"] += kept and first < start <= last
        c["read_outside"] += last < start or first >= end
        ops = [int(x) & 15 for x in rs["cigar"][int(rs["cigar_first"][r]):int(rs["cigar_first"][r + 1])]]
        c["soft_clipped_read"] += kept and 4 in ops
    have = set(major.tolist())
    c["coverage_gap"] = sum(1 for p in range(start + 1, end) if p not in have and p - 1 in have)
    return c


def main():
    out, total = {}, {}
    for k, spec in enumerate(SETS):
        rs = make_set(**spec)
        codes = np.concatenate([rs["seq"] >> 4, rs["seq"] & 15])
        assert np.isin(codes, [0, 1, 2, 4, 8]).all(), "a non-ACGT read base"
        major, channels, depth, alleles, cols, spans = reference_columns(rs)
        for name in FIELDS:
            out[f"{k}_{name}"] = rs[name]
        out[f"{k}_ref"], out[f"{k}_ref_first"], out[f"{k}_start"], out[f"{k}_end"] = rs["ref_bytes"], rs["ref_first"], rs["start"], rs["end"]
        out[f"{k}_major"], out[f"{k}_channels"], out[f"{k}_depth"], out[f"{k}_alleles"] = major, channels, depth, alleles
        for name, v in conditions(rs, cols, spans, major).items():
            total[name] = total.get(name, 0) + int(v)
        print(f"set {k}: {len(rs['pos'])} reads, {len(major)} columns, mean depth {depth.mean():.1f}")
    print(total)
    short = {name: v for name, v in total.items() if v < MIN_PER_CONDITION}
    assert not short, f"conditions that occur fewer than {MIN_PER_CONDITION} times: {short}"
    np.savez_compressed(OUT, n_sets=len(SETS), min_mq=MIN_MQ, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
