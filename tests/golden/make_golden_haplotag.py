#!/usr/bin/env python3
"""Golden read tags and pair alleles of the REAL reference functions haplotag_read / realign_read / cigar_prefix_length
(src/clair3_full_alignment_dwell.c) with src/levenshtein.c, for read sets in BAM's own encoding (tests/test_haplotag.py holds
c3_fa_haplotag_host to them, tests/test_haplotag_gpu.py the device form).

Run in the build container only (needs the reference checkout and a C compiler, like make_golden_fa_reads.py), never where the GPU tests run:

    python tests/golden/make_golden_haplotag.py

At run time, in a temporary directory, the functions cigar_prefix_length, get_ref_seq, get_query_seq, update_haplotype_cost, realign_read
and haplotag_read are cut BY NAME out of the reference's source file, a prelude of this script's own is put in front (the htslib macros
bam_cigar_op / bam_cigar_oplen / bam_seqi with the BAM_C* op codes and seq_nt16_str, max / min; the reference's khash.h,
medaka_khcounter.h, clair3_full_alignment_dwell.h and levenshtein.h come in by -I), a main of this script's own that reads a case file is
put behind, and the whole is compiled with the reference's levenshtein.c and medaka_khcounter.c and run.  Nothing of the reference's text
or binaries is written into the repository: tests/golden/fa_haplotag.npz holds data only.

Three small read sets come from clair3_amd.synthetic.make_read_set (depth about 30, reads of 60 - 300 bases, put into coordinate order)
with make_phased_variants.  Per set k the file holds the read arrays, the reference, the variants, k_hap: the tag of every read with mapq
>= 20 from haplotag_read with the full variant list (0 for the others, as :629-632), and k_alleles / k_pair_first: per (read, variant)
pair the allele, obtained by calling haplotag_read with that single variant at genotype 1 (tag 1 / 2 / 0 is allele 1 / 2 / 0).  The pairs
of a read are the variants in [pos, end), and at end when an I op stands there.
conditions() counts what keeps the sets from being easy; it is asserted when the file is written.
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "fa_haplotag.npz")
sys.path.insert(0, ROOT)

from clair3_amd import synthetic as syn  # noqa: E402

MIN_PER_CONDITION = 8
MIN_HAPLOTAG_MQ = 20
SETS = (dict(n_sites=160, depth=30, seed=9101), dict(n_sites=150, depth=31, seed=9102), dict(n_sites=140, depth=29, seed=9103))
READ_FIELDS = ("pos", "flag", "mapq", "cigar_first", "cigar", "seq_first", "seq")
VARIANT_FIELDS = ("pos", "alt_base", "genotype", "phase_set")
FUNCTIONS = ("cigar_prefix_length", "get_ref_seq", "get_query_seq", "update_haplotype_cost", "realign_read", "haplotag_read")

PRELUDE = r"""
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "khash.h"
#include "medaka_khcounter.h"
#include "clair3_full_alignment_dwell.h"
#include "levenshtein.h"
enum { BAM_CMATCH, BAM_CINS, BAM_CDEL, BAM_CREF_SKIP, BAM_CSOFT_CLIP, BAM_CHARD_CLIP, BAM_CPAD, BAM_CEQUAL, BAM_CDIFF };
#define bam_cigar_op(c) ((c) & 0xf)
#define bam_cigar_oplen(c) ((c) >> 4)
#define bam_seqi(s, i) ((s)[(i) >> 1] >> ((~(i) & 1) << 2) & 0xf)
static const char seq_nt16_str[] = "=ACMGRSVTWYHKDBN";
#define max(a, b) ((a) > (b) ? (a) : (b))
#define min(a, b) ((a) < (b) ? (a) : (b))
"""

DRIVER = r"""
static void *get(FILE *f, size_t size, size_t n) {
    void *p = calloc(n + 1, size);
    if (n && fread(p, size, n, f) != n) exit(3);
    return p;
}
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int64_t h[7];
    if (!f || fread(h, 8, 7, f) != 7) return 2;
    const size_t n = h[0], n_ops = h[1], seq_bytes = h[2], nv = h[3], ref_len = h[5], n_pairs = h[6];
    int64_t *pos = get(f, 8, n), *cfirst = get(f, 8, n + 1), *sfirst = get(f, 8, n + 1), *vpos = get(f, 8, nv), *pair_first = get(f, 8, n + 1),
            *var_first = get(f, 8, n);
    uint8_t *mapq = get(f, 1, n), *seq = get(f, 1, seq_bytes), *valt = get(f, 1, nv), *vgt = get(f, 1, nv);
    uint32_t *cigar = get(f, 4, n_ops);
    int32_t *vps = get(f, 4, nv);
    char *ref = get(f, 1, ref_len);
    fclose(f);
    Variant *store = calloc(nv + 1, sizeof(Variant)), **all = calloc(nv + 1, sizeof(Variant *));
    for (size_t i = 0; i < nv; ++i) {
        store[i].position = (int)vpos[i], store[i].ref_base = 'N', store[i].alt_base = (char)valt[i], store[i].genotype = vgt[i], store[i].phase_set = vps[i];
        all[i] = &store[i];
    }
    uint8_t *hap = calloc(n + 1, 1);
    int8_t *alleles = calloc(n_pairs + 1, 1);
    for (size_t r = 0; r < n; ++r) {
        if (mapq[r] < min_haplotag_mq) continue;
        Read read;
        memset(&read, 0, sizeof(read));
        read.read_start = pos[r], read.cigartuples = cigar + cfirst[r], read.n_cigar = cfirst[r + 1] - cfirst[r], read.seqi = seq + sfirst[r];
        Variants_info info = {all, nv, 0};
        hap[r] = nv ? (uint8_t)haplotag_read(&info, &read, ref, (size_t)h[4]) : 0;
        for (int64_t p = pair_first[r]; p < pair_first[r + 1]; ++p) {
            Variant one = store[var_first[r] + (p - pair_first[r])], *list[1] = {&one};
            one.genotype = 1;
            Variants_info single = {list, 1, 0};
            alleles[p] = (int8_t)haplotag_read(&single, &read, ref, (size_t)h[4]);
        }
    }
    FILE *o = fopen(argv[2], "wb");
    fwrite(hap, 1, n, o), fwrite(alleles, 1, n_pairs, o);
    fclose(o);
    return 0;
}
"""


def cut(source, name):
    """the definition of ``name``: from its line at column 0 to the closing brace at column 0"""
    m = re.search(r"^[A-Za-z_][^\n;{]*\b" + name + r"\s*\([^;{]*\)\s*\{.*?^\}", source, re.S | re.M)
    assert m, f"{name} not found in the reference"
    return m.group(0)


def build(tmp):
    src = os.path.join(REF, "src")
    with open(os.path.join(src, "clair3_full_alignment_dwell.c")) as fh:
        source = fh.read()
    path = os.path.join(tmp, "haplotag_ref.c")
    with open(path, "w") as fh:
        fh.write(PRELUDE + "\n\n".join(cut(source, name) for name in FUNCTIONS) + DRIVER)
    exe = os.path.join(tmp, "haplotag_ref")
    subprocess.check_call(["gcc", "-O1", "-w", "-I", src, path, os.path.join(src, "levenshtein.c"), os.path.join(src, "medaka_khcounter.c"), "-o", exe, "-lm"])
    return exe


def read_ends(rs):
    """(end, an I op stands behind the last reference base) of every read"""
    end, tail = np.zeros(len(rs["pos"]), np.int64), np.zeros(len(rs["pos"]), bool)
    for r in range(len(rs["pos"])):
        at, t = int(rs["pos"][r]), False
        for c in rs["cigar"][rs["cigar_first"][r]:rs["cigar_first"][r + 1]]:
            op, n = int(c) & 15, int(c) >> 4
            if op in (0, 2, 3, 7, 8):
                at, t = at + n, False
            elif op == 1:
                t = True
        end[r], tail[r] = at, t
    return end, tail


def pair_ranges(rs, v):
    end, tail = read_ends(rs)
    lo = np.searchsorted(v["pos"], rs["pos"])
    hi = np.searchsorted(v["pos"], end + tail)
    count = np.where(rs["mapq"] >= MIN_HAPLOTAG_MQ, hi - lo, 0)
    return np.where(count > 0, lo, 0).astype(np.int64), np.concatenate([[0], np.cumsum(count)]).astype(np.int64)


def run_reference(exe, tmp, rs, v):
    var_first, pair_first = pair_ranges(rs, v)
    n = len(rs["pos"])
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as fh:
        np.array([n, len(rs["cigar"]), len(rs["seq"]), len(v["pos"]), rs["ref_first"], len(rs["ref_bytes"]), pair_first[-1]], np.int64).tofile(fh)
        for a, dt in ((rs["pos"], np.int64), (rs["cigar_first"], np.int64), (rs["seq_first"], np.int64), (v["pos"], np.int64), (pair_first, np.int64),
                      (var_first, np.int64), (rs["mapq"], np.uint8), (rs["seq"], np.uint8), (v["alt_base"], np.uint8), (v["genotype"], np.uint8),
                      (rs["cigar"], np.uint32), (v["phase_set"], np.int32), (rs["ref_bytes"], np.uint8)):
            np.ascontiguousarray(a, dtype=dt).tofile(fh)
    subprocess.check_call([exe, case, out])
    raw = np.fromfile(out, np.uint8)
    assert len(raw) == n + pair_first[-1]
    return raw[:n].copy(), raw[n:].astype(np.int8), pair_first, var_first


def make_set(n_sites, depth, seed):
    start = 2000
    hot_at = [(start + 6 + 19 * k, 1, 1 + k % 3) for k in range(n_sites // 19)]
    rs = syn.sort_read_set(syn.make_read_set(n_sites, depth, (60, 300), seed, start=start, ins=0.012, dele=0.012, soft_clip=0.5, hot=0.01,
                                             hot_at=hot_at, ref_other=0.03, low_mapq=0.06))
    near = np.arange(3, len(rs["pos"]), 40)
    v = syn.make_phased_variants(rs, seed + 1, rate=0.008, hot_at=hot_at, near=near, set_span=50)
    return rs, v


def conditions(rs, v, hap, alleles, pair_first, var_first):
    """how often each hard case occurs among the pairs / reads of a set"""
    c = dict.fromkeys(("in_m", "at_ins", "in_d", "first_10", "last_10", "ins_in_context", "del_in_context", "soft_clip_at_context", "allele_0",
                       "two_sets", "tie_across_sets", "zero_sum", "low_mapq", "lower_case_ref"), 0)
    ref, ref_first = rs["ref_bytes"], rs["ref_first"]
    end, _ = read_ends(rs)
    for r in range(len(rs["pos"])):
        if rs["mapq"][r] < MIN_HAPLOTAG_MQ:
            c["low_mapq"] += 1
            continue
        ops = [(int(x) & 15, int(x) >> 4) for x in rs["cigar"][rs["cigar_first"][r]:rs["cigar_first"][r + 1]]]
        p0, at = int(rs["pos"][r]), int(rs["pos"][r])
        ins_at, deleted, matched = set(), set(), set()
        for op, n in ops:
            if op == 1:
                ins_at.add(at)
            elif op == 2:
                deleted.update(range(at, at + n))
            elif op in (0, 7, 8):
                matched.update(range(at, at + n))
            if op in (0, 2, 3, 7, 8):
                at += n
        clip_front, clip_back = ops[0][0] == 4, ops[-1][0] == 4
        cost = {}
        for p in range(pair_first[r], pair_first[r + 1]):
            vi = var_first[r] + p - pair_first[r]
            x, a = int(v["pos"][vi]), int(alleles[p])
            c["at_ins"] += x in ins_at
            c["in_m"] += x not in ins_at and x in matched
            c["in_d"] += x not in ins_at and x in deleted
            c["first_10"] += x - p0 < 10
            c["last_10"] += end[r] - x <= 10
            c["ins_in_context"] += any(x - 10 < i <= x + 10 and i != x for i in ins_at)
            c["del_in_context"] += any(x - 10 <= d < x + 11 and d != x for d in deleted)
            c["soft_clip_at_context"] += (clip_front and x - p0 <= 10) or (clip_back and end[r] - x <= 11)
            c["allele_0"] += a == 0
            c["lower_case_ref"] += bool((ref[x - 10 - ref_first:x + 11 - ref_first] >= 97).any())
            if a:
                s = int(v["phase_set"][vi])
                cost[s] = cost.get(s, 0) + (1 if a == int(v["genotype"][vi]) else -1)
        c["two_sets"] += len(cost) >= 2
        if len(cost) >= 2 and max(cost.values()) > 0 and max(cost.values()) == -min(cost.values()):
            c["tie_across_sets"] += 1
            assert hap[r] == 2
        if cost and max(cost.values()) <= 0 and min(cost.values()) >= 0:
            c["zero_sum"] += 1
            assert hap[r] == 0
    return c


def main():
    out, total = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for k, spec in enumerate(SETS):
            rs, v = make_set(**spec)
            hap, alleles, pair_first, var_first = run_reference(exe, tmp, rs, v)
            for name, n in conditions(rs, v, hap, alleles, pair_first, var_first).items():
                total[name] = total.get(name, 0) + n
            for name in READ_FIELDS:
                out[f"{k}_{name}"] = rs[name]
            for name in VARIANT_FIELDS:
                out[f"{k}_v_{name}"] = v[name]
            out[f"{k}_ref_bytes"], out[f"{k}_ref_first"] = rs["ref_bytes"], np.int64(rs["ref_first"])
            out[f"{k}_hap"], out[f"{k}_alleles"], out[f"{k}_pair_first"] = hap, alleles, pair_first
            print(f"set {k}: {len(hap)} reads, {len(v['pos'])} variants, {len(alleles)} pairs, tags {np.bincount(hap, minlength=3)}, "
                  f"alleles {np.bincount(alleles, minlength=3)}")
    print(total)
    short = {name: n for name, n in total.items() if n < MIN_PER_CONDITION}
    assert not short, f"conditions that occur fewer than {MIN_PER_CONDITION} times: {short}"
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
