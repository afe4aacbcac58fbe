"""What the pileup-from-reads tests share: the golden read sets (tests/golden/make_golden_pileup_reads.py), a one-column read set, and the sets
that take the device form to its capacity edges (a megabase region with three clusters of reads, event tables on the size rule's boundary)."""
import functools
import os

import numpy as np

from clair3_amd import synthetic as syn
from tests.util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "pileup_reads.npz")
FIELDS = ("pos", "flag", "mapq", "cigar_first", "cigar", "seq_first", "seq")


def golden_sets():
    with np.load(GOLDEN) as z:
        for k in range(int(z["n_sets"])):
            rs = {name: z[f"{k}_{name}"] for name in FIELDS}
            rs.update(start=int(z[f"{k}_start"]), end=int(z[f"{k}_end"]), ref_bytes=z[f"{k}_ref"], ref_first=int(z[f"{k}_ref_first"]), min_mq=int(z["min_mq"]))
            yield k, rs, {name: z[f"{k}_{name}"] for name in ("major", "channels", "depth", "alleles")}


def insertion_column(n_reads=300, n_strings=40, seed=5):
    """n_reads reads that all carry an insertion behind one position, n_strings distinct strings of lengths 1 .. 6 on both strands"""
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), size=400))
    strings = set()
    while len(strings) < n_strings:
        strings.add("".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 7)))))
    strings = sorted(strings)
    reads = []
    for i in range(n_reads):
        s = strings[i % n_strings] if i < 2 * n_strings else strings[int(rng.integers(0, n_strings))]
        reads.append((100, 16 * int(rng.integers(0, 2)), 60, f"50M{len(s)}I50M", ref[100:150] + s + ref[150:200]))
    rs = syn.pack_reads(reads)
    rs.update(start=120, end=190, ref_bytes=np.frombuffer(ref.encode(), np.uint8), ref_first=0, min_mq=5)
    return rs


LONG_CIGARS = dict(n_sites=300, depth=12, read_len=(2000, 4000), seed=33, ins=0.04, dele=0.04, d_then_i=0.01, i_then_d=0.01, pad=0.2, eqx=True,
                   non_acgt=0.01, ref_other=0.02)  # full alignment's long_cigars: reads of hundreds of ops


def _cluster(ref, at, n_reads, rng):
    """n_reads reads of 80 .. 200 reference bases that start in [at, at + 300), the first one at ``at``.  Variant sites every 30 positions from at + 40: a
    substitution, 15 behind it an insertion (T or GA by the read's parity), 10 behind that a deletion (of 1 or 2); a read over a site
    carries its variant with probability 1 / 2, on either strand"""
    reads = []
    for i in range(n_reads):
        pos, n = at + (int(rng.integers(0, 300)) if i else 0), int(rng.integers(80, 201))
        ops, seq, p = [], [], pos
        for site in range(at + 40, pos + n - 12, 5):
            kind = {0: "X", 15: "I", 25: "D"}.get((site - at - 40) % 30)
            if kind is None or site < p + 2 or rng.random() < 0.5:
                continue
            ops.append(("M", site + 1 - p)), seq.append(ref[p:site + 1])
            p = site + 1
            if kind == "X":
                seq[-1] = seq[-1][:-1] + "ACGT"[("ACGT".index(ref[site]) + 1) % 4]
            elif kind == "I":
                s = "T" if i % 2 else "GA"
                ops.append(("I", len(s))), seq.append(s)
            else:
                ops.append(("D", 1 + i % 2))
                p += 1 + i % 2
        ops.append(("M", pos + n - p)), seq.append(ref[p:pos + n])
        merged = []
        for op, ln in ops:  # (a substitution leaves M behind M)
            if merged and merged[-1][0] == op:
                merged[-1] = (op, merged[-1][1] + ln)
            else:
                merged.append((op, ln))
        reads.append((pos, 16 * int(rng.integers(0, 2)), 60, merged, "".join(seq)))
    return reads


def three_clusters(n_sites, boundary, reads_per_cluster=200, start=1000, seed=41):
    """a region of n_sites sites from ``start`` with reads in three clusters only: over its start (the first reads begin in front of it),
    straddling site ``boundary``, and over its end (the last reads reach beyond it).  rs["clusters"]: the position each cluster starts at"""
    rng = np.random.default_rng(seed)
    end = start + n_sites
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=end + 600)]
    at = [start - 60, start + boundary - 250, end - 420]
    reads = []
    for a in at:
        reads += _cluster(ref[a:a + 520].tobytes().decode().rjust(a + 520), a, reads_per_cluster, rng)
    rs = syn.pack_reads(reads)
    rs.update(start=start, end=end, ref_bytes=ref, ref_first=0, min_mq=5, clusters=at)
    return rs


@functools.lru_cache(maxsize=None)  # (shared between tests and left unchanged by them)
def big_region():
    """(rs, tile): three_clusters over tile * tile + 2 * tile + 5 sites, tile the sites of a compaction tile and the tiles one step of the
    scan holds: tile + 3 tiles, the last one of 5 sites, the middle cluster across the step's boundary"""
    from clair3_amd import _lib
    tile = _lib.lib().c3_pileup_tile_sites()
    return three_clusters(tile * tile + 2 * tile + 5, tile * tile), tile


WRAP_SHIFT = 5  # distinct_events(32, shift=5): two probes start at the last of 64 slots (tests/test_pileup_reads.py asserts it)
# every column a candidate (thresholds 0 and call_ht): more candidates than a pileup lane of the ring takes
MANY_CANDIDATES = dict(n_sites=1500, depth=20, read_len=(150, 400), seed=45)


def distinct_events(n_ops, dropped=3, shift=0):
    """kept reads that hold exactly n_ops I and D ops, every one an event of its own (its own column, or the other kind), and ``dropped``
    reads with indels that are dropped by flag or mapq and count for nothing; shift moves the kept reads (other columns: other keys)"""
    rng = np.random.default_rng(n_ops)
    ref = "".join(rng.choice(list("ACGT"), size=400))
    reads = []
    for i in range(n_ops // 2):  # an insertion behind pos + 9, a deletion behind pos + 19
        pos = 100 + shift + 3 * i
        reads.append((pos, 16 * (i % 2), 60, "10M1I10M1D10M", ref[pos:pos + 10] + "ACGT"[i % 4] + ref[pos + 10:pos + 20] + ref[pos + 21:pos + 31]))
    if n_ops % 2:
        reads.append((230, 0, 60, "10M2I10M", ref[230:240] + "TT" + ref[240:250]))
    for i in range(dropped):
        reads.append((120 + i, 0x400 if i % 2 else 0, 60 if i % 2 else 2, "10M3I10M2D5M", ref[120 + i:130 + i] + "GGG" + ref[130 + i:140 + i] + ref[142 + i:147 + i]))
    rs = syn.pack_reads(reads)
    rs.update(start=90, end=300, ref_bytes=np.frombuffer(ref.encode(), np.uint8), ref_first=0, min_mq=5)
    return rs


def take_reads(rs, n):
    """the first n reads of a read set (its region and reference kept)"""
    out = dict(rs)
    c, q = int(rs["cigar_first"][n]), int(rs["seq_first"][n])
    out.update(pos=rs["pos"][:n], flag=rs["flag"][:n], mapq=rs["mapq"][:n], cigar_first=rs["cigar_first"][:n + 1], cigar=rs["cigar"][:c],
               seq_first=rs["seq_first"][:n + 1], seq=rs["seq"][:q])
    return out


def one_read(seed=21):
    """ONE read over a 200-site region: soft clip, matches with two substitutions, an insertion, a deletion, an N op, a non-ACGT base"""
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), size=600))
    a, b, c, d = ref[250:290], ref[290:330], ref[333:360], ref[372:400]  # 40M 2I 40M 3D 27M 12N 28M
    a = a[:7] + ("A" if a[7] != "A" else "C") + a[8:30] + "N" + a[31:]
    c = c[:5] + ("G" if c[5] != "G" else "T") + c[6:]
    rs = syn.pack_reads([(250, 16, 60, "5S40M2I40M3D27M12N28M", "TTTTT" + a + "GA" + b + c + d)])
    rs.update(start=200, end=400, ref_bytes=np.frombuffer(ref.encode(), np.uint8), ref_first=0, min_mq=5)
    return rs
