"""What the pileup-from-reads tests share: the golden read sets (tests/golden/make_golden_pileup_reads.py) and a one-column read set."""
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
