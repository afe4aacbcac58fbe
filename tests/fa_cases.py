"""Read sets shared by the tests of full alignment from reads: the golden sets, generated sets in coordinate order, and small sets by hand."""
import os

import numpy as np

from clair3_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fa_reads.npz")
READ_FIELDS = ("pos", "flag", "mapq", "cigar_first", "cigar", "seq_first", "seq")
EXTRA_FIELDS = ("qual_first", "qual", "haplotype", "name_key")


def golden_sets():
    """(k, rs, ex, centres, expected) per set of the fixture; expected: rows, counts, alt"""
    with np.load(GOLDEN) as z:
        for k in range(int(z["n_sets"])):
            rs = {n: z[f"{k}_{n}"] for n in READ_FIELDS}
            rs["ref_bytes"], rs["ref_first"], rs["min_mq"] = z[f"{k}_ref"], int(z[f"{k}_ref_first"]), int(z["min_mq"])
            ex = {n: z[f"{k}_{n}"] for n in EXTRA_FIELDS}
            yield k, rs, ex, z[f"{k}_centres"], {"rows": z[f"{k}_rows"], "counts": z[f"{k}_counts"], "alt": z[f"{k}_alt"]}


def generated(seed, extras_seed=None, duplicate_names=0.02, phased=0.6, **spec):
    """(rs, ex) of synthetic.make_read_set(**spec) in coordinate order"""
    rs0 = syn.make_read_set(seed=seed, **spec)
    ex0 = syn.make_read_extras(rs0, seed + 1 if extras_seed is None else extras_seed, phased=phased, duplicate_names=duplicate_names)
    return syn.sort_read_set(rs0), syn.sort_read_extras(rs0, ex0)


def by_hand(reads, quals=None, haps=None, names=None, ref="ACGT" * 100, ref_first=0):
    """(rs, ex) from a list of (pos, flag, mapq, cigar, seq) in the order given; quals: per read a list or one value for every base"""
    rs = syn.pack_reads(reads)
    rs["ref_bytes"], rs["ref_first"] = np.frombuffer(ref.encode(), np.uint8), ref_first
    qlen = syn.query_lengths(rs)
    quals = [30] * len(reads) if quals is None else quals
    q = [np.full(int(n), v, np.uint8) if np.isscalar(v) else np.asarray(v, np.uint8) for n, v in zip(qlen, quals)]
    ex = {"qual_first": np.concatenate([[0], np.cumsum([len(x) for x in q])]).astype(np.int64),
          "qual": np.concatenate(q) if q else np.zeros(0, np.uint8),
          "haplotype": np.array([0] * len(reads) if haps is None else haps, np.uint8),
          "name_key": np.arange(1, len(reads) + 1, dtype=np.uint64) if names is None else np.array(names, np.uint64)}
    return rs, ex


def alt_counts(line):
    """{entry: count} of one of the library's lines ("pos-depth-ref-K n K n ") -> (depth, dict)"""
    _, _, rest = line.partition("-")
    depth, _, rest = rest.partition("-")
    _, _, rest = rest.partition("-")
    items = rest.split(" ")
    return int(depth), {k: int(v) for k, v in zip(items[0::2], items[1::2]) if k}
