"""A Python mirror of the haplotag rule, written from the description in clair3_amd/csrc/c3_hap_rule.h (not from its code): it walks every
read's CIGAR once with a cursor over the variants, as the description's clauses are ordered, where the C++ resolves every pair on its own
by binary search.  tests/test_haplotag.py and tests/test_haplotag_gpu.py hold the host and device forms to it on generated read sets."""
import numpy as np

NT16 = "=ACMGRSVTWYHKDBN"
OVERHANG = 10
M_OPS = (0, 7, 8)  # M = X


def edit_distance(a, b):
    """Levenshtein distance of two byte strings, the textbook two-row form"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        row = [i]
        for j, y in enumerate(b, 1):
            row.append(min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = row
    return prev[-1]


def c_string(b):
    """what strlen sees of a buffer"""
    return b.split(b"\0", 1)[0]


def context(ops, order, first_part, want):
    """(reference bases, query bases) of a context walk over ``ops`` taken in ``order``; the first op counts with ``first_part`` bases.
    (0, 0) when the ops run out before ``want`` reference bases are consumed"""
    ref = query = 0
    for n, k in enumerate(order):
        op, length = ops[k]
        if n == 0:
            length = first_part
        if length == 0:
            continue
        if op in M_OPS:
            ref, query = ref + length, query + length
            if ref >= want:
                return want, query - (ref - want)
        elif op == 2:
            ref += length
            if ref >= want:
                return want, query
        elif op == 1:
            query += length
        elif op == 3:
            return want, query
    return 0, 0


def realign(ops, k, consumed, query_pos, letters, v, alt_base, ref, ref_first):
    length = ops[k][1]
    left_ref, left_query = context(ops, range(k, -1, -1), consumed, OVERHANG)
    right_ref, right_query = context(ops, range(k, len(ops)), max(length - consumed, 0), OVERHANG + 1)
    q0, q1 = query_pos - left_query, query_pos + right_query
    if q0 == q1:
        return 0
    query = letters[q0:q1]
    ref_buf = bytes(ref[v - left_ref - ref_first:v + right_ref - ref_first])
    ref_s = c_string(ref_buf)
    alt_buf = bytearray(len(ref_buf) + 2)
    alt_buf[:len(ref_s)] = ref_s
    alt_buf[left_ref] = alt_base
    alt_s = c_string(bytes(alt_buf))
    d_ref, d_alt = edit_distance(query, ref_s), edit_distance(query, alt_s)
    return 1 if d_ref < d_alt else 2 if d_ref > d_alt else 0


def haplotag(rs, variants, ref, ref_first, min_haplotag_mq=20):
    """(hap, alleles, pair_first) as c3_fa_haplotag_result gives them"""
    vpos = [int(p) for p in variants["pos"]]
    valt, vgt, vps = variants["alt_base"], variants["genotype"], variants["phase_set"]
    n = len(rs["pos"])
    hap, alleles, pair_first = np.zeros(n, np.uint8), [], [0]
    ref = np.asarray(ref, np.uint8)
    for r in range(n):
        if int(rs["mapq"][r]) < min_haplotag_mq or not vpos:
            pair_first.append(len(alleles))
            continue
        ops = [(int(c) & 15, int(c) >> 4) for c in rs["cigar"][rs["cigar_first"][r]:rs["cigar_first"][r + 1]]]
        packed = rs["seq"][rs["seq_first"][r]:rs["seq_first"][r + 1]]
        codes = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)
        letters = bytes(ord(NT16[c]) for c in codes)
        ref_pos, query_pos = int(rs["pos"][r]), 0
        j = int(np.searchsorted(vpos, ref_pos))
        cost = {}

        def pair(k, consumed, q):
            a = realign(ops, k, consumed, q, letters, vpos[j], int(valt[j]), ref, ref_first)
            alleles.append(a)
            if a:
                cost[int(vps[j])] = cost.get(int(vps[j]), 0) + (1 if a == int(vgt[j]) else -1)

        for k, (op, length) in enumerate(ops):
            if op in M_OPS:
                while j < len(vpos) and vpos[j] < ref_pos + length:
                    pair(k, vpos[j] - ref_pos, query_pos + vpos[j] - ref_pos)
                    j += 1
                ref_pos, query_pos = ref_pos + length, query_pos + length
            elif op == 1:
                if j < len(vpos) and vpos[j] == ref_pos:
                    pair(k, 0, query_pos)
                    j += 1
                query_pos += length
            elif op == 2:
                while j < len(vpos) and vpos[j] < ref_pos + length:
                    pair(k, vpos[j] - ref_pos, query_pos)
                    j += 1
                ref_pos += length
            elif op == 3:
                while j < len(vpos) and vpos[j] < ref_pos + length:
                    alleles.append(0)
                    j += 1
                ref_pos += length
            elif op == 4:
                query_pos += length
        pair_first.append(len(alleles))
        if cost:
            hi, lo = max(0, max(cost.values())), min(0, min(cost.values()))
            hap[r] = 0 if hi == 0 and lo == 0 else 1 if hi > -lo else 2
    return hap, np.array(alleles, np.int8), np.array(pair_first, np.int64)


# ---- the read sets both test files use
def periodic_ref(n=400):
    return np.frombuffer((b"ACGT" * (n // 4 + 1))[:n], np.uint8).copy()


def variants_of(pos, alt, genotype, phase_set):
    return {"pos": np.array(pos, np.int64), "alt_base": np.frombuffer(alt.encode(), np.uint8).copy(), "genotype": np.array(genotype, np.uint8),
            "phase_set": np.array(phase_set, np.int32)}


def hand_read(cigar, first=100, mapq=60, carry=None, inserted="", ref=None):
    """one read at ``first`` over the periodic reference (or ``ref``, a changed copy of it): it carries the periodic bases except at the
    positions of ``carry`` ({position: base});
    I ops take their bases from ``inserted``, S ops are 'T's"""
    import re
    from clair3_amd import synthetic as syn
    ref, carry = periodic_ref() if ref is None else ref, carry or {}
    at, seq, ins = first, [], iter(inserted)
    for m in re.finditer(r"(\d+)([MIDNSHP=X])", cigar):
        n, op = int(m.group(1)), m.group(2)
        if op in "M=X":
            seq += [carry.get(p, "ACGT"[p % 4]) for p in range(at, at + n)]
        elif op == "I":
            seq += [next(ins) for _ in range(n)]
        elif op == "S":
            seq += ["T"] * n
        if op in "M=XDN":
            at += n
    rs = syn.pack_reads([(first, 0, mapq, cigar, "".join(seq))])
    rs.update(ref_bytes=ref, ref_first=0)
    return rs


def hand_cases():
    """(name, read set, variants, the expected tag).  The reference's own functions gave exactly these tags on every one of them (run
    through the driver of tests/golden/make_golden_haplotag.py when this file was written)"""
    alt110 = {110: "T"}  # the reference has G at 110
    return [
        ("a_alt_gt2", hand_read("30M", carry=alt110), variants_of([110], "T", [2], [1]), 1),
        ("a_alt_gt1", hand_read("30M", carry=alt110), variants_of([110], "T", [1], [1]), 2),
        ("b_mapq19", hand_read("30M", mapq=19, carry=alt110), variants_of([110], "T", [2], [1]), 0),
        # no right context in the last 10 bases: the read carries the alt base at 125 and still votes "reference"
        ("c_tail_gt1", hand_read("30M", carry={125: "A"}), variants_of([125], "A", [1], [1]), 1),
        ("c_tail_gt2", hand_read("30M", carry={125: "A"}), variants_of([125], "A", [2], [1]), 2),
        ("d_two_sets", hand_read("30M", carry=alt110), variants_of([110, 115], "TA", [2, 2], [1, 2]), 2),
        ("d_one_set", hand_read("30M", carry=alt110), variants_of([110, 115], "TA", [2, 2], [1, 1]), 0),
        ("e_at_insertion_alt", hand_read("15M2I15M", carry={115: "G"}, inserted="CC"), variants_of([115], "G", [2], [1]), 1),
        ("e_at_insertion_ref", hand_read("15M2I15M", inserted="CC"), variants_of([115], "G", [2], [1]), 2),
        ("head_no_left_context", hand_read("30M", carry={105: "A"}), variants_of([105], "A", [2], [1]), 1),
        ("short_read_no_context", hand_read("9M", carry={104: "G"}), variants_of([104], "G", [2], [1]), 0),
        ("insertion_behind_the_end", hand_read("30M3I4S", inserted="GGG"), variants_of([130], "T", [1], [1]), 1),
        ("inside_deletion", hand_read("12M3D15M"), variants_of([113], "T", [1], [1]), 0),
        ("inside_n", hand_read("12M6N12M"), variants_of([114], "T", [1], [1]), 0),
    ]


def rough_sets():
    """(name, read set, variants): generated sets with what the golden sets leave out"""
    from clair3_amd import synthetic as syn
    out = []
    specs = [("eqx_pad", dict(eqx=True, pad=0.4, ins=0.02, dele=0.02)), ("d_i", dict(d_then_i=0.012, i_then_d=0.012, ins=0.01, dele=0.01)),
             ("non_acgt_ref_other", dict(non_acgt=0.03, ref_other=0.08)), ("n_ops", dict(n_op=0.006, ins=0.01, dele=0.01, soft_clip=0.8))]
    for k, (name, kw) in enumerate(specs):
        rs = syn.sort_read_set(syn.make_read_set(120, 12, (60, 200), 9300 + k, **kw))
        out.append((name, rs, syn.make_phased_variants(rs, 9400 + k, rate=0.02, near=range(2, len(rs["pos"]), 11), dense=(2040, 2070))))
    rs = syn.sort_read_set(syn.make_read_set(60, 8, (60, 120), 9350, ins=0.01, dele=0.01))
    lo, hi = int(rs["ref_first"]) + 10, int(rs["ref_first"]) + len(rs["ref_bytes"]) - 11
    pos = np.arange(lo, hi, 2)
    rng = np.random.default_rng(9351)
    out.append(("every_2_bases", rs, {"pos": pos, "alt_base": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(pos))],
                                      "genotype": rng.integers(1, 3, len(pos)).astype(np.uint8), "phase_set": (pos // 40).astype(np.int32)}))
    # insertions of 100+ bases inside a context, and N ops inside one
    ref = periodic_ref(800)
    reads = []
    for k, cigar in enumerate(("20M120I30M", "8M100I5M150I40M", "30M221I30M", "25M5N25M", "12M3N3M2N30M", "5S14M101I2D20M6S")):
        r = hand_read(cigar, first=100 + 3 * k, inserted="ACGGTCA" * 60, ref=ref)
        reads.append((100 + 3 * k, 0, 60, cigar, "".join(NT16[c] for c in np.stack([r["seq"] >> 4, r["seq"] & 15], 1).reshape(-1))[:int(syn.query_lengths(r)[0])]))
    rs = syn.pack_reads(reads)
    rs.update(ref_bytes=ref, ref_first=0)
    pos = np.arange(96, 190, 3)
    out.append(("long_insertions_n_ops", rs, {"pos": pos, "alt_base": np.full(len(pos), ord("T"), np.uint8), "genotype": np.ones(len(pos), np.uint8),
                                              "phase_set": (pos // 30).astype(np.int32)}))
    return out
