"""Full alignment from reads in plain Python / numpy, written from the rule's description (csrc/c3_fa_rule.h) in the shape of the reference's
loop: a walker per read that fills a table per flanking position, then a loop over the candidates.  It does not use the library; only
synthetic.fa_keys / subsample_rank (the counter hash of deviation (a)) come from the package."""
import numpy as np

from clair3_amd import synthetic as syn

NT16 = "=ACMGRSVTWYHKDBN"
COUNT_BASE = {"A": 100, "C": 25, "D": -100, "G": 75, "I": -50, "N": 100, "T": 50}
ACGT_NUM = {"C": 1, "G": 2, "T": 3}
HAP_V = (60, 30, 90)


class RefSkip(Exception):
    pass


def _code(seq, first, q):
    return (int(seq[first + (q >> 1)]) >> (0 if q & 1 else 4)) & 15


def walk_read(rs, ex, r, flank):
    """{position: [base char or None when deleted, bq, insertion strings in op order, deletion length]} over the flanking positions the
    read spans, and the read's end"""
    info = {}
    pos, q = int(rs["pos"][r]), 0
    start = pos
    sf, qf = int(rs["seq_first"][r]), int(ex["qual_first"][r])
    for k in range(int(rs["cigar_first"][r]), int(rs["cigar_first"][r + 1])):
        op, ln = int(rs["cigar"][k]) & 15, int(rs["cigar"][k]) >> 4
        if op in (0, 7, 8):
            for p in range(pos, pos + ln):
                if p in flank:
                    e = info.setdefault(p, [None, 0, [], 0])
                    b = int(ex["qual"][qf + q])
                    e[0], e[1] = NT16[_code(rs["seq"], sf, q)], int(100 * b / 40.0) if b < 40 else 100
                q += 1
            pos += ln
        elif op == 2:
            if pos - 1 >= start and pos - 1 in flank:
                info.setdefault(pos - 1, [None, 0, [], 0])[3] = ln
            for p in range(pos, pos + ln):
                if p in flank:
                    info.setdefault(p, [None, 0, [], 0])[0] = None
            pos += ln
        elif op == 1:
            if pos - 1 >= start and pos - 1 in flank:
                info.setdefault(pos - 1, [None, 0, [], 0])[2].append("".join(NT16[_code(rs["seq"], sf, q + i)] for i in range(ln)))
            q += ln
        elif op == 3:
            if any(p in flank for p in range(pos, pos + ln)):
                raise RefSkip(f"read {r}")
            pos += ln
        elif op == 4:
            q += ln
    return info, pos


def fa_mirror(rs, ex, centres, ref_bytes, ref_first, min_mq=5, max_indel_length=50, matrix_depth=89, seed=0, names=True):
    """(rows (n_rows, 33, 8) int8, counts, depths, lines)"""
    centres = [int(c) for c in centres]
    flank = set()
    for c in centres:
        flank.update(range(c - 16, c + 17))
    ref = bytes(np.asarray(ref_bytes, np.uint8)).decode("latin-1").upper()
    seen, reads = set(), []  # reads: (index, start, end, info)
    for r in range(len(rs["pos"])):
        if int(rs["flag"][r]) & syn.FA_DROP_FLAGS or int(rs["mapq"][r]) < min_mq:
            continue
        if names and ex.get("name_key") is not None:
            if int(ex["name_key"][r]) in seen:
                continue
            seen.add(int(ex["name_key"][r]))
        info, end = walk_read(rs, ex, r, flank)
        if not any(p in flank for p in range(int(rs["pos"][r]), end)):
            continue
        reads.append((r, int(rs["pos"][r]), end, info))
    rows, counts, depths, lines = [], [], [], []
    for c in centres:
        over = [x for x in reads if x[1] < c + 17 and x[2] > c - 16]
        # the centre tallies over ALL overlapping reads
        depth, acgt, ins_n, del_n = 0, [0, 0, 0, 0], {}, {}
        for _, _, _, info in over:
            e = info.get(c)
            if e is None:
                continue
            depth += 1
            if e[0] is not None:
                acgt[ACGT_NUM.get(e[0], 0)] += 1
            for s in e[2]:
                ins_n[s] = ins_n.get(s, 0) + 1
            if e[3]:
                del_n[e[3]] = del_n.get(e[3], 0) + 1
        if len(over) > matrix_depth:
            keep = syn.subsample_rank(syn.fa_keys(seed, c, [x[0] for x in over]), matrix_depth)
            over = [x for x, k in zip(over, keep) if k]
        over.sort(key=lambda x: (int(ex["haplotype"][x[0]]), x[0]))
        counts.append(len(over)), depths.append(depth)
        for r, _, _, info in over:
            m = np.zeros((33, 8), np.int8)
            alt = None
            for p in range(33):
                e = info.get(c - 16 + p)
                if e is None or e[0] is None:
                    continue
                ref_base = ref[c - 16 + p - ref_first]
                alt_v = 0
                if e[2]:
                    s = e[2][-1]
                    if p < 32:
                        for i in range(min(len(s), 33 - p)):
                            m[p + i, 6] = COUNT_BASE.get(s[i], 0)
                    if p == 16:
                        alt = ("I", s)
                    alt_v = -50
                elif e[3]:
                    if p == 16:
                        alt = ("D", e[3])
                    alt_v = -100
                elif e[0] != ref_base:
                    if p == 16:
                        alt = ("X", e[0])
                    alt_v = COUNT_BASE.get(e[0], 0)
                mq = int(rs["mapq"][r])
                m[p, 0], m[p, 1], m[p, 2] = COUNT_BASE.get(ref_base, 0), alt_v, 50 if int(rs["flag"][r]) & 16 else 100
                m[p, 3], m[p, 4], m[p, 7] = int(100 * mq / 60.0) if mq < 60 else 100, e[1], HAP_V[int(ex["haplotype"][r])]
            if alt is not None:
                n = ins_n[alt[1]] if alt[0] == "I" else del_n[alt[1]] if alt[0] == "D" else acgt[ACGT_NUM.get(alt[1], 0)]
                x = np.float32(n) / np.float32(depth)
                af = int(np.float32(100) * x) if x < 1.0 else 100
                if af > 0:
                    m[m[:, 0] != 0, 5] = af
            rows.append(m)
        rb = ref[c - ref_first]
        ri = ACGT_NUM.get(rb, 0)
        line = f"{c + 1}-{depth}-{rb}-"
        for j in range(4):
            if j != ri and acgt[j] > 0:
                line += f"X{'ACGT'[j]} {acgt[j]} "
        raw = bytes(np.asarray(ref_bytes, np.uint8)).decode("latin-1")
        for ln in sorted(del_n):
            if ln <= max_indel_length:
                line += f"D{raw[c - ref_first + 1:c - ref_first + 1 + ln]} {del_n[ln]} "
        for s in sorted(ins_n, key=lambda s: (len(s), s)):
            if len(s) <= max_indel_length:
                line += f"I{rb}{s} {ins_n[s]} "
        ref_count = acgt[ri] - sum(ins_n.values()) - sum(del_n.values())
        if ref_count > 0:
            line += f"R{rb} {ref_count} "
        lines.append(line)
    rows = np.stack(rows) if rows else np.zeros((0, 33, 8), np.int8)
    return rows, np.array(counts, np.int32), np.array(depths, np.int32), lines
