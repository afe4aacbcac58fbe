"""The dwell channel in plain Python, written from the rule's description (csrc/c3_dwell_rule.h) in the shape of the reference's loops: the
signal lengths of a read by one pass over its move table, then a walker per read that fills a table per flanking position op by op, then a
loop over the candidates.  Channels 0 .. 7 are tests/fa_mirror.py as it is; the rows' reads are chosen again here by the same rule (and
checked against fa_mirror's counts).  It does not use the library; only synthetic.fa_keys / subsample_rank come from the package."""
import numpy as np

from clair3_amd import synthetic as syn
from tests.fa_mirror import fa_mirror, walk_read


def signal_lengths(mv, l, reverse):
    """the reference's loop: None (no table) or a list of l ints"""
    if len(mv) <= 1 or l == 0:
        return None
    sig = [0] * l
    base = -1
    for idx in range(1, len(mv)):
        if int(mv[idx]) != 0:
            base += 1
            if base >= l:
                break
            sig[base] += 1
        elif base >= 0:
            sig[base] += 1
    return sig[::-1] if reverse else sig


def walk_dwell(rs, r, sig, l, flank):
    """({position: signal sum or None when deleted}, {position: the kinds of cell it is}) over the flanking positions the read spans"""
    info, ops_at, kinds = {}, {}, {}
    pos, q = int(rs["pos"][r]), 0
    start = pos
    for k in range(int(rs["cigar_first"][r]), int(rs["cigar_first"][r + 1])):
        op, ln = int(rs["cigar"][k]) & 15, int(rs["cigar"][k]) >> 4
        if op in (0, 7, 8):
            for p in range(pos, pos + ln):
                if p in flank:
                    info[p] = sig[q] if sig is not None and q < l else 0
                q += 1
            pos += ln
        elif op == 2:
            if pos - 1 >= start and pos - 1 in flank:
                ops_at.setdefault(pos - 1, []).append("D")
            for p in range(pos, pos + ln):
                if p in flank:
                    info[p] = None
            pos += ln
        elif op == 1:
            if pos - 1 >= start and pos - 1 in flank:
                ops_at.setdefault(pos - 1, []).append("I")
                if info.get(pos - 1) is not None and sig is not None:
                    total = 0
                    for i in range(ln):
                        if q + i < l:
                            total += sig[q + i]
                    info[pos - 1] += total
                    if total > 0:
                        kinds.setdefault(pos - 1, set()).add("ins_nonzero")
            q += ln
        elif op == 3:
            pos += ln
        elif op == 4:
            q += ln
    for p, ops in ops_at.items():
        shown = info.get(p) is not None
        for name, hit in (("two_i", shown and ops.count("I") >= 2), ("i_then_d", shown and ops[0] == "I" and "D" in ops),
                          ("d_then_i", not shown and "I" in ops)):
            if hit:
                kinds.setdefault(p, set()).add(name)
    return info, kinds


def dwell_mirror(rs, ex, moves, centres, ref_bytes, ref_first, min_mq=5, max_indel_length=50, matrix_depth=89, seed=0, names=True):
    """(rows (n_rows, 33, 9) int8, counts, depths, lines, seen)"""
    rows8, counts, depths, lines = fa_mirror(rs, ex, centres, ref_bytes, ref_first, min_mq=min_mq, max_indel_length=max_indel_length,
                                             matrix_depth=matrix_depth, seed=seed, names=names)
    centres = [int(c) for c in centres]
    flank = set()
    for c in centres:
        flank.update(range(c - 16, c + 17))
    seen = dict.fromkeys(("ins_nonzero", "two_i", "i_then_d", "d_then_i", "reverse_cells", "wrapped_128", "wrapped_256", "untagged_reads",
                          "k_below_l", "k_above_l"), 0)
    names_seen, reads = set(), []
    for r in range(len(rs["pos"])):
        if int(rs["flag"][r]) & syn.FA_DROP_FLAGS or int(rs["mapq"][r]) < min_mq:
            continue
        if names and ex.get("name_key") is not None:
            if int(ex["name_key"][r]) in names_seen:
                continue
            names_seen.add(int(ex["name_key"][r]))
        _, end = walk_read(rs, ex, r, flank)
        if not any(p in flank for p in range(int(rs["pos"][r]), end)):
            continue
        l = int(ex["qual_first"][r + 1]) - int(ex["qual_first"][r])
        mv = moves["mv"][int(moves["mv_first"][r]):int(moves["mv_first"][r + 1])]
        reverse = bool(int(rs["flag"][r]) & 16)
        sig = signal_lengths(mv, l, reverse)
        k = int(np.count_nonzero(mv[1:]))
        seen["untagged_reads"] += sig is None
        seen["k_below_l"] += sig is not None and k < l
        seen["k_above_l"] += sig is not None and k > l
        reads.append((r, int(rs["pos"][r]), end, walk_dwell(rs, r, sig, l, flank), reverse))
    ch8 = []
    for i, c in enumerate(centres):
        over = [x for x in reads if x[1] < c + 17 and x[2] > c - 16]
        if len(over) > matrix_depth:
            keep = syn.subsample_rank(syn.fa_keys(seed, c, [x[0] for x in over]), matrix_depth)
            over = [x for x, k in zip(over, keep) if k]
        over.sort(key=lambda x: (int(ex["haplotype"][x[0]]), x[0]))
        assert len(over) == counts[i]
        for _, _, _, (info, kinds), reverse in over:
            col = np.zeros(33, np.int8)
            for p in range(33):
                s = info.get(c - 16 + p)
                for name in kinds.get(c - 16 + p, ()):
                    seen[name] += 1
                if s is None:
                    continue
                col[p] = ((s + 128) % 256) - 128  # (int8_t) of the int32 sum
                seen["reverse_cells"] += reverse
                seen["wrapped_128"] += 128 <= s < 256
                seen["wrapped_256"] += s >= 256
            ch8.append(col)
    rows = np.zeros((len(rows8), 33, 9), np.int8)
    rows[:, :, :8] = rows8
    if ch8:
        rows[:, :, 8] = np.stack(ch8)
    return rows, counts, depths, lines, seen
