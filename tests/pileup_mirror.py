"""A numpy and dict restatement of the pileup-from-reads rule, written from its description and not from the C: reads are walked one
reference position at a time, every column keeps plain dicts.  Slow and obvious on purpose; tests/test_pileup_reads.py holds the host C
form to it."""
from collections import defaultdict

import numpy as np

NT16 = "=ACMGRSVTWYHKDBN"
DROP = 0x4 | 0x100 | 0x800 | 0x200 | 0x400
BASE_CHANNEL = {1: 0, 2: 1, 4: 2, 8: 3}


def read_codes(rs, r):
    packed = rs["seq"][int(rs["seq_first"][r]):int(rs["seq_first"][r + 1])]
    codes = np.empty(2 * len(packed), np.uint8)
    codes[0::2], codes[1::2] = packed >> 4, packed & 15
    return codes


def read_ops(rs, r):
    return [(int(c) & 15, int(c) >> 4) for c in rs["cigar"][int(rs["cigar_first"][r]):int(rs["cigar_first"][r + 1])]]


_M64 = (1 << 64) - 1


def _mix(x):  # pileup_mix of csrc/c3_pileup.h: the finaliser of splitmix64
    x ^= x >> 30
    x = x * 0xbf58476d1ce4e5b9 & _M64
    x ^= x >> 27
    x = x * 0x94d049bb133111eb & _M64
    return x ^ x >> 31


def event_slots(rs, start, end, min_mq=5, hash_mask=_M64):
    """The device's event table restated in Python integers (pileup_walk_kernel of csrc/c3_pileup.h): the table's size from the I and D
    ops of the kept reads, and per distinct event its key, the slot its probe starts at and the slot linear probing gives it.  The set of
    occupied slots under linear probing does not depend on the order of insertion; which key sits where does, so ``wrapped`` is stated on
    what does not: more probes start at or behind some slot s than the table has slots from s to its last one -- whatever the order, one
    of them steps from the last slot to slot 0.
    Returns dict(cap, events, keys {event: key}, first {event: slot}, occupied, wrapped); an event is (column, reverse, is insertion, length, codes)"""
    indel_ops, events = 0, {}
    for r in range(len(rs["pos"])):
        if int(rs["flag"][r]) & DROP or int(rs["mapq"][r]) < min_mq:
            continue
        rev = 1 if int(rs["flag"][r]) & 16 else 0
        codes, ops = read_codes(rs, r), read_ops(rs, r)
        p, q = int(rs["pos"][r]), 0
        for k, (op, n) in enumerate(ops):
            if op in (1, 2):
                indel_ops += 1
                j = k - 1
                while j >= 0 and ops[j][0] == 6:
                    j -= 1
                if j >= 0 and ops[j][0] in (0, 7, 8, 2) and start <= p - 1 < end:
                    total = n
                    if op == 1:
                        for o2, n2 in ops[k + 1:]:
                            if o2 != 1:
                                break
                            total += n2
                    ev = (p - 1 - start, rev, int(op == 1), total, tuple(int(x) for x in codes[q:q + total]) if op == 1 else ())
                    events[ev] = events.get(ev, 0) + 1
            if op in (0, 7, 8, 2, 3):
                p += n
            if op in (0, 7, 8, 1, 4):
                q += n
    cap = 64
    while cap < 2 * indel_ops:
        cap <<= 1
    keys, first = {}, {}
    for ev in events:
        col, rev, ins, total, bases = ev
        h = 0
        for code in bases:
            h = ((h ^ code) * 0x100000001b3 + 0x9e3779b97f4a7c15) & _M64
        ident = col | rev << 40 | ins << 41
        keys[ev] = (_mix(ident) ^ _mix((h + total * 0xd6e8feb86659fd93) & _M64)) & hash_mask & ~(1 << 63)
        first[ev] = (_mix(keys[ev] ^ 0x2545f4914f6cdd1d) & 0xffffffff) & (cap - 1)
    occupied = set()
    for key in sorted(set(keys.values())):  # (any order gives the same set)
        s = first[next(ev for ev in keys if keys[ev] == key)]
        while s in occupied:
            s = (s + 1) & (cap - 1)
        occupied.add(s)
    starts = [first[next(ev for ev in keys if keys[ev] == key)] for key in set(keys.values())]
    wrapped = any(sum(t >= s for t in starts) > cap - s for s in starts)
    return {"cap": cap, "events": events, "keys": keys, "first": first, "occupied": occupied, "wrapped": wrapped}


def pileup(rs, start, end, ref_bytes, ref_first, min_depth=0, min_snp_af=0.0, min_indel_af=0.0, min_mq=5, max_indel_length=50,
           call_snp_only=False, gvcf=True, call_ht=False):
    ref = bytes(bytearray(ref_bytes))
    cols = {}  # position -> column

    def column(p):
        if p not in cols:
            cols[p] = {"ch": [0] * 18, "depth": 0, "del": [defaultdict(int), defaultdict(int)], "ins": [defaultdict(int), defaultdict(int)]}
        return cols[p]

    for r in range(len(rs["pos"])):
        if int(rs["flag"][r]) & DROP or int(rs["mapq"][r]) < min_mq:
            continue
        rev = 1 if int(rs["flag"][r]) & 16 else 0
        codes, ops = read_codes(rs, r), read_ops(rs, r)
        p, q = int(rs["pos"][r]), 0
        for k, (op, n) in enumerate(ops):
            if op in (0, 7, 8):  # M = X
                for i in range(n):
                    if start <= p + i < end:
                        c = column(p + i)
                        c["depth"] += 1
                        code = int(codes[q + i])
                        if code in BASE_CHANNEL:
                            c["ch"][BASE_CHANNEL[code] + 9 * rev] += 1
                p, q = p + n, q + n
            elif op == 2:  # D
                for i in range(n):
                    if start <= p + i < end:
                        c = column(p + i)
                        c["depth"] += 1
                        c["ch"][8 + 9 * rev] += 1
                p += n
            elif op == 3:  # N
                for i in range(n):
                    if start <= p + i < end:
                        column(p + i)
                p += n
            elif op in (1, 4):  # I S
                q += n
            if op not in (0, 7, 8, 2) or not start <= p - 1 < end:
                continue
            rest = [x for x in ops[k + 1:]]
            while rest and rest[0][0] == 6:
                rest.pop(0)
            if not rest:
                continue
            if rest[0][0] == 1:
                total = 0
                for o2, n2 in rest:
                    if o2 != 1:
                        break
                    total += n2
                column(p - 1)["ins"][rev]["".join(NT16[int(x)] for x in codes[q:q + total])] += 1
            elif rest[0][0] == 2:
                column(p - 1)["del"][rev][rest[0][1]] += 1

    n_sites = end - start
    n_ref, n_total = np.zeros(n_sites if gvcf else 0, np.int64), np.zeros(n_sites if gvcf else 0, np.int64)
    counts, major, lines, cand_pos, cand_depth = [], [], [], [], []
    f32 = np.float32
    for p in sorted(cols):
        c = cols[p]
        ch = list(c["ch"])
        for s in (0, 1):
            ch[6 + 9 * s], ch[7 + 9 * s] = sum(c["del"][s].values()), max(c["del"][s].values(), default=0)
            ch[4 + 9 * s], ch[5 + 9 * s] = sum(c["ins"][s].values()), max(c["ins"][s].values(), default=0)
        raw = ref[p - ref_first]
        ref_base = raw - 32 if ord("a") <= raw <= ord("z") else raw
        r = {ord("C"): 1, ord("G"): 2, ord("T"): 3}.get(ref_base, 0)
        ref_count = alt_count = all_alt = 0
        major_alt = 0
        for i in range(4):
            both = ch[i] + ch[9 + i]
            if i == r:
                ref_count = both
            elif both > alt_count:
                alt_count, major_alt = both, ord("ACGT"[i])
                all_alt += alt_count
        del_count, ins_count = ch[6] + ch[15], ch[4] + ch[13]
        x = [ch[i] + ch[9 + i] for i in range(4)]
        ch[r], ch[9 + r] = -sum(ch[0:4]), -sum(ch[9:13])
        counts.append(ch), major.append(p)
        if gvcf:
            n_ref[p - start], n_total[p - start] = ref_count, ref_count + all_alt + del_count + ins_count
        depth = max(1, c["depth"])
        # the flanking count: consecutive existing columns directly to the left, reset by a gap and behind position 0
        flank, t = 0, p
        while t - 1 in cols and t - 1 != 0 and flank < 16:
            flank, t = flank + 1, t - 1
        majority = ref_count < alt_count or ref_count < ins_count or ref_count < del_count
        tie = ref_count > 0 and ref_count == alt_count and ref_base - major_alt < 0
        snp = f32(alt_count) / f32(depth) >= f32(min_snp_af)
        if call_snp_only:
            ok = snp
        else:
            ok = majority or tie or snp or f32(del_count) / f32(depth) >= f32(min_indel_af) or f32(ins_count) / f32(depth) >= f32(min_indel_af)
        ok = ok and depth >= min_depth and ref_base in b"ACGT" and (call_ht or flank >= 16)
        if not ok:
            continue
        line = f"{p + 1}-{depth}-{chr(ref_base)}-"
        for i in range(4):
            if i != r and x[i] > 0:
                line += f"X{'ACGT'[i]} {x[i]} "
        dels = defaultdict(int)
        for s in (0, 1):
            for n, v in c["del"][s].items():
                dels[n] += v
        for n in sorted(dels):
            if n <= max_indel_length:
                line += "D" + ref[p - ref_first + 1:p - ref_first + 1 + n].decode("latin-1") + f" {dels[n]} "
        inss = defaultdict(int)
        for s in (0, 1):
            for b, v in c["ins"][s].items():
                inss[b] += v
        for b in sorted(inss, key=lambda b: (len(b), b.encode())):
            if len(b) <= max_indel_length:
                line += f"I{chr(ref_base)}{b} {inss[b]} "
        ref_depth = ref_count - del_count - ins_count
        if ref_depth > 0:
            line += f"R{chr(ref_base)} {ref_depth} "
        lines.append(line), cand_pos.append(p), cand_depth.append(depth)
    return {"counts": np.array(counts, np.int32).reshape(-1, 18), "major": np.array(major, np.int64), "lines": lines,
            "cand_pos": np.array(cand_pos, np.int64), "cand_depth": np.array(cand_depth, np.int32), "n_ref": n_ref, "n_total": n_total}
