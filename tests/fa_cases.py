"""Read sets shared by the tests of full alignment from reads: the golden sets, generated sets in coordinate order, small sets by hand, and the
sets that take the device form to its capacity edges (table_fill, indel_column, many_candidates) with what each is built to hold."""
import functools
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


FA_DROP_BITS = (0x4, 0x8, 0x100, 0x800)  # the bits of 2316


@functools.lru_cache(maxsize=None)  # (shared between tests and left unchanged by them)
def table_fill(levels, first_centre=300, spacing=200, skipped=0.3, short=0.3, seed=61):
    """(rs, ex, info): one group of M-only reads per entry of ``levels``, group g around the centre first_centre + g * spacing, in coordinate
    order, so that EXACTLY levels[g] kept reads overlap that centre's window.  A group opens with a long read over its centre (the prefix
    maximum of the ends then holds every later read of the group inside the candidate's read range) and closes with a read over its centre that carries the
    alt base: the table's last entry counts in every tally.
    In read order, a share ``short`` of the overlapping reads ends in [c - 15, c - 1] (in the window, not over the centre), and in between
    them, a share ``skipped`` of all reads, sit reads no window of c takes: one dropped flag bit of 2316 each in turn, a mapq below 5, or a
    kept read that ends at or in front of c - 16.  The starts step from c - 60 to c - 21, so the window of c - 56 holds about the first
    half of the group: with that centre in the call the short reads in front are kept reads (a read over no flanking position of any
    candidate is in no window at all).  One covering read in five carries info["alt"] at c.  Haplotypes cycle 0, 1, 2, both strands,
    every read its own quality.  info: centres, and per read pos / end / kept (by flag and mapq), whether it carries the alt base."""
    rng = np.random.default_rng(seed)
    n_ref = first_centre + spacing * len(levels) + 100
    ref = "".join(rng.choice(list("ACGT"), size=n_ref))
    reads, quals, haps, end_of, kept_of, alt_of = [], [], [], [], [], []
    for g, n_over in enumerate(levels):
        c = first_centre + g * spacing
        alt = "ACGT"[("ACGT".index(ref[c]) + 1) % 4]
        kinds, over, turn = ["cover"], 1, 0
        while over < n_over:
            if rng.random() < skipped:
                kinds.append(("flag", "flag", "flag", "flag", "mapq", "miss", "miss")[turn % 7])
                turn += 1
            else:
                kinds.append("short" if rng.random() < short else "cover")
                over += 1
        kinds[-1] = "cover"  # (the last read of the table is one that every tally counts, and carries the alt base)
        n_flag = 0
        for i, kind in enumerate(kinds):
            pos = c - 60 + 40 * i // len(kinds)
            end = {"short": c - 15 + int(rng.integers(0, 15)), "miss": c - 16 - int(rng.integers(0, 4))}.get(kind, c + 1 + int(rng.integers(0, 31)))
            flag, mapq = 16 * int(rng.integers(0, 2)), 5 + (7 * i) % 56
            if kind == "flag":
                flag |= FA_DROP_BITS[n_flag % 4]
                n_flag += 1
            if kind == "mapq":
                mapq = i % 5
            seq = ref[pos:end]
            carries = kind == "cover" and (i % 5 == 3 or i == len(kinds) - 1)
            if carries:
                seq = seq[:c - pos] + alt + seq[c - pos + 1:]
            n = len(reads)
            reads.append((pos, flag, mapq, f"{end - pos}M", seq))
            quals.append((11 * n) % 60), haps.append(n % 3), end_of.append(end), kept_of.append(kind not in ("flag", "mapq")), alt_of.append(carries)
    rs, ex = by_hand(reads, quals=quals, haps=haps, ref=ref)
    info = {"centres": [first_centre + g * spacing for g in range(len(levels))], "pos": rs["pos"].copy(), "end": np.array(end_of, np.int64),
            "kept": np.array(kept_of, bool), "alt": np.array(alt_of, bool), "ref": ref}
    return rs, ex, info


def window_numbers(info, c):
    """(overlapping kept reads, of them over c, of them with the alt base at c) of the window of centre c, by interval arithmetic alone"""
    over = info["kept"] & (info["pos"] < c + 17) & (info["end"] > c - 16)
    at = over & (info["pos"] <= c) & (info["end"] > c)
    return int(over.sum()), int(at.sum()), int((at & info["alt"]).sum())


def read_range(info, c):
    """(lo, hi) of the candidate's read range as the rule states it: hi the first read with pos >= c + 17, lo the first whose prefix
    maximum of ends is > c - 16 (over all reads: a dropped read's end counts too)"""
    hi = int(np.searchsorted(info["pos"], c + 17, side="left"))
    lo = int(np.searchsorted(np.maximum.accumulate(info["end"]), c - 16, side="right"))
    return lo, hi


INDEL_CENTRE, INDEL_REF = 130, "ACGT" * 100


@functools.lru_cache(maxsize=None)
def indel_column(extras=True):
    """(rs, ex, expected, kinds): 700 reads over centre 130 of "ACGT" * 100 in coordinate order, starts stepping over 25 positions.  Of every 7
    consecutive reads three carry an insertion behind the centre (G, GG, GT: two of one length and different bytes), two a deletion (of 1
    and of 2), two are plain.  extras adds, at read indices above 256: three reads with two consecutive I ops (G then GG), four with an I
    (GT) followed by a D of 2, and above index 512 the one read with the insertion TTT.  expected: (depth, {entry: count}) of the centre's
    line, by construction; kinds: what every read carries, in read order"""
    core = 700
    what = [("I", "G"), ("D", 1), None, ("I", "GG"), ("D", 2), ("I", "GT"), None]
    kinds = [what[i % 7] for i in range(core)]
    if extras:
        for at, kind in ((300, ("II", "G", "GG")), (301, ("II", "G", "GG")), (420, ("II", "G", "GG")), (330, ("ID", "GT", 2)), (331, ("ID", "GT", 2)),
                         (500, ("ID", "GT", 2)), (620, ("ID", "GT", 2)), (650, ("I", "TTT"))):
            kinds.insert(at, kind)
    c, ref = INDEL_CENTRE, INDEL_REF
    reads, count = [], {}
    for i, kind in enumerate(kinds):
        pos = c - 25 + 25 * i // len(kinds)
        head, m = ref[pos:c + 1], c + 1 - pos
        if kind is None:
            cigar, seq = f"{m + 20}M", head + ref[c + 1:c + 21]
        elif kind[0] == "I":
            cigar, seq = f"{m}M{len(kind[1])}I20M", head + kind[1] + ref[c + 1:c + 21]
        elif kind[0] == "D":
            cigar, seq = f"{m}M{kind[1]}D20M", head + ref[c + 1 + kind[1]:c + 21 + kind[1]]
        elif kind[0] == "II":
            cigar, seq = f"{m}M{len(kind[1])}I{len(kind[2])}I20M", head + kind[1] + kind[2] + ref[c + 1:c + 21]
        else:
            cigar, seq = f"{m}M{len(kind[1])}I{kind[2]}D20M", head + kind[1] + ref[c + 1 + kind[2]:c + 21 + kind[2]]
        for x in (kind or ())[1:]:
            key = "I" + ref[c] + x if isinstance(x, str) else "D" + ref[c + 1:c + 1 + x]
            count[key] = count.get(key, 0) + 1
        reads.append((pos, 16 * (i % 2), 20 + i % 41, cigar, seq))
    n = len(reads)
    count["R" + ref[c]] = n - sum(count.values())  # every read shows the reference base at the centre; each indel op is taken off
    rs, ex = by_hand(reads, quals=[(7 * i) % 60 for i in range(n)], haps=[i % 3 for i in range(n)], ref=ref)
    return rs, ex, (n, count), kinds


def alt_counts(line):
    """{entry: count} of one of the library's lines ("pos-depth-ref-K n K n ") -> (depth, dict)"""
    _, _, rest = line.partition("-")
    depth, _, rest = rest.partition("-")
    _, _, rest = rest.partition("-")
    items = rest.split(" ")
    return int(depth), {k: int(v) for k, v in zip(items[0::2], items[1::2]) if k}


def fill_centres(info):
    """the centres of a table_fill set and, in front of each, the centre 56 to its left"""
    return sorted([c - 56 for c in info["centres"]] + list(info["centres"]))


def check_fill(r, stats, info, depth):
    """counts, centre depths and the alt base's count of a table_fill call over fill_centres(info), against window_numbers"""
    centres = fill_centres(info)
    numbers = [window_numbers(info, c) for c in centres]
    assert r["counts"].tolist() == [min(n, depth) for n, _, _ in numbers] and r["depths"].tolist() == [at for _, at, _ in numbers]
    assert stats["deep_windows"] == sum(n > depth for n, _, _ in numbers) and stats["rows"] == int(r["counts"].sum())
    assert stats["reads_kept"] == int(info["kept"].sum()) and stats["reads_dropped"] == int((~info["kept"]).sum())
    lines = r["text"].decode("ascii").split("\n")[:-1]
    for c, line, (_, at, n_alt) in zip(centres, lines, numbers):
        if c in info["centres"]:
            alt = "ACGT"[("ACGT".index(info["ref"][c]) + 1) % 4]
            assert alt_counts(line) == (at, {"X" + alt: n_alt, "R" + info["ref"][c]: at - n_alt}) and n_alt > 0


BASE_OF_CH6 = {100: "A", 25: "C", 75: "G", 50: "T"}


def check_indel_rows(r, expected, window=1):
    """channel 5 of every row of the indel_column window: an insertion row (its string read back from channel 6) and a deletion row (its
    length from the zero cells behind the centre) carry int(float32(100) * (float32(count) / float32(depth))), a plain row 0.  Returns the
    numbers of insertion and deletion rows seen"""
    depth, count = expected
    first = int(r["counts"][:window].sum())
    seen = [0, 0]
    for w in r["rows"][first:first + int(r["counts"][window])]:
        shown = w[:, 0] != 0
        if w[16, 1] == -50:
            s = ""
            while w[16 + len(s), 6] != 0:
                s += BASE_OF_CH6[int(w[16 + len(s), 6])]
            n, seen[0] = count["I" + INDEL_REF[INDEL_CENTRE] + s], seen[0] + 1
        elif w[16, 1] == -100:
            d = 1 if w[18, 0] != 0 else 2
            assert w[17, 0] == 0 and w[17 + d, 0] != 0
            n, seen[1] = count["D" + INDEL_REF[INDEL_CENTRE + 1:INDEL_CENTRE + 1 + d]], seen[1] + 1
        else:
            assert not w[:, 5].any()
            continue
        af = int(np.float32(100) * (np.float32(n) / np.float32(depth)))
        assert 0 < af < 100 and (w[shown, 5] == af).all() and not w[~shown, 5].any() and shown[16]
    return seen


def many_candidates(n_centres, max_indel_length=10, **spec):
    """(rs, ex, centres): a generated set and n_centres adjacent centres that end at the last one the reference bytes allow, tens of
    windows behind the last read (make_read_set's reads stop 72 in front of the end of its reference)"""
    rs, ex = generated(**spec)
    last = rs["ref_first"] + len(rs["ref_bytes"]) - 17 - max_indel_length
    return rs, ex, np.arange(last + 1 - n_centres, last + 1)


def _many():
    from clair3_amd import _lib
    tile = _lib.lib().c3_pileup_tile_sites()  # full alignment scans its row counts with pileup's kernel: a step holds this many candidates
    return (2 * tile + 600,), dict(n_sites=2300, depth=20, read_len=(80, 300), seed=72), dict(matrix_depth=24, max_indel_length=10, seed=2)


MANY = _many()  # (arguments, spec) of many_candidates and the call's options: more candidates than two steps of the scan
# a batch for the chained predict: more windows than one scan step and than a ring lane takes, over-deep ones and, at the end, empty ones
RAGGED = (1200,), dict(n_sites=700, depth=60, read_len=(80, 300), seed=73), dict(matrix_depth=55, max_indel_length=10, seed=5)


def _lds_reads():
    from clair3_amd import _lib
    return _lib.lib().c3_fa_lds_reads()


LDS = _lds_reads()  # reads the candidate kernel's table holds
STEP = 256          # reads a step of its compaction and of every table loop takes
FILL_LEVELS = (STEP - 1, STEP, STEP + 1, LDS // 2, LDS - 1, LDS)
