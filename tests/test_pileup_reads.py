"""Pileup from reads, the host form (c3_pileup_reads_host; no GPU): against the golden columns of the reference's generate_tensor
(tests/golden/make_golden_pileup_reads.py), against the numpy / dict mirror (tests/pileup_mirror.py), on hand-worked columns, and its errors."""
import numpy as np
import pytest

from clair3_amd import _lib, pileup_reads as pr, synthetic as syn
from tests import pileup_mirror as pm
from tests.pileup_cases import FIELDS, LONG_CIGARS, MANY_CANDIDATES, WRAP_SHIFT, big_region, distinct_events, golden_sets, insertion_column


def host(rs, start=None, end=None, **cfg):
    return pr.pileup_counts(rs, rs["start"] if start is None else start, rs["end"] if end is None else end, rs["ref_bytes"], rs["ref_first"], path="host", **cfg)


def parse_line(line):
    """(pos, depth, ref base, {key: count}) of an alt-info line"""
    pos, depth, ref, rest = line.split("-", 3)
    items = rest.split(" ")
    assert items[-1] == "" and len(items) % 2 == 1
    return int(pos), int(depth), ref, {items[i]: int(items[i + 1]) for i in range(0, len(items) - 1, 2)}


def test_host_form_equals_the_reference_columns():
    n = 0
    for k, rs, want in golden_sets():
        counts, major, lines, _ = host(rs, min_mq=rs["min_mq"], max_indel_length=100, call_ht=True)
        assert np.array_equal(major, want["major"]), k
        assert np.array_equal(counts, want["channels"]), k
        assert len(lines) == len(major), "thresholds at zero and call_ht: every column is a candidate"
        for line, p, depth, alleles in zip(lines, want["major"], want["depth"], want["alleles"]):
            pos, d, _ref, entries = parse_line(line)
            assert (pos, d) == (p + 1, depth)
            got = ";".join(f"{key} {v}" for key, v in sorted(entries.items()) if key[0] in "XID")
            assert got == str(alleles), (k, p)
        n += len(major)
    assert n > 900


MIRROR_CASES = {
    "plain": dict(n_sites=260, depth=24, read_len=(150, 400), seed=11),
    "odd": dict(n_sites=220, depth=20, read_len=(150, 400), seed=12, n_op=0.003, non_acgt=0.03, d_then_i=0.004, i_then_d=0.004, pad=0.2, eqx=True, gaps=2,
                ref_other=0.03),
    "long_cigars": LONG_CIGARS,  # reads of more than 64 and more than 128 ops: the op table's carry between its steps
}
MIRROR_CONFIGS = {
    "defaults": dict(),
    "thresholds": dict(min_snp_af=0.08, min_indel_af=0.15),
    "call_snp_only": dict(call_snp_only=True, min_snp_af=0.08, min_indel_af=0.15),
    "call_ht": dict(call_ht=True, min_snp_af=0.08, min_indel_af=0.15),
    "min_depth": dict(min_depth=18, min_snp_af=0.08, min_indel_af=0.15),
    "max_indel_50": dict(max_indel_length=50, min_snp_af=0.08, min_indel_af=0.15),
    "max_indel_1": dict(max_indel_length=1),
    "no_gvcf": dict(gvcf=False),
}
_made = {}


def mirror_case(name):
    if name not in _made:
        _made[name] = syn.make_read_set(**MIRROR_CASES[name])
    return _made[name]


@pytest.mark.parametrize("cfg", sorted(MIRROR_CONFIGS))
@pytest.mark.parametrize("case", sorted(MIRROR_CASES))
def test_host_form_equals_the_mirror(case, cfg):
    rs, c = mirror_case(case), MIRROR_CONFIGS[cfg]
    counts, major, lines, (n_ref, n_total) = host(rs, **c)
    want = pm.pileup(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], **c)
    assert np.array_equal(major, want["major"]) and np.array_equal(counts, want["counts"])
    assert lines == want["lines"]
    assert np.array_equal(n_ref, want["n_ref"]) and np.array_equal(n_total, want["n_total"])
    assert len(major) > 100 and (cfg == "min_depth" or len(lines) > 0)


def test_the_odd_case_holds_what_it_is_for():
    rs = mirror_case("odd")
    ops = rs["cigar"] & 15
    pairs = set(zip(ops[:-1].tolist(), ops[1:].tolist()))
    assert (2, 1) in pairs and (1, 2) in pairs and (6, 1) in pairs and 3 in ops and 7 in ops and 8 in ops
    codes = np.concatenate([rs["seq"] >> 4, rs["seq"] & 15])
    assert (codes == 15).any() and (codes == 3).any()
    want = pm.pileup(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"])
    assert len(want["major"]) < rs["end"] - rs["start"], "a coverage gap"


def test_a_region_inside_the_reads_and_one_beside_them():
    rs = mirror_case("plain")
    for start, end in ((rs["start"] + 50, rs["start"] + 120), (rs["start"] - 700, rs["start"] - 600)):
        counts, major, lines, (n_ref, _) = host(rs, start, end)
        want = pm.pileup(rs, start, end, rs["ref_bytes"], rs["ref_first"])
        assert np.array_equal(counts, want["counts"]) and np.array_equal(major, want["major"]) and lines == want["lines"]
        assert len(n_ref) == end - start


# ---- the read sets the device tests take to the kernels' capacity edges (tests/test_pileup_reads_gpu.py): the host form against the mirror on
# each of them, and what each set is built to hold
CFG = dict(min_snp_af=0.08, min_indel_af=0.15)


def test_the_long_cigars_case_holds_what_it_is_for():
    rs = mirror_case("long_cigars")
    n_ops = np.diff(rs["cigar_first"])
    assert n_ops.max() > 128 and (n_ops > 64).sum() > 10, "reads whose op table needs the carry between 64-op steps, more than once"
    kept = ((rs["flag"] & 0xF04) == 0) & (rs["mapq"] >= 5)
    assert (n_ops[kept] > 128).any() and (rs["pos"][kept & (n_ops > 128)] < rs["end"]).any()


def test_a_region_of_more_tiles_than_one_scan_step():
    rs, tile = big_region()
    start, end, n = rs["start"], rs["end"], rs["end"] - rs["start"]
    tiles = (n + tile - 1) // tile
    assert tiles > tile and n % tile == 5 and tiles == tile + 3
    step = start + tile * tile  # the first site of the scan's second step
    for cfg in (CFG, {}):
        counts, major, lines, (n_ref, n_total) = host(rs, **cfg)
        cand = np.array([int(x.split("-")[0]) - 1 for x in lines])
        assert len(n_ref) == len(n_total) == n and 1000 < len(major) < 3 * 520
        # columns in all three clusters, across the step and in the last tile; candidates on both sides of the step
        assert (major < start + 520).any() and ((major >= step - 250) & (major < step)).any() and ((major >= step) & (major < step + 270)).any()
        assert (major >= end - 5).any() and major.max() == end - 1 and major.min() == start
        assert (cand < step - 250).sum() > 10 and ((cand >= step - 250) & (cand < step)).any() and (cand >= step).sum() > 10 and (cand >= end - 420).any()
        for a in rs["clusters"]:
            s, e = max(start, a - 20), min(end, a + 540)
            want = pm.pileup(rs, s, e, rs["ref_bytes"], rs["ref_first"], **cfg)
            inside = (major >= s) & (major < e)
            assert len(want["major"]) > 300 and np.array_equal(major[inside], want["major"]) and np.array_equal(counts[inside], want["counts"])
            assert [x for x, p in zip(lines, cand) if s <= p < e] == want["lines"] and len(want["lines"]) > 5
            assert np.array_equal(n_ref[s - start:e - start], want["n_ref"]) and np.array_equal(n_total[s - start:e - start], want["n_total"])
            if cfg:  # the variants are built at allele fractions around one half: every kind is a candidate under the thresholds
                text = "".join(want["lines"])
                assert (" I" in text or "-I" in text) and (" D" in text or "-D" in text) and (" X" in text or "-X" in text)


@pytest.mark.parametrize("n_ops", (32, 33))
def test_event_table_size_on_its_boundary(n_ops):
    rs = distinct_events(n_ops)
    t = pm.event_slots(rs, rs["start"], rs["end"])
    assert t["cap"] == (64 if n_ops == 32 else 128) and len(t["events"]) == n_ops and set(t["events"].values()) == {1}
    assert len(set(t["keys"].values())) == n_ops and len(t["occupied"]) == n_ops
    kept = ((rs["flag"] & 0xF04) == 0) & (rs["mapq"] >= 5)
    ops = rs["cigar"] & 15
    per_read = np.add.reduceat(((ops == 1) | (ops == 2)).astype(np.int64), rs["cigar_first"][:-1])
    assert per_read[kept].sum() == n_ops and per_read[~kept].sum() > 0
    with pr.Context(None) as ctx:
        r = ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], call_ht=True).fetch()
        assert ctx.stats()["events"] == n_ops
    want = pm.pileup(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], call_ht=True)
    assert np.array_equal(r["counts"], want["counts"]) and r["text"].decode().split("\n")[:-1] == want["lines"]


def test_a_probe_of_the_event_table_wraps():
    """32 distinct events in 64 slots, placed so that two probes start at the last slot: one of them goes on at slot 0"""
    rs = distinct_events(32, shift=WRAP_SHIFT)
    t = pm.event_slots(rs, rs["start"], rs["end"])
    assert t["cap"] == 64 and len(set(t["keys"].values())) == 32 and t["wrapped"]
    assert sorted(t["first"].values())[-2:] == [63, 63] and 0 in t["occupied"] and 63 in t["occupied"]
    assert not pm.event_slots(distinct_events(32), 90, 300)["wrapped"]
    counts, major, lines, _ = host(rs, call_ht=True)
    want = pm.pileup(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], call_ht=True)
    assert np.array_equal(counts, want["counts"]) and lines == want["lines"]


def test_one_slot_counted_a_thousand_times():
    rs = insertion_column(n_reads=3000)
    t = pm.event_slots(rs, rs["start"], rs["end"])
    assert sum(t["events"].values()) == 3000 and len(t["events"]) <= 80 and max(t["events"].values()) > 1000 // 40
    counts, major, lines, _ = host(rs, call_ht=True, **CFG)
    col = int(np.flatnonzero(major == 149)[0])
    assert counts[col, 4] + counts[col, 13] == 3000 and lines[0].startswith("150-3000-")
    want = pm.pileup(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], call_ht=True, **CFG)
    assert np.array_equal(counts, want["counts"]) and lines == want["lines"]


def test_more_candidates_than_a_ring_lane_takes():
    rs = syn.make_read_set(**MANY_CANDIDATES)
    counts, major, lines, _ = host(rs, call_ht=True)
    assert len(lines) == len(major) > 1024, "every column a candidate, above lane_max_batch of a pileup handle"
    want = pm.pileup(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], call_ht=True)
    assert np.array_equal(counts, want["counts"]) and lines == want["lines"]


# ---- hand-worked columns.  Every case: the reference is written out, the reads lie at position `pos` with the CIGAR given
def hand(ref, reads, start, end, **cfg):
    rs = syn.pack_reads([(pos, flag, 60, cigar, seq) for pos, flag, cigar, seq in reads])
    counts, major, lines, pair = pr.pileup_counts(rs, start, end, ref.encode(), 0, path="host", **cfg)
    return counts, major, [parse_line(x) for x in lines], lines, pair


def test_equal_majority_tie_in_both_orders():
    ref = "GGGGACGGGG" + "G" * 60
    alt = "GGGGCAGGGG"  # column 4: reference A against C, column 5: reference C against A
    counts, major, cand, lines, _ = hand(ref, [(0, 0, "10M", ref[:10]), (0, 16, "10M", ref[:10]), (0, 0, "10M", alt), (0, 16, "10M", alt)], 0, 10,
                                         call_ht=True, min_snp_af=0.9, min_indel_af=0.9)
    # both columns: ref_count 2 == alt_count 2, ratio 0.5 below the threshold.  'A' - 'C' < 0 passes, 'C' - 'A' > 0 does not
    assert lines == ["5-4-A-XC 2 RA 2 "]
    assert counts[4].tolist() == [-2, 1, 0, 0, 0, 0, 0, 0, 0, -2, 1, 0, 0, 0, 0, 0, 0, 0]
    assert counts[5].tolist() == [1, -2, 0, 0, 0, 0, 0, 0, 0, 1, -2, 0, 0, 0, 0, 0, 0, 0]


def test_flanking_count_15_against_16():
    ref = "A" * 160
    _, major, cand, _, _ = hand(ref, [(10, 0, "30M", "C" * 30)], 5, 60)  # every column: reference count 0 below alt count 1
    assert major.tolist() == list(range(10, 40))
    # column 25 has the 15 columns 10 .. 24 to its left, column 26 has 16
    assert [c[0] - 1 for c in cand] == list(range(26, 40))
    _, _, cand, _, _ = hand(ref, [(10, 0, "30M", "C" * 30)], 5, 60, call_ht=True)
    assert [c[0] - 1 for c in cand] == list(range(10, 40))
    # a gap resets the count: columns 10 .. 39 and 41 .. 79; behind the gap the first candidate is 41 + 16
    _, _, cand, _, _ = hand(ref, [(10, 0, "30M", "C" * 30), (41, 0, "39M", "C" * 39)], 5, 100)
    assert [c[0] - 1 for c in cand] == list(range(26, 40)) + list(range(57, 80))


def test_a_column_at_position_0():
    ref = "A" * 160
    _, major, cand, _, _ = hand(ref, [(0, 0, "30M", "C" * 30)], 0, 60)
    assert major[0] == 0
    # the column behind position 0 starts at 0 again (pre_pos == 0): column p has p - 1, so 17 is the first with 16
    assert [c[0] - 1 for c in cand] == list(range(17, 30))
    _, _, cand, _, _ = hand(ref, [(0, 0, "30M", "C" * 30)], 1, 60)  # the same reads, region from 1: column 1 is the first, 17 has 16
    assert [c[0] - 1 for c in cand] == list(range(17, 30))
    _, _, cand, _, _ = hand(ref, [(1, 0, "30M", "C" * 30)], 0, 60)  # no column at 0
    assert [c[0] - 1 for c in cand] == list(range(17, 31))


def test_float32_ratio_exactly_on_the_threshold():
    ref = "G" * 4 + "A" + "G" * 70
    reads = [(0, 0, "10M", ref[:10])] * 9 + [(0, 0, "10M", "GGGGCGGGGG")]
    # alt 1 of depth 10: 1 / 10 in float32 equals float32(0.1), the threshold as the reference holds it; in double it would lie below
    assert np.float32(1) / np.float32(10) == np.float32(0.1) and 1 / 10 < float(np.float32(0.1))
    _, _, _, lines, _ = hand(ref, reads, 0, 10, call_ht=True, min_snp_af=0.1, min_indel_af=0.9)
    assert lines == ["5-10-A-XC 1 RA 9 "]
    above = float(np.nextafter(np.float32(0.1), np.float32(1)))
    _, _, _, lines, _ = hand(ref, reads, 0, 10, call_ht=True, min_snp_af=above, min_indel_af=0.9)
    assert lines == []


def test_a_deletion_longer_than_max_indel_length():
    ref = "ACGTACGTACGTACGTACGT" + "G" * 60
    reads = [(0, 0, "20M", ref[:20])] * 3 + [(0, 16, "6M4D10M", ref[:6] + ref[10:20])]
    counts, _, _, lines, (n_ref, n_total) = hand(ref, reads, 0, 20, call_ht=True, min_snp_af=0.9, min_indel_af=0.2, max_indel_length=3)
    # column 5 (reference C): 4 reads, one starts a deletion of 4 > 3: no D entry, but it is taken off ref_depth: 4 - 1 = 3
    assert lines == ["6-4-C-RC 3 "]
    assert counts[5, 15] == 1 and counts[5, 16] == 1 and counts[6:10, 17].tolist() == [1] * 4
    assert (n_ref[5], n_total[5]) == (4, 5)
    _, _, _, lines, _ = hand(ref, reads, 0, 20, call_ht=True, min_snp_af=0.9, min_indel_af=0.2, max_indel_length=4)
    assert lines == ["6-4-C-DGTAC 1 RC 3 "]


def test_insertions_merge_strands_and_sort_by_length_then_bytes():
    ref = "ACGTACGTAC" + "G" * 60
    def ins(s):
        return ref[:5] + s + ref[5:10]
    reads = [(0, 0, "5M2I5M", ins("TT")), (0, 16, "5M2I5M", ins("TT")), (0, 0, "5M2I5M", ins("CA")), (0, 0, "5M1I5M", ins("G")),
             (0, 0, "5M1I1I5M", ins("AT")), (0, 0, "5M1P1I5M", ins("G")), (0, 0, "3S7M", "TTT" + ref[:7]), (2, 0, "2I8M", "GG" + ref[2:10])]
    counts, _, cand, lines, _ = hand(ref, reads, 0, 10, call_ht=True, min_snp_af=0.9, min_indel_af=0.5)
    # column 4 (reference A): 7 reads span it (the soft-clipped one too, the one that starts at 2 too; its leading insertion is dropped)
    assert lines == ["5-8-A-IAG 2 IAAT 1 IACA 1 IATT 2 RA 2 "]
    assert counts[4, 4] == 5 and counts[4, 5] == 2 and counts[4, 13] == 1 and counts[4, 14] == 1


# ---- errors: refused before anything is computed
def test_errors():
    rs = syn.pack_reads([(10, 0, 60, "10M", "ACGTACGTAC"), (12, 0, 60, "4M2I4M", "ACGTACGTAC")])
    ref = np.frombuffer(b"A" * 200, np.uint8)
    ok = pr.pileup_counts(rs, 5, 40, ref, 0, path="host")
    assert len(ok[1]) == 10
    with pytest.raises(_lib.C3Error, match="do not cover"):
        pr.pileup_counts(rs, 5, 40, ref[:60], 0, path="host", max_indel_length=50)  # covers the region, not the 50 behind it
    with pytest.raises(_lib.C3Error, match="do not cover"):
        pr.pileup_counts(rs, 5, 40, ref, 6, path="host")
    with pytest.raises(_lib.C3Error, match="end <= start"):
        pr.pileup_counts(rs, 40, 40, ref, 0, path="host")
    bad = dict(rs, cigar_first=np.array([0, 3, 2], np.int64))
    with pytest.raises(_lib.C3Error, match="cigar_first is not non-decreasing"):
        pr.pileup_counts(bad, 5, 40, ref, 0, path="host")
    bad = dict(rs, cigar=np.array([10 << 4, 4 << 4, 3 << 4 | 1, 4 << 4], np.uint32))  # 4M3I4M over 10 bases
    with pytest.raises(_lib.C3Error, match="consumes 11 bases, its seq holds 10"):
        pr.pileup_counts(bad, 5, 40, ref, 0, path="host")
    bad = dict(rs, cigar=np.array([10 << 4, 4 << 4, 2 << 4 | 9, 4 << 4], np.uint32))
    with pytest.raises(_lib.C3Error, match="op code 9"):
        pr.pileup_counts(bad, 5, 40, ref, 0, path="host")
    with pytest.raises(TypeError, match="unknown pileup option"):
        pr.pileup_counts(rs, 5, 40, ref, 0, path="host", min_af=0.1)
    with pr.Context(None) as ctx:
        with pytest.raises(_lib.C3Error, match="without a device"):
            ctx.run(rs, 5, 40, ref, 0, path="device")


def test_an_empty_read_set_gives_no_columns():
    rs = syn.pack_reads([])
    counts, major, lines, (n_ref, n_total) = pr.pileup_counts(rs, 100, 160, b"A" * 400, 0, path="host")
    assert counts.shape == (0, 18) and len(major) == 0 and lines == []
    assert len(n_ref) == 60 and not n_ref.any() and not n_total.any()


def test_all_reads_filtered_and_stats():
    rs = mirror_case("plain")
    dropped = dict(rs, flag=rs["flag"] | 0x400)
    with pr.Context(None) as ctx:
        r = ctx.run(dropped, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"]).fetch()
        assert r["counts"].shape == (0, 18) and r["text"] == b""
        assert ctx.stats()["reads_kept"] == 0 and ctx.stats()["reads_dropped"] == len(rs["pos"])
        ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"])
        s = ctx.stats()
        kept = int((((rs["flag"] & 0xF04) == 0) & (rs["mapq"] >= 5)).sum())
        assert s["reads_kept"] == kept and s["reads_kept"] + s["reads_dropped"] == len(rs["pos"]) and s["events"] > 0 and s["on_host"] and not s["fell_back"]


def test_command_line(tmp_path, capsys):
    rs = mirror_case("plain")
    np.savez(tmp_path / "reads.npz", **{name: rs[name] for name in FIELDS})
    contig = b"N" * rs["ref_first"] + bytes(rs["ref_bytes"])
    with open(tmp_path / "ref.fa", "wb") as fh:
        fh.write(b">other\nACGT\n>ctg extra words\n" + b"\n".join(contig[i:i + 60] for i in range(0, len(contig), 60)) + b"\n")
    rc = pr.main(["--reads", str(tmp_path / "reads.npz"), "--ref_fn", str(tmp_path / "ref.fa"), "--ctgName", "ctg", "--ctgStart", str(rs["start"] + 1),
                  "--ctgEnd", str(rs["end"]), "--path", "host", "--output_fn", str(tmp_path / "out.npz")])
    assert rc == 0
    want = host(rs, min_snp_af=0.08, min_indel_af=0.15)
    assert capsys.readouterr().out == "".join(x + "\n" for x in want[2]) and len(want[2]) > 0
    with np.load(tmp_path / "out.npz") as z:
        assert np.array_equal(z["counts"], want[0]) and np.array_equal(z["major"], want[1]) and np.array_equal(z["n_total"], want[3][1])
