"""Full alignment from reads, the host form (csrc/c3_fa_rule.h, c3_fa_reads_host; no device): against the golden windows of the reference's
own generate_tensor (tests/golden/fa_reads.npz, every cell, nothing masked), against a numpy mirror written from the rule's description
(tests/fa_mirror.py), hand-worked windows, every refusal, and the same code as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/host/fa_reads_host_check.cpp).  The device form is held to the host form in tests/test_fa_reads_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from clair3_amd import _lib, fa_reads as fa, synthetic as syn
from tests.fa_cases import (FA_DROP_BITS, FILL_LEVELS, INDEL_CENTRE, LDS, MANY, RAGGED, STEP, alt_counts, by_hand, check_fill, check_indel_rows,
                            fill_centres, generated, golden_sets, indel_column, many_candidates, read_range, table_fill, window_numbers)
from tests.fa_mirror import fa_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "ACGT" * 100


@pytest.fixture(scope="module")
def ctx():
    with fa.Context(None) as c:
        yield c


def run(ctx, rs, ex, centres, **cfg):
    return ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path="host", **cfg).fetch()


def lines_of(r):
    return r["text"].decode("ascii").split("\n")[:-1]


def test_golden_windows(ctx):
    n_rows = 0
    for k, rs, ex, centres, want in golden_sets():
        r = run(ctx, rs, ex, centres, min_mq=rs["min_mq"])
        assert np.array_equal(r["counts"], want["counts"]), f"set {k}: counts"
        assert r["rows"].shape == want["rows"].shape and np.array_equal(r["rows"], want["rows"]), f"set {k}: cells"
        lines = lines_of(r)
        assert len(lines) == len(centres)
        for c, line, alt in zip(centres, lines, want["alt"]):
            depth, mine = alt_counts(line)
            assert line.startswith(f"{c + 1}-")
            if not str(alt):  # (generate_tensor returns nothing for a window without reads)
                assert depth == 0 and not mine
                continue
            d, _, rest = str(alt).partition("-")
            items = rest.split(" ")
            assert depth == int(d) and mine == {a: int(b) for a, b in zip(items[0::2], items[1::2]) if a}, f"set {k} at {c}"
        n_rows += len(want["rows"])
        assert ctx.stats()["on_host"] and not ctx.stats()["fell_back"] and ctx.stats()["deep_windows"] == 0
    assert n_rows > 9000


MIRRORED = {
    "plain": (dict(n_sites=200, depth=30, read_len=(60, 200), seed=51), dict()),
    "every_op": (dict(n_sites=200, depth=25, read_len=(60, 200), seed=52, d_then_i=0.004, i_then_d=0.004, pad=0.2, eqx=True, ref_other=0.03, non_acgt=0.02,
                      ins=0.02, dele=0.01), dict(max_indel_length=2)),
    "over_deep": (dict(n_sites=60, depth=70, read_len=(60, 200), seed=53), dict(matrix_depth=55, seed=9)),
}


@pytest.mark.parametrize("name", sorted(MIRRORED))
def test_numpy_mirror(ctx, name):
    spec, cfg = MIRRORED[name]
    rs, ex = generated(duplicate_names=0.05, **spec)
    centres = np.arange(rs["start"], rs["end"], 2)
    r = run(ctx, rs, ex, centres, **cfg)
    rows, counts, depths, lines = fa_mirror(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **cfg)
    assert np.array_equal(r["counts"], counts) and np.array_equal(r["depths"], depths)
    assert r["rows"].shape == rows.shape and np.array_equal(r["rows"], rows)
    assert lines_of(r) == lines
    if name == "over_deep":
        assert ctx.stats()["deep_windows"] > 10 and counts.max() == 55
    # without the name keys no read is dropped for its name
    ex2 = dict(ex, name_key=None)
    r2 = ctx.run(rs, fa.ReadExtras.from_dict(ex, names=False), centres, rs["ref_bytes"], rs["ref_first"], path="host", **cfg).fetch()
    m2 = fa_mirror(rs, ex2, centres, rs["ref_bytes"], rs["ref_first"], **cfg)
    assert np.array_equal(r2["rows"], m2[0]) and r2["counts"].sum() >= r["counts"].sum()


def test_a_candidate_with_no_read(ctx):
    rs, ex = by_hand([(100, 0, 60, "20M", REF[100:120])])
    r = run(ctx, rs, ex, [50, 110, 300])
    assert r["counts"].tolist() == [0, 1, 0] and r["depths"].tolist() == [0, 1, 0] and r["rows"].shape == (1, 33, 8)
    assert lines_of(r) == ["51-0-G-", "111-1-G-RG 1 ", "301-0-A-"]
    assert not syn.pad_fa_rows(r["rows"], r["counts"])[0].any() and not syn.pad_fa_rows(r["rows"], r["counts"])[2].any()


def test_one_read_by_hand(ctx):
    """reverse strand, mapq 30, haplotype 2: 10M 2I 10M 3D 10M at 100; centre 109 is the insertion's anchor.  Reference ACGT...: position p holds
    "ACGT"[p % 4]; the read repeats the reference but for a T at 105 (reference C)"""
    seq = REF[100:105] + "T" + REF[106:110] + "GC" + REF[110:120] + REF[123:133]
    quals = list(range(10)) + [40, 50] + [20] * 20
    rs, ex = by_hand([(100, 16, 30, "10M2I10M3D10M", seq)], quals=[quals], haps=[2])
    r = run(ctx, rs, ex, [109])
    assert r["counts"].tolist() == [1] and r["depths"].tolist() == [1]
    w = r["rows"][0]
    # columns 0 .. 6 lie in front of the read (93 .. 99); 7 .. 32 are 100 .. 125
    assert not w[:7].any()
    base_v = {"A": 100, "C": 25, "G": 75, "T": 50}
    for col in range(7, 33):
        p = 93 + col
        deleted = 120 <= p < 123
        if deleted:
            assert not w[col, [0, 1, 2, 3, 4, 5, 7]].any()
            continue
        assert w[col, 0] == base_v[REF[p]] and w[col, 2] == 50 and w[col, 3] == 50 and w[col, 7] == 90
        assert w[col, 5] == 100  # the insertion is on the one read there is: 1 / 1
    assert w[12, 1] == 50 and w[16, 1] == -50 and w[26, 1] == -100 and not w[[7, 8, 13, 17, 25], 1].any()
    assert w[7:17, 4].tolist() == [int(100 * q / 40) for q in range(10)] and w[17, 4] == 50
    assert w[16, 6] == 75 and w[17, 6] == 25 and not w[18:, 6].any() and not w[:16, 6].any()
    assert lines_of(r) == ["110-1-C-ICGC 1 "]  # (ref_count 1 - 1 insertion: no R entry)
    # the deletion's anchor as the centre: D and the reference bytes behind it
    assert lines_of(run(ctx, rs, ex, [119]))[0] == "120-1-T-DACG 1 "
    assert lines_of(run(ctx, rs, ex, [105]))[0] == "106-1-C-XT 1 "


def test_float32_allele_fraction(ctx):
    """29 of 50: 100 * (29 / 50) is 57 in double (57.99999...) and 58 in float32 (the quotient rounds up to 0.58000004); the rule is the C
    function's float32.  Found by enumeration over depths below 130: (29, 50), (29, 100), (53, 100), (57, 100), (58, 100), (59, 100)"""
    assert int(100 * (29 / 50.0)) == 57 and int(np.float32(100) * (np.float32(29) / np.float32(50))) == 58
    alt = REF[100:110] + "T" + REF[111:120]  # position 110 holds G
    rs, ex = by_hand([(100, 0, 60, "20M", alt if i < 29 else REF[100:120]) for i in range(50)])
    r = run(ctx, rs, ex, [110])
    assert r["counts"].tolist() == [50] and r["depths"].tolist() == [50]
    assert (r["rows"][:29, 6:26, 5] == 58).all() and not r["rows"][:29, :6, 5].any() and not r["rows"][:29, 26:, 5].any() and not r["rows"][29:, :, 5].any()
    assert lines_of(r) == ["111-50-G-XT 29 RG 21 "]


def test_over_deep_selection_and_order(ctx):
    """120 reads over one candidate, matrix_depth 89 and 55: the kept reads are those of smallest (key, index) by synthetic's hash, rows by
    (haplotype, index).  The reads are told apart by their base qualities"""
    n = 120
    haps = [(7 * i) % 3 for i in range(n)]
    rs, ex = by_hand([(100, 0, 5 + i % 50, "20M", REF[100:120]) for i in range(n)], quals=[i % 40 for i in range(n)], haps=haps)
    for depth, seed in ((89, 1), (55, 2), (55, 3)):
        r = run(ctx, rs, ex, [110], matrix_depth=depth, seed=seed)
        keep = np.flatnonzero(syn.subsample_rank(syn.fa_keys(seed, 110, np.arange(n)), depth))
        order = sorted(keep, key=lambda i: (haps[i], i))
        assert r["counts"].tolist() == [depth] and r["depths"].tolist() == [n]
        assert r["rows"][:, 16, 4].tolist() == [int(100 * (i % 40) / 40) for i in order]
        assert r["rows"][:, 16, 7].tolist() == [(60, 30, 90)[haps[i]] for i in order]
        assert ctx.stats()["deep_windows"] == 1
    assert not np.array_equal(run(ctx, rs, ex, [110], matrix_depth=55, seed=2)["rows"], run(ctx, rs, ex, [110], matrix_depth=55, seed=3)["rows"])
    # below the depth: haplotype order alone
    r = run(ctx, rs, ex, [110], matrix_depth=128)
    assert r["rows"][:, 16, 7].tolist() == [(60, 30, 90)[h] for h in sorted(haps)] and ctx.stats()["deep_windows"] == 0


def test_duplicate_names_and_filters(ctx):
    reads = [(100, 0, 60, "20M", REF[100:120]), (101, 0, 60, "20M", REF[101:121]), (102, 0x100, 60, "20M", REF[102:122]),
             (103, 0, 3, "20M", REF[103:123]), (104, 16, 60, "20M", REF[104:124]), (105, 0x8, 60, "20M", REF[105:125])]
    rs, ex = by_hand(reads, names=[7, 7, 9, 7, 9, 11], quals=[1, 2, 3, 4, 5, 6])
    r = run(ctx, rs, ex, [110])
    # read 1 repeats read 0's name; read 2 (secondary) and read 3 (mapq) are dropped before their names count, so read 4 is the first "9"; read 5: mate unmapped
    assert r["counts"].tolist() == [2] and r["rows"][:, 16, 4].tolist() == [2, 12]
    s = ctx.stats()
    assert s["reads_kept"] == 2 and s["reads_dropped"] == 4
    r = ctx.run(rs, fa.ReadExtras.from_dict(ex, names=False), [110], rs["ref_bytes"], 0, path="host").fetch()
    assert r["counts"].tolist() == [3]


def test_max_indel_length_boundary(ctx):
    ins3 = REF[100:110] + "GGG" + REF[110:120]
    reads = [(100, 0, 60, "10M3I10M", ins3), (100, 0, 60, "10M3I10M", ins3), (100, 0, 60, "10M4D6M", REF[100:110] + REF[114:120]),
             (100, 0, 60, "20M", REF[100:120])]
    rs, ex = by_hand(reads)
    assert lines_of(run(ctx, rs, ex, [109], max_indel_length=4))[0] == "110-4-C-DGTAC 1 ICGGG 2 RC 1 "
    assert lines_of(run(ctx, rs, ex, [109], max_indel_length=3))[0] == "110-4-C-ICGGG 2 RC 1 "
    assert lines_of(run(ctx, rs, ex, [109], max_indel_length=2))[0] == "110-4-C-RC 1 "  # (R still has every indel taken off)


def test_refusals(ctx):
    rs, ex = by_hand([(100, 0, 60, "30M", REF[100:130]), (104, 16, 60, "10M5N15M", REF[104:114] + REF[119:134])])
    with pytest.raises(fa.RefSkipError, match="N op"):
        run(ctx, rs, ex, [110])
    assert run(ctx, rs, ex, [300])["counts"].tolist() == [0]  # (the N op lies in no window)
    good, gex = by_hand([(100, 0, 60, "30M", REF[100:130]), (104, 16, 60, "25M", REF[104:129])])
    assert run(ctx, good, gex, [110, 120])["counts"].tolist() == [2, 2]
    for what, centres, match in (("below 16", [15], "below 16"), ("descending", [120, 110], "ascending"), ("twice", [110, 110], "ascending")):
        with pytest.raises(_lib.C3Error, match=match):
            run(ctx, good, gex, centres)
    bad = dict(good, pos=good["pos"][::-1].copy())
    with pytest.raises(_lib.C3Error, match="coordinate order"):
        run(ctx, bad, gex, [110])
    short = dict(good, ref_bytes=good["ref_bytes"][:170])
    with pytest.raises(_lib.C3Error, match="do not cover"):
        run(ctx, short, gex, [110], max_indel_length=50)
    assert run(ctx, short, gex, [110], max_indel_length=10)["counts"].tolist() == [2]
    with pytest.raises(_lib.C3Error, match="haplotype"):
        run(ctx, good, dict(gex, haplotype=np.array([0, 3], np.uint8)), [110])
    with pytest.raises(_lib.C3Error, match="matrix_depth"):
        run(ctx, good, gex, [110], matrix_depth=129)
    with pytest.raises(_lib.C3Error, match="without a device"):
        ctx.run(good, gex, [110], good["ref_bytes"], 0, path="device")
    # a refused call leaves no stale result behind
    assert ctx.sizes()[:2] == (0, 0)


# ---- the read sets the device tests take to the kernels' capacity edges (tests/test_fa_reads_gpu.py): here the host form against the mirror
# on each of them, and what each set is built to hold
def assert_mirror(r, rs, ex, centres, **cfg):
    rows, counts, depths, lines = fa_mirror(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **cfg)
    assert np.array_equal(r["counts"], counts) and np.array_equal(r["depths"], depths)
    assert r["rows"].shape == rows.shape and np.array_equal(r["rows"], rows)
    assert lines_of(r) == lines


@pytest.mark.parametrize("n_over", FILL_LEVELS + (LDS + 1, 88, 89, 90, 300))
def test_table_fill_levels(ctx, n_over):
    rs, ex, info = table_fill((n_over,))
    c = info["centres"][0]
    lo, hi = read_range(info, c)
    over, at, n_alt = window_numbers(info, c)
    assert over == n_over and 0 < n_alt < at < over and (lo, hi) == (0, len(rs["pos"]))
    assert hi - lo >= 5 * STEP or n_over < LDS - 1
    # no step of the compaction has a full ballot; in the range sit a read of each dropped flag bit, of a low mapq, and kept short reads in
    # front of the window, some of them kept in the rule's own sense: inside the window of c - 56
    taken = info["kept"] & (info["end"] > c - 16)
    assert all(not taken[b:b + STEP].all() for b in range(lo, hi, STEP))
    if n_over >= STEP - 1:
        assert all((rs["flag"] & bit).any() for bit in FA_DROP_BITS) and (rs["mapq"] < 5).any()
        assert (info["kept"] & (info["end"] <= c - 16) & (info["end"] > c - 56 - 16)).any()
    assert set(ex["haplotype"][taken].tolist()) == {0, 1, 2} and set((rs["flag"][taken] & 16).tolist()) == {0, 16}
    centres = fill_centres(info)
    for depth in (89, 128, 1) if n_over == 300 else (89, 128):
        r = run(ctx, rs, ex, centres, matrix_depth=depth, seed=depth)
        check_fill(r, ctx.stats(), info, depth)
        assert r["counts"][1] == min(n_over, depth) and r["depths"][1] == at
        assert_mirror(r, rs, ex, centres, matrix_depth=depth, seed=depth)
    if n_over in (88, 89, 90):  # the boundary of the selection: the window of c alone
        r = run(ctx, rs, ex, [c], matrix_depth=89)
        assert r["counts"].tolist() == [min(n_over, 89)] and ctx.stats()["deep_windows"] == (1 if n_over == 90 else 0)


def test_two_table_fill_levels_in_one_call(ctx):
    rs, ex, info = table_fill((LDS, 300))
    centres = fill_centres(info)
    assert [window_numbers(info, c)[0] for c in info["centres"]] == [LDS, 300]
    spans = [read_range(info, c) for c in info["centres"]]
    assert spans[0][1] == spans[1][0] and (spans[0][1] - spans[0][0]) // STEP > (spans[1][1] - spans[1][0]) // STEP
    r = run(ctx, rs, ex, centres, matrix_depth=89)
    check_fill(r, ctx.stats(), info, 89)
    assert_mirror(r, rs, ex, centres, matrix_depth=89)


INDEL_CENTRES = [INDEL_CENTRE - 16, INDEL_CENTRE, INDEL_CENTRE + 16, INDEL_CENTRE + 17]


def test_indel_column_across_the_256_boundary(ctx):
    rs, ex, expected, kinds = indel_column(extras=False)
    assert len(kinds) == 700 and lines_of(run(ctx, rs, ex, INDEL_CENTRES))[1] == "131-700-G-DT 100 DTA 100 IGG 100 IGGG 100 IGGT 100 RG 200 "
    rs, ex, expected, kinds = indel_column()
    # what the set is for: every kind of indel on both sides of read 256, the doubled ops only behind it, one string once and behind 512
    for kind in (("I", "G"), ("I", "GG"), ("I", "GT"), ("D", 1), ("D", 2)):
        at = [i for i, k in enumerate(kinds) if k == kind]
        assert min(at) < STEP and sum(i >= STEP for i in at) > 50 and sum(i >= 2 * STEP for i in at) > 20
    assert min(i for i, k in enumerate(kinds) if k and k[0] in ("II", "ID")) > STEP
    once = [i for i, k in enumerate(kinds) if k == ("I", "TTT")]
    assert len(once) == 1 and once[0] > 2 * STEP and expected[1]["IGTTT"] == 1
    assert (rs["pos"] <= INDEL_CENTRE).all() and (np.diff(rs["pos"]) >= 0).all() and len(set(rs["pos"].tolist())) == 25
    for depth in (89, 128, 1):
        r = run(ctx, rs, ex, INDEL_CENTRES, matrix_depth=depth, seed=3)
        assert alt_counts(lines_of(r)[1]) == expected and r["depths"][1] == len(kinds) == 708
        assert_mirror(r, rs, ex, INDEL_CENTRES, matrix_depth=depth, seed=3)
        n_ins, n_del = check_indel_rows(r, expected)
        assert depth == 1 or (n_ins > 20 and n_del > 10)
    # the column of the indels is the last column of the left window, the first of the right one, and outside the one behind it
    r = run(ctx, rs, ex, INDEL_CENTRES, matrix_depth=128, seed=3)
    first = np.concatenate([[0], np.cumsum(r["counts"])])
    assert (r["rows"][first[0]:first[1], 32, 1] == -50).any() and (r["rows"][first[2]:first[3], 0, 1] == -100).any()
    assert not (r["rows"][first[3]:first[4], :, 1] == -50).any()


def test_more_candidates_than_two_scan_steps(ctx):
    tile = _lib.lib().c3_pileup_tile_sites()  # (full alignment scans its row counts with pileup's kernel: a step holds this many candidates)
    rs, ex, centres = many_candidates(*MANY[0], **MANY[1])
    cfg = MANY[2]
    n_over = run(ctx, rs, ex, centres, **dict(cfg, matrix_depth=128))["counts"]  # (no window of the set holds more than 128 reads)
    r = run(ctx, rs, ex, centres, **cfg)
    assert len(centres) > 2 * tile and len(r["counts"]) == len(centres) and (np.diff(centres) == 1).all() and n_over.max() < 128
    assert (r["counts"][-10:] == 0).all() and 10 < (r["counts"] == 0).sum() < 100 and r["counts"][:tile + 1].min() > 0
    # over-deep windows in each of the scan's three steps
    assert ctx.stats()["deep_windows"] == (n_over > 24).sum() and all((n_over[a:a + tile] > 24).sum() > 50 for a in (0, tile, 2 * tile))
    assert np.array_equal(r["counts"], np.minimum(n_over, 24))
    # the mirror on a hundred centres across the step (it is quadratic): the windows of a candidate do not depend on the other candidates
    lo, hi = tile - 50, tile + 50
    first = np.concatenate([[0], np.cumsum(r["counts"])])
    part = {"rows": r["rows"][first[lo]:first[hi]], "counts": r["counts"][lo:hi], "depths": r["depths"][lo:hi],
            "text": "".join(x + "\n" for x in lines_of(r)[lo:hi]).encode()}
    assert_mirror(part, rs, ex, centres[lo:hi], **cfg)
    # the first candidates alone: the same rows
    for n in (tile, tile + 1):
        r2 = run(ctx, rs, ex, centres[:n], **cfg)
        assert np.array_equal(r2["rows"], r["rows"][:first[n]]) and np.array_equal(r2["counts"], r["counts"][:n])


def test_the_ragged_batch_holds_what_it_is_for(ctx):
    tile = _lib.lib().c3_pileup_tile_sites()
    rs, ex, centres = many_candidates(*RAGGED[0], **RAGGED[1])
    r = run(ctx, rs, ex, centres, **RAGGED[2])
    # above a full-alignment lane's 512 windows and above one scan step; empty windows, over-deep ones, no window over the table
    assert len(centres) >= 1100 and len(centres) > tile and (r["counts"] == 0).sum() > 10 and ctx.stats()["deep_windows"] > 100
    assert r["counts"].max() == 55 and (r["counts"] < 55).sum() > 100 and r["depths"].max() < LDS // 4
    lo, hi = tile - 20, tile + 20
    first = np.concatenate([[0], np.cumsum(r["counts"])])
    part = {"rows": r["rows"][first[lo]:first[hi]], "counts": r["counts"][lo:hi], "depths": r["depths"][lo:hi],
            "text": "".join(x + "\n" for x in lines_of(r)[lo:hi]).encode()}
    assert_mirror(part, rs, ex, centres[lo:hi], **RAGGED[2])


def _case_file(path, rs, ex, centres, cfg):
    head = np.array([len(rs["pos"]), len(rs["cigar"]), len(rs["seq"]), len(ex["qual"]), len(centres), rs["ref_first"], len(rs["ref_bytes"]),
                     cfg["min_mq"], cfg["max_indel_length"], cfg["matrix_depth"], cfg["seed"], 1], np.int64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for a in (rs["pos"], rs["flag"], rs["mapq"], rs["cigar_first"], rs["cigar"], rs["seq_first"], rs["seq"], ex["qual_first"], ex["qual"],
                  ex["haplotype"], ex["name_key"], np.asarray(centres, np.int64), rs["ref_bytes"]):
            f.write(np.ascontiguousarray(a).tobytes())


def test_host_form_under_sanitizers(ctx, tmp_path):
    """the rule header as a stand-alone program (its own main, no Python, no library) under -fsanitize=address,undefined: the refusals, and two
    read sets whose output must be the library's byte for byte"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fa_reads_host_check")
    # (the sanitizers' runtimes are linked statically: the program then runs whatever else the environment loads in front of it)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                          [os.path.join(ROOT, "tests", "host", "fa_reads_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, "--errors"], env=env, capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout and not p.stderr, p.stdout + p.stderr
    sets = [(rs, ex, centres, dict(min_mq=5, max_indel_length=50, matrix_depth=89, seed=0)) for k, rs, ex, centres, _ in golden_sets() if k == 0]
    rs, ex = generated(n_sites=80, depth=60, read_len=(60, 200), seed=54, d_then_i=0.004, i_then_d=0.004, pad=0.2, eqx=True, non_acgt=0.02, ref_other=0.03)
    sets.append((rs, ex, np.arange(rs["start"], rs["end"], 2), dict(min_mq=5, max_indel_length=3, matrix_depth=55, seed=4)))
    for i, (rs, ex, centres, cfg) in enumerate(sets):
        case, out = str(tmp_path / f"case{i}.bin"), str(tmp_path / f"out{i}.bin")
        _case_file(case, rs, ex, centres, cfg)
        p = subprocess.run([exe, case, out], env=env, capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr
        want = run(ctx, rs, ex, centres, **cfg)
        raw = open(out, "rb").read()
        n_rows, text_bytes = np.frombuffer(raw[:16], np.int64)
        assert n_rows == len(want["rows"]) and n_rows > 1000
        body = raw[16:]
        assert body[:n_rows * 264] == want["rows"].tobytes()
        off = n_rows * 264
        assert body[off:off + 4 * len(centres)] == want["counts"].tobytes() and body[off + 4 * len(centres):off + 8 * len(centres)] == want["depths"].tobytes()
        assert body[off + 8 * len(centres):] == want["text"] and len(want["text"]) == text_bytes
