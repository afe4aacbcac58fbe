"""The dwell channel from move tables, the host form (csrc/c3_dwell_rule.h, c3_fa_reads_dwell_host, c3_fa_dwell_cum_host; no device): the
per-read rule against the signal lengths of the reference's own compute_signal_lengths_from_mv_tag (tests/golden/fa_dwell_tables.npz), the
9-channel windows against a Python mirror written from the rule's description (tests/dwell_mirror.py), channels 0 .. 7 against the
8-channel entries, one hand-worked read per clause, the refusals, and the same code as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/host/dwell_host_check.cpp).  The device form is held to the host form in tests/test_dwell_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from clair3_amd import _lib, fa_reads as fa, synthetic as syn
from tests.dwell_cases import REF, SETS, generated, golden_tables, moves_by_hand, op_kinds, table_of
from tests.dwell_mirror import dwell_mirror
from tests.fa_cases import by_hand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEN = {}  # what the mirrored sets hold, summed by test_mirror and asserted by test_the_sets_hold_what_they_are_for


@pytest.fixture(scope="module")
def ctx():
    with fa.Context(None) as c:
        yield c


def run(ctx, rs, ex, moves, centres, **cfg):
    return ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path="host", moves=moves, **cfg).fetch()


def test_golden_signal_lengths():
    n = {"table": 0, "none": 0}
    for mv, l, reverse, tagged, sig in golden_tables():
        cum, has = fa.dwell_cum(mv if tagged else mv[:0], l, reverse)
        assert cum.shape == (l + 1,) and cum[0] == 0
        if sig is None:
            assert not has and not cum.any()
            n["none"] += 1
        else:
            assert has and np.array_equal(np.diff(cum), sig)
            n["table"] += 1
    assert n["table"] > 200 and n["none"] > 40


@pytest.mark.parametrize("name", sorted(SETS) + ["op_kinds"])
def test_mirror(ctx, name):
    if name == "op_kinds":
        rs, ex, moves, centres, _ = op_kinds()
        cfg = {}
    else:
        rs, ex, moves, centres, cfg = generated(name)
    r = run(ctx, rs, ex, moves, centres, **cfg)
    rows, counts, depths, lines, seen = dwell_mirror(rs, ex, moves, centres, rs["ref_bytes"], rs["ref_first"], **cfg)
    assert ctx.channels() == 9 and r["rows"].shape == rows.shape and rows.shape[1:] == (33, 9)
    assert np.array_equal(r["counts"], counts) and np.array_equal(r["depths"], depths)
    assert np.array_equal(r["rows"], rows)
    assert r["text"].decode("ascii").split("\n")[:-1] == lines
    if name == "over_deep":
        assert ctx.stats()["deep_windows"] > 10 and counts.max() == 55
    SEEN[name] = seen
    # the invariant: everything but channel 8 is what the 8-channel entry gives on the same reads
    r8 = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path="host", **cfg).fetch()
    assert ctx.channels() == 8 and r8["rows"].shape[1:] == (33, 8)
    assert np.array_equal(r["rows"][:, :, :8], r8["rows"]) and r["text"] == r8["text"]
    assert np.array_equal(r["counts"], r8["counts"]) and np.array_equal(r["depths"], r8["depths"])
    assert ctx.dwell_table().size == 0  # (the last call was no dwell call)


def test_the_sets_hold_what_they_are_for():
    assert set(SEEN) == set(SETS) | {"op_kinds"}, "run the whole file: test_mirror fills the counters"
    total = {k: sum(s[k] for s in SEEN.values()) for k in next(iter(SEEN.values()))}
    assert all(n >= 8 for n in total.values()), total
    assert SETS["plain"][1].get("matrix_depth", 89) == 89 and SETS["over_deep"][1]["matrix_depth"] == 55


def test_phased_form_keeps_the_other_channels(ctx):
    rs, ex, moves, centres, cfg = generated("plain")
    v = syn.make_phased_variants(rs, 7, rate=0.03)
    r = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path="host", moves=moves, variants=v, **cfg).fetch()
    tags = ctx.haplotag_pairs(pairs=False)[0]
    r8 = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path="host", variants=v, **cfg).fetch()
    assert r["rows"].shape[2] == 9 and np.array_equal(r["rows"][:, :, :8], r8["rows"]) and r["text"] == r8["text"]
    assert np.array_equal(tags, ctx.haplotag_pairs(pairs=False)[0]) and set(tags.tolist()) == {0, 1, 2}
    # the tags as given haplotypes: the same 9-channel rows, channel 8 included
    r9 = run(ctx, rs, dict(ex, haplotype=tags), moves, centres, **cfg)
    assert np.array_equal(r["rows"], r9["rows"])


def test_the_table_of_a_call(ctx):
    rs, ex, moves, centres, cfg = generated("every_op")
    run(ctx, rs, ex, moves, centres, **cfg)
    cum = ctx.dwell_table()
    n = len(rs["pos"])
    assert cum.shape == (int(ex["qual_first"][n]) + n,)
    for r in range(n):
        l = int(ex["qual_first"][r + 1] - ex["qual_first"][r])
        want, _ = fa.dwell_cum(moves["mv"][moves["mv_first"][r]:moves["mv_first"][r + 1]], l, bool(rs["flag"][r] & 16))
        at = int(ex["qual_first"][r]) + r
        assert np.array_equal(cum[at:at + l + 1], want)


# ---- one read per clause, the bytes written out.  Read at 100 of "ACGT" * 100, centre 110: column p shows position 94 + p
def one_read(ctx, cigar, seq, table, flag=0, centre=110):
    rs, ex = by_hand([(100, flag, 60, cigar, seq)])
    r = run(ctx, rs, ex, moves_by_hand([table]), [centre])
    assert r["rows"].shape == (1, 33, 9)
    return r["rows"][0, :, 8].tolist()


def test_by_hand_a_shown_cell_and_the_cells_that_are_none(ctx):
    # 20M, base q dwells q + 1 entries: positions 100 .. 119 are columns 6 .. 25
    ch8 = one_read(ctx, "20M", REF[100:120], table_of(range(1, 21)))
    assert ch8 == [0] * 6 + list(range(1, 21)) + [0] * 7
    # the strand: the table is in sequencing order, the bases in the BAM's; base q shows sig[19 - q]
    assert one_read(ctx, "20M", REF[100:120], table_of(range(1, 21)), flag=16) == [0] * 6 + list(range(20, 0, -1)) + [0] * 7
    # no tag, the stride alone: no table, channel 8 is zero
    assert not any(one_read(ctx, "20M", REF[100:120], None)) and not any(one_read(ctx, "20M", REF[100:120], [5]))
    # zeros in front of the first move belong to nobody; K < l: the bases behind have 0; the last base takes the rest of the table
    assert one_read(ctx, "20M", REF[100:120], [5, 0, 0, 0, 1, 0, 1, 0, 0])[6:10] == [2, 3, 0, 0]
    # K > l: the surplus moves are dropped, and the last base does NOT take them
    assert one_read(ctx, "20M", REF[100:120], table_of([2] * 25))[6:26] == [2] * 20
    # any non-zero value is a move, and element 0 is none whatever it holds
    assert one_read(ctx, "20M", REF[100:120], [1] + [-1, 0, 5, 0, 0, -128, 127])[6:11] == [2, 3, 1, 1, 0]


def test_by_hand_deleted_cells_and_insertions(ctx):
    # 10M 2I 10M: the insertion's bases (q 10, 11) add to position 109 (column 15): 10 + 11 + 12
    seq = REF[100:110] + "GT" + REF[110:120]
    ch8 = one_read(ctx, "10M2I10M", seq, table_of(range(1, 23)))
    assert ch8[6:16] == list(range(1, 10)) + [10 + 11 + 12] and ch8[16:26] == list(range(13, 23)) and not any(ch8[26:])
    # two consecutive I ops BOTH add (channel 6 keeps only the last string)
    ch8 = one_read(ctx, "10M1I2I10M", REF[100:110] + "G" + "TT" + REF[110:120], table_of(range(1, 24)))
    assert ch8[15] == 10 + 11 + 12 + 13 and ch8[16] == 14
    # I followed by D: the I adds; the deleted positions (columns 16, 17) are 0
    ch8 = one_read(ctx, "10M2I2D8M", REF[100:110] + "GT" + REF[112:120], table_of(range(1, 21)))
    assert ch8[15] == 10 + 11 + 12 and ch8[16:18] == [0, 0] and ch8[18] == 13
    # D directly followed by I: the I attaches to the last deleted position, which is 0; nothing else takes its bases
    ch8 = one_read(ctx, "10M2D3I8M", REF[100:110] + "CCC" + REF[112:120], table_of(range(1, 22)))
    assert ch8[15] == 10 and ch8[16:18] == [0, 0] and ch8[18] == 14
    # an I in front of the first reference position attaches to nothing
    ch8 = one_read(ctx, "2I20M", "TT" + REF[100:120], table_of(range(1, 23)))
    assert ch8[:6] == [0] * 6 and ch8[6:26] == list(range(3, 23))
    # the cells behind the read's end that channel 6 writes into stay 0 in channel 8: 10M 3I at 100, centre 100
    rs, ex = by_hand([(100, 0, 60, "10M3I", REF[100:110] + "GGG")])
    r = run(ctx, rs, ex, moves_by_hand([table_of([2] * 13)]), [100])
    assert r["rows"][0, 25, 8] == 2 + 6 and r["rows"][0, 26:28, 6].tolist() == [75, 75] and not r["rows"][0, 26:, 8].any()
    # fewer moves than bases (K < l): the last move takes the rest of the table, the insertion's base behind it adds 0
    ch8 = one_read(ctx, "10M2I10M", seq, table_of(range(1, 12)))
    assert ch8[15] == 10 + 11 and ch8[16] == 0


def test_by_hand_the_int8_quirk(ctx):
    """(int8_t) of the int32 sum, no clamp: 127 stays, 128 is -128, 200 is -56, 255 is -1, 256 is 0, 300 is 44"""
    dwells = [127, 128, 200, 255, 256, 300] + [1] * 14
    assert one_read(ctx, "20M", REF[100:120], table_of(dwells))[6:13] == [127, -128, -56, -1, 0, 44, 1]
    # a sum that wraps: the base (100) and its two inserted bases (100, 100) make 300
    seq = REF[100:110] + "GT" + REF[110:120]
    assert one_read(ctx, "10M2I10M", seq, table_of([1] * 9 + [100] * 3 + [1] * 10))[15] == 44


def test_refusals(ctx):
    rs, ex, moves, centres, _ = op_kinds()
    L = _lib.lib()
    reads, extras, m = fa.ReadSet.from_dict(rs), fa.ReadExtras.from_dict(ex), fa.ReadMoves.from_dict(moves)
    cen = np.asarray(centres, np.int64)
    ref = np.ascontiguousarray(rs["ref_bytes"])
    cfg, hcfg = fa.config(), fa.hap_config()
    v = fa.PhasedVariants.from_dict(syn.make_phased_variants(rs, 3, rate=0.05))

    def call(moves_c, variants_c=None, hap_c=None):
        return L.c3_fa_reads_dwell_host(ctx.h, C.byref(reads.c), C.byref(extras.c), moves_c, variants_c, cen.ctypes.data, len(cen), ref.ctypes.data,
                                        int(rs["ref_first"]), len(ref), C.byref(cfg), hap_c)

    assert call(C.byref(m.c)) == 0 and ctx.sizes()[0] == len(cen)
    assert call(None) == 1 and "null moves" in _lib.last_error() and ctx.sizes()[:2] == (0, 0)
    assert call(C.byref(m.c), C.byref(v.c), None) == 1 and "both" in _lib.last_error()
    assert call(C.byref(m.c), None, C.byref(hcfg)) == 1 and "both" in _lib.last_error()
    assert call(C.byref(m.c), C.byref(v.c), C.byref(hcfg)) == 0
    down = dict(moves, mv_first=moves["mv_first"].copy())
    down["mv_first"][3] = down["mv_first"][2] - 1
    with pytest.raises(_lib.C3Error, match="not non-decreasing"):
        run(ctx, rs, ex, down, centres)
    negative = dict(moves, mv_first=moves["mv_first"] - 1)
    with pytest.raises(_lib.C3Error, match="negative"):
        run(ctx, rs, ex, negative, centres)
    assert ctx.sizes()[:2] == (0, 0) and ctx.dwell_table().size == 0  # a refused call leaves no stale result behind
    # every refusal of c3_fa_reads still applies
    with pytest.raises(_lib.C3Error, match="ascending"):
        run(ctx, rs, ex, moves, centres[::-1])
    with pytest.raises(_lib.C3Error, match="without a device"):
        ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path="device", moves=moves)
    with pytest.raises(ValueError, match="move tables for"):
        ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path="host", moves=moves_by_hand([[5, 1]]))
    # offsets that do not start at 0 are rebased
    shifted = {"mv_first": moves["mv_first"] + 7, "mv": np.concatenate([np.full(7, 9, np.int8), moves["mv"]])}
    assert np.array_equal(run(ctx, rs, ex, shifted, centres)["rows"], run(ctx, rs, ex, moves, centres)["rows"])


def test_make_read_moves():
    rs = syn.make_read_set(n_sites=300, depth=30, read_len=(60, 200), seed=5)
    ex = syn.make_read_extras(rs, 6)
    before = {k: np.array(v, copy=True) for k, v in rs.items() if isinstance(v, np.ndarray)}
    a = syn.make_read_moves(rs, ex, 7, stall=0.02, untagged=0.1, surplus=0.1, short=0.1)
    b = syn.make_read_moves(rs, ex, 7, stall=0.02, untagged=0.1, surplus=0.1, short=0.1)
    assert all(np.array_equal(a[k], b[k]) for k in a) and all(np.array_equal(rs[k], v) for k, v in before.items())
    assert a["mv"].dtype == np.int8 and a["mv_first"].dtype == np.int64 and len(a["mv_first"]) == len(rs["pos"]) + 1
    l = np.diff(ex["qual_first"])
    k = np.array([np.count_nonzero(a["mv"][a["mv_first"][r] + 1:a["mv_first"][r + 1]]) for r in range(len(l))])
    size = np.diff(a["mv_first"])
    assert (size == 0).sum() >= 8 and ((size > 0) & (k > l)).sum() >= 8 and ((size > 0) & (k < l)).sum() >= 8
    assert not np.isin(a["mv"], (0, 1)).all()
    calm = syn.make_read_moves(rs, ex, 7, stall=0.0, untagged=0.0, surplus=0.0, short=0.0)
    assert 2.0 < len(calm["mv"]) / l.sum() < 2.5  # about ``mean`` entries per base
    runs = np.diff(np.flatnonzero(a["mv"]))
    assert (runs >= 128).sum() >= 8 and (runs >= 256).sum() >= 8
    order = np.argsort(rs["pos"], kind="stable")
    s = syn.sort_read_moves(rs, a)
    assert np.array_equal(np.diff(s["mv_first"]), size[order])
    r = int(order[5])
    assert np.array_equal(s["mv"][s["mv_first"][5]:s["mv_first"][6]], a["mv"][a["mv_first"][r]:a["mv_first"][r + 1]])


def _case_file(path, rs, ex, moves, centres, cfg):
    head = np.array([len(rs["pos"]), len(rs["cigar"]), len(rs["seq"]), len(ex["qual"]), len(centres), rs["ref_first"], len(rs["ref_bytes"]),
                     cfg["min_mq"], cfg["max_indel_length"], cfg["matrix_depth"], cfg["seed"], 1, len(moves["mv"])], np.int64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for a in (rs["pos"], rs["flag"], rs["mapq"], rs["cigar_first"], rs["cigar"], rs["seq_first"], rs["seq"], ex["qual_first"], ex["qual"],
                  ex["haplotype"], ex["name_key"], np.asarray(centres, np.int64), rs["ref_bytes"], moves["mv_first"], moves["mv"]):
            f.write(np.ascontiguousarray(a).tobytes())


def test_host_form_under_sanitizers(ctx, tmp_path):
    """the rule headers as a stand-alone program (its own main, no Python, no library) under -fsanitize=address,undefined: tables by hand
    and the refusals, and two read sets whose rows and tables must be the library's byte for byte.  Every array sits in a heap block of
    exactly its size; the last read of each set has a table, so it ends exactly at the end of the staged array"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dwell_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                          [os.path.join(ROOT, "tests", "host", "dwell_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, "--tables"], env=env, capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout and not p.stderr, p.stdout + p.stderr
    for i, name in enumerate(("every_op", "over_deep")):
        rs, ex, moves, centres, cfg = generated(name)
        n = len(rs["pos"])
        assert moves["mv_first"][n] == len(moves["mv"]) and moves["mv_first"][n] - moves["mv_first"][n - 1] > 1
        cfg = dict(dict(min_mq=5, max_indel_length=50, matrix_depth=89, seed=0), **cfg)
        case, out = str(tmp_path / f"case{i}.bin"), str(tmp_path / f"out{i}.bin")
        _case_file(case, rs, ex, moves, centres, cfg)
        p = subprocess.run([exe, case, out], env=env, capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr
        want = run(ctx, rs, ex, moves, centres, **cfg)
        raw = open(out, "rb").read()
        n_rows, n_cum = np.frombuffer(raw[:16], np.int64)
        assert n_rows == len(want["rows"]) and n_rows > 1000
        assert raw[16:16 + n_rows * 297] == want["rows"].tobytes()
        assert raw[16 + n_rows * 297:] == ctx.dwell_table().tobytes() and n_cum == ctx.dwell_table().size
