"""Pileup from reads on the device (csrc/c3_pileup.h): c3_pileup_reads against the host form bit for bit -- matrix, major, candidates, depths,
count arrays, alt-info text -- on the golden sets and on generated ones, the fallback on key collisions, buffer reuse across calls, and the
count pair against gVCF mode's own region kernel.  Behind those, the capacity edges: a region of more tiles than one step of the scan holds,
reads of more than 128 ops, the event table's size rule on its boundary, a probe that wraps, and a chained batch above a ring lane's size."""
import numpy as np
import pytest

from clair3_amd import gvcf, pileup_reads as pr, synthetic as syn
from tests.pileup_cases import (LONG_CIGARS, MANY_CANDIDATES, WRAP_SHIFT, big_region, distinct_events, golden_sets, insertion_column, one_read,
                                take_reads)

pytestmark = pytest.mark.gpu

KEYS = ("counts", "major", "cand_pos", "cand_depth", "n_ref", "n_total", "text")
CFG = dict(min_snp_af=0.08, min_indel_af=0.15)


@pytest.fixture(scope="module")
def ctx():
    with pr.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def host_ctx():
    with pr.Context(None) as c:
        yield c


def both(ctx, host_ctx, rs, start=None, end=None, **cfg):
    start, end = rs["start"] if start is None else start, rs["end"] if end is None else end
    want = host_ctx.run(rs, start, end, rs["ref_bytes"], rs["ref_first"], **cfg).fetch()
    got = ctx.run(rs, start, end, rs["ref_bytes"], rs["ref_first"], **cfg).fetch()
    return got, want


def assert_same(got, want, what=""):
    for k in KEYS:
        if k == "text":
            assert got[k] == want[k], f"{what}: text"
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{what}: {k}"


def test_golden_sets(ctx, host_ctx):
    for k, rs, _ in golden_sets():  # (the host form against the fixture's columns: tests/test_pileup_reads.py)
        for cfg in (dict(min_mq=rs["min_mq"], max_indel_length=100, call_ht=True), dict(CFG), dict(CFG, call_snp_only=True), dict(CFG, max_indel_length=1)):
            got, want = both(ctx, host_ctx, rs, **cfg)
            assert_same(got, want, f"set {k} {cfg}")
            assert not ctx.stats()["fell_back"] and not ctx.stats()["on_host"]


GENERATED = {
    "forty_reads": (dict(n_sites=200, depth=12, read_len=(150, 250), seed=22), {}),  # (the first 40 of them)
    # more than one tile of sites, more than one block of every kernel, two gaps, every kind of op
    "two_thousand_reads": (dict(n_sites=3000, depth=60, read_len=(60, 120), seed=23, gaps=2, n_op=0.002, non_acgt=0.01, d_then_i=0.002, i_then_d=0.002,
                                pad=0.1, eqx=True, ref_other=0.01), {}),
    "all_filtered": (dict(n_sites=300, depth=10, read_len=150, seed=24, filtered=1.0), {}),
    "no_gvcf_call_ht": (dict(n_sites=1100, depth=20, read_len=(150, 400), seed=25), dict(gvcf=False, call_ht=True)),
    # reads of more than 64 and more than 128 ops: the op table's carry between its 64-op steps, read by the walk
    "long_cigars": (LONG_CIGARS, {}),
}


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_sets(ctx, host_ctx, name):
    spec, cfg = GENERATED[name]
    rs = syn.make_read_set(**spec)
    if name == "forty_reads":
        rs = take_reads(rs, 40)
        assert len(rs["pos"]) == 40 and rs["end"] - rs["start"] == 200
    got, want = both(ctx, host_ctx, rs, **dict(CFG, **cfg))
    assert_same(got, want, name)
    s = ctx.stats()
    assert not s["fell_back"] and s["reads_kept"] + s["reads_dropped"] == len(rs["pos"])
    if name == "forty_reads":
        assert s["reads_kept"] > 20 and len(want["major"]) > 100
    if name == "two_thousand_reads":
        assert len(rs["pos"]) >= 2000 and 2000 < len(want["major"]) < 3000 and len(want["cand_pos"]) > 10 and s["events"] > 1000
    if name == "all_filtered":
        assert s["reads_kept"] == 0 and len(want["major"]) == 0 and got["text"] == b""
    if name == "long_cigars":
        assert np.diff(rs["cigar_first"]).max() > 128 and s["events"] > 300 and len(want["major"]) == 300
    # thresholds at zero: every column with sixteen neighbours is a candidate, every allele is printed
    got, want = both(ctx, host_ctx, rs)
    assert_same(got, want, name + " thresholds 0")


def test_one_read(ctx, host_ctx):
    """n_reads == 1: one live wave in the op table's workgroup, one workgroup of every per-op kernel, a walk over eight ops"""
    rs = one_read()
    assert len(rs["pos"]) == 1 and len(rs["cigar"]) == 8
    for cfg in (dict(call_ht=True), dict(CFG), dict()):
        got, want = both(ctx, host_ctx, rs, **cfg)
        assert_same(got, want, f"one read {cfg}")
    s = ctx.stats()
    assert s["reads_kept"] == 1 and s["reads_dropped"] == 0 and s["events"] == 2 and not s["fell_back"]
    got, want = both(ctx, host_ctx, rs, call_ht=True)
    assert want["major"].tolist() == list(range(250, 400)) and len(want["cand_pos"]) == 150  # (thresholds 0: every column; the N op's columns too)
    col = want["counts"][want["major"] == 289][0]
    assert col[13] == 1 and col[14] == 1 and want["counts"][want["major"] == 329][0][15] == 1
    assert want["counts"][(want["major"] >= 330) & (want["major"] < 333), 17].tolist() == [1, 1, 1]
    assert not want["counts"][(want["major"] >= 360) & (want["major"] < 372)].any()
    # the same read dropped by its mapq: nothing
    got, want = both(ctx, host_ctx, rs, min_mq=61)
    assert_same(got, want, "one read, dropped")
    assert len(want["major"]) == 0 and ctx.stats()["reads_dropped"] == 1


def test_a_region_that_cuts_every_read(ctx, host_ctx):
    rs = syn.make_read_set(n_sites=400, depth=20, read_len=(300, 500), seed=26, filtered=0, low_mapq=0)
    start, end = rs["start"] + 170, rs["start"] + 230
    spans = rs["pos"] + 300
    assert ((rs["pos"] < start) | (spans > end)).all()  # no read lies inside the region
    got, want = both(ctx, host_ctx, rs, start, end, call_ht=True, **CFG)
    assert_same(got, want)
    assert len(want["major"]) == 60 and want["counts"][:, 8].sum() + want["counts"][:, 17].sum() > 0


def test_one_column_of_300_insertions_and_the_fallback(ctx, host_ctx):
    rs = insertion_column()
    got, want = both(ctx, host_ctx, rs, call_ht=True, **CFG)
    assert_same(got, want)
    s = ctx.stats()
    assert s["events"] == 300 and s["collisions"] == 0 and not s["fell_back"] and not s["on_host"]
    line = want["text"].decode().split("\n")[0]
    assert line.startswith("150-300-") and line.count(" I") + line.count("-I") == 40
    col = int(np.flatnonzero(want["major"] == 149)[0])
    assert want["counts"][col, 4] + want["counts"][col, 13] == 300
    # sixteen keys for forty strings: collisions are certain; the call answers through the host form and says so
    got = ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], call_ht=True, hash_mask=0xF, **CFG).fetch()
    s = ctx.stats()
    assert s["collisions"] > 0 and s["fell_back"] and s["on_host"]
    assert_same(got, want, "fallback")
    # ... and the context is as good as before
    got = ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], call_ht=True, **CFG).fetch()
    assert_same(got, want, "after the fallback")
    assert not ctx.stats()["fell_back"]


def test_two_calls_on_one_context_smaller_then_larger(host_ctx):
    a = syn.make_read_set(n_sites=1500, depth=30, read_len=(100, 200), seed=27)
    b = syn.make_read_set(n_sites=300, depth=10, read_len=(100, 200), seed=28)
    c = syn.make_read_set(n_sites=2500, depth=40, read_len=(100, 200), seed=29, gaps=1)
    with pr.Context(0) as fresh:
        for rs in (a, a, b, a, c, b):
            got, want = both(fresh, host_ctx, rs, **CFG)
            assert_same(got, want)


def test_count_pair_feeds_gvcf_mode_as_the_region_does(ctx):
    rs = syn.make_read_set(n_sites=2200, depth=30, read_len=(100, 300), seed=30, gaps=2, n_op=0.001)
    r = ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], **CFG).fetch()
    n = rs["end"] - rs["start"]
    ref = rs["ref_bytes"][rs["start"] - rs["ref_first"]:rs["end"] - rs["ref_first"]]
    with gvcf.Context() as g:
        from_counts = g.blocks_from_counts(r["n_ref"], r["n_total"], ref, rs["start"] + 1)
        from_region = g.blocks_from_region(r["counts"], r["major"], ref, rs["start"], n, rs["start"] + 1)
    assert len(from_counts) > 10 and from_counts.tobytes() == from_region.tobytes()


# ---- the chained entry: the held result as a candidate batch of the ring, the matrix staying on the device
@pytest.fixture(scope="module")
def chained():
    """a 1 000-site set whose depth lies around the rescaling threshold 1.5 x 144 = 216, a gap in it, and a model"""
    from tests.test_parity_gpu import make_model
    rs = syn.make_read_set(n_sites=1000, depth=240, read_len=(100, 200), seed=31, gaps=1)
    m = make_model(syn.PILEUP, 18, False, syn.make_state_dict(syn.PILEUP, 18, False, seed=531))
    return rs, m


@pytest.mark.parametrize("head_tail", [False, True])
def test_chained_entry_equals_candidates_on_the_fetched_arrays(ctx, chained, head_tail):
    rs, m = chained
    r = ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], **CFG).fetch()
    assert not ctx.stats()["on_host"]
    d = r["cand_depth"]
    assert len(d) > 20 and (d > 216).any() and (d <= 216).any() and len(r["major"]) < 1000
    want_rows, want_status = m.predict_candidates(r["counts"], r["major"], r["cand_pos"], depths=d, head_tail=head_tail)
    assert "rescaled=0" not in m.describe()
    rows, status = m.predict_reads(ctx, head_tail=head_tail)
    assert np.array_equal(status, want_status) and rows.shape == want_rows.shape and rows.tobytes() == want_rows.tobytes()
    assert len(rows) > 20 and (not head_tail or len(rows) >= len(m.predict_candidates(r["counts"], r["major"], r["cand_pos"], depths=d)[0]))
    # through submit and wait on a slot that is not 0, the context reused in between
    ticket = m.submit_reads(ctx, slot=2, head_tail=head_tail)
    rows2, status2 = m.wait(ticket)
    assert np.array_equal(status2, want_status) and rows2.tobytes() == want_rows.tobytes()
    # the next call on the context waits for the batch's copy of the matrix: submit, overwrite the held result, then wait
    ticket = m.submit_reads(ctx, slot=1, head_tail=head_tail)
    other = insertion_column()
    ctx.run(other, other["start"], other["end"], other["ref_bytes"], other["ref_first"], call_ht=True)
    rows3, status3 = m.wait(ticket)
    assert np.array_equal(status3, want_status) and rows3.tobytes() == want_rows.tobytes()


# ---- the capacity edges: the read sets of tests/pileup_cases.py that tests/test_pileup_reads.py holds to the mirror and to their construction
def test_more_tiles_than_one_scan_step(ctx, host_ctx, chained):
    """tile + 3 tiles: the scan's second step, the sums it carries across (columns and candidates of the first cluster), its totals behind
    tile_base's last tile, a last tile of 5 sites; then the chained entry over three stretches of columns a megabase apart"""
    rs, tile = big_region()
    n = rs["end"] - rs["start"]
    step = rs["start"] + tile * tile
    assert (n + tile - 1) // tile > tile and n % tile == 5
    for cfg in (dict(CFG), dict()):
        got, want = both(ctx, host_ctx, rs, **cfg)
        assert_same(got, want, f"more than {tile} tiles {cfg}")
        s = ctx.stats()
        assert not s["fell_back"] and not s["on_host"] and len(got["n_ref"]) == len(got["n_total"]) == n and s["events"] > 500
        major, cand = want["major"], want["cand_pos"]
        assert (major < rs["start"] + 520).any() and ((major >= step - 250) & (major < step)).any() and (major >= step).any() and major.max() == rs["end"] - 1
        assert (cand < step - 250).sum() > 10 and ((cand >= step - 250) & (cand < step)).any() and (cand >= step).sum() > 10 and (cand >= rs["end"] - 420).any()
    m = chained[1]
    r = ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], **CFG).fetch()
    assert len(syn.pileup_chunks(r["major"])[0]) == 3 and len(r["cand_pos"]) > 100
    for head_tail in (False, True):
        want_rows, want_status = m.predict_candidates(r["counts"], r["major"], r["cand_pos"], depths=r["cand_depth"], head_tail=head_tail)
        rows, status = m.predict_reads(ctx, head_tail=head_tail)
        assert np.array_equal(status, want_status) and rows.shape == want_rows.shape and rows.tobytes() == want_rows.tobytes() and len(rows) > 20


@pytest.mark.parametrize("n_ops", (32, 33))
def test_event_table_size_on_its_boundary(ctx, host_ctx, n_ops):
    """32 I and D ops in the kept reads: a table of 64 slots, half full; 33: 128 slots.  Every op an event of its own"""
    rs = distinct_events(n_ops)
    got, want = both(ctx, host_ctx, rs, call_ht=True)
    assert_same(got, want)
    s = ctx.stats()
    assert s["events"] == n_ops and s["collisions"] == 0 and not s["fell_back"] and not s["on_host"] and s["reads_dropped"] == 3
    text = want["text"].decode()
    assert text.count(" I") + text.count("-I") == (n_ops + 1) // 2 and text.count(" D") + text.count("-D") == n_ops // 2


def test_a_probe_of_the_event_table_wraps(ctx, host_ctx):
    """two probes start at the last of 64 slots (tests/test_pileup_reads.py shows it from the kernel's key and slot arithmetic): one goes on at slot 0"""
    rs = distinct_events(32, shift=WRAP_SHIFT)
    got, want = both(ctx, host_ctx, rs, call_ht=True)
    assert_same(got, want)
    s = ctx.stats()
    assert s["events"] == 32 and s["collisions"] == 0 and not s["fell_back"] and not s["on_host"]


def test_one_slot_counted_a_thousand_times(ctx, host_ctx):
    rs = insertion_column(n_reads=3000)
    got, want = both(ctx, host_ctx, rs, call_ht=True, **CFG)
    assert_same(got, want)
    s = ctx.stats()
    assert s["events"] == 3000 and s["collisions"] == 0 and not s["fell_back"]
    col = int(np.flatnonzero(got["major"] == 149)[0])
    assert got["counts"][col, 4] + got["counts"][col, 13] == 3000 and max(got["counts"][col, 5], got["counts"][col, 14]) > 1000 // 80


@pytest.mark.parametrize("head_tail", [False, True])
def test_chained_entry_above_the_lane_limit(ctx, chained, head_tail):
    """every column a candidate: more than the 1024 windows a pileup lane of the ring takes"""
    m = chained[1]
    rs = syn.make_read_set(**MANY_CANDIDATES)
    r = ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], call_ht=True).fetch()
    assert not ctx.stats()["on_host"] and len(r["cand_pos"]) == len(r["major"]) > 1024
    want_rows, want_status = m.predict_candidates(r["counts"], r["major"], r["cand_pos"], depths=r["cand_depth"], head_tail=head_tail)
    rows, status = m.predict_reads(ctx, head_tail=head_tail)
    assert np.array_equal(status, want_status) and rows.shape == want_rows.shape and rows.tobytes() == want_rows.tobytes()
    assert len(rows) > 1024 and np.isfinite(rows).all()


def test_chained_entry_of_a_host_result_and_of_no_candidates(ctx, host_ctx, chained):
    rs, m = chained
    r = host_ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], **CFG).fetch()
    want_rows, want_status = m.predict_candidates(r["counts"], r["major"], r["cand_pos"], depths=r["cand_depth"])
    rows, status = m.predict_reads(host_ctx)
    assert np.array_equal(status, want_status) and rows.tobytes() == want_rows.tobytes()
    # a fallback leaves a host result in a device context: the same
    ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], hash_mask=0x3, **CFG)
    assert ctx.stats()["fell_back"]
    rows, status = m.predict_reads(ctx)
    assert np.array_equal(status, want_status) and rows.tobytes() == want_rows.tobytes()
    # no candidate: no row
    ctx.run(rs, rs["start"], rs["end"], rs["ref_bytes"], rs["ref_first"], min_depth=100000)
    rows, status = m.predict_reads(ctx)
    assert rows.shape == (0, m.row_size) and len(status) == 0
