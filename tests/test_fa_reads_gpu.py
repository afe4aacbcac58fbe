"""Full alignment from reads on the device (csrc/c3_fa_reads.h): c3_fa_reads against the host form bit for bit -- rows, counts, centre depths,
alt-info text -- on the golden sets and on generated ones, the fallback over the lowered LDS cap, buffer reuse across calls, and the chained
predict against c3_predict_rows on the fetched rows.  Behind those, the capacity edges: the candidate kernel's table at 255 .. 1024 reads and
one read over it, indels counted across its 256-read steps, more candidates than two steps of the scan, matrix_depth 1 and 128, and chained
batches above a ring lane's size with empty windows in them and behind a real fallback."""
import ctypes as C

import numpy as np
import pytest

from clair3_amd import _lib, fa_reads as fa, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests.fa_cases import (FILL_LEVELS, INDEL_CENTRE, LDS, MANY, RAGGED, STEP, alt_counts, by_hand, check_fill, check_indel_rows, fill_centres,
                            generated, golden_sets, indel_column, many_candidates, read_range, table_fill, window_numbers)

pytestmark = pytest.mark.gpu

KEYS = ("rows", "counts", "depths", "text")


@pytest.fixture(scope="module")
def ctx():
    with fa.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def host_ctx():
    with fa.Context(None) as c:
        yield c


def both(ctx, host_ctx, rs, ex, centres, **cfg):
    want = host_ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **cfg).fetch()
    got = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **cfg).fetch()
    return got, want


def assert_same(got, want, what=""):
    for k in KEYS:
        if k == "text":
            assert got[k] == want[k], f"{what}: text"
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{what}: {k}"


def test_golden_sets(ctx, host_ctx):
    for k, rs, ex, centres, _ in golden_sets():  # (the host form against the fixture: tests/test_fa_reads.py)
        for cfg in (dict(min_mq=rs["min_mq"]), dict(matrix_depth=55, max_indel_length=1), dict(matrix_depth=12, seed=3)):
            got, want = both(ctx, host_ctx, rs, ex, centres, **cfg)
            assert_same(got, want, f"set {k} {cfg}")
            assert not ctx.stats()["fell_back"] and not ctx.stats()["on_host"]


def test_one_candidate_one_read(ctx, host_ctx):
    rs, ex = by_hand([(100, 16, 60, "10M2I10M3D10M", "ACGTACGTAC" + "GG" + "ACGTACGTAC" + "ACGTACGTAC")], haps=[2])
    got, want = both(ctx, host_ctx, rs, ex, [110])
    assert_same(got, want)
    assert want["counts"].tolist() == [1] and want["depths"].tolist() == [1] and not ctx.stats()["fell_back"]


GENERATED = {
    # 600 adjacent candidates over 700 sites: windows overlap, every kernel runs more than one block
    "adjacent": (dict(n_sites=700, depth=30, read_len=(80, 300), seed=31), dict(), lambda rs: np.arange(rs["start"] + 50, rs["start"] + 650)),
    "deep_89": (dict(n_sites=120, depth=150, read_len=(80, 200), seed=32), dict(matrix_depth=89, seed=11), lambda rs: np.arange(rs["start"], rs["end"], 2)),
    "deep_55": (dict(n_sites=120, depth=150, read_len=(80, 200), seed=32), dict(matrix_depth=55, seed=12), lambda rs: np.arange(rs["start"], rs["end"], 2)),
    # reads of up to 600 ops
    "long_cigars": (dict(n_sites=300, depth=12, read_len=(2000, 4000), seed=33, ins=0.04, dele=0.04, d_then_i=0.01, i_then_d=0.01, pad=0.2, eqx=True,
                         non_acgt=0.01, ref_other=0.02), dict(), lambda rs: np.arange(rs["start"], rs["end"], 3)),
    # candidates at both edges, where coverage ends (make_read_set's reads stop 2 * read_len + 64 outside the region)
    "edges": (dict(n_sites=100, depth=20, read_len=100, seed=34), dict(max_indel_length=10),
              lambda rs: np.concatenate([np.arange(rs["ref_first"] + 16, rs["ref_first"] + 60), np.arange(rs["end"] + 200, rs["end"] + 301)])),
    "all_filtered": (dict(n_sites=100, depth=10, read_len=100, seed=35, filtered=1.0), dict(), lambda rs: np.arange(rs["start"], rs["end"], 5)),
}


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_sets(ctx, host_ctx, name):
    spec, cfg, pick = GENERATED[name]
    rs, ex = generated(**spec)
    if name == "all_filtered":  # (make_read_set's dropped flags are pileup's: two of them are not among the 2316 of this rule)
        rs["flag"] = rs["flag"] | np.uint16(0x4)
    centres = pick(rs)
    got, want = both(ctx, host_ctx, rs, ex, centres, **cfg)
    assert_same(got, want, name)
    s = ctx.stats()
    assert not s["fell_back"] and not s["on_host"] and s["rows"] == len(want["rows"])
    if name == "adjacent":
        assert len(centres) == 600 and want["counts"].min() > 5
    if name.startswith("deep"):
        assert s["deep_windows"] > 30 and want["counts"].max() == cfg["matrix_depth"] and want["depths"].max() > 100
    if name == "long_cigars":
        n_ops = np.diff(rs["cigar_first"])
        assert n_ops.max() > 300, n_ops.max()
    if name == "edges":
        assert (want["counts"] == 0).any() and (want["counts"] > 0).any()
    if name == "all_filtered":
        assert s["reads_kept"] == 0 and len(want["rows"]) == 0 and not want["counts"].any()


def test_lowered_cap_falls_back(ctx, host_ctx):
    rs, ex = generated(n_sites=80, depth=30, read_len=(80, 200), seed=36)
    centres = np.arange(rs["start"], rs["end"], 4)
    got, want = both(ctx, host_ctx, rs, ex, centres, lds_reads=8)
    assert_same(got, want, "lowered cap")
    s = ctx.stats()
    assert s["fell_back"] and s["on_host"] and want["counts"].max() > 8
    got, want = both(ctx, host_ctx, rs, ex, centres)
    assert_same(got, want, "the table's own cap")
    assert not ctx.stats()["fell_back"]


def test_buffer_reuse(ctx, host_ctx):
    big = generated(n_sites=400, depth=40, read_len=(80, 300), seed=37)
    small = generated(n_sites=40, depth=10, read_len=(60, 100), seed=38)
    for (rs, ex), step in ((big, 1), (small, 3), (big, 2)):
        centres = np.arange(rs["start"], rs["end"], step)
        got, want = both(ctx, host_ctx, rs, ex, centres)
        assert_same(got, want, f"step {step}")


# ---- the capacity edges: the read sets of tests/fa_cases.py that tests/test_fa_reads.py holds to the mirror and to their construction
@pytest.mark.parametrize("n_over", FILL_LEVELS)
def test_table_fill_levels(ctx, host_ctx, n_over):
    """exactly n_over reads in the candidate kernel's table, gathered over ragged 256-read steps: every table loop, the tally, the
    (key, index) rank and the (haplotype, index) row at 255 .. 1024 reads, sel[] filled to 89 and to 128"""
    rs, ex, info = table_fill((n_over,))
    centres = fill_centres(info)
    lo, hi = read_range(info, info["centres"][0])
    assert window_numbers(info, info["centres"][0])[0] == n_over and (hi - lo >= 5 * STEP or n_over < LDS - 1)
    for depth in (89, 128):
        got, want = both(ctx, host_ctx, rs, ex, centres, matrix_depth=depth, seed=depth)
        s = ctx.stats()
        assert not s["fell_back"] and not s["on_host"]
        assert_same(got, want, f"{n_over} reads, matrix_depth {depth}")
        check_fill(got, s, info, depth)
        assert got["counts"][1] == min(n_over, depth)


def test_one_read_more_than_the_table_holds(ctx, host_ctx):
    rs, ex, info = table_fill((LDS + 1,))
    centres = fill_centres(info)
    assert window_numbers(info, info["centres"][0])[0] == LDS + 1
    got, want = both(ctx, host_ctx, rs, ex, centres)
    s = ctx.stats()
    assert s["fell_back"] and s["on_host"]
    assert_same(got, want, "over the table")
    check_fill(got, s, info, 89)
    # the next call on the context, at the table's own size, answers on the device again
    rs, ex, info = table_fill((LDS,))
    got, want = both(ctx, host_ctx, rs, ex, fill_centres(info))
    assert_same(got, want, "the table's size behind a fallback")
    assert not ctx.stats()["fell_back"] and not ctx.stats()["on_host"]


@pytest.mark.parametrize("n_over", (88, 89, 90))
def test_boundary_of_deep_selection(ctx, host_ctx, n_over):
    rs, ex, info = table_fill((n_over,))
    got, want = both(ctx, host_ctx, rs, ex, info["centres"], matrix_depth=89)
    assert_same(got, want)
    s = ctx.stats()
    assert got["counts"].tolist() == [min(n_over, 89)] and s["deep_windows"] == (1 if n_over == 90 else 0) and not s["fell_back"]


def test_matrix_depth_1(ctx, host_ctx):
    rs, ex, info = table_fill((300,))
    got, want = both(ctx, host_ctx, rs, ex, fill_centres(info), matrix_depth=1, seed=4)
    assert_same(got, want)
    check_fill(got, ctx.stats(), info, 1)
    assert got["counts"].tolist() == [1, 1] and ctx.stats()["deep_windows"] == 2 and not ctx.stats()["fell_back"]


def test_neighbouring_candidates_of_different_trip_counts(ctx, host_ctx):
    rs, ex, info = table_fill((LDS, 300))
    centres = fill_centres(info)
    assert [window_numbers(info, c)[0] for c in info["centres"]] == [LDS, 300]
    for depth in (89, 128):
        got, want = both(ctx, host_ctx, rs, ex, centres, matrix_depth=depth)
        assert_same(got, want)
        check_fill(got, ctx.stats(), info, depth)
        assert not ctx.stats()["fell_back"]


@pytest.mark.parametrize("depth", (89, 128, 1))
def test_indels_counted_across_the_256_boundary(ctx, host_ctx, depth):
    rs, ex, expected, kinds = indel_column()
    centres = [INDEL_CENTRE - 16, INDEL_CENTRE, INDEL_CENTRE + 16, INDEL_CENTRE + 17]
    got, want = both(ctx, host_ctx, rs, ex, centres, matrix_depth=depth, seed=3)
    assert_same(got, want)
    assert not ctx.stats()["fell_back"] and len(kinds) > 2 * STEP
    assert alt_counts(got["text"].decode("ascii").split("\n")[1]) == expected and got["depths"][1] == len(kinds)
    n_ins, n_del = check_indel_rows(got, expected)
    assert depth == 1 or (n_ins > 20 and n_del > 10)


def test_more_candidates_than_two_scan_steps(ctx, host_ctx):
    """the scan's second and third step, its carry and the totals behind it: the first 1024 and 1025 candidates and all of them; equal
    rows mean that every candidate's base offset is right"""
    tile = _lib.lib().c3_pileup_tile_sites()
    rs, ex, centres = many_candidates(*MANY[0], **MANY[1])
    assert len(centres) > 2 * tile
    for n in (tile, tile + 1, len(centres)):
        got, want = both(ctx, host_ctx, rs, ex, centres[:n], **MANY[2])
        assert_same(got, want, f"{n} candidates")
        s = ctx.stats()
        assert len(got["counts"]) == n and s["deep_windows"] > 50 and s["rows"] == len(want["rows"]) and not s["fell_back"]
    assert (got["counts"] == 0).any() and (got["counts"][2 * tile:] == MANY[2]["matrix_depth"]).any()


@pytest.fixture(scope="module")
def models():
    out = {}
    for depth in (89, 55):
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=41)
        m = Clair3_F(add_indel_length=True, predict=True, input_channels=8)
        m.set_geometry(depth, 33)
        m = m.to("cuda:0")
        m.eval()
        m.decode_columns(True)  # (the rows carry the decoder columns behind the probabilities)
        m.load_state_dict(sd)
        out[depth] = m
    return out


@pytest.mark.parametrize("depth", (89, 55))
def test_chained_predict(ctx, models, depth):
    m = models[depth]
    rs, ex = generated(n_sites=90, depth=70, read_len=(80, 200), seed=42)
    centres = np.arange(rs["start"], rs["end"], 2)
    r = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], matrix_depth=depth, seed=5).fetch()
    assert r["counts"].max() == depth or depth == 89
    want = m.predict_rows(r["rows"], r["counts"])
    got = m.predict_reads(ctx)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.shape[1] == m.row_size and np.isfinite(got).all()
    # the context's next call waits for the copy; the held rows of the next call are its own
    r2 = ctx.run(rs, ex, centres[:10], rs["ref_bytes"], rs["ref_first"], matrix_depth=depth, seed=5).fetch()
    assert np.array_equal(r2["rows"], r["rows"][:int(r["counts"][:10].sum())])
    got2 = m.predict_reads(ctx)
    assert np.array_equal(got2.view(np.uint32), want[:10].view(np.uint32))
    # a held result of the host form is staged from the host
    with fa.Context(0) as c2:
        c2.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path="host", matrix_depth=depth, seed=5)
        assert np.array_equal(m.predict_reads(c2).view(np.uint32), want.view(np.uint32))


def test_chained_predict_large_and_ragged(ctx, models):
    """more windows than a ring lane takes (512) and than one step of the scan, empty windows and over-deep ones among them: the rows go
    from the context to the slot on the device"""
    m = models[55]
    tile = _lib.lib().c3_pileup_tile_sites()
    rs, ex, centres = many_candidates(*RAGGED[0], **RAGGED[1])
    r = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **RAGGED[2]).fetch()
    s = ctx.stats()
    assert not s["on_host"] and len(centres) >= 1100 and len(centres) > tile and s["deep_windows"] > 100
    assert (r["counts"] == 0).sum() > 10 and (r["counts"] == 55).any() and ((r["counts"] > 0) & (r["counts"] < 55)).any()
    want = m.predict_rows(r["rows"], r["counts"])
    got = m.predict_reads(ctx)
    assert got.shape == want.shape == (len(centres), m.row_size) and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # through submit and wait on a slot that is not 0
    y, n = np.empty_like(want), C.c_int64(0)
    _lib.check(_lib.lib().c3_predict_submit_fa_reads(m._handle, ctx.h, y.ctypes.data, C.byref(n), 2), "c3_predict_submit_fa_reads")
    got2 = m.wait((2, y))
    assert n.value == len(centres) and np.array_equal(got2.view(np.uint32), want.view(np.uint32))


def test_chained_predict_behind_a_real_fallback(ctx, host_ctx, models):
    """a window of one read more than the table holds: the device context is left with the host form's result, and the chained entry
    stages that"""
    m = models[55]
    rs, ex, info = table_fill((LDS + 1,))
    centres = fill_centres(info)
    ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], matrix_depth=55, seed=6)
    assert ctx.stats()["fell_back"] and ctx.stats()["on_host"]
    r = host_ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], matrix_depth=55, seed=6).fetch()
    assert r["counts"].tolist() == [55, 55]
    want = m.predict_rows(r["rows"], r["counts"])
    got = m.predict_reads(ctx)
    assert np.isfinite(got).all() and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_chained_refusals(ctx, models):
    rs, ex = generated(n_sites=40, depth=10, read_len=(60, 100), seed=43)
    centres = np.arange(rs["start"], rs["end"], 4)
    ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], matrix_depth=55)
    with pytest.raises(_lib.C3Error, match="matrix_depth 55"):
        models[89].predict_reads(ctx)
    sd = syn.make_state_dict(syn.PILEUP, 18, False, seed=44)
    p = Clair3_P(add_indel_length=False, predict=True, input_channels=18).to("cuda:0")
    p.eval()
    p.load_state_dict(sd)
    y = np.zeros((len(centres), p.row_size), np.float32)
    assert _lib.lib().c3_predict_fa_reads(p._handle, ctx.h, y.ctypes.data, None) != 0 and "pileup handle" in _lib.last_error()
    sd9 = syn.make_state_dict(syn.FULL_ALIGNMENT, 9, True, seed=45)
    m9 = Clair3_F(add_indel_length=True, predict=True, input_channels=9).to("cuda:0")
    m9.eval()
    m9.load_state_dict(sd9)
    ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], matrix_depth=89)
    with pytest.raises(_lib.C3Error, match="9 channels"):
        m9.predict_reads(ctx)
    # nothing was queued: the handles still answer
    assert models[89].predict_reads(ctx).shape == (len(centres), models[89].row_size)
