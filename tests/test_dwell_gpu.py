"""The dwell channel on the device (csrc/c3_dwell.h): the table kernel against the host rule at its step edges and at every byte alignment
of a table's start, the 9-channel windows against the host form bit for bit -- rows, counts, centre depths, text -- with the 297-byte blocks
on all four byte alignments and ragged last steps, the 8-channel call unchanged around a dwell call, the fallback, and the chained predict
of a 9-channel model against c3_predict_rows on the fetched rows."""
import functools

import numpy as np
import pytest

from clair3_amd import _lib, fa_reads as fa, synthetic as syn
from clair3_amd.model import Clair3_F
from tests.dwell_cases import REF, SETS, generated, moves_by_hand, op_kinds, table_of

pytestmark = pytest.mark.gpu

KEYS = ("rows", "counts", "depths", "text")
S = _lib.lib().c3_fa_dwell_step()


@pytest.fixture(scope="module")
def ctx():
    with fa.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def host_ctx():
    with fa.Context(None) as c:
        yield c


def both(ctx, host_ctx, rs, ex, moves, centres, **cfg):
    want = host_ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], moves=moves, **cfg).fetch()
    got = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], moves=moves, **cfg).fetch()
    return got, want


def assert_same(got, want, what=""):
    for k in KEYS:
        if k == "text":
            assert got[k] == want[k], f"{what}: text"
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{what}: {k}"


# ---- the table kernel
LENGTHS = (0, 1, 2, 15, 16, 17, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S + 1)


@functools.lru_cache(maxsize=None)
def packed_tables():
    """(rs, ex, moves, what): reads of one base at 100 whose move tables are packed back to back.  In front of each table under test stands a
    filler table of 0 .. 15 entries, so that the starts fall on every byte alignment modulo 16.  what[r]: the kind of table read r has"""
    rng = np.random.default_rng(91)
    tables, ls, flags, what = [], [], [], []
    at = 0

    def add(kind, make, l=None, flag=0, align=None):
        """make(A): the table of a read that starts at byte A; l: its quality bytes (None: K + (-1, 0, 1) in turn)"""
        nonlocal at
        if align is not None:
            fill = (align - at) % 16
            t = np.where(rng.random(fill) < 0.5, 1, 0).astype(np.int8)
            tables.append(t), ls.append(int(rng.integers(1, 4))), flags.append(0), what.append("filler")
            at += fill
        t = np.asarray(make(at), np.int8)
        k = int(np.count_nonzero(t[1:]))
        tables.append(t), ls.append(max(k + len(tables) % 3 - 1, 0) if l is None else l), flags.append(flag), what.append(kind)
        at += len(t)

    n = 0
    for L in LENGTHS:
        for density in (0.45, 0.9):
            for flag in (0, 16):
                add(f"L{L}", lambda A, L=L, d=density: np.where(rng.random(L) < d, rng.choice((1, 1, -1, 5), size=L), 0), flag=flag, align=(5 * n + 3) % 16)
                n += 1

    def edge(A):  # a move on the last entry of the first step and on the first entry of the second, and on those of the next boundary
        t = np.zeros(2 * S + 40, np.int8)
        b = S - A % 16
        t[[b - 1, b, b + S - 1, b + S]] = 1
        t[0] = 7
        return t

    def long_run(A):  # a dwell above S: a whole step that adds nothing to the carry
        t = np.zeros(3 * S + 9, np.int8)
        t[[0, 3, 2 * S + 300, 2 * S + 301, 3 * S + 8]] = 1
        return t

    for a in (0, 1, 7, 15):
        for flag in (0, 16):
            add("edge", edge, l=4, flag=flag, align=a)
            add("long_run", long_run, l=5, flag=flag, align=a)
    for l in (1, 3):
        add("stride_only", lambda A: [5] + [0] * 39, l=l, align=9)  # a non-zero only in element 0: it must not count
    for k_over_l in (-1, 0, 1):  # around a step's end, K one below, equal to and one above l
        for flag in (0, 16):
            t = np.where(rng.random(S + 30) < 0.5, 1, 0).astype(np.int8)
            add("k_l", lambda A, t=t: t, l=max(int(np.count_nonzero(t[1:])) - k_over_l, 0), flag=flag, align=11)
    # one read of 40 000 bases beside reads of 60
    for i in range(6):
        add("short", lambda A: table_of(1 + rng.poisson(1.2, size=60), lead=i % 3), l=60, flag=16 * (i % 2))
    add("long", lambda A: table_of(1 + rng.poisson(1.2, size=40000)), l=40000, flag=16, align=13)
    add("short", lambda A: table_of(1 + rng.poisson(1.2, size=60)), l=60)
    reads = [(100, f, 60, "1M" if l else "1D", "A" if l else "") for f, l in zip(flags, ls)]
    rs = syn.pack_reads(reads)
    rs["ref_bytes"], rs["ref_first"] = np.frombuffer(REF.encode(), np.uint8), 0
    ex = {"qual_first": np.concatenate([[0], np.cumsum(ls)]).astype(np.int64), "qual": np.full(int(np.sum(ls)), 30, np.uint8),
          "haplotype": np.zeros(len(ls), np.uint8), "name_key": np.arange(1, len(ls) + 1, dtype=np.uint64)}
    return rs, ex, moves_by_hand(tables), what


def test_table_kernel_against_the_host_rule(ctx, host_ctx):
    rs, ex, moves, what = packed_tables()
    n = len(what)
    first, size, l = moves["mv_first"], np.diff(moves["mv_first"]), np.diff(ex["qual_first"])
    under_test = np.array([w != "filler" for w in what])
    # what the set is for
    assert set((first[:-1][under_test] % 16).tolist()) == set(range(16)) and set(size[under_test].tolist()) >= set(LENGTHS)
    assert n < _lib.lib().c3_fa_lds_reads() and l.max() == 40000 and set(rs["flag"].tolist()) == {0, 16}
    for r in np.flatnonzero([w == "edge" for w in what]):
        t, b = moves["mv"][first[r]:first[r + 1]], S - int(first[r]) % 16
        assert int(first[r]) + b - S == int(first[r]) // 16 * 16 and t[b - 1]  # (a read's steps start at the 16-byte boundary in front of it) and t[b] and t[b + S - 1] and t[b + S] and np.count_nonzero(t[1:]) == 4
    for r in np.flatnonzero([w == "long_run" for w in what]):
        t = moves["mv"][first[r]:first[r + 1]]
        assert np.diff(np.flatnonzero(t[1:])).max() > 2 * S
    k = np.array([np.count_nonzero(moves["mv"][first[r] + 1:first[r + 1]]) for r in range(n)])
    at_k_l = np.array([w == "k_l" for w in what])
    assert set((k - l)[at_k_l].tolist()) == {-1, 0, 1}
    got, want = both(ctx, host_ctx, rs, ex, moves, [100], matrix_depth=128)
    assert not ctx.stats()["fell_back"] and not ctx.stats()["on_host"]
    cum, host_cum = ctx.dwell_table(), host_ctx.dwell_table()
    assert cum.shape == host_cum.shape == (int(l.sum()) + n,)
    for r in range(n):  # the per-read rule, read by read, so that a failure names the table
        one, _ = fa.dwell_cum(moves["mv"][first[r]:first[r + 1]], int(l[r]), bool(rs["flag"][r] & 16))
        a = int(ex["qual_first"][r]) + r
        assert np.array_equal(cum[a:a + int(l[r]) + 1], one), f"read {r} ({what[r]}): {size[r]} entries from byte {first[r]}, l {l[r]}, flag {rs['flag'][r]}"
    assert np.array_equal(cum, host_cum)
    assert cum.max() > S  # (the dwell above a step)
    assert_same(got, want)


# ---- the windows
@pytest.mark.parametrize("name", sorted(SETS) + ["op_kinds"])
def test_windows_against_the_host_form(ctx, host_ctx, name):
    if name == "op_kinds":
        rs, ex, moves, centres, _ = op_kinds()
        cfg = {}
    else:
        rs, ex, moves, centres, cfg = generated(name)
    got, want = both(ctx, host_ctx, rs, ex, moves, centres, **cfg)
    assert_same(got, want, name)
    s = ctx.stats()
    assert got["rows"].shape[1:] == (33, 9) and ctx.channels() == 9 and not s["fell_back"] and not s["on_host"] and got["rows"][:, :, 8].any()
    assert np.array_equal(ctx.dwell_table(), host_ctx.dwell_table())
    assert set(s["kernel_ms"]) >= {"moves_staged", "dwell_table"}
    # the 8-channel call on the same context, behind the dwell call and in front of the next: the bytes it gave
    before = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **cfg).fetch()
    assert ctx.channels() == 8 and before["rows"].shape[1:] == (33, 8) and ctx.dwell_table().size == 0
    again, _ = both(ctx, host_ctx, rs, ex, moves, centres, **cfg)
    after = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **cfg).fetch()
    want8 = host_ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **cfg).fetch()
    assert_same(again, want, name)
    assert_same(before, want8, name), assert_same(after, want8, name)
    assert np.array_equal(got["rows"][:, :, :8], before["rows"])


@functools.lru_cache(maxsize=None)
def block_alignments():
    """(rs, ex, moves, centres, counts): candidates 60 apart with counts[i] reads each (40M from centre - 16, so that the first and the last
    cell of every row are shown); the base under a row's last column dwells 1 + (read index % 100) entries"""
    counts = [1, 2, 3, 4, 1, 89, 2, 128, 3, 1, 4, 2, 89, 1]
    reads, tables = [], []
    for i, n in enumerate(counts):
        c = 120 + 60 * i
        for _ in range(n):
            r = len(reads)
            reads.append((c - 16, 16 * (r % 2), 60, "40M", (REF * 4)[c - 16:c + 24]))
            dwell = [1 + (r + q) % 7 for q in range(40)]
            dwell[7 if r % 2 else 32] = 1 + r % 100  # (query offset 32 is column 32; on the reverse strand the table runs the other way)
            tables.append(table_of(dwell))
    from tests.fa_cases import by_hand
    rs, ex = by_hand(reads, quals=[(5 * i) % 40 for i in range(len(reads))], haps=[i % 3 for i in range(len(reads))], ref=REF * 4)
    return rs, ex, moves_by_hand(tables), [120 + 60 * i for i in range(len(counts))], counts


def test_blocks_on_every_byte_alignment(ctx, host_ctx):
    rs, ex, moves, centres, counts = block_alignments()
    got, want = both(ctx, host_ctx, rs, ex, moves, centres, matrix_depth=128)
    assert got["counts"].tolist() == counts and 89 == 12 * 7 + 5 and 128 % 7 != 0
    first = 297 * np.concatenate([[0], np.cumsum(counts)])
    assert set((first[:-1] % 4).tolist()) == {0, 1, 2, 3}
    assert counts[:4] == [1, 2, 3, 4] and set((first[:4] % 4).tolist()) == {0, 1, 2, 3}  # (297 = 4 x 74 + 1)
    g, w = got["rows"].reshape(-1).view(np.uint8), want["rows"].reshape(-1).view(np.uint8)
    for i in range(len(counts)):  # the first and the last byte of every block, and the neighbours' bytes beside them
        a, b = int(first[i]), int(first[i + 1])
        assert g[a] == w[a] != 0 and g[b - 1] == w[b - 1] != 0, f"candidate {i}: its own edge bytes"
        if i > 0:
            assert g[a - 1] == w[a - 1] and g[a - 1] != g[b - 1], f"candidate {i}: the byte in front is the neighbour's last"
        if i + 1 < len(counts):
            assert g[b] == w[b], f"candidate {i}: the byte behind is the neighbour's first"
    assert_same(got, want)


def test_lowered_cap_falls_back_with_nine_channels(ctx, host_ctx):
    rs, ex, moves, centres, cfg = generated("plain")
    got, want = both(ctx, host_ctx, rs, ex, moves, centres, **dict(cfg, lds_reads=8))
    s = ctx.stats()
    assert s["fell_back"] and s["on_host"] and ctx.channels() == 9 and got["rows"].shape[1:] == (33, 9)
    assert_same(got, want)
    assert np.array_equal(ctx.dwell_table(), host_ctx.dwell_table())
    got, want = both(ctx, host_ctx, rs, ex, moves, centres, **cfg)  # and the next call is a device call again
    assert not ctx.stats()["fell_back"]
    assert_same(got, want)


# ---- chained
@pytest.fixture(scope="module")
def models():
    out = {}
    for ch in (9, 8):
        sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, True, seed=46)
        m = Clair3_F(add_indel_length=True, predict=True, input_channels=ch)
        m.set_geometry(89, 33)
        m = m.to("cuda:0")
        m.eval()
        m.decode_columns(True)
        m.load_state_dict(sd)
        out[ch] = m
    return out


@functools.lru_cache(maxsize=None)
def chained_set():
    rs0 = syn.make_read_set(n_sites=300, depth=40, read_len=(80, 200), seed=47)
    ex0 = syn.make_read_extras(rs0, 48)
    mv0 = syn.make_read_moves(rs0, ex0, 49, stall=0.03)
    rs = syn.sort_read_set(rs0)
    return rs, syn.sort_read_extras(rs0, ex0), syn.sort_read_moves(rs0, mv0), syn.make_phased_variants(rs, 50, rate=0.03)


@pytest.mark.parametrize("n_cand", (5, 300))
@pytest.mark.parametrize("phased", (False, True))
def test_chained_predict(ctx, models, n_cand, phased):
    m = models[9]
    rs, ex, moves, variants = chained_set()
    centres = np.arange(rs["start"], rs["start"] + n_cand)
    kw = dict(moves=moves, variants=variants if phased else None)
    r = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], **kw).fetch()
    assert r["rows"].shape[1:] == (33, 9) and not ctx.stats()["on_host"] and len(r["counts"]) == n_cand
    want = m.predict_rows(r["rows"], r["counts"])
    got = m.predict_reads(ctx)
    assert got.shape == want.shape == (n_cand, m.row_size) and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if phased:  # the tags never visited the host on the way; fetched now, they are the stand-alone call's
        tags = ctx.haplotag_pairs(pairs=False)[0]
        assert np.array_equal(tags, ctx.haplotag(rs, variants, rs["ref_bytes"], rs["ref_first"])) and set(tags.tolist()) == {0, 1, 2}
    # the dwell channel matters to the network: without it the rows differ
    r0 = r["rows"].copy()
    r0[:, :, 8] = 0
    assert not np.array_equal(m.predict_rows(r0, r["counts"]), want)


def test_chained_refusals(ctx, models):
    rs, ex, moves, _ = chained_set()
    centres = np.arange(rs["start"], rs["start"] + 5)
    ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], moves=moves)
    with pytest.raises(_lib.C3Error, match="8 channels; the held windows have 9"):
        models[8].predict_reads(ctx)
    assert models[9].predict_reads(ctx).shape == (5, models[9].row_size)  # nothing was queued: the result still answers
    ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"])
    with pytest.raises(_lib.C3Error, match="9 channels; the held windows have 8"):
        models[9].predict_reads(ctx)
    assert models[8].predict_reads(ctx).shape == (5, models[8].row_size)
