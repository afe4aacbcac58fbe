"""Full alignment from reads on the device (csrc/c3_fa_reads.h): c3_fa_reads against the host form bit for bit -- rows, counts, centre depths,
alt-info text -- on the golden sets and on generated ones, the fallback over the lowered LDS cap, buffer reuse across calls, and the chained
predict against c3_predict_rows on the fetched rows."""
import numpy as np
import pytest

from clair3_amd import _lib, fa_reads as fa, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests.fa_cases import by_hand, generated, golden_sets

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
