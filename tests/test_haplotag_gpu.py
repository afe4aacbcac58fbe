"""Haplotagging the reads on the device (csrc/c3_hap_reads.h): c3_fa_haplotag against the host form bit for bit -- tags, pair alleles, pair
offsets -- on the golden sets, the rougher generated ones and the hand-worked reads, reads of 600 ops, the empty shapes, the capacity edges
of the two kernels (pairs around the pair kernel's workgroup, one read over more variants than a step of the vote kernel, a query of 221
bases in one context, reads of exactly 10, 11, 20 and 21 reference bases), buffer reuse across calls, and the chained call
c3_fa_reads_phased against the host chain, through the window step's fallback too, with the chained predict behind it."""
import ctypes as C

import numpy as np
import pytest

from clair3_amd import _lib, fa_reads as fa, synthetic as syn
from clair3_amd.model import Clair3_F
from tests import hap_mirror as hm
from tests.test_haplotag import ROUGH, golden_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with fa.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def host_ctx():
    with fa.Context(None) as c:
        yield c


def both(ctx, host_ctx, rs, v, **cfg):
    """the device's (hap, alleles, pair_first), after holding them to the host form's"""
    want_hap = host_ctx.haplotag(rs, v, rs["ref_bytes"], rs["ref_first"], path="host", **cfg)
    want = host_ctx.haplotag_pairs()
    got_hap = ctx.haplotag(rs, v, rs["ref_bytes"], rs["ref_first"], path="device", **cfg)
    got = ctx.haplotag_pairs()
    assert np.array_equal(got_hap, want_hap) and got_hap.dtype == np.uint8
    for g, w, what in zip(got, want, ("hap", "alleles", "pair_first")):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, np.flatnonzero(g != w)[:10])
    hs, ds = host_ctx.haplotag_stats(), ctx.haplotag_stats()
    assert not ds["on_host"] and hs["on_host"] and all(ds[k] == hs[k] for k in ("reads_hap", "reads_low_mapq", "pairs_realigned", "pairs_allele0"))
    return got


def shape():
    block, chunk = C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().c3_fa_haplotag_shape(C.byref(block), C.byref(chunk)), "c3_fa_haplotag_shape")
    return block.value, chunk.value


def test_golden_sets(ctx, host_ctx):
    for k, rs, v, hap, alleles, pair_first in golden_sets():
        got = both(ctx, host_ctx, rs, v)
        assert np.array_equal(got[0], hap) and np.array_equal(got[1], alleles) and np.array_equal(got[2], pair_first)
        assert ctx.haplotag_stats()["kernel_ms"]["pairs"] > 0


@pytest.mark.parametrize("name", sorted(ROUGH))
def test_rough_sets(ctx, host_ctx, name):
    rs, v = ROUGH[name]
    got = both(ctx, host_ctx, rs, v)
    assert len(got[1]) > 90 and (got[1] != 0).any()
    for mq in (0, 45):
        both(ctx, host_ctx, rs, v, min_haplotag_mq=mq)


def test_reads_by_hand(ctx, host_ctx):
    for name, rs, v, want in hm.hand_cases():
        assert both(ctx, host_ctx, rs, v)[0].tolist() == [want], name


def long_read(n_variants, step=2, cigar=None, mapq=60, carry_every=3):
    """one read over ``n_variants`` variants ``step`` bases apart (it carries every ``carry_every``-th alt base), between two reads below
    the mapq, which have no pairs"""
    span = n_variants * step + 40
    ref = hm.periodic_ref(span + 300)
    pos = 120 + step * np.arange(n_variants)
    alt = np.frombuffer(b"ACGT", np.uint8)[(pos + 1) % 4]
    carry = {int(p): chr(a) for p, a in zip(pos[::carry_every], alt[::carry_every])}
    reads = []
    for first, mq, c in ((100, 3, "50M"), (100, mapq, cigar or f"{span}M"), (101, 7, "50M")):
        r = hm.hand_read(c, first=first, mapq=mq, carry=carry, inserted="GATTACA" * 200, ref=ref)
        letters = "".join(hm.NT16[x] for x in np.stack([r["seq"] >> 4, r["seq"] & 15], 1).reshape(-1))[:int(syn.query_lengths(r)[0])]
        reads.append((first, 0, mq, c, letters))
    rs = syn.pack_reads(reads)
    rs.update(ref_bytes=ref, ref_first=0)
    rng = np.random.default_rng(n_variants)
    v = {"pos": pos, "alt_base": alt, "genotype": rng.integers(1, 3, n_variants).astype(np.uint8), "phase_set": (pos // 50).astype(np.int32)}
    return rs, v


def test_a_read_of_600_ops(ctx, host_ctx):
    cigar = "10M" + "2M1I2M1D" * 149 + "1S" + "1H"
    rs, v = long_read(300, step=3, cigar=cigar)
    assert rs["cigar_first"][2] - rs["cigar_first"][1] == 599
    got = both(ctx, host_ctx, rs, v)
    assert len(got[1]) > 200 and len(set(got[1])) == 3


def test_empty_shapes(ctx, host_ctx):
    rs, v = ROUGH["eqx_pad"]
    none = {"pos": np.zeros(0, np.int64), "alt_base": np.zeros(0, np.uint8), "genotype": np.zeros(0, np.uint8), "phase_set": np.zeros(0, np.int32)}
    got = both(ctx, host_ctx, rs, none)  # zero variants
    assert not got[0].any() and len(got[0]) == len(rs["pos"]) and len(got[1]) == 0 and not got[2].any()
    no_reads = dict(syn.pack_reads([]), ref_bytes=rs["ref_bytes"], ref_first=rs["ref_first"])
    got = both(ctx, host_ctx, no_reads, v)  # zero reads
    assert len(got[0]) == 0 and got[2].tolist() == [0]
    behind = np.arange(rs["ref_first"] + len(rs["ref_bytes"]) - 60, rs["ref_first"] + len(rs["ref_bytes"]) - 11, 2)  # behind every read
    far = {k: a[:len(behind)] for k, a in v.items()}
    far["pos"] = behind
    got = both(ctx, host_ctx, rs, far)  # reads that meet no variant
    assert len(behind) > 20 and not got[0].any() and len(got[1]) == 0
    got = both(ctx, host_ctx, rs, v, min_haplotag_mq=61)  # every read below the mapq
    assert not got[0].any() and len(got[1]) == 0 and ctx.haplotag_stats()["reads_low_mapq"] == len(rs["pos"])


def test_pairs_around_the_pair_kernels_workgroup(ctx, host_ctx):
    block, _ = shape()
    for n in (block - 1, block, block + 1, 2 * block):
        rs, v = long_read(n)
        got = both(ctx, host_ctx, rs, v)
        assert got[2].tolist() == [0, 0, n, n] and (got[1] == 2).sum() >= n // 3 - 12 and (got[1] == 1).sum() > n // 2


def test_one_read_over_more_variants_than_a_vote_step(ctx, host_ctx):
    _, chunk = shape()
    tags = set()
    for n in (chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 5 * chunk + 3):
        for every in (2, 3):
            rs, v = long_read(n, carry_every=every)
            got = both(ctx, host_ctx, rs, v)
            want = hm.haplotag(rs, v, rs["ref_bytes"], 0)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0][0] == got[0][2] == 0
            tags.add(int(got[0][1]))
        # one phase set whose votes lie in different steps, and a set per variant
        for sets in (np.zeros(n, np.int32), np.arange(n, dtype=np.int32)):
            both(ctx, host_ctx, rs, dict(v, phase_set=sets))
    assert tags == {1, 2}


def test_a_query_of_221_bases_in_one_context(ctx, host_ctx):
    ref = hm.periodic_ref(600)
    rs = hm.hand_read("30M200I30M", inserted="ACCGT" * 40, ref=ref)
    v = hm.variants_of([121, 130, 131], "AAA", [1, 2, 1], [1, 1, 2])
    got = both(ctx, host_ctx, rs, v)
    want = hm.haplotag(rs, v, ref, 0)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and len(got[1]) == 3


@pytest.mark.parametrize("length", (10, 11, 20, 21))
def test_contexts_at_both_ends_of_short_reads(ctx, host_ctx, length):
    ref = hm.periodic_ref()
    pos = np.arange(95, 100 + length + 5)
    alt = np.frombuffer(b"ACGT", np.uint8)[(pos + 2) % 4]
    v = {"pos": pos, "alt_base": alt, "genotype": np.ones(len(pos), np.uint8), "phase_set": (pos // 7).astype(np.int32)}
    carry = {int(p): chr(a) for p, a in zip(pos[::2], alt[::2])}
    reads = [(100, 0, 60, f"{length}M", "".join(carry.get(p, "ACGT"[p % 4]) for p in range(100, 100 + length))),
             (100, 0, 60, f"3S{length}M2S", "TTT" + "".join(carry.get(p, "ACGT"[p % 4]) for p in range(100, 100 + length)) + "TT")]
    rs = syn.pack_reads(reads)
    rs.update(ref_bytes=ref, ref_first=0)
    got = both(ctx, host_ctx, rs, v)
    want = hm.haplotag(rs, v, ref, 0)
    assert got[2].tolist() == [0, length, 2 * length] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    # 10 bases: no context on either side of any variant, so no allele
    assert (length > 10) == bool(got[1].any())


def test_buffer_reuse_large_small_large(ctx, host_ctx):
    large, small = ROUGH["d_i"], ROUGH["long_insertions_n_ops"]
    first = both(ctx, host_ctx, *large)
    both(ctx, host_ctx, *small)
    again = both(ctx, host_ctx, *large)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # a plain c3_fa_reads in between leaves the held tags alone
    rs, v = large
    ex = syn.make_read_extras(rs, 5)
    ctx.run(rs, ex, np.arange(2020, 2100, 7), rs["ref_bytes"], rs["ref_first"])
    assert np.array_equal(ctx.haplotag_pairs()[0], first[0]) and np.array_equal(ctx.haplotag_pairs()[1], first[1])


KEYS = ("rows", "counts", "depths", "text")


def chain(c, rs, ex, v, centres, path, **cfg):
    r = c.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], path=path, variants=v, **cfg).fetch()
    return r, c.haplotag_pairs()


def test_phased_chain_against_the_host_chain(ctx, host_ctx):
    for k, rs, v, hap, alleles, _ in golden_sets():
        ex = {name: a for name, a in syn.make_read_extras(rs, 80 + k, duplicate_names=0.03).items() if name != "haplotype"}
        centres = np.arange(2018, 2018 + 110, 2)
        for cfg in (dict(matrix_depth=89, seed=k), dict(matrix_depth=55, seed=3, lds_reads=8)):
            want, want_tags = chain(host_ctx, rs, ex, v, centres, "host", **cfg)
            got, got_tags = chain(ctx, rs, ex, v, centres, "device", **cfg)
            for key in KEYS:
                assert np.array_equal(got[key], want[key]) if key != "text" else got[key] == want[key], (k, key)
            assert all(np.array_equal(a, b) for a, b in zip(got_tags, want_tags)) and np.array_equal(got_tags[0], hap)
            s = ctx.stats()
            assert s["fell_back"] == ("lds_reads" in cfg) and s["on_host"] == ("lds_reads" in cfg) and not ctx.haplotag_stats()["on_host"]
            assert got["counts"].max() > 20 and set(np.unique(got["rows"][:, :, 7])) >= {30, 90}
        # the chain is c3_fa_reads fed the tags
        plain = ctx.run(rs, dict(ex, haplotype=hap), centres, rs["ref_bytes"], rs["ref_first"], matrix_depth=89, seed=k).fetch()
        assert np.array_equal(plain["rows"], chain(ctx, rs, ex, v, centres, "device", matrix_depth=89, seed=k)[0]["rows"])
    # no candidates: tags only; a refusal leaves nothing behind
    r, tags = chain(ctx, rs, ex, v, [], "device")
    assert len(r["counts"]) == 0 and np.array_equal(tags[0], hap) and np.array_equal(tags[1], alleles)
    with pytest.raises(_lib.C3Error, match="genotype 3"):
        chain(ctx, rs, ex, dict(v, genotype=np.full(len(v["pos"]), 3, np.uint8)), centres, "device")
    assert ctx.haplotag_pairs()[0].size == 0 and ctx.sizes()[0] == 0


def test_chained_predict_after_a_phased_run(ctx):
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, 8, True, seed=41)
    m = Clair3_F(add_indel_length=True, predict=True, input_channels=8)
    m.set_geometry(55, 33)
    m = m.to("cuda:0")
    m.eval()
    m.decode_columns(True)
    m.load_state_dict(sd)
    _, rs, v, hap, _, _ = next(iter(golden_sets()))
    ex = {name: a for name, a in syn.make_read_extras(rs, 90).items() if name != "haplotype"}
    centres = np.arange(2020, 2120, 2)
    r = ctx.run(rs, ex, centres, rs["ref_bytes"], rs["ref_first"], variants=v, matrix_depth=55, seed=2).fetch()
    assert not ctx.stats()["on_host"] and r["counts"].max() > 20
    want = m.predict_rows(r["rows"], r["counts"])
    got = m.predict_reads(ctx)
    assert got.shape == want.shape == (len(centres), m.row_size) and np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ctx.haplotag_pairs()[0], hap)
