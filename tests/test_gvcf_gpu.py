"""gVCF mode on the device (csrc/c3_gvcf.h): both device entries and both dtypes against the sequential C rule and the reference's lines, every
tile and wave boundary on every kind of break, the shapes where the hierarchy can go wrong, table growth, two contexts, the max_blocks
protocol, the condition against serial or quadratic behaviour, and the drop-in on the device path."""
import ctypes as C
import time

import numpy as np
import pytest

from clair3_amd import _lib, gvcf
from clair3_amd import synthetic as syn
from tests import gvcf_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with gvcf.Context() as c:
        yield c


def hierarchy_sites():
    """more than twice the span of the top level, and no multiple of a tile"""
    L = _lib.lib()
    tile, span = L.c3_gvcf_tile_sites(), L.c3_gvcf_top_span()
    n = 2 * span + 3 * tile + 77
    assert n > 2 * span and n % tile and span >= 128 * tile and n > 300_000
    return n


def region_for(n_ref, n_total, ref, seed=0):
    """a region matrix whose counts are (n_ref, n_total): reference channel pair negated, the rest on A/C/G/T of both strands and the
    indel channels; some sites have no column"""
    rng = np.random.default_rng(seed)
    n = len(n_total)
    up = ref & 0xDF
    r = np.select([up == ord("C"), up == ord("G"), up == ord("T")], [1, 2, 3], 0)
    rest = (n_total - n_ref).astype(np.int64)
    m = np.zeros((n, 18), np.int64)
    fwd_ref = rng.integers(0, n_ref + 1)
    alt = rng.integers(0, rest + 1)          # one alternative base (the running maximum of one base is its count)
    k = (r + 1 + rng.integers(0, 3, size=n)) % 4
    ins = rng.integers(0, rest - alt + 1)
    dele = rest - alt - ins
    rows = np.arange(n)
    alt_fwd = rng.integers(0, alt + 1)
    m[rows, k], m[rows, 9 + k] = alt_fwd, alt - alt_fwd
    m[rows, r], m[rows, 9 + r] = -(fwd_ref + alt_fwd), -((n_ref - fwd_ref) + (alt - alt_fwd))
    m[:, 4], m[:, 13] = ins // 2, ins - ins // 2
    m[:, 6], m[:, 15] = dele // 2, dele - dele // 2
    m[:, [5, 7, 8, 14, 16, 17]] = rng.integers(0, 5, size=(n, 6))  # channels the counts do not read
    keep = ~((n_total == 0) & (rng.random(n) < 0.5))  # a site without a column is 0 / 0
    return m[keep], np.flatnonzero(keep).astype(np.int64)


@pytest.mark.parametrize("bp", [False, True])
def test_fixture_through_both_entries_and_dtypes(ctx, bp):
    z = gc.fixture()
    n_ref, n_total, ref, first = gc.region_b()
    ctg, clen = z["meta"]["ctg"], z["meta"]["contig_len"]
    with gvcf.Context(bp_resolution=bp) as c:
        want = gvcf.blocks_host(n_ref, n_total, ref, first, bp_resolution=bp)
        region, cols = region_for(n_ref, n_total, ref)
        assert (np.array(syn.gvcf_region_counts(region, cols + 900, ref, 900, len(ref))) == np.array([n_ref, n_total])).all()
        for dt in (np.int32, np.int64):
            got = c.blocks_from_counts(n_ref.astype(dt), n_total.astype(dt), ref, first)
            gc.assert_same_records(got, want, f"counts {dt.__name__}")
            assert gvcf.text(got, ctg, clen, first, len(ref)) == z["b_text_bp" if bp else "b_text"].tobytes()
            got = c.blocks_from_region(region.astype(dt), cols + 900, ref, 900, len(ref), first)
            gc.assert_same_records(got, want, f"region {dt.__name__}")
            assert gvcf.text(got, ctg, clen, first, len(ref)) == z["b_text_bp" if bp else "b_text"].tobytes()


def through_every_entry_and_dtype(c, n_ref, n_total, ref, first, seed):
    """the records of both device entries for int32 and int64 inputs, each compared with c3_gvcf_blocks_host; one of them is returned"""
    want = gvcf.blocks_host(n_ref, n_total, ref, first)
    region, cols = region_for(n_ref, n_total, ref, seed)
    assert (np.array(syn.gvcf_region_counts(region, cols + 40, ref, 40, len(ref))) == np.array([n_ref, n_total])).all()
    for dt in (np.int32, np.int64):
        gc.assert_same_records(c.blocks_from_counts(n_ref.astype(dt), n_total.astype(dt), ref, first), want, f"counts {dt.__name__}")
        gc.assert_same_records(c.blocks_from_region(region.astype(dt), cols + 40, ref, 40, len(ref), first), want, f"region {dt.__name__}")
    return want, region, cols


def test_contig_end_and_empty_region(ctx):
    """fixture (c) through both entries and both dtypes: records identical to the C rule's, text identical to the golden"""
    z = gc.fixture()
    n_ref, n_total, ref, _ = gc.region_b()
    ctg, clen = z["meta"]["ctg"], z["meta"]["contig_len"]
    k, first = int(z["c_end_sites"]), int(z["c_end_first"])
    want, _, _ = through_every_entry_and_dtype(ctx, n_ref[:k], n_total[:k], ref[:k], first, 1)
    assert want["end"][-1] == clen - 1 and gvcf.text(want, ctg, clen, first, k) == z["c_end_text"].tobytes()
    # the all-zero region, over a stretch with N and lower-case bases: columns with zero counts for about half of the sites, none for the rest
    k, first = int(z["c_empty_sites"]), int(z["c_empty_first"])
    zero, zref = np.zeros(k, np.int64), ref[600:600 + k]
    want, region, cols = through_every_entry_and_dtype(ctx, zero, zero, zref, first, 2)
    assert 0 < len(cols) < k and len(want) > 1
    assert gvcf.text(want, ctg, clen, first, k) == z["c_empty_text"].tobytes()
    assert len(gvcf.text(want, ctg, clen, first, 0).splitlines()) == len(want)  # (n_sites = 0: the records as they are)
    for dt in (np.int32, np.int64):  # no column at all
        got = ctx.blocks_from_region(np.zeros((0, 18), dt), np.zeros(0, np.int64), zref, 0, k, first)
        gc.assert_same_records(got, want, f"no columns {dt.__name__}")
    assert len(ctx.blocks_from_counts(zero[:0], zero[:0], b"", 1)) == 0  # (n_sites = 0: nothing is launched)


def test_every_boundary_on_every_kind_of_break(ctx):
    """0 .. 69 sites of a second region in front of fixture (b): tile and wave boundaries move over every break"""
    n_ref, n_total, ref, first = gc.region_b()
    a, t, r = gc.second_region(69)
    for k in range(70):
        nr, nt, rb = np.r_[a[:k], n_ref], np.r_[t[:k], n_total], np.r_[r[:k], ref]
        gc.assert_same_records(ctx.blocks_from_counts(nr, nt, rb, first), gvcf.blocks_host(nr, nt, rb, first), f"{k} sites in front")


SHAPES = ("zero", "constant", "alternating", "ramp", "poisson", "one_deep")


def shape(name, n):
    rng = np.random.default_rng(11)
    if name == "zero":
        t = np.zeros(n, np.int64)
    elif name == "constant":
        t = np.full(n, 30, np.int64)
    elif name == "alternating":
        t = np.where(np.arange(n) % 2 == 0, 10, 14).astype(np.int64)  # f(10) = 13: every site is a block
    elif name == "ramp":
        t = 20 + np.arange(n, dtype=np.int64) // 4096
    elif name == "poisson":
        t = rng.poisson(30, size=n).astype(np.int64)
    else:
        t = np.full(n, 30, np.int64)
        t[n // 2 + 5] = 65535
    return t, t.copy(), np.full(n, ord("A"), np.uint8)


@pytest.mark.parametrize("name", SHAPES)
def test_shapes_where_the_hierarchy_can_go_wrong(ctx, name):
    n = hierarchy_sites()
    n_ref, n_total, ref = shape(name, n)
    want = gvcf.blocks_host(n_ref, n_total, ref, 1)
    got = ctx.blocks_from_counts(n_ref, n_total, ref, 1)
    gc.assert_same_records(got, want, name)
    if name == "zero":
        assert len(got) == 1 and got["end"][0] == n
    if name == "alternating":
        assert len(got) == n  # the capacity edge
    if name == "one_deep":
        assert got["max_dp"].max() == 65535 and len(got) == 3


def test_table_growth(ctx):
    with gvcf.Context() as c:
        for depth, seed in ((40, 1), (300, 2), (25, 3), (_lib.lib().c3_gvcf_table_depth() + 500, 4)):
            rng = np.random.default_rng(seed)
            t = rng.integers(0, depth + 1, size=5000)
            t[17] = depth
            a = rng.binomial(t, 0.9)
            ref = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=len(t))
            gc.assert_same_records(c.blocks_from_counts(a, t, ref, 1), gvcf.blocks_host(a, t, ref, 1), f"depth {depth}")


def test_two_contexts_interleaved():
    n_ref, n_total, ref, first = gc.region_b()
    with gvcf.Context() as c1, gvcf.Context(base_err=0.01, gq_bin_size=10, bp_resolution=True) as c2:
        w1 = gvcf.blocks_host(n_ref, n_total, ref, first)
        w2 = gvcf.blocks_host(n_ref, n_total, ref, first, 0.01, 10, True)
        assert len(w1) != len(w2)
        for _ in range(3):
            gc.assert_same_records(c1.blocks_from_counts(n_ref, n_total, ref, first), w1, "first context")
            gc.assert_same_records(c2.blocks_from_counts(n_ref, n_total, ref, first), w2, "second context")


def test_max_blocks_protocol_and_refusals(ctx):
    n_ref, n_total, ref, first = gc.region_b()
    full = gvcf.blocks_host(n_ref, n_total, ref, first)
    L = _lib.lib()
    n = C.c_int64(0)
    for cap in (0, 1, len(full) - 1, len(full), len(full) + 5):
        out = np.zeros(len(full) + 8, gvcf.BLOCK_DTYPE)
        out["reserved"] = -7
        rc = L.c3_gvcf_blocks_counts(ctx.h, n_ref.ctypes.data, n_total.ctypes.data, _lib.DTYPE_I64, ref.ctypes.data, len(n_total), first,
                                     out.ctypes.data if cap else None, cap, C.byref(n))
        assert n.value == len(full) and rc == (_lib.GVCF_MORE if cap < len(full) else 0)
        k = min(cap, len(full))
        gc.assert_same_records(out[:k], full[:k], f"max_blocks {cap}")
        assert (out["reserved"][k:] == -7).all()
    for bad_ref, bad_total in ((3, 2), (-1, 2), (2, 65536)):
        a, t = n_ref.copy(), n_total.copy()
        a[4000], t[4000] = bad_ref, bad_total
        with pytest.raises(_lib.C3Error, match="refused count"):
            ctx.blocks_from_counts(a, t, ref, first)
    region, cols = region_for(n_ref, n_total, ref)
    region[100, 1 if (ref[cols[100]] & 0xDF) != ord("C") else 2] = -3  # a negative count of a base that is not the reference's
    with pytest.raises(_lib.C3Error, match="refused count"):
        ctx.blocks_from_region(region, cols, ref, 0, len(ref), first)
    with pytest.raises(_lib.C3Error, match="strictly increasing"):
        ctx.blocks_from_region(region[:4], np.array([5, 6, 6, 7]), ref, 0, len(ref), first)
    gc.assert_same_records(ctx.blocks_from_counts(n_ref, n_total, ref, first), full, "after the refusals")


def test_neither_serial_nor_quadratic(ctx):
    """One block of the whole region (depth 0) and Poisson(30) noise at the same site count: medians of 5 calls after a warm-up, host
    clock around calls that end in a device-to-host copy, must lie within 10x of each other.  A condition, not a measurement: O(n log n)
    keeps them within a small factor; a scan per block start, or one lane per run between hard breaks, is off by thousands.  Measured on one
    MI355X at 527 437 sites (profiles/gvcf_blocks.txt): 0.877 ms and 5.622 ms."""
    n = hierarchy_sites()
    times = {}
    for name in ("zero", "poisson"):
        n_ref, n_total, ref = shape(name, n)
        ctx.blocks_from_counts(n_ref, n_total, ref, 1)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            ctx.blocks_from_counts(n_ref, n_total, ref, 1)
            t.append(time.perf_counter() - t0)
        times[name] = float(np.median(t))
    print(f"gvcf blocks_from_counts, {n} sites, median of 5: depth 0 {times['zero'] * 1e3:.3f} ms, Poisson(30) {times['poisson'] * 1e3:.3f} ms")
    assert times["zero"] < 10 * times["poisson"] and times["poisson"] < 10 * times["zero"], times


def test_install_on_the_device_path(tmp_path, monkeypatch):
    """install() writes the reference class's file byte for byte with C3HIP_GVCF=device; skipped without the staged reference"""
    monkeypatch.setenv("C3HIP_GVCF", "device")
    with gc.reference_utils() as U:
        if U is None:
            pytest.skip("the reference is not staged")
        z = gc.fixture()
        n_ref, n_total, ref, first = gc.region_b()
        for bp in (False, True):
            cls = gvcf.install()
            try:
                got = gc.run_producer_loop(cls, tmp_path, n_ref, n_total, ref, first, bp)
            finally:
                gvcf.uninstall()
            assert got.encode() == z["b_text_bp" if bp else "b_text"].tobytes()
            assert got == gc.run_producer_loop(U.variantInfoCalculator, tmp_path, n_ref, n_total, ref, first, bp)
