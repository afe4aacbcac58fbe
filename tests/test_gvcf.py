"""gVCF mode without a GPU (csrc/c3_gvcf.h, clair3_amd/gvcf.py): the site record, the sequential rule and the text in C against what the
reference's own variantInfoCalculator wrote (tests/golden/gvcf_blocks.npz), the numpy mirror against the C path, the counts of the region
form, refused inputs, the max_blocks protocol, the record size, and the drop-in against the reference's class."""
import ctypes as C
import re

import numpy as np
import pytest

from clair3_amd import _lib, gvcf
from clair3_amd import synthetic as syn
from tests import gvcf_cases as gc
from tests import util


def test_fixture_conditions():
    """what make_golden_gvcf.py asserts when it writes the fixture, on the committed file: every case of the rule occurs at least 8 times"""
    mk = gc.generator()
    counts = mk.conditions(gc.fixture())
    low = {k: v for k, v in counts.items() if v < mk.MIN_PER_CONDITION}
    assert not low, f"conditions that occur fewer than {mk.MIN_PER_CONDITION} times: {low}"
    n_ref, n_total, ref = mk.make_region()  # (recipe drift: the committed inputs are what the generator makes today)
    z = gc.fixture()
    assert (n_ref == z["b_n_ref"]).all() and (n_total == z["b_n_total"]).all() and ref == z["b_ref"].tobytes()


def test_block_record_size():
    assert C.sizeof(_lib.GvcfBlock) == 48 == gvcf.BLOCK_DTYPE.itemsize
    header = open(util.ROOT + "/include/c3hip.h").read()
    assert re.search(r"typedef struct c3_gvcf_block \{ /\* 48 bytes \*/", header)
    for name, (dt, off) in gvcf.BLOCK_DTYPE.fields.items():
        assert getattr(_lib.GvcfBlock, name).offset == off, name


@pytest.mark.parametrize("t", [0, 1])
def test_site_table_equals_the_reference(t):
    z = gc.fixture()
    base_err, bin_size, depth = z["meta"]["tables"][t]
    want = z[f"a_table{t}"]
    got = gvcf.site_table(depth, base_err, bin_size)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} pairs differ, first index {bad[0]}: {got[bad[0]]} against {want[bad[0]]}"
    # c3_gvcf_site itself on every pair, the four bases in turn; a base outside ACGT on every pair keeps validPL and nothing else
    L = _lib.lib()
    cfg = _lib.GvcfConfig(base_err, bin_size, 0)
    six = (C.c_int32 * 6)()
    i = 0
    for nt in range(depth + 1):
        for nr in range(nt + 1):
            assert L.c3_gvcf_site(C.byref(cfg), nr, nt, b"ACGT"[i & 3], six) == 0
            assert tuple(six) == tuple(want[i]), (nr, nt)
            assert L.c3_gvcf_site(C.byref(cfg), nr, nt, b"NaR*"[i & 3], six) == 0
            assert tuple(six) == (1, 1, want[i][2], 0, 0, 0), (nr, nt)
            i += 1
    assert i == len(want)
    # the numpy mirror on a sample of the pairs
    rng = np.random.default_rng(5)
    for nt in np.r_[0, 1, depth, rng.integers(0, depth + 1, size=40)]:
        nr = int(rng.integers(0, nt + 1))
        row = tuple(want[nt * (nt + 1) // 2 + nr])
        assert gvcf.site(nr, nt, "C", base_err, bin_size) == row
        g, b, v, pl = syn.gvcf_site(nr, int(nt), base_err, bin_size)
        assert (g, b, int(v)) + pl == row


def test_site_outside_acgt():
    for byte in "NnaRY*":
        gq, binned, valid, *pl = gvcf.site(2, 20, byte)
        assert (gq, binned, pl) == (1, 1, [0, 0, 0]) and valid == gvcf.site(2, 20, "A")[2] == 0


def test_f_host_and_numpy_agree():
    """f(x) = ceil(x + x * 0.3) in double over every depth, through one-block / two-block answers of the C rule"""
    x = np.arange(0, 65536, dtype=np.int64)
    f = syn.gvcf_f(x)
    assert f[10] == 13 and f[30] == 39 and f[0] == 0
    rng = np.random.default_rng(1)
    for d in np.r_[20, 30, 65535 // 2, rng.integers(20, 50000, size=60)]:  # (all-reference sites from depth 20 on share gq 50)
        hi = min(int(f[d]), 65535)
        for top, blocks in ((hi, 1), (hi + 1, 2)):
            if top > 65535:
                continue
            got = gvcf.blocks_host([d, top], [d, top], b"AA", 1)
            assert len(got) == blocks, (d, top)


@pytest.mark.parametrize("bp", [False, True])
def test_host_rule_and_text_equal_the_reference(bp):
    z = gc.fixture()
    n_ref, n_total, ref, first = gc.region_b()
    b = gvcf.blocks_host(n_ref, n_total, ref, first, bp_resolution=bp)
    text = gvcf.text(b, z["meta"]["ctg"], z["meta"]["contig_len"], first, len(n_total))
    assert text == z["b_text_bp" if bp else "b_text"].tobytes()
    if not bp:
        want = z["b_records"]
        assert len(b) == len(want)
        for f in gc.LINE_FIELDS:
            assert (b[f] == want[f]).all(), f


def record_lines(b, ctg, contig_len):
    """the lines of write_to_gvcf (preprocess/utils.py:608-622) for records, formatted here"""
    out = []
    for r in b:
        end = contig_len if r["end"] == contig_len - 1 else r["end"]
        out.append(f"{ctg}\t{r['pos']}\t.\t{chr(r['ref'])}\t<NON_REF>\t0\t.\tEND={end}\tGT:GQ:MIN_DP:PL\t{'0/0' if r['gt'] else './.'}:{r['gq']}:{r['min_dp']}:"
                   f"{r['pl'][0]},{r['pl'][1]},{r['pl'][2]}\n")
    return "".join(out).encode()


def test_contig_end_and_empty_region():
    z = gc.fixture()
    n_ref, n_total, ref, _ = gc.region_b()
    ctg, clen = z["meta"]["ctg"], z["meta"]["contig_len"]
    k, first = int(z["c_end_sites"]), int(z["c_end_first"])
    b = gvcf.blocks_host(n_ref[:k], n_total[:k], ref[:k], first)
    assert b["end"][-1] == clen - 1
    assert gvcf.text(b, ctg, clen, first, k) == z["c_end_text"].tobytes() == record_lines(b, ctg, clen)
    assert gvcf.text(b, ctg, 0, first, k) != z["c_end_text"].tobytes()  # (a contig the header does not know: END as it is)
    k, first = int(z["c_empty_sites"]), int(z["c_empty_first"])
    ref = ref[600:600 + k]  # (a stretch with N and lower-case bases: depth-0 sites then make several records)
    b = gvcf.blocks_host(np.zeros(k, np.int64), np.zeros(k, np.int64), ref, first)
    assert len(b) > 1 and (b["max_dp"] == 0).all()
    assert gvcf.text(b, ctg, clen, first, k) == z["c_empty_text"].tobytes()
    # n_sites = 0: the records as they are -- what make_gvcf_online itself writes for depth-0 sites, not the empty-pileup line
    assert gvcf.text(b, ctg, clen, first, 0) == record_lines(b, ctg, clen)
    assert len(gvcf.text(b, ctg, clen, first, 0).splitlines()) == len(b) > 1
    assert gvcf.text(b[:0], ctg, clen, first, k) == b""


@pytest.mark.parametrize("bp", [False, True])
def test_numpy_mirror_agrees_with_c(bp):
    n_ref, n_total, ref, first = gc.region_b()
    gc.assert_same_records(syn.gvcf_blocks(n_ref, n_total, ref, first, bp_resolution=bp), gvcf.blocks_host(n_ref, n_total, ref, first, bp_resolution=bp), "fixture (b)")
    for seed in range(6):
        a, t, r = gc.second_region(300 + seed, seed)
        for cfg in ((0.001, 5), (0.01, 10)):
            gc.assert_same_records(syn.gvcf_blocks(a, t, r, 7, cfg[0], cfg[1], bp), gvcf.blocks_host(a, t, r, 7, cfg[0], cfg[1], bp), f"seed {seed}")
    assert len(syn.gvcf_blocks([], [], b"")) == 0 == len(gvcf.blocks_host([], [], b""))


def test_dtypes_give_one_answer():
    n_ref, n_total, ref, first = gc.region_b()
    a = gvcf.blocks_host(n_ref.astype(np.int32), n_total.astype(np.int32), ref, first)
    gc.assert_same_records(a, gvcf.blocks_host(n_ref, n_total, ref.tobytes(), first))


def test_region_counts_against_a_direct_derivation():
    """a synthetic region: the reference base is the one channel pair the producer negated; the counts from how the region was drawn"""
    region, major = syn.make_pileup_region(900, n_chunks=4, seed=3, empty_fraction=0.05, depth=40)
    r = np.argmin(region[:, 0:4] + region[:, 9:13], axis=1)  # (an all-zero column: 0, as base2index gives for a base outside CGT)
    ref_cols = np.frombuffer(b"ACGT", np.uint8)[r]
    first_major, n_sites = int(major[0]) - 3, int(major[-1] - major[0]) + 9
    ref = np.full(n_sites, ord("A"), np.uint8)
    ref[major - first_major] = ref_cols
    ref[::17] |= 0x20  # lower case reads the same channels
    n_ref, n_total = syn.gvcf_region_counts(region, major, ref, first_major, n_sites)
    # direct: the bases of both strands, the reference's own count from the negated sums
    pair = (region[:, 0:4] + region[:, 9:13]).astype(np.int64)
    rows = np.arange(len(region))
    strand_sum = -pair[rows, r]
    others = pair.sum(axis=1) - pair[rows, r]
    want_ref = strand_sum - others
    alt = pair.copy()
    alt[rows, r] = 0
    run_max = np.maximum.accumulate(alt, axis=1)
    rises = np.c_[alt[:, 0] > 0, alt[:, 1:] > run_max[:, :-1]]
    want_total = want_ref + (run_max * rises).sum(axis=1) + region[:, [4, 13, 6, 15]].sum(axis=1)
    site = major - first_major
    assert (n_ref[site] == want_ref).all() and (n_total[site] == want_total).all()
    missing = np.setdiff1d(np.arange(n_sites), site)
    assert missing.size > 0 and (n_ref[missing] == 0).all() and (n_total[missing] == 0).all()
    assert (want_total != want_ref + alt.sum(axis=1) + region[:, [4, 13, 6, 15]].sum(axis=1)).any()  # (the running maximum is not the plain sum)
    gc.assert_same_records(gvcf.blocks_from_region(region, major, ref, first_major, n_sites, 11, path="host"), gvcf.blocks_host(n_ref, n_total, ref, 11))


def test_refused_inputs():
    L = _lib.lib()
    cfg = _lib.GvcfConfig(0.001, 5, 0)
    out = np.zeros(8, gvcf.BLOCK_DTYPE)
    n = C.c_int64(0)

    def host(n_ref, n_total, ref=b"AAAA", dtype=_lib.DTYPE_I64, cfg=cfg):
        a, t = np.asarray(n_ref, np.int64), np.asarray(n_total, np.int64)
        return L.c3_gvcf_blocks_host(C.byref(cfg), a.ctypes.data, t.ctypes.data, dtype, ref, len(t), 1, out.ctypes.data, len(out), C.byref(n))

    assert host([30, 31, 32, 33], [30, 31, 32, 33]) == 0 and n.value == 1
    for bad_ref, bad_total, word in (([1, 3, 3, 4], [1, 2, 3, 4], "n_ref > n_total"), ([1, -1, 3, 4], [1, 2, 3, 4], "negative"),
                                     ([1, 2, 3, 4], [1, 2, -3, 4], "negative"), ([1, 2, 3, 4], [1, 2, 3, 65536], "65535")):
        assert host(bad_ref, bad_total) == 1 and word in _lib.last_error()
    assert host([1, 2, 3, 65535], [1, 2, 3, 65535]) == 0
    assert host([1], [1], dtype=_lib.DTYPE_I8) == 1 and "int32 or int64" in _lib.last_error()
    a = np.ones(4, np.int64)
    assert L.c3_gvcf_blocks_host(C.byref(cfg), None, a.ctypes.data, _lib.DTYPE_I64, b"AAAA", 4, 1, out.ctypes.data, 8, C.byref(n)) == 1
    assert L.c3_gvcf_blocks_host(C.byref(cfg), a.ctypes.data, a.ctypes.data, _lib.DTYPE_I64, None, 4, 1, out.ctypes.data, 8, C.byref(n)) == 1
    assert L.c3_gvcf_blocks_host(C.byref(cfg), a.ctypes.data, a.ctypes.data, _lib.DTYPE_I64, b"AAAA", 4, 1, None, 8, C.byref(n)) == 1
    assert L.c3_gvcf_blocks_host(C.byref(cfg), a.ctypes.data, a.ctypes.data, _lib.DTYPE_I64, b"AAAA", 4, 1, out.ctypes.data, 8, None) == 1
    assert L.c3_gvcf_blocks_host(None, a.ctypes.data, a.ctypes.data, _lib.DTYPE_I64, b"AAAA", 4, 1, out.ctypes.data, 8, C.byref(n)) == 1
    assert host([1], [1], cfg=_lib.GvcfConfig(0.0, 5, 0)) == 1 and host([1], [1], cfg=_lib.GvcfConfig(0.001, 0, 0)) == 1
    six = (C.c_int32 * 6)()
    assert L.c3_gvcf_site(C.byref(cfg), 3, 2, ord("A"), six) == 1 and L.c3_gvcf_site(C.byref(cfg), 1, 2, ord("A"), None) == 1
    assert L.c3_gvcf_destroy(None) == 0
    assert L.c3_gvcf_blocks_counts(None, a.ctypes.data, a.ctypes.data, _lib.DTYPE_I64, b"AAAA", 4, 1, out.ctypes.data, 8, C.byref(n)) == 1
    with pytest.raises(ValueError):
        syn.gvcf_blocks([3], [2], b"A")


def test_max_blocks_protocol():
    n_ref, n_total, ref, first = gc.region_b()
    full = gvcf.blocks_host(n_ref, n_total, ref, first)
    L = _lib.lib()
    cfg = _lib.GvcfConfig(0.001, 5, 0)
    n = C.c_int64(0)
    for cap in (0, 1, len(full) - 1, len(full), len(full) + 5):
        out = np.zeros(len(full) + 8, gvcf.BLOCK_DTYPE)
        out["reserved"] = -7  # (what the library must leave alone beyond max_blocks)
        rc = L.c3_gvcf_blocks_host(C.byref(cfg), n_ref.ctypes.data, n_total.ctypes.data, _lib.DTYPE_I64, ref.ctypes.data, len(n_total), first,
                                   out.ctypes.data if cap else None, cap, C.byref(n))
        assert n.value == len(full)
        assert rc == (_lib.GVCF_MORE if cap < len(full) else 0)
        k = min(cap, len(full))
        gc.assert_same_records(out[:k], full[:k], f"max_blocks {cap}")
        assert (out["reserved"][k:] == -7).all()
    assert _lib.GVCF_MORE not in (0, 1)
    with pytest.raises(_lib.C3Error, match="do not fit"):
        gvcf.blocks_host(n_ref, n_total, ref, first, max_blocks=3)
    need = C.c_int64(0)
    buf = C.create_string_buffer(16)
    assert L.c3_gvcf_text(full.ctypes.data, len(full), b"chrG", 0, first, 0, buf, 16, C.byref(need)) == _lib.GVCF_MORE and need.value > 16
    assert buf.raw == b"\0" * 16


def test_command_line(tmp_path):
    z = gc.fixture()
    n_ref, n_total, ref, first = gc.region_b()
    ctg, clen = z["meta"]["ctg"], z["meta"]["contig_len"]
    contig = bytearray(b"A" * clen)
    contig[first - 1:first - 1 + len(ref)] = ref.tobytes()
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b">other\nACGT\n>" + ctg.encode() + b" some text\n" + b"\n".join(bytes(contig[i:i + 60]) for i in range(0, clen, 60)) + b"\n>next\nAC\n")
    np.savez(tmp_path / "counts.npz", n_ref=n_ref, n_total=n_total, first_pos=first)
    assert gvcf.main(["--counts", str(tmp_path / "counts.npz"), "--ref_fn", str(fa), "--ctgName", ctg, "--output_fn", str(tmp_path / "out.gvcf"),
                      "--path", "host"]) == 0
    assert (tmp_path / "out.gvcf").read_bytes() == z["b_text"].tobytes()
    # an all-zero chunk: the empty-pileup line; with coverage only at ctgEnd (read by the producer's check, not walked): depth-0 records
    k, f0 = int(z["c_empty_sites"]), int(z["c_empty_first"])
    zero = np.zeros(k + 1, np.int64)
    base_args = ["--ref_fn", str(fa), "--ctgName", ctg, "--output_fn", str(tmp_path / "out.gvcf"), "--path", "host", "--with_ctg_end", "--ctgStart", str(f0)]
    np.savez(tmp_path / "zero.npz", n_ref=zero, n_total=zero)
    assert gvcf.main(["--counts", str(tmp_path / "zero.npz")] + base_args) == 0
    contig_a = (tmp_path / "out.gvcf").read_bytes()
    covered = zero.copy()
    covered[-1] = 9
    np.savez(tmp_path / "last.npz", n_ref=covered, n_total=covered)
    assert gvcf.main(["--counts", str(tmp_path / "last.npz")] + base_args) == 0
    b = gvcf.blocks_host(zero[:k], zero[:k], bytes(contig[f0 - 1:f0 - 1 + k]), f0)
    assert (tmp_path / "out.gvcf").read_bytes() == record_lines(b, ctg, clen) != contig_a
    assert contig_a.count(b"\n") == 1 and contig_a.endswith(f"END={f0 + k}\tGT:GQ:MIN_DP:PL\t./.:1:0:0,0,0\n".encode())


def test_install_against_the_reference_class(tmp_path, monkeypatch):
    """the rebinding of install() against the reference's own class on fixture (b), host path; skipped without the reference"""
    monkeypatch.setenv("C3HIP_GVCF", "host")
    with gc.reference_utils() as U:
        if U is None:
            pytest.skip("the reference is not staged")
        z = gc.fixture()
        n_ref, n_total, ref, first = gc.region_b()
        base = U.variantInfoCalculator
        for bp in (False, True):
            want = gc.run_producer_loop(base, tmp_path, n_ref, n_total, ref, first, bp)
            assert want.encode() == z["b_text_bp" if bp else "b_text"].tobytes()
            cls = gvcf.install()
            try:
                assert U.variantInfoCalculator is cls and issubclass(cls, base) and gvcf.install() is cls
                got = gc.run_producer_loop(cls, tmp_path, n_ref, n_total, ref, first, bp)
            finally:
                gvcf.uninstall()
            assert U.variantInfoCalculator is base
            assert got == want
        # a batch whose sites are all depth 0 (a chunk covered only at its last, unwalked site; a flush by push_current): the reference
        # writes depth-0 block records for it, not the empty-pileup line, and so does the drop-in
        k = 300
        zero = np.zeros(k, np.int64)
        ref = ref[600:600 + k]  # (a stretch with N and lower-case bases)
        want = gc.run_producer_loop(base, tmp_path, zero, zero, ref, first)
        assert len(want.splitlines()) > 1 and "0/0:1:0:" in want
        cls = gvcf.install()
        try:
            got = gc.run_producer_loop(cls, tmp_path, zero, zero, ref, first)
            # ... and flushed in the middle by push_current, with a change of contig name behind it
            c = gc.make_calculator(cls, tmp_path)
            for i in range(k):
                c.make_gvcf_online({"chr": z["meta"]["ctg"], "pos": first + i, "ref": chr(ref[i]), "n_total": 0, "n_ref": 0})
                if i == 100:
                    c.make_gvcf_online(None, push_current=True)
            c.make_gvcf_online({"chr": "other", "pos": 5, "ref": "A", "n_total": 0, "n_ref": 0})
            c.close_vcf_writer()
            got_split = c.vcf_writer.getvalue()
        finally:
            gvcf.uninstall()
        assert got == want
        c = gc.make_calculator(base, tmp_path)
        for i in range(k):
            c.make_gvcf_online({"chr": z["meta"]["ctg"], "pos": first + i, "ref": chr(ref[i]), "n_total": 0, "n_ref": 0})
            if i == 100:
                c.make_gvcf_online(None, push_current=True)
        c.make_gvcf_online({"chr": "other", "pos": 5, "ref": "A", "n_total": 0, "n_ref": 0})
        c.make_gvcf_online(None, push_current=True)
        assert got_split == c.vcf_writer.getvalue()
        # write_empty_pileup stays the reference's
        c_text = z["c_empty_text"].tobytes().decode()
        cls = gvcf.install()
        try:
            import io
            import sys
            keep, sys.stdout = sys.stdout, io.StringIO()
            try:
                c = cls("PIPE", str(tmp_path / "ref.fa"), 0.001, 5, z["meta"]["ctg"], sample_name="S")
            finally:
                sys.stdout = keep
            c.vcf_writer = io.StringIO()
            c.write_empty_pileup(z["meta"]["ctg"], int(z["c_empty_first"]), int(z["c_empty_first"]) + int(z["c_empty_sites"]))
            assert c.vcf_writer.getvalue() == c_text
        finally:
            gvcf.uninstall()
