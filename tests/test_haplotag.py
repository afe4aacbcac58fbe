"""Haplotagging the reads, the host form (csrc/c3_hap_rule.h, c3_fa_haplotag_host; no device): against the golden tags and pair alleles of the
reference's own haplotag_read (tests/golden/fa_haplotag.npz, nothing masked), against a Python mirror written from the rule's description
(tests/hap_mirror.py) on rougher generated sets, hand-worked reads, every refusal, the chained host entry against the two host calls it
stands for, the VCF reader, and the same code as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/host/haplotag_host_check.cpp).  The device form is held to the host form in tests/test_haplotag_gpu.py."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

from clair3_amd import _lib, fa_reads as fa, synthetic as syn
from tests import hap_mirror as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fa_haplotag.npz")
READ_FIELDS = ("pos", "flag", "mapq", "cigar_first", "cigar", "seq_first", "seq")


def golden_sets():
    """(k, read set, variants, hap, alleles, pair_first) of the fixture"""
    with np.load(GOLDEN) as z:
        k = 0
        while f"{k}_pos" in z.files:
            rs = {name: z[f"{k}_{name}"] for name in READ_FIELDS}
            rs.update(ref_bytes=z[f"{k}_ref_bytes"], ref_first=int(z[f"{k}_ref_first"]))
            v = {name: z[f"{k}_v_{name}"] for name in ("pos", "alt_base", "genotype", "phase_set")}
            yield k, rs, v, z[f"{k}_hap"], z[f"{k}_alleles"], z[f"{k}_pair_first"]
            k += 1


@pytest.fixture(scope="module")
def ctx():
    with fa.Context(None) as c:
        yield c


def tag(ctx, rs, v, **cfg):
    hap = ctx.haplotag(rs, v, rs["ref_bytes"], rs["ref_first"], path="host", **cfg)
    got, alleles, first = ctx.haplotag_pairs()
    assert (got == hap).all()
    return hap, alleles, first


def test_golden_tags_and_alleles(ctx):
    n_sets = 0
    for k, rs, v, hap, alleles, pair_first in golden_sets():
        got = tag(ctx, rs, v)
        assert (got[2] == pair_first).all(), k
        assert (got[1] == alleles).all(), (k, np.flatnonzero(got[1] != alleles)[:10])
        assert (got[0] == hap).all(), (k, np.flatnonzero(got[0] != hap)[:10])
        s = ctx.haplotag_stats()
        assert s["reads_hap"] == tuple(int(x) for x in np.bincount(hap, minlength=3)) and s["pairs_allele0"] == int((alleles == 0).sum())
        assert s["reads_low_mapq"] == int((rs["mapq"] < 20).sum()) and s["pairs_realigned"] == len(alleles) and s["on_host"]
        assert len(set(hap)) == 3 and len(set(alleles)) == 3
        n_sets += 1
    assert n_sets == 3


ROUGH = {name: (rs, v) for name, rs, v in hm.rough_sets()}


@pytest.mark.parametrize("name", sorted(ROUGH))
def test_python_mirror(ctx, name):
    rs, v = ROUGH[name]
    want = hm.haplotag(rs, v, rs["ref_bytes"], rs["ref_first"])
    got = tag(ctx, rs, v)
    assert len(want[1]) > 90 and (want[1] != 0).any()
    for g, w in zip(got, want):
        assert g.shape == w.shape and (g == w).all(), np.flatnonzero(g != w)[:10]


def test_min_haplotag_mq_is_a_config_field(ctx):
    rs, v = ROUGH["d_i"]
    for mq in (0, 30, 45, 61):
        want = hm.haplotag(rs, v, rs["ref_bytes"], rs["ref_first"], min_haplotag_mq=mq)
        got = tag(ctx, rs, v, min_haplotag_mq=mq)
        assert all((g == w).all() for g, w in zip(got, want))
    assert not got[0].any() and len(got[1]) == 0 and ctx.haplotag_stats()["reads_low_mapq"] == len(rs["pos"])


@pytest.mark.parametrize("case", hm.hand_cases(), ids=lambda c: c[0])
def test_reads_by_hand(ctx, case):
    _, rs, v, want = case
    hap, alleles, first = tag(ctx, rs, v)
    assert hap.tolist() == [want]
    mirror = hm.haplotag(rs, v, rs["ref_bytes"], 0)
    assert (mirror[0] == hap).all() and (mirror[1] == alleles).all() and (mirror[2] == first).all()


def test_soft_masked_reference_differs_from_every_base(ctx):
    """the reference bytes are compared as they are: with the variant's own base in lower case the read matches neither string there, and
    the alt string wins only when the read carries the alt base"""
    ref = hm.periodic_ref()
    ref[110] |= 0x20
    v = hm.variants_of([110], "T", [2], [1])
    assert tag(ctx, hm.hand_read("30M", ref=ref), v)[1].tolist() == [0]                    # 1 against 1: a tie
    assert tag(ctx, hm.hand_read("30M", carry={110: "T"}, ref=ref), v)[1].tolist() == [2]  # 1 against 0


def test_a_nul_byte_ends_the_strings(ctx):
    """C strings: a NUL byte of the reference in the left context cuts ref and alt there (alt_base lands behind the cut and is not seen)"""
    ref = hm.periodic_ref()
    ref[105] = 0
    rs, v = hm.hand_read("30M", carry={110: "T"}, ref=ref), hm.variants_of([110], "T", [2], [1])
    got = tag(ctx, rs, v)
    want = hm.haplotag(rs, v, ref, 0)
    assert got[1].tolist() == want[1].tolist() == [0]


def test_refusals(ctx):
    rs, v = ROUGH["d_i"]
    reads = fa.ReadSet.from_dict(rs)

    def refused(variants, message, ref=rs["ref_bytes"], ref_first=rs["ref_first"], reads=reads, **cfg):
        with pytest.raises(_lib.C3Error, match=message):
            ctx.haplotag(reads, variants, ref, ref_first, path="host", **cfg)
        assert ctx.haplotag_pairs()[0].size == 0  # no stale tags

    def changed(**kw):
        return fa.PhasedVariants.from_dict(dict(v, **kw))

    pos = v["pos"].copy()
    pos[[3, 4]] = pos[[4, 3]]
    refused(changed(pos=pos), "not strictly ascending at 4")
    pos = v["pos"].copy()
    pos[5] = pos[4]
    refused(changed(pos=pos), "not strictly ascending at 5")
    gt = v["genotype"].copy()
    gt[7] = 3
    refused(changed(genotype=gt), "variant 7 has the genotype 3")
    gt[7] = 0
    refused(changed(genotype=gt), "variant 7 has the genotype 0")
    null = fa.PhasedVariants.from_dict(v)
    null.c.alt_base = None
    refused(null, "a null array in the variants")
    covered = np.flatnonzero((v["pos"] >= rs["pos"].min()) & (v["pos"] < rs["pos"].max()))
    first, last = int(v["pos"][covered[0]]), int(v["pos"][covered[-1]])
    off = first - 9 - rs["ref_first"]
    refused(v, "do not cover", ref=rs["ref_bytes"][off:], ref_first=first - 9)
    refused(v, "do not cover", ref=rs["ref_bytes"][:last + 10 - rs["ref_first"]])
    refused(v, "negative min_haplotag_mq", min_haplotag_mq=-1)
    with pytest.raises(TypeError):
        ctx.haplotag(reads, v, rs["ref_bytes"], rs["ref_first"], path="host", min_mq=3)
    bad = dict(rs, cigar=rs["cigar"].copy())
    bad["cigar"][2] &= 15
    refused(v, "CIGAR op of length 0", reads=fa.ReadSet.from_dict(bad))
    with fa.Context(None) as c:
        with pytest.raises(_lib.C3Error, match="created without a device"):
            c.haplotag(reads, v, rs["ref_bytes"], rs["ref_first"], path="device")
    # c3_fa_reads with a NULL haplotype stays refused
    ex = fa.ReadExtras.from_dict({k: a for k, a in syn.make_read_extras(rs, 1).items() if k != "haplotype"})
    with pytest.raises(_lib.C3Error, match="a null array in the read set or the extras"):
        ctx.run(reads, ex, [2050], rs["ref_bytes"], rs["ref_first"], path="host")


def test_phased_host_chain_is_the_two_host_calls(ctx):
    n = 0
    for k, rs, v, hap, _, _ in golden_sets():
        ex = syn.make_read_extras(rs, 70 + k, duplicate_names=0.03)
        centres = np.arange(2020, 2020 + 100, 3)
        cfg = dict(min_mq=5, matrix_depth=55 if k == 1 else 89, seed=k)
        tags = ctx.haplotag(rs, v, rs["ref_bytes"], rs["ref_first"], path="host")
        want = ctx.run(rs, dict(ex, haplotype=tags), centres, rs["ref_bytes"], rs["ref_first"], path="host", **cfg).fetch()
        want_stats = ctx.stats()
        without = {name: a for name, a in ex.items() if name != "haplotype"}
        got = ctx.run(rs, without, centres, rs["ref_bytes"], rs["ref_first"], path="host", variants=v, **cfg).fetch()
        for name in ("rows", "counts", "depths"):
            assert got[name].shape == want[name].shape and (got[name] == want[name]).all(), (k, name)
        assert got["text"] == want["text"] and ctx.stats() == want_stats
        assert (ctx.haplotag_pairs()[0] == hap).all() and got["counts"].max() > 20
        # channel 7 carries the tags (the untagged reads of these sets are mostly those below mapq 20, which min_mq drops)
        assert set(np.unique(got["rows"][:, :, 7])) >= {30, 90}
        # the haplotype of the extras is not read
        again = ctx.run(rs, dict(ex, haplotype=np.full(len(tags), 9, np.uint8)), centres, rs["ref_bytes"], rs["ref_first"], path="host", variants=v, **cfg).fetch()
        assert (again["rows"] == want["rows"]).all()
        n += 1
    assert n == 3
    # what c3_fa_reads refuses, the chained entry refuses, and it leaves no tags behind
    with pytest.raises(_lib.C3Error, match="candidates are not strictly ascending"):
        ctx.run(rs, without, [2050, 2050], rs["ref_bytes"], rs["ref_first"], path="host", variants=v)
    assert ctx.haplotag_pairs()[0].size == 0 and ctx.sizes()[0] == 0
    with pytest.raises(_lib.C3Error, match="not strictly ascending at 1"):
        ctx.run(rs, without, [2050], rs["ref_bytes"], rs["ref_first"], path="host", variants=dict(v, pos=v["pos"][::-1].copy()))
    # no candidates: the tags are computed all the same
    ctx.run(rs, without, [], rs["ref_bytes"], rs["ref_first"], path="host", variants=v)
    assert (ctx.haplotag_pairs()[0] == hap).all() and ctx.sizes()[:2] == (0, 0)


VCF = """##fileformat=VCFv4.2
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE
chr1\t101\t.\tA\tC\t30\tPASS\t.\tGT:GQ:PS\t0|1:30:101
chr1\t150\t.\tG\tT\t30\tPASS\t.\tGT:GQ\t0/1:30
chr2\t160\t.\tG\tT\t30\tPASS\t.\tGT:GQ:PS\t1|0:30:101
chr1\t170\t.\tC\tG\t30\tPASS\t.\tGT:GQ:PS\t1|0:30:101
chr1\t180\t.\tT\tA\t30\tPASS\t.\tGT:GQ:PS\t1|1:30:171
"""


def test_phased_variants_from_vcf(tmp_path):
    plain, zipped, indel = str(tmp_path / "p.vcf"), str(tmp_path / "p.vcf.gz"), str(tmp_path / "indel.vcf")
    with open(plain, "w") as f:
        f.write(VCF)
    with gzip.open(zipped, "wt") as f:
        f.write(VCF)
    for path in (plain, zipped):
        v = fa.PhasedVariants.from_vcf(path, "chr1")
        assert v.arrays["pos"].tolist() == [100, 169, 179] and v.arrays["alt_base"].tobytes() == b"CGA"
        assert v.arrays["genotype"].tolist() == [1, 2, 2] and v.arrays["phase_set"].tolist() == [101, 101, 171] and len(v) == 3
        assert [a.dtype for a in v.arrays.values()] == [np.int64, np.uint8, np.uint8, np.int32]
    assert fa.PhasedVariants.from_vcf(plain, "chr2").arrays["pos"].tolist() == [159]
    with open(indel, "w") as f:
        f.write(VCF + "chr1\t190\t.\tTA\tT\t30\tPASS\t.\tGT:PS\t0|1:171\n")
    with pytest.raises(ValueError, match="chr1:190"):
        fa.PhasedVariants.from_vcf(indel, "chr1")
    assert len(fa.PhasedVariants.from_vcf(indel, "chr2")) == 1


def test_make_phased_variants():
    rs = ROUGH["eqx_pad"][0]
    v = syn.make_phased_variants(rs, 3, rate=0.01, hot_at=[(2050, 1, 2), (2051, 2, 1)], dense=(2000, 2030), near=[0, 5])
    assert (np.diff(v["pos"]) > 0).all() and set(v["genotype"]) == {1, 2} and len(set(v["phase_set"])) > 3
    assert v["pos"].min() >= rs["ref_first"] + 10 and v["pos"].max() + 11 <= rs["ref_first"] + len(rs["ref_bytes"])
    assert (v["alt_base"] != rs["ref_bytes"][v["pos"] - rs["ref_first"]]).all()
    at = int(np.searchsorted(v["pos"], 2050))
    assert v["pos"][at] == 2050 and v["alt_base"][at] == b"ACGT"[(b"ACGT".index(bytes([rs["ref_bytes"][2050 - rs["ref_first"]] & 0xDF])) + 2) % 4]
    dense = v["pos"][(v["pos"] >= 2000) & (v["pos"] < 2030)]
    assert np.diff(dense).max() <= 3 and rs["pos"][0] in v["pos"] and rs["pos"][5] + 10 in v["pos"]
    same = syn.make_phased_variants(rs, 3, rate=0.01, hot_at=[(2050, 1, 2), (2051, 2, 1)], dense=(2000, 2030), near=[0, 5])
    assert all((same[k] == v[k]).all() for k in v)


def _case_file(path, rs, v, mq):
    head = np.array([len(rs["pos"]), len(rs["cigar"]), len(rs["seq"]), len(v["pos"]), rs["ref_first"], len(rs["ref_bytes"]), mq], np.int64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for a, dt in ((rs["pos"], np.int64), (rs["mapq"], np.uint8), (rs["cigar_first"], np.int64), (rs["cigar"], np.uint32), (rs["seq_first"], np.int64),
                      (rs["seq"], np.uint8), (v["pos"], np.int64), (v["alt_base"], np.uint8), (v["genotype"], np.uint8), (v["phase_set"], np.int32),
                      (rs["ref_bytes"], np.uint8)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())


def test_host_form_under_sanitizers(ctx, tmp_path):
    """the rule header as a stand-alone program (its own main, no Python, no library) under -fsanitize=address,undefined: the refusals, and two
    read sets whose output must be the library's byte for byte"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "haplotag_host_check")
    # (the sanitizers' runtimes are linked statically: the program then runs whatever else the environment loads in front of it)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                          [os.path.join(ROOT, "tests", "host", "haplotag_host_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, "--errors"], env=env, capture_output=True, text=True)
    assert p.returncode == 0 and "WRONG" not in p.stdout and not p.stderr, p.stdout + p.stderr
    golden = next(iter(golden_sets()))
    for i, (rs, v, mq) in enumerate(((golden[1], golden[2], 20), ROUGH["long_insertions_n_ops"] + (20,), ROUGH["n_ops"] + (30,))):
        case, out = str(tmp_path / f"case{i}.bin"), str(tmp_path / f"out{i}.bin")
        _case_file(case, rs, v, mq)
        p = subprocess.run([exe, case, out], env=env, capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr
        want = tag(ctx, rs, v, min_haplotag_mq=mq)
        raw = open(out, "rb").read()
        n, m = np.frombuffer(raw[:16], np.int64)
        assert (n, m) == (len(want[0]), len(want[1])) and m > 90
        assert raw[16:] == want[0].tobytes() + want[1].tobytes() + want[2].tobytes()


def test_command_line_with_a_phased_vcf(ctx, tmp_path, capsys):
    _, rs, v, hap, _, _ = next(iter(golden_sets()))
    ex = {name: a for name, a in syn.make_read_extras(rs, 60).items() if name != "haplotype"}
    centres = np.arange(2030, 2090, 5)
    reads_fn, ref_fn, cand_fn, vcf_fn, out_fn = (str(tmp_path / n) for n in ("reads.npz", "ref.fa", "pos.txt", "phased.vcf", "out.npz"))
    np.savez(reads_fn, **{name: rs[name] for name in READ_FIELDS}, **ex)  # (no haplotype array)
    with open(ref_fn, "w") as f:
        f.write(">other\nACGT\n>ctg\n" + "N" * rs["ref_first"] + rs["ref_bytes"].tobytes().decode("ascii") + "\n")
    with open(cand_fn, "w") as f:
        f.write("".join(f"{c + 1}\n" for c in centres))
    with open(vcf_fn, "w") as f:
        f.write("##fileformat=VCFv4.2\n")
        for p, a, g, s in zip(v["pos"], v["alt_base"], v["genotype"], v["phase_set"]):
            f.write(f"ctg\t{p + 1}\t.\tN\t{chr(a)}\t30\tPASS\t.\tGT:PS\t{'0|1' if g == 1 else '1|0'}:{s}\n")
        f.write("other\t2\t.\tC\tG\t30\tPASS\t.\tGT:PS\t0|1:1\n")
    assert fa.main(["--reads", reads_fn, "--ref_fn", ref_fn, "--ctgName", "ctg", "--candidates", cand_fn, "--output_fn", out_fn, "--path", "host",
                    "--phased_vcf_fn", vcf_fn]) == 0
    text = capsys.readouterr().out
    want = ctx.run(rs, dict(ex, haplotype=hap), centres, rs["ref_bytes"], rs["ref_first"], path="host").fetch()
    with np.load(out_fn) as z:
        assert np.array_equal(z["rows"], want["rows"]) and np.array_equal(z["counts"], want["counts"]) and np.array_equal(z["depths"], want["depths"])
    assert text.encode() == want["text"] and want["counts"].max() > 20
