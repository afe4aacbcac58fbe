"""What tests/test_gvcf.py and tests/test_gvcf_gpu.py share: the fixture of tests/golden/make_golden_gvcf.py, seeded depth shapes, and the
reference's own variantInfoCalculator under the stand-in cffi of the generator."""
import contextlib
import functools
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

from tests import util

FIXTURE = os.path.join(util.GOLDEN, "gvcf_blocks.npz")
# what a record of the library and a record parsed from a line share (END before the contig-end rule: compare text for that)
LINE_FIELDS = ("pos", "end", "min_dp", "gq", "pl", "ref", "gt")


@functools.lru_cache(maxsize=None)
def fixture():
    z = dict(np.load(FIXTURE))
    z["meta"] = json.loads(z["meta"].tobytes().decode())
    return z


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("make_golden_gvcf", os.path.join(util.GOLDEN, "make_golden_gvcf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def region_b():
    z = fixture()
    return z["b_n_ref"], z["b_n_total"], z["b_ref"], int(z["meta"]["region_first"])


def second_region(n, seed=77):
    """a seeded region of every kind of site, to put in front of fixture (b)"""
    rng = np.random.default_rng(seed)
    total = rng.choice([0, 3, 20, 26, 30, 30, 30, 34, 39, 40], size=n).astype(np.int64)
    n_ref = np.where(rng.random(n) < 0.15, total // 8, total)
    ref = rng.choice(np.frombuffer(b"ACGTACGTACGTNNa", np.uint8), size=n)
    return n_ref, total, ref


def assert_same_records(a, b, what=""):
    assert len(a) == len(b), f"{what}: {len(a)} records against {len(b)}"
    for f in a.dtype.names:
        bad = np.flatnonzero((a[f] != b[f]).reshape(len(a), -1).any(axis=1)) if len(a) else np.zeros(0, np.int64)
        assert bad.size == 0, f"{what}: field {f} differs first at record {bad[0]}: {a[bad[0]]} against {b[bad[0]]}"


@contextlib.contextmanager
def reference_utils():
    """preprocess.utils of the staged reference with the generator's stand-in cffi in place (None where the reference is absent); the
    modules and the path entry it brought are taken out again, so that no other test sees them"""
    from oracle import stage_reference
    root = stage_reference.reference_root()
    if root is None:
        yield None
        return
    before, path = set(sys.modules), list(sys.path)
    cffi = types.ModuleType("cffi")

    class FFI:
        def cdef(self, *_a, **_k):
            pass

        def verify(self, *_a, **_k):
            raise RuntimeError("no cffi here: the Python definitions run")

    cffi.FFI = FFI
    had = sys.modules.get("cffi")
    sys.modules["cffi"] = cffi
    sys.path.insert(0, root)
    try:
        import preprocess.utils as U
        yield U
    finally:
        for name in set(sys.modules) - before:
            if name.split(".")[0] in ("preprocess", "shared", "cffi"):
                del sys.modules[name]
        if had is not None:
            sys.modules["cffi"] = had
        else:
            sys.modules.pop("cffi", None)
        sys.path[:] = path


def make_calculator(cls, tmp_path, bp=False):
    """a calculator of the class over the fixture's contig, writing into memory"""
    z = fixture()
    ctg, contig_len = z["meta"]["ctg"], z["meta"]["contig_len"]
    fa = os.path.join(str(tmp_path), "ref.fa")
    with open(fa, "w") as fh:
        fh.write(f">{ctg}\n")
    with open(fa + ".fai", "w") as fh:
        fh.write(f"{ctg}\t{contig_len}\t{len(ctg) + 2}\t60\t61\n")
    keep, sys.stdout = sys.stdout, io.StringIO()
    try:
        c = cls("PIPE", fa, 0.001, 5, ctg, bp_resolution=bp, sample_name="S")
    finally:
        sys.stdout = keep
    c.vcf_writer = io.StringIO()
    return c


def run_producer_loop(cls, tmp_path, n_ref, n_total, ref, first, bp=False):
    """the producer's loop over a calculator class (preprocess/CreateTensorPileupFromCffi.py:419-441): the text it wrote"""
    ctg = fixture()["meta"]["ctg"]
    c = make_calculator(cls, tmp_path, bp)
    for i in range(len(n_total)):
        c.make_gvcf_online({"chr": ctg, "pos": first + i, "ref": chr(ref[i]), "n_total": int(n_total[i]), "n_ref": int(n_ref[i])})
    if len(c.current_block) != 0:
        c.write_to_gvcf_batch(c.current_block, c.cur_min_DP, c.cur_raw_gq)
    if getattr(c, "_c3hip_gvcf", False):
        c.close_vcf_writer()
    return c.vcf_writer.getvalue()
