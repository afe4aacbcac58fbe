#!/usr/bin/env python3
"""Golden window selection of the REAL reference pileup producer: which candidates of a region it turns into windows, in which order, and
the int32 windows themselves (preprocess/CreateTensorPileupFromCffi.py CreateTensorPileup, the loop :343-397 behind
__enforce_pileup_chunk_contiguity :180-236), with --enable_variant_calling_at_sequence_head_and_tail off and on.

Run in the build container only (needs the reference checkout, like make_golden_deep.py):

    python tests/golden/make_golden_candidates.py

The reference's own function runs, not a transcription of it.  What it cannot have here is libclair3 (its C pileup over a BAM): a stand-in
module of that name is put into sys.modules before the reference module is imported -- an ``ffi`` with buffer / string / gc and a ``lib``
whose calculate_clair3_pileup hands back a seeded synthetic plp_data (matrix, major, minor, alt-info strings) -- next to a one-line .fai
in a temporary directory.  tests/stubs/libclair3.py is another stand-in for another purpose and is not involved.

The region (make_inputs) is made so that every case of the rule occurs, and conditions() asserts that it does -- here when the fixture is
written and again in tests/test_candidates.py on the committed file.  Stored in tests/golden/pileup_candidates.npz: matrix (int64, the
size_t matrix of plp_data), major, candidate positions and depths, and per mode the kept positions in the reference's order and the
windows it returned; seeds and digests in the file's own ``meta``.
"""
import hashlib
import json
import os
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from clair3_amd import synthetic as syn  # noqa: E402

C, T, F = syn.PILEUP_CHANNELS, syn.NO_OF_POSITIONS, 16
REGION_SEED = 9101
FIRST_POSITION = 250000
# columns of the chunks and the missing positions between them (a step of gap + 1 > 1 in major cuts the pileup)
CHUNK_LENS = (140, 1, 32, 33, 34, 35, 180, 70, 110)
GAPS = (2, 5, 40, 1, 2, 7, 60, 3)
DEEP_CHUNK = 6          # drawn at depth 400: its candidates declare depths the rescaling rule acts on
# all-zero columns, as (chunk, offset from the chunk's first column; negative: from its last)
EMPTY = ((0, 60), (6, 4), (6, -4), (6, 90), (8, 50), (8, 51))
NO_WINDOW, MAIN, EMPTY_COLUMN, HEAD, TAIL = 0, 1, 2, 3, 4
MIN_PER_STATUS = 8


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def chunk_bounds():
    """[(first column, columns, first position, last position)] of the chunks"""
    out, col, pos = [], 0, FIRST_POSITION
    for k, n in enumerate(CHUNK_LENS):
        out.append((col, n, pos, pos + n - 1))
        col += n
        pos += n + (GAPS[k] if k < len(GAPS) else 0)
    return out


def make_inputs():
    """(matrix int64 [n_cols, 18], major int64 [n_cols], candidate positions int64 [n_cand], depths int32 [n_cand]) from the seeds alone"""
    rng = np.random.default_rng(REGION_SEED)
    chunks = chunk_bounds()
    n_cols = sum(CHUNK_LENS)
    major = np.concatenate([np.arange(p0, p1 + 1) for _, _, p0, p1 in chunks]).astype(np.int64)
    # counts of the realistic recipe laid end to end (no column of it is all zero: every position holds its reads)
    matrix = syn.make_pileup_windows(n_cols // T + 1, seed=REGION_SEED + 1, dtype=np.int32, depth=120).reshape(-1, C)[:n_cols].astype(np.int64)
    c0, n, _, _ = chunks[DEEP_CHUNK]
    matrix[c0:c0 + n] = syn.make_pileup_windows(n // T + 1, seed=REGION_SEED + 2, dtype=np.int32, depth=400).reshape(-1, C)[:n]
    assert not (matrix == 0).all(axis=1).any()
    for k, off in EMPTY:
        c0, n, _, _ = chunks[k]
        matrix[c0 + off if off >= 0 else c0 + n + off] = 0
    cand = []
    for c0, n, p0, p1 in chunks:  # the edges of the rule, for every chunk (a short chunk's land in its gaps or its neighbours)
        cand += [p0, p0 + F, p0 + F + 1, p1 - F - 1, p1 - F, p1 - F + 1, p1]
        if n >= 100:
            cand += list(range(p0 + 1, p0 + F + 1, 2)) + list(range(p1 - F + 2, p1, 2))
    # around every empty column: windows that hold it at their first, middle and last column, and in between
    for k, off in EMPTY:
        _, n, p0, _ = chunks[k]
        e = p0 + (off if off >= 0 else n + off)
        cand += [e + F + 1, e + 1, e - F + 1] + [e + d for d in (-F, -9, -4, 5, 11, F)]
    # outside every chunk: before the first, in the gaps, behind the last
    cand += [FIRST_POSITION - 40, FIRST_POSITION - 1, chunks[-1][3] + 1, chunks[-1][3] + 30]
    for k in range(len(chunks) - 1):
        if chunks[k + 1][2] - chunks[k][3] > 1:
            cand.append(chunks[k][3] + 1)
    cand += rng.integers(FIRST_POSITION - 20, chunks[-1][3] + 20, size=160).tolist()
    cand = rng.permutation(np.unique(np.array(cand, dtype=np.int64)))  # no position twice; NOT sorted: the order is the caller's
    depth = rng.choice(np.array([30, 80, 150, 216, 217, 400, 3000], np.int32), size=len(cand)).astype(np.int32)
    return matrix, major, cand, depth


# ------------------------------------------------------------------------------------------------ the reference, driven
class _PlpData:
    pass


class _Ffi:
    def buffer(self, arr, nbytes):
        b = np.ascontiguousarray(arr).tobytes()
        assert len(b) == nbytes, (len(b), nbytes)
        return b

    def string(self, b):
        return b

    def gc(self, obj, destructor):
        return obj


class _Lib:
    featlenclair3 = C

    def __init__(self):
        self.plp = None
        self.calls = 0

    def create_bam_fset(self, bam, fasta):
        return object()

    def destroy_bam_fset(self, fset):
        pass

    def calculate_clair3_pileup(self, *args):
        self.calls += 1
        return self.plp

    def destroy_plp_data(self, *args):
        pass


def reference_selection(matrix, major, cand, depth, head_tail, workdir):
    """(kept positions in the reference's order, int32 windows [n_kept, 33, 18]) from CreateTensorPileup itself"""
    mod = sys.modules.get("libclair3")
    if mod is None or not isinstance(getattr(mod, "lib", None), _Lib):
        mod = types.ModuleType("libclair3")
        mod.ffi, mod.lib = _Ffi(), _Lib()
        sys.modules["libclair3"] = mod
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from preprocess import CreateTensorPileupFromCffi as producer
    plp = _PlpData()
    plp.matrix, plp.n_cols = np.ascontiguousarray(matrix, dtype=np.int64), len(major)
    plp.major, plp.minor = np.ascontiguousarray(major, dtype=np.int64), np.zeros(len(major), np.int64)
    plp.candidates_num = len(cand)
    plp.all_alt_info = [f"{int(p)}-{int(d)}-A-X1 5".encode() for p, d in zip(cand, depth)]
    mod.lib.plp = plp
    fasta = os.path.join(workdir, "ref.fa")
    with open(fasta, "w") as fh:
        fh.write(">chr1\nA\n")
    with open(fasta + ".fai", "w") as fh:
        fh.write("chr1\t100000000\t6\t60\t61\n")
    args = types.SimpleNamespace(
        ctgName="chr1", ctgStart=int(major[0]), ctgEnd=int(major[-1]), ref_fn=fasta, bam_fn="reads.bam", chunk_id=None, chunk_num=None,
        snp_min_af=0.08, indel_min_af=0.15, minCoverage=2, minMQ=5, platform="ont", enable_variant_calling_at_sequence_head_and_tail=head_tail,
        vcf_fn=None, extend_bed=None, fast_mode=False, call_snp_only=False, enable_long_indel=False, gvcf=False, tensor_can_fn="PIPE",
        samtools="samtools", temp_file_dir=workdir, sampleName="sample", bp_resolution=False, base_err=0.001, gq_bin_size=5)
    calls = mod.lib.calls
    windows, position_info, alt_info = producer.CreateTensorPileup(args)
    assert mod.lib.calls == calls + 1, "the reference did not take its pileup from the stand-in"
    windows = np.asarray(windows, dtype=np.int32).reshape(-1, T, C)
    kept = np.array([int(s.split(":")[1]) for s in position_info], dtype=np.int64)
    assert len(kept) == len(windows) == len(alt_info)
    return kept, windows


# ------------------------------------------------------------------------------------------------ what the fixture promises
def classify(matrix, major, cand, head_tail):
    """the status of every candidate, one candidate at a time (conditions() checks its kept ones against the reference's)"""
    cuts = np.flatnonzero(np.diff(major) != 1) + 1
    a, b = np.r_[0, cuts], np.r_[cuts, len(major)]
    empty = (matrix == 0).all(axis=1)
    status, where = [], []
    for pos in cand.tolist():
        st, hit = NO_WINDOW, None
        for c0, c1 in zip(a, b):
            first, last = int(major[c0]), int(major[c1 - 1])
            if not first <= pos <= last:
                continue
            lo = pos - F - 1
            if lo >= first and pos + F + 1 <= last:
                col = c0 + lo - first
                hit = np.flatnonzero(empty[col:col + T])
                st = EMPTY_COLUMN if len(hit) else MAIN
            elif head_tail and lo < first:
                st = HEAD if lo + T - 1 <= last else NO_WINDOW
            elif head_tail:
                st = TAIL
        status.append(st)
        where.append(hit)
    return np.array(status, np.uint8), where


def conditions(matrix, major, cand, depth, kept, windows):
    """asserts what the fixture promises; kept / windows: {mode: array} for mode "main" and "head_tail".  Returns {mode: status counts}."""
    cuts = np.flatnonzero(np.diff(major) != 1) + 1
    a, b = np.r_[0, cuts], np.r_[cuts, len(major)]
    lens = set((b - a).tolist())
    assert len(a) >= 3 and {1, 32, 33, 34, 35} <= lens and max(lens) >= 100, sorted(lens)
    assert len(set(cand.tolist())) == len(cand) and (np.diff(cand) < 0).any(), "candidates: no duplicates, not sorted"
    cs = set(cand.tolist())
    for c0, c1 in zip(a, b):
        first, last = int(major[c0]), int(major[c1 - 1])
        assert {first, first + F, first + F + 1, last - F - 1, last - F, last - F + 1, last} <= cs, (first, last)
    inside = np.isin(cand, major)
    assert (~inside).sum() >= 8 and (cand < major[0]).any() and (cand > major[-1]).any()
    counts = {}
    for mode, ht in (("main", False), ("head_tail", True)):
        status, where = classify(matrix, major, cand, ht)
        is_kept = np.isin(status, (MAIN, HEAD, TAIL))
        assert np.array_equal(cand[is_kept], kept[mode]), f"{mode}: the reference kept other candidates"
        assert windows[mode].shape == (int(is_kept.sum()), T, C) and windows[mode].dtype == np.int32
        counts[mode] = {int(s): int((status == s).sum()) for s in range(5)}
        for s in (NO_WINDOW, MAIN, EMPTY_COLUMN) + ((HEAD, TAIL) if ht else ()):
            assert counts[mode][s] >= MIN_PER_STATUS, (mode, counts[mode])
        if not ht:
            assert counts[mode][HEAD] == counts[mode][TAIL] == 0
        dropped_at = {int(h[0]) for s, h in zip(status, where) if s == EMPTY_COLUMN and len(h) == 1}
        assert {0, T // 2, T - 1} <= dropped_at, f"{mode}: windows dropped for an empty column at {sorted(dropped_at)}"
        w = windows[mode]
        zero_rows = (w == 0).all(axis=2)
        kept_status = status[is_kept]
        if ht:
            # a kept head / tail window that holds an empty column of the matrix (not only its padding): a zero row strictly inside its data
            n_inside = 0
            for j in np.flatnonzero(np.isin(kept_status, (HEAD, TAIL))):
                rows = np.flatnonzero(~zero_rows[j])
                n_inside += bool(zero_rows[j, rows[0]:rows[-1]].any())
            assert n_inside >= 1, "no kept head / tail window holds an empty column"
            assert zero_rows[kept_status == HEAD, 0].all() or (kept_status == HEAD).sum() == 0
        else:
            assert not zero_rows.any(), "a main window with an empty column was kept"
        d = depth[is_kept]
        assert ((d > 0) & (d > 1.5 * syn.MAX_DEPTH)).any() and (d <= 216).any(), f"{mode}: rescaled and untouched windows among the kept"
    return counts


def main():
    matrix, major, cand, depth = make_inputs()
    kept, windows = {}, {}
    with tempfile.TemporaryDirectory() as workdir:
        for mode, ht in (("main", False), ("head_tail", True)):
            kept[mode], windows[mode] = reference_selection(matrix, major, cand, depth, ht, workdir)
    counts = conditions(matrix, major, cand, depth, kept, windows)
    meta = dict(region_seed=REGION_SEED, n_cols=len(major), n_cand=len(cand), chunk_lens=list(CHUNK_LENS), gaps=list(GAPS), status_counts=counts,
                matrix_sha=digest(matrix), major_sha=digest(major), cand_sha=digest(cand), depth_sha=digest(depth),
                kept_sha={m: digest(kept[m]) for m in kept}, windows_sha={m: digest(windows[m]) for m in windows}, numpy=np.__version__)
    path = os.path.join(HERE, "pileup_candidates.npz")
    np.savez_compressed(path, matrix=matrix, major=major, cand=cand, depth=depth, kept_main=kept["main"], windows_main=windows["main"],
                        kept_head_tail=kept["head_tail"], windows_head_tail=windows["head_tail"], meta=np.array(json.dumps(meta)))
    print(f"pileup_candidates: {len(major)} columns, {len(cand)} candidates, status counts {counts}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
