"""Full alignment from reads: the candidate windows of the reference's calculate_clair3_full_alignment
(src/clair3_full_alignment_dwell.c:437-1054) from aligned reads as the arrays a BAM record holds (csrc/c3_fa_rule.h states the rule and where
it leaves the reference, csrc/c3_fa_reads.h holds the kernels).  The reads' haplotypes are an input, or are computed from phased variants
by the reference's haplotag_read (csrc/c3_hap_rule.h, csrc/c3_hap_reads.h) in the same call.  Limits: no BAM or VCF index is read, het
SNPs only (as the reference).  With the reads' move tables (ReadMoves) the windows have the ninth, dwell-time channel of
--enable_dwell_time (csrc/c3_dwell_rule.h, csrc/c3_dwell.h): the caller converts any B subtype of the mv tag to int8 (only zero or
non-zero matters), and only synthetic tables have been run so far.

    pileup_reads.ReadSet.from_arrays(...)                  c3_read_set: BAM's own encoding, reads in COORDINATE ORDER
    ReadExtras.from_arrays(qual_first, qual, haplotype, name_key=None)   c3_read_extras: a quality byte per query base, HP tag, name key
    fa_windows(reads, extras, centres, ref_bytes, ref_first, path=None, **cfg)   (rows, counts, depths, alt_info_list): rows (n_rows, 33, 8)
        int8 are the occupied rows of all windows back to back, counts[b] of them for candidate b -- the arguments of
        Clair3_F.predict_rows; synthetic.pad_fa_rows(rows, counts, depth=matrix_depth) is the dense tensor
    Context(device)                                        keeps the device buffers between calls; .run .sizes .fetch .stats;
        Clair3_F.predict_reads(context) runs the held windows through the network without fetching them
    PhasedVariants.from_arrays(pos, alt_base, genotype, phase_set) / .from_dict / .from_vcf(path, ctg_name)   c3_phased_variants: the phased
        heterozygous SNPs of one contig, positions 0-based and strictly ascending
    Context.haplotag(reads, variants, ref_bytes, ref_first, path=None, min_haplotag_mq=20)   uint8 tags (0, 1, 2) of every read;
        .haplotag_pairs() the allele of every (read, variant) pair with the n + 1 offsets, .haplotag_stats()
    Context.run(..., variants=V) / fa_windows(..., variants=V)   tag and build the windows in one call: extras need no haplotype, and on
        the device the tags never visit the host
    ReadMoves.from_arrays(mv_first, mv) / .from_dict        c3_read_moves: the mv tags of the reads back to back, element 0 the stride
    Context.run(..., moves=M) / fa_windows(..., moves=M)   rows (n_rows, 33, 9): channel 8 is the dwell channel; with or without variants.
        Context.dwell_table() the per-read prefix tables the cells read; Clair3_F.predict_reads(context) then needs a 9-channel model

    python -m clair3_amd.fa_reads --reads X.npz --ref_fn ref.fa --ctgName c --candidates pos.txt [--chkpnt_fn M] [--output_fn F.npz]
                                  [--path device|host] [--min_mq N] [--max_indel_length N] [--matrix_depth N] [--seed N]
                                  [--phased_vcf_fn V.vcf[.gz]]   (the reads are haplotagged from it; X.npz then needs no haplotype)
                                  [--enable_dwell_time]   (X.npz also holds mv_first and mv; 9-channel windows)
        X.npz: the seven arrays of ReadSet.from_arrays and qual_first, qual, haplotype[, name_key].  pos.txt: one 1-based position per
        line, ascending.  The alt-info lines go to stdout; --output_fn gets rows, counts, depths (and, with --chkpnt_fn, a checkpoint
        of Clair3_F, the probability rows y).

``path``: "device" runs the kernels, "host" the same rule as sequential C (no GPU needed); None reads $C3HIP_FA_READS, whose default is
"device" where a GPU is visible and "host" otherwise.  Both give the same bytes.  A device call with a candidate that more than 1024 reads
overlap answers through the host form (stats()["fell_back"]).
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _lib
from .pileup_reads import ReadSet, _read_contig, _ref_array

FA_POSITIONS, FA_CHANNELS = 33, 8
ERR_REFSKIP = 2  # C3_FA_ERR_REFSKIP

DEFAULTS = dict(min_mq=5, max_indel_length=50, matrix_depth=89, lds_reads=0, seed=0)
HAP_DEFAULTS = dict(min_haplotag_mq=20)  # min_haplotag_mq, src/clair3_full_alignment_dwell.h:20


class RefSkipError(_lib.C3Error):
    """a kept read has an N op over a flanking position of a candidate (C3_FA_ERR_REFSKIP)"""


def default_path():
    """$C3HIP_FA_READS (device | host); unset: device where a GPU is visible, host otherwise (as $C3HIP_PILEUP)"""
    v = os.environ.get("C3HIP_FA_READS")
    if v is not None:
        if v not in ("device", "host"):
            raise ValueError(f"C3HIP_FA_READS={v}: expected device or host")
        return v
    try:
        return "device" if _lib.device_count() > 0 else "host"
    except _lib.C3Error:
        return "host"


def config(**cfg):
    unknown = set(cfg) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}; expected some of {sorted(DEFAULTS)}")
    c = dict(DEFAULTS, **cfg)
    return _lib.FaConfig(int(c["min_mq"]), int(c["max_indel_length"]), int(c["matrix_depth"]), int(c["lds_reads"]), int(c["seed"]) & ((1 << 64) - 1))


class ReadExtras:
    """c3_read_extras: the arrays are kept alive by this object"""
    FIELDS = (("qual_first", np.int64), ("qual", np.uint8), ("haplotype", np.uint8), ("name_key", np.uint64))

    def __init__(self, arrays):
        self.arrays = arrays
        if arrays["haplotype"] is None:  # (Context.run(..., variants=V) computes it)
            if len(arrays["qual_first"]) < 1:
                raise ValueError("qual_first of n + 1 offsets expected")
        elif len(arrays["qual_first"]) != len(arrays["haplotype"]) + 1:
            raise ValueError("qual_first of n + 1 offsets and haplotype of n reads expected")
        if int(arrays["qual_first"][-1]) > len(arrays["qual"]):
            raise ValueError("the last offset of qual_first lies behind the end of qual")
        if arrays["name_key"] is not None and len(arrays["name_key"]) != len(arrays["qual_first"]) - 1:
            raise ValueError("name_key of n reads expected")
        self.c = _lib.ReadExtrasC(*[arrays[name].ctypes.data if arrays[name] is not None and arrays[name].size else None for name, _ in self.FIELDS])

    @classmethod
    def from_arrays(cls, qual_first, qual, haplotype=None, name_key=None):
        given = dict(qual_first=qual_first, qual=qual, haplotype=haplotype, name_key=name_key)
        return cls({name: None if given[name] is None else np.ascontiguousarray(given[name], dtype=dt).reshape(-1) for name, dt in cls.FIELDS})

    @classmethod
    def from_dict(cls, d, names=True):
        """from the dict synthetic.make_read_extras returns, or an .npz; names=False drops the name keys (no duplicate-name filter)"""
        keys = d.files if hasattr(d, "files") else d
        has = names and "name_key" in keys
        return cls.from_arrays(d["qual_first"], d["qual"], d["haplotype"] if "haplotype" in keys else None, d["name_key"] if has else None)

    def __len__(self):
        return len(self.arrays["qual_first"]) - 1


class ReadMoves:
    """c3_read_moves: read r owns mv[mv_first[r] : mv_first[r + 1]], its mv tag as int8 (element 0 is the stride); the arrays are kept
    alive by this object"""

    def __init__(self, mv_first, mv):
        self.arrays = {"mv_first": mv_first, "mv": mv}
        if len(mv_first) < 1:
            raise ValueError("mv_first of n + 1 offsets expected")
        if int(mv_first[-1]) > len(mv):
            raise ValueError("the last offset of mv_first lies behind the end of mv")
        self.c = _lib.ReadMovesC(mv_first.ctypes.data, mv.ctypes.data if mv.size else None)

    @classmethod
    def from_arrays(cls, mv_first, mv):
        return cls(np.ascontiguousarray(mv_first, dtype=np.int64).reshape(-1), np.ascontiguousarray(mv, dtype=np.int8).reshape(-1))

    @classmethod
    def from_dict(cls, d):
        """from the dict synthetic.make_read_moves returns, or an .npz"""
        return cls.from_arrays(d["mv_first"], d["mv"])

    def __len__(self):
        return len(self.arrays["mv_first"]) - 1


def dwell_cum(mv, l, reverse=False):
    """(cum (l + 1,) int32, has_table) of one read by c3_fa_dwell_cum_host: mv its move table (element 0 the stride), l its query length"""
    mv = np.ascontiguousarray(mv, dtype=np.int8).reshape(-1)
    cum = np.zeros(int(l) + 1, np.int32)
    has = _lib.lib().c3_fa_dwell_cum_host(mv.ctypes.data if mv.size else None, len(mv), int(l), int(bool(reverse)), cum.ctypes.data)
    return cum, bool(has)


def hap_config(**cfg):
    unknown = set(cfg) - set(HAP_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}; expected some of {sorted(HAP_DEFAULTS)}")
    return _lib.HaplotagConfig(int(dict(HAP_DEFAULTS, **cfg)["min_haplotag_mq"]), 0)


class PhasedVariants:
    """c3_phased_variants: the phased heterozygous SNPs of one contig; the arrays are kept alive by this object"""
    FIELDS = (("pos", np.int64), ("alt_base", np.uint8), ("genotype", np.uint8), ("phase_set", np.int32))

    def __init__(self, arrays):
        self.arrays = arrays
        n = len(arrays["pos"])
        if any(len(arrays[name]) != n for name, _ in self.FIELDS):
            raise ValueError("pos, alt_base, genotype and phase_set of one length expected")
        self.c = _lib.PhasedVariantsC(n, *[arrays[name].ctypes.data if n else None for name, _ in self.FIELDS])

    @classmethod
    def from_arrays(cls, pos, alt_base, genotype, phase_set):
        given = dict(pos=pos, alt_base=alt_base, genotype=genotype, phase_set=phase_set)
        if isinstance(alt_base, (bytes, str)):
            given["alt_base"] = np.frombuffer(alt_base.encode("ascii") if isinstance(alt_base, str) else alt_base, np.uint8)
        return cls({name: np.ascontiguousarray(given[name], dtype=dt).reshape(-1) for name, dt in cls.FIELDS})

    @classmethod
    def from_dict(cls, d):
        """from the dict synthetic.make_phased_variants returns, or an .npz"""
        return cls.from_arrays(d["pos"], d["alt_base"], d["genotype"], d["phase_set"])

    @classmethod
    def from_vcf(cls, path, ctg_name=None):
        """the rule of preprocess/CreateTensorFullAlignmentFromCffi.py:84-102: plain or gzip; rows of ``ctg_name`` whose GT holds '|';
        genotype 1 for 0|1, else 2; PS is the last field of the sample column; pos - 1.  A REF or ALT of more than one base raises
        ValueError (the reference's cffi char would)."""
        import gzip
        with open(path, "rb") as fh:
            zipped = fh.read(2) == b"\x1f\x8b"
        pos, alt, gt, ps = [], [], [], []
        with (gzip.open(path, "rt") if zipped else open(path, "rt")) as fh:
            for row in fh:
                row = row.rstrip()
                if not row or row[0] == "#":
                    continue
                columns = row.strip().split("\t")
                if ctg_name and columns[0] != ctg_name:
                    continue
                info = columns[9].split(":")
                genotype, phase_set = info[0], info[-1]
                if "|" not in genotype:
                    continue
                if len(columns[3]) != 1 or len(columns[4]) != 1:
                    raise ValueError(f"{path}: {columns[0]}:{columns[1]} has REF {columns[3]} and ALT {columns[4]}: phased SNPs of one base expected")
                pos.append(int(columns[1]) - 1), alt.append(ord(columns[4])), gt.append(1 if genotype == "0|1" else 2), ps.append(int(phase_set))
        return cls.from_arrays(pos, alt, gt, ps)

    def __len__(self):
        return len(self.arrays["pos"])


class Context:
    """c3_fa_reads_create: with a device, a stream and buffers that grow and never shrink (use one per process and keep it); device=None: a
    context without a GPU, for the host form"""

    def __init__(self, device=0):
        self.h = None
        self._destroy = _lib.lib().c3_fa_reads_destroy
        self.device = device
        self.h = _lib.lib().c3_fa_reads_create(-1 if device is None else int(device))
        if not self.h:
            raise _lib.C3Error(f"c3_fa_reads_create: {_lib.last_error()}")

    def close(self):
        if self.h:
            self._destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _path(self, path):
        path = path or ("host" if self.device is None else "device")
        if path not in ("device", "host"):
            raise ValueError(f"path={path}: expected device or host")
        return path

    def haplotag(self, reads, variants, ref_bytes, ref_first, path=None, **cfg):
        """(n,) uint8: the tag (0, 1, 2) of every read.  The tags stay in the context (after a device call: on the device)"""
        if not isinstance(reads, ReadSet):
            reads = ReadSet.from_dict(reads)
        if not isinstance(variants, PhasedVariants):
            variants = PhasedVariants.from_dict(variants)
        path = self._path(path)
        ref = _ref_array(ref_bytes)
        c = hap_config(**cfg)
        L = _lib.lib()
        fn, what = (L.c3_fa_haplotag, "c3_fa_haplotag") if path == "device" else (L.c3_fa_haplotag_host, "c3_fa_haplotag_host")
        _lib.check(fn(self.h, C.byref(reads.c), C.byref(variants.c), ref.ctypes.data if ref.size else None, int(ref_first), len(ref), C.byref(c)), what)
        return self.haplotag_pairs(pairs=False)[0]

    def haplotag_pairs(self, pairs=True):
        """(hap, alleles, pair_first) of the held tags: alleles (n_pairs,) int8 in read order, then variant order (0 none, 1 reference,
        2 alternative), pair_first (n + 1,) int64; pairs=False: alleles is None"""
        n, m = C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.lib().c3_fa_haplotag_sizes(self.h, C.byref(n), C.byref(m)), "c3_fa_haplotag_sizes")
        hap, first = np.zeros(n.value, np.uint8), np.zeros(n.value + 1, np.int64)
        alleles = np.zeros(m.value, np.int8) if pairs else None
        _lib.check(_lib.lib().c3_fa_haplotag_result(self.h, hap.ctypes.data if hap.size else None,
                                                    alleles.ctypes.data if pairs and alleles.size else None, first.ctypes.data), "c3_fa_haplotag_result")
        return hap, alleles, first

    def haplotag_stats(self):
        s = _lib.HaplotagCounters()
        _lib.check(_lib.lib().c3_fa_haplotag_stats(self.h, C.byref(s)), "c3_fa_haplotag_stats")
        names = ("staging", "op_table", "pairs", "votes")
        return {"reads_hap": tuple(s.reads_hap), "reads_low_mapq": s.reads_low_mapq, "pairs_realigned": s.pairs_realigned,
                "pairs_allele0": s.pairs_allele0, "on_host": bool(s.on_host), "kernel_ms": dict(zip(names, list(s.kernel_ms)))}

    def run(self, reads, extras, centres, ref_bytes, ref_first, path=None, variants=None, min_haplotag_mq=None, moves=None, **cfg):
        """one call; centres 0-based, strictly ascending.  The result stays in the context (after a device call: the rows on the device).
        variants (PhasedVariants or a dict of its arrays): the reads are haplotagged first and the extras' haplotype is not read.
        moves (ReadMoves or a dict of its arrays): the windows get the dwell channel (9 channels)"""
        if not isinstance(reads, ReadSet):
            reads = ReadSet.from_dict(reads)
        if not isinstance(extras, ReadExtras):
            extras = ReadExtras.from_dict(extras)
        if len(extras) != len(reads):
            raise ValueError(f"{len(extras)} extras for {len(reads)} reads")
        path = self._path(path)
        ref = _ref_array(ref_bytes)
        centres = np.ascontiguousarray(centres, dtype=np.int64).reshape(-1)
        c = config(**cfg)
        L = _lib.lib()
        args = (centres.ctypes.data if centres.size else None, len(centres), ref.ctypes.data if ref.size else None, int(ref_first), len(ref), C.byref(c))
        if variants is not None and not isinstance(variants, PhasedVariants):
            variants = PhasedVariants.from_dict(variants)
        if moves is not None:
            if not isinstance(moves, ReadMoves):
                moves = ReadMoves.from_dict(moves)
            if len(moves) != len(reads):
                raise ValueError(f"{len(moves)} move tables for {len(reads)} reads")
            if variants is None and min_haplotag_mq is not None:
                raise TypeError("min_haplotag_mq without variants")
            hc = None if variants is None else hap_config(**({} if min_haplotag_mq is None else {"min_haplotag_mq": min_haplotag_mq}))
            fn, what = (L.c3_fa_reads_dwell, "c3_fa_reads_dwell") if path == "device" else (L.c3_fa_reads_dwell_host, "c3_fa_reads_dwell_host")
            rc = fn(self.h, C.byref(reads.c), C.byref(extras.c), C.byref(moves.c), None if variants is None else C.byref(variants.c), *args,
                    None if hc is None else C.byref(hc))
        elif variants is not None:
            hc = hap_config(**({} if min_haplotag_mq is None else {"min_haplotag_mq": min_haplotag_mq}))
            fn, what = (L.c3_fa_reads_phased, "c3_fa_reads_phased") if path == "device" else (L.c3_fa_reads_phased_host, "c3_fa_reads_phased_host")
            rc = fn(self.h, C.byref(reads.c), C.byref(extras.c), C.byref(variants.c), *args, C.byref(hc))
        else:
            if min_haplotag_mq is not None:
                raise TypeError("min_haplotag_mq without variants")
            fn, what = (L.c3_fa_reads, "c3_fa_reads") if path == "device" else (L.c3_fa_reads_host, "c3_fa_reads_host")
            rc = fn(self.h, C.byref(reads.c), C.byref(extras.c), *args)
        if rc == ERR_REFSKIP:
            raise RefSkipError(f"{what}: {_lib.last_error()}")
        _lib.check(rc, what)
        return self

    def sizes(self):
        v = [C.c_int64(0) for _ in range(3)]
        d = C.c_int32(0)
        _lib.check(_lib.lib().c3_fa_reads_sizes(self.h, *[C.byref(x) for x in v], C.byref(d)), "c3_fa_reads_sizes")
        return tuple(x.value for x in v) + (d.value,)  # n_cand, n_rows, text_bytes, matrix_depth

    def fetch(self):
        """dict of the held result: rows (n_rows, 33, 8) int8 (33, 9 after a call with moves), counts, depths (n_cand,) int32, text (bytes:
        one line per candidate)"""
        n_cand, n_rows, text_bytes, _ = self.sizes()
        out = {"rows": np.zeros((n_rows, FA_POSITIONS, self.channels()), np.int8), "counts": np.zeros(n_cand, np.int32), "depths": np.zeros(n_cand, np.int32)}
        text = C.create_string_buffer(max(text_bytes, 1))
        ptr = [out[k].ctypes.data if out[k].size else None for k in ("rows", "counts", "depths")]
        _lib.check(_lib.lib().c3_fa_reads_result(self.h, *ptr, text), "c3_fa_reads_result")
        out["text"] = text.raw[:text_bytes]
        return out

    def channels(self):
        """8, or 9 when the held result has the dwell channel"""
        return int(_lib.lib().c3_fa_reads_channels(self.h))

    def dwell_table(self):
        """(qual_first[n] - qual_first[0] + n,) int32: the prefix tables of the last call with moves, read r's l + 1 entries at
        qual_first[r] - qual_first[0] + r (after a device call: fetched from the device); empty after any other call"""
        n = int(_lib.lib().c3_fa_dwell_table(self.h, None))
        if n < 0:
            raise _lib.C3Error(f"c3_fa_dwell_table: {_lib.last_error()}")
        cum = np.zeros(n, np.int32)
        if n and _lib.lib().c3_fa_dwell_table(self.h, cum.ctypes.data) != n:
            raise _lib.C3Error(f"c3_fa_dwell_table: {_lib.last_error()}")
        return cum

    def stats(self):
        s = _lib.FaCounters()
        _lib.check(_lib.lib().c3_fa_reads_stats(self.h, C.byref(s)), "c3_fa_reads_stats")
        names = ("staging", "op_table", "candidates", "scan", "fill", "fetch", "moves_staged", "dwell_table")
        return {"reads_kept": s.reads_kept, "reads_dropped": s.reads_dropped, "rows": s.rows, "deep_windows": s.deep_windows,
                "fell_back": bool(s.fell_back), "on_host": bool(s.on_host), "kernel_ms": dict(zip(names, list(s.kernel_ms)))}


_contexts = {}


def _shared_context(path):
    key = (os.getpid(), path)
    if key not in _contexts:
        _contexts[key] = Context(0 if path == "device" else None)
    return _contexts[key]


def fa_windows(reads, extras, centres, ref_bytes, ref_first, path=None, context=None, variants=None, moves=None, **cfg):
    """(rows, counts, depths, alt_info_list) of the candidates at ``centres`` (0-based, strictly ascending, each >= 16).  cfg: DEFAULTS above;
    variants: the reads are haplotagged from them first; moves: rows with the dwell channel (Context.run)"""
    path = path or default_path()
    ctx = context or _shared_context(path)
    r = ctx.run(reads, extras, centres, ref_bytes, ref_first, path=path, variants=variants, moves=moves, **cfg).fetch()
    return r["rows"], r["counts"], r["depths"], r["text"].decode("ascii").split("\n")[:-1]


def main(argv=None):
    from argparse import ArgumentParser
    ap = ArgumentParser(description="full-alignment windows (and, with a checkpoint, their probability rows) from decoded reads")
    ap.add_argument("--reads", required=True)
    ap.add_argument("--ref_fn", required=True)
    ap.add_argument("--ctgName", required=True)
    ap.add_argument("--candidates", required=True)
    ap.add_argument("--chkpnt_fn")
    ap.add_argument("--output_fn")
    ap.add_argument("--path", choices=("device", "host"))
    ap.add_argument("--phased_vcf_fn", help="phased het SNPs (plain or gzip): the reads are haplotagged from them")
    ap.add_argument("--enable_dwell_time", action="store_true", help="9-channel windows: the reads file also holds mv_first and mv")
    for name in ("min_mq", "max_indel_length", "matrix_depth", "seed"):
        ap.add_argument("--" + name, type=int, default=DEFAULTS[name])
    a = ap.parse_args(argv)
    ref = _read_contig(a.ref_fn, a.ctgName)
    with open(a.candidates) as fh:
        centres = np.array([int(line.split()[0]) - 1 for line in fh if line.strip()], np.int64)
    with np.load(a.reads) as z:
        reads, extras = ReadSet.from_dict(z), ReadExtras.from_dict(z)
        moves = ReadMoves.from_dict(z) if a.enable_dwell_time else None
    path = a.path or default_path()
    cfg = dict(min_mq=a.min_mq, max_indel_length=a.max_indel_length, matrix_depth=a.matrix_depth, seed=a.seed)
    out = {}
    with Context(0 if path == "device" else None) as ctx:
        variants = PhasedVariants.from_vcf(a.phased_vcf_fn, a.ctgName) if a.phased_vcf_fn else None
        r = ctx.run(reads, extras, centres, ref, 0, path=path, variants=variants, moves=moves, **cfg).fetch()
        out.update(rows=r["rows"], counts=r["counts"], depths=r["depths"])
        if a.chkpnt_fn:
            import torch
            from .model import Clair3_F
            sd = torch.load(a.chkpnt_fn, map_location="cpu")
            m = Clair3_F(add_indel_length=True, predict=True, input_channels=9 if a.enable_dwell_time else 8).to("cuda:0")
            m.eval()
            m.load_state_dict(sd.get("state_dict", sd))
            out["y"] = m.predict_reads(ctx)
    sys.stdout.write(r["text"].decode("ascii"))
    if a.output_fn:
        np.savez(a.output_fn, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
