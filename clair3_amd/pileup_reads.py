"""Pileup from reads: the region matrix, major, the candidates' alt-info and the gVCF count pair of the reference's
calculate_clair3_pileup (src/clair3_pileup.c:208-461) from aligned reads as the arrays a BAM record holds (csrc/c3_pileup_rule.h states the
rule and where it leaves the reference, csrc/c3_pileup.h holds the kernels).  No BAM file is read here: the feature starts at decoded records.

    ReadSet.from_arrays(pos, flag, mapq, cigar_first, cigar, seq_first, seq)   c3_read_set: BAM's own encoding, reads in any order
    pileup_counts(reads, start, end, ref_bytes, ref_first, path=None, **cfg)   (counts, major, alt_info_list, (n_ref, n_total)): what
        pileup_counts_clair3 hands the reference's loop (preprocess/CreateTensorPileupFromCffi.py); region [start, end), 0-based
    Context(device)                                                            keeps the device buffers between calls; .stats()

    python -m clair3_amd.pileup_reads --reads X.npz --ref_fn ref.fa --ctgName c --ctgStart s --ctgEnd e [--output_fn F.npz] [--path device|host]
                                      [--min_depth N] [--min_snp_af F] [--min_indel_af F] [--min_mq N] [--max_indel_length N]
                                      [--call_snp_only] [--no_gvcf] [--call_ht]
        X.npz: the seven arrays of ReadSet.from_arrays.  --ctgStart / --ctgEnd are 1-based and inclusive, as the reference's are.  The
        alt-info lines go to stdout; with --output_fn the arrays counts, major, n_ref, n_total are written.

``path``: "device" runs the kernels, "host" the same rule as sequential C (no GPU needed); None reads $C3HIP_PILEUP, whose default is
"device" where a GPU is visible and "host" otherwise.  Both give the same bytes.  A device call that finds two different indels under one
key of its table answers through the host form (stats()["fell_back"]).
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _lib

PILEUP_CHANNELS = 18  # shared/param_p.py:32-33

DEFAULTS = dict(min_depth=0, min_snp_af=0.0, min_indel_af=0.0, min_mq=5, max_indel_length=50, call_snp_only=False, gvcf=True, call_ht=False,
                hash_mask=0xFFFFFFFFFFFFFFFF)


def default_path():
    """$C3HIP_PILEUP (device | host); unset: device where a GPU is visible, host otherwise.  Asking whether one is visible initialises the
    HIP runtime in this process: a run that fans out into many producer processes should set the variable explicitly"""
    v = os.environ.get("C3HIP_PILEUP")
    if v is not None:
        if v not in ("device", "host"):
            raise ValueError(f"C3HIP_PILEUP={v}: expected device or host")
        return v
    try:
        return "device" if _lib.device_count() > 0 else "host"
    except _lib.C3Error:
        return "host"


def config(**cfg):
    unknown = set(cfg) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown pileup option(s) {sorted(unknown)}; expected some of {sorted(DEFAULTS)}")
    c = dict(DEFAULTS, **cfg)
    return _lib.PileupConfig(int(c["min_depth"]), float(c["min_snp_af"]), float(c["min_indel_af"]), int(c["min_mq"]), int(c["max_indel_length"]),
                             1 if c["call_snp_only"] else 0, 1 if c["gvcf"] else 0, 1 if c["call_ht"] else 0, 0, int(c["hash_mask"]))


class ReadSet:
    """c3_read_set: the arrays are kept alive by this object"""
    FIELDS = (("pos", np.int64), ("flag", np.uint16), ("mapq", np.uint8), ("cigar_first", np.int64), ("cigar", np.uint32),
              ("seq_first", np.int64), ("seq", np.uint8))

    def __init__(self, arrays):
        self.arrays = arrays
        n = len(arrays["pos"])
        if len(arrays["flag"]) != n or len(arrays["mapq"]) != n or len(arrays["cigar_first"]) != n + 1 or len(arrays["seq_first"]) != n + 1:
            raise ValueError("pos, flag, mapq of n reads and cigar_first, seq_first of n + 1 offsets expected")
        if int(arrays["cigar_first"][-1]) > len(arrays["cigar"]) or int(arrays["seq_first"][-1]) > len(arrays["seq"]):
            raise ValueError("the last offset of cigar_first / seq_first lies behind the end of cigar / seq")
        self.c = _lib.ReadSetC(n, *[arrays[name].ctypes.data if arrays[name].size else None for name, _ in self.FIELDS])

    @classmethod
    def from_arrays(cls, pos, flag, mapq, cigar_first, cigar, seq_first, seq):
        given = dict(pos=pos, flag=flag, mapq=mapq, cigar_first=cigar_first, cigar=cigar, seq_first=seq_first, seq=seq)
        return cls({name: np.ascontiguousarray(given[name], dtype=dt).reshape(-1) for name, dt in cls.FIELDS})

    @classmethod
    def from_dict(cls, d):
        """from the dict synthetic.make_read_set / pack_reads return, or an .npz of the seven arrays"""
        return cls.from_arrays(*[d[name] for name, _ in cls.FIELDS])

    def __len__(self):
        return int(self.c.n_reads)


def _ref_array(ref_bytes):
    if isinstance(ref_bytes, str):
        ref_bytes = ref_bytes.encode()
    if isinstance(ref_bytes, (bytes, bytearray)):
        return np.frombuffer(bytes(ref_bytes), dtype=np.uint8)
    return np.ascontiguousarray(ref_bytes, dtype=np.uint8).reshape(-1)


class Context:
    """c3_pileup_create: with a device, a stream and buffers that grow and never shrink (use one per process and keep it); device=None: a
    context without a GPU, for the host form"""

    def __init__(self, device=0):
        self.h = None
        self._destroy = _lib.lib().c3_pileup_destroy
        self.device = device
        self.h = _lib.lib().c3_pileup_create(-1 if device is None else int(device))
        if not self.h:
            raise _lib.C3Error(f"c3_pileup_create: {_lib.last_error()}")

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

    def run(self, reads, start, end, ref_bytes, ref_first, path=None, **cfg):
        """one call; the result stays in the context (after a device call: on the device) until the next one"""
        if not isinstance(reads, ReadSet):
            reads = ReadSet.from_dict(reads)
        path = path or ("host" if self.device is None else "device")
        if path not in ("device", "host"):
            raise ValueError(f"path={path}: expected device or host")
        ref = _ref_array(ref_bytes)
        c = config(**cfg)
        L = _lib.lib()
        fn, what = (L.c3_pileup_reads, "c3_pileup_reads") if path == "device" else (L.c3_pileup_reads_host, "c3_pileup_reads_host")
        _lib.check(fn(self.h, C.byref(reads.c), int(start), int(end), ref.ctypes.data if ref.size else None, int(ref_first), len(ref), C.byref(c)), what)
        return self

    def sizes(self):
        v = [C.c_int64(0) for _ in range(4)]
        _lib.check(_lib.lib().c3_pileup_sizes(self.h, *[C.byref(x) for x in v]), "c3_pileup_sizes")
        return tuple(x.value for x in v)  # n_cols, n_cand, n_sites, text_bytes

    def fetch(self):
        """dict of the held result: counts (n_cols, 18) int32, major, cand_pos (0-based), cand_depth, n_ref, n_total (empty without gvcf),
        text (bytes: one line per candidate)"""
        n_cols, n_cand, n_sites, text_bytes = self.sizes()
        out = {"counts": np.zeros((n_cols, PILEUP_CHANNELS), np.int32), "major": np.zeros(n_cols, np.int64), "cand_pos": np.zeros(n_cand, np.int64),
               "cand_depth": np.zeros(n_cand, np.int32), "n_ref": np.zeros(n_sites, np.int64), "n_total": np.zeros(n_sites, np.int64)}
        text = C.create_string_buffer(max(text_bytes, 1))
        ptr = [out[k].ctypes.data if out[k].size else None for k in ("counts", "major", "cand_pos", "cand_depth", "n_ref", "n_total")]
        _lib.check(_lib.lib().c3_pileup_result(self.h, *ptr, text), "c3_pileup_result")
        out["text"] = text.raw[:text_bytes]
        return out

    def stats(self):
        s = _lib.PileupCounters()
        _lib.check(_lib.lib().c3_pileup_stats(self.h, C.byref(s)), "c3_pileup_stats")
        names = ("op_table", "walk", "indel_table", "reduce", "site", "compaction", "staging", "fetch")
        return {"reads_kept": s.reads_kept, "reads_dropped": s.reads_dropped, "events": s.events, "collisions": s.collisions,
                "fell_back": bool(s.fell_back), "on_host": bool(s.on_host), "kernel_ms": dict(zip(names, list(s.kernel_ms)))}


_contexts = {}


def _shared_context(path):
    key = (os.getpid(), path)
    if key not in _contexts:
        _contexts[key] = Context(0 if path == "device" else None)
    return _contexts[key]


def pileup_counts(reads, start, end, ref_bytes, ref_first, path=None, context=None, **cfg):
    """(counts, major, alt_info_list, (n_ref, n_total)) of the region [start, end): counts (n_cols, 18) int32 and major (n_cols,) int64 as
    plp_data.matrix / major, alt_info_list the candidates' lines as pileup_counts_clair3 decodes all_alt_info, and the gVCF pair indexed by
    p - start (two empty arrays with gvcf=False).  cfg: DEFAULTS above, the arguments of calculate_clair3_pileup"""
    path = path or default_path()
    ctx = context or _shared_context(path)
    r = ctx.run(reads, start, end, ref_bytes, ref_first, path=path, **cfg).fetch()
    lines = r["text"].decode("ascii").split("\n")[:-1]
    return r["counts"], r["major"], lines, (r["n_ref"], r["n_total"])


def _read_contig(ref_fn, ctg):
    """one contig of a FASTA file as bytes (plain text: no index needed)"""
    out, on = [], False
    with open(ref_fn, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                on = line[1:].split()[0].decode() == ctg if line[1:].split() else False
            elif on:
                out.append(line.strip())
    if not out:
        raise ValueError(f"{ref_fn} holds no contig {ctg}")
    return b"".join(out)


def main(argv=None):
    from argparse import ArgumentParser
    ap = ArgumentParser(description="pileup counts, candidates and gVCF counts from decoded reads")
    ap.add_argument("--reads", required=True)
    ap.add_argument("--ref_fn", required=True)
    ap.add_argument("--ctgName", required=True)
    ap.add_argument("--ctgStart", type=int, required=True)
    ap.add_argument("--ctgEnd", type=int, required=True)
    ap.add_argument("--output_fn")
    ap.add_argument("--path", choices=("device", "host"))
    ap.add_argument("--min_depth", type=int, default=DEFAULTS["min_depth"])
    ap.add_argument("--min_snp_af", type=float, default=0.08)
    ap.add_argument("--min_indel_af", type=float, default=0.15)
    ap.add_argument("--min_mq", type=int, default=DEFAULTS["min_mq"])
    ap.add_argument("--max_indel_length", type=int, default=DEFAULTS["max_indel_length"])
    ap.add_argument("--call_snp_only", action="store_true")
    ap.add_argument("--no_gvcf", action="store_true")
    ap.add_argument("--call_ht", action="store_true")
    a = ap.parse_args(argv)
    ref = _read_contig(a.ref_fn, a.ctgName)
    with np.load(a.reads) as z:
        reads = ReadSet.from_dict(z)
    counts, major, lines, (n_ref, n_total) = pileup_counts(
        reads, a.ctgStart - 1, a.ctgEnd, ref, 0, path=a.path, min_depth=a.min_depth, min_snp_af=a.min_snp_af, min_indel_af=a.min_indel_af,
        min_mq=a.min_mq, max_indel_length=a.max_indel_length, call_snp_only=a.call_snp_only, gvcf=not a.no_gvcf, call_ht=a.call_ht)
    sys.stdout.write("".join(line + "\n" for line in lines))
    if a.output_fn:
        np.savez(a.output_fn, counts=counts, major=major, n_ref=n_ref, n_total=n_total)
    return 0


if __name__ == "__main__":
    sys.exit(main())
