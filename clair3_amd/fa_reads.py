"""Full alignment from reads: the candidate windows of the reference's calculate_clair3_full_alignment
(src/clair3_full_alignment_dwell.c:437-1054) from aligned reads as the arrays a BAM record holds (csrc/c3_fa_rule.h states the rule and where
it leaves the reference, csrc/c3_fa_reads.h holds the kernels).  Limits: no BAM file is read, the reads' haplotypes are an input (the
reference's haplotag_read is not built), 8 channels only (no dwell channel).

    pileup_reads.ReadSet.from_arrays(...)                  c3_read_set: BAM's own encoding, reads in COORDINATE ORDER
    ReadExtras.from_arrays(qual_first, qual, haplotype, name_key=None)   c3_read_extras: a quality byte per query base, HP tag, name key
    fa_windows(reads, extras, centres, ref_bytes, ref_first, path=None, **cfg)   (rows, counts, depths, alt_info_list): rows (n_rows, 33, 8)
        int8 are the occupied rows of all windows back to back, counts[b] of them for candidate b -- the arguments of
        Clair3_F.predict_rows; synthetic.pad_fa_rows(rows, counts, depth=matrix_depth) is the dense tensor
    Context(device)                                        keeps the device buffers between calls; .run .sizes .fetch .stats;
        Clair3_F.predict_reads(context) runs the held windows through the network without fetching them

    python -m clair3_amd.fa_reads --reads X.npz --ref_fn ref.fa --ctgName c --candidates pos.txt [--chkpnt_fn M] [--output_fn F.npz]
                                  [--path device|host] [--min_mq N] [--max_indel_length N] [--matrix_depth N] [--seed N]
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
        if len(arrays["qual_first"]) != len(arrays["haplotype"]) + 1:
            raise ValueError("qual_first of n + 1 offsets and haplotype of n reads expected")
        if int(arrays["qual_first"][-1]) > len(arrays["qual"]):
            raise ValueError("the last offset of qual_first lies behind the end of qual")
        if arrays["name_key"] is not None and len(arrays["name_key"]) != len(arrays["haplotype"]):
            raise ValueError("name_key of n reads expected")
        self.c = _lib.ReadExtrasC(*[arrays[name].ctypes.data if arrays[name] is not None and arrays[name].size else None for name, _ in self.FIELDS])

    @classmethod
    def from_arrays(cls, qual_first, qual, haplotype, name_key=None):
        given = dict(qual_first=qual_first, qual=qual, haplotype=haplotype, name_key=name_key)
        return cls({name: None if given[name] is None else np.ascontiguousarray(given[name], dtype=dt).reshape(-1) for name, dt in cls.FIELDS})

    @classmethod
    def from_dict(cls, d, names=True):
        """from the dict synthetic.make_read_extras returns, or an .npz; names=False drops the name keys (no duplicate-name filter)"""
        has = names and "name_key" in (d.files if hasattr(d, "files") else d)
        return cls.from_arrays(d["qual_first"], d["qual"], d["haplotype"], d["name_key"] if has else None)

    def __len__(self):
        return len(self.arrays["haplotype"])


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

    def run(self, reads, extras, centres, ref_bytes, ref_first, path=None, **cfg):
        """one call; centres 0-based, strictly ascending.  The result stays in the context (after a device call: the rows on the device)"""
        if not isinstance(reads, ReadSet):
            reads = ReadSet.from_dict(reads)
        if not isinstance(extras, ReadExtras):
            extras = ReadExtras.from_dict(extras)
        if len(extras) != len(reads):
            raise ValueError(f"{len(extras)} extras for {len(reads)} reads")
        path = path or ("host" if self.device is None else "device")
        if path not in ("device", "host"):
            raise ValueError(f"path={path}: expected device or host")
        ref = _ref_array(ref_bytes)
        centres = np.ascontiguousarray(centres, dtype=np.int64).reshape(-1)
        c = config(**cfg)
        L = _lib.lib()
        fn, what = (L.c3_fa_reads, "c3_fa_reads") if path == "device" else (L.c3_fa_reads_host, "c3_fa_reads_host")
        rc = fn(self.h, C.byref(reads.c), C.byref(extras.c), centres.ctypes.data if centres.size else None, len(centres),
                ref.ctypes.data if ref.size else None, int(ref_first), len(ref), C.byref(c))
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
        """dict of the held result: rows (n_rows, 33, 8) int8, counts, depths (n_cand,) int32, text (bytes: one line per candidate)"""
        n_cand, n_rows, text_bytes, _ = self.sizes()
        out = {"rows": np.zeros((n_rows, FA_POSITIONS, FA_CHANNELS), np.int8), "counts": np.zeros(n_cand, np.int32), "depths": np.zeros(n_cand, np.int32)}
        text = C.create_string_buffer(max(text_bytes, 1))
        ptr = [out[k].ctypes.data if out[k].size else None for k in ("rows", "counts", "depths")]
        _lib.check(_lib.lib().c3_fa_reads_result(self.h, *ptr, text), "c3_fa_reads_result")
        out["text"] = text.raw[:text_bytes]
        return out

    def stats(self):
        s = _lib.FaCounters()
        _lib.check(_lib.lib().c3_fa_reads_stats(self.h, C.byref(s)), "c3_fa_reads_stats")
        names = ("staging", "op_table", "candidates", "scan", "fill", "fetch")
        return {"reads_kept": s.reads_kept, "reads_dropped": s.reads_dropped, "rows": s.rows, "deep_windows": s.deep_windows,
                "fell_back": bool(s.fell_back), "on_host": bool(s.on_host), "kernel_ms": dict(zip(names, list(s.kernel_ms)))}


_contexts = {}


def _shared_context(path):
    key = (os.getpid(), path)
    if key not in _contexts:
        _contexts[key] = Context(0 if path == "device" else None)
    return _contexts[key]


def fa_windows(reads, extras, centres, ref_bytes, ref_first, path=None, context=None, **cfg):
    """(rows, counts, depths, alt_info_list) of the candidates at ``centres`` (0-based, strictly ascending, each >= 16).  cfg: DEFAULTS above"""
    path = path or default_path()
    ctx = context or _shared_context(path)
    r = ctx.run(reads, extras, centres, ref_bytes, ref_first, path=path, **cfg).fetch()
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
    for name in ("min_mq", "max_indel_length", "matrix_depth", "seed"):
        ap.add_argument("--" + name, type=int, default=DEFAULTS[name])
    a = ap.parse_args(argv)
    ref = _read_contig(a.ref_fn, a.ctgName)
    with open(a.candidates) as fh:
        centres = np.array([int(line.split()[0]) - 1 for line in fh if line.strip()], np.int64)
    with np.load(a.reads) as z:
        reads, extras = ReadSet.from_dict(z), ReadExtras.from_dict(z)
    path = a.path or default_path()
    cfg = dict(min_mq=a.min_mq, max_indel_length=a.max_indel_length, matrix_depth=a.matrix_depth, seed=a.seed)
    out = {}
    with Context(0 if path == "device" else None) as ctx:
        r = ctx.run(reads, extras, centres, ref, 0, path=path, **cfg).fetch()
        out.update(rows=r["rows"], counts=r["counts"], depths=r["depths"])
        if a.chkpnt_fn:
            import torch
            from .model import Clair3_F
            sd = torch.load(a.chkpnt_fn, map_location="cpu")
            m = Clair3_F(add_indel_length=True, predict=True).to("cuda:0")
            m.eval()
            m.load_state_dict(sd.get("state_dict", sd))
            out["y"] = m.predict_reads(ctx)
    sys.stdout.write(r["text"].decode("ascii"))
    if a.output_fn:
        np.savez(a.output_fn, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
