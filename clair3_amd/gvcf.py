"""gVCF mode: the <NON_REF> block records of the reference's --gvcf from the per-site counts of the pileup step (csrc/c3_gvcf.h;
preprocess/utils.py variantInfoCalculator, preprocess/CreateTensorPileupFromCffi.py:399-441).

    blocks_from_counts(n_ref, n_total, ref_bytes, first_pos)        records (synthetic.GVCF_BLOCK_DTYPE) from pos_ref_count / pos_total_count
    blocks_from_region(region, major, ref_bytes, first_major, ...)  the same from the region matrix of calculate_clair3_pileup
    text(blocks, ctg_name, contig_len, first_pos, n_sites)          the lines of write_to_gvcf
    install()                                                       rebinds preprocess.utils.variantInfoCalculator (below)

    python -m clair3_amd.gvcf --counts X.npz --ref_fn ref.fa --ctgName chr20 [--ctgStart P] [--output_fn F] [--bp_resolution]
                              [--base_err 0.001] [--gq_bin_size 5]
                              [--with_ctg_end] [--path device|host]
        X.npz: n_ref, n_total (one entry per site), optionally first_pos (default --ctgStart, else 1).  The lines go to --output_fn or stdout.
        The empty-pileup rule looks at the sites given; the reference's check also reads the site at ctgEnd, which its loop does not
        walk: with --with_ctg_end the file's last entry is that site.

``path``: "device" runs the kernels, "host" the sequential C rule (no GPU needed); None reads $C3HIP_GVCF, whose default is "device" where a
GPU is visible and "host" otherwise.  Both give the same records.  Limits: one contig per call, depths up to 65535.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _lib
from . import synthetic as syn

BLOCK_DTYPE = syn.GVCF_BLOCK_DTYPE
assert BLOCK_DTYPE.itemsize == C.sizeof(_lib.GvcfBlock) == 48


def default_path():
    """$C3HIP_GVCF (device | host); unset: device where a GPU is visible, host otherwise.  Asking whether one is visible initialises the HIP
    runtime in this process: a run that fans out into many producer processes should set the variable explicitly"""
    v = os.environ.get("C3HIP_GVCF")
    if v is not None:
        if v not in ("device", "host"):
            raise ValueError(f"C3HIP_GVCF={v}: expected device or host")
        return v
    try:
        return "device" if _lib.device_count() > 0 else "host"
    except _lib.C3Error:
        return "host"


def _config(base_err, gq_bin_size, bp_resolution):
    return _lib.GvcfConfig(float(base_err), int(gq_bin_size), 1 if bp_resolution else 0)


def _ref_array(ref_bytes, n):
    ref = np.frombuffer(ref_bytes.encode() if isinstance(ref_bytes, str) else bytes(ref_bytes), dtype=np.uint8) \
        if isinstance(ref_bytes, (str, bytes, bytearray)) else np.ascontiguousarray(ref_bytes, dtype=np.uint8)
    if ref.shape != (n,):
        raise ValueError(f"{n} sites need {n} reference bytes, {ref.shape} given")
    return ref


def _counts_arrays(n_ref, n_total):
    n_ref, n_total = np.asarray(n_ref), np.asarray(n_total)
    dt = np.int32 if n_ref.dtype == np.int32 and n_total.dtype == np.int32 else np.int64
    n_ref, n_total = np.ascontiguousarray(n_ref, dtype=dt), np.ascontiguousarray(n_total, dtype=dt)
    if n_ref.ndim != 1 or n_ref.shape != n_total.shape:
        raise ValueError("n_ref and n_total: two one-dimensional arrays of one length")
    return n_ref, n_total, (_lib.DTYPE_I32 if dt == np.int32 else _lib.DTYPE_I64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _call(fn, what, n_sites, max_blocks=None):
    """one call of a blocks entry.  The records of a call cannot outnumber its sites, so without ``max_blocks`` the buffer holds n_sites
    records (untouched pages of it cost nothing) and the call never has to be made twice; with it, records that do not fit are an error"""
    cap = int(max_blocks) if max_blocks is not None else int(n_sites)
    out = np.zeros(cap, dtype=BLOCK_DTYPE)
    n = C.c_int64(0)
    rc = fn(_ptr(out), cap, C.byref(n))
    if rc == _lib.GVCF_MORE:
        raise _lib.C3Error(f"{what}: {n.value} records do not fit max_blocks = {cap}")
    if rc != 0:
        raise _lib.C3Error(f"{what}: {_lib.last_error()}")
    return out[:n.value] if 2 * n.value >= cap else out[:n.value].copy()  # (a short answer does not keep the long buffer alive)


class Context:
    """c3_gvcf_create: a device context (a stream, workspaces, the table of site records); use one per process and keep it"""

    def __init__(self, device=0, base_err=0.001, gq_bin_size=5, bp_resolution=False):
        self.cfg = _config(base_err, gq_bin_size, bp_resolution)
        self.h = None
        self._destroy = _lib.lib().c3_gvcf_destroy
        self.pid = os.getpid()
        self.h = _lib.lib().c3_gvcf_create(int(device), C.byref(self.cfg))
        if not self.h:
            raise _lib.C3Error(f"c3_gvcf_create: {_lib.last_error()}")

    def close(self):
        if self.h:
            self._destroy(self.h)
            self.h = None

    def __del__(self):  # (at interpreter shutdown the module's globals may be gone: the bound function was kept at creation)
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def blocks_from_counts(self, n_ref, n_total, ref_bytes, first_pos=1, max_blocks=None):
        n_ref, n_total, dt = _counts_arrays(n_ref, n_total)
        ref = _ref_array(ref_bytes, len(n_total))
        L = _lib.lib()
        return _call(lambda out, cap, n: L.c3_gvcf_blocks_counts(self.h, _ptr(n_ref), _ptr(n_total), dt, _ptr(ref), len(n_total), int(first_pos), out, cap, n),
                     "c3_gvcf_blocks_counts", len(n_total), max_blocks)

    def blocks_from_region(self, region, major, ref_bytes, first_major, n_sites, first_pos=1, max_blocks=None):
        region = np.asarray(region)
        dt = np.int32 if region.dtype == np.int32 else np.int64
        region = np.ascontiguousarray(region, dtype=dt)
        major = np.ascontiguousarray(major, dtype=np.int64)
        if region.ndim != 2 or region.shape[1] != syn.PILEUP_CHANNELS or major.shape != (len(region),):
            raise ValueError("region (n_cols, 18) and major (n_cols,) expected")
        ref = _ref_array(ref_bytes, int(n_sites))
        L = _lib.lib()
        x_dtype = _lib.DTYPE_I32 if dt == np.int32 else _lib.DTYPE_I64
        return _call(lambda out, cap, n: L.c3_gvcf_blocks_region(self.h, _ptr(region), x_dtype, len(region), _ptr(major), _ptr(ref), int(first_major),
                                                                 int(n_sites), int(first_pos), out, cap, n),
                     "c3_gvcf_blocks_region", int(n_sites), max_blocks)


def blocks_host(n_ref, n_total, ref_bytes, first_pos=1, base_err=0.001, gq_bin_size=5, bp_resolution=False, max_blocks=None):
    """c3_gvcf_blocks_host: the sequential rule in C, no GPU"""
    n_ref, n_total, dt = _counts_arrays(n_ref, n_total)
    ref = _ref_array(ref_bytes, len(n_total))
    cfg = _config(base_err, gq_bin_size, bp_resolution)
    L = _lib.lib()
    return _call(lambda out, cap, n: L.c3_gvcf_blocks_host(C.byref(cfg), _ptr(n_ref), _ptr(n_total), dt, _ptr(ref), len(n_total), int(first_pos), out, cap, n),
                 "c3_gvcf_blocks_host", len(n_total), max_blocks)


_contexts = {}


def _context(device, base_err, gq_bin_size, bp_resolution):
    """the process's context of a configuration.  A forked child of a process that already opened the GPU cannot open it again (and must
    not use the parent's handle): that is refused here, with the way out"""
    pid = os.getpid()
    if any(c.pid != pid for c in _contexts.values()):
        raise _lib.C3Error("gvcf: this process was forked from one that holds a GPU context: use path='host' (C3HIP_GVCF=host) here, or start "
                           "the workers before the first device call")
    key = (int(device), float(base_err), int(gq_bin_size), bool(bp_resolution))
    if key not in _contexts:
        _contexts[key] = Context(device, base_err, gq_bin_size, bp_resolution)
    return _contexts[key]


def blocks_from_counts(n_ref, n_total, ref_bytes, first_pos=1, base_err=0.001, gq_bin_size=5, bp_resolution=False, path=None, device=0):
    if (path or default_path()) == "host":
        return blocks_host(n_ref, n_total, ref_bytes, first_pos, base_err, gq_bin_size, bp_resolution)
    return _context(device, base_err, gq_bin_size, bp_resolution).blocks_from_counts(n_ref, n_total, ref_bytes, first_pos)


def blocks_from_region(region, major, ref_bytes, first_major, n_sites, first_pos=1, base_err=0.001, gq_bin_size=5, bp_resolution=False,
                       path=None, device=0):
    if (path or default_path()) == "host":
        n_ref, n_total = syn.gvcf_region_counts(region, major, _ref_array(ref_bytes, int(n_sites)), first_major, int(n_sites))
        return blocks_host(n_ref, n_total, ref_bytes, first_pos, base_err, gq_bin_size, bp_resolution)
    return _context(device, base_err, gq_bin_size, bp_resolution).blocks_from_region(region, major, ref_bytes, first_major, n_sites, first_pos)


def site(n_ref, n_total, ref_byte="A", base_err=0.001, gq_bin_size=5):
    """c3_gvcf_site: (gq, binned_gq, validPL, PL0, PL1, PL2)"""
    out = (C.c_int32 * 6)()
    cfg = _config(base_err, gq_bin_size, False)
    b = ref_byte if isinstance(ref_byte, int) else ord(ref_byte)
    _lib.check(_lib.lib().c3_gvcf_site(C.byref(cfg), int(n_ref), int(n_total), b, out), "c3_gvcf_site")
    return tuple(out)


def site_table(depth, base_err=0.001, gq_bin_size=5):
    """c3_gvcf_site_table: (pairs, 6) int32, pair (n_total, n_ref) at n_total * (n_total + 1) // 2 + n_ref"""
    out = np.zeros(((depth + 1) * (depth + 2) // 2, 6), dtype=np.int32)
    cfg = _config(base_err, gq_bin_size, False)
    _lib.check(_lib.lib().c3_gvcf_site_table(C.byref(cfg), int(depth), _ptr(out)), "c3_gvcf_site_table")
    return out


def text(blocks, ctg_name, contig_len=0, first_pos=1, n_sites=0):
    """c3_gvcf_text: the lines of write_to_gvcf as bytes.  n_sites > 0 turns the empty-pileup rule on: where every record has max_dp 0,
    the one line of write_empty_pileup for first_pos .. first_pos + n_sites stands in their place"""
    blocks = np.ascontiguousarray(blocks, dtype=BLOCK_DTYPE)
    L = _lib.lib()
    need = C.c_int64(0)
    cap = 96 * len(blocks) + 256
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        rc = L.c3_gvcf_text(_ptr(blocks), len(blocks), str(ctg_name).encode(), int(contig_len), int(first_pos), int(n_sites), buf, cap, C.byref(need))
        if rc == 0:
            return buf.raw[:need.value]
        if rc != _lib.GVCF_MORE:
            raise _lib.C3Error(f"c3_gvcf_text: {_lib.last_error()}")
        cap = need.value
    raise _lib.C3Error("c3_gvcf_text: the size changed between two calls")


# ------------------------------------------------------------------------------------------ the drop-in
def install(path=None, device=0):
    """Rebind preprocess.utils.variantInfoCalculator (the reference's package must be importable) with a subclass whose make_gvcf_online only
    records (pos, ref, n_ref, n_total) and whose closing write_to_gvcf_batch / close_vcf_writer answer through the library: the file is
    the one the reference writes.  Header, the lz4 writer and write_empty_pileup stay the reference's.  Returns the subclass.

    The reference starts one producer process per chunk: with path "device" every one of them opens the GPU.  Where more processes than a
    shared machine allows would hold it at once, use path "host" (or C3HIP_GVCF=host), or route the chunks through fewer processes."""
    import preprocess.utils as ref_utils
    base = ref_utils.variantInfoCalculator
    if getattr(base, "_c3hip_gvcf", False):
        return base
    chosen = path

    class variantInfoCalculator(base):
        _c3hip_gvcf = True
        _c3hip_base = base

        def __init__(self, *a, **k):
            self._sites = []
            self._pending = [None]  # what the producer finds in current_block while sites wait: it then calls write_to_gvcf_batch
            super().__init__(*a, **k)

        def make_gvcf_online(self, variant_summary, push_current=False):
            if push_current:
                self._answer()
                return
            s = variant_summary
            if self._sites and s["chr"] != self._sites[-1][0]:
                self._answer()
            self._sites.append((s["chr"], s["pos"], s["ref"], s["n_ref"], s["n_total"]))
            self.current_block = self._pending

        def write_to_gvcf_batch(self, block, block_min_dp, block_min_raw_gq):
            if block is self._pending:
                self._answer()
            else:
                super().write_to_gvcf_batch(block, block_min_dp, block_min_raw_gq)

        def close_vcf_writer(self):
            self._answer()
            if self.CW is not None:
                super().close_vcf_writer()

        def _answer(self):
            sites, self._sites, self.current_block = self._sites, [], []
            if not sites:
                return
            ctg = sites[0][0]
            pos = np.array([s[1] for s in sites], dtype=np.int64)
            ref = np.frombuffer("".join((s[2] if len(s[2]) == 1 else "N") for s in sites).encode("latin-1"), dtype=np.uint8)
            n_ref = np.array([s[3] for s in sites], dtype=np.int64)
            n_total = np.array([s[4] for s in sites], dtype=np.int64)
            b = blocks_from_counts(n_ref, n_total, ref, 0, self.p_error, self.gq_bin_size, self.bp_resolution, path=chosen, device=device).copy()
            b["pos"], b["end"] = pos[b["pos"]], pos[b["end"]]  # (records are made over site indices: positions need not be consecutive)
            self.vcf_writer.write(text(b, ctg, self.contig_length_dict.get(ctg, 0)).decode("latin-1"))

    variantInfoCalculator.__qualname__ = variantInfoCalculator.__name__ = "variantInfoCalculator"
    ref_utils.variantInfoCalculator = variantInfoCalculator
    return variantInfoCalculator


def uninstall():
    """put the reference's own class back"""
    import preprocess.utils as ref_utils
    cur = ref_utils.variantInfoCalculator
    if getattr(cur, "_c3hip_gvcf", False):
        ref_utils.variantInfoCalculator = cur._c3hip_base


# ------------------------------------------------------------------------------------------ the command line
def read_contig(ref_fn, ctg_name):
    """the bytes of one contig of a FASTA file, as they stand (case kept)"""
    seq, on = [], False
    with open(ref_fn, "rb") as fh:
        for line in fh:
            if line.startswith(b">"):
                if on:
                    break
                on = line[1:].split()[0].decode() == ctg_name if line[1:].split() else False
            elif on:
                seq.append(line.strip())
    if not on and not seq:
        raise ValueError(f"{ref_fn}: no contig {ctg_name}")
    return b"".join(seq)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="gVCF non-variant block lines from per-site counts")
    ap.add_argument("--counts", required=True, help=".npz with n_ref, n_total and optionally first_pos")
    ap.add_argument("--ref_fn", required=True)
    ap.add_argument("--ctgName", required=True)
    ap.add_argument("--ctgStart", type=int, default=None)
    ap.add_argument("--output_fn", default=None)
    ap.add_argument("--base_err", type=float, default=0.001)
    ap.add_argument("--gq_bin_size", type=int, default=5)
    ap.add_argument("--bp_resolution", action="store_true")
    ap.add_argument("--path", choices=("device", "host"), default=None)
    ap.add_argument("--with_ctg_end", action="store_true",
                    help="the file's last entry is the site at ctgEnd: the producer's empty-pileup check reads it, its loop does not walk it")
    a = ap.parse_args(argv)
    z = np.load(a.counts)
    n_ref, n_total = z["n_ref"], z["n_total"]
    # the producer sums the totals of ctgStart .. ctgEnd for its empty check but walks ctgStart .. ctgEnd - 1 (:413-421)
    extra = int(n_total[-1]) if a.with_ctg_end and len(n_total) else 0
    if a.with_ctg_end:
        n_ref, n_total = n_ref[:-1], n_total[:-1]
    first = int(a.ctgStart if a.ctgStart is not None else z["first_pos"] if "first_pos" in z.files else 1)
    contig = read_contig(a.ref_fn, a.ctgName)
    n = len(n_total)
    if first < 1 or first - 1 + n > len(contig):
        raise SystemExit(f"sites {first} .. {first + n - 1} do not lie in {a.ctgName} ({len(contig)} bases)")
    ref = contig[first - 1:first - 1 + n]
    b = blocks_from_counts(n_ref, n_total, ref, first, a.base_err, a.gq_bin_size, a.bp_resolution, path=a.path)
    out = text(b, a.ctgName, len(contig), first, n if extra == 0 else 0)
    if a.output_fn:
        with open(a.output_fn, "wb") as fh:
            fh.write(out)
    else:
        sys.stdout.buffer.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
