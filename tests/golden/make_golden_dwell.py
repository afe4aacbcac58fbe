#!/usr/bin/env python3
"""Golden signal lengths of the REAL reference function compute_signal_lengths_from_mv_tag (src/clair3_full_alignment_dwell.c:20-74) for
move tables as the mv:B:c tag holds them (tests/test_dwell.py holds c3_fa_dwell_cum_host to them, tests/test_dwell_gpu.py the table kernel).

Run in the build container only (needs the reference checkout and a C compiler, like make_golden_haplotag.py), never where the GPU tests run:

    python tests/golden/make_golden_dwell.py

At run time, in a temporary directory, the function is cut BY NAME out of the reference's source file, a prelude of this script's own is
put in front (the reference's sam.h cannot be used: its htslib includes are not there; the prelude declares a minimal bam1_t with
core.l_qseq and an aux buffer, and bam_aux_get / bam_auxB_len / bam_auxB2i over that buffer), a main of this script's own that reads a
case file is put behind, and the whole is compiled and run.  Nothing of the reference's text or binaries is written into the repository:
tests/golden/fa_dwell_tables.npz (fa_dwell.npz beside it is the forward pass's golden of the 9-channel model) holds data only -- mv_first /
mv: the tables back to back (element 0 the stride), l: the query length, reverse: the strand, has: 0 where the function returned NULL,
sig_first / sig: its l int32 otherwise.
conditions() counts each kind of table; it is asserted when the file is written.
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "fa_dwell_tables.npz")
MIN_PER_CONDITION = 8
STEP = 4096  # c3_fa_dwell_step(): the entries a step of the table kernel covers

PRELUDE = r"""
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef struct { struct { int32_t l_qseq; } core; uint8_t *aux; } bam1_t;  /* aux: NULL (no tag) or 'B', an int64 count, the int8 values */
static uint8_t *bam_aux_get(const bam1_t *b, const char *tag) { (void)tag; return b->aux; }
static int64_t bam_auxB_len(const uint8_t *s) { int64_t n; memcpy(&n, s + 1, 8); return n; }
static int64_t bam_auxB2i(const uint8_t *s, int64_t i) { return (int8_t)s[9 + i]; }
"""

DRIVER = r"""
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    int64_t n;
    if (!f || !o || fread(&n, 8, 1, f) != 1) return 2;
    for (int64_t i = 0; i < n; ++i) {
        int64_t h[4];  /* L, l, reverse, tagged */
        if (fread(h, 8, 4, f) != 4) return 3;
        uint8_t *aux = calloc(9 + h[0] + 1, 1);
        aux[0] = 'B', memcpy(aux + 1, &h[0], 8);
        if (h[0] && fread(aux + 9, 1, h[0], f) != (size_t)h[0]) return 3;
        bam1_t b;
        b.core.l_qseq = (int32_t)h[1], b.aux = h[3] ? aux : NULL;
        int32_t *sig = compute_signal_lengths_from_mv_tag(&b, h[2] != 0);
        const int64_t has = sig != NULL;
        fwrite(&has, 8, 1, o);
        if (sig) fwrite(sig, 4, h[1], o);
        free(sig), free(aux);
    }
    fclose(f), fclose(o);
    return 0;
}
"""


def cut(source, name):
    """the definition of ``name``: from its line at column 0 to the closing brace at column 0"""
    m = re.search(r"^[A-Za-z_][^\n;{]*\b" + name + r"\s*\([^;{]*\)\s*\{.*?^\}", source, re.S | re.M)
    assert m, f"{name} not found in the reference"
    return m.group(0)


def build(tmp):
    with open(os.path.join(REF, "src", "clair3_full_alignment_dwell.c")) as fh:
        source = fh.read()
    path = os.path.join(tmp, "dwell_ref.c")
    with open(path, "w") as fh:
        fh.write(PRELUDE + cut(source, "compute_signal_lengths_from_mv_tag") + DRIVER)
    exe = os.path.join(tmp, "dwell_ref")
    subprocess.check_call(["gcc", "-O1", "-w", path, "-o", exe])
    return exe


def table(rng, L, density, values=(1,), lead=0):
    """L entries: the stride, ``lead`` zeros, then moves with the given density"""
    mv = np.where(rng.random(L) < density, rng.choice(values, size=L), 0).astype(np.int8)
    if L:
        mv[0] = rng.choice((0, 5))  # (the stride: zero or not, it must not count)
    mv[1:1 + lead] = 0
    return mv


def cases():
    """(mv, l, reverse, tagged) per table"""
    rng = np.random.default_rng(20240)
    out = []
    for i in range(16):  # the shortest tables, with and without the tag
        for L in (0, 1, 2):
            out.append((table(rng, L, 0.7), int(rng.integers(0, 6)) + (i % 4 == 0), i % 2, not (L == 0 and i % 4 < 2)))
    for i in range(12):  # a query of no bases
        out.append((table(rng, int(rng.integers(2, 40)), 0.5), 0, i % 2, True))
    for i in range(16):  # no move at all behind the stride
        mv = table(rng, int(rng.integers(3, 60)), 0.0)
        out.append((mv, int(rng.integers(1, 14)), i % 2, True))
    for i in range(170):  # random tables: every relation of K and l, values other than 1, zeros in front
        L = int(rng.integers(3, 60))
        mv = table(rng, L, rng.choice((0.1, 0.3, 0.5, 0.9)), values=((1,), (1, -1, 5), (-128, 127, 2))[i % 3], lead=int(rng.integers(0, 4)))
        k = int(np.count_nonzero(mv[1:]))
        l = max(k + (i % 3 - 1) * int(rng.integers(1, 4)), 1) if i % 4 else int(rng.integers(1, 14))
        out.append((mv, l, i % 2, True))
    for i, L in enumerate(sorted((STEP - 1, STEP, STEP + 1, STEP + 15, STEP + 16, STEP + 17, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1, 2 * STEP + 17) * 2)):
        mv = table(rng, L, 0.45, values=(1, -1) if i % 2 else (1,), lead=i % 3)
        k = int(np.count_nonzero(mv[1:]))
        out.append((mv, k + (i % 3 - 1), i % 2, True))
    return out


def run_reference(exe, tmp, cs):
    case, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as fh:
        np.array([len(cs)], np.int64).tofile(fh)
        for mv, l, reverse, tagged in cs:
            np.array([len(mv), l, reverse, tagged], np.int64).tofile(fh)
            mv.tofile(fh)
    subprocess.check_call([exe, case, out])
    raw = open(out, "rb").read()
    has, sigs, at = [], [], 0
    for mv, l, reverse, tagged in cs:
        h = int(np.frombuffer(raw[at:at + 8], np.int64)[0])
        at += 8
        has.append(h)
        sigs.append(np.frombuffer(raw[at:at + 4 * l * h], np.int32).copy())
        at += 4 * l * h
    assert at == len(raw)
    return np.array(has, np.uint8), sigs


def conditions(cs, has, sigs):
    c = dict.fromkeys(("L0", "L1", "L2", "untagged", "l0", "all_zero", "k_below_l", "k_equals_l", "k_above_l", "forward", "reverse", "other_values",
                       "zeros_in_front", "one_step", "two_steps", "no_table", "table"), 0)
    for (mv, l, reverse, tagged), h, sig in zip(cs, has, sigs):
        L, k = len(mv), int(np.count_nonzero(mv[1:]))
        c["no_table" if not h else "table"] += 1
        assert h == (tagged and L > 1 and l > 0)
        for name, hit in (("L0", L == 0), ("L1", L == 1), ("L2", L == 2), ("untagged", not tagged), ("l0", l == 0 and L > 1)):
            c[name] += hit
        if not h:
            continue
        c["all_zero"] += k == 0
        c["k_below_l"] += 0 < k < l
        c["k_equals_l"] += k == l
        c["k_above_l"] += k > l
        c["reverse" if reverse else "forward"] += 1
        c["other_values"] += bool(np.isin(mv[1:], (0, 1), invert=True).any())
        c["zeros_in_front"] += k > 0 and mv[1] == 0
        c["one_step"] += abs(L - STEP) <= 17
        c["two_steps"] += abs(L - 2 * STEP) <= 17
        assert len(sig) == l and (k == 0) == (not sig.any())
    return c


def main():
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        has, sigs = run_reference(build(tmp), tmp, cs)
    total = conditions(cs, has, sigs)
    print(len(cs), "tables", total)
    short = {name: n for name, n in total.items() if n < MIN_PER_CONDITION}
    assert not short, f"conditions that occur fewer than {MIN_PER_CONDITION} times: {short}"
    np.savez_compressed(OUT, mv_first=np.concatenate([[0], np.cumsum([len(c[0]) for c in cs])]).astype(np.int64),
                        mv=np.concatenate([c[0] for c in cs]), l=np.array([c[1] for c in cs], np.int64),
                        reverse=np.array([c[2] for c in cs], np.uint8), tagged=np.array([c[3] for c in cs], np.uint8), has=has,
                        sig_first=np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64),
                        sig=np.concatenate(sigs).astype(np.int32))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 100_000


if __name__ == "__main__":
    main()
