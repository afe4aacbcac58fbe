"""c3_vcf_rows (csrc/c3_rows.h) on decoder columns that are not whole numbers it can cast: the class column of the reference base and
the entry column of the class are floats the device wrote, and a NaN row, an infinity or a value beyond int range must send the row back
to the Python path (status 1) instead of reaching an (int) cast, which is undefined behaviour.  Plain host code of libc3hip.so: no GPU and
no reference checkout needed (the configuration is filled in by hand with the reference's constants)."""
import ctypes as C

import numpy as np
import pytest

from clair3_amd import _lib
from clair3_amd import decode as dec

WIDTH = 24  # pileup rows without indel heads
FLANK = 16  # shared/param_p.py flankingBaseNum
CLS_COL = 23  # decoder column of the class for reference base A (+ base index)
POS_COL = 13  # decoder column of the entry of class 1 (+ class - 1)


def _config():
    cf = _lib.RowsConfig()
    cf.width, cf.flank, cf.show_reference, cf.keep_iupac = WIDTH, FLANK, 1, 0
    cf.has_qs_pass, cf.qs_pass = 0, 0.0
    cf.pileup, cf.max_len, cf.infer = 1, dec.MAX_LEN, 5
    cf.phred_trans = -10.0 / np.log(10.0)  # CallVariants.Phred_Trans
    cf.f32_arith = int((1.0 - np.float32(0.25)).dtype == np.float32)
    cf.walk, cf.gvcf, cf.haploid, cf.long_indel = 1, 0, 0, 0
    for k, g in enumerate(("0/0", "1/1", "0/1", "1/2")):
        cf.gt[k].value = g.encode()
    return cf


def _rows(n):
    """n reference calls (class 0) at reference base A: every one printable by the C pass"""
    seq = "C" * FLANK + "A" + "G" * FLANK
    pos = [f"chr1:{1000 + 7 * i}:{seq}" for i in range(n)]
    alt = [f"{30 + i}-XC 2 XG 1" for i in range(n)]
    y = np.zeros((n, WIDTH + dec.DECODE_COLS), np.float32)
    y[:, :WIDTH] = np.linspace(0.01, 0.9, WIDTH, dtype=np.float32)
    cols = y[:, WIDTH:]
    cols[:, 0:9] = np.arange(9, dtype=np.float32)[None, :] / 16 + 0.01  # nine distinct maxima
    cols[:, 9:13] = 0.97
    cols[:, 13:22] = 0.0
    cols[:, 23:27] = 0.0  # class 0 whatever the base
    return pos, alt, y


def _print(cf, pos, alt, y):
    L = _lib.lib()
    n = len(pos)
    pos_b = b"\0".join(p.encode() for p in pos)
    alt_b = b"\0".join(a.encode() for a in alt)
    cap = 256 * n + 4096
    out = np.zeros(cap, np.uint8)
    off = np.zeros(n + 1, np.int64)
    status = np.full(n, 255, np.uint8)
    y = np.ascontiguousarray(y)
    rc = L.c3_vcf_rows(C.byref(cf), n, pos_b, len(pos_b), alt_b, len(alt_b), y.ctypes.data, y.shape[1], out.ctypes.data, cap,
                       off.ctypes.data, status.ctypes.data)
    assert rc == 0, _lib.last_error()
    text = out[: int(off[n])].tobytes().decode("ascii")
    return [text[off[i]:off[i + 1]] for i in range(n)], status.tolist()


BAD = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9]


@pytest.mark.parametrize("column", ["class", "entry"])
def test_non_finite_decoder_columns_are_handed_back(column):
    cf = _config()
    n = 2 * len(BAD) + 1
    pos, alt, y = _rows(n)
    texts0, status0 = _print(cf, pos, alt, y)
    assert status0 == [0] * n and all(t.startswith("chr1\t") for t in texts0), (status0, texts0[:2])
    poisoned = list(range(1, n, 2))  # every other row; its neighbours stay ordinary
    for i, v in zip(poisoned, BAD):
        y[i, WIDTH + (CLS_COL if column == "class" else POS_COL)] = v
    texts, status = _print(cf, pos, alt, y)
    for i in range(n):
        if i in poisoned:
            assert status[i] == 1 and texts[i] == "", (i, y[i, WIDTH + CLS_COL], y[i, WIDTH + POS_COL], status[i], texts[i])
        else:
            assert status[i] == 0 and texts[i] == texts0[i], (i, status[i], texts[i], texts0[i])


def test_out_of_range_class_columns_are_handed_back():
    """classes below 0 or above 9 were handed back before the cast was guarded: they still are, finite or not"""
    cf = _config()
    pos, alt, y = _rows(4)
    y[1, WIDTH + CLS_COL] = -1.0
    y[2, WIDTH + CLS_COL] = 10.0
    texts, status = _print(cf, pos, alt, y)
    assert status == [0, 1, 1, 0] and texts[1] == texts[2] == ""
