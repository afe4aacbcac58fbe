#!/usr/bin/env python3
"""Golden windows and rows for full-alignment windows handed over as their occupied read rows (csrc/c3_expand.h): ragged windows written
as the reference's stream lines, padded to the matrix depth by the REAL reference generator, rows by the REAL reference module.

Run in the build container only (needs the reference checkout, like make_golden.py):

    python tests/golden/make_golden_fa_rows.py

Every window is a run of read rows drawn with clair3_amd/synthetic.py make_fa_windows; its rows go into one line of the stream format
(``chrom\\tcoord\\tseq\\ttensor\\talt_info``, the tensor as space-separated integers) and the lines through the reference's own
``clair3.utils.tensor_generator_from("PIPE", ...)`` with sys.stdin replaced -- the statement that pads a window with
``prefix = int(padding_depth / 2)`` zero rows in front and the rest behind (clair3/utils.py:113-121).  The padded tensor then goes through
the reference Clair3_F in fp32 on the CPU with one thread.  Stored: the ragged rows, the counts, the padded tensor, the rows of
probabilities, seeds and digests -- tests/golden/fa_rows.npz (8 channels, 89 rows, plus a 55-row set padded with platform='hifi': padded
tensor only) and fa_rows_dwell.npz (9 channels).  The conditions a label comparison rests on are asserted here and again by
tests/test_fa_rows.py.
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from clair3_amd import synthetic as syn  # noqa: E402

# read rows per window: no read, one, an odd and an even padding (89 - 10 = 79, 89 - 44 = 45, 89 - 45 = 44, 89 - 61 = 28), depth - 1, depth
COUNTS_89 = [0, 1, 10, 44, 88, 89, 2, 45, 30, 61]
COUNTS_55 = [0, 1, 10, 21, 54, 55]
INPUT_SEED = 8101
MIN_GAP = 1e-5  # smallest distance between a head's top two reference probabilities the fixture accepts
HEAD_SLICES = ((0, 21), (21, 24), (24, 57), (57, 90))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def sd_digest(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


def ragged_rows(counts, channels, seed):
    """(rows int8 (sum(counts), 33, C), counts int32): window i takes counts[i] rows from row i on out of a pool of read rows of the
    realistic recipe -- the windows overlap in their reads, which keeps the compressed fixture small, and differ in where their runs sit"""
    pool, _, _ = syn.pack_fa_rows(syn.make_fa_windows(4, seed=seed, channels=channels))
    pool = pool[(pool != 0).any(axis=(1, 2))]  # (interior rows of a run are reads too: none is empty in this recipe)
    assert len(pool) >= max(counts) + len(counts)
    rows = np.concatenate([pool[i:i + c] for i, c in enumerate(counts)])
    assert (rows != 0).any(axis=(1, 2)).all()
    return rows, np.array(counts, dtype=np.int32)


def stream_lines(rows, counts):
    """the windows as lines of the reference's tensor stream (what CreateTensorFullAlignment prints and the generator splits at tabs)"""
    seq = "ACGT" * 8 + "A"  # 33 reference bases; seq[flankingBaseNum] must be a base (clair3/utils.py:132)
    lines, at = [], 0
    for i, c in enumerate(counts):
        tensor = " ".join(str(int(v)) for v in rows[at:at + c].ravel())
        lines.append("\t".join(("chr1", str(1000 + i), seq, tensor, f"{int(c)}-")) + "\n")
        at += c
    return lines


def reference_pad(lines, platform, dwell):
    """clair3.utils.tensor_generator_from in PIPE mode with sys.stdin replaced"""
    sys.path.insert(0, REF)
    from clair3 import utils
    stdin = sys.stdin
    sys.stdin = io.StringIO("".join(lines))
    try:
        out = [X.copy() for X, _, _ in utils.tensor_generator_from("PIPE", len(lines), False, platform, enable_dwell_time=dwell)]
    finally:
        sys.stdin = stdin
    x = np.concatenate(out)
    assert x.dtype == np.int8 and len(x) == len(lines)
    return x


def top_two_gap(y):
    gap = np.inf
    for lo, hi in HEAD_SLICES:
        if lo >= y.shape[1]:
            break
        s = np.sort(y[:, lo:hi], axis=1)
        gap = min(gap, float((s[:, -1] - s[:, -2]).min()))
    return gap


def conditions(counts, depth):
    """what the fixture promises about its counts"""
    pads = depth - np.asarray(counts)
    assert {0, 1, depth - 1, depth} <= set(int(c) for c in counts)
    assert (pads[(pads > 0) & (pads < depth)] % 2 == 1).any() and (pads[(pads > 0) & (pads < depth)] % 2 == 0).any()
    assert len(counts) <= 32


def reference_rows(sd, indel, channels, x):
    import torch
    sys.path.insert(0, REF)
    from clair3.model import Clair3_F
    torch.set_num_threads(1)
    m = Clair3_F(add_indel_length=indel, predict=True, input_channels=channels)
    m.eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    with torch.inference_mode():
        return m(torch.from_numpy(x)).detach().cpu().numpy().astype(np.float32), torch.__version__


def main():
    for name, channels, first_seed in (("fa_rows", 8, 8200), ("fa_rows_dwell", 9, 8300)):
        rows, counts = ragged_rows(COUNTS_89, channels, INPUT_SEED + channels)
        conditions(counts, 89)
        x = reference_pad(stream_lines(rows, counts), "ont", channels == 9)
        assert x.shape == (len(counts), 89, 33, channels)
        assert np.array_equal(x, syn.pad_fa_rows(rows, counts, depth=89))
        for seed in range(first_seed, first_seed + 20):  # re-draw the weights while a head's top two are a near-tie somewhere
            sd = syn.make_state_dict(syn.FULL_ALIGNMENT, channels, True, seed=seed)
            y, torch_version = reference_rows(sd, True, channels, x)
            gap = top_two_gap(y)
            print(f"{name}: weight seed {seed}: smallest top-two gap {gap:.2e}")
            if gap >= MIN_GAP and np.isfinite(y).all():
                break
        else:
            raise SystemExit("no weight seed without a near-tie")
        meta = dict(kind=syn.FULL_ALIGNMENT, channels=channels, add_indel_length=True, weight_seed=seed, input_seed=INPUT_SEED + channels,
                    depth=89, batch=len(counts), top_two_gap=gap, rows_sha=digest(rows), counts_sha=digest(counts), x_sha=digest(x),
                    sd_sha=sd_digest(sd), y_sha=digest(y), torch=torch_version)
        out = dict(rows=rows, counts=counts, x=x, y_ref=y)
        if channels == 8:  # the 55-row matrix of hifi / ilmn (shared/param_f.py:11): padded tensor only, its rows come from the dense entry
            rows55, counts55 = ragged_rows(COUNTS_55, 8, INPUT_SEED + 55)
            conditions(counts55, 55)
            x55 = reference_pad(stream_lines(rows55, counts55), "hifi", False)
            assert x55.shape == (len(counts55), 55, 33, 8)
            out.update(rows55=rows55, counts55=counts55, x55=x55)
            meta.update(rows55_sha=digest(rows55), x55_sha=digest(x55))
        out["meta"] = np.array(json.dumps(meta))
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {len(counts)} windows, {int(counts.sum())} rows, gap {gap:.2e}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
