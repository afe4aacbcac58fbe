#!/usr/bin/env python3
"""Fixtures of score mode: what the REAL reference loss (clair3/Train.py:87-107 FocalLoss) and its validation pass (:210-257 _run_epoch with
train=False) give on committed reference rows and seeded labels.

Run in the build container only (needs the reference checkout, like make_golden.py):

    python tests/golden/make_golden_score.py

clair3.Train imports h5py at its top; nothing of it is used here, so empty stand-in modules for h5py, hdf5plugin and tables are placed in
sys.modules before the import.  Nothing of the reference is copied: its classes are imported and run.

Per case -- the committed rows ``y_ref`` of four golden cases and one case of hand-made rows (p = 0, 1, 1e-12, NaN, +-inf, ties in the
arg-max) -- tests/golden/score_<case>.npz holds:
  labels        (B, nout) int8 one-hot per task: half of the windows carry the row's arg-max, half a random class (small true-class
                probabilities occur)
  eln, weights  one seeded effective_label_num (nout,) and the class weights the reference's FocalLoss derives from it (nout,) float32
  loss_ref, loss_ref_w   (B, tasks) float32: FocalLoss.forward per window and task, without / with the weights
  epoch_ref, epoch_ref_w what _run_epoch(train=False) returns for the case cut into batches of 7 windows (a stand-in module that returns
                the recorded rows), without / with the weights
  loss_f64, loss_f64_w   (B, tasks) float64: the same formula on the same rows evaluated in numpy float64 (clamped in float32 as the
                reference clamps)
  rows          only the hand-made case: its rows
"""
import os
import sys
import types

import numpy as np

REF = os.environ.get("CLAIR3_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("pileup_realistic", "pileup_indel_heads", "fa_realistic", "fa_no_indel_heads")
HEADS = ((0, 21), (21, 24), (24, 57), (57, 90))
EPOCH_BATCH = 7


def heads(nout):
    return [h for h in HEADS if h[0] < nout]


def handmade_rows(rng):
    """(rows (B, 90) float32, labels (B, 90) int8): the corners of the rule, the same treatment in every task"""
    B = 14
    rows = np.zeros((B, 90), np.float32)
    labels = np.zeros((B, 90), np.int8)
    for lo, hi in HEADS:
        n = hi - lo
        soft = rng.random((B, n)).astype(np.float32) ** 4
        soft /= soft.sum(1, keepdims=True)
        r = soft.copy()
        true = rng.integers(0, n, size=B)
        r[0] = 0.0; r[0, true[0]] = 1.0                       # p = 1 at the true class: a zero term
        r[1, true[1]] = 0.0                                     # p = 0 at the true class: -ln(1e-9f)
        r[2, true[2]] = 1e-12                                   # below the clamp
        r[3] = np.nan                                           # a NaN row
        r[4, (true[4] + 1) % n] = np.nan                        # one NaN beside the true class
        r[5] = 0.01; r[5, [1, 2]] = 0.4; true[5] = 1            # a tie in the arg-max, the label on the lower index: counts as correct
        r[6] = 0.01; r[6, [1, 2]] = 0.4; true[6] = 2            # ... on the higher index: does not
        r[7, (true[7] + 1) % n] = np.inf                        # +inf clamps to 1
        r[8, true[8]] = -np.inf                                 # -inf clamps to 1e-9f
        r[9, true[9]] = 1.0 + 2.0 ** -20                        # just above 1
        r[10, true[10]] = np.float32(1e-9)                      # the clamp itself
        rows[:, lo:hi] = r
        labels[np.arange(B), lo + true] = 1
    return rows, labels


def f64_losses(rows, labels, weights, gamma=2):
    q = np.minimum(np.maximum(rows, np.float32(1e-9)), np.float32(1.0))
    q = np.where(np.isnan(rows), np.float32(np.nan), q).astype(np.float64)
    y = labels.astype(np.float64)
    with np.errstate(invalid="ignore"):
        t = (-y * np.log(q)) * ((1.0 - q) ** gamma * y)
        if weights is not None:
            t = t * weights.astype(np.float64)[None, :]
        return np.stack([t[:, lo:hi].sum(1) for lo, hi in heads(rows.shape[1])], axis=1)


def main():
    for name in ("h5py", "hdf5plugin", "tables"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    import torch
    from clair3.Train import FocalLoss, _run_epoch
    from shared import param_p
    torch.set_num_threads(1)

    class Recorded(torch.nn.Module):
        """the stand-in module: 'position matrices' are window numbers, the outputs the recorded rows of those windows per task"""

        def __init__(self, rows):
            super().__init__()
            self.rows = torch.from_numpy(rows)

        def forward(self, idx):
            r = self.rows[idx.long()]
            return [r[:, lo:hi] for lo, hi in heads(r.shape[1])]

    for k, case in enumerate(CASES + ("handmade",)):
        rng = np.random.default_rng(9100 + k)
        if case == "handmade":
            rows, labels = handmade_rows(rng)
        else:
            rows = np.load(os.path.join(HERE, f"{case}.npz"))["y_ref"].astype(np.float32)
            B, nout = rows.shape
            labels = np.zeros((B, nout), np.int8)
            for lo, hi in heads(nout):
                cls = np.where(rng.random(B) < 0.5, rows[:, lo:hi].argmax(1), rng.integers(0, hi - lo, size=B))
                labels[np.arange(B), lo + cls] = 1
        B, nout = rows.shape
        tasks = len(heads(nout))
        eln = rng.integers(1, 6000, size=nout).astype(np.float64)
        out = dict(labels=labels, eln=eln)
        for tag, e in (("", None), ("_w", eln)):
            funcs = [FocalLoss(param_p.label_shape_cum, t, e) for t in range(tasks)]
            y_true, y_pred = torch.from_numpy(labels).float(), torch.from_numpy(rows)
            out["loss_ref" + tag] = np.stack([funcs[t](y_true[:, lo:hi], y_pred[:, lo:hi]).numpy() for t, (lo, hi) in enumerate(heads(nout))],
                                             axis=1).astype(np.float32)
            loader = [(np.arange(i, min(i + EPOCH_BATCH, B)), labels[i:i + EPOCH_BATCH]) for i in range(0, B, EPOCH_BATCH)]
            out["epoch_ref" + tag] = np.float64(_run_epoch(Recorded(rows), loader, None, funcs, param_p.label_shape[:tasks], "cpu", train=False))
            if e is not None:
                out["weights"] = np.concatenate([f.cls_weights.numpy().reshape(-1) for f in funcs]).astype(np.float32)
        out["loss_f64"] = f64_losses(rows, labels, None)
        out["loss_f64_w"] = f64_losses(rows, labels, out["weights"])
        if case == "handmade":
            out["rows"] = rows
        path = os.path.join(HERE, f"score_{case}.npz")
        np.savez_compressed(path, **out)
        print(f"{case}: B={B} nout={nout} epoch {out['epoch_ref']:.9g} weighted {out['epoch_ref_w']:.9g} "
              f"loss_ref max {np.nanmax(out['loss_ref']):.6g} -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
