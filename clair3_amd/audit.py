"""How far the kernel forms are from the exact row, on a sample of the job's own windows.

``python -m clair3_amd.audit --chkpnt_fn M --tensor_fn X.npy [--pileup] [--plans "lstm2;proj2,lstm2"] [--tol 1e-4] [--near_tie 1e-6]
[--max_windows N] [--out FILE]`` builds ONE handle with the exact form enabled (model.exact: the network in fp64 from end to end on the
device, the arithmetic of the fp64 oracle) and the product forms kept whatever the weights look like (the semantics of C3HIP_FP32=0), runs
the sample through the exact form, through no plan (fp16x3 everywhere), through ``all`` (the fp32 forms) and through every named per-layer
precision plan (plans separated by ``;``, the layers of a plan by ``,``), and prints one JSON line per form.  Everything is measured
against the EXACT rows: ``windows``, ``max_abs_err`` overall and per head (``head_max_abs_err``, columns 0-21-24-57-90), the
``worst_window``, ``rows_over_tol``, the arg-max differences per head outside near-ties (``label_diffs``; a near-tie is an exact top-2 gap
<= near_tie), the excused ones (``near_ties``), and ``seconds`` / ``windows_per_s`` of the form's pass.  ``precision`` is what the handle
reports behind the pass (a form that met the range guard continues on fp32 and says so here), ``fp32_layers`` the plan in force.
With ``--label_fn L.npy`` (labels (N, 24|90) in the row's column layout, one-hot or soft) every line also carries what the form costs in
the unit the checkpoint was trained in: ``loss`` (the reference's validation loss, clair3/Train.py:87-107 and :236-240: the sum over the
tasks of the mean focal loss), ``task_loss`` and ``accuracy`` per task and ``nonfinite`` -- the forms' float32 rows scored on the device
(score mode, c3_score_rows), the exact form's double rows by the same rule in numpy (synthetic.focal_scores).
With ``--on-ring`` the same table is measured where a job runs: every form's rows travel through the submit / wait ring with verify mode
on every batch and the exact form as its reference (model.verify(reference="exact")), and the line is what the DEVICE compared --
``max_abs_err`` the double maximum (verify_extra), the per-head maxima its float32 roundings, ``worst_batch`` / ``worst_row`` instead of
``worst_window``, ``batches_checked`` / ``batches_skipped``; ``seconds`` then include the exact pass.  The rows are the same rows, so
``max_abs_err``, ``rows_over_tol``, ``label_diffs`` and ``near_ties`` are those of the table without it.
"""
import json
import sys
import time

import numpy as np

from . import _lib

HEAD_SLICES = ((0, 21), (21, 24), (24, 57), (57, 90))


def compare(y_exact, y_form, tol=1e-4, near_tie=1e-6):
    """Rows of a form against the exact rows, plain numpy: a dict of ``windows``, ``max_abs_err``, ``head_max_abs_err``, ``worst_window``,
    ``rows_over_tol``, ``label_diffs`` and ``near_ties`` (per head: arg-max differences where the exact top-2 gap exceeds near_tie / where it
    does not).  A value of the form that is not finite counts as an infinite error: its row is over tol."""
    ye, yf = np.asarray(y_exact, dtype=np.float64), np.asarray(y_form, dtype=np.float64)
    if ye.ndim != 2 or ye.shape != yf.shape or ye.shape[1] not in (24, 90):
        raise ValueError(f"rows must be two (B, 24|90) arrays, got {ye.shape} and {yf.shape}")
    with np.errstate(invalid="ignore"):
        d = np.abs(yf - ye)
    d[~np.isfinite(d)] = np.inf
    per_row = d.max(axis=1) if len(d) else np.zeros(0)
    out = dict(windows=int(len(ye)), tol=float(tol), near_tie=float(near_tie), max_abs_err=float(per_row.max()) if len(d) else 0.0,
               worst_window=int(per_row.argmax()) if len(d) else -1, rows_over_tol=int((per_row > tol).sum()),
               head_max_abs_err=[], label_diffs=[], near_ties=[])
    for lo, hi in HEAD_SLICES:
        if lo >= ye.shape[1]:
            break
        e, f = ye[:, lo:hi], yf[:, lo:hi]
        out["head_max_abs_err"].append(float(d[:, lo:hi].max()) if len(d) else 0.0)
        top2 = np.sort(e, axis=1)[:, -2:]
        tie = (top2[:, 1] - top2[:, 0]) <= near_tie
        differs = np.where(np.isfinite(f), f, -np.inf).argmax(axis=1) != e.argmax(axis=1)
        out["label_diffs"].append(int((differs & ~tie).sum()))
        out["near_ties"].append(int((differs & tie).sum()))
    return out


def parse_plans(text, kind):
    """"lstm2;proj2,lstm2" -> ["lstm2", "proj2,lstm2"], every plan checked against the network's layer names by the library
    (c3_layer_precision_check: plain host code, no device).  "" and "all" are always run and are not repeated."""
    plans = []
    for plan in (text or "").split(";"):
        plan = ",".join(p.strip() for p in plan.strip().split(",")) if plan.strip() else ""
        if not plan or plan == "all" or plan in plans:
            continue
        _lib.check(_lib.lib().c3_layer_precision_check(kind, plan.encode()), f"--plans {plan!r}")
        plans.append(plan)
    return plans


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m clair3_amd.audit", description=__doc__.split("\n\n")[0])
    ap.add_argument("--chkpnt_fn", required=True, help="the checkpoint (.pt)")
    ap.add_argument("--tensor_fn", required=True, help="windows of the job: .npy, full alignment int8 (N, depth, 33, channels), pileup int8 | int32 (N, 33, 18)")
    ap.add_argument("--pileup", action="store_true", help="the pileup network (default: full alignment)")
    ap.add_argument("--plans", default="", help="per-layer precision plans to audit besides none and all: plans separated by ';', layers by ','")
    ap.add_argument("--tol", type=float, default=1e-4, help="a row is over tol when one probability is further from the exact one (default 1e-4)")
    ap.add_argument("--near_tie", type=float, default=1e-6, help="an arg-max difference is excused when the exact top-2 gap is at most this (default 1e-6)")
    ap.add_argument("--label_fn", default=None, help="labels of the windows (.npy, (N, 24|90)): every line also carries loss and accuracy")
    ap.add_argument("--gamma", type=float, default=2.0, help="the focal loss's gamma (default 2, the reference's)")
    ap.add_argument("--max_windows", type=int, default=None, help="use the first n windows (default: all)")
    ap.add_argument("--platform", default="ont")
    ap.add_argument("--enable_dwell_time", action="store_true")
    ap.add_argument("--out", default=None, help="write the lines here as well")
    ap.add_argument("--on-ring", dest="on_ring", action="store_true",
                    help="measure through the submit / wait ring with verify mode against the exact form (the device's comparison)")
    args = ap.parse_args(argv)
    if not args.tol > 0 or not np.isfinite(args.tol):
        raise _lib.C3Error(f"--tol must be > 0, got {args.tol}")
    if not args.near_tie >= 0 or not np.isfinite(args.near_tie):
        raise _lib.C3Error(f"--near_tie must be >= 0, got {args.near_tie}")
    if args.max_windows is not None and args.max_windows < 1:
        raise _lib.C3Error(f"--max_windows must be >= 1, got {args.max_windows}")
    args.plan_list = parse_plans(args.plans, _lib.KIND_PILEUP if args.pileup else _lib.KIND_FULL_ALIGNMENT)
    return args


def score_fields(model, y, labels, gamma=2.0):
    """loss, task_loss, accuracy and nonfinite of a form's rows: float32 rows on the device, double rows by the numpy rule"""
    from . import synthetic as syn
    if np.asarray(y).dtype == np.float64:
        r = syn.focal_scores(y, labels, gamma=gamma)
        task = r["loss_sum"] / max(1, r["windows"])
        return dict(loss=float(sum(float(v) for v in task)), task_loss=[float(v) for v in task],
                    accuracy=[float(v) for v in r["correct"] / max(1, r["windows"])], nonfinite=int(r["nonfinite"]))
    r = model.score_rows(y, labels, gamma=gamma, window_loss=False)
    return dict(loss=float(r.loss), task_loss=[float(v) for v in r.task_loss], accuracy=[float(v) for v in r.accuracy], nonfinite=int(r.nonfinite))


def audit(model, x, plans=(), tol=1e-4, near_tie=1e-6, rows_out=None, labels=None, gamma=2.0):
    """The lines of the tool for a model with the exact form enabled: a list of dicts, the exact form first.  ``rows_out``: a dict that
    receives every form's rows under the form's name.  The handle's precision plan is put back to what it was."""
    import re
    before = ",".join(model.layer_precision())
    lines = []
    t0 = time.perf_counter()
    y_exact = model.predict_exact(x)
    dt = time.perf_counter() - t0
    forms = [("exact", None), ("none", ""), ("all", "all")] + [(p, p) for p in plans]
    try:
        for name, plan in forms:
            if plan is None:
                y = y_exact
            else:
                model.layer_precision(plan)
                model.predict_numpy(x)  # (the first call of a form pays its workspace and its kernels' load)
                t0 = time.perf_counter()
                y = model.predict_numpy(x)
                dt = time.perf_counter() - t0
            line = dict(form=name)
            line.update(compare(y_exact, y, tol, near_tie))
            prec = re.search(r"precision=(\S+)", model.describe())
            layers = re.search(r"fp32_layers=(\S+)", model.describe())
            line.update(seconds=dt, windows_per_s=len(x) / dt if dt > 0 else 0.0, precision="fp64" if plan is None else prec.group(1) if prec else "?",
                        fp32_layers="" if plan is None or not layers else layers.group(1))
            if labels is not None:
                line.update(score_fields(model, y, labels, gamma))
            lines.append(line)
            if rows_out is not None:
                rows_out[name] = y
    finally:
        model.layer_precision(before)
    return lines


def audit_on_ring(model, x, plans=(), tol=1e-4, near_tie=1e-6, rows_out=None):
    """The lines of ``--on-ring`` for a model with the exact form enabled: one dict per form (none, all, the plans), taken from the totals of
    verify mode with the exact form as its reference after one predict_numpy of the sample.  Verify mode, its reference and the precision
    plan are put back to what they were."""
    import re
    before, verify, ref, with_layers = ",".join(model.layer_precision()), model._verify, model._verify_ref, model._verify_layers
    heads = 4 if model.output_size == 90 else 2
    lines = []
    try:
        for name, plan in [("none", ""), ("all", "all")] + [(p, p) for p in plans]:
            model.layer_precision(plan)
            model.verify(every=1, tol=tol, near_tie=near_tie, reference="exact")
            model.predict_numpy(x)  # (the first call of a form pays its workspace and its kernels' load)
            model.verify_reset()
            t0 = time.perf_counter()
            y = model.predict_numpy(x)
            dt = time.perf_counter() - t0
            st, ex = model.verify_stats(), model.verify_extra()
            prec = re.search(r"precision=(\S+)", model.describe())
            layers = re.search(r"fp32_layers=(\S+)", model.describe())
            lines.append(dict(form=name, on_ring=True, windows=int(st["windows_checked"]), tol=float(st["tol"]), near_tie=float(st["near_tie"]),
                              max_abs_err=ex["max_abs_diff_f64"], worst_batch=int(st["worst_batch"]), worst_row=int(st["worst_row"]),
                              rows_over_tol=int(st["rows_over_tol"]), head_max_abs_err=[float(v) for v in st["head_max_abs_diff"][:heads]],
                              label_diffs=[int(v) for v in st["label_diffs"][:heads]], near_ties=[int(v) for v in st["near_ties"][:heads]],
                              batches_checked=int(st["batches_checked"]), batches_skipped=int(st["batches_skipped"]), seconds=dt,
                              windows_per_s=len(x) / dt if dt > 0 else 0.0, precision=prec.group(1) if prec else "?",
                              fp32_layers=layers.group(1) if layers else ""))
            if rows_out is not None:
                rows_out[name] = y
    finally:
        model.layer_precision(before)
        every, vtol, vtie, policy = verify if verify is not None else (0, 1e-4, 1e-6, _lib.VERIFY_REPORT)
        model.verify(every=every, tol=vtol, near_tie=vtie, escalate=policy == _lib.VERIFY_ESCALATE, replace=policy == _lib.VERIFY_REPLACE,
                     layers=with_layers, reference=ref)
    return lines


def main(argv=None, rows_out=None):
    args = parse_args(argv)  # (a bad plan name is refused here, before any device call)
    import os
    from . import predict
    x = np.load(args.tensor_fn, mmap_mode="r")
    if args.max_windows is not None:
        x = x[:args.max_windows]
    ok = (x.ndim == 3 and x.dtype in (np.int8, np.int32)) if args.pileup else (x.ndim == 4 and x.dtype == np.int8)
    if not ok or len(x) == 0:
        raise _lib.C3Error(f"{args.tensor_fn}: {'int8 | int32 windows (N, 33, 18)' if args.pileup else 'int8 windows (N, depth, 33, channels)'} expected, "
                           f"got {x.dtype} {x.shape}")
    x = np.ascontiguousarray(x)
    sd = predict._read_checkpoint(args.chkpnt_fn)
    saved = {k: os.environ.get(k) for k in ("C3HIP_FP32", "C3HIP_EXACT")}
    os.environ["C3HIP_FP32"] = "0"  # the product forms stay whatever the weights look like: the audit is ABOUT them
    os.environ.pop("C3HIP_EXACT", None)
    try:
        m = predict.build_model(args.pileup, "Y_indel_length_logits_1.weight" in sd, platform=args.platform, enable_dwell_time=args.enable_dwell_time)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    m.load_state_dict(sd)
    m.exact(True)
    labels = None
    if args.label_fn:
        labels = np.load(args.label_fn)
        if args.max_windows is not None:
            labels = labels[:args.max_windows]
        if labels.ndim != 2 or labels.shape[0] != len(x) or labels.shape[1] < m.output_size:
            raise _lib.C3Error(f"{args.label_fn}: labels {labels.shape} do not belong to {len(x)} windows of a model with {m.output_size} outputs")
        labels = np.ascontiguousarray(labels[:, :m.output_size], dtype=np.int8 if labels.dtype.kind in "biu" else np.float32)
    if args.on_ring:
        lines = audit_on_ring(m, x, args.plan_list, args.tol, args.near_tie, rows_out)
    else:
        lines = audit(m, x, args.plan_list, args.tol, args.near_tie, rows_out, labels, args.gamma)
    text = "".join(json.dumps(line) + "\n" for line in lines)
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
