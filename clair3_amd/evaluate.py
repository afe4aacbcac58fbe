"""The reference's validation pass on the library (score mode).

The one place where the reference runs its networks in ``eval()`` mode outside variant calling is the validation half of its training
loop: ``_run_epoch(..., train=False)`` (clair3/Train.py:210-257) -- a forward pass over labelled windows, ``FocalLoss.forward``
(:87-107) per head, a batch mean per head, a sum over heads, the mean over batches.  Here the same number comes from the library's
kernels (Clair3_P/F.score: c3_score_submit / c3_score_wait), with the probabilities never leaving the device.

    class_weights(effective_label_num, tasks)   the reference's class weights (Train.py:80-84), in the row's column layout
    run_validation_epoch(model, loader, ...)    what _run_epoch(train=False) returns
    install()                                   rebinds clair3.Train._run_epoch: validation passes run on the library
    census_report(census)                       accuracy, per-class precision / recall / F1, calibration error and near-tie counts from the
                                                census of score mode (Clair3_P/F.census(), synthetic.score_census)
    python -m clair3_amd.evaluate --chkpnt_fn M --tensor_fn X.npy --label_fn L.npy [--pileup] [--report [--report_json FILE]]

C3HIP_SCORE_CENSUS=1 makes the rebound _run_epoch(train=False) take the census of its epoch and leave one line per task on stderr.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import synthetic as syn

RING = 3  # batches of an epoch in flight


def class_weights(effective_label_num, tasks=None, beta=0.999):
    """The class weights of the reference's FocalLoss (clair3/Train.py:80-84, :94-98) for every task, concatenated in the row's column
    layout as float32: per task, with n_c the effective label count of class c and K the task's classes,
    w_c = (1 - beta) / (1 - beta^n_c), scaled so that the task's weights add up to K.  ``effective_label_num``: 24 or 90 counts (or 90 with
    tasks=2: the first two tasks are taken)."""
    n = np.asarray(effective_label_num, dtype=np.float64).reshape(-1)
    heads = syn.head_slices(len(n))
    if tasks is not None:
        heads = heads[:int(tasks)]
    if not heads or heads[-1][1] > len(n):
        raise ValueError(f"effective_label_num holds {len(n)} counts: 24 or 90 expected")
    out = []
    for lo, hi in heads:
        w = (1.0 - beta) / (1.0 - np.power(beta, n[lo:hi]))
        out.append(w / np.sum(w) * (hi - lo))
    return np.concatenate(out).astype(np.float32)


def run_validation_epoch(model, loader, class_weights=None, gamma=2.0):
    """What the reference's ``_run_epoch(model, loader, ..., train=False)`` returns: the mean over the loader's batches of
    sum_t (batch mean of task t's focal loss).  ``loader`` yields (position_matrix, label) pairs of numpy arrays, labels (B, >= output_size)
    in the row's column layout (any numeric dtype; the reference converts to float).  A model with submit_score / wait_score (Clair3_P/F)
    keeps up to RING batches on the ring; anything else with a ``score`` method is called batch by batch."""
    nout = model.output_size
    ring = hasattr(model, "submit_score") and hasattr(model, "wait_score")
    total, batches, pending = 0.0, 0, []

    def labels_of(label):
        label = np.asarray(label)[:, :nout]
        return np.ascontiguousarray(label, dtype=np.int8 if label.dtype.kind in "biu" else np.float32)

    for x, label in loader:
        x, label = np.asarray(x), labels_of(label)
        if not ring:
            total += model.score(x, label, class_weights=class_weights, gamma=gamma).loss
        else:
            if len(pending) == RING:
                total += model.wait_score(pending.pop(0)).loss
            pending.append(model.submit_score(x, label, slot=batches % RING, class_weights=class_weights, gamma=gamma))
        batches += 1
    for t in pending:
        total += model.wait_score(t).loss
    return total / max(1, batches)


def census_report(census):
    """What a reader wants from the census of score mode (a synthetic.Census): a dict with ``windows`` and per task, under ``tasks``,
    ``name``, ``accuracy`` (trace / sum of the confusion table), per class ``support`` (windows whose label is the class), ``precision``
    TP / (TP + FP), ``recall`` TP / (TP + FN) and ``f1`` 2 TP / (2 TP + FP + FN), each nan where its denominator is zero; ``macro_f1`` the
    mean F1 of the classes with support; ``ece`` the expected calibration error sum_b n_b / N |accuracy_b - confidence_b| over the
    reliability bins, with confidence_b = rel_conf_q32 / 2^32 / rel_windows and N the binned windows (nan without any); ``binned``,
    ``skipped`` (windows whose confidence is not a finite number in [0, 1]); ``gap_below`` the six cumulative near-tie counts."""
    def ratio(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(b == 0, np.nan, a / np.where(b == 0, 1, b))

    tasks = []
    for t in range(census.tasks):
        c = np.asarray(census.confusion[t], dtype=np.int64)
        tp, support, predicted = np.diag(c), c.sum(1), c.sum(0)
        f1 = ratio(2 * tp, support + predicted)
        with_support = support > 0
        n_b, ok_b = np.asarray(census.rel_windows[t], np.int64), np.asarray(census.rel_correct[t], np.int64)
        conf_b = ratio(np.asarray(census.rel_conf_q32[t], np.float64) / syn.CENSUS_CONF_UNIT, n_b)
        acc_b, binned = ratio(ok_b, n_b), int(n_b.sum())
        ece = float(np.nansum(n_b * np.abs(acc_b - conf_b)) / binned) if binned else float("nan")
        tasks.append(dict(name=syn.HEAD_NAMES[t], accuracy=float(ratio(tp.sum(), c.sum())), support=support, precision=ratio(tp, predicted),
                          recall=ratio(tp, support), f1=f1, macro_f1=float(f1[with_support].mean()) if with_support.any() else float("nan"),
                          ece=ece, binned=binned, skipped=int(census.rel_skipped[t]),
                          gap_below={f"{float(thr):g}": int(n) for thr, n in zip(syn.CENSUS_GAP_THR, census.gap_below[t])}))
    return dict(windows=int(census.windows), tasks=tasks)


def format_census_report(report):
    """the report as the lines ``--report`` prints"""
    lines = []
    for t in report["tasks"]:
        gaps = " ".join(f"<{k}:{v}" for k, v in t["gap_below"].items())
        lines.append(f"  {t['name']}: accuracy {t['accuracy']:.6f} macro-F1 {t['macro_f1']:.6f} ECE {t['ece']:.6f} binned {t['binned']} "
                     f"skipped {t['skipped']} gaps {gaps}")
        for c in np.flatnonzero((t["support"] > 0) | ~np.isnan(t["precision"])):
            lines.append(f"    class {c}: support {int(t['support'][c])} precision {t['precision'][c]:.6f} recall {t['recall'][c]:.6f} f1 {t['f1'][c]:.6f}")
    return lines


def report_json(report):
    """the report with lists and null in place of arrays and nan"""
    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple, np.ndarray)):
            return [plain(x) for x in v]
        if isinstance(v, (float, np.floating)):
            return None if np.isnan(v) else float(v)
        return int(v) if isinstance(v, np.integer) else v
    return plain(report)


def census_from_env():
    """C3HIP_SCORE_CENSUS=1: a validation pass of the rebound _run_epoch takes the census of its epoch; unset, empty or 0: it does not.
    Anything else raises."""
    value = (os.environ.get("C3HIP_SCORE_CENSUS") or "").strip()
    if value not in ("", "0", "1"):
        raise ValueError(f"C3HIP_SCORE_CENSUS must be 0 or 1, got {value!r}")
    return value == "1"


def validation_lines(report):
    """one line per task for stderr: accuracy, macro-F1, ECE and the windows whose best two probabilities lie closer than 1e-4"""
    return [f"[clair3_amd] validation: task={t['name']} windows={report['windows']} accuracy={t['accuracy']:.6f} macro_f1={t['macro_f1']:.6f} "
            f"ece={t['ece']:.6f} below_1e-4={t['gap_below']['0.0001']}" for t in report["tasks"]]


def run_validation_epoch_with_census(model, loader, class_weights=None, gamma=2.0, out=None):
    """run_validation_epoch with the census of score mode around it: the census is switched on and reset before the epoch, and one line per
    task goes to ``out`` (stderr) behind it.  Returns what run_validation_epoch returns."""
    model.score_census(True)
    model.census_reset()
    value = run_validation_epoch(model, loader, class_weights=class_weights, gamma=gamma)
    for line in validation_lines(census_report(model.census())):
        print(line, file=sys.stderr if out is None else out)
    return value


def handle_for(module, device=None):
    """A library handle holding the weights of a reference torch module (Clair3_P / Clair3_F by its class name; a DistributedDataParallel
    wrapper's ``module.`` prefix is stripped)"""
    from .model import Clair3_F, Clair3_P
    inner = getattr(module, "module", module)
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in module.state_dict().items()}
    cls = Clair3_P if type(inner).__name__ == "Clair3_P" else Clair3_F if type(inner).__name__ == "Clair3_F" else None
    if cls is None:
        raise TypeError(f"no library form of {type(inner).__name__}: Clair3_P and Clair3_F only")
    first = sd["LSTM1.weight_ih_l0" if cls is Clair3_P else "conv1.conv.weight"]
    channels = int(first.shape[1])
    m = cls(add_indel_length=bool(getattr(inner, "add_indel_length", False)), predict=True, input_channels=channels)
    m.to(0 if device is None else device)
    m.load_state_dict(sd)
    return m


def loss_setting(loss_funcs):
    """(gamma, class weights or None) of the reference's list of FocalLoss objects, one per task"""
    gammas = {float(f.gamma) for f in loss_funcs}
    if len(gammas) != 1:
        raise ValueError(f"the tasks' focal losses differ in gamma ({sorted(gammas)}): one gamma per handle")
    ws = [getattr(f, "cls_weights", None) for f in loss_funcs]
    if all(w is None for w in ws):
        return gammas.pop(), None
    if any(w is None for w in ws):
        raise ValueError("some tasks carry class weights and some do not")
    return gammas.pop(), np.concatenate([np.asarray(w.detach().cpu().numpy() if hasattr(w, "detach") else w, dtype=np.float32).reshape(-1) for w in ws])


_ORIGINAL = None


def install(handle_factory=handle_for):
    """Rebind ``clair3.Train._run_epoch``: a pass with train=False and distributed=False reads the torch module's state_dict() into a library
    handle (``handle_factory(module)``) and runs on it; every other call goes to the reference's function.  Returns the reference's function;
    uninstall() puts it back."""
    global _ORIGINAL
    import clair3.Train as train_mod
    if _ORIGINAL is None:
        _ORIGINAL = train_mod._run_epoch
    original = _ORIGINAL

    def _run_epoch(model, loader, optimizer, loss_funcs, label_shapes, device, train=True, desc=None, distributed=False):
        if train or distributed:
            return original(model, loader, optimizer, loss_funcs, label_shapes, device, train=train, desc=desc, distributed=distributed)
        gamma, weights = loss_setting(loss_funcs)
        epoch = run_validation_epoch_with_census if census_from_env() else run_validation_epoch
        return epoch(handle_factory(model), loader, class_weights=weights, gamma=gamma)

    train_mod._run_epoch = _run_epoch
    return original


def uninstall():
    global _ORIGINAL
    if _ORIGINAL is not None:
        import clair3.Train as train_mod
        train_mod._run_epoch, _ORIGINAL = _ORIGINAL, None


def main(argv=None):
    ap = argparse.ArgumentParser(description="focal loss per task and accuracy of labelled windows on the device")
    ap.add_argument("--chkpnt_fn", required=True, help="checkpoint (.pt / state dict) of the network")
    ap.add_argument("--tensor_fn", required=True, help=".npy of the windows (int8; pileup also int32)")
    ap.add_argument("--label_fn", required=True, help=".npy of the labels (B, 24|90), one-hot or soft, in the row's column layout")
    ap.add_argument("--pileup", action="store_true")
    ap.add_argument("--platform", default="ont")
    ap.add_argument("--enable_dwell_time", action="store_true")
    ap.add_argument("--gamma", type=float, default=2.0)
    ap.add_argument("--effective_label_num", default=None, help=".npy of per-class label counts: class weights as the reference derives them")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--report", action="store_true", help="behind the loss: accuracy, per-class precision / recall / F1, calibration error and "
                    "near-tie counts from the census of score mode")
    ap.add_argument("--report_json", default=None, help="with --report: write the report to this file as JSON instead of printing it")
    a = ap.parse_args(argv)
    from . import predict
    x, labels = np.load(a.tensor_fn, mmap_mode="r"), np.load(a.label_fn)
    sd = predict._read_checkpoint(a.chkpnt_fn)
    model = predict.build_model(a.pileup, "Y_indel_length_logits_1.weight" in sd, platform=a.platform, enable_dwell_time=a.enable_dwell_time,
                                device=a.device)
    model.load_state_dict(sd)
    if labels.ndim != 2 or labels.shape[0] != x.shape[0] or labels.shape[1] < model.output_size:
        raise SystemExit(f"{a.label_fn}: labels {labels.shape} do not belong to {x.shape[0]} windows of a model with {model.output_size} outputs")
    labels = np.ascontiguousarray(labels[:, :model.output_size], dtype=np.int8 if labels.dtype.kind in "biu" else np.float32)
    w = None if a.effective_label_num is None else class_weights(np.load(a.effective_label_num)[:model.output_size])
    if a.report_json and not a.report:
        raise SystemExit("--report_json needs --report")
    if a.report:
        model.score_mode(a.gamma, w).score_census(True).census_reset()
    r = model.score(np.ascontiguousarray(x), labels, class_weights=w, gamma=a.gamma)
    print(f"windows {r.windows} nonfinite {r.nonfinite} loss {r.loss:.9g}")
    for t, name in enumerate(syn.HEAD_NAMES[:len(r.task_loss)]):
        print(f"  {name}: loss {r.task_loss[t]:.9g} accuracy {r.accuracy[t]:.6f}")
    if a.report:
        report = census_report(model.census())
        if a.report_json:
            with open(a.report_json, "w") as fh:
                json.dump(report_json(report), fh, indent=1)
        else:
            print("\n".join(format_census_report(report)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
