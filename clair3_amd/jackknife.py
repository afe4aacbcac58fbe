"""Does a full-alignment call survive when one read of its window is taken away, and which read does it lean on?

``python -m clair3_amd.jackknife --chkpnt_fn M --tensor_fn X.npy [--layout recentre|in_place] [--gap 1e-4] [--top N] [--max_windows N]
[--out FILE]`` builds one full-alignment handle with decoder columns on, runs the windows of ``X.npy`` (int8 (N, depth, 33, channels))
through jackknife mode (model.jackknife: for every window the device builds one variant per read of its run -- the window without that
row --, runs them through the forward pass beside the window itself and reduces their rows to one record) and prints JSON lines:

* one line per window in which some variant flips a label, at most ``--top`` of them, windows with the most flips first:
  ``window``, ``reads``, ``flips`` (per head: variants whose arg-max differs from the window's), ``decision_flips`` (per reference base
  A C G T: variants whose first decoder decision differs), ``lean_read`` / ``lean_drop`` (per head: the read whose removal takes most
  from the called class's probability, and how much), ``max_delta`` and ``min_gap``, the window's own distance from a tie;
* a last line of totals: ``windows``, ``variants``, ``windows_head_flip`` / ``windows_decision_flip`` (windows with any), ``nonfinite``, and
  ``near_tie_table``, the 2 x 2 table of "within ``--gap`` of a tie in the window's own row" (refine mode's selection,
  synthetic.refine_select) against "some variant flips": ``[[far & stable, far & flips], [near & stable, near & flips]]``.
"""
import json
import sys

import numpy as np

from . import _lib, synthetic as syn


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m clair3_amd.jackknife", description=__doc__.split("\n\n")[0])
    ap.add_argument("--chkpnt_fn", required=True, help="the checkpoint (.pt)")
    ap.add_argument("--tensor_fn", required=True, help="full-alignment windows of the job: .npy, int8 (N, depth, 33, channels)")
    ap.add_argument("--layout", default="recentre", help="where a variant's rows go: recentre (the reference's padding rule, default) or in_place")
    ap.add_argument("--gap", type=float, default=1e-4, help="a window is near a tie when a gap of its own row is at most this (default 1e-4)")
    ap.add_argument("--top", type=int, default=20, help="print at most this many windows with a flip (default 20)")
    ap.add_argument("--max_windows", type=int, default=None, help="use the first n windows (default: all)")
    ap.add_argument("--platform", default="ont")
    ap.add_argument("--enable_dwell_time", action="store_true")
    ap.add_argument("--out", default=None, help="write the lines here as well")
    args = ap.parse_args(argv)
    if args.layout not in _lib.JACKKNIFE_LAYOUT:
        raise _lib.C3Error(f"--layout must be recentre or in_place, got {args.layout!r}")
    if not args.gap >= 0 or not np.isfinite(np.float32(args.gap)):
        raise _lib.C3Error(f"--gap must be a finite number >= 0, got {args.gap}")
    if args.top < 0:
        raise _lib.C3Error(f"--top must be >= 0, got {args.top}")
    if args.max_windows is not None and args.max_windows < 1:
        raise _lib.C3Error(f"--max_windows must be >= 1, got {args.max_windows}")
    return args


def report(result, nout, gap=1e-4, top=20):
    """The lines of the tool from what model.jackknife / jackknife_rows returned (plain numpy): the windows with a flip, then the totals."""
    rec, base = result["rows"], result["base_rows"]
    heads = len(syn.head_slices(nout))
    near = np.zeros(len(rec), dtype=bool)
    selected, min_gap = syn.refine_select(base, nout, gap)
    near[selected] = True
    head_flip = (rec["flips"] > 0).any(axis=1)
    decision_flip = (rec["decision_flips"] > 0).any(axis=1)
    flips = head_flip | decision_flip
    weight = rec["flips"].sum(axis=1, dtype=np.int64) + rec["decision_flips"].sum(axis=1, dtype=np.int64)
    order = [int(b) for b in np.argsort(-weight, kind="stable") if flips[b]][:top]
    lines = [dict(window=b, reads=int(rec["reads"][b]), flips=[int(v) for v in rec["flips"][b, :heads]],
                  decision_flips=[int(v) for v in rec["decision_flips"][b]], lean_read=[int(v) for v in rec["lean_read"][b, :heads]],
                  lean_drop=[float(v) for v in rec["lean_drop"][b, :heads]], max_delta=float(rec["max_delta"][b]), min_gap=float(min_gap[b]))
             for b in order]
    table = [[int((~near & ~flips).sum()), int((~near & flips).sum())], [int((near & ~flips).sum()), int((near & flips).sum())]]
    lines.append(dict(windows=int(len(rec)), variants=int(rec["reads"].sum(dtype=np.int64)), windows_head_flip=int(head_flip.sum()),
                      windows_decision_flip=int(decision_flip.sum()), nonfinite=int(rec["nonfinite"].sum(dtype=np.int64)), gap=float(gap),
                      near_tie_table=table, on_fp32=bool(result.get("on_fp32", False))))
    return lines


def main(argv=None):
    args = parse_args(argv)  # (argument errors are raised here, before any device call)
    from . import predict
    x = np.load(args.tensor_fn, mmap_mode="r")
    if args.max_windows is not None:
        x = x[:args.max_windows]
    if x.ndim != 4 or x.dtype != np.int8 or len(x) == 0:
        raise _lib.C3Error(f"{args.tensor_fn}: int8 windows (N, depth, 33, channels) expected, got {x.dtype} {x.shape}")
    x = np.ascontiguousarray(x)
    sd = predict._read_checkpoint(args.chkpnt_fn)
    m = predict.build_model(False, "Y_indel_length_logits_1.weight" in sd, platform=args.platform, enable_dwell_time=args.enable_dwell_time)
    m.load_state_dict(sd)
    m.decode_columns(True)
    lines = report(m.jackknife(x, layout=args.layout), m.output_size, args.gap, args.top)
    text = "".join(json.dumps(line) + "\n" for line in lines)
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
