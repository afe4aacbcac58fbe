"""At what coverage does a full-alignment call hold?

``python -m clair3_amd.subsample --chkpnt_fn M --tensor_fn X.npy [--depths 10,20,30,40] [--replicates 8] [--seed 0]
[--layout recentre|in_place] [--top N] [--max_windows N] [--out FILE]`` builds one full-alignment handle with decoder columns on, runs the
windows of ``X.npy`` (int8 (N, depth, 33, channels)) through subsample mode (model.subsample: for every target depth below a window's own
the device draws ``--replicates`` random subsets of that many of its reads, runs them through the forward pass beside the window itself and
reduces their rows) and prints JSON lines:

* one line per window in which some variant flips a label, at most ``--top`` of them, the windows that hold latest first: ``window``,
  ``reads``, ``hold_level`` (per head: the lowest level from which on no replicate flips the head's arg-max; ``len(depths)`` when the
  deepest level itself flips), ``hold_decision`` (the same for the decoder's first decisions), ``hold_depth`` (the target depth at the
  latest of them, ``null`` when the call does not hold at the deepest level), and per level that ran ``depth``, ``keep``, ``flips``,
  ``decision_flips``, ``min_kept``;
* a last line of totals: ``windows``, ``variants``, per level ``windows_run`` / ``windows_head_flip`` / ``windows_decision_flip``, and
  ``hold_level_genotype``, how many windows hold the genotype head from level 0, 1, .. , ``len(depths)`` on.

Subsampling a window is a proxy for a shallower BAM, not a replacement: candidate selection and phasing upstream of the window saw every read.
"""
import json
import sys

import numpy as np

from . import _lib, synthetic as syn


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m clair3_amd.subsample", description=__doc__.split("\n\n")[0])
    ap.add_argument("--chkpnt_fn", required=True, help="the checkpoint (.pt)")
    ap.add_argument("--tensor_fn", required=True, help="full-alignment windows of the job: .npy, int8 (N, depth, 33, channels)")
    ap.add_argument("--depths", default="10,20,30,40", help="target depths, strictly increasing, at most 8 (default 10,20,30,40)")
    ap.add_argument("--replicates", type=int, default=8, help="random subsets per window and depth, 1 .. 32 (default 8)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the counter hash (default 0)")
    ap.add_argument("--layout", default="recentre", help="where a variant's rows go: recentre (the reference's padding rule, default) or in_place")
    ap.add_argument("--top", type=int, default=20, help="print at most this many windows with a flip (default 20)")
    ap.add_argument("--max_windows", type=int, default=None, help="use the first n windows (default: all)")
    ap.add_argument("--platform", default="ont")
    ap.add_argument("--enable_dwell_time", action="store_true")
    ap.add_argument("--out", default=None, help="write the lines here as well")
    args = ap.parse_args(argv)
    if args.layout not in _lib.JACKKNIFE_LAYOUT:
        raise _lib.C3Error(f"--layout must be recentre or in_place, got {args.layout!r}")
    try:
        depths = [int(v) for v in args.depths.split(",")]
    except ValueError:
        raise _lib.C3Error(f"--depths must be integers separated by commas, got {args.depths!r}") from None
    if not 1 <= len(depths) <= syn.SUBSAMPLE_MAX_LEVELS or depths[0] < 1 or any(b <= a for a, b in zip(depths, depths[1:])):
        raise _lib.C3Error(f"--depths must be 1 .. {syn.SUBSAMPLE_MAX_LEVELS} strictly increasing depths >= 1, got {args.depths!r}")
    args.depths = tuple(depths)
    if not 1 <= args.replicates <= syn.SUBSAMPLE_MAX_REPLICATES:
        raise _lib.C3Error(f"--replicates must lie in 1 .. {syn.SUBSAMPLE_MAX_REPLICATES}, got {args.replicates}")
    if not 0 <= args.seed < 1 << 64:
        raise _lib.C3Error(f"--seed must lie in [0, 2^64), got {args.seed}")
    if args.top < 0:
        raise _lib.C3Error(f"--top must be >= 0, got {args.top}")
    if args.max_windows is not None and args.max_windows < 1:
        raise _lib.C3Error(f"--max_windows must be >= 1, got {args.max_windows}")
    return args


def report(result, nout, depths, top=20):
    """The lines of the tool from what model.subsample / subsample_rows / subsample_reduce returned (plain numpy): the windows with a flip,
    those that hold latest first, then the totals."""
    lev, rec = result["levels"], result["rows"]
    depths = [int(d) for d in depths]
    heads = len(syn.head_slices(nout))
    latest = np.maximum(rec["hold_level"].max(axis=1), rec["hold_decision"]) if len(rec) else np.zeros(0, np.int32)
    order = [int(b) for b in np.argsort(-latest.astype(np.int64), kind="stable") if latest[b] > 0][:top]
    lines = []
    for b in order:
        ran = [l for l in range(len(depths)) if lev["run"][b, l]]
        lines.append(dict(window=b, reads=int(rec["reads"][b]), hold_level=[int(v) for v in rec["hold_level"][b, :heads]],
                          hold_decision=int(rec["hold_decision"][b]), hold_depth=depths[latest[b]] if latest[b] < len(depths) else None,
                          levels=[dict(depth=depths[l], keep=int(lev["keep"][b, l]), flips=[int(v) for v in lev["flips"][b, l, :heads]],
                                       decision_flips=int(lev["decision_flips"][b, l]), nonfinite=int(lev["nonfinite"][b, l]),
                                       min_kept=[float(v) for v in lev["min_kept"][b, l, :heads]]) for l in ran]))
    run = lev["run"] > 0
    genotype = rec["hold_level"][:, 1] if heads > 1 else np.zeros(len(rec), np.int32)
    lines.append(dict(windows=int(len(rec)), variants=int(lev["run"].sum(dtype=np.int64)), depths=depths,
                      windows_run=[int(v) for v in run.sum(axis=0)], windows_head_flip=[int(v) for v in (lev["flips"] > 0).any(axis=2).sum(axis=0)],
                      windows_decision_flip=[int(v) for v in (lev["decision_flips"] > 0).sum(axis=0)],
                      nonfinite=int(lev["nonfinite"].sum(dtype=np.int64)),
                      hold_level_genotype=[int((genotype == l).sum()) for l in range(len(depths) + 1)], on_fp32=bool(result.get("on_fp32", False))))
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
    result = m.subsample(x, depths=args.depths, replicates=args.replicates, seed=args.seed, layout=args.layout)
    lines = report(result, m.output_size, args.depths, args.top)
    text = "".join(json.dumps(line) + "\n" for line in lines)
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
