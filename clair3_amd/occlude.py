"""Which input channels and which columns does a call lean on?

``python -m clair3_amd.occlude --chkpnt_fn M --tensor_fn X.npy [--pileup] [--band n] [--what channels|bands|both] [--head 0..3]
[--max_windows N] [--out FILE]`` builds one handle with decoder columns on -- the full-alignment network, or with ``--pileup`` the pileup
network --, runs the windows of ``X.npy`` (full alignment: int8 (N, depth, 33, channels); pileup: int8 or int32 (N, 33, channels)) through
occlusion mode (model.occlude: for every window the device builds one variant per channel -- that channel set to zero -- and one per band
of ``--band`` columns -- those columns set to zero --, runs them through the forward pass beside the window itself and reduces their rows)
and prints JSON lines for the head ``--head`` (0: the 21 genotypes, 1: zygosity, 2 / 3: the indel lengths):

* one line per channel (``channel``: its index) and one per band (``band``: its index, ``columns``: [first, behind the last]):
  ``flips`` -- the windows whose arg-max in the head flips when it is set to zero --, ``mean_drop`` and ``max_drop`` -- the mean and the
  largest, over the windows, of what it takes from the called class's probability (NaN drops left out) --, ``lean`` -- in how many windows
  it is the member of its group with the largest drop;
* a last line of totals: ``windows``, ``variants``, ``head``, ``band``, ``channels``, ``bands``, ``windows_head_flip`` /
  ``windows_decision_flip`` (windows with any, per group), ``nonfinite``, ``max_delta``, ``on_fp32``.
"""
import json
import sys

import numpy as np

from . import _lib, synthetic as syn


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m clair3_amd.occlude", description=__doc__.split("\n\n")[0])
    ap.add_argument("--chkpnt_fn", required=True, help="the checkpoint (.pt)")
    ap.add_argument("--tensor_fn", required=True, help="windows of the job: .npy, int8 (N, depth, 33, channels), or with --pileup int8 / int32 (N, 33, channels)")
    ap.add_argument("--pileup", action="store_true", help="the pileup network (default: full alignment)")
    ap.add_argument("--what", default="both", help="what is set to zero: channels, bands or both (default)")
    ap.add_argument("--band", type=int, default=1, help="columns per band (default 1)")
    ap.add_argument("--head", type=int, default=0, help="the head the lines speak of, 0 .. 3 (default 0)")
    ap.add_argument("--max_windows", type=int, default=None, help="use the first n windows (default: all)")
    ap.add_argument("--platform", default="ont")
    ap.add_argument("--enable_dwell_time", action="store_true")
    ap.add_argument("--out", default=None, help="write the lines here as well")
    args = ap.parse_args(argv)
    if args.what not in _lib.OCCLUDE_WHAT:
        raise _lib.C3Error(f"--what must be channels, bands or both, got {args.what!r}")
    if not 1 <= args.band <= syn.NO_OF_POSITIONS:
        raise _lib.C3Error(f"--band must lie in 1 .. {syn.NO_OF_POSITIONS}, got {args.band}")
    if not 0 <= args.head <= 3:
        raise _lib.C3Error(f"--head must lie in 0 .. 3, got {args.head}")
    if args.max_windows is not None and args.max_windows < 1:
        raise _lib.C3Error(f"--max_windows must be >= 1, got {args.max_windows}")
    return args


def report(result, nout, head=0):
    """The lines of the tool from what model.occlude / occlude_rows returned with drops=True (plain numpy): one per channel, one per band,
    then the totals."""
    heads = len(syn.head_slices(nout))
    if not 0 <= head < heads:
        raise _lib.C3Error(f"head {head}: rows of {nout} probabilities hold the heads 0 .. {heads - 1}")
    rec, drops = result["rows"], np.asarray(result["drops"])
    nc, nb, band = int(result["channels"]), int(result["bands"]), int(result["band"])
    base = np.asarray(result["base_rows"], dtype=np.float32)
    lo, hi = syn.head_slices(nout)[head]
    lines = []
    if "variant_rows" in result and len(rec):  # the windows whose arg-max flips, member by member
        v = np.asarray(result["variant_rows"]).reshape(len(rec), nc + nb, -1)
        t = syn._first_argmax(base[:, lo:hi])
        flips = (syn._first_argmax(v[:, :, lo:hi].reshape(len(rec) * (nc + nb), hi - lo)).reshape(len(rec), nc + nb) != t[:, None]).sum(axis=0)
    else:
        flips = None
    for j in range(nc + nb):
        g, k = (0, j) if j < nc else (1, j - nc)
        d = drops[:, j, head].astype(np.float64)
        d = d[~np.isnan(d)]
        line = dict(channel=k) if g == 0 else dict(band=k, columns=[k * band, min(syn.NO_OF_POSITIONS, (k + 1) * band)])
        if flips is not None:
            line["flips"] = int(flips[j])
        line.update(mean_drop=float(d.mean()) if d.size else 0.0, max_drop=float(d.max()) if d.size else 0.0, lean=int((rec["lean"][:, g, head] == k).sum()))
        lines.append(line)
    lines.append(dict(windows=int(len(rec)), variants=int(rec["variants"].sum(dtype=np.int64)), head=int(head), band=band, channels=nc, bands=nb,
                      windows_head_flip=[int((rec["flips"][:, g, head] > 0).sum()) for g in range(2)],
                      windows_decision_flip=[int((rec["decision_flips"][:, g] > 0).any(axis=1).sum()) for g in range(2)],
                      nonfinite=int(rec["nonfinite"].sum(dtype=np.int64)), max_delta=float(rec["max_delta"].max()) if len(rec) else 0.0,
                      on_fp32=bool(result.get("on_fp32", False))))
    return lines


def main(argv=None):
    args = parse_args(argv)  # (argument errors are raised here, before any device call)
    from . import predict
    x = np.load(args.tensor_fn, mmap_mode="r")
    if args.max_windows is not None:
        x = x[:args.max_windows]
    if args.pileup and (x.ndim != 3 or x.dtype not in (np.dtype(np.int8), np.dtype(np.int32)) or len(x) == 0):
        raise _lib.C3Error(f"{args.tensor_fn}: int8 or int32 windows (N, 33, channels) expected, got {x.dtype} {x.shape}")
    if not args.pileup and (x.ndim != 4 or x.dtype != np.int8 or len(x) == 0):
        raise _lib.C3Error(f"{args.tensor_fn}: int8 windows (N, depth, 33, channels) expected, got {x.dtype} {x.shape}")
    x = np.ascontiguousarray(x)
    sd = predict._read_checkpoint(args.chkpnt_fn)
    m = predict.build_model(args.pileup, "Y_indel_length_logits_1.weight" in sd, platform=args.platform, enable_dwell_time=args.enable_dwell_time)
    m.load_state_dict(sd)
    m.decode_columns(True)
    lines = report(m.occlude(x, what=args.what, band=args.band, drops=True, variant_rows=True), m.output_size, args.head)
    text = "".join(json.dumps(line) + "\n" for line in lines)
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
