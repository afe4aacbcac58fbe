"""Calibration of the full-alignment network's channel exponents from observed activations: the file a job hands to its worker processes,
and the command that writes it.

    python -m clair3_amd.calibrate --chkpnt_fn M --tensor_fn X.npy [--windows n] [--cap_log2 10] [--platform ont] [--enable_dwell_time] --out F

``X.npy`` holds full-alignment windows of the job, int8 (N, depth, 33, channels) -- what the model call receives.  The first ``n`` of them
(all by default) run on the fp32 forms, the census of their activations goes through the rule of include/c3hip.h (c3_calibration_rule), and
``F`` receives the result.  ``C3HIP_CALIBRATION=F`` then makes every full-alignment model built by clair3_amd.predict load with it.
INTEGRATION.md 8 says when to calibrate and on what sample.

The file is JSON: ``format`` (FORMAT), ``channels`` and ``depth`` of the windows, ``cap_log2`` and ``windows`` of the calibration, ``k0`` --
the 896 channel exponents the load-time rule gives the checkpoint: the fingerprint a file is checked against before it is applied -- and
``lowering``, by how many powers of two each of them comes down.  Both lists run stage0 | inner0 | stage1 | inner1 | stage2 | inner2.
"""
import json
import sys

import numpy as np

from . import _lib

FORMAT = "clair3_amd-calibration-1"
CHANNELS = 896
# (name, first entry, channels, the convolutions whose outputs the group's exponents scale)
GROUPS = (("stage0", 0, 64, (0, 2)), ("inner0", 64, 64, (1,)), ("stage1", 128, 128, (3, 5)), ("inner1", 256, 128, (4,)),
          ("stage2", 384, 256, (6, 8)), ("inner2", 640, 256, (7,)))


def rule(scaled_max, cap_log2=10):
    """the lowering of ONE group from the largest scaled activation of each of its channels (c3_calibration_rule; plain host code)"""
    s = np.ascontiguousarray(scaled_max, dtype=np.float32)
    if s.ndim != 1:
        raise _lib.C3Error(f"scaled_max must be one-dimensional, got shape {s.shape}")
    out = np.zeros(s.shape[0], dtype=np.uint8)
    _lib.check(_lib.lib().c3_calibration_rule(s.ctypes.data, s.shape[0], int(cap_log2), out.ctypes.data), "c3_calibration_rule")
    return out


def as_lowering(values, what="lowering"):
    """896 integers in [0, 255] as the uint8 array the C ABI takes; anything else raises"""
    try:
        a = np.asarray(values)
    except (TypeError, ValueError) as e:
        raise _lib.C3Error(f"{what} must hold {CHANNELS} integers") from e
    if a.shape != (CHANNELS,) or a.dtype.kind not in "iu" or (a < 0).any() or (a > 255).any():
        raise _lib.C3Error(f"{what} must hold {CHANNELS} integers in [0, 255], got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a, dtype=np.uint8)


def group_maxima(census):
    """(896,) the largest |activation| of every channel of the six groups in the checkpoint's units: for a stage the larger of its two layers"""
    census = np.asarray(census)
    return np.concatenate([np.max([census[l, :n] for l in layers], axis=0) for _, _, n, layers in GROUPS]).astype(np.float64)


def summary(census, k0, lowering):
    """what a calibration did, per group: channels, how many were lowered, the group shift (the smallest lowering: what a silent channel
    got) and the largest scaled activation -- what the fp16 planes hold -- before and after"""
    a, k0, lowering = group_maxima(census), np.asarray(k0, dtype=np.int64), np.asarray(lowering, dtype=np.int64)
    groups = []
    for name, at, n, _ in GROUPS:
        g = slice(at, at + n)
        groups.append(dict(name=name, channels=n, lowered=int(np.count_nonzero(lowering[g])), shift=int(lowering[g].min()),
                           max_before=float(np.ldexp(a[g], k0[g]).max()), max_after=float(np.ldexp(a[g], k0[g] - lowering[g]).max())))
    return dict(groups=groups, lowered=int(np.count_nonzero(lowering)))


def summary_text(s):
    lines = [f"calibration: cap 2^{s['cap_log2']}, {s['windows']} windows, {s['lowered']} of {CHANNELS} channel exponents lowered"
             + ("" if s.get("applied", True) else " (not applied)")]
    for g in s["groups"]:
        lines.append(f"  {g['name']}: {g['lowered']:3d} of {g['channels']:3d} lowered, group shift {g['shift']:2d}, "
                     f"largest scaled activation {g['max_before']:.4g} -> {g['max_after']:.4g}")
    return "\n".join(lines)


def write_file(path, *, channels, depth, cap_log2, windows, k0, lowering):
    doc = dict(format=FORMAT, channels=int(channels), depth=int(depth), cap_log2=int(cap_log2), windows=int(windows),
               k0=[int(v) for v in np.asarray(k0).reshape(-1)], lowering=[int(v) for v in as_lowering(lowering)])
    if len(doc["k0"]) != CHANNELS:
        raise _lib.C3Error(f"k0 must hold {CHANNELS} integers, got {len(doc['k0'])}")
    with open(path, "w") as f:
        json.dump(doc, f)
        f.write("\n")


def read_file(path):
    """the fields of a calibration file, checked: ``k0`` int8 (896), ``lowering`` uint8 (896), the rest integers.  A file that is missing,
    is not such a file or holds values out of range raises C3Error naming the file and the field"""
    try:
        with open(path) as f:
            doc = json.load(f)
    except OSError as e:
        raise _lib.C3Error(f"calibration file {path}: {e.strerror or e}") from e
    except ValueError as e:
        raise _lib.C3Error(f"calibration file {path}: not JSON ({e})") from e
    if not isinstance(doc, dict) or doc.get("format") != FORMAT:
        raise _lib.C3Error(f"calibration file {path}: format must be {FORMAT!r}, got {doc.get('format') if isinstance(doc, dict) else type(doc).__name__!r}")
    out = {}
    for key, lo, hi in (("channels", 1, 10), ("depth", 1, 2 ** 31 - 1), ("cap_log2", 0, 13), ("windows", 0, 2 ** 63 - 1)):
        v = doc.get(key)
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise _lib.C3Error(f"calibration file {path}: {key} must be an integer in [{lo}, {hi}], got {v!r}")
        out[key] = v
    for key, lo, hi, dtype in (("k0", -40, 40, np.int8), ("lowering", 0, 255, np.uint8)):
        v = doc.get(key)
        if (not isinstance(v, list) or len(v) != CHANNELS
                or any(isinstance(e, bool) or not isinstance(e, int) or not lo <= e <= hi for e in v)):
            raise _lib.C3Error(f"calibration file {path}: {key} must hold {CHANNELS} integers in [{lo}, {hi}]")
        out[key] = np.array(v, dtype=dtype)
    if (out["k0"].astype(np.int64) - out["lowering"] < -40).any():
        raise _lib.C3Error(f"calibration file {path}: k0 - lowering must stay at or above -40")
    return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m clair3_amd.calibrate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--chkpnt_fn", required=True, help="the full-alignment checkpoint (.pt)")
    ap.add_argument("--tensor_fn", required=True, help="windows of the job: .npy, int8 (N, depth, 33, channels)")
    ap.add_argument("--windows", type=int, default=None, help="use the first n windows (default: all)")
    ap.add_argument("--cap_log2", type=int, default=10, help="scaled activations of the sample stay below 2^cap (4 .. 13; default 10)")
    ap.add_argument("--platform", default="ont")
    ap.add_argument("--enable_dwell_time", action="store_true")
    ap.add_argument("--out", required=True, help="the calibration file to write")
    args = ap.parse_args(argv)
    import os
    from . import predict
    os.environ.pop("C3HIP_CALIBRATION", None)  # (the file written is this sample's, whatever this process was told to apply)
    x = np.load(args.tensor_fn, mmap_mode="r")
    if args.windows is not None:
        if args.windows < 1:
            raise _lib.C3Error(f"--windows must be >= 1, got {args.windows}")
        x = x[:args.windows]
    if x.dtype != np.int8 or x.ndim != 4 or len(x) == 0:
        raise _lib.C3Error(f"{args.tensor_fn}: int8 windows (N, depth, 33, channels) expected, got {x.dtype} {x.shape}")
    sd = predict._read_checkpoint(args.chkpnt_fn)
    m = predict.build_model(False, "Y_indel_length_logits_1.weight" in sd, platform=args.platform, enable_dwell_time=args.enable_dwell_time)
    m.load_state_dict(sd)
    step = 256
    for off in range(0, len(x) - step, step):
        m.calibrate(np.ascontiguousarray(x[off:off + step]), cap_log2=args.cap_log2, apply=False)
    s = m.calibrate(np.ascontiguousarray(x[max(0, (len(x) - 1) // step * step):]), cap_log2=args.cap_log2, apply=True)
    m.save_calibration(args.out)
    print(summary_text(s))
    print(f"written to {args.out}: C3HIP_CALIBRATION={args.out} applies it where a full-alignment model is built")
    return 0


if __name__ == "__main__":
    sys.exit(main())
