"""Seeded synthetic weights and candidate-window tensors for the two Clair3 networks.

There is no network access for real checkpoints or BAMs, so tests, goldens and ``bench.py`` all use the
recipes below.  Everything is generated from ``numpy.random.default_rng`` (PCG64,
stable across numpy versions) so that the GPU box can rebuild byte-identical weights/inputs from a seed
instead of shipping megabytes of fixtures.

state_dict key names / shapes follow the reference modules:
  Clair3_P -- /root/reference/clair3/model.py:96-125
  Clair3_F -- /root/reference/clair3/model.py:317-365 (+ BasicConv2D :183-197, BasicBlock :200-235)
"""
import collections
from collections import OrderedDict

import numpy as np

PILEUP = "pileup"
FULL_ALIGNMENT = "full_alignment"

NO_OF_POSITIONS = 33      # shared/param_p.py:35, shared/param_f.py:30
PILEUP_CHANNELS = 18      # shared/param_p.py:32-33
FA_DEPTH_ONT = 89         # shared/param_f.py:11 matrix_depth_dict['ont']
FA_CHANNELS = 8           # shared/param_f.py:24-27 (9 with --enable_dwell_time, CallVariantsFromCffi.py:241-243)
HEAD_SIZES = (21, 3, 33, 33)  # shared/param_p.py:37 label_shape
HEAD_NAMES = ("Y_gt21_logits", "Y_genotype_logits", "Y_indel_length_logits_1", "Y_indel_length_logits_2")

# conv layers of Clair3_F in execution order: (state_dict prefix of conv, prefix of bn, Cin (None = input), Cout, stride)
FA_CONV_LAYERS = (
    ("conv1.conv", "conv1.bn", None, 64, 2),
    ("res_block1.0.conv1", "res_block1.0.bn1", 64, 64, 1),
    ("res_block1.0.conv2", "res_block1.0.bn2", 64, 64, 1),
    ("conv3.conv", "conv3.bn", 64, 128, 2),
    ("res_block2.0.conv1", "res_block2.0.bn1", 128, 128, 1),
    ("res_block2.0.conv2", "res_block2.0.bn2", 128, 128, 1),
    ("conv5.conv", "conv5.bn", 128, 256, 2),
    ("res_block3.0.conv1", "res_block3.0.bn1", 256, 256, 1),
    ("res_block3.0.conv2", "res_block3.0.bn2", 256, 256, 1),
)


def n_outputs(add_indel_length):
    return 90 if add_indel_length else 24


def state_dict_spec(kind, in_channels=None, add_indel_length=False):
    """Ordered (name, shape) list of the float parameters/buffers of the reference module."""
    spec = []
    nb = 4 if add_indel_length else 2
    if kind == PILEUP:
        c = PILEUP_CHANNELS if in_channels is None else in_channels
        for layer, inp, hid in (("LSTM1", c, 128), ("LSTM2", 256, 160)):
            for sfx in ("", "_reverse"):
                spec += [(f"{layer}.weight_ih_l0{sfx}", (4 * hid, inp)), (f"{layer}.weight_hh_l0{sfx}", (4 * hid, hid)),
                         (f"{layer}.bias_ih_l0{sfx}", (4 * hid,)), (f"{layer}.bias_hh_l0{sfx}", (4 * hid,))]
        fc_in, fc = NO_OF_POSITIONS * 320, 128
    elif kind == FULL_ALIGNMENT:
        c = FA_CHANNELS if in_channels is None else in_channels
        for conv, bn, cin, cout, _ in FA_CONV_LAYERS:
            cin = c if cin is None else cin
            spec += [(f"{conv}.weight", (cout, cin, 3, 3)), (f"{conv}.bias", (cout,)),
                     (f"{bn}.weight", (cout,)), (f"{bn}.bias", (cout,)),
                     (f"{bn}.running_mean", (cout,)), (f"{bn}.running_var", (cout,))]
        fc_in, fc = 14 * 256, 256
    else:
        raise ValueError(f"unknown model kind {kind!r}")
    spec += [("L4.weight", (fc, fc_in)), ("L4.bias", (fc,))]
    for i in range(nb):
        spec += [(f"L5_{i + 1}.weight", (128, fc)), (f"L5_{i + 1}.bias", (128,))]
    for i in range(nb):
        spec += [(f"{HEAD_NAMES[i]}.weight", (HEAD_SIZES[i], 128)), (f"{HEAD_NAMES[i]}.bias", (HEAD_SIZES[i],))]
    return spec


def make_state_dict(kind, in_channels=None, add_indel_length=False, seed=0, peaked=False, trained_like=False):
    """Seeded random float32 state_dict (numpy arrays) that loads strictly into the reference module.

    BatchNorm statistics are randomised (default init is an identity and would hide BN-folding bugs);
    ``peaked=True`` scales the head weights x8 so the soft-max outputs approach 0/1 like a trained model;
    ``trained_like=True`` re-parametrises the same network the way training leaves one (``_trained_like``): per-channel
    scales spread over orders of magnitude, zero ``bias_hh``, a few large LSTM weights.
    """
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    spec = state_dict_spec(kind, in_channels, add_indel_length)
    shapes = dict(spec)
    for name, shape in spec:
        leaf = name.rsplit(".", 1)[1]
        if name.startswith("LSTM"):
            hid = shape[0] // 4
            k = 1.0 / np.sqrt(hid)
            v = rng.uniform(-k, k, size=shape)
            if name.startswith("LSTM1.weight_ih"):
                v *= 0.05  # raw counts reach +-100: keep the gate pre-activations O(1) so errors are visible
        elif leaf == "running_mean":
            v = rng.normal(0.0, 0.5, size=shape)
        elif leaf == "running_var":
            v = rng.uniform(0.5, 2.0, size=shape)
        elif ".bn" in name and leaf == "weight":
            v = rng.uniform(0.5, 1.5, size=shape)
        elif ".bn" in name and leaf == "bias":
            v = rng.normal(0.0, 0.2, size=shape)
        elif len(shape) == 4:  # conv weight, He init
            v = rng.normal(0.0, np.sqrt(2.0 / (shape[1] * 9)), size=shape)
        elif "conv" in name and leaf == "bias":
            v = rng.normal(0.0, 0.1, size=shape)
        else:  # nn.Linear default init
            fan_in = shapes[name.rsplit(".", 1)[0] + ".weight"][1]
            k = 1.0 / np.sqrt(fan_in)
            v = rng.uniform(-k, k, size=shape)
            if kind == PILEUP and leaf == "weight":
                v *= 4.0  # LSTM outputs are bounded: widen the FC gains so windows give visibly different rows
            if peaked and name.startswith("Y_"):
                v *= 8.0 if kind == FULL_ALIGNMENT else 2.0
        sd[name] = np.ascontiguousarray(v, dtype=np.float32)
        if leaf == "running_var":
            sd[name[: -len("running_var")] + "num_batches_tracked"] = np.array(0, dtype=np.int64)
    if trained_like:
        _trained_like(sd, kind, np.random.default_rng(seed + 7919))
    return sd


def _trained_like(sd, kind, rng):
    """What a TRAINED checkpoint looks like that seeded initialisation does not: per-channel magnitudes spread over orders of
    magnitude.  Every change below is a re-parametrisation under which the network computes the same function (up to
    rounding), so activations stay in their ordinary range while the weights do not:

    full alignment
      * pre-BatchNorm scale t_c = 10^U(-1.5, 1.5) of every convolution output channel: conv weight / bias, running_mean times
        t_c, running_var times t_c^2 -- gamma / sqrt(running_var) then spreads over 1e-3 .. 1e3 between channels;
      * post-BatchNorm scale s_c = 10^U(-2.5, 0.3) of every channel (ReLU is positively homogeneous): gamma and beta of its
        producers times s_c, the weights of its consumers that read it divided by s_c.  Channels of a stage are produced by the
        stage convolution AND the residual block's second BatchNorm (the identity add) and consumed by the block's first
        convolution and the next stage (the last stage: by L4 through the pyramid pooling, 14 bins x 256 channels); channels
        inside a block by bn1 / conv2.  The BatchNorm-folded weights of a channel then scale with s_c: 2.8 decades between
        the channels of one tensor, and 2.8 decades between the input channels inside every consumer row.
    pileup (the TF -> torch converter leaves LSTM biases that way, convert_tf_checkpoint_to_torch.py:95-106)
      * bias_hh = 0 (TF has one bias per gate; it lands in bias_ih);
      * one weight in a thousand of W_ih / W_hh replaced by +-8.
    """
    if kind == PILEUP:
        for name in list(sd):
            if name.startswith("LSTM") and ".bias_hh" in name:
                sd[name][...] = 0.0
            elif name.startswith("LSTM") and ".weight_" in name:
                w = sd[name]
                hit = rng.random(w.shape) < 1e-3
                w[hit] = np.where(rng.random(int(hit.sum())) < 0.5, -8.0, 8.0).astype(np.float32)
                if name.startswith("LSTM1.weight_ih"):
                    w[hit] *= 0.05  # the counts reach +-100 (see make_state_dict)
        return
    for conv, bn, _, cout, _ in FA_CONV_LAYERS:
        t = (10.0 ** rng.uniform(-1.5, 1.5, size=cout)).astype(np.float32)
        sd[f"{conv}.weight"] *= t[:, None, None, None]
        sd[f"{conv}.bias"] *= t
        sd[f"{bn}.running_mean"] *= t
        sd[f"{bn}.running_var"] *= t * t
    stages = (("conv1", "res_block1.0", "conv3.conv"), ("conv3", "res_block2.0", "conv5.conv"), ("conv5", "res_block3.0", None))
    for stage, block, nxt in stages:
        cout = sd[f"{stage}.bn.weight"].shape[0]
        s_stage = (10.0 ** rng.uniform(-2.5, 0.3, size=cout)).astype(np.float32)
        s_inner = (10.0 ** rng.uniform(-2.5, 0.3, size=cout)).astype(np.float32)
        for bn in (f"{stage}.bn", f"{block}.bn2"):  # producers of the stage's channels
            sd[f"{bn}.weight"] *= s_stage
            sd[f"{bn}.bias"] *= s_stage
        sd[f"{block}.conv1.weight"] /= s_stage[None, :, None, None]
        if nxt is not None:
            sd[f"{nxt}.weight"] /= s_stage[None, :, None, None]
        else:  # PyramidPolling flattens (bin, channel): L4 column bin * 256 + c reads channel c
            sd["L4.weight"] /= np.tile(s_stage, sd["L4.weight"].shape[1] // cout)[None, :]
        sd[f"{block}.bn1.weight"] *= s_inner
        sd[f"{block}.bn1.bias"] *= s_inner
        sd[f"{block}.conv2.weight"] /= s_inner[None, :, None, None]


def make_pileup_windows(batch, seed=0, recipe="realistic", dtype=np.int8, channels=PILEUP_CHANNELS, depth=None, return_depth=False):
    """(batch, 33, 18) pileup count tensors.

    realistic: per-position strand-split base counts with the reference-base channel negated
    (src/clair3_pileup.c:370-371) and sparse indel channels; uniform: iid integers in [-60, 60].
    depth: mean read depth of the realistic recipe (default: Poisson(50) clipped to [4, 127], what int8 holds); given, the
    depths are Poisson(depth) without the upper clip -- counts of high-coverage regions, for int32 windows.
    return_depth: also return the per-window depth the recipe drew, (windows, int32 depths) -- what the leading integer of a
    candidate's alt_info says; the windows of a seed are the same either way.
    """
    rng = np.random.default_rng(seed)
    if recipe == "uniform":
        x = rng.integers(-60, 61, size=(batch, NO_OF_POSITIONS, channels))
        if return_depth:
            raise ValueError("the uniform recipe draws no read depth")
        return x.astype(dtype)
    x = np.zeros((batch, NO_OF_POSITIONS, channels), dtype=np.int64)
    if depth is None:
        depth = np.clip(rng.poisson(50, size=(batch, 1)), 4, 127)
    else:
        depth = np.maximum(rng.poisson(depth, size=(batch, 1)), 4)
    fwd = rng.binomial(depth, 0.5, size=(batch, NO_OF_POSITIONS))
    rev = depth - fwd
    ref = rng.integers(0, 4, size=(batch, NO_OF_POSITIONS))
    for strand, tot in ((0, fwd), (9, rev)):
        probs = np.full((batch, NO_OF_POSITIONS, 4), 0.05 / 3)
        np.put_along_axis(probs, ref[..., None], 0.95, axis=2)
        # multinomial split of the strand depth over A,C,G,T by successive binomials
        left = tot.copy()
        base = np.zeros((batch, NO_OF_POSITIONS, 4), dtype=np.int64)
        rem_p = np.ones((batch, NO_OF_POSITIONS))
        for b in range(4):
            p = np.clip(probs[..., b] / np.maximum(rem_p, 1e-12), 0.0, 1.0)
            base[..., b] = rng.binomial(left, p) if b < 3 else left
            left = left - base[..., b]
            rem_p = rem_p - probs[..., b]
        tot_bases = base.sum(axis=2)
        np.put_along_axis(base, ref[..., None], -tot_bases[..., None], axis=2)
        x[..., strand:strand + 4] = base
        indel = rng.random((batch, NO_OF_POSITIONS, 5)) < 0.03
        amt = (rng.random((batch, NO_OF_POSITIONS, 5)) * 0.3 * tot[..., None]).astype(np.int64)
        x[..., strand + 4:strand + 9] = np.where(indel, amt, 0)
    if channels != PILEUP_CHANNELS:
        x = np.resize(x, (batch, NO_OF_POSITIONS, channels))
    if return_depth:
        return x.astype(dtype), depth.ravel().astype(np.int32)
    return x.astype(dtype)  # int8 wraps like the reference's GPU .npy path (CreateTensorPileupFromCffi.py:447)


MAX_DEPTH = 144  # shared/param_p.py:15 max_depth_dict, every platform


def rescale_deep_windows(x, depths, max_depth=MAX_DEPTH):
    """What both in-process loops of the reference do to int32 pileup windows before their model call
    (clair3/CallVariantsFromCffi.py:278-285, clair3/utils.py:104-111), in numpy, for tests and callers without a GPU.  Window b with
    depths[b] > 0 and depths[b] > 1.5 * max_depth becomes trunc(x / s) with s = depths[b] / max_depth: one rounding for s (a double,
    as Python's int / int), a second one for every quotient (double), then towards zero into int32.  Deliberately not the exact
    rational x * max_depth / depths[b] (x = 217, depth = 248: 125 here, 126 there).  Every other window is returned as it came.
    Returns a new int32 array; ``x`` is not modified."""
    x = np.asarray(x)
    if x.dtype != np.int32:
        raise TypeError(f"the rescaling rule is defined on int32 counts, got {x.dtype}")
    depths = np.asarray(depths)
    if depths.shape != (x.shape[0],):
        raise ValueError(f"one depth per window: {depths.shape} for {x.shape[0]} windows")
    if max_depth <= 0:
        raise ValueError("max_depth must be positive")
    out = x.copy()
    d = depths.astype(np.int64)
    deep = (d > 0) & (d.astype(np.float64) > 1.5 * float(max_depth))
    if deep.any():
        s = d[deep].astype(np.float64) / np.float64(max_depth)
        q = x[deep].astype(np.float64) / s.reshape((-1,) + (1,) * (x.ndim - 1))
        out[deep] = np.trunc(q).astype(np.int32)
    return out


# status of a candidate in select_pileup_windows (C3_CAND_* in include/c3hip.h)
CAND_NO_WINDOW, CAND_MAIN, CAND_EMPTY_COLUMN, CAND_HEAD, CAND_TAIL = 0, 1, 2, 3, 4
CAND_KEPT = (CAND_MAIN, CAND_HEAD, CAND_TAIL)


def pileup_chunks(major):
    """(first column, one-past-last column) of the chunks of a region: the maximal runs of ``major`` with steps of exactly 1
    (preprocess/CreateTensorPileupFromCffi.py:180-236 cuts wherever major jumps by more than 1; major is strictly increasing)."""
    major = np.asarray(major, dtype=np.int64)
    if major.ndim != 1:
        raise ValueError("major must be one-dimensional")
    if len(major) > 1 and (np.diff(major) <= 0).any():
        raise ValueError("major must be strictly increasing")
    if len(major) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    cuts = np.flatnonzero(np.diff(major) != 1) + 1
    return np.r_[0, cuts].astype(np.int64), np.r_[cuts, len(major)].astype(np.int64)


def select_pileup_starts(region, major, positions, head_tail=False):
    """The selection rule of select_pileup_windows without the windows: (status uint8 [n_cand], chunk index int64 [n_cand], offset int64
    [n_cand]) -- the window of candidate i is columns offset[i] .. offset[i] + 32 of its chunk, where columns outside the chunk (head / tail
    windows only) are zero rows; for a main window chunk start + offset is its first column in ``region``."""
    region = np.asarray(region)
    major = np.asarray(major, dtype=np.int64)
    pos = np.asarray(positions, dtype=np.int64)
    if region.ndim != 2 or len(major) != len(region) or pos.ndim != 1:
        raise ValueError("region (n_cols, C), major (n_cols,), positions (n_cand,) expected")
    T, F = NO_OF_POSITIONS, (NO_OF_POSITIONS - 1) // 2
    a, b = pileup_chunks(major)
    status = np.zeros(len(pos), np.uint8)
    chunk = np.zeros(len(pos), np.int64)
    off = np.zeros(len(pos), np.int64)
    if len(a) == 0 or len(pos) == 0:
        return status, chunk, off
    first, last = major[a], major[b - 1]
    k = np.searchsorted(first, pos, side="right") - 1
    inside = (k >= 0) & (pos <= last[np.maximum(k, 0)])
    k = np.maximum(k, 0)
    lo = pos - F - 1  # first position of the window (the reference's offset = start - first - 1 with start = pos - F)
    main = inside & (lo >= first[k]) & (pos + F + 1 <= last[k])
    empty = np.r_[0, np.cumsum((region == 0).all(axis=1))]
    col = np.where(main, a[k] + lo - first[k], 0)
    has_empty = main & (empty[np.minimum(col + T, len(region))] - empty[col] > 0)
    status[main] = CAND_MAIN
    status[has_empty] = CAND_EMPTY_COLUMN
    if head_tail:
        rest = inside & ~main
        head = rest & (lo < first[k])
        status[head & (lo + T - 1 <= last[k])] = CAND_HEAD
        status[rest & ~head] = CAND_TAIL
    kept = np.isin(status, CAND_KEPT)
    chunk[kept], off[kept] = k[kept], (lo - first[k])[kept]
    return status, chunk, off


def select_pileup_windows(region, major, positions, head_tail=False):
    """Which windows the reference's pileup producer feeds the model (preprocess/CreateTensorPileupFromCffi.py:343-397), in numpy: for
    callers without a GPU and for the tests.  region: (n_cols, C) counts; major: plp_data.major (strictly increasing; `minor` is not read:
    the Clair3 pileup emits no insertion columns); positions: the candidates' positions, in the caller's order.

    Chunks are the maximal runs of major with steps of 1 (first .. last).  A candidate's window covers positions pos-17 .. pos+15.  Main
    (pos-17 >= first and pos+17 <= last): 33 in-chunk columns, CAND_MAIN, or CAND_EMPTY_COLUMN (dropped) when one of them is all zero.  With
    head_tail, where the main test failed and first <= pos <= last: pos-17 < first gives CAND_HEAD iff pos+15 <= last (zero rows before
    first), else CAND_TAIL (zero rows after last); neither is tested for empty columns.  Everything else: CAND_NO_WINDOW.

    Returns (status uint8 [n_cand], windows int32 [n_kept, 33, C]) -- the windows of the kept candidates in candidate order."""
    region = np.asarray(region)
    status, chunk, off = select_pileup_starts(region, major, positions, head_tail)
    a, b = pileup_chunks(major)
    kept = np.flatnonzero(np.isin(status, CAND_KEPT))
    T = NO_OF_POSITIONS
    windows = np.zeros((len(kept), T, region.shape[1]), dtype=np.int32)
    for j, i in enumerate(kept):
        c0, c1 = a[chunk[i]], b[chunk[i]]
        lo, hi = c0 + off[i], c0 + off[i] + T  # columns of the region; the part outside [c0, c1) stays zero
        s, e = max(lo, c0), min(hi, c1)
        windows[j, s - lo:e - lo] = region[s:e]
    return status, windows


def make_pileup_region(n_cols, n_chunks=1, seed=0, empty_fraction=0.0, empty_runs=(), depth=None, first=100000):
    """A region as calculate_clair3_pileup returns it, for select_pileup_windows / Clair3_P.predict_candidates: (region int32 (n_cols, 18),
    major int64 (n_cols,)).  Counts of the realistic window recipe laid end to end; ``n_chunks`` runs of consecutive positions separated by
    1 .. 49 missing ones, cut at seeded columns; ``empty_fraction`` of the columns, and the ``empty_runs`` (first column, columns), all zero."""
    rng = np.random.default_rng(seed)
    region = make_pileup_windows(n_cols // NO_OF_POSITIONS + 1, seed=seed + 1, dtype=np.int32, depth=depth).reshape(-1, PILEUP_CHANNELS)[:n_cols].copy()
    step = np.ones(n_cols, dtype=np.int64)
    if n_chunks > 1:
        cuts = rng.choice(np.arange(1, n_cols), size=n_chunks - 1, replace=False)
        step[cuts] += rng.integers(1, 50, size=n_chunks - 1)
    step[0] = first
    if empty_fraction > 0:
        region[rng.random(n_cols) < empty_fraction] = 0
    for c0, n in empty_runs:
        region[c0:c0 + n] = 0
    return region, np.cumsum(step)


def make_fa_windows(batch, seed=0, recipe="realistic", channels=FA_CHANNELS, depth=FA_DEPTH_ONT, positions=NO_OF_POSITIONS):
    """(batch, 89, 33, 8|9) int8 full-alignment tensors; ``depth`` x ``positions`` windows of the same recipe
    for other geometries (the default call draws what it always drew)."""
    rng = np.random.default_rng(seed)
    shape = (batch, depth, positions, channels)
    if recipe == "uniform":
        return rng.integers(-100, 101, size=shape).astype(np.int8)
    x = np.zeros(shape, dtype=np.int16)
    base_codes = np.array([100, 25, 75, 50])
    alt_codes = np.array([100, 25, 75, 50, -50, -100])
    n_reads = rng.integers(10, depth + 1, size=batch)
    for b in range(batch):
        n = int(n_reads[b])
        top = (depth - n) // 2  # reads centred, zero rows above/below (clair3_full_alignment_dwell.c:139-150)
        rows = slice(top, top + n)
        ref = base_codes[rng.integers(0, 4, size=positions)]
        cover = np.ones((n, positions), dtype=bool)
        partial = rng.random(n) < 0.1
        starts = np.where(partial, rng.integers(0, positions // 2, size=n), 0)
        ends = np.where(partial, rng.integers(positions // 2, positions, size=n), positions)
        pos = np.arange(positions)[None, :]
        cover &= (pos >= starts[:, None]) & (pos < ends[:, None])
        hap = np.sort(rng.choice(np.array([30, 60, 90]), size=n))
        x[b, rows, :, 0] = np.where(cover, ref[None, :], 0)
        alt = np.where(rng.random((n, positions)) < 0.1, alt_codes[rng.integers(0, 6, size=(n, positions))], 0)
        x[b, rows, :, 1] = np.where(cover, alt, 0)
        x[b, rows, :, 2] = np.where(cover, rng.choice(np.array([50, 100]), size=(n, 1)), 0)
        x[b, rows, :, 3] = np.where(cover, rng.integers(0, 101, size=(n, 1)), 0)
        x[b, rows, :, 4] = np.where(cover, rng.integers(0, 101, size=(n, positions)), 0)
        x[b, rows, :, 5] = np.where(cover, rng.integers(0, 101, size=(n, 1)), 0)
        ins = np.where(rng.random((n, positions)) < 0.03, base_codes[rng.integers(0, 4, size=(n, positions))], 0)
        x[b, rows, :, 6] = np.where(cover, ins, 0)
        x[b, rows, :, 7] = np.where(cover, hap[:, None], 0)
        if channels > 8:  # dwell channel, zero where no base (clair3_full_alignment_dwell.c:905-911)
            dwell = np.clip(rng.geometric(0.12, size=(n, positions)), 0, 127)
            x[b, rows, :, 8] = np.where(cover, dwell, 0)
    return x.astype(np.int8)


def pad_fa_rows(rows, counts, firsts=None, depth=FA_DEPTH_ONT):
    """Dense full-alignment windows (B, depth, positions, C) int8 from their occupied rows, in numpy, for tests and callers without a GPU:
    ``rows`` (n_rows, positions, C) holds the rows of all windows back to back, window b owns counts[b] of them and is zero except rows
    [first, first + counts[b]).  firsts=None: first = (depth - counts[b]) // 2, what the reference's generator pads by
    (clair3/utils.py:113-121: prefix = int(padding_depth / 2), the rest behind) and its C producer lays out
    (src/clair3_full_alignment_dwell.c:139-150); else first = firsts[b]."""
    rows = np.asarray(rows)
    counts = np.asarray(counts, dtype=np.int64)
    if rows.ndim != 3 or counts.ndim != 1:
        raise ValueError("rows (n_rows, positions, C) and counts (B,) expected")
    if (counts < 0).any() or (counts > depth).any() or int(counts.sum()) != len(rows):
        raise ValueError(f"counts must lie in [0, {depth}] and add up to the {len(rows)} rows given")
    first = (depth - counts) // 2 if firsts is None else np.asarray(firsts, dtype=np.int64)
    if first.shape != counts.shape or (first < 0).any() or (first + counts > depth).any():
        raise ValueError(f"every run must lie inside the {depth} rows of a window")
    x = np.zeros((len(counts), depth) + rows.shape[1:], dtype=rows.dtype)
    src = np.r_[0, np.cumsum(counts)]
    for b in range(len(counts)):
        x[b, first[b]:first[b] + counts[b]] = rows[src[b]:src[b + 1]]
    return x


def pack_fa_rows(x):
    """The inverse, as c3_pack_rows states it: (rows, firsts int32, counts int32) of dense windows (B, depth, positions, C) -- for every
    window the run from its first to its last non-zero row (interior zero rows stay inside the run; an all-zero window: count 0, first 0)."""
    x = np.asarray(x)
    if x.ndim != 4:
        raise ValueError("windows (B, depth, positions, C) expected")
    occupied = (x != 0).any(axis=(2, 3))
    firsts, counts = np.zeros(len(x), np.int32), np.zeros(len(x), np.int32)
    parts = []
    for b in range(len(x)):
        nz = np.flatnonzero(occupied[b])
        if len(nz):
            firsts[b], counts[b] = nz[0], nz[-1] - nz[0] + 1
            parts.append(x[b, nz[0]:nz[-1] + 1])
    rows = np.concatenate(parts) if parts else np.zeros((0,) + x.shape[2:], dtype=x.dtype)
    return rows, firsts, counts


def make_windows(kind, batch, seed=0, recipe="realistic", channels=None):
    if kind == PILEUP:
        return make_pileup_windows(batch, seed, recipe, channels=channels or PILEUP_CHANNELS)
    return make_fa_windows(batch, seed, recipe, channels=channels or FA_CHANNELS)


# ---- score mode in numpy: the rule of csrc/c3_score.h for callers without a GPU ----
def head_slices(nout):
    """the (lo, hi) column ranges of the tasks a row of ``nout`` probabilities holds"""
    out, lo = [], 0
    for n in HEAD_SIZES:
        if lo >= nout:
            break
        out.append((lo, lo + n))
        lo += n
    return out


def focal_scores(rows, labels, gamma=2.0, class_weights=None):
    """The reference's focal loss (clair3/Train.py:87-107) and the arg-max accuracy of labelled rows, in float64 -- the rule the device
    evaluates (c3_score_rows, Clair3_P/F.score).  rows: (B, >= nout) probabilities, float32 (clamped in float32 as the reference clamps them:
    q = min(max(p, 1e-9f), 1.0f)) or float64 (the exact form's: clamped in double at the same two float32 constants); labels: (B, nout) in
    the row's column layout, any numeric dtype, hard or soft; class_weights: nout floats or None.  Per window and task
    L_t = sum_c w_c y_c (-ln q_c) (1 - q_c)^gamma y_c, one chain over the columns in ascending order.  Returns a dict: ``window_loss``
    (B, tasks) float64, ``loss_sum`` (tasks,) their sums in window order, ``correct`` (tasks,) windows whose arg-max of p is the arg-max of y
    (first maximum; a NaN is never one), ``nonfinite`` windows holding a probability that is not finite, ``windows``, ``tasks``."""
    labels = np.asarray(labels)
    nout = labels.shape[1]
    rows = np.asarray(rows)
    if rows.ndim != 2 or labels.ndim != 2 or rows.shape[0] != labels.shape[0] or rows.shape[1] < nout or nout not in (24, 90):
        raise ValueError(f"rows {rows.shape} and labels {labels.shape} do not belong together")
    p = rows[:, :nout]
    lo_c, hi_c = np.float32(1e-9), np.float32(1.0)
    if p.dtype != np.float64:
        p = p.astype(np.float32, copy=False)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(p < lo_c, lo_c, np.where(p > hi_c, hi_c, p)).astype(np.float64)  # (a NaN stays a NaN)
        y = labels.astype(np.float64)
        rest = 1.0 - q
        terms = (-y * np.log(q)) * ((rest * rest if gamma == 2 else np.power(rest, float(gamma))) * y)
        if class_weights is not None:
            w = np.asarray(class_weights, dtype=np.float32).astype(np.float64)
            if w.shape != (nout,):
                raise ValueError(f"class_weights must hold {nout} entries, got shape {w.shape}")
            terms = terms * w[None, :]
    heads = head_slices(nout)
    B = len(p)
    window_loss = np.zeros((B, len(heads)), dtype=np.float64)
    correct = np.zeros(len(heads), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t, (lo, hi) in enumerate(heads):
            acc = np.zeros(B, dtype=np.float64)
            for c in range(lo, hi):  # one chain in column order
                acc = acc + terms[:, c]
            window_loss[:, t] = acc
            pa = np.where(np.isnan(p[:, lo:hi]), -np.inf, p[:, lo:hi]).argmax(1) if B else np.zeros(0, np.int64)
            ya = np.where(np.isnan(y[:, lo:hi]), -np.inf, y[:, lo:hi]).argmax(1) if B else np.zeros(0, np.int64)
            correct[t] = int((pa == ya).sum())
    loss_sum = np.zeros(len(heads), dtype=np.float64)
    for b in range(B):  # in window order
        loss_sum = loss_sum + window_loss[b]
    return dict(window_loss=window_loss, loss_sum=loss_sum, correct=correct, nonfinite=int((~np.isfinite(p)).any(1).sum()) if B else 0,
                windows=B, tasks=len(heads))


# ---- score mode's census in numpy: the rule of csrc/c3_census.h, whose definitions these constants repeat (tests/test_score_census.py
# holds them against that header) ----
CENSUS_BINS = 20                                                                  # kScoreCensusBins
CENSUS_GAP_THR = np.array([1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1], dtype=np.float32)  # score_census_gap_thr
CENSUS_CONF_UNIT = 2.0 ** 32                                                      # kScoreCensusConfUnit
CENSUS_CELL_OFF = (0, 441, 450, 1539)                                             # kScoreCensusCellOff: task t's K_t x K_t cells of c3_score_census.confusion

# what score_census and Clair3_P/F.census() return: ``confusion`` four (K_t, K_t) int64 arrays [truth][pred]; ``rel_windows``, ``rel_correct``,
# ``rel_conf_q32`` (4, 20) int64; ``rel_skipped`` (4,); ``gap_below`` (4, 6), cumulative.  The tables of tasks a model lacks are zero.
Census = collections.namedtuple("Census", "windows tasks confusion rel_windows rel_correct rel_conf_q32 rel_skipped gap_below")


def empty_census(tasks=0):
    return Census(0, tasks, [np.zeros((k, k), np.int64) for k in HEAD_SIZES], np.zeros((4, CENSUS_BINS), np.int64),
                  np.zeros((4, CENSUS_BINS), np.int64), np.zeros((4, CENSUS_BINS), np.int64), np.zeros(4, np.int64),
                  np.zeros((4, len(CENSUS_GAP_THR)), np.int64))


def score_census(rows, labels):
    """The census of score mode (c3_model_set_score_census; csrc/c3_census.h states the rule and its constants) of labelled float32 rows:
    per task the confusion table of arg-max(y) against arg-max(p) -- the arg-maxima of focal_scores' ``correct`` -- the reliability table
    over 20 confidence bins with fixed-point confidence sums, and the cumulative counts of windows whose best two probabilities lie closer
    than 1e-6 .. 1e-1.  rows: (B, >= nout) float32 probabilities as they come out (not clamped); labels: (B, nout).  Returns a Census."""
    labels = np.asarray(labels)
    rows = np.asarray(rows)
    if rows.ndim != 2 or labels.ndim != 2 or rows.shape[0] != labels.shape[0] or rows.shape[1] < labels.shape[1] or labels.shape[1] not in (24, 90):
        raise ValueError(f"rows {rows.shape} and labels {labels.shape} do not belong together")
    nout = labels.shape[1]
    p_all, y_all = rows[:, :nout].astype(np.float32, copy=False), labels.astype(np.float32)
    heads = head_slices(nout)
    B = len(p_all)
    out = empty_census(len(heads))._replace(windows=B)
    if B == 0:
        return out
    at = np.arange(B)
    for t, (lo, hi) in enumerate(heads):
        p = np.where(np.isnan(p_all[:, lo:hi]), np.float32(-np.inf), p_all[:, lo:hi])  # a NaN is never a maximum
        y = np.where(np.isnan(y_all[:, lo:hi]), np.float32(-np.inf), y_all[:, lo:hi])
        pred, truth = p.argmax(1), y.argmax(1)  # the first maximum; index 0 when nothing exceeds -inf
        np.add.at(out.confusion[t], (truth, pred), 1)
        conf = p[at, pred]  # -inf when the head is all NaN
        others = p.copy()
        others[at, pred] = -np.inf
        second = others.max(1)
        with np.errstate(invalid="ignore"):
            gap = conf - second  # float32
            ok = np.isfinite(conf) & (conf >= 0) & (conf <= 1)
            b = np.minimum(CENSUS_BINS - 1, (conf[ok] * np.float32(CENSUS_BINS)).astype(np.int64))
            np.add.at(out.rel_windows[t], b, 1)
            np.add.at(out.rel_correct[t], b, (pred == truth)[ok].astype(np.int64))
            np.add.at(out.rel_conf_q32[t], b, np.rint(conf[ok].astype(np.float64) * CENSUS_CONF_UNIT).astype(np.int64))
            out.rel_skipped[t] = int((~ok).sum())
            for k, thr in enumerate(CENSUS_GAP_THR):
                out.gap_below[t, k] = int((gap < thr).sum())
    return out


# ---- refine mode in numpy: the rule of csrc/c3_refine.h (tests/test_refine.py holds the two together) ----
DECODE_COLS = 31  # kDecodeCols (csrc/c3_decode.h)


def _top2_gap(v):
    """largest minus second-largest value of every row of ``v`` in float32: 0 when the maximum occurs twice, NaN when the row holds a NaN"""
    s = np.sort(v.astype(np.float32, copy=False), axis=1)  # (a NaN sorts behind everything: the difference is then a NaN)
    with np.errstate(invalid="ignore"):
        return (s[:, -1] - s[:, -2]).astype(np.float32)


def refine_gaps(rows, nout, columns=None):
    """The gaps refine mode looks at (c3_model_set_refine; csrc/c3_refine.h states the rule), (B, 5) float32: columns 0 .. 3 the top-2 gap of
    every head of the ``nout`` probabilities (+inf for a head the row does not have), column 4 the decoder gap -- for every reference base
    A, C, G, T that does not take the early exit (bit b of decoder column 22) the top-2 gap among decoder column 9 + b and columns 0 .. 8,
    the minimum over those bases; +inf when all four take it or the rows carry no decoder columns.  columns: None = the rows carry them iff
    they are wider than ``nout``; False = ignore them."""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.ndim != 2 or nout not in (24, 90) or rows.shape[1] not in (nout, nout + DECODE_COLS):
        raise ValueError(f"rows {rows.shape} are not rows of {nout} probabilities with or without the {DECODE_COLS} decoder columns")
    has_cols = rows.shape[1] > nout
    if columns is None:
        columns = has_cols
    if columns and not has_cols:
        raise ValueError("columns=True needs rows with the decoder columns")
    out = np.full((len(rows), 5), np.inf, dtype=np.float32)
    if len(rows) == 0:
        return out
    for h, (lo, hi) in enumerate(head_slices(nout)):
        out[:, h] = _top2_gap(rows[:, lo:hi])
    if columns:
        cols = rows[:, nout:]
        with np.errstate(invalid="ignore"):
            early = np.nan_to_num(cols[:, 22], nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)
        per_base = [np.where(early >> b & 1, np.float32(np.inf), _top2_gap(np.concatenate([cols[:, 9 + b:10 + b], cols[:, 0:9]], axis=1)))
                    for b in range(4)]
        out[:, 4] = np.fmin.reduce(np.stack(per_base), axis=0)  # (a NaN gap of one base is left out, as refine_select leaves a NaN head gap out)
    return out


def refine_select(rows, nout, gap, columns=None):
    """(index, min_gap) of refine mode's selection (c3_refine_select): the windows any of whose gaps is <= ``gap`` in float32, ascending, as
    int32; and every window's minimum gap with NaN gaps left out (NaN when all of them are).  A NaN gap selects nothing."""
    g = refine_gaps(rows, nout, columns)
    with np.errstate(invalid="ignore"):
        sel = (g <= np.float32(gap)).any(axis=1)
    return np.flatnonzero(sel).astype(np.int32), np.fmin.reduce(g, axis=1) if len(g) else np.zeros(0, np.float32)


# ---- jackknife mode in numpy: the definitions of csrc/c3_jackknife.h (tests/test_jackknife.py holds the two together) ----
JACKKNIFE_LAYOUTS = ("recentre", "in_place")  # C3_JACKKNIFE_RECENTRE, C3_JACKKNIFE_IN_PLACE
# c3_jackknife_window (include/c3hip.h), 80 bytes
JACKKNIFE_DTYPE = np.dtype([("reads", "<i4"), ("nonfinite", "<i4"), ("flips", "<i4", (4,)), ("decision_flips", "<i4", (4,)),
                            ("lean_read", "<i4", (4,)), ("lean_drop", "<f4", (4,)), ("max_delta", "<f4"), ("reserved", "<i4")])


def leave_one_out(rows, counts, firsts=None, depth=FA_DEPTH_ONT, layout="recentre"):
    """The leave-one-read-out variants of windows given as their occupied rows (pad_fa_rows's arguments), dense, (sum(counts), depth,
    positions, C) int8 in the order of c3_jackknife_rows: window after window, variant j of a window being the window without row j of its
    run.  layout "recentre": the counts[b] - 1 rows that stay are laid out by the reference's padding rule for THAT count, first =
    (depth - (counts[b] - 1)) // 2; "in_place": they start where the base window's run starts (firsts[b], or its centred first)."""
    if layout not in JACKKNIFE_LAYOUTS:
        raise ValueError(f"layout must be one of {JACKKNIFE_LAYOUTS}, got {layout!r}")
    rows = np.asarray(rows)
    counts = np.asarray(counts, dtype=np.int64)
    pad_fa_rows(rows, counts, firsts, depth)  # (its checks)
    base_first = (depth - counts) // 2 if firsts is None else np.asarray(firsts, dtype=np.int64)
    src = np.r_[0, np.cumsum(counts)]
    v_rows, v_counts, v_firsts = [], [], []
    for b in range(len(counts)):
        run = rows[src[b]:src[b + 1]]
        for j in range(int(counts[b])):
            v_rows.append(np.delete(run, j, axis=0))
            v_counts.append(counts[b] - 1)
            v_firsts.append(base_first[b] if layout == "in_place" else (depth - (counts[b] - 1)) // 2)
    flat = np.concatenate(v_rows) if v_rows else np.zeros((0,) + rows.shape[1:], dtype=rows.dtype)
    return pad_fa_rows(flat, np.asarray(v_counts, dtype=np.int64), np.asarray(v_firsts, dtype=np.int64), depth)


def _first_argmax(v):
    """arg-max of every row of ``v`` by the rule of the census and of refine mode: the first maximum, a NaN never, index 0 when nothing
    exceeds -inf"""
    return np.where(np.isnan(v), np.float32(-np.inf), v).argmax(1) if len(v) else np.zeros(0, np.int64)


def jackknife_records(base_rows, variant_rows, counts, nout, columns=None):
    """(records, drops) of jackknife mode (c3_jackknife_reduce; csrc/c3_jackknife.h states the definitions): ``base_rows`` (B, row) float32,
    ``variant_rows`` (sum(counts), row) the rows of every window's variants in window order, read order; row = nout or nout + DECODE_COLS.
    records: (B,) of JACKKNIFE_DTYPE; drops: (sum(counts), 4) float32, y[t_h] - v_j[t_h].  columns: None = the rows carry decoder columns
    iff they are wider than ``nout``; False = ignore them."""
    base = np.asarray(base_rows, dtype=np.float32)
    var = np.asarray(variant_rows, dtype=np.float32)
    counts = np.asarray(counts, dtype=np.int64)
    if base.ndim != 2 or var.ndim != 2 or nout not in (24, 90) or base.shape[1] not in (nout, nout + DECODE_COLS) or var.shape[1] != base.shape[1]:
        raise ValueError(f"base rows {base.shape} and variant rows {var.shape} are not rows of {nout} probabilities with or without the decoder columns")
    if counts.shape != (len(base),) or (counts < 0).any() or int(counts.sum()) != len(var):
        raise ValueError(f"counts must hold one entry >= 0 per window and add up to the {len(var)} variant rows given")
    has_cols = base.shape[1] > nout
    if columns is None:
        columns = has_cols
    if columns and not has_cols:
        raise ValueError("columns=True needs rows with the decoder columns")
    heads = head_slices(nout)
    rec = np.zeros(len(base), dtype=JACKKNIFE_DTYPE)
    rec["lean_read"] = -1
    drops = np.zeros((len(var), 4), dtype=np.float32)
    at = np.r_[0, np.cumsum(counts)]
    for b in range(len(base)):
        y, v = base[b], var[at[b]:at[b + 1]]
        n = len(v)
        rec["reads"][b] = n
        if n == 0:
            continue
        finite = np.isfinite(v[:, :nout]).all(axis=1)
        rec["nonfinite"][b] = int((~finite).sum())
        with np.errstate(invalid="ignore"):
            delta = np.abs(v[finite, :nout] - y[None, :nout])  # float32
            delta = delta[~np.isnan(delta)]
            rec["max_delta"][b] = delta.max() if delta.size else np.float32(0)
            for h, (lo, hi) in enumerate(heads):
                t = lo + int(_first_argmax(y[None, lo:hi])[0])
                rec["flips"][b, h] = int((lo + _first_argmax(v[:, lo:hi]) != t).sum())
                d = (y[t] - v[:, t]).astype(np.float32)  # one float32 subtraction
                drops[at[b]:at[b + 1], h] = d
                ok = finite & ~np.isnan(d)
                if ok.any():
                    j = int(np.where(ok, d, np.float32(-np.inf)).argmax())  # the first of the largest: -0 and +0 are a tie
                    if not ok[j]:  # (every candidate is -inf and a variant that is none comes first)
                        j = int(np.flatnonzero(ok)[0])
                    rec["lean_read"][b, h] = j
                    rec["lean_drop"][b, h] = d[j] + np.float32(0)  # (a zero drop is reported as +0)
            if columns:
                for k in range(4):
                    rec["decision_flips"][b, k] = int((v[:, nout + 23 + k] != y[nout + 23 + k]).sum())
    return rec, drops


# ---- subsample mode in numpy: the rule of csrc/c3_subsample.h (tests/test_subsample.py holds the two together) ----
# c3_subsample_level (48 bytes) and c3_subsample_window (32 bytes) of include/c3hip.h
SUBSAMPLE_LEVEL_DTYPE = np.dtype([("keep", "<i4"), ("run", "<i4"), ("nonfinite", "<i4"), ("decision_flips", "<i4"), ("flips", "<i4", (4,)),
                                  ("min_kept", "<f4", (4,))])
SUBSAMPLE_WINDOW_DTYPE = np.dtype([("reads", "<i4"), ("levels_run", "<i4"), ("hold_level", "<i4", (4,)), ("hold_decision", "<i4"), ("reserved", "<i4")])
SUBSAMPLE_MAX_LEVELS, SUBSAMPLE_MAX_REPLICATES, SUBSAMPLE_MAX_DEPTH = 8, 32, 128
_M64 = (1 << 64) - 1


def subsample_mix(z):
    """the SplitMix64 finaliser on a uint64 array (arithmetic mod 2^64)"""
    z = np.asarray(z, dtype=np.uint64).copy()
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def subsample_keys(seed, w, r, n, depth, replicates):
    """(n,) uint64: key(w, r, j) = mix(seed + 0x9E3779B97F4A7C15 * (1 + (w * R + r) * depth + j)) for the reads j < n of window ``w`` (its
    index in the call) in replicate ``r``; ``depth`` is the handle's"""
    first = (1 + (int(w) * int(replicates) + int(r)) * int(depth)) & _M64
    counter = np.uint64(first) + np.arange(int(n), dtype=np.uint64)
    return subsample_mix(np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * counter)


def subsample_rank(keys, k):
    """(n,) bool: the ``k`` reads of smallest (key, j) -- rank by key, the lowest j first on equal keys"""
    keys = np.asarray(keys, dtype=np.uint64)
    mask = np.zeros(len(keys), dtype=bool)
    mask[np.argsort(keys, kind="stable")[:max(int(k), 0)]] = True
    return mask


def _subsample_plan(counts, depths, replicates):
    counts = np.asarray(counts, dtype=np.int64)
    depths = [int(d) for d in depths]
    if counts.ndim != 1 or (counts < 0).any():
        raise ValueError("counts (B,) >= 0 expected")
    if not 1 <= len(depths) <= SUBSAMPLE_MAX_LEVELS or depths[0] < 1 or any(b <= a for a, b in zip(depths, depths[1:])):
        raise ValueError(f"1 .. {SUBSAMPLE_MAX_LEVELS} strictly increasing target depths >= 1 expected, got {depths}")
    if not 1 <= int(replicates) <= SUBSAMPLE_MAX_REPLICATES:
        raise ValueError(f"replicates must lie in 1 .. {SUBSAMPLE_MAX_REPLICATES}, got {replicates}")
    return counts, depths, int(replicates)


def subsample_variant_counts(counts, depths, replicates):
    """(B,) int64: the variants of every window -- ``replicates`` per level with D_l < counts[w]"""
    counts, depths, R = _subsample_plan(counts, depths, replicates)
    return R * (np.asarray(depths, dtype=np.int64)[None, :] < counts[:, None]).sum(axis=1)


def subsample_masks(counts, depths, replicates, seed, depth):
    """(variants, 2) uint64: the kept-read bitmask of every variant in the rule's order -- window by window, level by level (only levels with
    D_l < counts[w]: k == n is not run), replicate by replicate --, bit j of the pair = read j kept (j < 64 in word 0)"""
    counts, depths, R = _subsample_plan(counts, depths, replicates)
    if (counts > depth).any() or depth > SUBSAMPLE_MAX_DEPTH:
        raise ValueError(f"counts must lie in [0, {depth}] and the depth in [1, {SUBSAMPLE_MAX_DEPTH}]")
    out = []
    for w, n in enumerate(counts):
        keys = [subsample_keys(seed, w, r, n, depth, R) for r in range(R)]
        for k in depths:
            if k >= n:
                continue
            for r in range(R):
                bits = sum(1 << int(j) for j in np.flatnonzero(subsample_rank(keys[r], k)))
                out.append((bits & _M64, bits >> 64))
    return np.array(out, dtype=np.uint64).reshape(len(out), 2)


def subsample_variants(rows, counts, firsts=None, depths=(10, 20, 30, 40), replicates=8, seed=0, depth=FA_DEPTH_ONT, layout="recentre"):
    """The variants of subsample mode of windows given as their occupied rows (pad_fa_rows's arguments), dense, (variants, depth, positions, C)
    int8 in the rule's order.  A variant keeps the reads its mask names, in read order; layout "recentre": they start at dense row
    (depth - k) // 2; "in_place": where the base window's run starts (firsts[w], or its centred first)."""
    if layout not in JACKKNIFE_LAYOUTS:
        raise ValueError(f"layout must be one of {JACKKNIFE_LAYOUTS}, got {layout!r}")
    rows = np.asarray(rows)
    counts, depths, R = _subsample_plan(counts, depths, replicates)
    pad_fa_rows(rows, counts, firsts, depth)  # (its checks)
    base_first = (depth - counts) // 2 if firsts is None else np.asarray(firsts, dtype=np.int64)
    masks = subsample_masks(counts, depths, R, seed, depth)
    src = np.r_[0, np.cumsum(counts)]
    v_rows, v_counts, v_firsts, at = [], [], [], 0
    for w, n in enumerate(counts):
        run = rows[src[w]:src[w + 1]]
        for k in depths:
            if k >= n:
                continue
            for r in range(R):
                bits = int(masks[at, 0]) | int(masks[at, 1]) << 64
                v_rows.append(run[[j for j in range(n) if bits >> j & 1]])
                v_counts.append(k)
                v_firsts.append(base_first[w] if layout == "in_place" else (depth - k) // 2)
                at += 1
    flat = np.concatenate(v_rows) if v_rows else np.zeros((0,) + rows.shape[1:], dtype=rows.dtype)
    return pad_fa_rows(flat, np.asarray(v_counts, dtype=np.int64), np.asarray(v_firsts, dtype=np.int64), depth)


def subsample_records(base_rows, variant_rows, counts, depths, replicates, nout):
    """(levels, windows) of subsample mode (c3_subsample_reduce; csrc/c3_subsample.h states the rule): ``base_rows`` (B, row) float32,
    ``variant_rows`` (variants, row) in the rule's order; row = nout or nout + DECODE_COLS.  levels: (B, L) of SUBSAMPLE_LEVEL_DTYPE;
    windows: (B,) of SUBSAMPLE_WINDOW_DTYPE."""
    base = np.asarray(base_rows, dtype=np.float32)
    var = np.asarray(variant_rows, dtype=np.float32)
    counts, depths, R = _subsample_plan(counts, depths, replicates)
    if base.ndim != 2 or var.ndim != 2 or nout not in (24, 90) or base.shape[1] not in (nout, nout + DECODE_COLS) or var.shape[1] != base.shape[1]:
        raise ValueError(f"base rows {base.shape} and variant rows {var.shape} are not rows of {nout} probabilities with or without the decoder columns")
    per_window = subsample_variant_counts(counts, depths, R)
    if counts.shape != (len(base),) or int(per_window.sum()) != len(var):
        raise ValueError(f"counts must hold one entry per window and the plan's {int(per_window.sum())} variants must be the {len(var)} rows given")
    columns = base.shape[1] > nout
    heads = head_slices(nout)
    L = len(depths)
    lev = np.zeros((len(base), L), dtype=SUBSAMPLE_LEVEL_DTYPE)
    win = np.zeros(len(base), dtype=SUBSAMPLE_WINDOW_DTYPE)
    at = 0
    for b in range(len(base)):
        y, n = base[b], int(counts[b])
        t = [lo + int(_first_argmax(y[None, lo:hi])[0]) for lo, hi in heads]
        win["reads"][b] = n
        for l, d in enumerate(depths):
            k = min(n, d)
            rec = lev[b, l]
            rec["keep"] = k
            for h in range(len(heads)):
                rec["min_kept"][h] = y[t[h]]
            if k == n:
                continue
            v = var[at:at + R]
            at += R
            rec["run"] = R
            win["levels_run"][b] += 1
            finite = np.isfinite(v[:, :nout]).all(axis=1)
            rec["nonfinite"] = int((~finite).sum())
            for h, (lo, hi) in enumerate(heads):
                rec["flips"][h] = int((lo + _first_argmax(v[:, lo:hi]) != t[h]).sum())
                if finite.any():
                    kept = v[finite, t[h]]
                    rec["min_kept"][h] = kept[int(np.argmin(kept))]  # the first of the smallest: -0 and +0 are a tie
                if rec["flips"][h]:
                    win["hold_level"][b, h] = l + 1
            if columns:
                rec["decision_flips"] = int((v[:, nout + 23:nout + 27] != y[None, nout + 23:nout + 27]).any(axis=1).sum())
                if rec["decision_flips"]:
                    win["hold_decision"][b] = l + 1
    return lev, win


# ---- occlusion mode in numpy: the definitions of csrc/c3_occlude.h (tests/test_occlude.py holds the two together) ----
OCCLUDE_WHAT = {"channels": 1, "bands": 2, "both": 3}  # C3_OCCLUDE_CHANNELS, C3_OCCLUDE_BANDS, both
# c3_occlude_window (include/c3hip.h), 144 bytes; [g]: group 0 = channels, group 1 = bands
OCCLUDE_DTYPE = np.dtype([("variants", "<i4"), ("nonfinite", "<i4"), ("flips", "<i4", (2, 4)), ("decision_flips", "<i4", (2, 4)),
                          ("lean", "<i4", (2, 4)), ("lean_drop", "<f4", (2, 4)), ("max_delta", "<f4"), ("reserved", "<i4")])


def occlude_groups(positions, channels, what="both", band=1):
    """(channels of group 0, bands of group 1) of a call: C or 0, and nb = ceil(P / band) or 0"""
    if what not in OCCLUDE_WHAT:
        raise ValueError(f"what must be one of {tuple(OCCLUDE_WHAT)}, got {what!r}")
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or not 1 <= band <= positions:
        raise ValueError(f"band must be an integer in 1 .. {positions}, got {band!r}")
    code = OCCLUDE_WHAT[what]
    return (channels if code & 1 else 0), (-(-positions // int(band)) if code & 2 else 0)


def occlude_variants(x, what="both", band=1):
    """The variants of occlusion mode of the windows ``x`` (B, ..., positions, channels) -- full-alignment (B, depth, P, C) or pileup
    (B, P, C), any dtype --, dense, (B * K, ...) in the order of c3_occlude: window after window, for each first the C variants with one
    channel set to zero (when what is "channels" or "both"), then the nb = ceil(P / band) variants with every channel of the columns
    [k * band, min(P, (k + 1) * band)) set to zero (when what is "bands" or "both").  Nothing else moves."""
    x = np.asarray(x)
    if x.ndim < 3:
        raise ValueError(f"windows (B, ..., positions, channels) expected, got shape {x.shape}")
    P, C = x.shape[-2:]
    nc, nb = occlude_groups(P, C, what, band)
    out = np.repeat(x[:, None], nc + nb, axis=1)  # (B, K, ..., P, C), a copy
    for c in range(nc):
        out[:, c, ..., c] = 0
    for k in range(nb):
        out[:, nc + k, ..., k * band:(k + 1) * band, :] = 0
    return out.reshape((len(x) * (nc + nb),) + x.shape[1:])


def occlude_records(base_rows, variant_rows, channels, bands, nout):
    """(records, drops) of occlusion mode (c3_occlude_reduce; csrc/c3_occlude.h states the definitions): ``base_rows`` (B, row) float32,
    ``variant_rows`` (B * K, row) with K = channels + bands, every window's variants in the order of occlude_variants; ``channels`` and
    ``bands`` are the sizes of the two groups (either may be 0); row = nout or nout + DECODE_COLS.  records: (B,) of OCCLUDE_DTYPE;
    drops: (B, K, 4) float32, y[t_h] - v_j[t_h].  Within a group the rule is jackknife_records' with the group's members as the reads."""
    base = np.asarray(base_rows, dtype=np.float32)
    var = np.asarray(variant_rows, dtype=np.float32)
    if channels < 0 or bands < 0:
        raise ValueError(f"group sizes must be >= 0, got {channels} and {bands}")
    K = int(channels) + int(bands)
    if base.ndim != 2 or var.ndim != 2 or nout not in (24, 90) or base.shape[1] not in (nout, nout + DECODE_COLS) or var.shape[1] != base.shape[1]:
        raise ValueError(f"base rows {base.shape} and variant rows {var.shape} are not rows of {nout} probabilities with or without the decoder columns")
    if len(var) != len(base) * K:
        raise ValueError(f"{len(base)} windows of {K} variants need {len(base) * K} variant rows, {len(var)} given")
    B, row = base.shape
    var = var.reshape(B, K, row)
    rec = np.zeros(B, dtype=OCCLUDE_DTYPE)
    rec["variants"] = K
    rec["lean"] = -1
    drops = np.zeros((B, K, 4), dtype=np.float32)
    for g, (lo, n) in enumerate(((0, int(channels)), (int(channels), int(bands)))):
        r, d = jackknife_records(base, var[:, lo:lo + n].reshape(B * n, row), np.full(B, n, np.int64), nout)
        rec["nonfinite"] += r["nonfinite"]
        rec["flips"][:, g], rec["decision_flips"][:, g] = r["flips"], r["decision_flips"]
        rec["lean"][:, g], rec["lean_drop"][:, g] = r["lean_read"], r["lean_drop"]
        rec["max_delta"] = np.maximum(rec["max_delta"], r["max_delta"])
        drops[:, lo:lo + n] = d.reshape(B, n, 4)
    return rec, drops


# ---- gVCF mode: the numpy mirror of csrc/c3_gvcf.h, for callers without a GPU and for the tests
GVCF_BLOCK_DTYPE = np.dtype([("pos", "<i8"), ("end", "<i8"), ("min_dp", "<i4"), ("max_dp", "<i4"), ("gq", "<i4"), ("pl", "<i4", (3,)),
                             ("ref", "u1"), ("gt", "u1"), ("per_site", "u1"), ("first_n", "u1"), ("reserved", "<i4")])  # c3_gvcf_block
GVCF_MAX_DEPTH = 65535
_GVCF_LOG_10, _GVCF_LOG_2, _GVCF_MAX_GQ = 2.3025, 0.3010, 50  # preprocess/utils.py:18-19, :360, as the reference writes them


def gvcf_site(n_ref, n_total, base_err=0.001, gq_bin_size=5):
    """(gq, binned_gq, validPL, (PL0, PL1, PL2)) of one site with an ACGT reference base: _cal_reference_likelihood and the PL lines of
    reference_likelihood (preprocess/utils.py:490-568) with the Python math of mathcalculator (speedUp off), round(., 6) included."""
    import math
    logp, log1p = math.log(base_err) / _GVCF_LOG_10, math.log1p(-base_err) / _GVCF_LOG_10

    def normalize(v):
        m = max(v)
        lse = round(m + math.log10(sum(pow(10.0, x - m) for x in v)), 6)
        return [min(x - lse, 0) for x in v]

    if n_total == 0:
        l = normalize([-1.0, -1.0, -1.0])
    else:
        n_alts = n_total - n_ref
        l = normalize([n_ref * log1p + n_alts * logp, -n_total * _GVCF_LOG_2, n_ref * logp + n_alts * log1p])
    ptrue = math.pow(10, l[0])
    gq = 50 if ptrue == 1 else round(-10 * (math.log(1 - ptrue) / _GVCF_LOG_10), 6)
    gq = int(min(int(gq), _GVCF_MAX_GQ))
    binned = (gq - 1) // gq_bin_size * gq_bin_size + 1 if gq >= 1 else 0
    t = [-10 * x for x in l]
    return gq, binned, l[0] == max(l), tuple(int(x - min(t)) for x in t)


def gvcf_f(x):
    """ceil(x + x * 0.3) in double: the block's largest depth may reach f(its smallest) (preprocess/utils.py:465, :476)"""
    x = np.asarray(x, dtype=np.float64)
    return np.ceil(x + x * 0.3).astype(np.int64)


def gvcf_region_counts(region, major, ref_bytes, first_major, n_sites):
    """(n_ref, n_total) int64 [n_sites] from a region as calculate_clair3_pileup leaves it (src/clair3_pileup.c:355-371, :452-455): site j
    takes the column whose major is first_major + j, a site without a column has 0 / 0.  The reference index is C 1, G 2, T 3, anything
    else 0 (base2index of the upper-cased byte); the strand sums are minus the two negated reference channels, ref_count the sums minus
    the other three bases' counts, all_alt_count the reference's running-maximum sum in index order, del 6 + 15, ins 4 + 13."""
    region = np.asarray(region).astype(np.int64)
    major = np.asarray(major, dtype=np.int64)
    ref = np.frombuffer(bytes(ref_bytes), dtype=np.uint8) if isinstance(ref_bytes, (bytes, bytearray)) else np.asarray(ref_bytes, dtype=np.uint8)
    if region.ndim != 2 or region.shape[1] != PILEUP_CHANNELS or major.shape != (len(region),) or len(ref) != n_sites:
        raise ValueError("region (n_cols, 18), major (n_cols,), ref_bytes (n_sites,) expected")
    n_ref, n_total = np.zeros(n_sites, np.int64), np.zeros(n_sites, np.int64)
    site = major - first_major
    keep = (site >= 0) & (site < n_sites)
    m, site = region[keep], site[keep]
    up = ref[site] & 0xDF
    r = np.select([up == ord("C"), up == ord("G"), up == ord("T")], [1, 2, 3], 0)
    ref_count = -(m[:, 0:4].sum(axis=1) + m[:, 9:13].sum(axis=1))  # -(negated sums) - (the other three bases), on both strands
    alt, all_alt = np.zeros(len(m), np.int64), np.zeros(len(m), np.int64)
    for k in range(4):
        cur = np.where(r == k, 0, m[:, k] + m[:, 9 + k])
        up_k = cur > alt
        alt = np.where(up_k, cur, alt)
        all_alt = all_alt + np.where(up_k, alt, 0)
    n_ref[site] = ref_count
    n_total[site] = ref_count + all_alt + m[:, 6] + m[:, 15] + m[:, 4] + m[:, 13]
    return n_ref, n_total


def gvcf_blocks(n_ref, n_total, ref_bytes, first_pos=0, base_err=0.001, gq_bin_size=5, bp_resolution=False):
    """The records of make_gvcf_online / write_to_gvcf_batch (preprocess/utils.py:398-488, :577-606) as (n,) of GVCF_BLOCK_DTYPE, by the
    reduction csrc/c3_gvcf.h states: a block from s runs on while no hard break (binned_gq, gt, is-exactly-N against the previous site)
    lies in it and max(dp) <= gvcf_f(min(dp))."""
    n_ref, n_total = np.asarray(n_ref, dtype=np.int64), np.asarray(n_total, dtype=np.int64)
    ref = np.frombuffer(bytes(ref_bytes), dtype=np.uint8) if isinstance(ref_bytes, (bytes, bytearray)) else np.asarray(ref_bytes, dtype=np.uint8)
    n = len(n_total)
    if n_ref.shape != (n,) or ref.shape != (n,):
        raise ValueError("n_ref, n_total and ref_bytes of one length expected")
    if n and ((n_ref < 0).any() or (n_ref > n_total).any() or (n_total > GVCF_MAX_DEPTH).any()):
        raise ValueError("counts must satisfy 0 <= n_ref <= n_total <= 65535")
    pairs, inv = np.unique(np.stack([n_total, n_ref], axis=1), axis=0, return_inverse=True) if n else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    recs = [gvcf_site(int(b), int(a), base_err, gq_bin_size) for a, b in pairs]
    inv = inv.reshape(-1)
    gq = np.array([r[0] for r in recs], np.int64)[inv] if n else np.zeros(0, np.int64)
    binned = np.array([r[1] for r in recs], np.int64)[inv] if n else np.zeros(0, np.int64)
    valid = np.array([r[2] for r in recs], bool)[inv] if n else np.zeros(0, bool)
    pl = np.array([r[3] for r in recs], np.int64).reshape(-1, 3)[inv] if n else np.zeros((0, 3), np.int64)
    acgt = np.isin(ref, np.frombuffer(b"ACGT", np.uint8))
    gq, binned, pl = np.where(acgt, gq, 1), np.where(acgt, binned, 1), np.where(acgt[:, None], pl, 0)
    is_n = ref == ord("N")
    printed = np.where(acgt, ref, ord("N")).astype(np.uint8)
    f = gvcf_f(np.arange(int(n_total.max()) + 1 if n else 1))  # by the smallest depth
    out = []

    def close(s, e, mn, mx, mgq):
        if (bp_resolution or not valid[s]) and acgt[s]:
            for i in range(s, e + 1):
                out.append((first_pos + i, first_pos + i, n_total[i], n_total[i], binned[i], tuple(pl[i]), printed[i], valid[i], 1, 0, 0))
        elif not acgt[s]:
            out.append((first_pos + s, first_pos + e, mn, mx, 1, (0, 0, 0), ord("N"), 0, 0, 1, 0))
        else:
            out.append((first_pos + s, first_pos + e, mn, mx, mgq, tuple(pl[s]), printed[s], valid[s], 0, 0, 0))

    s = 0
    for i in range(n):
        d = int(n_total[i])
        if i == 0:
            mn = mx = d
            mgq = gq[i]
            continue
        hard = binned[i] != binned[i - 1] or valid[i] != valid[i - 1] or is_n[i] != is_n[i - 1]
        mn2, mx2 = min(mn, d), max(mx, d)
        if hard or mx2 > f[mn2]:
            close(s, i - 1, mn, mx, mgq)
            s, mn, mx, mgq = i, d, d, gq[i]
        else:
            mn, mx, mgq = mn2, mx2, min(mgq, gq[i])
    if n:
        close(s, n - 1, mn, mx, mgq)
    return np.array(out, dtype=GVCF_BLOCK_DTYPE) if out else np.zeros(0, GVCF_BLOCK_DTYPE)


# ---- pileup from reads: read sets in BAM's own encoding (c3_read_set, include/c3hip.h)
NT16 = "=ACMGRSVTWYHKDBN"  # htslib's seq_nt16_str: the letter of a 4-bit code
CIGAR_OPS = "MIDNSHP=X"
PILEUP_DROP_FLAGS = (0x4, 0x100, 0x800, 0x200, 0x400)  # src/medaka_bamiter.c:20


def pack_reads(reads):
    """A read set from a list of (pos, flag, mapq, cigar, seq): cigar a string ("12M3I4M") or a list of (op letter, length), seq a string
    of nt16 letters.  The arrays of c3_read_set as a dict: pos, flag, mapq, cigar_first, cigar, seq_first, seq."""
    import re
    pos, flag, mapq, cfirst, cig, sfirst, seq = [], [], [], [0], [], [0], []
    for p, f, q, c, s in reads:
        if isinstance(c, str):
            c = [(m.group(2), int(m.group(1))) for m in re.finditer(r"(\d+)([MIDNSHP=X])", c)]
        pos.append(p), flag.append(f), mapq.append(q)
        cig.extend(n << 4 | CIGAR_OPS.index(o) for o, n in c)
        cfirst.append(len(cig))
        codes = np.array([NT16.index(b) for b in s], dtype=np.uint8)
        seq.append(_pack_nt16(codes))
        sfirst.append(sfirst[-1] + len(seq[-1]))
    return {"pos": np.array(pos, np.int64), "flag": np.array(flag, np.uint16), "mapq": np.array(mapq, np.uint8),
            "cigar_first": np.array(cfirst, np.int64), "cigar": np.array(cig, np.uint32), "seq_first": np.array(sfirst, np.int64),
            "seq": np.concatenate(seq) if seq else np.zeros(0, np.uint8)}


def _pack_nt16(codes):
    """4-bit codes, two per byte, high nibble first, padded to a byte"""
    if len(codes) & 1:
        codes = np.append(codes, np.uint8(0))
    return (codes[0::2] << 4 | codes[1::2]).astype(np.uint8)


def make_read_set(n_sites, depth, read_len, seed, start=2000, sub=0.01, ins=0.004, dele=0.004, soft_clip=0.2, n_op=0.0, non_acgt=0.0,
                  filtered=0.05, low_mapq=0.05, gaps=0, hot=0.03, d_then_i=0.0, i_then_d=0.0, pad=0.0, eqx=False, ref_other=0.0, min_mq=5,
                  hot_at=(), gap_at=()):
    """Aligned reads over a random reference, as a dict: the arrays of pack_reads, and start, end (the region [start, start + n_sites)),
    ref_bytes (uint8) with ref_first, and min_mq (what low_mapq is low against).  read_len: the reference span of a read, an int or
    (low, high).  Rates per reference position of a read: sub(stitutions), ins(ertions), dele(tions), n_op (N ops), d_then_i / i_then_d
    (a deletion directly followed by an insertion and the other way round), pad (a P op in front of an indel); non_acgt: read bases turned
    into other nt16 codes; per read: soft_clip (S or H at either end), filtered (one of the dropped flags), low_mapq.  hot: the share of
    reference positions that are variant sites, where half the reads carry one of a few alleles (two strings of one length, two deletion
    lengths): what makes candidates, and shared alleles on both strands; hot_at: (position, kind, alt) of variant sites placed by hand,
    kind 1 a SNP, 2 insertions of alt bases, 3 deletions of alt and alt + 1 bases.  gaps: stretches of the region no read covers (a read
    that would becomes two reads, one in front of the gap and one behind it), spread over the region; gap_at: (first, behind) of gaps placed by hand.  ref_other: reference bytes that are lower case or N.  Reads reach beyond both ends of the region, some lie wholly outside, none is sorted."""
    rng = np.random.default_rng(seed)
    lo_len, hi_len = (read_len, read_len) if np.isscalar(read_len) else read_len
    end = start + n_sites
    margin = 2 * hi_len + 64
    ref_first = max(0, start - margin)
    ref_len = end + margin + 64 - ref_first
    ref_codes = rng.integers(0, 4, size=ref_len)
    ref = np.frombuffer(b"ACGT", np.uint8)[ref_codes].copy()
    if ref_other > 0:
        odd = rng.random(ref_len) < ref_other
        ref[odd] = np.where(rng.random(int(odd.sum())) < 0.5, ref[odd] | 0x20, ord("N"))
    code_of = np.array([1, 2, 4, 8], np.uint8)
    # variant sites: kind 1 a SNP, 2 insertions, 3 deletions; each with two alleles
    hot_kind = np.where(rng.random(ref_len) < hot, rng.integers(1, 4, size=ref_len), 0)
    hot_alt = rng.integers(1, 4, size=ref_len)       # SNP: the alt base = ref + this (mod 4); indels: a length 1 .. 3
    hot_seed = rng.integers(0, 1 << 30, size=ref_len)
    for at, k, alt in hot_at:
        hot_kind[at - ref_first], hot_alt[at - ref_first] = k, alt
    gap_list = []
    for g in range(gaps):
        a = start + (g + 1) * n_sites // (gaps + 1)
        gap_list.append((a, a + int(rng.integers(3, 30))))
    gap_list = sorted(gap_list + [tuple(g) for g in gap_at])
    span_lo, span_hi = ref_first + 8, end + margin - hi_len - 8
    mean_len = (lo_len + hi_len) / 2.0
    n_reads = max(1, int(round(depth * (span_hi + mean_len - span_lo) / mean_len)))
    reads_pos, flags, mapqs, cfirst, cig, sfirst, seqs = [], [], [], [0], [], [0], []
    seq_bytes = 0
    M = CIGAR_OPS.index

    def random_bases(n):
        return code_of[rng.integers(0, 4, size=n)]

    def spans():
        """(first position, reference span) of every read; one that would cover a gap becomes two, in front of the gap and behind it"""
        for _ in range(n_reads):
            L = int(rng.integers(lo_len, hi_len + 1))
            p0 = int(rng.integers(span_lo, span_hi))
            last = p0 + L
            for a, b in gap_list:  # (ascending)
                if p0 < b and last > a:
                    if a - p0 >= 30:
                        yield p0, a - p0
                    p0 = b
            if last - p0 >= 30:
                yield p0, last - p0

    for p0, L in spans():
        o = p0 - ref_first
        q = code_of[ref_codes[o:o + L]].copy()
        s = rng.random(L) < sub
        q[s] = code_of[(ref_codes[o:o + L][s] + rng.integers(1, 4, size=int(s.sum()))) % 4]
        u = rng.random(L)
        kind = np.zeros(L, np.int8)
        edge = 0.0
        for code, rate in ((1, ins), (2, dele), (3, n_op), (4, d_then_i), (5, i_then_d)):
            kind[(u >= edge) & (u < edge + rate)] = code
            edge += rate
        hk = hot_kind[o:o + L]
        carry = (hk > 0) & (rng.random(L) < 0.5)
        second = rng.random(L) < 0.4  # the site's second allele
        snp = carry & (hk == 1)
        q[snp] = code_of[(ref_codes[o:o + L][snp] + hot_alt[o:o + L][snp] + second[snp]) % 4]
        kind[carry & (hk == 2)] = 6
        kind[carry & (hk == 3)] = 7
        kind[:2] = 0
        kind[-12:] = 0
        m_op = M("M") if not eqx else (M("M"), M("="), M("X"))[int(rng.integers(0, 3))]
        ops, pieces, cur = [], [], 0

        def emit_m(to):
            nonlocal cur
            if to > cur:
                if ops and ops[-1][0] == m_op:
                    ops[-1][1] += to - cur
                else:
                    ops.append([m_op, to - cur])
                pieces.append(q[cur:to])
                cur = to

        def emit_i(bases):
            ops.append([M("I"), len(bases)])
            pieces.append(bases)

        for i in np.flatnonzero(kind):
            i = int(i)
            if i < cur:
                continue
            emit_m(i + 1)
            k = int(kind[i])
            if pad > 0 and rng.random() < pad and k != 3:
                ops.append([M("P"), 1])
            room = L - 12 - cur
            if k == 1:
                emit_i(random_bases(int(min(1 + rng.geometric(0.5), 12))))
            elif k == 2 and room > 0:
                d = int(min(rng.geometric(0.5), room))
                ops.append([M("D"), d])
                cur += d
            elif k == 3 and room > 0:
                d = int(min(rng.integers(5, 40), room))
                ops.append([M("N"), d])
                cur += d
            elif k == 4 and room > 0:
                d = int(min(rng.geometric(0.5), room))
                ops.append([M("D"), d])
                cur += d
                emit_i(random_bases(int(rng.integers(1, 4))))
            elif k == 5 and room > 0:
                emit_i(random_bases(int(rng.integers(1, 4))))
                d = int(min(rng.geometric(0.5), room))
                ops.append([M("D"), d])
                cur += d
            elif k == 6:  # the site's insertion alleles: two strings of one length
                r2 = np.random.default_rng(int(hot_seed[o + i]) + int(second[i]))
                emit_i(code_of[r2.integers(0, 4, size=int(hot_alt[o + i]))])
            elif k == 7 and room > 0:  # the site's deletion alleles: two lengths
                d = int(min(int(hot_alt[o + i]) + int(second[i]), room))
                ops.append([M("D"), d])
                cur += d
        emit_m(L)
        if non_acgt > 0:
            for piece in pieces:
                bad = rng.random(len(piece)) < non_acgt
                piece[bad] = rng.choice(np.array([15, 3, 5, 0], np.uint8), size=int(bad.sum()))
        for front in (True, False):
            if rng.random() < soft_clip:
                n_clip = int(rng.integers(1, 20))
                hard = rng.random() < 0.3
                op = [M("H") if hard else M("S"), n_clip]
                ops.insert(0, op) if front else ops.append(op)
                if not hard:
                    pieces.insert(0, random_bases(n_clip)) if front else pieces.append(random_bases(n_clip))
        flag = 16 if rng.random() < 0.5 else 0
        if rng.random() < filtered:
            flag |= PILEUP_DROP_FLAGS[int(rng.integers(0, 5))]
        mapq = int(rng.integers(0, max(min_mq, 1))) if rng.random() < low_mapq else int(rng.integers(max(min_mq, 20), 61))
        reads_pos.append(p0), flags.append(flag), mapqs.append(mapq)
        cig.extend(n << 4 | op for op, n in ops)
        cfirst.append(len(cig))
        packed = _pack_nt16(np.concatenate(pieces))
        seqs.append(packed)
        seq_bytes += len(packed)
        sfirst.append(seq_bytes)
    return {"pos": np.array(reads_pos, np.int64), "flag": np.array(flags, np.uint16), "mapq": np.array(mapqs, np.uint8),
            "cigar_first": np.array(cfirst, np.int64), "cigar": np.array(cig, np.uint32), "seq_first": np.array(sfirst, np.int64),
            "seq": np.concatenate(seqs) if seqs else np.zeros(0, np.uint8), "start": start, "end": end, "ref_bytes": ref, "ref_first": ref_first,
            "min_mq": min_mq}


def tile_read_set(rs, copies):
    """`copies` shifted copies of a read set laid end to end: a long region at the cost of generating a short one (the rate tool)"""
    n_sites = rs["end"] - rs["start"]
    first, last = rs["start"] - rs["ref_first"], rs["end"] - rs["ref_first"]
    ref = np.concatenate([rs["ref_bytes"][:first]] + [rs["ref_bytes"][first:last]] * copies + [rs["ref_bytes"][last:]])
    out = dict(rs)
    out["pos"] = np.concatenate([rs["pos"] + k * n_sites for k in range(copies)])
    for name in ("flag", "mapq", "cigar", "seq"):
        out[name] = np.tile(rs[name], copies)
    for name, data in (("cigar_first", "cigar"), ("seq_first", "seq")):
        out[name] = np.concatenate([rs[name][:-1] + k * len(rs[data]) for k in range(copies)] + [np.array([copies * len(rs[data])], np.int64)])
    out["end"], out["ref_bytes"] = rs["start"] + copies * n_sites, ref
    return out


# ---- full alignment from reads: what a window needs beyond the read set (c3_read_extras, include/c3hip.h)
FA_DROP_FLAGS = 2316  # SAMTOOLS_VIEW_FILTER_FLAG, src/clair3_full_alignment_dwell.h:27


def sort_read_set(rs):
    """The read set in coordinate order (stable), as full alignment from reads wants it: make_read_set's reads are in none.  Returns a new
    dict; keys that are no read arrays are passed on."""
    order = np.argsort(rs["pos"], kind="stable")
    out = dict(rs)
    for name in ("pos", "flag", "mapq"):
        out[name] = rs[name][order]
    for first, data in (("cigar_first", "cigar"), ("seq_first", "seq")):
        pieces = [rs[data][rs[first][r]:rs[first][r + 1]] for r in order]
        out[data] = np.concatenate(pieces) if pieces else rs[data][:0]
        out[first] = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)
    return out


def query_lengths(rs):
    """(n,) int64: the query bases every read's CIGAR consumes (M, I, S, =, X)"""
    op, ln = rs["cigar"] & 15, (rs["cigar"] >> 4).astype(np.int64)
    consumed = np.where(np.isin(op, (0, 1, 4, 7, 8)), ln, 0)
    total = np.concatenate([[0], np.cumsum(consumed)])
    return total[rs["cigar_first"][1:]] - total[rs["cigar_first"][:-1]]


def make_read_extras(rs, seed, phased=0.6, duplicate_names=0.0):
    """Qualities, haplotypes and name keys for the reads of ``rs`` (make_read_set / pack_reads, in the order they have there), as a dict:
    qual_first, qual (one byte per query base, 0 .. 59), haplotype (0 with probability 1 - phased, else 1 or 2) and name_key (uint64; a
    share ``duplicate_names`` of the reads repeats the key of an earlier read).  ``rs`` is not changed."""
    rng = np.random.default_rng(seed)
    n = len(rs["pos"])
    qlen = query_lengths(rs)
    qual_first = np.concatenate([[0], np.cumsum(qlen)]).astype(np.int64)
    qual = rng.integers(0, 60, size=int(qual_first[-1])).astype(np.uint8)
    hap = np.where(rng.random(n) < phased, rng.integers(1, 3, size=n), 0).astype(np.uint8)
    key = rng.integers(1, 1 << 62, size=n).astype(np.uint64)
    for r in np.flatnonzero(rng.random(n) < duplicate_names):
        if r > 0:
            key[r] = key[int(rng.integers(0, r))]
    return {"qual_first": qual_first, "qual": qual, "haplotype": hap, "name_key": key}


def sort_read_extras(rs, extras):
    """``extras`` of the unsorted ``rs`` put into the order sort_read_set(rs) gives the reads"""
    order = np.argsort(rs["pos"], kind="stable")
    pieces = [extras["qual"][extras["qual_first"][r]:extras["qual_first"][r + 1]] for r in order]
    return {"qual_first": np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64),
            "qual": np.concatenate(pieces) if pieces else extras["qual"][:0], "haplotype": extras["haplotype"][order],
            "name_key": extras["name_key"][order]}


def make_read_moves(rs, extras, seed, mean=2.2, stall=0.002, untagged=0.05, surplus=0.05, short=0.05):
    """Nanopore move tables (the mv:B:c tag) for the reads of ``rs`` in the order they have there, as a dict: mv_first (n + 1,) int64 and mv
    int8, read r owning mv[mv_first[r]:mv_first[r + 1]].  Element 0 of a table is the stride (5: non-zero, and it must not count); up to
    three zeros may stand in front of the first move.  A move is 1 (now and then -1 or 5) and is followed by its zeros: about ``mean``
    entries per base; a share ``stall`` of the bases dwells 128 .. 191 entries and a quarter of that share 256 .. 319.  A share
    ``untagged`` of the reads has no table, a share ``surplus`` more moves than quality bytes (K > l), a share ``short`` fewer (K < l).
    Seeded; ``rs`` and ``extras`` are not changed."""
    rng = np.random.default_rng(seed)
    qlen = np.diff(np.asarray(extras["qual_first"], np.int64))
    tables = []
    for l in qlen.tolist():
        kind = rng.random()
        if kind < untagged or l == 0:
            tables.append(np.zeros(0, np.int8))
            continue
        k = l
        if kind < untagged + surplus:
            k = l + int(rng.integers(1, 6))
        elif kind < untagged + surplus + short:
            k = max(l - int(rng.integers(1, 6)), 0)
        dwell = 1 + rng.poisson(max(mean - 1.0, 0.0), size=k)
        u = rng.random(k)
        dwell = np.where(u < stall, 128 + rng.integers(0, 64, size=k), dwell)
        dwell = np.where(u < stall / 4, 256 + rng.integers(0, 64, size=k), dwell)
        lead = int(rng.integers(0, 4))
        at = 1 + lead + np.concatenate([[0], np.cumsum(dwell)]).astype(np.int64)
        mv = np.zeros(int(at[-1]), np.int8)
        mv[0] = 5
        mv[at[:-1]] = np.where(rng.random(k) < 0.9, 1, np.where(rng.random(k) < 0.5, -1, 5))
        tables.append(mv)
    return {"mv_first": np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64),
            "mv": np.concatenate(tables) if tables else np.zeros(0, np.int8)}


def sort_read_moves(rs, moves):
    """``moves`` of the unsorted ``rs`` put into the order sort_read_set(rs) gives the reads"""
    order = np.argsort(rs["pos"], kind="stable")
    pieces = [moves["mv"][moves["mv_first"][r]:moves["mv_first"][r + 1]] for r in order]
    return {"mv_first": np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64),
            "mv": np.concatenate(pieces) if pieces else moves["mv"][:0]}


def fa_keys(seed, centre, reads):
    """(n,) uint64: fa_key(seed, centre, read) of csrc/c3_fa_rule.h for the read indices ``reads`` -- the counter hash of subsample mode, the
    selection being subsample_rank(keys, matrix_depth)"""
    g = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        inner = subsample_mix(np.uint64(int(seed) & _M64) + g * np.uint64((1 + int(centre)) & _M64))
        return subsample_mix(inner + g * (np.uint64(1) + np.asarray(reads, dtype=np.uint64)))


# ---- haplotagging the reads: the phased heterozygous SNPs of a contig (c3_phased_variants, include/c3hip.h)
def make_phased_variants(rs, seed, rate=0.02, hot_at=(), dense=None, near=(), set_span=80):
    """Phased het SNPs over the reference of ``rs`` (make_read_set / a dict with pos, cigar_first, cigar, ref_bytes, ref_first), as a dict:
    pos (int64, 0-based, strictly ascending), alt_base (uint8 letters), genotype (uint8, 1 = 0|1, 2 = 1|0), phase_set (int32).  Sites: a
    share ``rate`` of the reference positions; the SNP sites of ``hot_at`` (the (position, 1, alt) entries given to make_read_set: the alt
    base is the site's first allele there, so about half the reads carry it); ``dense`` = (first, behind): a site every 2 or 3 bases in
    that stretch; ``near``: read indices of ``rs`` -- sites at those reads' first and last bases, 9 / 10 / 11 bases inside either end,
    just behind the end, and at, in front of and behind every I, D and N op.  Phase sets are stretches of ``set_span`` bases (a set's
    name is its first position + 1), so that a read usually touches several.  Every site keeps 10 bases of reference in front of it and 11
    behind, so that every context is covered."""
    rng = np.random.default_rng(seed)
    ref, ref_first = np.asarray(rs["ref_bytes"]), int(rs["ref_first"])
    lo, hi = ref_first + 10, ref_first + len(ref) - 11
    sites = {}
    for p in np.flatnonzero(rng.random(len(ref)) < rate):
        sites[int(p) + ref_first] = None
    if dense is not None:
        p = int(dense[0])
        while p < int(dense[1]):
            sites[p] = None
            p += int(rng.integers(2, 4))
    for r in near:
        r = int(r)
        p0 = int(rs["pos"][r])
        at, marks = p0, [p0, p0 + 9, p0 + 10, p0 + 11]
        for c in rs["cigar"][rs["cigar_first"][r]:rs["cigar_first"][r + 1]]:
            op, n = int(c) & 15, int(c) >> 4
            if op in (1, 2, 3):
                marks += [at - 1, at, at + 1]
            if op in (2, 3):
                marks += [at + n - 1, at + n]
            if op in (0, 2, 3, 7, 8):
                at += n
        marks += [at - 12, at - 11, at - 10, at - 1, at]
        for p in marks:
            sites[p] = None
    for p, kind, alt in hot_at:
        if kind == 1:
            sites[int(p)] = int(alt)
    pos = np.array(sorted(p for p in sites if lo <= p < hi), np.int64)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ref_at = ref[pos - ref_first]
    code = np.searchsorted(acgt, ref_at & 0xDF).clip(0, 3)  # (a byte that is no base counts as one: the alt base is some other letter)
    shift = np.array([sites[int(p)] if sites[int(p)] is not None else int(rng.integers(1, 4)) for p in pos], np.int64).reshape(-1)
    return {"pos": pos, "alt_base": acgt[(code + shift) % 4].astype(np.uint8), "genotype": rng.integers(1, 3, size=len(pos)).astype(np.uint8),
            "phase_set": ((pos // set_span) * set_span + 1).astype(np.int32)}
