"""Drop-in replacements for the model-call helpers of the reference worker
(/root/reference/clair3/CallVariantsFromCffi.py:19-52) and the GPU-slot probe of the GPU wrapper
(/root/reference/clair3/CallVariantsFromCffiGPU.py:13-43).  Same names, same argument meaning, same
error behaviour (loaders raise; callers keep their sys.exit handling).
"""
import numpy as np

from . import _lib
from .model import Clair3_F, Clair3_P, _device_index


def _read_checkpoint(checkpoint_path):
    """the state dict of a checkpoint file, as _load_torch_checkpoint reads it: '.pt' appended when missing, a bare state_dict or
    {"state_dict": ...}.  The file is read by clair3_amd/ptfile.py (numpy only: a worker process that never needs torch never imports it,
    clair3_amd/lazy_torch.py); what that reader does not handle -- the legacy non-zip format, exotic dtypes, pickled modules -- goes to
    torch.load(map_location='cpu') as before (C3HIP_PTFILE=0: always)."""
    import os
    from . import ptfile
    if not checkpoint_path.endswith('.pt'):
        checkpoint_path = checkpoint_path + '.pt'
    checkpoint = None
    if os.environ.get("C3HIP_PTFILE", "1").strip().lower() not in ("0", "false", "no", "off"):
        try:
            checkpoint = ptfile.load(checkpoint_path)
        except ptfile.Unsupported:
            checkpoint = None
    if checkpoint is None:
        import torch
        checkpoint = torch.load(checkpoint_path, map_location="cpu")
    if isinstance(checkpoint, dict) and "state_dict" in checkpoint:
        return checkpoint["state_dict"]
    return checkpoint


def _load_torch_checkpoint(model, checkpoint_path, device=None):
    """clair3/CallVariantsFromCffi.py:19-28: append '.pt' when missing, deserialise, accept a bare state_dict or {"state_dict": ...},
    strict load; then what the environment asks of a model where it is built (C3HIP_CALIBRATION, C3HIP_VERIFY, C3HIP_REFINE)."""
    model.load_state_dict(_read_checkpoint(checkpoint_path))
    _register_current(model)
    calibration_from_env(model)
    verify_from_env(model)
    exact_from_env(model)
    answer_from_env(model)
    refine_from_env(model)
    range_guard_from_env(model)


def parse_answer_env(value):
    """C3HIP_ANSWER=exact | product -> "exact" | "product"; None when unset or empty.  Anything else raises."""
    value = (value or "").strip().lower()
    if not value:
        return None
    if value not in _lib.ANSWER:
        raise _lib.C3Error(f"C3HIP_ANSWER must be exact or product, got {value!r}")
    return value


def parse_verify_ref_env(value):
    """C3HIP_VERIFY_REF=exact | fp32 -> "exact" | "fp32"; None when unset or empty.  Anything else raises."""
    value = (value or "").strip().lower()
    if not value:
        return None
    if value not in _lib.VERIFY_REF:
        raise _lib.C3Error(f"C3HIP_VERIFY_REF must be exact or fp32, got {value!r}")
    return value


def exact_from_env(model):
    """C3HIP_EXACT=1: the model takes the exact form along where it is built (model.exact(): the double weights travel with its loads);
    unset, empty or 0: the model is left alone.  Anything else raises.  C3HIP_ANSWER=exact and C3HIP_VERIFY_REF=exact (with C3HIP_VERIFY
    on) imply it, as C3HIP_EXACT=1 does."""
    import os
    value = (os.environ.get("C3HIP_EXACT") or "").strip()
    answer = parse_answer_env(os.environ.get("C3HIP_ANSWER"))
    ref = parse_verify_ref_env(os.environ.get("C3HIP_VERIFY_REF"))
    implied = answer == "exact" or (ref == "exact" and parse_verify_env(os.environ.get("C3HIP_VERIFY")) is not None)
    implied = implied or parse_refine_env(os.environ.get("C3HIP_REFINE")) is not None  # (refine mode answers near-ties from the exact form)
    if value not in ("", "0", "1"):
        raise _lib.C3Error(f"C3HIP_EXACT must be 0 or 1, got {value!r}")
    if value != "1" and (not implied or getattr(model, "_exact", False)):  # (implied only: verify_from_env may have enabled it already)
        return False
    model.exact(True)
    return True


def answer_from_env(model):
    """C3HIP_ANSWER=exact: the model answers the batches of the ring from the exact form where it is built (model.answer()); product, unset
    or empty: the model is left alone.  Called behind exact_from_env, which placed the double weights."""
    import os
    answer = parse_answer_env(os.environ.get("C3HIP_ANSWER"))
    if answer != "exact":
        return False
    model.answer("exact")
    return True


def parse_refine_env(value):
    """C3HIP_REFINE=<gap> -> the gap of ``model.refine`` as a float; None when unset, empty or 0.  Anything that is not a number >= 0
    raises: a job asked to refine its near-ties must not run unrefined because of a typo."""
    if value is None or not value.strip():
        return None
    try:
        gap = float(value)
    except ValueError as e:
        raise _lib.C3Error(f"C3HIP_REFINE must be a gap >= 0 (0 = off), got {value!r}") from e
    if not gap >= 0 or not np.isfinite(gap):
        raise _lib.C3Error(f"C3HIP_REFINE must be a gap >= 0 (0 = off), got {value!r}")
    return gap if gap > 0 else None


# models of this process that run in refine mode because the environment said so: their totals go to stderr when the process ends
_REFINED = []


def refine_from_env(model):
    """C3HIP_REFINE=<gap>: refine mode where the model is built (model.refine(gap); README), behind exact_from_env, which placed the double
    weights it implies.  Together with C3HIP_VERIFY it raises: the two own the same rows.  In a worker process one summary line per such
    model goes to stderr at exit; stdout and the VCF stay untouched."""
    import os
    gap = parse_refine_env(os.environ.get("C3HIP_REFINE"))
    if gap is None:
        return False
    if parse_verify_env(os.environ.get("C3HIP_VERIFY")) is not None:
        raise _lib.C3Error("C3HIP_REFINE and C3HIP_VERIFY are both set: refine mode and verify mode own the same rows, choose one")
    model.refine(gap)
    if not any(v is model for v in _REFINED):
        import atexit
        if not _REFINED:
            atexit.register(_report_refined)
        _REFINED.append(model)  # (held until the process ends, like _VERIFIED)
    return True


def refine_summary(model):
    """the line a worker leaves on stderr: the totals of refine mode (INTEGRATION.md 8 says how to read it)"""
    st = model.refine_stats()
    return ("[clair3_amd] refine: gap={:g} batches={} refined={} skipped={} windows={} selected={} changed={} per_head={} decoder={} "
            "min_gap={} max_abs_diff={:.3g}").format(
        st["gap"], st["batches"], st["batches_refined"], st["batches_skipped"], st["windows"], st["windows_selected"], st["windows_changed"],
        "/".join(str(v) for v in st["head_selected"]), st["decoder_selected"], "/".join(f"{v:.3g}" for v in st["min_gap"]), st["max_abs_diff"])


def _report_refined():
    import sys
    for model in _REFINED:
        if model._handle is None:
            continue
        try:
            print(refine_summary(model), file=sys.stderr)
        except Exception as e:  # noqa: BLE001  (the process is ending: say it, do not raise)
            print(f"[clair3_amd] refine: no summary ({e})", file=sys.stderr)


def calibration_from_env(model):
    """C3HIP_CALIBRATION=<file>: a full-alignment model takes the calibration file (clair3_amd/calibrate.py) where it is built, so that every
    worker process of a job runs the same channel exponents; a pileup model ignores it.  A file that is missing, invalid or made for another
    checkpoint raises: a job asked to run calibrated must not run uncalibrated because of a typo."""
    import os
    path = os.environ.get("C3HIP_CALIBRATION")
    if not path or not path.strip() or getattr(model, "KIND", None) != _lib.KIND_FULL_ALIGNMENT:
        return False
    if model._pending_sd is None:  # built without a checkpoint: the file is checked now and applied by the model's first load_state_dict
        from . import calibrate as cal
        cal.read_file(path.strip())
        model._calibration_file = path.strip()
        return True
    model.load_calibration(path.strip())
    return True


def parse_verify_env(value, tol=None):
    """C3HIP_VERIFY=<n> | <n>,escalate | <n>,replace (and C3HIP_VERIFY_TOL=<tol>) -> the keyword arguments of ``model.verify``; None when
    unset, empty or 0.  Anything else that is not such a setting raises: a job asked to verify must not run unverified because of a typo.
    ``replace`` appears among the keywords only when the word is used: without it the result is what it always was."""
    if value is None or not value.strip():
        return None
    parts = [p.strip().lower() for p in value.split(",")]
    if len(parts) > 2 or (len(parts) == 2 and parts[1] not in ("escalate", "report", "replace")):
        raise _lib.C3Error(f"C3HIP_VERIFY must be <n> or <n>,escalate (every n-th batch; 0 = off), got {value!r}")
    try:
        every = int(parts[0])
    except ValueError as e:
        raise _lib.C3Error(f"C3HIP_VERIFY must be <n> or <n>,escalate (every n-th batch; 0 = off), got {value!r}") from e
    if every < 0:
        raise _lib.C3Error(f"C3HIP_VERIFY: n must be >= 0, got {every}")
    kw = dict(every=every, escalate=len(parts) == 2 and parts[1] == "escalate")
    if len(parts) == 2 and parts[1] == "replace":
        kw["replace"] = True
    if tol is not None and tol.strip():
        try:
            kw["tol"] = float(tol)
        except ValueError as e:
            raise _lib.C3Error(f"C3HIP_VERIFY_TOL must be a number > 0, got {tol!r}") from e
        if not kw["tol"] > 0:
            raise _lib.C3Error(f"C3HIP_VERIFY_TOL must be a number > 0, got {tol!r}")
    return kw if every > 0 else None


# models of this process that run in verify mode because the environment said so: their totals go to stderr when the process ends
_VERIFIED = []


def verify_from_env(model):
    """Switch verify mode on where the model is built, as C3HIP_VERIFY / C3HIP_VERIFY_TOL say (README).  In a worker process one summary
    line per such model goes to stderr at exit; stdout and the VCF stay untouched."""
    import os
    kw = parse_verify_env(os.environ.get("C3HIP_VERIFY"), os.environ.get("C3HIP_VERIFY_TOL"))
    if kw is None:
        return False
    if os.environ.get("C3HIP_VERIFY_LAYERS", "").strip().lower() not in ("", "0", "false", "no", "off"):
        kw["layers"] = True  # (only when set: without it the call is what it was; _report_verified follows the handle, not the environment)
    ref = parse_verify_ref_env(os.environ.get("C3HIP_VERIFY_REF"))
    if ref is not None and ref != "fp32":
        kw["reference"] = ref  # (only when the reference is not the default's)
        if not getattr(model, "_exact", False):
            model.exact(True)  # (the reference needs the double weights: implied, as by C3HIP_EXACT=1)
    model.verify(**kw)
    if not any(v is model for v in _VERIFIED):
        import atexit
        if not _VERIFIED:
            atexit.register(_report_verified)
        _VERIFIED.append(model)  # (held until the process ends: the loop's own reference is gone by then, and with it the handle's totals)
    return True


def verify_summary(model):
    """the line a worker leaves on stderr: the handle's precision and the totals of verify mode (INTEGRATION.md says how to read it)"""
    import re
    st = model.verify_stats()
    prec = re.search(r"precision=(\S+)", model.describe())
    line = ("[clair3_amd] verify: precision={} every={} policy={} tol={:g} batches submitted={} checked={} skipped={} windows={} "
            "max_abs_diff={:.3g} per_head={} worst=(batch {}, row {}) rows_over_tol={} label_diffs={} near_ties={} escalations={}").format(
        prec.group(1) if prec else "?", st["every"], st["policy"], st["tol"], st["batches_submitted"], st["batches_checked"],
        st["batches_skipped"], st["windows_checked"], st["max_abs_diff"], "/".join(f"{v:.3g}" for v in st["head_max_abs_diff"]),
        st["worst_batch"], st["worst_row"], st["rows_over_tol"], st["label_diffs"], st["near_ties"], st["escalations"])
    extra = model.verify_extra() if hasattr(model, "verify_extra") else None
    if extra is not None and extra["reference"] == "exact":  # (at the end, and only then: the line is otherwise what it always was)
        line += " ref=exact replaced={}".format(extra["rows_replaced"])
    return line


# the suite's layer gate (tests/test_caller_inputs_gpu.py LAYER_TOL): a layer whose rel = max_abs_diff / max(1, ref_max_abs) exceeds it is marked
LAYER_TOL = 2e-5


def verify_layer_lines(layers):
    """the lines a worker leaves behind its summary line under C3HIP_VERIFY_LAYERS=1, one per layer of ``model.verify_layers()`` in network
    order (INTEGRATION.md 8 says how to read them).  A layer beyond LAYER_TOL ends on " <<"."""
    lines = []
    for e in layers:
        if e["status"] != "compared":
            lines.append("[clair3_amd] verify layer {:<10s} {}".format(e["name"], "fused (not materialised by the product form)" if e["status"] == "fused"
                                                                   else "no batch compared"))
            continue
        lines.append("[clair3_amd] verify layer {:<10s} batches={} windows={} max_abs_diff={:.3g} ref_max_abs={:.3g} test_max_abs={:.3g} rel={:.3g} "
                     "worst=(batch {}, window {}, index {}){}".format(
                         e["name"], e["batches"], e["windows"], e["max_abs_diff"], e["ref_max_abs"], e["test_max_abs"], e["rel"],
                         e["worst_batch"], e["worst_window"], e["worst_index"], " <<" if not e["rel"] <= LAYER_TOL else ""))
    return lines


def _report_verified():
    import sys
    for model in _VERIFIED:
        if model._handle is None:
            continue
        try:
            print(verify_summary(model), file=sys.stderr)
            if getattr(model, "_verify_layers", False):
                for line in verify_layer_lines(model.verify_layers()):
                    print(line, file=sys.stderr)
        except Exception as e:  # noqa: BLE001  (the process is ending: say it, do not raise)
            print(f"[clair3_amd] verify: no summary ({e})", file=sys.stderr)


# full-alignment models of this process built under C3HIP_RANGE_GUARD: what their range guard did goes to stderr when the process ends
_GUARDED = []


def range_guard_from_env(model):
    """C3HIP_RANGE_GUARD=sticky | recalibrate | recalibrate:<n> is read by the library where the handle is created (README); here the
    model is only noted, so that a worker process whose handle tripped leaves one line on stderr at exit.  stdout and the VCF stay untouched."""
    import os
    value = os.environ.get("C3HIP_RANGE_GUARD")
    if not value or getattr(model, "KIND", None) != _lib.KIND_FULL_ALIGNMENT or any(g is model for g in _GUARDED):
        return False
    import atexit
    if not _GUARDED:
        atexit.register(_report_guarded)
    _GUARDED.append(model)  # (held until the process ends, like _VERIFIED)
    return True


def range_guard_summary(model):
    """the line a worker leaves on stderr when its range guard tripped (INTEGRATION.md 8 says how to read it); None without a trip"""
    import re
    st = model.range_stats()
    if st["trips"] == 0:
        return None
    prec = re.search(r"precision=(\S+)", model.describe())
    return ("[clair3_amd] range guard: policy={}:{} precision={} trips={} recalibrations={} reruns={} channels_lowered={} cap_log2={} "
            "census_windows={} fell_back={}").format(
        st["policy"], st["max_recalibrations"], prec.group(1) if prec else "?", st["trips"], st["recalibrations"], st["reruns"],
        st["channels_lowered"], st["cap_log2"], st["census_windows"], repr(st["fell_back"]) if st["fell_back"] else "no")


def _report_guarded():
    import sys
    for model in _GUARDED:
        if model._handle is None:
            continue
        try:
            line = range_guard_summary(model)
            if line:
                print(line, file=sys.stderr)
        except Exception as e:  # noqa: BLE001  (the process is ending: say it, do not raise)
            print(f"[clair3_amd] range guard: no summary ({e})", file=sys.stderr)


# The model the worker process is calling variants with: the reference loop creates ONE model, loads it here, and only then
# creates its batch generator (clair3/CallVariantsFromCffi.py:246-273), so the rebound generator (callvar.install: the
# transport of clair3_amd/worker.py behind tensor_generator_for_chunk) can find the handle it should run ahead on.
_CURRENT_MODEL = None
# id(X) -> (model, group, X, lo, hi) of batches the rebound generator has already submitted (worker.lookahead_batches)
_PENDING = {}


def _register_current(model):
    global _CURRENT_MODEL
    import weakref
    _CURRENT_MODEL = weakref.ref(model) if hasattr(model, "submit") else None


def current_model():
    return _CURRENT_MODEL() if _CURRENT_MODEL is not None else None


def _select_device(use_gpu=True):
    """clair3/CallVariantsFromCffi.py:31-34 returns cpu when no GPU is usable; this path has no CPU
    implementation, so an unusable GPU is an error instead of a silent fallback."""
    if not use_gpu:
        raise _lib.C3Error("clair3_amd is the GPU path; run the reference for CPU inference")
    if _lib.device_count() < 1:
        raise _lib.C3Error("no MI355X / HIP device visible")
    return "cuda:0"


# set by callvar.install(decoder=True): the rows (24 or 90 probabilities) also carry the decoder columns
# (clair3_amd/decode.py) that the rebound batch_output consumes
DECODER_COLUMNS = False


def _hip_predict(model, device, X):
    """_torch_predict(model, device, X) (clair3/CallVariantsFromCffi.py:48-52): numpy windows in, numpy
    float32 (B, 24|90) probabilities out; H2D, forward and D2H are done by libc3hip (pinned staging).
    With DECODER_COLUMNS the rows are followed by model.DECODE_COLS decoder columns."""
    if device is not None and model._device is not None and _device_index(device) != model._device:
        model.to(device)
    ent = _PENDING.pop(id(X), None)
    if ent is not None and ent[0] is model and ent[2] is X:
        # submitted ahead by the rebound batch generator (worker.lookahead_batches), alone or in a group of consecutive
        # batches: the rows are on their way or here
        return ent[1].take(ent[3], ent[4])
    want = bool(DECODER_COLUMNS)
    if want != model._decode_cols:
        model.decode_columns(want)
    return model.predict_numpy(np.asarray(X))


_torch_predict = _hip_predict  # the name the reference call sites use


def depths_from_alt_info(alt_info_list):
    """The per-window depths of a batch as the reference's loops read them before they rescale deep pileup windows
    (clair3/CallVariantsFromCffi.py:280, clair3/utils.py:106: ``int(alt_info.split('-', maxsplit=1)[0])``), as the int32 array
    ``Clair3_P.predict_numpy(x, depths=...)`` / ``predict_region`` / ``submit`` take."""
    out = np.empty(len(alt_info_list), dtype=np.int32)
    for i, alt_info in enumerate(alt_info_list):
        try:
            out[i] = int(alt_info.split('-', maxsplit=1)[0])
        except (ValueError, AttributeError, OverflowError) as e:
            raise _lib.C3Error(f"alt_info {i} does not start with an integer depth: {alt_info!r}") from e
    return out


def pack_rows(x):
    """(rows, firsts, counts) of dense full-alignment windows ``x`` (B, depth, positions, C) int8, as ``Clair3_F.predict_rows(rows, counts,
    firsts)`` takes them (c3_pack_rows; plain host code, no device): for every window the run from its first to its last non-zero row --
    interior zero rows stay inside the run, an all-zero window gives count 0 and first 0.  ``x`` is not written."""
    x = np.ascontiguousarray(x)
    if x.dtype != np.int8 or x.ndim != 4:
        raise _lib.C3Error(f"windows must be (B, depth, positions, C) int8, got {x.dtype} {x.shape}")
    b, depth, positions, channels = x.shape
    firsts, counts = np.empty(b, dtype=np.int32), np.empty(b, dtype=np.int32)
    rows = np.empty((b * depth, positions, channels), dtype=np.int8)
    n = _lib.lib().c3_pack_rows(depth, positions, channels, x.ctypes.data, b, rows.ctypes.data, firsts.ctypes.data, counts.ctypes.data)
    if n < 0:
        raise _lib.C3Error(f"c3_pack_rows: {_lib.last_error()}")
    return rows[:n], firsts, counts


def build_model(pileup, add_indel_length, platform="ont", enable_dwell_time=False, device=0, chkpnt_fn=None):
    """Model factory block of call_variants_from_cffi (clair3/CallVariantsFromCffi.py:223-248)."""
    if platform != "ont":
        # hifi/ilmn use a 55-row matrix (shared/param_f.py:11); golden case fa_hifi_depth55
        depth = 55
    else:
        depth = 89
    if pileup:
        m = Clair3_P(add_indel_length=add_indel_length, predict=True, input_channels=18)
    else:
        m = Clair3_F(add_indel_length=add_indel_length, predict=True, input_channels=9 if enable_dwell_time else 8)
        m.set_geometry(depth, 33)
    m.to(device)
    m.eval()
    if chkpnt_fn is not None:
        _load_torch_checkpoint(m, chkpnt_fn, device)
    else:  # (with a checkpoint the loader has done both)
        calibration_from_env(m)
        verify_from_env(m)
        exact_from_env(m)
        answer_from_env(m)
        refine_from_env(m)
        range_guard_from_env(m)
    return m


def get_gpu_memory(gpu_id=None):
    """Free device memory in MB, one entry per queried device -- same return shape as the nvidia-smi parser it
    replaces (clair3/CallVariantsFromCffiGPU.py:13-19) but through hipMemGetInfo (c3_mem_info)."""
    ids = range(_lib.device_count()) if gpu_id is None else [int(gpu_id)]
    return [int(_lib.mem_info(d)[0] // (1024 * 1024)) for d in ids]


# Worker processes ("GPU threads") per MI355X.  The reference sizes this for 16-80 GB CUDA cards: free_MB // 8000 (full
# alignment) or // 5000 (pileup) processes per device (clair3/CallVariantsFromCffiGPU.py:33-34,55-56) -- 36 / 57 on a 288 GB
# MI355X, each with its own HIP context, workspace (up to ~3 GB for pileup), staging threads and `cpu_threads` decode
# processes, all behind one PCIe link.  One libc3hip handle fed through its submit / wait ring already fills the chip
# (bench.py: host-inclusive rate 0.9-0.97 of the device-resident one; three handles side by side add < 10 % on the device and
# LOSE when fed from the host), so the slot count is 1 per device unless C3HIP_SLOTS_PER_GPU says otherwise
# (capped by the reference's own memory rule).
def slots_per_gpu():
    import os
    try:
        return max(1, int(os.environ.get("C3HIP_SLOTS_PER_GPU", "1")))
    except ValueError:
        return 1


def check_gpu_memory(memory, device_ids=None, print_log=True):
    """clair3/CallVariantsFromCffiGPU.py:21-43: returns the device id repeated once per worker slot.  The reference gives
    every `memory` MB of free device memory a slot; here a device gets min(that, slots_per_gpu()) slots -- see above.
    ``device_ids`` (from ``--device=cuda:2,3``, :60-65) are the PHYSICAL ids the caller exported as CUDA_VISIBLE_DEVICES
    before asking: visible ordinal i is physical device_ids[i], and that is what a slot must carry, because the slot's
    worker sets CUDA_VISIBLE_DEVICES to it (clair3/CallVariantsFromCffi.py:216; the reference returns the ordinal there).
    The reference sys.exit(1)s when nothing is usable; this raises C3Error and the installed wrapper
    (callvar.install) converts it back into the exit."""
    all_device_ids = list(range(_lib.device_count()))
    if device_ids is None:
        device_ids = all_device_ids
    if not all_device_ids:
        return
    gpu_id_list = []
    cap = slots_per_gpu()
    for device_id in all_device_ids:
        free_mem = get_gpu_memory(gpu_id=device_id)[0]
        by_memory = int(free_mem // memory)
        gpu_threads = min(by_memory, cap)
        physical = device_ids[device_id] if device_id < len(device_ids) else device_id
        gpu_id_list += [physical] * gpu_threads
        if print_log:
            print(f"GPU {physical} free memory: {free_mem} MB, assigning {memory} MB per thread, "
                  f"{gpu_threads} threads available (one libc3hip worker fills an MI355X; the reference's "
                  f"free // {memory} rule would start {by_memory}; C3HIP_SLOTS_PER_GPU overrides)")
    if len(device_ids) == 0:
        raise _lib.C3Error("No GPU available, Please disabling --use_gpu for variant calling, exiting.")
    if len(gpu_id_list) == 0:
        raise _lib.C3Error("No memory in GPU, Please assign GPU memory first, exiting.")
    return gpu_id_list
