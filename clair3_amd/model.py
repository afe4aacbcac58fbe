"""Host-side mirror of the reference's model interface for the hot path.

``Clair3_P`` / ``Clair3_F`` take the same constructor arguments as the reference modules
(/root/reference/clair3/model.py:61, :285), load the same state_dict / ``.pt`` checkpoints
(clair3/CallVariantsFromCffi.py:19-28) and are called the same way -- ``Y = model(X)`` -- but the forward
pass runs in hand-written HIP kernels (libc3hip.so) instead of ATen.  PyTorch is used only to read
checkpoints and, optionally, to own device tensors handed to ``model(X)``.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from . import synthetic as syn

_NP_DTYPE = {np.dtype(np.int8): _lib.DTYPE_I8, np.dtype(np.int32): _lib.DTYPE_I32}


def _device_index(device):
    """int | 'cuda' | 'cuda:1' | torch.device -> HIP device ordinal (a CPU device is an error: no fallback)."""
    if device is None:
        return 0
    if isinstance(device, int):
        return device
    s = str(device)
    if s.startswith("cuda") or s.startswith("hip"):
        return int(s.split(":")[1]) if ":" in s else 0
    raise _lib.C3Error(f"clair3_amd models only run on an MI355X HIP device, not on {s!r} (there is no CPU path)")


class _CandidateBatch:
    """what a candidate batch in flight writes into (Clair3_P.submit_candidates): c3_predict_wait fills all three"""

    def __init__(self, n, row_size):
        self.rows = np.empty((n, row_size), dtype=np.float32)
        self.status = np.empty(n, dtype=np.uint8)
        self.n_rows = C.c_int64(-1)


_LABEL_DTYPE = {np.dtype(np.int8): _lib.DTYPE_I8, np.dtype(np.float32): _lib.DTYPE_F32}

# what score() / wait_score() / score_rows() return: ``loss`` the sum over the tasks of the batch means (what the reference's validation pass
# adds up per batch, clair3/Train.py:236-240), ``task_loss`` the batch mean per task, ``accuracy`` per task the share of windows whose arg-max
# of p is the arg-max of y, ``windows``, ``nonfinite`` the windows that held a probability that is not finite; ``window_loss`` (B, tasks)
# float32 and ``rows`` (B, row_size) float32 when asked for, else None; ``loss_sum`` / ``correct`` the record's own totals
ScoreResult = collections.namedtuple("ScoreResult", "loss task_loss accuracy windows nonfinite window_loss rows loss_sum correct")


def _score_result(rec, window_loss=None, rows=None):
    t, n = rec.tasks, max(1, rec.windows)
    loss_sum, correct = np.array(rec.loss_sum[:t], dtype=np.float64), np.array(rec.correct[:t], dtype=np.int64)
    task_loss = loss_sum / n
    total = 0.0
    for v in task_loss:  # in task order
        total += float(v)
    return ScoreResult(total, task_loss, correct / n, int(rec.windows), int(rec.nonfinite), window_loss, rows, loss_sum, correct)


class _HipModel:
    KIND = None
    DEFAULT_CHANNELS = None

    def __init__(self, add_indel_length=False, predict=False, input_channels=None, device=None):
        self.add_indel_length = bool(add_indel_length)
        self.predict = bool(predict)
        self.input_channels = self.DEFAULT_CHANNELS if input_channels is None else int(input_channels)
        self.output_size = 90 if self.add_indel_length else 24
        self._handle = None
        self._device = None
        self._pending_sd = None
        self._keep = False
        self._taps = ""
        self._geometry = None
        self._decode_cols = False
        self._verify = None
        self._verify_layers = False
        self._layer_precision = None
        self._lowering = None   # calibration (set_calibration): the channel lowering a handle created anew takes along ...
        self._cal_meta = None   # ... and (cap_log2, windows) of the calibration it came from, for save_calibration
        self._exact = False     # the exact form (exact()): a handle created anew takes the setting along
        self._answer = "product"      # what answers a batch of the ring (answer()) ...
        self._verify_ref = "fp32"     # ... and what verify mode compares with (verify(reference=)): both need the exact form, both travel with it
        self._refine = None     # refine mode (refine): the gap, or None = off; needs the exact form and travels with it
        self._score = None      # score mode (score_mode): (gamma, class weights or None) a handle created anew takes along
        self._score_census = False  # ... and its census (score_census): on or off travels too, the totals belong to the handle
        self._range_policy = None  # the range-guard policy (range_policy): (policy, max_recalibrations) a handle created anew takes along
        self._recal_seen = 0       # recalibrations of the handle whose lowering self._lowering already mirrors (_sync_recalibration)
        self._calibration_file = None  # C3HIP_CALIBRATION of a model built without a checkpoint (predict.calibration_from_env): applied by the first load
        if device is not None:
            self.to(device)

    # ---- torch.nn.Module look-alikes used by the reference call sites ----
    def to(self, device):
        idx = _device_index(device)
        if self._handle is not None and idx == self._device:
            return self
        return self._create(idx)

    def _create(self, idx):
        """a fresh handle on device ``idx`` with every setting the object carries, loaded from the state dict it holds"""
        if self._handle is not None:
            self._sync_recalibration()  # (what the old handle learned online travels as the lowering)
        sd = self._pending_sd
        self._destroy()
        self._device = idx
        self._recal_seen = 0
        h = _lib.lib().c3_model_create(self.KIND, self.input_channels, int(self.add_indel_length), idx)
        if not h:
            raise _lib.C3Error(f"c3_model_create: {_lib.last_error()}")
        self._handle = C.c_void_p(h)
        if self._geometry is not None:
            _lib.check(_lib.lib().c3_model_set_geometry(self._handle, *self._geometry), "c3_model_set_geometry")
        if self._keep:
            _lib.check(_lib.lib().c3_debug_keep_activations(self._handle, 1), "c3_debug_keep_activations")
        if self._taps:
            _lib.check(_lib.lib().c3_debug_tap(self._handle, self._taps.encode()), "c3_debug_tap")
        if self._decode_cols:
            _lib.check(_lib.lib().c3_model_set_decode_columns(self._handle, 1), "c3_model_set_decode_columns")
        if self._verify is not None:
            _lib.check(_lib.lib().c3_model_set_verify(self._handle, *self._verify), "c3_model_set_verify")
        if self._verify_layers:
            _lib.check(_lib.lib().c3_model_set_verify_layers(self._handle, 1), "c3_model_set_verify_layers")
        if self._layer_precision is not None:
            _lib.check(_lib.lib().c3_model_set_layer_precision(self._handle, self._layer_precision.encode()), "c3_model_set_layer_precision")
        if self._lowering is not None:
            _lib.check(_lib.lib().c3_model_set_channel_lowering(self._handle, self._lowering.ctypes.data), "c3_model_set_channel_lowering")
            if self._cal_meta is not None:
                _lib.check(_lib.lib().c3_model_set_calibration_origin(self._handle, *self._cal_meta), "c3_model_set_calibration_origin")
        if self._exact:
            _lib.check(_lib.lib().c3_model_set_exact(self._handle, 1), "c3_model_set_exact")
        if self._score is not None:
            self._set_score(*self._score)
            if self._score_census:
                _lib.check(_lib.lib().c3_model_set_score_census(self._handle, 1), "c3_model_set_score_census")
        if self._range_policy is not None:  # (before the load: under "recalibrate" it keeps the tensors)
            _lib.check(_lib.lib().c3_model_set_range_policy(self._handle, *self._range_policy), "c3_model_set_range_policy")
        if sd is not None:
            self._load(sd)
        return self

    def cuda(self, device=0):
        return self.to(device)

    def eval(self):  # inference only: dropout is identity, BatchNorm uses running statistics
        return self

    def train(self, mode=True):
        if mode:
            raise _lib.C3Error("clair3_amd implements the inference path only")
        return self

    def set_geometry(self, depth=89, positions=33):
        geometry = (int(depth), int(positions))
        if self._handle is not None and geometry == (self._geometry or (89, 33)):
            return self  # (the geometry the handle has: nothing to free, nothing to load again -- also with a batch in flight)
        if self._handle is not None:  # (refused -- a batch in flight, a fan-in L4 cannot take -- the object keeps the geometry the handle has)
            _lib.check(_lib.lib().c3_model_set_geometry(self._handle, *geometry), "c3_model_set_geometry")
        self._geometry = geometry
        if self._handle is not None:
            if self.KIND == _lib.KIND_FULL_ALIGNMENT:  # (a census counts windows of ONE geometry: the layers' shapes follow it)
                _lib.check(_lib.lib().c3_model_calibrate_reset(self._handle), "c3_model_calibrate_reset")
            if self._pending_sd is not None:
                self._load(self._pending_sd)
        return self

    DECODE_COLS = 31  # C3_DECODE_COLS (include/c3hip.h)

    @property
    def row_size(self):
        """floats per output row: output_size, + DECODE_COLS decoder columns when decode_columns() is on"""
        return self.output_size + (self.DECODE_COLS if self._decode_cols else 0)

    def decode_columns(self, enable=True):
        """Append the decoder columns (clair3_amd/decode.py) to every output row."""
        self._decode_cols = bool(enable)
        if self._handle is not None:
            _lib.check(_lib.lib().c3_model_set_decode_columns(self._handle, int(self._decode_cols)),
                       "c3_model_set_decode_columns")
        return self

    def load_state_dict(self, state_dict, strict=True):
        """Same contract as nn.Module.load_state_dict(strict=True): missing / unexpected / mis-shaped keys raise."""
        if not strict:
            raise _lib.C3Error("only strict loading is supported (as the reference inference loaders do)")
        sd = {}
        for k, v in state_dict.items():
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            v = np.asarray(v)
            if k.endswith("num_batches_tracked"):
                continue
            sd[k] = np.ascontiguousarray(v, dtype=np.float32)
        self._pending_sd = sd
        if self._handle is None:
            self.to(0)
        else:
            if self.KIND == _lib.KIND_FULL_ALIGNMENT:  # (the census was about the checkpoint before; a lowering stays, as the precision plan does)
                _lib.check(_lib.lib().c3_model_calibrate_reset(self._handle), "c3_model_calibrate_reset")
            self._load(sd)
        if self._calibration_file is not None:
            path, self._calibration_file = self._calibration_file, None
            self.load_calibration(path)
        return self

    def _load(self, sd):
        self._sync_recalibration()  # (a load starts the handle's count of recalibrations again; the lowering they left stays with it)
        n = len(sd)
        descs = (_lib.TensorDesc * n)()
        keep = []
        for i, (k, v) in enumerate(sd.items()):
            name = k.encode()
            keep.append(name)
            descs[i].name = name
            descs[i].dtype = _lib.DTYPE_F32
            descs[i].ndim = v.ndim
            for j, s in enumerate(v.shape):
                descs[i].shape[j] = s
            descs[i].data = v.ctypes.data
        rc = _lib.lib().c3_model_load(self._handle, descs, n)
        if rc != 0:
            raise _lib.C3Error(f"Error(s) in loading state_dict for {type(self).__name__}: {_lib.last_error()}")
        self._recal_seen = 0
        # what needs the double weights on the device (answer(), verify(reference="exact")) and was asked for before this load placed them,
        # or of a handle created anew: the library keeps both across reloads, so setting them again changes nothing
        if self._verify_ref != "fp32":
            _lib.check(_lib.lib().c3_model_set_verify_reference(self._handle, _lib.VERIFY_REF[self._verify_ref]), "c3_model_set_verify_reference")
        if self._answer != "product":
            _lib.check(_lib.lib().c3_model_set_answer(self._handle, _lib.ANSWER[self._answer]), "c3_model_set_answer")
        if self._refine is not None:  # (refine mode needs them too)
            _lib.check(_lib.lib().c3_model_set_refine(self._handle, 1, self._refine), "c3_model_set_refine")

    # ---- the forward pass ----
    def __call__(self, x):
        return self.forward(x)

    def forward(self, x, checked=False):
        """x: numpy (host) or torch tensor (host or cuda).  Returns the same container kind holding the
        (B, 24|90) float32 probabilities (``predict=True`` layout of the reference, model.py:152-159).
        Host inputs always carry the fp16-range guard (c3_predict_wait); for a cuda tensor ``checked=True`` selects
        c3_predict_device_checked (synchronises the stream), the default stays asynchronous and unchecked --
        ``range_status()`` tells afterwards whether any batch raised the flag."""
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        if not self.predict:
            raise _lib.C3Error("only predict=True (concatenated heads) is implemented, as the call sites use "
                               "(clair3/CallVariantsFromCffi.py:232,243)")
        is_torch = hasattr(x, "data_ptr") and hasattr(x, "is_cuda")
        if is_torch and x.is_cuda:
            import torch
            if x.device.index not in (None, self._device) and x.device.index != self._device:
                raise _lib.C3Error(f"input on cuda:{x.device.index} but model on device {self._device}")
            x = x.contiguous()
            dt = {torch.int8: _lib.DTYPE_I8, torch.int32: _lib.DTYPE_I32}.get(x.dtype)
            if dt is None:
                raise _lib.C3Error(f"unsupported window dtype {x.dtype}")
            self._check_shape(tuple(x.shape), dt)
            y = torch.empty((x.shape[0], self.row_size), dtype=torch.float32, device=x.device)
            stream = torch.cuda.current_stream(x.device).cuda_stream
            fn = _lib.lib().c3_predict_device_checked if checked else _lib.lib().c3_predict_device
            _lib.check(fn(self._handle, x.data_ptr(), dt, x.shape[0], y.data_ptr(), C.c_void_p(stream)),
                       "c3_predict_device_checked" if checked else "c3_predict_device")
            return y
        xn = x.numpy() if is_torch else np.asarray(x)
        y = self.predict_numpy(xn)
        if is_torch:
            import torch
            return torch.from_numpy(y)
        return y

    def _check_shape(self, shape, dt):
        if self.KIND == _lib.KIND_FULL_ALIGNMENT and len(shape) == 4 and shape[-1] == self.input_channels:
            # the reference network is convolutional + pyramid pooling: the same module takes the 89-row ONT matrix
            # and the 55-row hifi / ilmn one (shared/param_f.py:11), and its call sites construct it without naming
            # the depth (clair3/CallVariantsFromCffi.py:239-243) -- follow the tensor
            geometry = (int(shape[1]), int(shape[2]))
            if geometry != (self._geometry or (89, 33)):
                self.set_geometry(*geometry)
        wbytes = _lib.lib().c3_model_window_bytes(self._handle, dt)
        item = 4 if dt == _lib.DTYPE_I32 else 1
        n = 1
        for s in shape[1:]:
            n *= s
        if n * item != wbytes or shape[-1] != self.input_channels:
            raise _lib.C3Error(f"window shape {shape[1:]} does not match the model "
                               f"({wbytes // item} elements per window, {self.input_channels} channels)")

    @staticmethod
    def _depths(depths, n):
        """one int32 depth per window, as the C ABI takes them"""
        d = np.ascontiguousarray(depths, dtype=np.int32)
        if d.shape != (n,):
            raise _lib.C3Error(f"depths must hold one entry per window: shape {d.shape} for {n} windows")
        return d

    def _window_batch(self, x):
        """(contiguous windows, their C ABI dtype), checked against the model's geometry: the head of every host-side entry"""
        x = np.ascontiguousarray(x)
        dt = _NP_DTYPE.get(x.dtype)
        if dt is None:
            raise _lib.C3Error(f"unsupported window dtype {x.dtype} (int8 / int32 expected)")
        self._check_shape(x.shape, dt)
        return x, dt

    def predict_numpy(self, x, depths=None):
        """depths: per-window read depths (predict.depths_from_alt_info); given, windows deeper than 1.5 x max_depth are rescaled on the
        device the way the reference's in-process loops do before their model call (c3_predict_depth; pileup, int32 windows)."""
        x, dt = self._window_batch(x)
        y = np.empty((x.shape[0], self.row_size), dtype=np.float32)
        if depths is None:
            _lib.check(_lib.lib().c3_predict(self._handle, x.ctypes.data, dt, x.shape[0], y.ctypes.data), "c3_predict")
        else:
            d = self._depths(depths, x.shape[0])
            _lib.check(_lib.lib().c3_predict_depth(self._handle, x.ctypes.data, dt, x.shape[0], d.ctypes.data, y.ctypes.data), "c3_predict_depth")
        return y

    def submit(self, x, slot=0, depths=None):
        """Asynchronous half of predict_numpy (c3_predict_submit / c3_predict_submit_depth); returns a handle for wait()."""
        x, dt = self._window_batch(x)
        y = np.empty((x.shape[0], self.row_size), dtype=np.float32)
        if depths is None:
            _lib.check(_lib.lib().c3_predict_submit(self._handle, x.ctypes.data, dt, x.shape[0], y.ctypes.data, slot),
                       "c3_predict_submit")
        else:
            d = self._depths(depths, x.shape[0])
            _lib.check(_lib.lib().c3_predict_submit_depth(self._handle, x.ctypes.data, dt, x.shape[0], d.ctypes.data, y.ctypes.data, slot),
                       "c3_predict_submit_depth")
        return slot, y

    def submit_dev(self, x, y_dev_ptr, slot=0):
        """submit() with the rows left on the device: the forward pass writes them at device address ``y_dev_ptr``
        (len(x) * row_size floats; c3_predict_submit_dev) -- what a rank of a sharded job does with rows that go to the gather.
        wait() on the ticket returns None (it still runs the range guard)."""
        x, dt = self._window_batch(x)
        _lib.check(_lib.lib().c3_predict_submit_dev(self._handle, x.ctypes.data, dt, x.shape[0], C.c_void_p(int(y_dev_ptr)), slot),
                   "c3_predict_submit_dev")
        return slot, None

    def _parts_args(self, arrays):
        """(windows, pointer table, counts, rows, pointer table, dtype) of a batch of parts as the C ABI takes them.  An entry is an array of
        windows, or a pair (windows, rows) whose rows -- float32 (n, row_size), C-contiguous -- the caller owns: a server hands the mapped
        regions of its clients' segments over that way, and nothing is copied on either side of the library"""
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        arrays = list(arrays)
        n = len(arrays)
        if not 1 <= n <= _lib.MAX_PARTS:
            raise _lib.C3Error(f"a batch takes 1 to {_lib.MAX_PARTS} parts, got {n}")
        xs, ys, dt = [], [], None
        for i, a in enumerate(arrays):
            x, y = a if isinstance(a, tuple) else (a, None)
            x, d = self._window_batch(x)
            if dt is not None and d != dt:
                raise _lib.C3Error(f"part {i}: dtype {x.dtype} differs from the parts before it (one dtype per batch)")
            dt = d
            if y is None:
                y = np.empty((x.shape[0], self.row_size), dtype=np.float32)
            elif y.dtype != np.float32 or y.shape != (x.shape[0], self.row_size) or not y.flags.c_contiguous or not y.flags.writeable:
                raise _lib.C3Error(f"part {i}: rows must be writeable C-contiguous float32 {(x.shape[0], self.row_size)}, got {y.dtype} {y.shape}")
            xs.append(x), ys.append(y)
        xp = (C.c_void_p * n)(*[x.ctypes.data for x in xs])
        yp = (C.c_void_p * n)(*[y.ctypes.data for y in ys])
        counts = (C.c_int64 * n)(*[x.shape[0] for x in xs])
        return xs, xp, counts, ys, yp, dt

    def predict_parts(self, arrays):
        """One forward pass over the windows of several arrays (c3_predict_parts): the list of their rows, each bit-identical to predict_numpy
        on that array alone.  An array of 0 windows is legal."""
        xs, xp, counts, ys, yp, dt = self._parts_args(arrays)
        _lib.check(_lib.lib().c3_predict_parts(self._handle, xp, counts, len(xs), dt, yp), "c3_predict_parts")
        return ys

    def submit_parts(self, arrays, slot=0):
        """Asynchronous half of predict_parts (c3_predict_submit_parts); wait() on the ticket returns the list of rows."""
        xs, xp, counts, ys, yp, dt = self._parts_args(arrays)
        _lib.check(_lib.lib().c3_predict_submit_parts(self._handle, xp, counts, len(xs), dt, yp, slot), "c3_predict_submit_parts")
        return slot, ys

    def wait(self, ticket):
        slot, y = ticket
        _lib.check(_lib.lib().c3_predict_wait(self._handle, slot), "c3_predict_wait")
        if isinstance(y, _CandidateBatch):  # submit_candidates: the rows of the kept candidates and every candidate's status
            return y.rows[:y.n_rows.value], y.status
        return y

    def sharing(self, handles=1):
        """Tell the handle how many handles feed its GPU side by side (c3_model_set_sharing; a speed hint only)."""
        _lib.check(_lib.lib().c3_model_set_sharing(self._handle, int(handles)), "c3_model_set_sharing")
        return self

    def describe(self):
        """which kernel forms the last forward pass took (c3_model_describe)"""
        buf = C.create_string_buffer(1024)
        _lib.check(_lib.lib().c3_model_describe(self._handle, buf, 1024), "c3_model_describe")
        return buf.value.decode()

    # ---- verify mode (c3_model_set_verify) ----
    @staticmethod
    def _verify_args(every, tol, near_tie, escalate, replace=False):
        """(every, tol, near_tie, policy) as the C ABI takes them; anything it would refuse is refused here with the same words"""
        if escalate and replace:
            raise _lib.C3Error("escalate and replace are two policies: choose one")
        if isinstance(every, bool) or not isinstance(every, (int, np.integer)):
            raise _lib.C3Error(f"every must be an integer >= 0 (0 = off), got {every!r}")
        if every < 0 or every > 2 ** 31 - 1:
            raise _lib.C3Error(f"every must be >= 0 (0 = off), got {every}")
        try:
            tol, near_tie = float(tol), float(near_tie)
        except (TypeError, ValueError) as e:
            raise _lib.C3Error(f"tol and near_tie must be numbers, got {tol!r}, {near_tie!r}") from e
        if not np.float32(tol) > 0 or not np.isfinite(tol):
            raise _lib.C3Error(f"tol must be > 0, got {tol}")
        if not near_tie >= 0 or not np.isfinite(near_tie):
            raise _lib.C3Error(f"near_tie must be >= 0, got {near_tie}")
        return int(every), tol, near_tie, _lib.VERIFY_ESCALATE if escalate else _lib.VERIFY_REPLACE if replace else _lib.VERIFY_REPORT

    def verify(self, every=1, tol=1e-4, near_tie=1e-6, escalate=False, layers=False):
        """Verify mode as the base of the model classes states it: the call below with the reference left what it is and no row repaired.
        The model classes (Clair3_P, Clair3_F) take the two further keywords: _RingVerify.verify."""
        return self._verify_with(every, tol, near_tie, escalate, layers, self._verify_ref, False)

    def _verify_with(self, every, tol, near_tie, escalate, layers, reference, replace):
        """Verify mode: every ``every``-th batch of the submit / wait ring (predict_numpy, submit and everything built on them) also runs on the
        fp32-MFMA forms from the same staged input and the two sets of rows are compared on the device (c3_model_set_verify).  ``tol`` and
        ``near_tie`` default to the project's own gates (north_star's 1e-4, tests/util.py NEAR_TIE).  escalate=False: the rows stay the
        fp16x3 ones, bit for bit; escalate=True: a batch that disagrees is answered with its fp32 rows and the handle continues on the
        fp32 forms.  every=0 switches it off.  verify_stats() reads the totals.  layers=True: every compared batch also compares the
        two forms layer by layer on the device (c3_model_set_verify_layers); verify_layers() reads that table.
        reference="exact": a selected batch runs the exact form (exact()) instead of the fp32 forms and is compared with its fp64 rows
        (c3_model_set_verify_reference; with layers=True the product layers are compared with the exact layers); verify_extra() reads the
        double maximum.  replace=True (with either
        reference; not together with escalate): only the rows that disagree are overwritten with the reference's rows, every other row
        stays the product row and the handle stays on the forms it was on (C3_VERIFY_REPLACE)."""
        if not isinstance(replace, (bool, np.bool_)):
            raise _lib.C3Error(f"replace must be True or False, got {replace!r}")
        args = self._verify_args(every, tol, near_tie, escalate, replace)
        if not isinstance(layers, (bool, np.bool_)):
            raise _lib.C3Error(f"layers must be True or False, got {layers!r}")
        if reference not in _lib.VERIFY_REF:
            raise _lib.C3Error(f"reference must be 'fp32' or 'exact', got {reference!r}")
        if self._handle is None:  # (a call that fails leaves nothing behind for a later .to(device) to apply)
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        if args[0] > 0 and self._refine is not None:
            raise _lib.C3Error("verify() is refused while refine mode is on (refine()): the two own the same rows")
        if reference != self._verify_ref:  # (in front of everything else: refused, it leaves the setting what it was)
            if self._pending_sd is not None or reference == "fp32":  # (no weights yet: the first load sets it, behind the double weights)
                _lib.check(_lib.lib().c3_model_set_verify_reference(self._handle, _lib.VERIFY_REF[reference]), "c3_model_set_verify_reference")
            elif not self._exact:
                raise _lib.C3Error("reference='exact' needs the exact form: call exact() first")
            self._verify_ref = reference
        _lib.check(_lib.lib().c3_model_set_verify(self._handle, *args), "c3_model_set_verify")
        _lib.check(_lib.lib().c3_model_set_verify_layers(self._handle, int(layers)), "c3_model_set_verify_layers")
        self._verify = args  # a handle created anew by .to(another device) takes the setting along
        self._verify_layers = bool(layers)
        return self

    def verify_extra(self):
        """what verify_stats() has no room for (c3_model_verify_extra), since the last load / verify_reset(): ``reference`` ("fp32" | "exact"),
        ``rows_replaced`` and ``batches_with_replacements`` of verify(replace=True), ``max_abs_diff_f64`` of verify(reference="exact")"""
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        ex = _lib.VerifyExtra()
        _lib.check(_lib.lib().c3_model_verify_extra(self._handle, C.byref(ex)), "c3_model_verify_extra")
        return dict(reference="exact" if ex.reference == _lib.VERIFY_REF["exact"] else "fp32", rows_replaced=int(ex.rows_replaced),
                    batches_with_replacements=int(ex.batches_with_replacements), max_abs_diff_f64=float(ex.max_abs_diff_f64))

    def verify_stats(self):
        """the totals of verify mode since the last load / verify_reset() as a dict (c3_model_verify_stats; include/c3hip.h names the fields)"""
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        st = _lib.VerifyStats()
        _lib.check(_lib.lib().c3_model_verify_stats(self._handle, C.byref(st)), "c3_model_verify_stats")
        out = {}
        for name, _ in _lib.VerifyStats._fields_:
            v = getattr(st, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        out["policy"] = _lib.VERIFY_POLICY.get(st.policy, "report")
        return out

    def verify_layers(self):
        """the layer records of verify(layers=True) since the last load / verify_reset(): one dict per layer in network order
        (c3_model_verify_layers; include/c3hip.h names the fields), each with ``rel`` = max_abs_diff / max(1, ref_max_abs) -- the measure of
        the suite's layer gate.  Empty when layers was never switched on."""
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        buf = (_lib.VerifyLayer * 16)()
        n = _lib.lib().c3_model_verify_layers(self._handle, buf, 16)
        if n < 0:
            raise _lib.C3Error(f"c3_model_verify_layers: {_lib.last_error()}")
        out = []
        for e in buf[:n]:
            d = {name: getattr(e, name) for name, _ in _lib.VerifyLayer._fields_ if not name.startswith("reserved")}
            d["name"], d["status"] = e.name.decode(), _lib.VERIFY_LAYER_STATUS.get(e.status, "?")
            d["rel"] = float(np.float32(e.max_abs_diff) / max(np.float32(1), np.float32(e.ref_max_abs)))
            out.append(d)
        return out

    def verify_reset(self):
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        _lib.check(_lib.lib().c3_model_verify_reset(self._handle), "c3_model_verify_reset")
        return self

    # ---- per-layer precision (c3_model_set_layer_precision) ----
    @staticmethod
    def _layer_names(names):
        """the plan as the C ABI takes it: a string as it is, an iterable of names joined by commas"""
        if isinstance(names, bytes):
            names = names.decode()
        if isinstance(names, str):
            return names
        try:
            names = list(names)
        except TypeError as e:
            raise _lib.C3Error(f"layer names must be a string or an iterable of strings, got {names!r}") from e
        for n in names:
            if not isinstance(n, str) or not n or "," in n:
                raise _lib.C3Error(f"layer names must be non-empty strings without commas, got {n!r}")
        return ",".join(names)

    def layer_precision(self, names=None):
        """The per-layer precision plan: the layers ``names`` (a string "lstm2,l4" or an iterable of names; "" = none, "all" = every layer)
        run their fp32-MFMA forms, every other layer its fp16x3 form (c3_model_set_layer_precision; include/c3hip.h lists the names of
        both networks).  Without an argument: the plan in force as a tuple of names in network order."""
        if names is None:
            if self._handle is None:
                raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
            buf = C.create_string_buffer(256)
            _lib.check(_lib.lib().c3_model_layer_precision(self._handle, buf, 256), "c3_model_layer_precision")
            return tuple(n for n in buf.value.decode().split(",") if n)
        text = self._layer_names(names)
        _lib.check(_lib.lib().c3_layer_precision_check(self.KIND, text.encode()), "c3_layer_precision_check")
        if self._handle is None:  # (a call that fails leaves nothing behind for a later .to(device) to apply)
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        _lib.check(_lib.lib().c3_model_set_layer_precision(self._handle, text.encode()), "c3_model_set_layer_precision")
        self._layer_precision = text  # a handle created anew by .to(another device) takes the plan along
        return self

    # ---- calibration of the channel exponents from observed activations (c3_model_calibrate; full alignment; DESIGN.md 1 Range) ----
    def _need_handle(self):
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")

    def calibrate(self, x, cap_log2=10, apply=True):
        """Measure the activations of the windows ``x`` on the fp32 forms (added to the handle's census), work out by how many powers of two
        every channel's exponent has to come down for them to stay below 2^cap_log2 (c3_model_calibration_solve; include/c3hip.h states the
        rule) and, with apply=True, set that lowering and load the held state dict again with it.  Exact rescaling: the rows stay the
        checkpoint's.  Returns a summary (clair3_amd/calibrate.py summary): per group the channels lowered, the group shift and the largest scaled activation
        before and after.  INTEGRATION.md 8 says when and on what sample."""
        from . import calibrate as cal
        self._need_handle()
        if isinstance(cap_log2, bool) or not isinstance(cap_log2, (int, np.integer)) or not 4 <= cap_log2 <= 13:
            raise _lib.C3Error(f"cap_log2 must be an integer in [4, 13], got {cap_log2!r}")
        x, dt = self._window_batch(x)
        _lib.check(_lib.lib().c3_model_calibrate(self._handle, x.ctypes.data, dt, x.shape[0], None), "c3_model_calibrate")
        lowering = np.zeros(cal.CHANNELS, dtype=np.uint8)
        _lib.check(_lib.lib().c3_model_calibration_solve(self._handle, int(cap_log2), lowering.ctypes.data), "c3_model_calibration_solve")
        state = self.calibration()
        if apply:
            self.set_calibration(lowering, reload=True, cap_log2=int(cap_log2), windows=state["windows"])
        out = cal.summary(state["census"], state["k0"], lowering)
        out.update(cap_log2=int(cap_log2), windows=state["windows"], applied=bool(apply), lowering=lowering)
        return out

    def calibration(self):
        """the handle's calibration state as a dict: ``census`` (9, 256) max |x| per convolution and channel in the checkpoint's units and
        the ``windows`` it counts (c3_model_calibration_census), ``k0`` / ``k`` (896) the channel exponents of the last load as the load-time
        rule gave them / as the handle runs them (c3_model_channel_exps), ``lowering`` (896, or None while none is set)"""
        self._need_handle()
        self._sync_recalibration()
        census, windows = np.zeros((9, 256), dtype=np.float32), C.c_int64(0)
        _lib.check(_lib.lib().c3_model_calibration_census(self._handle, census.ctypes.data, C.byref(windows)), "c3_model_calibration_census")
        k0, k = np.zeros(896, dtype=np.int8), np.zeros(896, dtype=np.int8)
        _lib.check(_lib.lib().c3_model_channel_exps(self._handle, k0.ctypes.data, k.ctypes.data), "c3_model_channel_exps")
        return dict(census=census, windows=int(windows.value), k0=k0, k=k, lowering=None if self._lowering is None else self._lowering.copy())

    def set_calibration(self, lowering, reload=False, cap_log2=0, windows=0):
        """Set the channel lowering (896 entries, stage0 | inner0 | stage1 | inner1 | stage2 | inner2; None = none).  It takes effect at the
        next load -- load_state_dict, or here with reload=True from the state dict the object holds -- and stays with the model from then on
        (c3_model_set_channel_lowering).  ``cap_log2`` and ``windows`` say where it came from (c3_model_set_calibration_origin: what describe()
        and save_calibration report with it; 0 = not known)."""
        from . import calibrate as cal
        self._need_handle()
        self._sync_recalibration()  # (what the handle learned online is on record before this call replaces it)
        if lowering is not None:
            lowering = cal.as_lowering(lowering)
        _lib.check(_lib.lib().c3_model_set_channel_lowering(self._handle, None if lowering is None else lowering.ctypes.data),
                   "c3_model_set_channel_lowering")
        if lowering is not None:
            _lib.check(_lib.lib().c3_model_set_calibration_origin(self._handle, int(cap_log2), int(windows)), "c3_model_set_calibration_origin")
        self._lowering, self._cal_meta = lowering, None if lowering is None else (int(cap_log2), int(windows))
        if reload and self._pending_sd is not None:
            self._load(self._pending_sd)
        return self

    # ---- the range-guard policy: recalibrate on a trip and stay on the fp16x3 kernels (c3_model_set_range_policy; DESIGN.md 1 Range) ----
    _RANGE_POLICIES = {"sticky": _lib.RANGE_STICKY, "recalibrate": _lib.RANGE_RECALIBRATE}

    def range_policy(self, policy=None, max_recalibrations=4):
        """What the range guard does when a batch comes back beyond the fp16 range.  "sticky" (the default): the batch runs again on the
        fp32 forms and the handle stays there.  "recalibrate": that re-run also takes the census of calibrate(), the channel exponents come
        down by the rule, the weights are packed again and the handle stays on the fp16x3 kernels -- at most ``max_recalibrations`` times
        between two loads, after which (or when the census is not finite, or asks for nothing) it behaves as sticky.  Full alignment only.
        The library keeps the float32 tensors of its loads while the policy is "recalibrate", so a handle that already has weights is
        created anew and loaded from the state dict the object holds.  Without an argument: (policy, max_recalibrations) in force."""
        self._need_handle()
        if policy is None:
            st = self.range_stats()
            return st["policy"], st["max_recalibrations"]
        if policy not in self._RANGE_POLICIES:
            raise _lib.C3Error(f"policy must be 'sticky' or 'recalibrate', got {policy!r}")
        if isinstance(max_recalibrations, bool) or not isinstance(max_recalibrations, (int, np.integer)) or not 0 <= max_recalibrations < 2 ** 31:
            raise _lib.C3Error(f"max_recalibrations must be an integer >= 0, got {max_recalibrations!r}")
        args = (self._RANGE_POLICIES[policy], int(max_recalibrations))
        # a loaded handle that kept no tensors cannot start to recalibrate (the library says so): it is created anew and loads from the held state dict
        anew = (args[0] == _lib.RANGE_RECALIBRATE and self._pending_sd is not None and self.range_stats()["policy"] != "recalibrate")
        if anew and self.KIND != _lib.KIND_FULL_ALIGNMENT:
            anew = False  # (refused below with the library's words)
        if anew:
            old, self._range_policy = self._range_policy, args
            try:
                self._create(self._device)
            except _lib.C3Error:
                self._range_policy = old
                raise
            return self
        _lib.check(_lib.lib().c3_model_set_range_policy(self._handle, *args), "c3_model_set_range_policy")
        self._range_policy = args
        return self

    def range_stats(self):
        """the totals of the range-guard policy since the last load as a dict (c3_model_range_stats; include/c3hip.h names the fields);
        ``fell_back``: the reason as text, "" while the handle has not fallen back to the sticky behaviour"""
        self._need_handle()
        st = _lib.RangeStats()
        _lib.check(_lib.lib().c3_model_range_stats(self._handle, C.byref(st)), "c3_model_range_stats")
        out = {name: getattr(st, name) for name, _ in _lib.RangeStats._fields_ if name not in ("reason", "fell_back", "policy")}
        out["policy"] = "recalibrate" if st.policy == _lib.RANGE_RECALIBRATE else "sticky"
        out["fell_back"] = st.reason.decode() if st.fell_back else ""
        return out

    def _sync_recalibration(self):
        """after an online recalibration the lowering in force is the handle's, not the one this object set: mirror it (k0 - k of the last
        packing) with its origin, so that calibration(), save_calibration() and a handle created anew carry what was learned"""
        if self._handle is None or self.KIND != _lib.KIND_FULL_ALIGNMENT:
            return
        st = _lib.RangeStats()
        if _lib.lib().c3_model_range_stats(self._handle, C.byref(st)) != 0 or st.recalibrations == self._recal_seen:
            return
        k0, k = np.zeros(896, dtype=np.int8), np.zeros(896, dtype=np.int8)
        _lib.check(_lib.lib().c3_model_channel_exps(self._handle, k0.ctypes.data, k.ctypes.data), "c3_model_channel_exps")
        self._lowering = (k0.astype(np.int16) - k.astype(np.int16)).astype(np.uint8)
        self._cal_meta = (int(st.cap_log2), int(st.census_windows))
        self._recal_seen = int(st.recalibrations)

    def calibration_reset(self):
        """zero the census and its window count (c3_model_calibrate_reset); a lowering that is set stays"""
        self._need_handle()
        _lib.check(_lib.lib().c3_model_calibrate_reset(self._handle), "c3_model_calibrate_reset")
        return self

    def save_calibration(self, path):
        """the lowering in force as a calibration file (clair3_amd/calibrate.py names the format): what C3HIP_CALIBRATION=<file> hands to
        every worker process of a job"""
        from . import calibrate as cal
        self._sync_recalibration()
        if self._lowering is None:
            raise _lib.C3Error("no calibration is set: calibrate() first")
        cap, windows = self._cal_meta or (0, 0)
        depth = (self._geometry or (89, 33))[0]
        cal.write_file(path, channels=self.input_channels, depth=depth, cap_log2=cap, windows=windows, k0=self.calibration()["k0"],
                       lowering=self._lowering)
        return self

    def load_calibration(self, path):
        """Apply a calibration file: checked against this model (input channels, depth, and ``k0`` -- the channel exponents of the checkpoint
        it was made for -- against the loaded checkpoint's), set, and the held state dict loaded again with it.  Anything that does not fit raises."""
        from . import calibrate as cal
        self._need_handle()
        k0 = self.calibration()["k0"]  # (a pileup handle, or one without weights, is refused here with the library's words)
        f = cal.read_file(path)
        depth = (self._geometry or (89, 33))[0]
        if f["channels"] != self.input_channels or f["depth"] != depth:
            raise _lib.C3Error(f"{path}: made for windows of {f['channels']} channels and depth {f['depth']}, this model has {self.input_channels} and {depth}")
        if not np.array_equal(f["k0"], k0):
            raise _lib.C3Error(f"{path}: made for another checkpoint (its channel exponents k0 differ from the loaded checkpoint's)")
        self.set_calibration(f["lowering"], reload=True, cap_log2=f["cap_log2"], windows=f["windows"])
        return self

    # ---- score mode: focal loss and accuracy of labelled windows on the device (c3_model_set_score) ----
    def _set_score(self, gamma, weights):
        _lib.check(_lib.lib().c3_model_set_score(self._handle, 1, gamma, None if weights is None else weights.ctypes.data), "c3_model_set_score")

    def score_mode(self, gamma=2.0, class_weights=None, enable=True):
        """Enable score mode with the reference's ``gamma`` and class weights (output_size floats in the row's column layout, e.g.
        evaluate.class_weights; None = none).  score(), submit_score() and score_rows() set it themselves when their arguments differ from
        what is in force; enable=False switches it off."""
        self._need_handle()
        if not enable:
            _lib.check(_lib.lib().c3_model_set_score(self._handle, 0, 0.0, None), "c3_model_set_score")
            self._score, self._score_census = None, False  # (the census needs score mode)
            return self
        try:
            gamma = float(gamma)
        except (TypeError, ValueError) as e:
            raise _lib.C3Error(f"gamma must be a number >= 0, got {gamma!r}") from e
        w = None
        if class_weights is not None:
            w = np.ascontiguousarray(class_weights, dtype=np.float32)
            if w.shape != (self.output_size,):
                raise _lib.C3Error(f"class_weights must hold {self.output_size} entries, got shape {w.shape}")
        self._set_score(gamma, w)
        self._score = (gamma, w)
        return self

    def _score_setting(self, gamma, class_weights):
        cur = self._score
        same = cur is not None and cur[0] == float(gamma) and ((cur[1] is None) == (class_weights is None)) and \
            (class_weights is None or np.array_equal(cur[1], np.asarray(class_weights, dtype=np.float32)))
        if not same:
            self.score_mode(gamma, class_weights)

    def _labels(self, labels, n):
        labels = np.ascontiguousarray(labels)
        dt = _LABEL_DTYPE.get(labels.dtype)
        if dt is None:
            raise _lib.C3Error(f"unsupported label dtype {labels.dtype} (int8 / float32 expected)")
        if labels.shape != (n, self.output_size):
            raise _lib.C3Error(f"labels must be {(n, self.output_size)} in the row's column layout, got {labels.shape}")
        return labels, dt

    def submit_score(self, x, labels, slot=0, class_weights=None, gamma=2.0, window_loss=False, rows=False):
        """Asynchronous half of score() (c3_score_submit); returns a ticket for wait_score()."""
        self._need_handle()
        self._score_setting(gamma, class_weights)
        x, dt = self._window_batch(x)
        labels, ldt = self._labels(labels, x.shape[0])
        y = np.empty((x.shape[0], self.row_size), dtype=np.float32) if rows else None
        wl = np.empty((x.shape[0], 4 if self.add_indel_length else 2), dtype=np.float32) if window_loss else None
        _lib.check(_lib.lib().c3_score_submit(self._handle, x.ctypes.data, dt, x.shape[0], labels.ctypes.data, ldt,
                                              None if y is None else y.ctypes.data, None if wl is None else wl.ctypes.data, slot), "c3_score_submit")
        return slot, y, wl

    def wait_score(self, ticket):
        slot, y, wl = ticket
        rec = _lib.ScoreResult()
        _lib.check(_lib.lib().c3_score_wait(self._handle, slot, C.byref(rec)), "c3_score_wait")
        return _score_result(rec, wl, y)

    def score(self, x, labels, class_weights=None, gamma=2.0, window_loss=False, rows=False):
        """The reference's validation loss of the labelled windows ``x`` (clair3/Train.py:87-107, :210-257): forward pass, focal loss per task,
        arg-max accuracy, all on the device (c3_score; blocking).  labels: (B, output_size) int8 or float32 in the row's column layout.
        Without rows=True the probabilities never leave the device.  Returns a ScoreResult."""
        self._need_handle()
        self._score_setting(gamma, class_weights)
        x, dt = self._window_batch(x)
        labels, ldt = self._labels(labels, x.shape[0])
        y = np.empty((x.shape[0], self.row_size), dtype=np.float32) if rows else None
        wl = np.empty((x.shape[0], 4 if self.add_indel_length else 2), dtype=np.float32) if window_loss else None
        rec = _lib.ScoreResult()
        _lib.check(_lib.lib().c3_score(self._handle, x.ctypes.data, dt, x.shape[0], labels.ctypes.data, ldt, None if y is None else y.ctypes.data,
                                       None if wl is None else wl.ctypes.data, C.byref(rec)), "c3_score")
        return _score_result(rec, wl, y)

    def score_rows(self, rows, labels, class_weights=None, gamma=2.0, window_loss=True):
        """score() of given float32 probability rows (B, >= output_size) without a forward pass (c3_score_rows): the reference's rows, the
        exact form's rounded to float32, adversarial ones."""
        self._need_handle()
        self._score_setting(gamma, class_weights)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] < self.output_size:
            raise _lib.C3Error(f"rows must be (B, >= {self.output_size}) float32, got {rows.shape}")
        labels, ldt = self._labels(labels, rows.shape[0])
        wl = np.empty((rows.shape[0], 4 if self.add_indel_length else 2), dtype=np.float32) if window_loss else None
        rec = _lib.ScoreResult()
        _lib.check(_lib.lib().c3_score_rows(self._handle, rows.ctypes.data, rows.shape[1], rows.shape[0], labels.ctypes.data, ldt, C.byref(rec),
                                            None if wl is None else wl.ctypes.data), "c3_score_rows")
        return _score_result(rec, wl, None)

    # ---- ... and its census: confusion, reliability and near-tie tables of the scored windows (c3_model_set_score_census) ----
    def score_census(self, enable=True):
        """Switch the census of score mode on or off: while on, every scored batch (score, submit_score / wait_score, score_rows) adds its
        windows to the handle's tables, counted on the device from the rows the batch is answered with.  Enables score mode with its defaults
        when it is off; refused while a submit is pending."""
        if not isinstance(enable, (bool, np.bool_)):
            raise _lib.C3Error(f"enable must be True or False, got {enable!r}")
        self._need_handle()
        if enable and self._score is None:
            self.score_mode()
        _lib.check(_lib.lib().c3_model_set_score_census(self._handle, int(enable)), "c3_model_set_score_census")
        self._score_census = bool(enable)
        return self

    def census(self):
        """The census since the last census_reset() (c3_score_census_read) as a synthetic.Census: ``confusion`` four (K, K) int64 arrays
        [truth][pred], ``rel_windows`` / ``rel_correct`` / ``rel_conf_q32`` (4, 20), ``rel_skipped`` (4,), ``gap_below`` (4, 6), ``windows``,
        ``tasks``.  evaluate.census_report turns it into accuracy, precision / recall / F1 and the calibration error."""
        self._need_handle()
        rec = _lib.ScoreCensus()
        _lib.check(_lib.lib().c3_score_census_read(self._handle, C.byref(rec)), "c3_score_census_read")
        flat = np.ctypeslib.as_array(rec.confusion).astype(np.int64)
        conf = [flat[o:o + k * k].reshape(k, k).copy() for o, k in zip(syn.CENSUS_CELL_OFF, syn.HEAD_SIZES)]
        arr = lambda a: np.ctypeslib.as_array(a).astype(np.int64)  # noqa: E731
        return syn.Census(int(rec.windows), int(rec.tasks), conf, arr(rec.rel_windows), arr(rec.rel_correct), arr(rec.rel_conf_q32),
                          arr(rec.rel_skipped), arr(rec.gap_below))

    def census_reset(self):
        self._need_handle()
        _lib.check(_lib.lib().c3_score_census_reset(self._handle), "c3_score_census_reset")
        return self

    # ---- the exact form: the network in fp64 from end to end on the device (c3_predict_exact) ----
    def exact(self, enable=True):
        """Enable the exact form: the double weights are placed on the device by a load, so the state dict the object holds is loaded again
        (c3_model_set_exact takes effect at the next c3_model_load); without one the next load_state_dict does it.  predict_exact() and
        exact_fetch() need it; nothing else changes: rows, precision, describe() apart from its last field `` exact=1``."""
        if not isinstance(enable, (bool, np.bool_)):
            raise _lib.C3Error(f"enable must be True or False, got {enable!r}")
        self._need_handle()
        _lib.check(_lib.lib().c3_model_set_exact(self._handle, int(enable)), "c3_model_set_exact")
        self._exact = bool(enable)
        if self._pending_sd is not None:
            self._load(self._pending_sd)
        return self

    def answer(self, form="exact"):
        """What answers the batches of the submit / wait ring (c3_model_set_answer): "exact" -- predict_numpy, submit / wait and everything
        built on them (depths, regions, candidates, rows, parts, submit_dev, score mode) return the float32 rounding of the exact rows,
        decoder columns computed from them; no product kernel runs, describe() says precision=exact, verify mode skips such batches --
        or "product", the default.  Needs exact(); forward() and forward(checked=True) stay the product forms."""
        if form not in _lib.ANSWER:
            raise _lib.C3Error(f"form must be 'exact' or 'product', got {form!r}")
        self._need_handle()
        if self._pending_sd is not None or form == "product":
            _lib.check(_lib.lib().c3_model_set_answer(self._handle, _lib.ANSWER[form]), "c3_model_set_answer")
        elif not self._exact:  # (no weights yet: the first load sets it, behind the double weights -- which exact() must have asked for)
            raise _lib.C3Error("answer('exact') needs the exact form: call exact() first")
        self._answer = form
        return self

    # ---- refine mode: the windows near a tie are answered by the exact form (c3_model_set_refine) ----
    def refine(self, gap=1e-4, enable=True):
        """Refine mode: every batch of sliced windows (predict_numpy and its chunks, submit / wait, submit_parts, submit_dev) is answered by
        the product forms as without it; the windows whose row lies within ``gap`` of a tie -- in a head, or with decoder columns on among
        the decoder's class maxima (synthetic.refine_gaps states the rule) -- then run through the exact form, and their rows and decoder
        columns become the float32 rounding of the exact ones.  Every other row stays the product row, bit for bit.  ``gap`` defaults to
        verify mode's tol, far above the forms' row error: every label is then the exact form's.  Needs exact(); refused while verify mode
        is on (the two own the same rows) or a submit is pending.  refine_stats() reads the totals; enable=False switches it off."""
        if not isinstance(enable, (bool, np.bool_)):
            raise _lib.C3Error(f"enable must be True or False, got {enable!r}")
        self._need_handle()
        if not enable:
            _lib.check(_lib.lib().c3_model_set_refine(self._handle, 0, 0.0), "c3_model_set_refine")
            self._refine = None
            return self
        try:
            gap = float(gap)
        except (TypeError, ValueError) as e:
            raise _lib.C3Error(f"gap must be a number >= 0, got {gap!r}") from e
        if not gap >= 0 or not np.isfinite(np.float32(gap)):
            raise _lib.C3Error(f"gap must be a finite number >= 0, got {gap}")
        if self._pending_sd is not None:
            _lib.check(_lib.lib().c3_model_set_refine(self._handle, 1, gap), "c3_model_set_refine")
        elif not self._exact:  # (no weights yet: the first load sets it, behind the double weights -- which exact() must have asked for)
            raise _lib.C3Error("refine() needs the exact form: call exact() first")
        elif self._verify is not None and self._verify[0] > 0:
            raise _lib.C3Error("refine() is refused while verify mode is on: the two own the same rows")
        self._refine = gap
        return self

    def refine_stats(self):
        """the totals of refine mode since the last load / refine_reset() as a dict (c3_model_refine_stats; include/c3hip.h names the fields)"""
        self._need_handle()
        st = _lib.RefineStats()
        _lib.check(_lib.lib().c3_model_refine_stats(self._handle, C.byref(st)), "c3_model_refine_stats")
        out = {}
        for name, _ in _lib.RefineStats._fields_:
            v = getattr(st, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out

    def refine_reset(self):
        self._need_handle()
        _lib.check(_lib.lib().c3_model_refine_reset(self._handle), "c3_model_refine_reset")
        return self

    def refine_select(self, rows, gap):
        """refine mode's selection alone on given rows (c3_refine_select), float32 (B, output_size) or (B, output_size + DECODE_COLS) with the
        decoder columns filled in: (index int32 ascending, min_gap float32 (B,)) -- what synthetic.refine_select gives."""
        self._need_handle()
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2:
            raise _lib.C3Error(f"rows must be (B, row_floats) float32, got {rows.shape}")
        n = rows.shape[0]
        index, gaps, count = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32), C.c_int64(0)
        _lib.check(_lib.lib().c3_refine_select(self._handle, rows.ctypes.data, rows.shape[1], n, float(gap), index.ctypes.data, C.byref(count),
                                               gaps.ctypes.data), "c3_refine_select")
        return index[:count.value].copy(), gaps

    # ---- jackknife mode: the reduction alone (c3_jackknife_reduce; Clair3_F.jackknife / jackknife_rows run the network) ----
    @staticmethod
    def _jackknife_layout(layout):
        if layout not in _lib.JACKKNIFE_LAYOUT:
            raise _lib.C3Error(f"layout must be 'recentre' or 'in_place', got {layout!r}")
        return _lib.JACKKNIFE_LAYOUT[layout]

    def jackknife_reduce(self, base_rows, variant_rows, counts, drops=False):
        """The records of jackknife mode for rows the caller holds (c3_jackknife_reduce): ``base_rows`` (B, row) float32, ``variant_rows``
        (sum(counts), row) the rows of every window's leave-one-read-out variants in window order, read order; row = output_size, or that
        + DECODE_COLS with the decoder columns filled in.  Returns a dict: ``rows`` (B,) of synthetic.JACKKNIFE_DTYPE, ``counts``, and with
        drops=True ``drops`` (sum(counts), 4) float32 -- what synthetic.jackknife_records gives.  Needs no weights."""
        self._need_handle()
        base = np.ascontiguousarray(base_rows, dtype=np.float32)
        var = np.ascontiguousarray(variant_rows, dtype=np.float32)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if base.ndim != 2 or var.ndim != 2 or var.shape[1] != base.shape[1]:
            raise _lib.C3Error(f"base rows (B, row) and variant rows (n, row) float32 expected, got {base.shape} and {var.shape}")
        if counts.shape != (len(base),):
            raise _lib.C3Error(f"counts must hold one entry per window: shape {counts.shape} for {len(base)} windows")
        if (counts >= 0).all() and int(counts.sum(dtype=np.int64)) != len(var):
            raise _lib.C3Error(f"counts add up to {int(counts.sum(dtype=np.int64))} variants, {len(var)} rows given")
        rec = np.zeros(len(base), dtype=syn.JACKKNIFE_DTYPE)
        d = np.zeros((len(var), 4), dtype=np.float32) if drops else None
        _lib.check(_lib.lib().c3_jackknife_reduce(self._handle, base.ctypes.data, var.ctypes.data, base.shape[1], counts.ctypes.data, len(base),
                                                  rec.ctypes.data, None if d is None else d.ctypes.data), "c3_jackknife_reduce")
        out = dict(rows=rec, counts=counts)
        if drops:
            out["drops"] = d
        return out

    # ---- subsample mode: the reduction alone (c3_subsample_reduce; Clair3_F.subsample / subsample_rows run the network) ----
    @staticmethod
    def _subsample_plan(depths, replicates, seed=0):
        """(depths int32 [L], replicates, seed) as the C ABI takes them, refused here as the library refuses them"""
        try:
            d = np.ascontiguousarray([int(v) for v in depths], dtype=np.int32)
        except (TypeError, ValueError, OverflowError):
            raise _lib.C3Error(f"depths must be a sequence of integers, got {depths!r}") from None
        if not 1 <= len(d) <= syn.SUBSAMPLE_MAX_LEVELS:
            raise _lib.C3Error(f"levels: 1 .. {syn.SUBSAMPLE_MAX_LEVELS} target depths expected, got {len(d)}")
        if d[0] < 1 or (np.diff(d.astype(np.int64)) <= 0).any():
            raise _lib.C3Error(f"depths must be >= 1 and strictly increasing, got {d.tolist()}")
        if isinstance(replicates, bool) or not isinstance(replicates, (int, np.integer)) or not 1 <= replicates <= syn.SUBSAMPLE_MAX_REPLICATES:
            raise _lib.C3Error(f"replicates must be an integer in 1 .. {syn.SUBSAMPLE_MAX_REPLICATES}, got {replicates!r}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 64:
            raise _lib.C3Error(f"seed must be an integer in [0, 2^64), got {seed!r}")
        return d, int(replicates), int(seed)

    def subsample_reduce(self, base_rows, variant_rows, counts, depths=(10, 20, 30, 40), replicates=8):
        """The records of subsample mode for rows the caller holds (c3_subsample_reduce): ``base_rows`` (B, row) float32, ``variant_rows``
        (variants, row) the rows of every window's variants in the rule's order -- window by window, level by level (only levels with
        D_l < counts[w]), replicate by replicate; row = output_size, or that + DECODE_COLS with the decoder columns filled in.  Returns a
        dict: ``levels`` (B, L) of synthetic.SUBSAMPLE_LEVEL_DTYPE, ``rows`` (B,) of synthetic.SUBSAMPLE_WINDOW_DTYPE, ``counts`` -- what
        synthetic.subsample_records gives.  Needs no weights."""
        d, replicates, _ = self._subsample_plan(depths, replicates)
        self._need_handle()
        base = np.ascontiguousarray(base_rows, dtype=np.float32)
        var = np.ascontiguousarray(variant_rows, dtype=np.float32)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if base.ndim != 2 or var.ndim != 2 or var.shape[1] != base.shape[1]:
            raise _lib.C3Error(f"base rows (B, row) and variant rows (n, row) float32 expected, got {base.shape} and {var.shape}")
        if counts.shape != (len(base),):
            raise _lib.C3Error(f"counts must hold one entry per window: shape {counts.shape} for {len(base)} windows")
        if (counts >= 0).all() and int(syn.subsample_variant_counts(counts, d, replicates).sum()) != len(var):
            raise _lib.C3Error(f"the plan has {int(syn.subsample_variant_counts(counts, d, replicates).sum())} variants, {len(var)} rows given")
        lev = np.zeros((len(base), len(d)), dtype=syn.SUBSAMPLE_LEVEL_DTYPE)
        rec = np.zeros(len(base), dtype=syn.SUBSAMPLE_WINDOW_DTYPE)
        _lib.check(_lib.lib().c3_subsample_reduce(self._handle, base.ctypes.data, var.ctypes.data, base.shape[1], counts.ctypes.data, len(base),
                                                  d.ctypes.data, len(d), replicates, rec.ctypes.data, lev.ctypes.data), "c3_subsample_reduce")
        return dict(levels=lev, rows=rec, counts=counts)

    # ---- occlusion mode: which channels and columns a call leans on (c3_occlude, c3_occlude_rows, c3_occlude_reduce) ----
    def _occlude_plan(self, what, band):
        """(the code of ``what``, band, channels of group 0, bands of group 1) for the handle's geometry"""
        if what not in _lib.OCCLUDE_WHAT:
            raise _lib.C3Error(f"what must be 'channels', 'bands' or 'both', got {what!r}")
        positions = (self._geometry or (89, 33))[1]
        if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or not 1 <= band <= positions:
            raise _lib.C3Error(f"band must be an integer in 1 .. {positions}, got {band!r}")
        nc, nb = syn.occlude_groups(positions, self.input_channels, what, int(band))
        return _lib.OCCLUDE_WHAT[what], int(band), nc, nb

    def _occlude_call(self, entry, head, batch, plan, drops, variant_rows, extra):
        code, band, nc, nb = plan
        K = nc + nb
        y = np.empty((batch, self.row_size), dtype=np.float32)
        rec = np.zeros(batch, dtype=syn.OCCLUDE_DTYPE)
        d = np.zeros((batch, K, 4), dtype=np.float32) if drops else None
        v = np.zeros((batch * K, self.row_size), dtype=np.float32) if variant_rows else None
        info = _lib.OccludeInfo()
        _lib.check(getattr(_lib.lib(), entry)(self._handle, *head, batch, code, band, y.ctypes.data, rec.ctypes.data,
                                              None if d is None else d.ctypes.data, None if v is None else v.ctypes.data, C.byref(info)), entry)
        out = dict(rows=rec, base_rows=y, channels=nc, bands=nb, band=band, on_fp32=bool(info.on_fp32), passes=int(info.passes),
                   bytes_staged=int(info.bytes_staged), expand_us=float(info.expand_us), reduce_us=float(info.reduce_us), **extra)
        if drops:
            out["drops"] = d
        if variant_rows:
            out["variant_rows"] = v
        return out

    def occlude(self, x, what="both", band=1, drops=False, variant_rows=False):
        """Which input channels and which columns the calls of the dense windows ``x`` lean on (c3_occlude; either network): for every window
        the device builds K variants -- the window with one channel set to zero (what "channels" or "both": C of them), the window with the
        columns [k * band, (k + 1) * band) set to zero ("bands" or "both": ceil(P / band)) --, runs them through the forward pass beside the
        window itself and reduces their rows to one record.  Returns a dict: ``rows`` (B,) of synthetic.OCCLUDE_DTYPE (variants, nonfinite;
        per group [0 = channels, 1 = bands]: flips per head, decision_flips per reference base, lean / lean_drop per head; max_delta),
        ``base_rows`` -- bit for bit predict_numpy(x) --, ``channels``, ``bands`` (the two groups' sizes), ``band``, ``on_fp32`` (full
        alignment: the range guard met the call and it ran on the fp32 forms; the handle stays as it was), ``passes``, ``bytes_staged``,
        ``expand_us`` / ``reduce_us``; with drops=True ``drops`` (B, K, 4), the map of every variant's drop in every head, with
        variant_rows=True ``variant_rows`` (B * K, row_size).  synthetic.occlude_variants / occlude_records are the same in numpy."""
        plan = self._occlude_plan(what, band)
        self._need_handle()
        x, dt = self._window_batch(x)
        extra = {}
        if self.KIND == _lib.KIND_FULL_ALIGNMENT:
            if x.ndim != 4:
                raise _lib.C3Error(f"windows (B, depth, positions, C) expected, got shape {x.shape}")
            extra["counts"] = syn.pack_fa_rows(x)[2]
        return self._occlude_call("c3_occlude", (x.ctypes.data, dt), x.shape[0], plan, drops, variant_rows, extra)

    def occlude_reduce(self, base_rows, variant_rows, channels, bands, drops=False):
        """The records of occlusion mode for rows the caller holds (c3_occlude_reduce): ``base_rows`` (B, row) float32, ``variant_rows``
        (B * (channels + bands), row) every window's variants, group 0 then group 1; row = output_size, or that + DECODE_COLS with the
        decoder columns filled in.  Returns a dict: ``rows`` (B,) of synthetic.OCCLUDE_DTYPE, ``channels``, ``bands``, and with drops=True
        ``drops`` (B, K, 4) -- what synthetic.occlude_records gives.  Needs no weights."""
        self._need_handle()
        base = np.ascontiguousarray(base_rows, dtype=np.float32)
        var = np.ascontiguousarray(variant_rows, dtype=np.float32)
        channels, bands = int(channels), int(bands)
        if base.ndim != 2 or var.ndim != 2 or var.shape[1] != base.shape[1]:
            raise _lib.C3Error(f"base rows (B, row) and variant rows (n, row) float32 expected, got {base.shape} and {var.shape}")
        if channels >= 0 and bands >= 0 and len(var) != len(base) * (channels + bands):
            raise _lib.C3Error(f"{len(base)} windows of {channels + bands} variants need {len(base) * (channels + bands)} variant rows, {len(var)} given")
        rec = np.zeros(len(base), dtype=syn.OCCLUDE_DTYPE)
        d = np.zeros((len(base), max(channels + bands, 0), 4), dtype=np.float32) if drops else None
        _lib.check(_lib.lib().c3_occlude_reduce(self._handle, base.ctypes.data, var.ctypes.data, base.shape[1], channels, bands, len(base),
                                                rec.ctypes.data, None if d is None else d.ctypes.data), "c3_occlude_reduce")
        out = dict(rows=rec, channels=channels, bands=bands)
        if drops:
            out["drops"] = d
        return out

    def predict_exact(self, x):
        """float64 (B, 24|90): the rows of the windows ``x`` in the arithmetic of the fp64 oracle, computed on the device (c3_predict_exact;
        blocking; windows only).  Whatever precision, plan or calibration the handle runs does not enter."""
        self._need_handle()
        x, dt = self._window_batch(x)
        y = np.empty((x.shape[0], self.output_size), dtype=np.float64)
        _lib.check(_lib.lib().c3_predict_exact(self._handle, x.ctypes.data, dt, x.shape[0], y.ctypes.data), "c3_predict_exact")
        return y

    def exact_fetch(self, name, first, shape):
        """windows first .. first + shape[0] of a layer output of the LAST PASS of the last predict_exact call as float64 (c3_exact_fetch);
        names and layouts are tap_fetch's"""
        self._need_handle()
        out = np.empty(shape, dtype=np.float64)
        _lib.check(_lib.lib().c3_exact_fetch(self._handle, name.encode(), int(first), int(shape[0]), out.ctypes.data, out.size), "c3_exact_fetch")
        return out

    def range_status(self):
        """(flag, on_fp32): flag != 0 when an fp16x3 batch of this handle produced an activation near the fp16 range
        (or a non-finite row under the checked entry); on_fp32 when the handle has switched to fp32 matrix
        instructions.  Synchronises the device."""
        f, o = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().c3_model_range_status(self._handle, C.byref(f), C.byref(o)), "c3_model_range_status")
        return f.value, bool(o.value)

    def synchronize(self):
        _lib.check(_lib.lib().c3_model_synchronize(self._handle), "c3_model_synchronize")

    # ---- introspection (parity tests / bench) ----
    def keep_activations(self, enable=True):
        self._keep = bool(enable)
        if self._handle is not None:
            _lib.check(_lib.lib().c3_debug_keep_activations(self._handle, int(enable)), "c3_debug_keep_activations")
        return self

    def debug_fetch(self, name, shape):
        out = np.empty(shape, dtype=np.float32)
        _lib.check(_lib.lib().c3_debug_fetch(self._handle, name.encode(), out.ctypes.data, out.size), "c3_debug_fetch")
        return out

    def tap(self, names):
        """capture these layer outputs of every later call on the forms it really runs (c3_debug_tap); names: iterable or
        comma-separated string, empty = off"""
        names = names if isinstance(names, str) else ",".join(names)
        self._taps = names
        if self._handle is not None:
            _lib.check(_lib.lib().c3_debug_tap(self._handle, names.encode()), "c3_debug_tap")
        return self

    def tap_fetch(self, name, first, shape):
        """windows first .. first + shape[0] of a tapped tensor of the last call (c3_debug_tap_fetch)"""
        out = np.empty(shape, dtype=np.float32)
        _lib.check(_lib.lib().c3_debug_tap_fetch(self._handle, name.encode(), int(first), int(shape[0]), out.ctypes.data, out.size),
                   "c3_debug_tap_fetch")
        return out

    def profile(self, enable=True):
        _lib.check(_lib.lib().c3_profile_enable(self._handle, int(enable)), "c3_profile_enable")

    def profile_reset(self):
        _lib.check(_lib.lib().c3_profile_reset(self._handle), "c3_profile_reset")

    def profile_read(self):
        buf = (_lib.KernelStat * 64)()
        n = _lib.lib().c3_profile_read(self._handle, buf, 64)
        if n < 0:
            raise _lib.C3Error(f"c3_profile_read: {_lib.last_error()}")
        return [dict(name=buf[i].name.decode(), launches=buf[i].launches, total_ms=buf[i].total_ms,
                     flops=buf[i].flops, bytes=buf[i].bytes, mfma_flops=buf[i].mfma_flops,
                     mfma_peak_tflops=buf[i].mfma_peak_tflops) for i in range(min(n, 64))]

    def _destroy(self):
        if self._handle is not None:
            _lib.lib().c3_model_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass


class _RingVerify(_HipModel):
    """verify mode of the model classes: the base's call and, behind its keywords, what the exact form on the ring added"""

    def verify(self, every=1, tol=1e-4, near_tie=1e-6, escalate=False, layers=False, reference="fp32", replace=False):
        """_HipModel._verify_with says what every keyword does.  The defaults keep the call what it was: the fp32 forms as the reference,
        no row repaired."""
        return self._verify_with(every, tol, near_tie, escalate, layers, reference, replace)


class Clair3_P(_RingVerify):
    """Pileup network: 2 x bidirectional LSTM + FC heads (reference: clair3/model.py:58-161)."""
    KIND = _lib.KIND_PILEUP
    DEFAULT_CHANNELS = 18  # shared/param_p.py:32-36

    def set_max_depth(self, n):
        """param.max_depth_dict[platform] of the rescaling rule (c3_model_set_max_depth; default 144, shared/param_p.py:15)"""
        if self._handle is None:
            self.to(0)
        _lib.check(_lib.lib().c3_model_set_max_depth(self._handle, int(n)), "c3_model_set_max_depth")
        return self

    def _region(self, region, dtypes):
        """(contiguous region matrix, its C ABI dtype); ``dtypes`` names what the entry takes in its refusal"""
        region = np.ascontiguousarray(region)
        # int64 / uint64: the size_t matrix of plp_data viewed in place (np.frombuffer(ffi.buffer(plp_data.matrix, ...)),
        # CreateTensorPileupFromCffi.py:140-146) -- no .copy(), no astype
        dt = _lib.DTYPE_I64 if region.dtype in (np.dtype(np.int64), np.dtype(np.uint64)) else _NP_DTYPE.get(region.dtype)
        if dt is None or region.ndim != 2 or region.shape[1] != self.input_channels:
            raise _lib.C3Error(f"region must be (n_cols, {self.input_channels}) {dtypes}, got {region.dtype} {region.shape}")
        return region, dt

    def _region_args(self, region, starts):
        region, dt = self._region(region, "int8/int32/int64")
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        return region, dt, starts, np.empty((len(starts), self.row_size), dtype=np.float32)

    def predict_region(self, region, starts, depths=None):
        """Rows for the windows region[starts[b] : starts[b] + 33] without materialising them: ``region`` is the
        (n_cols, 18) matrix of one pileup region, ``starts`` the per-candidate offsets the reference slices at
        (preprocess/CreateTensorPileupFromCffi.py:362-364).  Same rows, bit for bit, as predict_numpy on the slices -- with ``depths``
        (one per window) as predict_numpy(slices, depths): every window is rescaled by the factor of its own candidate."""
        region, dt, starts, y = self._region_args(region, starts)
        if depths is None:
            _lib.check(_lib.lib().c3_predict_pileup_region(self._handle, region.ctypes.data, dt, region.shape[0],
                                                           starts.ctypes.data, len(starts), y.ctypes.data),
                       "c3_predict_pileup_region")
        else:
            d = self._depths(depths, len(starts))
            _lib.check(_lib.lib().c3_predict_pileup_region_depth(self._handle, region.ctypes.data, dt, region.shape[0],
                                                                 starts.ctypes.data, len(starts), d.ctypes.data, y.ctypes.data),
                       "c3_predict_pileup_region_depth")
        return y

    def submit_region(self, region, starts, slot=0, depths=None):
        """Asynchronous half of predict_region (c3_predict_submit_region); returns a handle for wait()."""
        region, dt, starts, y = self._region_args(region, starts)
        d = None if depths is None else self._depths(depths, len(starts))
        _lib.check(_lib.lib().c3_predict_submit_region(self._handle, region.ctypes.data, dt, region.shape[0], starts.ctypes.data, len(starts),
                                                       None if d is None else d.ctypes.data, y.ctypes.data, slot),
                   "c3_predict_submit_region")
        return slot, y

    def _candidate_args(self, region, major, positions, depths):
        region, dt = self._region(region, "int32/int64")
        major = np.ascontiguousarray(major, dtype=np.int64)
        if major.shape != (region.shape[0],):
            raise _lib.C3Error(f"major must hold one entry per column: shape {major.shape} for {region.shape[0]} columns")
        positions = np.ascontiguousarray(positions, dtype=np.int64)
        if positions.ndim != 1:
            raise _lib.C3Error(f"positions must be one-dimensional, got shape {positions.shape}")
        d = None if depths is None else self._depths(depths, len(positions))
        return region, dt, major, positions, d, _CandidateBatch(len(positions), self.row_size)

    def predict_candidates(self, region, major, positions, depths=None, head_tail=False):
        """The rows of the windows the reference's pileup producer would have fed the model for these candidates
        (preprocess/CreateTensorPileupFromCffi.py:343-397), selected on the device: ``region`` is the (n_cols, 18) matrix of one pileup
        region (int32, or the int64 plp_data.matrix itself), ``major`` its plp_data.major, ``positions`` the candidates' positions in the
        caller's order, ``head_tail`` the reference's --enable_variant_calling_at_sequence_head_and_tail.  Returns (rows, status): the rows
        of the kept candidates in candidate order and one _lib.CAND_* byte per candidate (synthetic.select_pileup_windows states the rule).
        Same rows, bit for bit, as predict_numpy(windows[, depths of the kept]) on the materialised windows."""
        region, dt, major, positions, d, out = self._candidate_args(region, major, positions, depths)
        _lib.check(_lib.lib().c3_predict_pileup_candidates(
            self._handle, region.ctypes.data, dt, region.shape[0], major.ctypes.data, positions.ctypes.data, None if d is None else d.ctypes.data,
            len(positions), int(bool(head_tail)), out.rows.ctypes.data, out.status.ctypes.data, C.byref(out.n_rows)), "c3_predict_pileup_candidates")
        return out.rows[:out.n_rows.value], out.status

    def submit_candidates(self, region, major, positions, slot=0, depths=None, head_tail=False):
        """Asynchronous half of predict_candidates (c3_predict_submit_candidates); wait() on the ticket returns (rows, status)."""
        region, dt, major, positions, d, out = self._candidate_args(region, major, positions, depths)
        _lib.check(_lib.lib().c3_predict_submit_candidates(
            self._handle, region.ctypes.data, dt, region.shape[0], major.ctypes.data, positions.ctypes.data, None if d is None else d.ctypes.data,
            len(positions), int(bool(head_tail)), out.rows.ctypes.data, out.status.ctypes.data, C.byref(out.n_rows), slot),
            "c3_predict_submit_candidates")
        return slot, out

    def predict_reads(self, context, head_tail=False):
        """predict_candidates on the result a pileup_reads.Context holds (context.run(reads, start, end, ...) first): the region matrix goes
        from the context's device buffer into the batch without visiting the host (c3_predict_pileup_reads).  Returns (rows, status) as
        predict_candidates(counts, major, cand_pos, cand_depth) of context.fetch() does, bit for bit."""
        out = _CandidateBatch(context.sizes()[1], self.row_size)
        _lib.check(_lib.lib().c3_predict_pileup_reads(self._handle, context.h, int(bool(head_tail)), out.rows.ctypes.data, out.status.ctypes.data,
                                                      C.byref(out.n_rows)), "c3_predict_pileup_reads")
        return out.rows[:out.n_rows.value], out.status

    def submit_reads(self, context, slot=0, head_tail=False):
        """Asynchronous half of predict_reads (c3_predict_submit_pileup); wait() on the ticket returns (rows, status)."""
        out = _CandidateBatch(context.sizes()[1], self.row_size)
        _lib.check(_lib.lib().c3_predict_submit_pileup(self._handle, context.h, int(bool(head_tail)), out.rows.ctypes.data, out.status.ctypes.data,
                                                       C.byref(out.n_rows), slot), "c3_predict_submit_pileup")
        return slot, out


class Clair3_F(_RingVerify):
    """Full-alignment network: residual 3x3-conv stack + pyramid pooling + FC heads (clair3/model.py:282-416)."""
    KIND = _lib.KIND_FULL_ALIGNMENT
    DEFAULT_CHANNELS = 8  # shared/param_f.py:24-31 (9 with --enable_dwell_time)

    def _rows_args(self, rows, counts, firsts):
        """(rows int8 (n_rows, positions, C), counts int32 [B], firsts int32 [B] | None) as the C ABI takes them; the geometry is the handle's"""
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        depth, positions = self._geometry or (89, 33)
        rows = np.ascontiguousarray(rows)
        if rows.dtype != np.int8 or rows.ndim != 3 or rows.shape[1:] != (positions, self.input_channels):
            raise _lib.C3Error(f"rows must be (n_rows, {positions}, {self.input_channels}) int8, got {rows.dtype} {rows.shape}")
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if counts.ndim != 1:
            raise _lib.C3Error(f"counts must be one-dimensional, got shape {counts.shape}")
        if firsts is not None:
            firsts = np.ascontiguousarray(firsts, dtype=np.int32)
            if firsts.shape != counts.shape:
                raise _lib.C3Error(f"firsts must hold one entry per window: shape {firsts.shape} for {len(counts)} windows")
        # the library checks every count against the depth; the sum against the rows handed over is checked here, where the array's length is known
        if (counts >= 0).all() and int(counts.sum(dtype=np.int64)) != rows.shape[0]:
            raise _lib.C3Error(f"counts add up to {int(counts.sum(dtype=np.int64))} rows, {rows.shape[0]} given")
        return rows, counts, firsts, np.empty((len(counts), self.row_size), dtype=np.float32)

    def predict_rows(self, rows, counts, firsts=None):
        """Rows of probabilities for windows handed over as their occupied read rows (c3_predict_rows): ``rows`` holds the rows of all windows
        back to back, window b owns counts[b] of them; its dense form is zero except rows [first, first + counts[b]) with first =
        (depth - counts[b]) // 2 -- the padding rule of the reference's generator (clair3/utils.py:113-121) -- or firsts[b] where ``firsts`` is
        given.  The zero rows are restored on the device: same rows, bit for bit, as predict_numpy(synthetic.pad_fa_rows(rows, counts, firsts))."""
        rows, counts, firsts, y = self._rows_args(rows, counts, firsts)
        _lib.check(_lib.lib().c3_predict_rows(self._handle, rows.ctypes.data, None if firsts is None else firsts.ctypes.data, counts.ctypes.data,
                                              len(counts), y.ctypes.data), "c3_predict_rows")
        return y

    def predict_reads(self, context):
        """predict_rows on the result a fa_reads.Context holds (context.run(reads, extras, centres, ...) first): the rows go from the
        context's device buffer into the batch without visiting the host (c3_predict_fa_reads).  Returns the probability rows, one per
        candidate, bit for bit predict_rows(rows, counts) of context.fetch().  The handle's depth must be the result's matrix_depth."""
        if self._handle is None:
            raise _lib.C3Error("model has no device/weights yet: call .to(device) and .load_state_dict() first")
        y = np.empty((context.sizes()[0], self.row_size), dtype=np.float32)
        n = C.c_int64(0)
        _lib.check(_lib.lib().c3_predict_fa_reads(self._handle, context.h, y.ctypes.data if y.size else None, C.byref(n)), "c3_predict_fa_reads")
        return y

    # ---- jackknife mode: does a call survive when one read of its window is taken away? (c3_jackknife_rows) ----
    def _jackknife_out(self, counts, y, rec, drops, variant_rows, info):
        out = dict(rows=rec, counts=counts, base_rows=y, on_fp32=bool(info.on_fp32), passes=int(info.passes), bytes_staged=int(info.bytes_staged),
                   expand_us=float(info.expand_us), reduce_us=float(info.reduce_us))
        if drops is not None:
            out["drops"] = drops
        if variant_rows is not None:
            out["variant_rows"] = variant_rows
        return out

    def jackknife_rows(self, rows, counts, firsts=None, layout="recentre", drops=False, variant_rows=False):
        """Leave-one-read-out stability of windows handed over as their occupied rows (predict_rows's arguments; c3_jackknife_rows): for
        every window the device builds its counts[b] variants -- the window without one row of its run, laid out again by the reference's
        padding rule ("recentre") or left where the run starts ("in_place") --, runs them through the forward pass beside the window itself
        and reduces their rows to one record.  Returns a dict: ``rows`` (B,) of synthetic.JACKKNIFE_DTYPE (reads, nonfinite, flips per head,
        decision_flips per reference base, lean_read / lean_drop per head, max_delta), ``counts``, ``base_rows`` -- bit for bit
        predict_rows(rows, counts, firsts) --, ``on_fp32`` (the range guard met the call and it ran on the fp32 forms; the handle stays as it
        was), ``passes``, ``bytes_staged``, ``expand_us`` / ``reduce_us`` (device time of the two kernels' launches); with drops=True ``drops`` (sum(counts), 4), with variant_rows=True ``variant_rows``
        (sum(counts), row_size).  synthetic.leave_one_out / jackknife_records are the same in numpy."""
        code = self._jackknife_layout(layout)
        rows, counts, firsts, y = self._rows_args(rows, counts, firsts)
        total = int(np.clip(counts, 0, None).sum(dtype=np.int64))
        rec = np.zeros(len(counts), dtype=syn.JACKKNIFE_DTYPE)
        d = np.zeros((total, 4), dtype=np.float32) if drops else None
        v = np.zeros((total, self.row_size), dtype=np.float32) if variant_rows else None
        info = _lib.JackknifeInfo()
        _lib.check(_lib.lib().c3_jackknife_rows(self._handle, rows.ctypes.data, None if firsts is None else firsts.ctypes.data, counts.ctypes.data,
                                                len(counts), code, y.ctypes.data, rec.ctypes.data, None if d is None else d.ctypes.data,
                                                None if v is None else v.ctypes.data, C.byref(info)), "c3_jackknife_rows")
        return self._jackknife_out(counts, y, rec, d, v, info)

    def jackknife(self, x, layout="recentre", drops=False, variant_rows=False):
        """jackknife_rows of dense int8 windows (c3_jackknife): every window's run -- from its first to its last non-zero row -- is found on
        the host as synthetic.pack_fa_rows finds it, and its first row is the run's own.  ``counts`` of the result are the runs' lengths."""
        code = self._jackknife_layout(layout)
        self._need_handle()
        x, dt = self._window_batch(x)
        if x.ndim != 4:
            raise _lib.C3Error(f"windows (B, depth, positions, C) expected, got shape {x.shape}")
        _, _, counts = syn.pack_fa_rows(x)
        total = int(counts.sum(dtype=np.int64))
        y = np.empty((x.shape[0], self.row_size), dtype=np.float32)
        rec = np.zeros(len(x), dtype=syn.JACKKNIFE_DTYPE)
        d = np.zeros((total, 4), dtype=np.float32) if drops else None
        v = np.zeros((total, self.row_size), dtype=np.float32) if variant_rows else None
        info = _lib.JackknifeInfo()
        _lib.check(_lib.lib().c3_jackknife(self._handle, x.ctypes.data, dt, x.shape[0], code, y.ctypes.data, rec.ctypes.data,
                                           None if d is None else d.ctypes.data, None if v is None else v.ctypes.data, C.byref(info)), "c3_jackknife")
        return self._jackknife_out(counts, y, rec, d, v, info)

    # ---- subsample mode: at what coverage does a call hold? (c3_subsample_rows) ----
    def _subsample_call(self, entry, head, counts, y, plan, layout, masks, variant_rows):
        d, replicates, seed = plan
        total = int(syn.subsample_variant_counts(np.clip(counts, 0, None), d, replicates).sum())
        lev = np.zeros((len(counts), len(d)), dtype=syn.SUBSAMPLE_LEVEL_DTYPE)
        rec = np.zeros(len(counts), dtype=syn.SUBSAMPLE_WINDOW_DTYPE)
        mk = np.zeros((total, 2), dtype=np.uint64) if masks else None
        v = np.zeros((total, self.row_size), dtype=np.float32) if variant_rows else None
        info = _lib.SubsampleInfo()
        _lib.check(getattr(_lib.lib(), entry)(self._handle, *head, len(counts), d.ctypes.data, len(d), replicates, seed, layout, y.ctypes.data,
                                              rec.ctypes.data, lev.ctypes.data, None if mk is None else mk.ctypes.data,
                                              None if v is None else v.ctypes.data, C.byref(info)), entry)
        out = dict(levels=lev, rows=rec, counts=counts, base_rows=y, depths=d, replicates=replicates, seed=seed, variants=int(info.variants),
                   on_fp32=bool(info.on_fp32), passes=int(info.passes), bytes_staged=int(info.bytes_staged), expand_us=float(info.expand_us),
                   reduce_us=float(info.reduce_us))
        if masks:
            out["masks"] = mk
        if variant_rows:
            out["variant_rows"] = v
        return out

    def subsample_rows(self, rows, counts, firsts=None, depths=(10, 20, 30, 40), replicates=8, seed=0, layout="recentre", masks=False,
                       variant_rows=False):
        """Stability under random read subsampling of windows handed over as their occupied rows (predict_rows's arguments;
        c3_subsample_rows): for every target depth D of ``depths`` (1 .. 8 of them, strictly increasing) below a window's counts[w] the device
        draws ``replicates`` (1 .. 32) subsets of D of its reads from a counter hash of ``seed`` -- nested from level to level --, lays them
        out by the reference's padding rule ("recentre") or where the run starts ("in_place"), runs them through the forward pass beside the
        window itself and reduces their rows.  Returns a dict: ``levels`` (B, L) of synthetic.SUBSAMPLE_LEVEL_DTYPE (keep, run, nonfinite,
        decision_flips, flips and min_kept per head), ``rows`` (B,) of synthetic.SUBSAMPLE_WINDOW_DTYPE (reads, levels_run, hold_level per
        head, hold_decision), ``counts``, ``base_rows`` -- bit for bit predict_rows(rows, counts, firsts) --, ``variants``, ``on_fp32``,
        ``passes``, ``bytes_staged``, ``expand_us`` / ``reduce_us``; with masks=True ``masks`` (variants, 2) uint64, bit j = read j kept,
        with variant_rows=True ``variant_rows`` (variants, row_size).  synthetic.subsample_masks / subsample_variants /
        subsample_records are the same in numpy."""
        code = self._jackknife_layout(layout)
        plan = self._subsample_plan(depths, replicates, seed)
        rows, counts, firsts, y = self._rows_args(rows, counts, firsts)
        head = (rows.ctypes.data, None if firsts is None else firsts.ctypes.data, counts.ctypes.data)
        return self._subsample_call("c3_subsample_rows", head, counts, y, plan, code, masks, variant_rows)

    def subsample(self, x, depths=(10, 20, 30, 40), replicates=8, seed=0, layout="recentre", masks=False, variant_rows=False):
        """subsample_rows of dense int8 windows (c3_subsample): every window's run -- from its first to its last non-zero row -- is found on
        the host as synthetic.pack_fa_rows finds it, and its first row is the run's own.  ``counts`` of the result are the runs' lengths."""
        code = self._jackknife_layout(layout)
        plan = self._subsample_plan(depths, replicates, seed)
        self._need_handle()
        x, dt = self._window_batch(x)
        if x.ndim != 4:
            raise _lib.C3Error(f"windows (B, depth, positions, C) expected, got shape {x.shape}")
        _, _, counts = syn.pack_fa_rows(x)
        y = np.empty((x.shape[0], self.row_size), dtype=np.float32)
        return self._subsample_call("c3_subsample", (x.ctypes.data, dt), counts, y, plan, code, masks, variant_rows)

    def occlude_rows(self, rows, counts, firsts=None, what="both", band=1, drops=False, variant_rows=False):
        """occlude() of windows handed over as their occupied rows (predict_rows's arguments; c3_occlude_rows): the variants keep the run
        where ``firsts`` or the centring rule puts it.  ``base_rows`` of the result are bit for bit predict_rows(rows, counts, firsts)."""
        plan = self._occlude_plan(what, band)
        rows, counts, firsts, _ = self._rows_args(rows, counts, firsts)
        head = (rows.ctypes.data, None if firsts is None else firsts.ctypes.data, counts.ctypes.data)
        return self._occlude_call("c3_occlude_rows", head, len(counts), plan, drops, variant_rows, dict(counts=counts))

    def submit_rows(self, rows, counts, firsts=None, slot=0):
        """Asynchronous half of predict_rows (c3_predict_submit_rows); returns a handle for wait()."""
        rows, counts, firsts, y = self._rows_args(rows, counts, firsts)
        _lib.check(_lib.lib().c3_predict_submit_rows(self._handle, rows.ctypes.data, None if firsts is None else firsts.ctypes.data,
                                                     counts.ctypes.data, len(counts), y.ctypes.data, slot), "c3_predict_submit_rows")
        return slot, y
