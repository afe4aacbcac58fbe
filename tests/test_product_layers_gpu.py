"""Layer by layer on the kernel forms the product runs (needs an MI355X).  Keep mode (c3_debug_keep_activations) switches the fused forms
off -- conv1 inside res1a / res1b (the SRC8 direct plane kernel), the pyramid pooling as res3b's epilogue, the ring's lanes -- so the
keep-mode parity tests see every layer of OTHER forms than a default call runs.  Debug taps
(c3_debug_tap) copy a layer's output right behind the launch that produced it without changing the form: every tapped tensor of the
default forms, at batch sizes that cross each form boundary, against the fp64 oracle, next to the fp32-MFMA forms (C3HIP_FP32=1) on
the same windows.  Bounds are the ones the keep-mode tests meet: 2e-5 of a tensor's range and of a channel's own scale, and no worse
than 5x the fp32 forms' error (+3e-7 per tensor, +1e-6 per channel); rows within 2e-5 of the oracle, labels identical outside near-ties."""
import numpy as np
import pytest

from clair3_amd import synthetic as syn
from tests import util
from tests.test_parity_gpu import make_model

pytestmark = pytest.mark.gpu

FA_TAPS = tuple(f"act{l}" for l in range(9)) + ("spp", "l4_out")
P_TAPS = ("lstm1_out", "gx2", "lstm2_out", "l4_out")
FA_MICRO, P_MICRO = 2048, 16384  # windows per micro-batch (c3_model.h max_microbatch)
TABLE = []  # (what, per tensor, per channel) of every run, printed at the end of each test


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("C3HIP_FP32", "C3HIP_WINO", "C3HIP_KEEP_ACTIVATIONS"):
        monkeypatch.delenv(k, raising=False)


def sample(n, splits=()):
    """every window of a batch up to 64; else both ends, 8 on each side of every split (micro-batches) and 16 random"""
    if n <= 64:
        return np.arange(n)
    idx = set(range(8)) | set(range(n - 8, n))
    for s in splits:
        if 0 < s < n:
            idx |= set(range(max(0, s - 8), min(n, s + 8)))
    idx |= set(np.random.default_rng(1000 + n).choice(n, 16, replace=False).tolist())
    return np.array(sorted(idx))


def runs(idx):
    """contiguous (first, count) pieces of a sorted index list"""
    out, a = [], 0
    for i in range(1, len(idx) + 1):
        if i == len(idx) or idx[i] != idx[i - 1] + 1:
            out.append((int(idx[a]), i - a))
            a = i
    return out


def tapped(m, name, idx, tail):
    return np.concatenate([m.tap_fetch(name, a, (k,) + tail) for a, k in runs(idx)])


class Oracle:
    """the fp64 oracle's rows and debug tensors per window index of one pool of windows, computed once"""

    def __init__(self, kind, sd, x, indel):
        self.kind, self.sd, self.x, self.indel, self.cache = kind, sd, x, indel, {}

    def __call__(self, idx):
        from oracle import oracle
        todo = np.array([i for i in idx if i not in self.cache], dtype=np.int64)
        if len(todo):
            y, d = oracle.forward(self.kind, self.sd, self.x[todo], self.indel, debug=True)
            for j, i in enumerate(todo):
                self.cache[int(i)] = (y[j], {k: v[j] for k, v in d.items()})
        y = np.stack([self.cache[int(i)][0] for i in idx])
        d = {k: np.stack([self.cache[int(i)][1][k] for i in idx]) for k in self.cache[int(idx[0])][1]}
        return y, d


def _print_table(title):
    print(f"\n{title}: worst error per tensor / worst channel (x1e-6)")
    for what, whole, chan in TABLE:
        print(f"  {what:58s} " + " ".join(f"{k}={whole[k] * 1e6:.2f}" + (f"/{chan[k] * 1e6:.2f}" if k in chan else "") for k in whole))
    TABLE.clear()


# ------------------------------------------------------------------------------------------ full alignment
# (weights, channels, depth) -> [(env, batch sizes)]: together every form of the product stack
FA_POOLS = {
    ("plain", 8, 89): [({}, [1, 7, 17, 158, 159, 191, 192, 273, 274, 330, 333, 1100, FA_MICRO + 37]),
                       ({"C3HIP_WINO": "0"}, [17, 330]), ({"C3HIP_WINO": "1"}, [330])],
    ("peaked", 9, 55): [({}, [1, 17, 159, 274, 333, 1100]), ({"C3HIP_WINO": "0"}, [330])],
    ("trained_like", 8, 89): [({}, [7, 192, 330, FA_MICRO + 37]), ({"C3HIP_WINO": "0"}, [159])],
    ("trained_like", 9, 89): [({}, [17, 1100]), ({"C3HIP_WINO": "0"}, [274])],
}
FORMS_SEEN = set()


def _fa_pool(weights, ch, depth):
    # the weight seeds of the keep-mode tests (test_parity_gpu.py), whose activations stay inside the fp16 range guard
    seed = {"plain": 41, "peaked": 43, "trained_like": 141}[weights]
    sd = syn.make_state_dict(syn.FULL_ALIGNMENT, ch, True, seed=seed, peaked=weights != "plain", trained_like=weights == "trained_like")
    x = syn.make_fa_windows(FA_MICRO + 37, seed=seed + 1, channels=ch, depth=depth)
    return sd, x


def _fa_model(ch, depth, sd, taps):
    m = make_model(syn.FULL_ALIGNMENT, ch, True, sd, depth=depth)
    return m.tap(taps)


def _fa_layers(m, idx, d, names):
    return {name: tapped(m, name, idx, d[name].shape[1:]) for name in names}


@pytest.mark.parametrize("weights,ch,depth", list(FA_POOLS))
def test_full_alignment_product_layers(weights, ch, depth, monkeypatch):
    sd, x = _fa_pool(weights, ch, depth)
    oracle = Oracle(syn.FULL_ALIGNMENT, sd, x, True)
    plan = []
    for env, sizes in FA_POOLS[(weights, ch, depth)]:
        for n in sizes:
            plan.append((env, n, sample(n, [FA_MICRO])))
    # the comparison form: fp32 MFMA on fp32 activations, every layer written, one forward pass over the whole pool
    every = np.array(sorted(set().union(*[set(p[2].tolist()) for p in plan])))
    monkeypatch.setenv("C3HIP_FP32", "1")
    m32 = _fa_model(ch, depth, sd, FA_TAPS)
    monkeypatch.delenv("C3HIP_FP32")
    n32 = int(every.max()) + 1
    m32.wait(m32.submit(x[:n32], slot=0))
    assert "conv_stack=fp32-mfma" in m32.describe()
    y_all, d_all = oracle(every)
    f32 = _fa_layers(m32, every, d_all, FA_TAPS)
    pos = {int(i): j for j, i in enumerate(every)}
    for env, n, idx in plan:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = _fa_model(ch, depth, sd, FA_TAPS)
        y = m.wait(m.submit(x[:n], slot=0))  # one forward pass over all n (the blocking call would cut it into pieces)
        form = m.describe()
        for k in env:
            monkeypatch.delenv(k)
        FORMS_SEEN.add(form)
        assert "conv_stack=planes-f16x3" in form and "on_fp32=0" in form, form
        names = list(FA_TAPS)
        # the product form writes no act0 (conv1 inside res1a) and, on 12 x 5 images, no act8 (the pooling inside res3b)
        with pytest.raises(Exception, match="act0 is computed inside res1a"):
            m.tap_fetch("act0", 0, (1,) + d_all["act0"].shape[1:])
        names.remove("act0")
        if depth == 89:
            with pytest.raises(Exception, match="act8 is pooled inside res3b"):
                m.tap_fetch("act8", 0, (1,) + d_all["act8"].shape[1:])
            names.remove("act8")
        y_o, d = oracle(idx)
        sel = [pos[int(i)] for i in idx]
        mine = _fa_layers(m, idx, d, names)
        whole, chan = util.layer_errors(lambda k: mine[k], d, names, sd)
        w32, c32 = util.layer_errors(lambda k: f32[k][sel], d, names, sd)
        whole["y"] = util.assert_rows_match(y[idx], y_o, tol=2e-5, what=f"{weights} C={ch} depth={depth} n={n} {env}")
        what = f"{weights} C={ch} d={depth} n={n} {env or ''}"
        TABLE.append((what, whole, chan))
        TABLE.append(("   fp32 forms, same windows", w32, c32))
        for k in names:
            assert whole[k] <= 2e-5 and whole[k] <= 5 * w32[k] + 3e-7, (what, k, whole[k], w32[k])
            if k in chan:
                assert chan[k] <= 2e-5 and chan[k] <= 5 * c32[k] + 1e-6, (what, k, chan[k], c32[k])
        # the blocking call runs a large batch as pieces (on the ring's lanes): the same rows, and every piece's layers at their place
        if n == FA_MICRO + 37:
            assert np.array_equal(m.predict_numpy(x[:n]), y), "the blocking call's pieces changed the rows"
            for k in names:  # ... and its taps hold every piece's windows at their place in the call
                assert np.array_equal(tapped(m, k, idx, d[k].shape[1:]), mine[k]), (what, "c3_predict pieces", k)
    _print_table(f"full alignment, {weights} weights, C={ch}, depth {depth}")


def test_full_alignment_forms_seen(monkeypatch):
    """the sweep above ran every form of the stack (after it in file order; run alone, the sweep's calls are repeated for their forms)"""
    if not FORMS_SEEN:
        for (weights, ch, depth), legs in FA_POOLS.items():
            sd, x = _fa_pool(weights, ch, depth)
            for env, sizes in legs:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                m = _fa_model(ch, depth, sd, "")
                for n in sizes:
                    m.wait(m.submit(x[:n], slot=0))
                    FORMS_SEEN.add(m.describe())
                for k in env:
                    monkeypatch.delenv(k)
    seen = " | ".join(sorted(FORMS_SEEN))
    for want in ("stride1=ddwwwd", "stride1=dddddd", "stride1=ddwwdd", "conv3=one-workgroup-per-cu", "conv3=two-workgroups-per-cu",
                 "conv5=one-workgroup-per-cu", "conv5=two-workgroups-per-cu", "conv_stack=planes-f16x3"):
        assert want in seen, (want, seen)
    print("forms seen:\n  " + "\n  ".join(sorted(FORMS_SEEN)))


# ------------------------------------------------------------------------------------------ pileup
def _gx2(sd, h1):
    """LSTM2's input projection of both directions with both biases, float64: (B, T, 1280), PyTorch gate order"""
    out = []
    for sfx in ("", "_reverse"):
        w = sd[f"LSTM2.weight_ih_l0{sfx}"].astype(np.float64)
        b = sd[f"LSTM2.bias_ih_l0{sfx}"].astype(np.float64) + sd[f"LSTM2.bias_hh_l0{sfx}"].astype(np.float64)
        out.append(h1.astype(np.float64) @ w.T + b)
    return np.concatenate(out, axis=-1)


P_PLAN = [  # (weights, env, sharing hint, dtype, sizes)
    ("plain", {}, 1, np.int8, [1, 17, 189, 190, 191, 767, 768, 1024, 8192, P_MICRO + 37]),
    ("plain", {}, 2, np.int8, [8192]),
    ("plain", {}, 1, np.int32, [17, 1024]),
    ("trained_like", {}, 1, np.int8, [17, 1024]),
    ("trained_like", {"C3HIP_FP32": "0"}, 1, np.int8, [17, 1024]),
    ("trained_like", {"C3HIP_FP32": "0"}, 1, np.int32, [190]),
]


@pytest.mark.parametrize("weights", ["plain", "trained_like"])
def test_pileup_product_layers(weights, monkeypatch):
    sd = syn.make_state_dict(syn.PILEUP, 18, True, seed=151 if weights == "trained_like" else 51, trained_like=weights == "trained_like")
    x8 = syn.make_pileup_windows(P_MICRO + 37, seed=52)
    oracle = Oracle(syn.PILEUP, sd, x8, True)  # int32 windows carry the same counts: one oracle for both
    forms = set()
    for w, env, sharing, dt, sizes in P_PLAN:
        if w != weights:
            continue
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = make_model(syn.PILEUP, 18, True, sd).tap(P_TAPS)
        if sharing > 1:
            m.sharing(sharing)
        for n in sizes:
            idx = sample(n, [P_MICRO])
            y = m.wait(m.submit(x8[:n].astype(dt), slot=0))
            form = m.describe()
            forms.add(form.split(" on_fp32")[0] + f" precision={form.split('precision=')[1].split()[0]}")
            y_o, d = oracle(idx)
            d["gx2"] = _gx2(sd, d["lstm1_out"])
            whole = {}
            for name in P_TAPS:
                a = tapped(m, name, idx, d[name].shape[1:])
                assert np.isfinite(a).all(), name
                whole[name] = float(np.abs(a - d[name]).max()) / max(1.0, float(np.abs(d[name]).max()))
            what = f"{weights} n={n} {np.dtype(dt).name} sharing={sharing} {env or ''}"
            whole["y"] = util.assert_rows_match(y[idx], y_o, tol=2e-5, what=what)
            TABLE.append((what + f" [{form.split(' lstm1=')[1].split(' on_fp32')[0]}]", whole, {}))
            for k, v in whole.items():
                assert v <= 2e-5, (what, k, v)
        for k in env:
            monkeypatch.delenv(k)
    _print_table(f"pileup, {weights} weights (tensors relative to max(1, range))")
    seen = " | ".join(sorted(forms))
    print("forms seen:\n  " + "\n  ".join(sorted(forms)))
    if weights == "plain":
        for want in ("lstm1=fused-f16x3-half-tiles", "lstm1=fused-f16x3-full-tiles", "proj2=128x128-chunk-stream", "proj2=weights-resident ",
                     "proj2=weights-resident-half-grid"):
            assert want in seen + " ", (want, seen)
    else:
        assert "precision=fp32-auto" in seen and "precision=fp16x3" in seen, seen


# ------------------------------------------------------------------------------------------ taps change nothing
@pytest.mark.parametrize("kind,env,n", [(syn.FULL_ALIGNMENT, {}, 330), (syn.FULL_ALIGNMENT, {}, FA_MICRO + 37),
                                        (syn.PILEUP, {}, 1024), (syn.PILEUP, {}, P_MICRO + 37)])
def test_taps_change_no_form(kind, env, n, monkeypatch):
    """with taps set the call takes the same forms (describe()) and gives bit-identical rows; with the taps off again the
    handle launches the kernels it launched before any tap was set (c3_profile_read lists the same families and launches)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ch = 8 if kind == syn.FULL_ALIGNMENT else 18
    sd = syn.make_state_dict(kind, ch, True, seed=61)
    x = syn.make_windows(kind, n, seed=62, channels=ch)
    m = make_model(kind, ch, True, sd)

    def call():
        m.profile(True)
        m.profile_reset()
        y = m.wait(m.submit(x, slot=0))
        prof = [(r["name"], r["launches"]) for r in m.profile_read()]
        m.profile(False)
        return y, m.describe(), prof

    y0, d0, p0 = call()
    m.tap(FA_TAPS[1:8] + ("spp", "l4_out") if kind == syn.FULL_ALIGNMENT else P_TAPS)
    y1, d1, p1 = call()
    assert d1 == d0 and np.array_equal(y1, y0) and p1 == p0, (d0, d1, p0, p1)
    y2 = m.wait(m.submit(x, slot=0))  # ... and without the profiler (the ring's lanes)
    assert np.array_equal(y2, y0) and m.describe() == d0
    m.tap("")
    y3, d3, p3 = call()
    assert d3 == d0 and np.array_equal(y3, y0) and p3 == p0
    print(f"{kind} n={n} {env}: {d0}\n  kernels: {p0}")
    with pytest.raises(Exception, match="not tapped"):
        m.tap_fetch("l4_out", 0, (1, 256 if kind == syn.FULL_ALIGNMENT else 128))
    with pytest.raises(Exception, match="unknown tap tensor"):
        m.tap("lstm1_out" if kind == syn.FULL_ALIGNMENT else "act1")
