"""Serve mode on the device (needs an MI355X): c3_predict_submit_parts against c3_predict on the concatenation, the range guard over a batch
of parts, three client processes through a real server, and the reference's unmodified worker loop on its CPU branch with its model
behind the server.

Every child process is a fresh ``subprocess`` child with a timeout of its own; the server is terminated in a ``finally``; after a child
that faulted, aborted or ran into its timeout nothing further is started (``_STOPPED``).  At most the test process and ONE child hold the
GPU at a time: the GPU-branch worker runs that the last test compares with are made before the server starts."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from clair3_amd import _lib, client, synthetic as syn
from clair3_amd.model import Clair3_F, Clair3_P
from tests import refloop
from tests.test_calibration import recipe_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120
_STOPPED = []  # why nothing further may be started


def child_ok(what, returncode, out):
    """a child that faulted, aborted or was killed ends the file's use of the GPU; any other failure is just a failure"""
    if returncode in (134, 139, 124, 137, -6, -11, -9):
        _STOPPED.append(f"{what} ended with status {returncode}")
    assert returncode == 0, f"{what}: status {returncode}\n{out[-3000:]}"


def may_start():
    if _STOPPED:
        pytest.fail(f"nothing further is started: {_STOPPED[0]}")


def run_child(what, cmd, env=None, cwd=None, timeout=CHILD_TIMEOUT):
    may_start()
    try:
        r = subprocess.run(cmd, env=env, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _STOPPED.append(f"{what} did not end within {timeout} s")
        pytest.fail(f"{what}: no end within {timeout} s\n{(e.stdout or b'')[-2000:]}")
    child_ok(what, r.returncode, r.stdout + r.stderr)
    return r.stdout + r.stderr


def child_env(**extra):
    env = {k: v for k, v in os.environ.items() if k != "C3HIP_SERVER"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, refloop.STUBS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env.update(extra)
    return env


# ================================================================================================ 1: parts against the concatenation
_MODELS = {}


def model(kind, channels, indel, depth=89, decoder=False):
    """one handle per configuration for the whole file (synthetic weights, seed 3)"""
    key = (kind, channels, indel, depth, decoder)
    if key not in _MODELS:
        cls = Clair3_P if kind == syn.PILEUP else Clair3_F
        m = cls(add_indel_length=indel, predict=True, input_channels=channels)
        if kind == syn.FULL_ALIGNMENT:
            m.set_geometry(depth, 33)
        m.to("cuda:0")
        if decoder:
            m.decode_columns(True)
        m.load_state_dict(syn.make_state_dict(kind, channels, indel, seed=3))
        _MODELS[key] = m
    return _MODELS[key]


def split(x, counts):
    edges = np.cumsum([0] + list(counts))
    assert edges[-1] == len(x)
    return [x[a:b] for a, b in zip(edges, edges[1:])]


def assert_parts_equal_the_concatenation(m, x, counts):
    want = m.predict_numpy(x)
    assert want.shape == (len(x), m.row_size) and np.isfinite(want).all()
    parts = split(x, counts)
    got = m.predict_parts(parts)
    assert [g.shape for g in got] == [(n, m.row_size) for n in counts]
    assert np.array_equal(np.concatenate(got), want), "c3_predict_parts: bit for bit the rows of c3_predict on the concatenation"
    # the ring: another slot, rows into arrays the caller owns, the caller's windows overwritten as soon as submit returns
    mine = [(p.copy(), np.full((len(p), m.row_size), np.nan, dtype=np.float32)) for p in parts]
    ticket = m.submit_parts(mine, slot=2)
    for p, _ in mine:
        p[...] = 0
    out = m.wait(ticket)
    assert all(a is b for a, (_, b) in zip(out, mine))
    assert np.array_equal(np.concatenate(out), want)
    for p, w in zip(parts, split(want, counts)):  # ... and so of c3_predict on each part alone
        if len(p) in (1, 7):
            assert np.array_equal(m.predict_numpy(p), w)


PILEUP_PARTS = (1, 7, 16, 17, 0)  # the 8- and 16-window tile edges, and an empty part
FA_PARTS = (1, 2, 3, 0)           # odd counts: a window pair of the pooling tile lies across two parts


@pytest.mark.parametrize("dtype", [np.int8, np.int32])
@pytest.mark.parametrize("indel", [False, True])
def test_pileup_parts_are_the_concatenation(dtype, indel):
    m = model(syn.PILEUP, 18, indel)
    x = syn.make_pileup_windows(sum(PILEUP_PARTS), seed=11, dtype=dtype)
    assert_parts_equal_the_concatenation(m, x, PILEUP_PARTS)
    assert_parts_equal_the_concatenation(m, x, (0,) + PILEUP_PARTS[::-1])


@pytest.mark.parametrize("channels,depth", [(8, 89), (9, 89), (8, 55)])
def test_full_alignment_parts_are_the_concatenation(channels, depth):
    m = model(syn.FULL_ALIGNMENT, channels, True, depth=depth)
    x = syn.make_fa_windows(sum(FA_PARTS), seed=12, channels=channels, depth=depth)
    assert_parts_equal_the_concatenation(m, x, FA_PARTS)
    assert_parts_equal_the_concatenation(m, x, (3, 0, 1, 2))


@pytest.mark.parametrize("kind", [syn.PILEUP, syn.FULL_ALIGNMENT])
def test_parts_with_decoder_columns(kind):
    m = model(kind, 18 if kind == syn.PILEUP else 8, True, decoder=True)
    assert m.row_size == 90 + 31
    counts = PILEUP_PARTS if kind == syn.PILEUP else FA_PARTS
    x = syn.make_windows(kind, sum(counts), seed=13)
    assert_parts_equal_the_concatenation(m, x, counts)


def test_what_the_parts_entry_refuses():
    import ctypes as C
    m = model(syn.PILEUP, 18, False)
    x = syn.make_pileup_windows(2, seed=1)
    with pytest.raises(_lib.C3Error, match="1 to 64 parts"):
        m.predict_parts([])
    with pytest.raises(_lib.C3Error, match="1 to 64 parts"):
        m.predict_parts([x] * 65)
    got = m.predict_parts([x] * 64)
    assert all(np.array_equal(g, got[0]) for g in got)
    y = np.empty((2, m.row_size), dtype=np.float32)
    xp, yp, counts = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(y.ctypes.data), (C.c_int64 * 1)(2)
    L = _lib.lib()
    for n in (0, 65, -1):
        assert L.c3_predict_submit_parts(m._handle, xp, counts, n, _lib.DTYPE_I8, yp, 0) != 0 and "n_parts" in _lib.last_error()
    assert L.c3_predict_submit_parts(m._handle, xp, (C.c_int64 * 1)(-2), 1, _lib.DTYPE_I8, yp, 0) != 0 and "negative count" in _lib.last_error()
    assert L.c3_predict_submit_parts(m._handle, (C.c_void_p * 1)(None), counts, 1, _lib.DTYPE_I8, yp, 0) != 0 and "null buffer" in _lib.last_error()
    assert L.c3_predict_submit_parts(m._handle, xp, counts, 1, _lib.DTYPE_I64, yp, 0) != 0 and "int8" in _lib.last_error()
    fa = model(syn.FULL_ALIGNMENT, 8, True)
    assert L.c3_predict_submit_parts(fa._handle, xp, counts, 1, _lib.DTYPE_I32, yp, 0) != 0 and "int8" in _lib.last_error()
    # a refused call left every slot free
    assert np.array_equal(m.predict_parts([x])[0], m.predict_numpy(x))
    ticket = m.submit_parts([x], slot=1)
    with pytest.raises(_lib.C3Error, match="still in flight"):
        m.submit_parts([x], slot=1)
    assert np.array_equal(m.wait(ticket)[0], m.predict_numpy(x))


# ================================================================================================ 2: the range guard over a batch of parts
@pytest.mark.parametrize("policy", ["sticky", "recalibrate"])
def test_range_guard_answers_a_batch_of_parts_in_the_right_parts(policy, capfd):
    """the out-of-range recipe of tests/test_range_policy_gpu.py; the middle part carries the windows that suite trips the guard with.  Either
    policy answers the batch with the sticky guard's fp32 rows, scattered like any other batch's"""
    sd = recipe_state_dict()
    parts = [syn.make_fa_windows(2, seed=70), syn.make_fa_windows(7, seed=63), syn.make_fa_windows(3, seed=71)]

    def make(policy=None):
        m = Clair3_F(add_indel_length=True, predict=True, input_channels=8).to("cuda:0")
        if policy == "recalibrate":
            m.range_policy("recalibrate", 4)
        m.load_state_dict(sd)
        return m

    sticky = make()
    want = sticky.predict_numpy(np.concatenate(parts))
    assert sticky.range_status()[1], "the recipe trips the guard"
    m = make(policy)
    capfd.readouterr()
    got = m.predict_parts(parts)
    err = capfd.readouterr().err
    assert "libc3hip: activations beyond" in err
    for g, w, n in zip(got, split(want, [2, 7, 3]), ("first", "middle", "last")):
        assert np.array_equal(g, w), f"{n} part"
    if policy == "sticky":
        assert m.range_status()[1] and "precision=fp32-range-guard" in m.describe()
    else:
        st = m.range_stats()
        assert st["trips"] == 1 and st["recalibrations"] == 1 and st["fell_back"] == "", st
        assert not m.range_status()[1] and "precision=fp16x3" in m.describe()


# ================================================================================================ 3: through the server
CHANNELS_FA, INDEL = 8, True
SIZES = {"pileup": [300, 150], "alignment": [260, 41]}  # a few hundred windows for each network


@pytest.fixture(scope="module")
def ref():
    root = refloop.reference_root()
    if root is None:
        pytest.skip("no reference modules (oracle/_ref is staged by __graft_entry__.build())")
    return root


@pytest.fixture(scope="module")
def jobs(tmp_path_factory, ref):
    """per network: a checkpoint, a small refloop.write_job job and the VCF of the GPU-branch worker command on it -- made BEFORE the server
    starts, so that the worker and the server never hold the GPU together"""
    out = {}
    for name, kind, channels in (("pileup", syn.PILEUP, 18), ("alignment", syn.FULL_ALIGNMENT, CHANNELS_FA)):
        may_start()
        d = str(tmp_path_factory.mktemp(name))
        lst = refloop.write_job(d, kind, SIZES[name], channels=channels)
        ck = os.path.join(d, "model")
        sd = refloop.write_checkpoint(ck + ".pt", kind, channels, INDEL)
        vcf = os.path.join(d, "gpu_branch.vcf")
        try:  # one decode process: the rows are written in the order of the windows
            rc, text = refloop.run_worker(ref, lst, ck, vcf, name == "pileup", INDEL, hip=True, cpu_threads=1, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _STOPPED.append(f"the GPU-branch worker ({name}) did not end within {CHILD_TIMEOUT} s")
            raise
        child_ok(f"the GPU-branch worker ({name})", rc, text)
        out[name] = dict(dir=d, lst=lst, ck=ck, sd=sd, vcf=vcf, kind=kind, channels=channels)
    return out


@pytest.fixture(scope="module")
def server(tmp_path_factory, jobs):
    """python -m clair3_amd.serve with both models, as a fresh child; terminated in the finally"""
    may_start()
    d = tmp_path_factory.mktemp("serve")
    deep = d / ("scratch-" + "d" * 100)  # (deeper than an AF_UNIX address holds: client.socket_address)
    deep.mkdir()
    sock, log = str(deep / "c3.sock"), open(str(d / "serve.log"), "w+")
    cmd = [sys.executable, "-m", "clair3_amd.serve", "--socket", sock, "--model", f"pileup={jobs['pileup']['ck']}",
           "--model", f"alignment={jobs['alignment']['ck']}", "--add_indel_length"]
    proc = subprocess.Popen(cmd, env=child_env(), stdout=log, stderr=subprocess.STDOUT, cwd=str(d))
    try:
        end = time.monotonic() + CHILD_TIMEOUT
        while True:
            if proc.poll() is not None:
                log.seek(0)
                child_ok("the server", proc.returncode or 1, log.read())
            try:
                hello = client.control(sock, "hello", timeout=5)
                break
            except client.ServerError:
                if time.monotonic() > end:
                    _STOPPED.append("the server did not come up")
                    pytest.fail("the server did not come up")
                time.sleep(0.05)
        yield dict(sock=sock, hello=hello, proc=proc, log=log, dir=str(d))
        if proc.poll() is None:
            client.control(sock, "shutdown", timeout=10)
            proc.wait(timeout=30)
            log.seek(0)
            text = log.read()
            assert not os.path.exists(sock) and "[clair3_amd] serve:" in text, text[-2000:]
    finally:
        if proc.poll() is None:
            proc.terminate()
            try:
                proc.wait(timeout=20)
            except subprocess.TimeoutExpired:
                proc.kill()
                proc.wait()
        log.close()


CLIENT = r"""
import sys, numpy as np
from clair3_amd import client
sock, path = sys.argv[1], sys.argv[2]
data = np.load(path)
models = {n: client.RemoteModel(sock, n, add_indel_length=True) for n in ("pileup", "alignment")}
pending = {n: models[n].send(data[n]) for n in models}
print("sent", flush=True)
rows = {n: models[n].receive(pending[n]) for n in models}
np.savez(path + ".rows.npz", **rows)
assert "libamdhip64" not in open("/proc/self/maps").read()
"""

CLIENT_SHAPES = {"pileup": (7, 16, 17), "alignment": (1, 2, 3)}  # what client i sends of each network


def client_inputs(d, tag):
    paths = []
    for i in range(3):
        p = os.path.join(d, f"{tag}{i}.npz")
        np.savez(p, pileup=syn.make_pileup_windows(CLIENT_SHAPES["pileup"][i], seed=20 + i, dtype=np.int32),
                 alignment=syn.make_fa_windows(CLIENT_SHAPES["alignment"][i], seed=30 + i, channels=CHANNELS_FA))
        paths.append(p)
    return paths


@pytest.fixture(scope="module")
def local(jobs):
    """the same checkpoints in the test process: what every client's rows are compared with"""
    out = {}
    for name, cls in (("pileup", Clair3_P), ("alignment", Clair3_F)):
        m = cls(add_indel_length=INDEL, predict=True, input_channels=jobs[name]["channels"]).to("cuda:0")
        m.load_state_dict(jobs[name]["sd"])
        out[name] = m
    return out


def run_clients(server, paths, while_they_wait=None):
    may_start()
    procs = [subprocess.Popen([sys.executable, "-c", CLIENT, server["sock"], p], env=child_env(C3HIP_SERVER_TIMEOUT=str(CHILD_TIMEOUT)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for p in paths]
    try:
        for p in procs:
            assert p.stdout.readline().strip() == "sent", p.stdout.read()
        if while_they_wait:
            while_they_wait()
        for i, p in enumerate(procs):
            try:
                out, _ = p.communicate(timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                _STOPPED.append(f"client {i} did not end")
                raise
            child_ok(f"client {i}", p.returncode, out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.stdout.close()


def assert_client_rows(local, paths):
    for p in paths:
        x, y = np.load(p), np.load(p + ".rows.npz")
        for name in ("pileup", "alignment"):
            assert np.array_equal(y[name], local[name].predict_numpy(x[name])), f"{os.path.basename(p)} {name}: bit for bit the local rows"


def test_three_clients_while_paused_travel_in_one_pass(server, local):
    hello = server["hello"]["models"]
    assert set(hello) == {"pileup", "alignment"} and hello["pileup"]["row_size"] == 90 and not hello["alignment"]["decoder"]
    assert hello["alignment"]["sha256"] == client.file_sha256(hello["alignment"]["checkpoint"])
    paths = client_inputs(server["dir"], "paused")
    before = client.control(server["sock"], "stats")["stats"]
    client.control(server["sock"], "pause")

    def resume_when_all_wait():
        end = time.monotonic() + CHILD_TIMEOUT
        while set(client.control(server["sock"], "stats")["waiting"].values()) != {3}:
            assert time.monotonic() < end
            time.sleep(0.01)
        client.control(server["sock"], "resume")

    try:
        run_clients(server, paths, resume_when_all_wait)
    finally:
        client.control(server["sock"], "resume")
    assert_client_rows(local, paths)
    after = client.control(server["sock"], "stats")["stats"]
    for name in ("pileup", "alignment"):
        d = {k: after[name][k] - before[name][k] for k in ("requests", "passes", "windows")}
        assert d == dict(requests=3, passes=1, windows=sum(CLIENT_SHAPES[name])) and after[name]["max_parts"] == 3, (name, after[name])


def test_three_clients_unpaused_get_the_same_rows(server, local):
    paths = client_inputs(server["dir"], "free")
    run_clients(server, paths)
    assert_client_rows(local, paths)
    st = client.control(server["sock"], "stats")["stats"]
    assert all(st[n]["errors"] == 0 and st[n]["dropped"] == 0 for n in st), st


# ================================================================================================ 4: the reference's worker loop, CPU branch
DRIVER = r"""
import os, sys
import numpy as np
ref, job_dir, pileup = sys.argv[1], sys.argv[2], sys.argv[3] == "1"
sys.path.insert(0, ref)


def windows_of_the_job(args):
    # stands in for the tensor generator (libclair3 cannot be built offline): the windows of the job's tensor files, read as the
    # reference's own generator reads them (clair3/CallVariantsFromCffi.py:111-122), in one piece as CreateTensor*(args) returns them
    xs, positions, alt_infos = [], [], []
    for f in open(os.path.join(job_dir, "tensor_list")).read().strip().split("\n"):
        xs.append(np.load(os.path.join(job_dir, f + ".npy")))
        for row in open(os.path.join(job_dir, f + ".info")).read().strip().split("\n"):
            row = row.split("\t")
            positions.append(row[0]), alt_infos.append(row[1])
    x = np.concatenate(xs)
    return (x.astype(np.int32) if pileup else x), positions, alt_infos


if pileup:
    import preprocess.CreateTensorPileupFromCffi as ct
    ct.CreateTensorPileup = windows_of_the_job
else:
    import preprocess.CreateTensorFullAlignmentFromCffi as ct
    ct.CreateTensorFullAlignment = windows_of_the_job
from clair3_amd import run_reference
run_reference.main(sys.argv[4:])
assert "libamdhip64" not in open("/proc/self/maps").read(), "the worker on the CPU branch maps no HIP runtime"
"""


@pytest.mark.parametrize("name", ["pileup", "alignment"])
def test_unmodified_worker_loop_on_the_cpu_branch_behind_the_server(name, ref, jobs, server):
    job = jobs[name]
    got = os.path.join(job["dir"], "cpu_branch_served.vcf")
    before = client.control(server["sock"], "stats")["stats"][name]
    cmd = [sys.executable, "-c", DRIVER, ref, job["dir"], "1" if name == "pileup" else "0", "--ref", ref,
           "CallVariantsFromCffi", "--chkpnt_fn", job["ck"], "--bam_fn", "unused.bam", "--call_fn", got, "--sampleName", "SAMPLE",
           "--platform", "ont", "--threads", "4", "--add_indel_length"] + (["--pileup"] if name == "pileup" else [])
    out = run_child(f"the CPU-branch worker ({name})", cmd, env=child_env(C3HIP_SERVER=server["sock"], C3HIP_SERVER_TIMEOUT=str(CHILD_TIMEOUT)), cwd=job["dir"])
    assert f"Total processed positions : {sum(SIZES[name])}" in out, out[-3000:]
    after = client.control(server["sock"], "stats")["stats"][name]
    assert after["windows"] - before["windows"] == sum(SIZES[name]) and after["requests"] > before["requests"]
    with open(got) as a, open(job["vcf"]) as b:
        text_a, text_b = a.read(), b.read()
    assert len(refloop.vcf_records(got)) > 0
    assert text_a == text_b, "character for character the VCF of the GPU-branch worker command"


def test_a_worker_with_another_checkpoint_is_refused(ref, jobs, server):
    job, other = jobs["pileup"], jobs["alignment"]
    cmd = [sys.executable, "-c", DRIVER, ref, job["dir"], "1", "--ref", ref, "CallVariantsFromCffi",
           "--chkpnt_fn", other["ck"], "--bam_fn", "unused.bam", "--call_fn", os.path.join(job["dir"], "refused.vcf"), "--sampleName", "SAMPLE",
           "--platform", "ont", "--threads", "4", "--add_indel_length", "--pileup"]
    may_start()
    r = subprocess.run(cmd, env=child_env(C3HIP_SERVER=server["sock"]), cwd=job["dir"], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode != 0 and "another checkpoint" in r.stdout + r.stderr, (r.stdout + r.stderr)[-2000:]
