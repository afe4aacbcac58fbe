"""Serve mode without a device (clair3_amd/serve.py, clair3_amd/client.py): the server around a numpy stand-in for the model -- framing,
coalescing, pause / resume, clients that disappear, the checks of ``hello``, timeouts, and what callvar.install(server=...) rebinds."""
import json
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

from clair3_amd import client, serve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEADLINE = 20.0  # no wait in this file is open-ended


def rows_of(x, row_size):
    """what the stand-in answers: a row that only its own window determines"""
    s = x.reshape(len(x), int(np.prod(x.shape[1:]))).astype(np.int64).sum(axis=1).astype(np.float32)
    return s[:, None] + np.arange(row_size, dtype=np.float32)[None, :]


class StandIn:
    """a model as the server sees one: submit_parts / wait, rows written at wait() into the arrays the server handed over"""
    output_size = 24
    input_channels = 18
    add_indel_length = False
    _geometry = None

    def __init__(self, decoder=False, fail=None):
        self._decode_cols = decoder
        self.row_size = 24 + (31 if decoder else 0)
        self.passes, self.fail = [], fail

    def submit_parts(self, parts, slot=0):
        assert 1 <= len(parts) <= 64
        self.passes.append([len(x) for x, _ in parts])
        if self.fail:
            raise RuntimeError(self.fail)
        return slot, parts

    def wait(self, ticket):
        for x, y in ticket[1]:
            y[...] = rows_of(x, self.row_size)


def windows(n, seed):
    return np.random.default_rng(seed).integers(-20, 90, size=(n, 33, 18), dtype=np.int32)


@pytest.fixture
def sock_path(tmp_path):
    """a socket path as a job's scratch directory gives one: deeper than the 107 bytes an AF_UNIX address holds, whatever pytest's base directory is
    (client.socket_address; test_a_short_socket_path_is_used_as_it_is covers the other side)"""
    deep = tmp_path / ("scratch-" + "d" * 60) / ("chunk-" + "e" * 60)
    deep.mkdir(parents=True)
    path = str(deep / "c3.sock")
    assert len(path) > 150
    return path


@pytest.fixture
def running(sock_path):
    """start(model, **kw) -> server; everything started is shut down and joined afterwards"""
    started = []

    def start(model=None, **kw):
        model = model or StandIn()
        kw.setdefault("log", lambda text: None)
        s = serve.Server({"pileup": model}, sock_path, **kw).start()
        started.append(s)
        return s

    yield start
    for s in started:
        s.shutdown()
        s.join()


def wait_for(what, predicate):
    end = time.monotonic() + DEADLINE
    while not predicate():
        assert time.monotonic() < end, f"timed out waiting for {what}"
        time.sleep(0.005)


def queue_up(path, batches, seed=0):
    """one client per batch, each request sent (not awaited) in this order, the server having seen every one before the next leaves"""
    out = []
    for i, n in enumerate(batches):
        m = client.RemoteModel(path, "pileup", timeout=DEADLINE)
        x = windows(n, seed + i)
        out.append((m, x, m.send(x)))
        wait_for(f"request {i} to arrive", lambda: client.control(path, "stats")["waiting"]["pileup"] == i + 1)
    return out


def collect(queued):
    for m, x, pending in queued:
        y = m.receive(pending)
        assert y.shape == (len(x), m.row_size) and np.array_equal(y, rows_of(x, m.row_size)), "each client gets exactly its rows"
        m.close()


# ---------------------------------------------------------------------------------------------- framing
def test_message_framing_round_trips():
    a, b = socket.socketpair()
    try:
        msgs = [{"op": "hello"}, {"op": "predict", "shape": [3, 33, 18], "shm": "/c3hip-1-2-ab", "text": "käse ☃"}, {"big": "x" * 200000}, {}]
        for m in msgs:
            client.send_message(a, m)
        assert [client.recv_message(b) for _ in msgs] == msgs
        a.sendall(client.pack_message({"k": 1})[:3])  # a close inside a header is an error, a close between messages the end
        a.close()
        with pytest.raises(client.ServerError):
            client.recv_message(b)
    finally:
        b.close()
    a, b = socket.socketpair()
    try:
        a.close()
        assert client.recv_message(b) is None
    finally:
        b.close()
    a, b = socket.socketpair()
    try:
        a.sendall((client.MAX_MESSAGE + 1).to_bytes(4, "big"))
        with pytest.raises(client.ServerError, match="at most"):
            client.recv_message(b)
        with pytest.raises(client.ServerError):
            client.pack_message({"big": "x" * (client.MAX_MESSAGE + 1)})
    finally:
        a.close(), b.close()
    assert client.rows_offset(0) == 0 and client.rows_offset(1) == 256 and client.rows_offset(594 * 4) == 2560


# ---------------------------------------------------------------------------------------------- coalescing
def test_a_request_beyond_the_group_size_travels_alone(sock_path, running):
    model = StandIn()
    running(model, group_windows={"pileup": 10})
    client.control(sock_path, "pause")
    q = queue_up(sock_path, [4, 25, 3, 6, 2])
    assert model.passes == []
    client.control(sock_path, "resume")
    collect(q)
    assert model.passes == [[4], [25], [3, 6], [2]], "arrival order, at most 10 windows unless one request alone is larger"


def test_65_waiting_requests_are_two_passes(sock_path, running):
    model = StandIn()
    running(model)
    client.control(sock_path, "pause")
    q = queue_up(sock_path, [1] * 65)
    client.control(sock_path, "resume")
    collect(q)
    assert [len(p) for p in model.passes] == [64, 1]
    st = client.control(sock_path, "stats")["stats"]["pileup"]
    assert (st["requests"], st["passes"], st["windows"], st["max_parts"]) == (65, 2, 65, 64)


def test_pause_three_requests_resume_is_one_pass_of_three_parts(sock_path, running):
    model = StandIn()
    running(model)
    assert client.control(sock_path, "pause")["paused"]
    q = queue_up(sock_path, [5, 1, 17])
    st = client.control(sock_path, "stats")
    assert st["paused"] and st["stats"]["pileup"]["passes"] == 0 and st["waiting"]["pileup"] == 3
    assert not client.control(sock_path, "resume")["paused"]
    collect(q)
    assert model.passes == [[5, 1, 17]]
    st = client.control(sock_path, "stats")["stats"]["pileup"]
    assert (st["requests"], st["passes"], st["windows"], st["max_parts"]) == (3, 1, 23, 3)


def test_a_request_of_zero_windows_is_answered(sock_path, running):
    running()
    m = client.RemoteModel(sock_path, "pileup", timeout=DEADLINE)
    y = m.predict_numpy(np.zeros((0, 33, 18), dtype=np.int32))
    assert y.shape == (0, 24) and y.dtype == np.float32
    x = windows(3, 9)
    assert np.array_equal(m(x), rows_of(x, 24)), "... and the connection serves the next request"
    m.close()


def test_a_library_error_answers_every_part_with_its_text(sock_path, running):
    running(StandIn(fail="slot 0 still in flight"))
    client.control(sock_path, "pause")
    q = queue_up(sock_path, [2, 3])
    client.control(sock_path, "resume")
    for m, _, pending in q:
        with pytest.raises(client.ServerError, match="slot 0 still in flight"):
            m.receive(pending)
        m.close()
    assert client.control(sock_path, "stats")["stats"]["pileup"]["errors"] == 1


# ---------------------------------------------------------------------------------------------- clients that disappear
CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from clair3_amd import client
m = client.RemoteModel(sys.argv[2], "pileup", timeout=float(sys.argv[3]))
x = np.full((int(sys.argv[4]), 33, 18), 7, dtype=np.int32)
pending = m.send(x)
print("sent", pending[0].name, flush=True)
y = m.receive(pending)
maps = open("/proc/self/maps").read()
print("done", int(np.array_equal(y, x.reshape(len(x), -1).sum(1, dtype=np.int64).astype(np.float32)[:, None] + np.arange(m.row_size, dtype=np.float32))),
      int("libamdhip64" in maps), int("libc3hip" in maps), int("torch" in sys.modules), flush=True)
"""


def start_child(sock_path, n):
    env = {k: v for k, v in os.environ.items() if k != "C3HIP_SERVER"}
    return subprocess.Popen([sys.executable, "-c", CHILD, ROOT, sock_path, str(DEADLINE), str(n)], stdout=subprocess.PIPE, text=True, env=env)


def test_a_client_killed_before_its_answer_does_not_stall_the_others(sock_path, running):
    model = StandIn()
    running(model)
    client.control(sock_path, "pause")
    q = queue_up(sock_path, [4])
    child = start_child(sock_path, 6)
    try:
        line = child.stdout.readline().split()
        assert line[0] == "sent"
        wait_for("the child's request", lambda: client.control(sock_path, "stats")["waiting"]["pileup"] == 2)
        child.send_signal(signal.SIGKILL)
        child.wait(timeout=DEADLINE)
    finally:
        child.kill()
        child.stdout.close()
    q += [(m, x, m.send(x)) for m, x in [(client.RemoteModel(sock_path, "pileup", timeout=DEADLINE), windows(3, 5))]]
    client.control(sock_path, "resume")
    collect(q)
    st = client.control(sock_path, "stats")
    assert st["stats"]["pileup"]["requests"] == 3 and st["waiting"]["pileup"] == 0
    assert sum(sum(p) for p in model.passes) in (7, 13), "the survivors' windows, with or without the windows of the client that went"
    wait_for("the server to remove the segment of the client that went", lambda: not os.path.exists("/dev/shm" + line[1]))


def test_a_client_process_maps_no_hip_runtime(sock_path, running):
    running()
    child = start_child(sock_path, 5)
    try:
        out, _ = child.communicate(timeout=DEADLINE)
    finally:
        child.kill()
    done = [line.split() for line in out.splitlines() if line.startswith("done")]
    assert child.returncode == 0 and done == [["done", "1", "0", "0", "0"]], out


# ---------------------------------------------------------------------------------------------- what hello is checked against
def test_checkpoint_hash_and_decoder_mismatches_raise(sock_path, running, tmp_path):
    a, b = tmp_path / "a.pt", tmp_path / "b.pt"
    a.write_bytes(b"checkpoint a"), b.write_bytes(b"checkpoint b")
    running(info={"pileup": {"sha256": client.file_sha256(str(a))}})
    m = client.RemoteModel(sock_path, "pileup", add_indel_length=False, input_channels=18, decoder=False, timeout=DEADLINE)
    m.check_checkpoint(str(a))
    m.check_checkpoint(str(tmp_path / "a"))  # (the reference's loader appends .pt)
    with pytest.raises(client.ServerError, match="another checkpoint"):
        m.check_checkpoint(str(b))
    with pytest.raises(client.ServerError, match="holds no weights"):
        m.load_state_dict({})
    assert m.to("cpu") is m and m.eval() is m
    m.close()
    with pytest.raises(client.ServerError, match="decoder"):
        client.RemoteModel(sock_path, "pileup", decoder=True, timeout=DEADLINE)
    with pytest.raises(client.ServerError, match="add_indel_length"):
        client.RemoteModel(sock_path, "pileup", add_indel_length=True, timeout=DEADLINE)
    with pytest.raises(client.ServerError, match="input_channels"):
        client.RemoteModel(sock_path, "pileup", input_channels=9, timeout=DEADLINE)
    with pytest.raises(client.ServerError, match="no model 'alignment'"):
        client.RemoteModel(sock_path, "alignment", timeout=DEADLINE)


def test_decoder_rows_when_the_server_has_them(sock_path, running):
    running(StandIn(decoder=True))
    m = client.RemoteModel(sock_path, "pileup", decoder=True, timeout=DEADLINE)
    x = windows(2, 3)
    y = m.predict_numpy(x)
    assert y.shape == (2, 55) and np.array_equal(y, rows_of(x, 55))
    m.close()
    with pytest.raises(client.ServerError, match="decoder"):
        client.RemoteModel(sock_path, "pileup", decoder=False, timeout=DEADLINE)


def test_a_segment_smaller_than_the_request_is_refused(sock_path, running):
    """the library writes rows into the segment: its real size is checked, not the client's word"""
    running()
    seg = client.Segment.create(1024)
    try:
        c = client.Connection(sock_path, DEADLINE)
        with pytest.raises(client.ServerError, match="holds 1024 bytes"):
            c.request({"op": "predict", "model": "pileup", "shm": seg.name, "batch": 4, "dtype": "int32", "shape": [4, 33, 18]})
        with pytest.raises(client.ServerError):
            c.request({"op": "predict", "model": "pileup", "shm": "/c3hip-no-such-segment", "batch": 1, "dtype": "int32", "shape": [1, 33, 18]})
        c.close()
    finally:
        seg.close()


# ---------------------------------------------------------------------------------------------- timeouts, shutdown
def test_the_timeout_raises_when_nothing_answers(sock_path, monkeypatch):
    with pytest.raises(client.ServerError, match="cannot connect"):
        client.RemoteModel(sock_path, "pileup", timeout=0.2)
    deaf = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    with client.socket_address(sock_path) as addr:
        deaf.bind(addr)
    deaf.listen(1)  # connects, never answers
    try:
        monkeypatch.setenv("C3HIP_SERVER_TIMEOUT", "0.2")
        t0 = time.monotonic()
        with pytest.raises(client.ServerTimeout, match="C3HIP_SERVER_TIMEOUT"):
            client.RemoteModel(sock_path, "pileup")
        assert time.monotonic() - t0 < 5
    finally:
        deaf.close()
    monkeypatch.setenv("C3HIP_SERVER_TIMEOUT", "soon")
    with pytest.raises(client.ServerError, match="C3HIP_SERVER_TIMEOUT"):
        client.timeout_seconds()
    monkeypatch.delenv("C3HIP_SERVER_TIMEOUT")
    assert client.timeout_seconds() == 120.0


def test_a_short_socket_path_is_used_as_it_is():
    import tempfile
    with tempfile.TemporaryDirectory(prefix="c3", dir="/tmp") as d:
        path = os.path.join(d, "c3.sock")
        with client.socket_address(path) as addr:
            assert addr == path
        s = serve.Server({"pileup": StandIn()}, path, log=lambda text: None).start()
        try:
            m = client.RemoteModel(path, "pileup", timeout=DEADLINE)
            x = windows(2, 4)
            assert np.array_equal(m.predict_numpy(x), rows_of(x, 24))
            m.close()
        finally:
            s.shutdown()
            s.join()
        assert not os.path.exists(path)
    with pytest.raises(client.ServerError, match="socket file name"):
        with client.socket_address("/tmp/" + "n" * 200):
            pass


def test_the_socket_is_gone_after_shutdown(sock_path):
    lines = []
    s = serve.Server({"pileup": StandIn()}, sock_path, log=lines.append).start()
    assert os.path.exists(sock_path) and (os.stat(sock_path).st_mode & 0o077) == 0
    with pytest.raises(client.ServerError, match="already listening"):
        serve.Server({"pileup": StandIn()}, sock_path).start()
    m = client.RemoteModel(sock_path, "pileup", timeout=DEADLINE)
    m.predict_numpy(windows(2, 1))
    client.control(sock_path, "shutdown")
    s.join()
    assert not os.path.exists(sock_path)
    assert len(lines) == 1 and lines[0].startswith("[clair3_amd] serve:") and "pileup: requests=1 passes=1 windows=2 max_parts=1" in lines[0]


# ---------------------------------------------------------------------------------------------- the drop-in
INSTALL = r"""
import json, os, sys
root, ref, sock = sys.argv[1:4]
sys.path[:0] = [root, ref]
from clair3_amd import callvar, client, predict
from clair3_amd.model import Clair3_F, Clair3_P
import clair3.CallVariantsFromCffi as w
import clair3.CallVariants as legacy
import clair3.model as ref_model
plain = callvar.install(lazy_torch=False)
out = {"plain": plain,
       "plain_bindings": [ref_model.Clair3_P is Clair3_P, ref_model.Clair3_F is Clair3_F, w._torch_predict is predict._hip_predict,
                          w._load_torch_checkpoint is predict._load_torch_checkpoint, w._select_device is callvar._select_device_for_cffi_worker,
                          callvar.SERVER is None]}
if sock == "ENV":
    os.environ["C3HIP_SERVER"] = "/tmp/from-env.sock"
    names = callvar.install(lazy_torch=False)
else:
    names = callvar.install(lazy_torch=False, server=sock)
changed = [n for n, a, b in (("clair3.model.Clair3_P", ref_model.Clair3_P, Clair3_P), ("clair3.model.Clair3_F", ref_model.Clair3_F, Clair3_F),
                             ("clair3.CallVariantsFromCffi._torch_predict", w._torch_predict, predict._hip_predict),
                             ("clair3.CallVariantsFromCffi._load_torch_checkpoint", w._load_torch_checkpoint, predict._load_torch_checkpoint),
                             ("clair3.CallVariantsFromCffi._select_device", w._select_device, callvar._select_device_for_cffi_worker),
                             ("clair3.CallVariants._torch_predict", legacy._torch_predict, predict._hip_predict),
                             ("clair3.CallVariants._load_torch_checkpoint", legacy._load_torch_checkpoint, predict._load_torch_checkpoint),
                             ("clair3.CallVariants._select_device", legacy._select_device, callvar._select_device_for_worker)) if a is not b]
out.update(names=names, changed=changed, server=callvar.SERVER)
# with --use_gpu nothing changes: the class names still construct the HIP models (no handle is made before .to(device))
callvar._REMOTE_BRANCH = False
out["gpu_branch_model"] = type(ref_model.Clair3_P(add_indel_length=False, predict=True, input_channels=18)).__name__
out["gpu_branch_module"] = type(ref_model.Clair3_P(add_indel_length=False, predict=True, input_channels=18)).__module__
# without it: _select_device(False) is the opaque CPU device as before, and the class names construct RemoteModels (here: nobody listens)
dev = w._select_device(False)
out["cpu_device"] = str(dev)
try:
    ref_model.Clair3_F(add_indel_length=True, predict=True, input_channels=8)
    out["remote"] = "constructed"
except client.ServerError as e:
    out["remote"] = str(e)
print("RESULT " + json.dumps(out))
"""


@pytest.mark.parametrize("how", ["argument", "ENV"])
def test_install_with_a_server_rebinds_the_same_names(tmp_path, how):
    from tests import refloop
    ref = refloop.reference_root()
    if ref is None:
        pytest.skip("no reference modules staged (oracle/_ref: __graft_entry__.build())")
    sock = str(tmp_path / "nobody.sock")
    env = {k: v for k, v in os.environ.items() if k != "C3HIP_SERVER"}
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests", "stubs")])
    r = subprocess.run([sys.executable, "-c", INSTALL, ROOT, ref, "ENV" if how == "ENV" else sock], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][0][7:])
    assert all(out["plain_bindings"]), "install() without the opt-in binds what it bound before"
    assert out["names"] == out["plain"] and len(out["plain"]) == 14
    assert out["changed"] == ["clair3.model.Clair3_P", "clair3.model.Clair3_F", "clair3.CallVariantsFromCffi._torch_predict",
                              "clair3.CallVariantsFromCffi._load_torch_checkpoint", "clair3.CallVariantsFromCffi._select_device"]
    assert out["server"] == ("/tmp/from-env.sock" if how == "ENV" else sock)
    assert (out["gpu_branch_model"], out["gpu_branch_module"]) == ("Clair3_P", "clair3_amd.model")
    assert out["cpu_device"] == "cpu"
    assert "cannot connect to the clair3_amd server" in out["remote"]
