"""Serve mode: ONE GPU process answers the reference's CPU workers.

    python -m clair3_amd.serve --socket PATH --model pileup=CKPT --model alignment=CKPT [--add_indel_length] [--platform ont|hifi|ilmn]
                               [--enable_dwell_time] [--device N] [--decoder]

The reference's worker reaches a model in three ways (clair3/CallVariantsFromCffi.py:197-297): tensor files on the GPU branch, its own
modules on the CPU branch -- what ``parallel ... CallVariantsFromCffi`` runs, one process per chunk -- and ``--use_triton_gpu``
(:201-214,287-294), where those CPU workers send their batches to one GPU process under the model names ``pileup`` and ``alignment``.
This is the counterpart of the third: N chunk workers, one HIP context, one workspace, one copy of the weights.

What makes it cheap: a window's row is bit-identical whatever batch it travels in, so the requests that are waiting when a
ring slot falls free travel in ONE forward pass -- c3_predict_submit_parts stages every client's windows straight out of that client's
shared-memory segment and c3_predict_wait writes its rows straight back into it.  clair3_amd/client.py states the transport.

``Server`` takes model objects: anything with ``submit_parts(list_of_(windows, rows), slot)`` / ``wait(ticket)`` and the attributes
row_size, output_size, input_channels, add_indel_length (tests/test_serve.py hands it a numpy stand-in; nothing here needs a device).
"""
import argparse
import os
import socket
import sys
import threading
import time
from collections import deque

import numpy as np

from . import client as proto

MAX_PARTS = 64       # C3_MAX_PARTS (include/c3hip.h)
RING_SLOTS = 3       # passes in flight per model: staging of pass k + 1 runs under the kernels of pass k (c3_predict_submit / _wait ring)
GROUP_WINDOWS = {"pileup": 4000, "alignment": 2000}  # the drop-in's group sizes (worker.group_windows_for; C3HIP_PREFETCH_GROUP)


class _Request:
    __slots__ = ("conn", "model", "shm", "batch", "seg", "x", "y")

    def __init__(self, conn, model, shm, batch):
        self.conn, self.model, self.shm, self.batch = conn, model, shm, batch
        self.seg = self.x = self.y = None

    def release(self, unlink=False):
        """drop the mapped arrays, then the mapping; unlink: the client is gone, nobody else removes the name"""
        self.x = self.y = None
        if self.seg is not None:
            seg, self.seg = self.seg, None
            try:
                seg.close()
            except BufferError:  # (a view is still alive somewhere: the mapping goes with it)
                pass
            if unlink:
                seg.unlink()


class _Conn:
    def __init__(self, sock):
        self.sock, self.alive, self.lock = sock, True, threading.Lock()

    def send(self, obj):
        """answer; False when the client has gone (its request is dropped, nobody waits for it)"""
        with self.lock:
            if not self.alive:
                return False
            try:
                proto.send_message(self.sock, obj)
                return True
            except OSError:
                self.alive = False
                return False


class Server:
    def __init__(self, models, socket_path, info=None, group_windows=None, timeout=None, log=None):
        """models: {"pileup": model, "alignment": model} (either or both); info[name]: what ``hello`` adds per model (sha256, path)."""
        unknown = sorted(set(models) - set(proto.MODEL_NAMES))
        if unknown or not models:
            raise proto.ServerError(f"models must be named {proto.MODEL_NAMES}, got {sorted(models)}")
        self.models, self.socket_path = dict(models), socket_path
        self.info = {k: dict(v) for k, v in (info or {}).items()}
        self.group = dict(GROUP_WINDOWS)
        self.group.update(group_windows or {})
        self.timeout = proto.timeout_seconds() if timeout is None else float(timeout)
        self.log = log or (lambda text: print(text, file=sys.stderr, flush=True))
        self.cond = threading.Condition()
        self.queue = {name: deque() for name in self.models}
        self.paused = self.stopping = False
        # seconds: where the server's own time goes, summed per model -- map (a request's segment mapped and checked), stage (submit_parts: the
        # staging copies and the launches), wait (blocked in wait() for the oldest pass), reply (answers sent, segments unmapped)
        self.stats = {name: dict(requests=0, passes=0, windows=0, max_parts=0, dropped=0, errors=0, seconds=dict(map=0.0, stage=0.0, wait=0.0, reply=0.0))
                      for name in self.models}
        self.threads, self.listener = [], None
        self.started = time.time()

    # ---- hello ----
    def describe_model(self, name):
        m = self.models[name]
        geometry = getattr(m, "_geometry", None)
        out = dict(kind=name, row_size=int(m.row_size), output_size=int(m.output_size), input_channels=int(m.input_channels),
                   add_indel_length=bool(m.add_indel_length), decoder=bool(getattr(m, "_decode_cols", False)),
                   geometry=list(geometry) if geometry else None, sha256=None)
        # what answers a batch and what verify mode compares with (model.answer(), model.verify(reference=)): "product" / "fp32" unless asked otherwise
        out.update(answer=getattr(m, "_answer", "product"), verify_reference=getattr(m, "_verify_ref", "fp32"))
        out.update(self.info.get(name, {}))
        return out

    # ---- life cycle ----
    def start(self):
        """bind, listen and start the threads; returns at once (serve_forever() = start() + join())"""
        if os.path.exists(self.socket_path):
            probe = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
            probe.settimeout(1.0)
            try:
                with proto.socket_address(self.socket_path) as addr:
                    probe.connect(addr)
            except OSError:
                os.unlink(self.socket_path)  # (left behind by a server that was killed: nobody listens)
            else:
                raise proto.ServerError(f"{self.socket_path}: a server is already listening")
            finally:
                probe.close()
        self.listener = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        old = os.umask(0o077)  # the socket's file permissions are the authentication
        try:
            with proto.socket_address(self.socket_path) as addr:
                self.listener.bind(addr)
        finally:
            os.umask(old)
        self.listener.listen(128)
        self.listener.settimeout(0.2)
        for name in self.models:
            self._spawn(self._model_loop, name)
        self._spawn(self._accept_loop)
        return self

    def _spawn(self, fn, *args):
        t = threading.Thread(target=fn, args=args, daemon=True)
        t.start()
        self.threads = [u for u in self.threads if u.is_alive()] + [t]

    def shutdown(self):
        with self.cond:
            self.stopping = True
            self.cond.notify_all()

    def join(self):
        """wait for the threads that own the models and the listener, then remove the socket and print the summary line"""
        try:
            for t in list(self.threads):
                while t.is_alive():
                    t.join(0.5)
        finally:
            self.close()

    def close(self):
        self.shutdown()
        if self.listener is not None:
            self.listener.close()
            self.listener = None
            try:
                os.unlink(self.socket_path)
            except FileNotFoundError:
                pass
            self.log(self.summary())

    def serve_forever(self):
        self.start()
        self.join()

    def summary(self):
        parts = []
        for name, st in self.stats.items():
            parts.append("{}: requests={} passes={} windows={} max_parts={} dropped={} errors={}".format(
                name, st["requests"], st["passes"], st["windows"], st["max_parts"], st["dropped"], st["errors"]))
        return "[clair3_amd] serve: {:.1f} s; {}".format(time.time() - self.started, "; ".join(parts))

    # ---- connections ----
    def _accept_loop(self):
        while not self.stopping:
            try:
                sock, _ = self.listener.accept()
            except socket.timeout:
                continue
            except OSError:
                break
            self._spawn(self._conn_loop, _Conn(sock))

    def _recv(self, conn):
        """the next message of a connection: waits for its first byte as long as the server runs (an idle client is no error), for the rest
        of it no longer than the timeout"""
        conn.sock.settimeout(0.2)
        while not self.stopping:
            try:
                first = conn.sock.recv(1, socket.MSG_PEEK)
            except socket.timeout:
                continue
            if not first:
                return None
            conn.sock.settimeout(self.timeout)
            try:
                return proto.recv_message(conn.sock)
            finally:
                conn.sock.settimeout(0.2)
        return None

    def _conn_loop(self, conn):
        try:
            while True:
                msg = self._recv(conn)
                if msg is None:
                    break
                self._handle(conn, msg)
        except (OSError, proto.ServerError):
            pass
        finally:
            with conn.lock:
                conn.alive = False
            conn.sock.close()
            with self.cond:
                self.cond.notify_all()

    def _handle(self, conn, msg):
        op = msg.get("op")
        if op == "hello":
            conn.send(dict(ok=True, models={name: self.describe_model(name) for name in self.models}, max_parts=MAX_PARTS,
                           group_windows={name: self.group[name] for name in self.models}, paused=self.paused))
        elif op == "predict":
            t0 = time.perf_counter()
            try:
                req = self._map_request(conn, msg)
            except (proto.ServerError, OSError, ValueError, TypeError, KeyError) as e:
                conn.send(dict(ok=False, error=f"{type(e).__name__}: {e}"))
                return
            with self.cond:
                if self.stopping:
                    req.release()
                    conn.send(dict(ok=False, error="the server is shutting down"))
                    return
                self.stats[req.model]["requests"] += 1
                self.stats[req.model]["seconds"]["map"] += time.perf_counter() - t0
                self.queue[req.model].append(req)
                self.cond.notify_all()
        elif op == "stats":
            with self.cond:
                conn.send(dict(ok=True, paused=self.paused, stats={k: dict(v, seconds=dict(v["seconds"])) for k, v in self.stats.items()},
                               waiting={k: len(q) for k, q in self.queue.items()},
                               answer={k: getattr(m, "_answer", "product") for k, m in self.models.items()},
                               verify_reference={k: getattr(m, "_verify_ref", "fp32") for k, m in self.models.items()}))
        elif op in ("pause", "resume"):
            with self.cond:
                self.paused = op == "pause"
                self.cond.notify_all()
            conn.send(dict(ok=True, paused=self.paused))
        elif op == "shutdown":
            conn.send(dict(ok=True))
            self.shutdown()
        else:
            conn.send(dict(ok=False, error=f"unknown op {op!r}"))

    def _map_request(self, conn, msg):
        """a predict message -> the request with its segment mapped and checked against the model: every size the library will read or
        write is checked HERE against the segment's real size"""
        name = msg.get("model")
        if name not in self.models:
            raise proto.ServerError(f"no model {name!r} (serving {sorted(self.models)})")
        m = self.models[name]
        dtype = proto.DTYPES.get(msg.get("dtype"))
        if dtype is None:
            raise proto.ServerError(f"dtype must be one of {sorted(proto.DTYPES)}, got {msg.get('dtype')!r}")
        shape = tuple(int(s) for s in msg["shape"])
        batch = int(msg["batch"])
        if not shape or shape[0] != batch or batch < 0 or any(s <= 0 for s in shape[1:]) or len(shape) not in (3, 4):
            raise proto.ServerError(f"bad shape {shape} for a batch of {batch} windows")
        x_bytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        yoff = proto.rows_offset(x_bytes)
        req = _Request(conn, name, msg["shm"], batch)
        req.seg = proto.Segment.attach(msg["shm"], yoff + batch * int(m.row_size) * 4)
        req.x = req.seg.array(dtype, shape, 0)
        req.y = req.seg.array(np.float32, (batch, int(m.row_size)), yoff)
        return req

    # ---- passes ----
    def _take(self, name):
        """the requests of the next pass, in arrival order (called with the lock held): at most MAX_PARTS parts and the group size in
        windows; a request beyond the group size travels alone; a request whose client has gone is dropped.  Never waits for more."""
        q, group, windows = self.queue[name], [], 0
        while q and len(group) < MAX_PARTS:
            req = q[0]
            if not req.conn.alive:
                q.popleft()
                self.stats[name]["dropped"] += 1
                req.release(unlink=True)
                continue
            if group and (windows + req.batch > self.group[name] or req.x.dtype != group[0].x.dtype or req.x.shape[1:] != group[0].x.shape[1:]):
                break
            group.append(q.popleft())
            windows += req.batch
        return group

    def _answer(self, name, group, error=None):
        st, t0 = self.stats[name], time.perf_counter()
        for req in group:
            req.x = req.y = None
            sent = req.conn.send(dict(ok=True) if error is None else dict(ok=False, error=error))
            # unmapped here, on the model's thread: handing the mappings to a thread of their own made every connection's mmap wait for its
            # munmap (profiles/serve_mode.txt)
            req.release(unlink=not sent)  # (a client that has gone removes nothing: its segment's name goes here)
            if not sent:
                with self.cond:
                    st["dropped"] += 1
        st["seconds"]["reply"] += time.perf_counter() - t0  # (written by this model's thread alone)

    def _model_loop(self, name):
        m, inflight, slot = self.models[name], deque(), 0
        while True:
            group = None
            with self.cond:
                while True:
                    if self.queue[name] and len(inflight) < RING_SLOTS and (self.stopping or not self.paused):
                        group = self._take(name)
                        if group:
                            break
                        continue
                    if inflight or (self.stopping and not self.queue[name]):
                        break
                    self.cond.wait(0.5)
                if group is None and not inflight:
                    return
            if group is not None and self.stopping:
                self._answer(name, group, "the server is shutting down")
            elif group is not None:
                t0 = time.perf_counter()
                try:
                    ticket = m.submit_parts([(r.x, r.y) for r in group], slot)
                except Exception as e:  # noqa: BLE001  (a library error answers every part of the pass with its text)
                    with self.cond:
                        self.stats[name]["errors"] += 1
                    self._answer(name, group, f"{type(e).__name__}: {e}")
                    continue
                inflight.append((ticket, group))
                slot = (slot + 1) % RING_SLOTS
                with self.cond:
                    st = self.stats[name]
                    st["passes"] += 1
                    st["seconds"]["stage"] += time.perf_counter() - t0
                    st["windows"] += sum(r.batch for r in group)
                    st["max_parts"] = max(st["max_parts"], len(group))
            else:
                ticket, group = inflight.popleft()
                error, t0 = None, time.perf_counter()
                try:
                    m.wait(ticket)
                except Exception as e:  # noqa: BLE001
                    error = f"{type(e).__name__}: {e}"
                    with self.cond:
                        self.stats[name]["errors"] += 1
                self.stats[name]["seconds"]["wait"] += time.perf_counter() - t0
                ticket = None  # (the ticket holds the rows arrays: they go before the segments are unmapped)
                self._answer(name, group, error)


# ---- the command line ----
def build_models(args):
    """the models of the command line, built where predict.build_model builds them (C3HIP_VERIFY, C3HIP_CALIBRATION, C3HIP_RANGE_GUARD, ...
    are read there), at most one handle per name"""
    from . import predict
    models, info = {}, {}
    for spec in args.model:
        name, eq, path = spec.partition("=")
        if not eq or name not in proto.MODEL_NAMES or not path:
            raise proto.ServerError(f"--model takes pileup=CKPT or alignment=CKPT, got {spec!r}")
        if name in models:
            raise proto.ServerError(f"--model {name} given twice: one handle per model name")
        ckpt = proto.checkpoint_path(path)
        m = predict.build_model(name == "pileup", args.add_indel_length, platform=args.platform, enable_dwell_time=args.enable_dwell_time,
                                device=args.device, chkpnt_fn=path)
        if args.decoder:
            m.decode_columns(True)
        models[name], info[name] = m, dict(sha256=proto.file_sha256(ckpt), checkpoint=os.path.abspath(ckpt), platform=args.platform)
    if len(models) == 2:
        for m in models.values():
            m.sharing(2)
    return models, info


def group_windows_from_env(models):
    from . import worker
    out = {}
    for name, m in models.items():
        g = worker.group_windows_for(m)
        out[name] = g if g > 1 else 1  # (C3HIP_PREFETCH_GROUP=0 / 1: one request per pass)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m clair3_amd.serve", description="one GPU process for the reference's CPU workers")
    ap.add_argument("--socket", required=True)
    ap.add_argument("--model", action="append", required=True, metavar="NAME=CKPT")
    ap.add_argument("--add_indel_length", action="store_true")
    ap.add_argument("--platform", default="ont", choices=("ont", "hifi", "ilmn"))
    ap.add_argument("--enable_dwell_time", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--decoder", action="store_true")
    args = ap.parse_args(argv)
    import signal
    models, info = build_models(args)
    server = Server(models, args.socket, info=info, group_windows=group_windows_from_env(models))
    for sig in (signal.SIGTERM, signal.SIGINT):
        signal.signal(sig, lambda *_: server.shutdown())
    server.start()
    print(f"[clair3_amd] serve: listening on {args.socket} ({', '.join(sorted(models))})", file=sys.stderr, flush=True)
    server.join()
    return 0


if __name__ == "__main__":
    sys.exit(main())
