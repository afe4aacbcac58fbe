"""The client side of serve mode (clair3_amd/serve.py): a CPU worker of the reference sends its batches to ONE GPU process.

The reference's authors gave the per-chunk CPU workers of ``parallel ... CallVariantsFromCffi`` a branch that does this with a Triton
server (``--use_triton_gpu``, clair3/CallVariantsFromCffi.py:201-214,287-294); ``RemoteModel`` is what stands in for it here
(callvar.install(server=PATH) puts it behind the unmodified loop's ``_torch_predict``).

This module imports neither ``clair3_amd._lib`` nor torch: a client process never maps a HIP runtime (tests/test_serve.py reads
/proc/self/maps of one).  numpy and the standard library are all it needs.

Transport.  Control: an AF_UNIX stream socket, every message a 4-byte big-endian length and that many bytes of JSON.  Payload: POSIX
shared memory that the CLIENT creates, one segment per request -- the windows at offset 0, the rows region behind them at the next
multiple of 256 bytes; the server maps the segment, its library stages the windows out of it and writes the rows into it.  Every blocking
wait has a timeout: C3HIP_SERVER_TIMEOUT seconds (default 120).
"""
import hashlib
import itertools
import json
import mmap
import os
import socket
import struct

import numpy as np

MAX_MESSAGE = 1 << 20  # control messages are small: anything longer is a framing error, not a request
DTYPES = {"int8": np.dtype(np.int8), "int32": np.dtype(np.int32)}
# the names the reference's Triton branch gives its two models (clair3/CallVariantsFromCffi.py:227,236)
MODEL_NAMES = ("pileup", "alignment")


class ServerError(RuntimeError):
    """the server refused or failed a request, or its answers do not fit what this worker was started with"""


class ServerTimeout(ServerError):
    """nothing answered within C3HIP_SERVER_TIMEOUT seconds"""


def timeout_seconds():
    value = os.environ.get("C3HIP_SERVER_TIMEOUT", "").strip()
    if not value:
        return 120.0
    try:
        t = float(value)
    except ValueError as e:
        raise ServerError(f"C3HIP_SERVER_TIMEOUT must be a number of seconds > 0, got {value!r}") from e
    if not t > 0:
        raise ServerError(f"C3HIP_SERVER_TIMEOUT must be a number of seconds > 0, got {value!r}")
    return t


# ---- framing ----
def pack_message(obj):
    body = json.dumps(obj, separators=(",", ":")).encode()
    if len(body) > MAX_MESSAGE:
        raise ServerError(f"message of {len(body)} bytes: control messages hold at most {MAX_MESSAGE}")
    return struct.pack(">I", len(body)) + body


def send_message(sock, obj):
    sock.sendall(pack_message(obj))


def _recv_exact(sock, n):
    """n bytes, b"" when the peer closed before the first of them; a close inside them is an error"""
    buf = bytearray()
    while len(buf) < n:
        piece = sock.recv(n - len(buf))
        if not piece:
            if not buf:
                return b""
            raise ServerError(f"connection closed inside a message ({len(buf)} of {n} bytes)")
        buf += piece
    return bytes(buf)


def recv_message(sock):
    """the next message, None when the peer has closed the connection between two messages"""
    head = _recv_exact(sock, 4)
    if not head:
        return None
    (n,) = struct.unpack(">I", head)
    if n > MAX_MESSAGE:
        raise ServerError(f"message of {n} bytes announced: control messages hold at most {MAX_MESSAGE}")
    body = _recv_exact(sock, n) if n else b""
    if n and not body:
        raise ServerError("connection closed behind a message header")
    try:
        obj = json.loads(body.decode())
    except (UnicodeDecodeError, ValueError) as e:
        raise ServerError(f"message is not JSON: {e}") from e
    if not isinstance(obj, dict):
        raise ServerError("message is not a JSON object")
    return obj


# ---- POSIX shared memory (shm_open / shm_unlink as the standard library binds them; no resource tracker: the client that creates a segment
# is the one that removes it)
def _posixshmem():
    import _posixshmem
    return _posixshmem


def rows_offset(x_bytes):
    return (int(x_bytes) + 255) & ~255


class Segment:
    """one mapped POSIX shared-memory segment"""

    def __init__(self, name, fd, size, owner):
        self.name, self.size, self.owner = name, size, owner
        try:
            self.map = mmap.mmap(fd, size)
        finally:
            os.close(fd)

    @classmethod
    def create(cls, size):
        size = max(256, int(size))
        for _ in range(16):
            name = f"/c3hip-{os.getpid()}-{next(_COUNTER)}-{os.urandom(4).hex()}"
            try:
                fd = _posixshmem().shm_open(name, os.O_CREAT | os.O_EXCL | os.O_RDWR, mode=0o600)
            except FileExistsError:
                continue
            try:
                os.ftruncate(fd, size)
            except BaseException:
                os.close(fd)
                _posixshmem().shm_unlink(name)
                raise
            return cls(name, fd, size, True)
        raise ServerError("no free shared-memory name")

    @classmethod
    def attach(cls, name, need):
        """map an existing segment; refuses one that is smaller than ``need`` bytes (the library writes rows into it)"""
        if not isinstance(name, str) or not name.startswith("/") or "/" in name[1:] or len(name) > 200:
            raise ServerError(f"bad segment name {name!r}")
        fd = _posixshmem().shm_open(name, os.O_RDWR, mode=0o600)
        try:
            size = os.fstat(fd).st_size
        except BaseException:
            os.close(fd)
            raise
        if size < max(1, need):
            os.close(fd)
            raise ServerError(f"segment {name} holds {size} bytes, the request needs {need}")
        return cls(name, fd, size, False)

    def array(self, dtype, shape, offset):
        n = int(np.prod(shape, dtype=np.int64))
        return np.frombuffer(self.map, dtype=dtype, count=n, offset=offset).reshape(shape)

    def close(self):
        """unmap (every array handed out must be gone); the owner also removes the name"""
        if self.map is not None:
            self.map.close()
            self.map = None
        if self.owner:
            self.unlink()

    def unlink(self):
        try:
            _posixshmem().shm_unlink(self.name)
        except FileNotFoundError:
            pass
        self.owner = False


_COUNTER = itertools.count()


def file_sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for piece in iter(lambda: f.read(1 << 20), b""):
            h.update(piece)
    return h.hexdigest()


def checkpoint_path(path):
    """the file the reference's loader opens for --chkpnt_fn (clair3/CallVariantsFromCffi.py:20-22)"""
    return path if path.endswith(".pt") else path + ".pt"


class socket_address:
    """``with socket_address(path) as addr: sock.bind(addr) / sock.connect(addr)``.  An AF_UNIX address holds 107 bytes, a job's scratch
    directory is often deeper than that: such a path is reached through its directory's descriptor (/proc/self/fd/N/<name>), whatever its length"""
    LIMIT = 100

    def __init__(self, path):
        self.path, self.fd = path, None

    def __enter__(self):
        if len(os.fsencode(self.path)) <= self.LIMIT:
            return self.path
        directory, name = os.path.split(os.path.abspath(self.path))
        if len(os.fsencode(name)) > self.LIMIT - 32:
            raise ServerError(f"socket file name of {len(os.fsencode(name))} bytes: {name!r}")
        self.fd = os.open(directory, os.O_RDONLY | os.O_DIRECTORY)
        return f"/proc/self/fd/{self.fd}/{name}"

    def __exit__(self, *exc):
        if self.fd is not None:
            os.close(self.fd)
            self.fd = None
        return False


class Connection:
    """one control connection; request() is one message out, one answer in"""

    def __init__(self, path, timeout=None):
        self.path, self.timeout = path, timeout_seconds() if timeout is None else float(timeout)
        self.sock = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        self.sock.settimeout(self.timeout)
        try:
            with socket_address(path) as addr:
                self.sock.connect(addr)
        except socket.timeout as e:
            self.sock.close()
            raise ServerTimeout(f"{path}: no connection within {self.timeout:g} s") from e
        except OSError as e:
            self.sock.close()
            raise ServerError(f"{path}: cannot connect to the clair3_amd server ({e})") from e

    def send(self, obj):
        try:
            send_message(self.sock, obj)
        except socket.timeout as e:
            self.close()
            raise ServerTimeout(f"{self.path}: {obj.get('op')!r} not sent within {self.timeout:g} s (C3HIP_SERVER_TIMEOUT)") from e
        except (OSError, AttributeError) as e:
            self.close()
            raise ServerError(f"{self.path}: {obj.get('op')!r} failed: {e}") from e

    def receive(self, op):
        try:
            answer = recv_message(self.sock)
        except socket.timeout as e:
            self.close()
            raise ServerTimeout(f"{self.path}: no answer to {op!r} within {self.timeout:g} s (C3HIP_SERVER_TIMEOUT)") from e
        except (OSError, AttributeError) as e:
            self.close()
            raise ServerError(f"{self.path}: {op!r} failed: {e}") from e
        if answer is None:
            self.close()
            raise ServerError(f"{self.path}: the server closed the connection before it answered {op!r}")
        if not answer.get("ok"):
            raise ServerError(f"{self.path}: {op}: {answer.get('error', 'refused')}")
        return answer

    def request(self, obj):
        self.send(obj)
        return self.receive(obj.get("op"))

    def close(self):
        if self.sock is not None:
            try:
                self.sock.close()
            finally:
                self.sock = None


def control(path, op, timeout=None, **fields):
    """one control message on a connection of its own: hello, stats, pause, resume, shutdown"""
    c = Connection(path, timeout)
    try:
        return c.request(dict(op=op, **fields))
    finally:
        c.close()


class RemoteModel:
    """The model of a worker whose forward pass runs in the server behind ``socket_path``: predict_numpy(X), and the surface of the
    reference's module that its worker touches (to, eval, __call__; load_state_dict is refused -- the weights are the server's)."""

    def __init__(self, socket_path, name, add_indel_length=None, input_channels=None, decoder=None, timeout=None, **_ignored):
        if name not in MODEL_NAMES:
            raise ServerError(f"model name must be one of {MODEL_NAMES}, got {name!r}")
        self.socket_path, self.name = socket_path, name
        self._conn = Connection(socket_path, timeout)
        hello = self._conn.request({"op": "hello"})
        info = (hello.get("models") or {}).get(name)
        if info is None:
            raise ServerError(f"{socket_path}: the server has no model {name!r} (it serves {sorted(hello.get('models') or {})})")
        self.info = info
        self.row_size, self.output_size = int(info["row_size"]), int(info["output_size"])
        for key, want in (("add_indel_length", add_indel_length), ("input_channels", input_channels), ("decoder", decoder)):
            if want is not None and type(info[key])(want) != info[key]:
                raise ServerError(f"{socket_path}: model {name!r} was started with {key}={info[key]!r}, this worker asks for {want!r}")

    # ---- the reference module's surface ----
    def to(self, device):
        return self

    def eval(self):
        return self

    def load_state_dict(self, state_dict, strict=True):
        raise ServerError("a RemoteModel holds no weights: the checkpoint is loaded by the server (its sha256 is compared with --chkpnt_fn)")

    def __call__(self, x):
        return self.predict_numpy(np.asarray(x))

    def check_checkpoint(self, path):
        """raise unless the file behind --chkpnt_fn is byte for byte the one the server loaded"""
        mine = file_sha256(checkpoint_path(path))
        if mine != self.info.get("sha256"):
            raise ServerError(f"{self.socket_path}: model {self.name!r} was loaded from another checkpoint "
                              f"(sha256 {str(self.info.get('sha256'))[:12]}..., {checkpoint_path(path)} has {mine[:12]}...)")

    def send(self, x):
        """first half of predict_numpy: the windows in a fresh segment and the request on its way; returns what receive() takes"""
        x = np.ascontiguousarray(x)
        dtype = next((k for k, v in DTYPES.items() if v == x.dtype), None)
        if dtype is None:
            raise ServerError(f"unsupported window dtype {x.dtype} (int8 / int32 expected)")
        n = int(x.shape[0])
        yoff, ybytes = rows_offset(x.nbytes), n * self.row_size * 4
        seg = Segment.create(yoff + ybytes)
        try:
            if x.nbytes:
                seg.array(x.dtype, x.shape, 0)[...] = x
            self._conn.send({"op": "predict", "model": self.name, "shm": seg.name, "batch": n, "dtype": dtype, "shape": list(x.shape)})
        except BaseException:
            seg.close()
            raise
        return seg, n, yoff

    def receive(self, pending):
        """second half: wait for the answer (no longer than the timeout) and take the rows out of the segment, which is removed"""
        seg, n, yoff = pending
        try:
            self._conn.receive("predict")
            return seg.array(np.float32, (n, self.row_size), yoff).copy()
        finally:
            seg.close()

    def predict_numpy(self, x):
        return self.receive(self.send(x))

    def close(self):
        self._conn.close()
