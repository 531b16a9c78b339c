"""`RestClient` over `_wire.Pool`: keep-alive connections shared between
threads, against a byte server of this file's own.  The pool lends an fd to
one `_wire.exchange` at a time, so what a request sends and what a response
means stay exactly what the thread-local path makes of them."""

import http.client
import json
import os
import socket
import threading
import types

import pytest

from k8s_operator_libs_amd.core import restclient
from k8s_operator_libs_amd.core.restclient import RestClient
from k8s_operator_libs_amd.native import _wire

ENV_SWITCH = "K8S_OPERATOR_LIBS_NATIVE_WIRE"
HEAD = b"Host: test\r\n"


def ok(body, extra=b""):
    return (b"HTTP/1.1 200 OK\r\n" + extra + b"Content-Length: "
            + str(len(body)).encode() + b"\r\n\r\n" + body)


BODY = json.dumps({"kind": "Status", "items": list(range(40))}).encode()
CHUNKED = (b"HTTP/1.1 201 Created\r\nTransfer-Encoding: chunked\r\n\r\n"
           b"7;ext=1\r\n" + BODY[:7] + b"\r\n1\r\n" + BODY[7:8] + b"\r\n"
           + b"%x ; x\r\n" % len(BODY[8:]) + BODY[8:] + b"\r\n"
           b"0\r\nX-Trailer: 1\r\n\r\n")

#: (name, method, response bytes): the framings a response can have
CORPUS = [
    ("content-length", "GET", ok(BODY)),
    ("chunked", "POST", CHUNKED),
    ("204", "DELETE", b"HTTP/1.1 204 No Content\r\n\r\n"),
    ("304", "GET", b"HTTP/1.1 304 Not Modified\r\nContent-Length: 9\r\n\r\n"),
    ("head", "HEAD", b"HTTP/1.1 200 OK\r\nContent-Length: 9\r\n\r\n"),
    ("100-continue", "PUT", b"HTTP/1.1 100 Continue\r\n\r\n" + ok(BODY)),
    ("connection-close", "GET", ok(BODY, b"Connection: close\r\n")),
]
CLOSE = object()   # script step: close the connection without an answer


class ByteServer:
    """Answers each request on each connection by ``answer(path)``: bytes
    to send, or CLOSE.  Counts accepts and records request paths."""

    def __init__(self, answer):
        self._answer = answer
        self._listener = socket.socket()
        self._listener.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self._listener.bind(("127.0.0.1", 0))
        self._listener.listen(32)
        self.port = self._listener.getsockname()[1]
        self.url = f"http://127.0.0.1:{self.port}"
        self.accepted = 0
        self.paths = []
        self.raw = []           # whole requests, head and body
        self.closed_by_server = threading.Semaphore(0)
        self._lock = threading.Lock()
        self._conns = []
        self._threads = [threading.Thread(target=self._accept, daemon=True)]
        self._threads[0].start()

    def _accept(self):
        while True:
            try:
                conn, _ = self._listener.accept()
            except OSError:
                return
            conn.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            with self._lock:
                self.accepted += 1
                self._conns.append(conn)
            t = threading.Thread(target=self._serve, args=(conn,), daemon=True)
            t.start()
            self._threads.append(t)

    def _serve(self, conn):
        data = b""
        try:
            while True:
                while b"\r\n\r\n" not in data:
                    piece = conn.recv(65536)
                    if not piece:
                        return
                    data += piece
                head, _, data = data.partition(b"\r\n\r\n")
                length = 0
                for line in head.split(b"\r\n")[1:]:
                    name, _, value = line.partition(b":")
                    if name.strip().lower() == b"content-length":
                        length = int(value)
                while len(data) < length:
                    data += conn.recv(65536)
                path = head.split(b" ")[1].decode()
                with self._lock:
                    self.paths.append(path)
                    self.raw.append(head + b"\r\n\r\n" + data[:length])
                data = data[length:]
                reply = self._answer(path)
                if reply is CLOSE:
                    return
                conn.sendall(reply)
                if b"Connection: close" in reply:
                    return
        except OSError:
            pass
        finally:
            conn.close()
            self.closed_by_server.release()

    def close(self):
        try:
            self._listener.shutdown(socket.SHUT_RDWR)
        except OSError:
            pass
        self._listener.close()
        with self._lock:
            conns = list(self._conns)
        for conn in conns:
            try:
                conn.shutdown(socket.SHUT_RDWR)
            except OSError:
                pass
        for t in self._threads:
            t.join(5)


@pytest.fixture
def serve():
    servers = []

    def make(answer=lambda path: ok(b"{}")):
        srv = ByteServer(answer)
        servers.append(srv)
        return srv

    yield make
    for srv in servers:
        srv.close()


def in_thread(fn):
    box = []
    t = threading.Thread(target=lambda: box.append(fn()))
    t.start()
    t.join(10)
    assert box, "the thread did not finish"
    return box[0]


# ---------------------------------------------------------------------------
# what the pool is for
# ---------------------------------------------------------------------------

def _sixteen_short_lived_threads(client):
    for i in range(16):
        assert in_thread(lambda: [
            client._fast_request("GET", f"/t{i}/{j}").status_code
            for j in range(3)]) == [200, 200, 200]


def test_short_lived_threads_share_one_connection(serve):
    srv = serve()
    client = RestClient(srv.url)
    try:
        _sixteen_short_lived_threads(client)
        assert srv.accepted == 1
        stats = client._pool.stats()
        assert (stats["dials"], stats["reuses"], stats["idle"]) == (1, 47, 1)
        assert len(srv.paths) == 48
    finally:
        client.close()


def test_without_the_pool_every_thread_dials(serve, monkeypatch):
    monkeypatch.setattr(RestClient, "USE_POOL", False)
    srv = serve()
    client = RestClient(srv.url)
    try:
        _sixteen_short_lived_threads(client)
        assert srv.accepted == 16
        assert client._pool.stats()["dials"] == 0
    finally:
        client.close()


def test_max_idle_covers_the_concurrent_users(serve):
    from k8s_operator_libs_amd.upgrade.common_manager import (
        CommonUpgradeManager)
    from k8s_operator_libs_amd.upgrade.drain_manager import DrainManager
    from k8s_operator_libs_amd.upgrade.pod_manager import PodManager

    client = RestClient(serve().url)
    try:
        assert client._pool.max_idle == (
            1 + PodManager.MAX_CONCURRENT_NODE_WORKERS
            + DrainManager.MAX_CONCURRENT_NODE_WORKERS
            + CommonUpgradeManager.MAX_PARALLEL_NODE_OPS)
    finally:
        client.close()


def test_concurrent_threads_get_a_connection_each_and_leave_them_idle(serve):
    gate = threading.Barrier(4)

    def answer(path):
        if path.startswith("/gate"):
            gate.wait(5)   # all four requests are in flight at once
        return ok(b"{}")

    srv = serve(answer)
    client = RestClient(srv.url)
    try:
        threads = [threading.Thread(
            target=client._fast_request, args=("GET", f"/gate{i}"))
            for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(10)
        assert srv.accepted == 4
        assert client._pool.stats()["idle"] == 4
        for i in range(8):
            client._fast_request("GET", f"/after{i}")
        assert srv.accepted == 4
    finally:
        client.close()


# ---------------------------------------------------------------------------
# same bytes, same meaning
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,method,payload", CORPUS,
                         ids=[c[0] for c in CORPUS])
def test_exchange_on_a_pooled_fd_equals_exchange_on_a_socket(
        serve, name, method, payload):
    srv = serve(lambda path: payload)
    body = b"{}" if method in ("POST", "PUT") else None
    with socket.create_connection(("127.0.0.1", srv.port), timeout=5) as sock:
        plain = _wire.exchange(sock.fileno(), method, "/x", HEAD, body, 5.0)
    pool = _wire.Pool("127.0.0.1", srv.port, max_idle=2, connect_timeout=5.0)
    try:
        fd, reused = pool.checkout()
        assert not reused
        pooled = _wire.exchange(fd, method, "/x", HEAD, body, 5.0)
        pool.checkin(fd, pooled[2])
        assert pooled == plain
        assert pool.stats()["idle"] == (1 if plain[2] else 0)
    finally:
        pool.close()
    # and through the client, pool on and off
    results = []
    for use_pool in (True, False):
        client = RestClient(srv.url)
        client.USE_POOL = use_pool
        try:
            resp = client._fast_request(method, "/x", content=body)
            results.append((resp.status_code, resp._data))
        finally:
            client.close()
    assert results[0] == results[1] == plain[:2]


def test_request_bytes_are_the_same_with_and_without_the_pool(serve):
    seen = []
    for use_pool in (True, False):
        srv = serve()
        client = RestClient(srv.url, token="t0k")
        client.USE_POOL = use_pool
        try:
            client._fast_request("PATCH", "/api/v1/nodes/n1",
                                 params={"a": "b c"}, content='{"x": "é"}',
                                 headers={"Content-Type":
                                          "application/merge-patch+json"})
        finally:
            client.close()
        assert len(srv.raw) == 1
        seen.append(srv.raw[0].replace(str(srv.port).encode(), b"PORT"))
    assert seen[0] == seen[1]
    assert seen[0].startswith(b"PATCH /api/v1/nodes/n1?a=b+c HTTP/1.1\r\n")
    assert seen[0].endswith('{"x": "é"}'.encode())


# ---------------------------------------------------------------------------
# dead connections and errors
# ---------------------------------------------------------------------------

def test_dead_idle_connection_is_found_before_the_request_is_written(serve):
    srv = serve(lambda path: ok(b"{}", b"X-Bye: 1\r\n") if path != "/a"
                else ok(b'{"n": 1}'))
    client = RestClient(srv.url)
    try:
        assert client._fast_request("GET", "/a").json() == {"n": 1}
        # the server drops the idle keep-alive connection
        with srv._lock:
            srv._conns[0].shutdown(socket.SHUT_RDWR)
        assert srv.closed_by_server.acquire(timeout=5)
        assert client._fast_request("GET", "/b").status_code == 200
        stats = client._pool.stats()
        assert (stats["dials"], stats["stale_discards"], stats["reuses"]) == (
            2, 1, 0)
        assert srv.accepted == 2
        assert srv.paths == ["/a", "/b"]   # one redial, no replay
    finally:
        client.close()


def test_reused_connection_reset_after_the_write_is_redialled_once(serve):
    def answer(path):
        # the first /b is read and dropped unanswered; the second is served
        if path == "/b" and srv.paths.count("/b") == 1:
            return CLOSE
        return ok(b"{}")

    srv = serve(answer)
    client = RestClient(srv.url, retries=0)
    try:
        client._fast_request("GET", "/a")
        assert client._fast_request("GET", "/b").status_code == 200
        assert srv.accepted == 2
        assert srv.paths == ["/a", "/b", "/b"]
        assert client._pool.stats()["dials"] == 2
    finally:
        client.close()


def test_fresh_connection_that_fails_is_not_retried(serve):
    srv = serve(lambda path: CLOSE)
    client = RestClient(srv.url, retries=0)
    try:
        with pytest.raises(ConnectionError):
            client._fast_request("GET", "/a")
        assert srv.accepted == 1 and srv.paths == ["/a"]
        assert client._pool.stats()["idle"] == 0
    finally:
        client.close()


def test_malformed_response_is_a_protocol_error_and_not_resent(serve):
    srv = serve(lambda path: b"HTTP/1.1 200 OK\r\nContent-Length: -1\r\n\r\n"
                if path == "/bad" else ok(b"{}"))
    client = RestClient(srv.url, retries=0)
    try:
        client._fast_request("GET", "/warm")   # so that /bad reuses an fd
        with pytest.raises(http.client.HTTPException):
            client._fast_request("POST", "/bad", content="{}")
        assert srv.paths == ["/warm", "/bad"] and srv.accepted == 1
        assert client._pool.stats()["idle"] == 0   # closed, not pooled
        assert client._fast_request("GET", "/again").status_code == 200
        assert srv.accepted == 2
    finally:
        client.close()


def test_timeout_closes_the_connection_and_the_pool_stays_usable(serve):
    release = threading.Event()

    def answer(path):
        if path == "/stall":
            release.wait(5)
        return ok(b"{}")

    srv = serve(answer)
    client = RestClient(srv.url, timeout=0.2, retries=0)
    try:
        with pytest.raises(TimeoutError):
            client._fast_request("GET", "/stall")
        assert client._pool.stats()["idle"] == 0
        release.set()
        assert client._fast_request("GET", "/ok").status_code == 200
        assert srv.accepted == 2
    finally:
        release.set()
        client.close()


def test_refused_dial_surfaces_as_the_connection_error_it_is():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    pool = _wire.Pool("127.0.0.1", port, max_idle=1, connect_timeout=2.0)
    with pytest.raises(ConnectionRefusedError):
        pool.checkout()
    assert pool.stats() == {"dials": 0, "reuses": 0, "stale_discards": 0,
                            "idle": 0}


# ---------------------------------------------------------------------------
# close, fork
# ---------------------------------------------------------------------------

def test_pool_close_with_one_fd_checked_out(serve):
    srv = serve()
    pool = _wire.Pool("127.0.0.1", srv.port, max_idle=4, connect_timeout=5.0)
    a, _ = pool.checkout()
    b, _ = pool.checkout()
    pool.checkin(a, True)
    pool.close()
    assert pool.closed and pool.stats()["idle"] == 0
    # the lent fd still works and is closed when it comes back
    assert _wire.exchange(b, "GET", "/x", HEAD, None, 5.0)[0] == 200
    pool.checkin(b, True)
    with pytest.raises(OSError):
        os.fstat(b)
    with pytest.raises(RuntimeError):
        pool.checkout()


def test_client_close_closes_the_pool_and_the_client_still_works(serve):
    srv = serve()
    client = RestClient(srv.url)
    client._fast_request("GET", "/a")
    pool = client._pool
    client.close()
    assert pool.closed and client._pool is None
    assert srv.closed_by_server.acquire(timeout=5)   # the server saw it close
    # as before the pool: a closed client dials again when it is used again
    try:
        assert client._fast_request("GET", "/b").status_code == 200
        assert srv.accepted == 2
    finally:
        client.close()


@pytest.mark.skipif(not hasattr(os, "fork"), reason="needs fork")
def test_forked_child_starts_with_an_empty_pool(serve):
    srv = serve()
    pool = _wire.Pool("127.0.0.1", srv.port, max_idle=4, connect_timeout=5.0)
    try:
        fd, _ = pool.checkout()
        _wire.exchange(fd, "GET", "/x", HEAD, None, 5.0)
        pool.checkin(fd, True)
        assert pool.stats()["idle"] == 1
        pid = os.fork()
        if pid == 0:
            code = 1
            try:
                empty = pool.stats()["idle"] == 0
                try:
                    os.fstat(fd)
                    gone = False
                except OSError:
                    gone = True
                code = 0 if empty and gone else 1
            finally:
                os._exit(code)
        assert os.waitpid(pid, 0)[1] == 0
        # the parent's connection is not the child's to close
        fd2, reused = pool.checkout()
        assert reused and fd2 == fd
        assert _wire.exchange(fd2, "GET", "/y", HEAD, None, 5.0)[0] == 200
        pool.checkin(fd2, True)
        assert srv.accepted == 1
    finally:
        pool.close()


# ---------------------------------------------------------------------------
# fallbacks: each one is the thread-local path
# ---------------------------------------------------------------------------

def _uses_thread_local_socket(client):
    client._fast_request("GET", "/a")
    return getattr(client._fast_local, "sock", None) is not None


def test_pool_is_the_default(serve):
    client = RestClient(serve().url)
    try:
        assert client._pool is not None
        assert not _uses_thread_local_socket(client)
        assert client._pool.stats()["dials"] == 1
    finally:
        client.close()


def test_class_switch_falls_back(serve, monkeypatch):
    monkeypatch.setattr(RestClient, "USE_POOL", False)
    client = RestClient(serve().url)
    try:
        assert _uses_thread_local_socket(client)
    finally:
        client.close()


def test_environment_switch_falls_back(serve, monkeypatch):
    monkeypatch.setenv(ENV_SWITCH, "0")
    client = RestClient(serve().url)
    try:
        assert client._wire is None and client._pool is None
        assert client._fast_request("GET", "/a").status_code == 200
        assert getattr(client._fast_local, "conn", None) is not None
    finally:
        client.close()


def test_extension_without_pool_falls_back(serve, monkeypatch):
    older = types.SimpleNamespace(**{
        name: getattr(_wire, name)
        for name in ("exchange", "LineReader", "LinePump", "StreamWriter",
                     "parse_request_head")})
    monkeypatch.setattr(restclient, "_load_wire", lambda: older)
    client = RestClient(serve().url)
    try:
        assert client._wire is older and client._pool is None
        assert _uses_thread_local_socket(client)
    finally:
        client.close()

