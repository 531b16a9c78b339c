"""Native HTTP/1.1 wire path (`native/_wire`): parsers under sanitizers,
`exchange` and `LineReader` against scripted sockets, and the RestClient /
watch wiring against the in-repo apiserver — native path and forced
fallback must agree."""

import json
import os
import socket
import subprocess
import sys
import threading
import time

import pytest

_wire = pytest.importorskip("k8s_operator_libs_amd.native._wire")

from k8s_operator_libs_amd.core.apiserver import start_apiserver  # noqa: E402
from k8s_operator_libs_amd.core.cache import CachedClient  # noqa: E402
from k8s_operator_libs_amd.core.errors import ApiError, GoneError  # noqa: E402
from k8s_operator_libs_amd.core.restclient import RestClient  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NATIVE_DIR = os.path.join(REPO, "k8s_operator_libs_amd", "native")
ENV_SWITCH = "K8S_OPERATOR_LIBS_NATIVE_WIRE"


# ---------------------------------------------------------------------------
# parsers: stand-alone program under ASan + UBSan (nothing is preloaded)
# ---------------------------------------------------------------------------

def test_wire_core_selftest_under_sanitizers(tmp_path):
    exe = tmp_path / "wire_core_selftest"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "wire_core_selftest.cpp"),
         "-o", str(exe)],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr
    # the inherited environment stays as it is; the instrumented code is the
    # program itself, so ASan only needs to accept whatever library order
    # that environment gives it
    env = dict(os.environ)
    for name, extra in (
            ("ASAN_OPTIONS", "verify_asan_link_order=0"),
            ("UBSAN_OPTIONS", "halt_on_error=1:print_stacktrace=1")):
        env[name] = ":".join(v for v in (env.get(name), extra) if v)
    run = subprocess.run([str(exe)], capture_output=True, text=True,
                         timeout=120, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout


# ---------------------------------------------------------------------------
# a small socket server that plays one scripted handler per connection
# ---------------------------------------------------------------------------

class ScriptedServer:
    def __init__(self, handlers):
        self._handlers = list(handlers)
        self._listener = socket.socket()
        self._listener.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self._listener.bind(("127.0.0.1", 0))
        self._listener.listen(8)
        self.port = self._listener.getsockname()[1]
        self.url = f"http://127.0.0.1:{self.port}"
        self.accepted = 0
        self.requests = []      # raw request bytes, in arrival order
        self.release = threading.Event()  # handlers that idle wait on this
        self.errors = []
        self._threads = []
        self._accept_thread = threading.Thread(target=self._accept, daemon=True)
        self._accept_thread.start()

    def _accept(self):
        for handler in self._handlers:
            try:
                conn, _ = self._listener.accept()
            except OSError:
                return
            self.accepted += 1
            conn.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            t = threading.Thread(target=self._run, args=(handler, conn),
                                 daemon=True)
            t.start()
            self._threads.append(t)

    def _run(self, handler, conn):
        try:
            handler(self, conn)
        except Exception as exc:  # surfaced by close()
            self.errors.append(exc)
        finally:
            conn.close()

    def read_request(self, conn):
        data = b""
        while b"\r\n\r\n" not in data:
            piece = conn.recv(65536)
            if not piece:
                return None
            data += piece
        head, _, body = data.partition(b"\r\n\r\n")
        length = 0
        for line in head.split(b"\r\n")[1:]:
            name, _, value = line.partition(b":")
            if name.strip().lower() == b"content-length":
                length = int(value)
        while len(body) < length:
            body += conn.recv(65536)
        self.requests.append(head + b"\r\n\r\n" + body)
        return head, body

    def connect(self, timeout=5.0):
        sock = socket.create_connection(("127.0.0.1", self.port),
                                        timeout=timeout)
        sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        return sock

    def close(self):
        self.release.set()
        try:
            self._listener.shutdown(socket.SHUT_RDWR)  # wakes a pending accept
        except OSError:
            pass
        self._listener.close()
        self._accept_thread.join(5)
        for t in self._threads:
            t.join(5)
        assert not self.errors, self.errors


@pytest.fixture
def scripted():
    servers = []

    def make(*handlers):
        srv = ScriptedServer(handlers)
        servers.append(srv)
        return srv

    yield make
    for srv in servers:
        srv.close()


def respond(payload, dribble=False):
    """Handler: read one request, send `payload` (optionally a byte at a
    time), then hold the connection open until the test ends."""
    def handler(srv, conn):
        srv.read_request(conn)
        if dribble:
            for i in range(len(payload)):
                conn.sendall(payload[i:i + 1])
        else:
            conn.sendall(payload)
        srv.release.wait(10)
    return handler


def respond_and_close(payload):
    def handler(srv, conn):
        srv.read_request(conn)
        conn.sendall(payload)
    return handler


HEAD = b"Host: test\r\nContent-Type: application/json\r\n"
BODY = json.dumps({"kind": "Status", "items": list(range(40))}).encode()


def ok(body, extra=b""):
    return (b"HTTP/1.1 200 OK\r\n" + extra + b"Content-Length: "
            + str(len(body)).encode() + b"\r\n\r\n" + body)


# ---------------------------------------------------------------------------
# exchange against scripted bytes
# ---------------------------------------------------------------------------

def test_exchange_sends_one_wellformed_request(scripted):
    srv = scripted(respond(ok(BODY)))
    with srv.connect() as sock:
        status, body, reusable = _wire.exchange(
            sock.fileno(), "PATCH", "/api/v1/nodes/n1?x=1", HEAD,
            '{"a": "é"}', 5.0)
    assert (status, body, reusable) == (200, BODY, True)
    sent = '{"a": "é"}'.encode()
    assert srv.requests == [
        b"PATCH /api/v1/nodes/n1?x=1 HTTP/1.1\r\n" + HEAD
        + b"Content-Length: " + str(len(sent)).encode() + b"\r\n\r\n" + sent
    ]


def test_exchange_get_has_no_content_length(scripted):
    srv = scripted(respond(ok(b"{}")))
    with srv.connect() as sock:
        assert _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 5.0) == (
            200, b"{}", True)
    assert srv.requests == [b"GET /x HTTP/1.1\r\n" + HEAD + b"\r\n"]


def test_exchange_response_one_byte_at_a_time(scripted):
    payload = (b"HTTP/1.1 100 Continue\r\n\r\n"
               + ok(BODY, extra=b"cOnNeCtIoN: keep-alive\r\n"))
    srv = scripted(respond(payload, dribble=True))
    with srv.connect() as sock:
        assert _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 5.0) == (
            200, BODY, True)


def test_exchange_chunked_response_is_decoded(scripted):
    chunks = [BODY[:7], BODY[7:8], BODY[8:]]
    payload = b"HTTP/1.1 201 Created\r\nTransfer-Encoding: chunked\r\n\r\n"
    for c in chunks:
        payload += b"%x;ext=1\r\n" % len(c) + c + b"\r\n"
    payload += b"0\r\nX-Trailer: 1\r\n\r\n"
    srv = scripted(respond(payload, dribble=True), respond(payload))
    for _ in range(2):
        with srv.connect() as sock:
            assert _wire.exchange(sock.fileno(), "POST", "/x", HEAD, b"{}",
                                  5.0) == (201, BODY, True)


def test_exchange_unframed_response_reads_to_eof_and_is_not_reusable(scripted):
    srv = scripted(respond_and_close(b"HTTP/1.1 200 OK\r\n\r\n" + BODY))
    with srv.connect() as sock:
        assert _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 5.0) == (
            200, BODY, False)


def test_exchange_connection_close_is_not_reusable(scripted):
    srv = scripted(respond(ok(BODY, extra=b"Connection: close\r\n")))
    with srv.connect() as sock:
        assert _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 5.0) == (
            200, BODY, False)


def test_exchange_peer_close_mid_body_raises_connection_error(scripted):
    srv = scripted(respond_and_close(
        b"HTTP/1.1 200 OK\r\nContent-Length: 100\r\n\r\n0123456789"))
    with srv.connect() as sock:
        with pytest.raises(ConnectionError):
            _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 5.0)


def test_exchange_peer_close_before_response_raises_connection_error(scripted):
    srv = scripted(respond_and_close(b""))
    with srv.connect() as sock:
        with pytest.raises(ConnectionError):
            _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 5.0)


@pytest.mark.parametrize("payload", [
    b"HTTP/1.1 200 OK\r\nNoColon\r\n\r\n",
    b"HTTP/1.1 200 OK\nContent-Length: 0\n\n",
    b"HTTP/1.1 200 OK\r\nContent-Length: -1\r\n\r\n",
    b"HTTP/1.1 200 OK\r\nContent-Length: 99999999999999999999\r\n\r\n",
    b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\nzz\r\n",
    b"HTTP/1.1 200 OK\r\nX-Pad: " + b"a" * (65 * 1024) + b"\r\n\r\n",
])
def test_exchange_malformed_framing_raises_value_error(scripted, payload):
    srv = scripted(respond(payload))
    with srv.connect() as sock:
        with pytest.raises(ValueError):
            _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 5.0)


def test_exchange_honours_timeout(scripted):
    def silent(srv, conn):
        srv.read_request(conn)
        srv.release.wait(10)

    srv = scripted(silent)
    with srv.connect() as sock:
        t0 = time.monotonic()
        with pytest.raises(TimeoutError):
            _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 0.2)
        elapsed = time.monotonic() - t0
    assert 0.2 <= elapsed < 1.0, elapsed


def test_exchange_never_closes_the_fd(scripted):
    srv = scripted(respond_and_close(b"HTTP/1.1 200 OK\r\n\r\n" + BODY))
    with srv.connect() as sock:
        _wire.exchange(sock.fileno(), "GET", "/x", HEAD, None, 5.0)
        # still a valid descriptor owned by the socket object
        assert sock.getsockname()[1] > 0
        assert os.fstat(sock.fileno())


# ---------------------------------------------------------------------------
# RestClient transport behaviour over scripted bytes
# ---------------------------------------------------------------------------

def test_dead_keepalive_socket_reconnects_exactly_once(scripted):
    closed = threading.Event()

    def serve_one_then_close(srv, conn):
        srv.read_request(conn)
        conn.sendall(ok(b'{"n": 1}'))
        conn.shutdown(socket.SHUT_RDWR)
        closed.set()

    srv = scripted(serve_one_then_close, respond(ok(b'{"n": 2}')),
                   respond(ok(b'{"n": 3}')))
    client = RestClient(srv.url)
    assert client._wire is _wire
    try:
        assert client._fast_request("GET", "/a").json() == {"n": 1}
        assert closed.wait(5)
        assert client._fast_request("GET", "/b").json() == {"n": 2}
        assert srv.accepted == 2
        # the request went out once per connection: not replayed further
        assert [r.split(b" ")[1] for r in srv.requests] == [b"/a", b"/b"]
    finally:
        client.close()


def test_malformed_response_is_a_protocol_error_and_not_resent(scripted):
    import http.client

    srv = scripted(respond(b"HTTP/1.1 200 OK\r\nContent-Length: -1\r\n\r\n"),
                   respond(ok(b"{}")))
    client = RestClient(srv.url, retries=0)
    try:
        with pytest.raises(http.client.HTTPException):
            client._fast_request("POST", "/a", content="{}")
        assert srv.accepted == 1 and len(srv.requests) == 1
        assert getattr(client._fast_local, "sock", None) is None
    finally:
        client.close()


def test_header_block_is_encoded_once_per_client(scripted):
    srv = scripted(respond(ok(b"{}")))
    client = RestClient(srv.url, token="s3cret")
    try:
        client._fast_request("GET", "/a")
        head = client._wire_head()
        assert client._wire_head() is head
        patch_head = client._wire_head(
            {"Content-Type": "application/merge-patch+json"})
        assert client._wire_head(
            {"Content-Type": "application/merge-patch+json"}) is patch_head
        assert b"Authorization: Bearer s3cret\r\n" in srv.requests[0]
        assert f"Host: 127.0.0.1:{srv.port}\r\n".encode() in srv.requests[0]
        assert b"Content-Type: application/merge-patch+json\r\n" in patch_head
        assert b"Content-Type: application/json\r\n" not in patch_head
    finally:
        client.close()


def test_tls_endpoints_never_take_the_native_path():
    client = RestClient("https://127.0.0.1:1", verify=False)
    try:
        assert client._wire is None and client._fast_netloc is None
    finally:
        client.close()


# ---------------------------------------------------------------------------
# native path vs forced fallback against the threaded apiserver
# ---------------------------------------------------------------------------

THING_CRD = {
    "apiVersion": "apiextensions.k8s.io/v1",
    "kind": "CustomResourceDefinition",
    "metadata": {"name": "things.wire.amd.com"},
    "spec": {
        "group": "wire.amd.com", "scope": "Namespaced",
        "names": {"kind": "Thing", "plural": "things", "singular": "thing"},
        "versions": [{
            "name": "v1", "served": True, "storage": True,
            "schema": {"openAPIV3Schema": {
                "type": "object",
                "properties": {"spec": {
                    "type": "object",
                    "properties": {"n": {"type": "integer"}}}},
            }},
        }],
    },
}

_VOLATILE = ("uid", "creationTimestamp")


def _scrub(obj):
    if isinstance(obj, dict):
        return {k: _scrub(v) for k, v in obj.items() if k not in _VOLATILE}
    if isinstance(obj, list):
        return [_scrub(v) for v in obj]
    return obj


def _pod(i):
    return {"apiVersion": "v1", "kind": "Pod",
            "metadata": {"name": f"pod-{i:03d}", "namespace": "default",
                         "labels": {"app": "train", "idx": str(i)},
                         "annotations": {"pad": "x" * 160}},
            "spec": {"nodeName": f"node-{i % 8}",
                     "containers": [{"name": "c", "image": "img:1"}]}}


def _crud_script(client):
    """The same request sequence for either transport; returns the list of
    (status, scrubbed JSON, raw length) it produced."""
    merge = {"Content-Type": "application/merge-patch+json"}
    node = {"apiVersion": "v1", "kind": "Node",
            "metadata": {"name": "n1", "labels": {"a": "1"}}, "spec": {}}
    steps = [
        ("POST", "/api/v1/nodes", dict(content=json.dumps(node))),
        ("GET", "/api/v1/nodes/n1", {}),
        ("PATCH", "/api/v1/nodes/n1", dict(
            content=json.dumps({"metadata": {"labels": {"b": "2"}}}),
            headers=merge)),
        ("GET", "/api/v1/nodes", dict(params={"labelSelector": "b=2"})),
        ("POST", "/api/v1/nodes", dict(content=json.dumps(node))),   # 409
        ("GET", "/api/v1/nodes/missing", {}),                        # 404
        ("DELETE", "/api/v1/nodes/missing", {}),                     # 404
        ("POST", "/apis/wire.amd.com/v1/namespaces/default/things", dict(
            content=json.dumps({
                "apiVersion": "wire.amd.com/v1", "kind": "Thing",
                "metadata": {"name": "t1", "namespace": "default"},
                "spec": {"n": "not-a-number"}}))),                   # 422
    ]
    steps += [("POST", "/api/v1/namespaces/default/pods",
               dict(content=json.dumps(_pod(i)))) for i in range(300)]
    steps += [
        ("GET", "/api/v1/namespaces/default/pods", {}),              # > 64 KiB
        ("GET", "/api/v1/pods", dict(params={"limit": "7"})),
        ("POST", "/api/v1/namespaces/default/pods/pod-000/eviction", dict(
            content=json.dumps({
                "apiVersion": "policy/v1", "kind": "Eviction",
                "metadata": {"name": "pod-000", "namespace": "default"}}))),
        ("GET", "/api/v1/namespaces/default/pods/pod-000", {}),      # 404
        ("DELETE", "/api/v1/namespaces/default/pods/pod-001", dict(
            content=json.dumps({"apiVersion": "v1", "kind": "DeleteOptions",
                                "gracePeriodSeconds": 0}))),
        ("DELETE", "/api/v1/nodes/n1", {}),
        ("GET", "/api/v1/nodes/n1", {}),                             # 404
    ]
    out = []
    for method, path, kw in steps:
        resp = client._request(method, path, **kw)
        out.append((method, path, resp.status_code, _scrub(resp.json()),
                    len(resp.text)))
    return out


def _fresh_server():
    handle = start_apiserver()
    handle.cluster.create(json.loads(json.dumps(THING_CRD)))
    return handle


def test_crud_same_status_and_json_as_forced_fallback(monkeypatch):
    results = {}
    for label in ("native", "fallback"):
        if label == "fallback":
            monkeypatch.setenv(ENV_SWITCH, "0")
        handle = _fresh_server()
        client = RestClient(handle.url)
        try:
            assert (client._wire is _wire) == (label == "native")
            results[label] = _crud_script(client)
        finally:
            client.close()
            handle.stop()
    native, fallback = results["native"], results["fallback"]
    assert len(native) == len(fallback)
    for got, want in zip(native, fallback):
        assert got[:3] == want[:3]
        assert got[3] == want[3], got[:3]
    by_step = {(m, p): (s, j, n) for m, p, s, j, n in native}
    codes = [s for _, _, s, _, _ in native]
    assert {201, 200, 404, 409, 422} <= set(codes)
    status, listing, raw_len = by_step[("GET", "/api/v1/namespaces/default/pods")]
    assert status == 200 and len(listing["items"]) == 300
    assert raw_len > 64 * 1024
    conflict = [j for _, _, s, j, _ in native if s == 409][0]
    assert conflict["reason"] == "AlreadyExists" and conflict["code"] == 409
    invalid = [j for _, _, s, j, _ in native if s == 422][0]
    assert invalid["kind"] == "Status" and "invalid" in invalid["message"]


def test_typed_client_errors_through_native_path():
    from k8s_operator_libs_amd.core.errors import (
        AlreadyExistsError, InvalidError, NotFoundError)

    handle = _fresh_server()
    client = RestClient(handle.url)
    try:
        assert client._wire is _wire
        client.create({"apiVersion": "v1", "kind": "Node",
                       "metadata": {"name": "n1"}, "spec": {}})
        with pytest.raises(AlreadyExistsError):
            client.create({"apiVersion": "v1", "kind": "Node",
                           "metadata": {"name": "n1"}, "spec": {}})
        with pytest.raises(NotFoundError):
            client.get("v1", "Node", "nope")
        with pytest.raises(InvalidError):
            client.create({"apiVersion": "wire.amd.com/v1", "kind": "Thing",
                           "metadata": {"name": "t", "namespace": "default"},
                           "spec": {"n": "x"}})
        client.create(_pod(1))
        client.evict_pod("pod-001", "default")
        with pytest.raises(NotFoundError):
            client.get("v1", "Pod", "pod-001", "default")
    finally:
        client.close()
        handle.stop()


# ---------------------------------------------------------------------------
# LineReader and _HttpWatch
# ---------------------------------------------------------------------------

STREAM_HEAD = b"HTTP/1.1 200 OK\r\nContent-Type: application/json\r\n" \
              b"Connection: close\r\n\r\n"


def stream(head, *pieces, hold=True):
    def handler(srv, conn):
        srv.read_request(conn)
        conn.sendall(head)
        for piece in pieces:
            conn.sendall(piece)
        if hold:
            srv.release.wait(10)
    return handler


def _get(sock, path="/watch"):
    sock.sendall(b"GET " + path.encode() + b" HTTP/1.1\r\nHost: t\r\n\r\n")


def test_linereader_until_close_stream(scripted):
    srv = scripted(stream(
        STREAM_HEAD, b'\n\n{"a":1}\n{"b"', b':2}\r\n\n{"c":3}\n{"tail":4}',
        hold=False))
    with srv.connect() as sock:
        _get(sock)
        lr = _wire.LineReader(sock.fileno())
        assert lr.status is None
        assert lr.readline(5.0) == b'{"a":1}'   # consumes the head first
        assert lr.status == 200 and lr.chunked is False
        assert lr.readline(5.0) == b'{"b":2}'
        assert lr.readline(5.0) == b'{"c":3}'
        assert lr.readline(5.0) == b'{"tail":4}'  # unterminated last line
        with pytest.raises(EOFError):
            lr.readline(5.0)
        with pytest.raises(EOFError):
            lr.readline(5.0)


def test_linereader_chunked_stream_byte_at_a_time(scripted):
    events = [json.dumps({"type": "ADDED", "object": {"i": i}}).encode()
              for i in range(3)]
    body = events[0] + b"\n" + events[1] + b"\n\n" + events[2] + b"\n"
    cuts = [0, 5, len(events[0]) + 3, len(body) - 4, len(body)]
    payload = b"HTTP/1.1 200 OK\r\ntransfer-encoding: chunked\r\n\r\n"
    for a, b in zip(cuts, cuts[1:]):
        payload += b"%X\r\n" % (b - a) + body[a:b] + b"\r\n"
    payload += b"0\r\n\r\n"

    def dribble(srv, conn):
        srv.read_request(conn)
        for i in range(len(payload)):
            conn.sendall(payload[i:i + 1])
        srv.release.wait(10)

    srv = scripted(dribble)
    with srv.connect() as sock:
        _get(sock)
        lr = _wire.LineReader(sock.fileno())
        assert lr.read_head(5.0) == 200
        assert lr.chunked is True
        assert [lr.readline(5.0) for _ in range(3)] == events
        with pytest.raises(EOFError):   # terminating chunk, socket still open
            lr.readline(5.0)


def test_linereader_timeout_returns_none_then_resumes(scripted):
    go = threading.Event()

    def handler(srv, conn):
        srv.read_request(conn)
        conn.sendall(STREAM_HEAD + b'{"par')
        go.wait(10)
        conn.sendall(b'tial":1}\n')
        srv.release.wait(10)

    srv = scripted(handler)
    with srv.connect() as sock:
        _get(sock)
        lr = _wire.LineReader(sock.fileno())
        assert lr.read_head(5.0) == 200
        t0 = time.monotonic()
        assert lr.readline(0.1) is None
        assert 0.1 <= time.monotonic() - t0 < 1.0
        go.set()
        assert lr.readline(5.0) == b'{"partial":1}'


def test_linereader_malformed_chunk_raises_value_error(scripted):
    srv = scripted(stream(
        b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n", b"zz\r\n"))
    with srv.connect() as sock:
        _get(sock)
        lr = _wire.LineReader(sock.fileno())
        with pytest.raises(ValueError):
            lr.readline(5.0)


def test_shutdown_unblocks_a_blocked_readline_within_a_second(scripted):
    srv = scripted(stream(STREAM_HEAD))
    sock = srv.connect()
    try:
        _get(sock)
        lr = _wire.LineReader(sock.fileno())
        assert lr.read_head(5.0) == 200
        entered = threading.Event()
        result = {}

        def blocked():
            entered.set()
            t0 = time.monotonic()
            try:
                result["value"] = lr.readline(5)
            except BaseException as exc:
                result["exc"] = exc
            result["elapsed"] = time.monotonic() - t0

        t = threading.Thread(target=blocked, daemon=True)
        t.start()
        assert entered.wait(5)
        time.sleep(0.1)  # let it reach poll()
        t0 = time.monotonic()
        sock.shutdown(socket.SHUT_RDWR)
        t.join(1.0)
        assert not t.is_alive()
        assert time.monotonic() - t0 < 1.0
        assert isinstance(result.get("exc"), EOFError), result
        assert result["elapsed"] < 2.0
    finally:
        sock.close()  # only after the reader has returned


def test_readline_releases_the_gil(scripted):
    srv = scripted(stream(STREAM_HEAD), stream(STREAM_HEAD))
    socks = [srv.connect(), srv.connect()]
    try:
        readers = []
        for sock in socks:
            _get(sock)
            lr = _wire.LineReader(sock.fileno())
            assert lr.read_head(5.0) == 200
            readers.append(lr)
        barrier = threading.Barrier(3)
        results = []

        def wait(lr):
            barrier.wait(5)
            results.append(lr.readline(0.2))

        threads = [threading.Thread(target=wait, args=(lr,), daemon=True)
                   for lr in readers]
        for t in threads:
            t.start()
        t0 = time.monotonic()  # before any reader can start its deadline
        barrier.wait(5)
        for t in threads:
            t.join(5)
        elapsed = time.monotonic() - t0
        assert results == [None, None]
        # serialised under the GIL the two idle waits would take 0.4 s
        assert 0.2 <= elapsed < 0.35, elapsed
    finally:
        for sock in socks:
            sock.close()


def _node(name, labels=None):
    return {"apiVersion": "v1", "kind": "Node",
            "metadata": {"name": name, "labels": labels or {}}, "spec": {}}


@pytest.fixture(params=["thread", "uvicorn"])
def engine_server(request):
    if request.param == "uvicorn":
        pytest.importorskip("uvicorn")
    handle = start_apiserver(engine=request.param)
    yield handle
    handle.stop()


def test_watch_events_arrive_in_order(engine_server):
    client = RestClient(engine_server.url)
    w = None
    try:
        w = client.watch("v1", "Node")
        assert w._sock is not None and w._resp is None  # native reader
        names = [f"n{i}" for i in range(6)]
        for name in names:
            client.create(_node(name))
        client.patch("v1", "Node", "n0", {"metadata": {"labels": {"z": "1"}}})
        client.delete("v1", "Node", "n1")
        got = []
        while len(got) < 8:
            ev = w.next(5.0)
            assert ev is not None, got
            if ev[0] != "BOOKMARK":
                got.append((ev[0], ev[1]["metadata"]["name"]))
        assert got == [("ADDED", n) for n in names] + [
            ("MODIFIED", "n0"), ("DELETED", "n1")]
        assert w.alive()
        t0 = time.monotonic()
        w.stop()
        w._thread.join(1.0)
        assert not w._thread.is_alive() and time.monotonic() - t0 < 1.0
        assert not w.alive()
    finally:
        if w is not None:
            w.stop()
        client.close()


def test_uvicorn_watch_stream_is_chunked():
    pytest.importorskip("uvicorn")
    handle = start_apiserver(engine="uvicorn")
    try:
        handle.cluster.create(_node("n1"))
        host, port = handle.url[len("http://"):].split(":")
        with socket.create_connection((host, int(port)), timeout=5) as sock:
            _get(sock, "/api/v1/nodes?watch=true&sendInitialEvents=true"
                       "&resourceVersionMatch=NotOlderThan")
            lr = _wire.LineReader(sock.fileno())
            assert lr.read_head(5.0) == 200
            assert lr.chunked is True
            event = json.loads(lr.readline(5.0))
            assert event["type"] == "ADDED"
            assert event["object"]["metadata"]["name"] == "n1"
    finally:
        handle.stop()


def test_in_stream_error_410_passes_through(engine_server):
    client = RestClient(engine_server.url)
    try:
        client.create(_node("w1"))
        client.watch("v1", "Node").stop()   # turns on history
        client.patch("v1", "Node", "w1", {"metadata": {"labels": {"a": "1"}}})
        w = client.watch("v1", "Node", resource_version="1")
        try:
            ev = w.next(5.0)
            assert ev[0] == "ERROR"
            assert ev[1]["code"] == 410 and ev[1]["reason"] == "Expired"
        finally:
            w.stop()
    finally:
        client.close()


def test_http_410_raises_gone_and_other_errors_carry_code(scripted):
    srv = scripted(
        respond_and_close(b"HTTP/1.1 410 Gone\r\nContent-Length: 0\r\n\r\n"),
        respond_and_close(b"HTTP/1.1 403 Forbidden\r\nContent-Length: 2\r\n\r\n{}"),
    )
    client = RestClient(srv.url, token="tok")
    try:
        with pytest.raises(GoneError):
            client.watch("v1", "Node", resource_version="5",
                         label_selector="a=b")
        with pytest.raises(ApiError) as info:
            client.watch("v1", "Node")
        assert info.value.code == 403
        first = srv.requests[0].split(b"\r\n")
        assert first[0] == (b"GET /api/v1/nodes?watch=true&allowWatchBookmarks"
                            b"=true&resourceVersion=5&labelSelector=a%3Db"
                            b" HTTP/1.1")
        assert b"Authorization: Bearer tok" in first
    finally:
        client.close()


def test_bookmark_and_error_events_pass_through_and_drop_ends_alive(scripted):
    events = [
        {"type": "BOOKMARK", "object": {"metadata": {"resourceVersion": "9"}}},
        {"type": "ERROR", "object": {"kind": "Status", "code": 500}},
        {"type": "ADDED", "object": {"metadata": {"name": "n"}}},
    ]
    body = b"".join(json.dumps(e).encode() + b"\n" for e in events)
    srv = scripted(stream(STREAM_HEAD, body, b"not json\n", hold=False))
    client = RestClient(srv.url)
    try:
        w = client.watch("v1", "Node")
        got = [w.next(5.0) for _ in range(3)]
        assert got == [(e["type"], e["object"]) for e in events]
        # the server dropped the stream: alive() goes False by itself
        w._thread.join(5.0)
        assert not w.alive()
        assert w.next(0.01) is None
        w.stop()  # stopping a finished watch is harmless
    finally:
        client.close()


def test_server_drop_makes_informer_rewatch():
    handle = start_apiserver()
    client = RestClient(handle.url)
    cached = CachedClient(client)
    try:
        client.create(_node("w1"))
        assert cached.get("v1", "Node", "w1")
        inf = cached._informers[("v1", "Node")]
        old = inf._watch
        assert old._sock is not None and old.alive()
        # the threaded engine ends every open watch stream while this is set
        handle._server._shutting_down = True
        old._thread.join(5.0)
        handle._server._shutting_down = False
        assert not old.alive()
        client.patch("v1", "Node", "w1", {"metadata": {"labels": {"r": "1"}}})
        deadline = time.monotonic() + 10
        while time.monotonic() < deadline:
            labels = cached.get("v1", "Node", "w1")["metadata"].get("labels", {})
            if labels.get("r") == "1" and inf._watch is not old:
                break
            time.sleep(0.02)
        assert cached.get("v1", "Node", "w1")["metadata"]["labels"]["r"] == "1"
        assert inf._watch is not old and inf._watch.alive()
    finally:
        cached.stop()
        client.close()
        handle.stop()


# ---------------------------------------------------------------------------
# fallback switch
# ---------------------------------------------------------------------------

def _spy_on_wire(monkeypatch):
    """Record every call into the extension made on behalf of a RestClient
    constructed from now on (watch threads that other tests left behind may
    still be re-watching through clients of their own)."""
    calls, ports = [], set()
    real_exchange, real_reader = _wire.exchange, _wire.LineReader
    real_parse = _wire.parse_request_head
    real_init = RestClient.__init__

    def init(self, *args, **kw):
        real_init(self, *args, **kw)
        if self._fast_netloc is not None:
            ports.add(self._fast_netloc[1])

    def record(name, fd):
        peer = socket.socket(fileno=os.dup(fd))
        try:
            port = peer.getpeername()[1]
        finally:
            peer.close()
        if port in ports:
            calls.append(name)

    def exchange(fd, *args):
        record("exchange", fd)
        return real_exchange(fd, *args)

    def line_reader(fd):
        record("LineReader", fd)
        return real_reader(fd)

    def parse_request_head(data):
        # called from a request handler of the threaded apiserver: the one
        # these clients talk to listens on one of `ports`
        handler = sys._getframe(1).f_locals.get("self")
        if handler is None or handler.server.server_address[1] in ports:
            calls.append("parse_request_head")
        return real_parse(data)

    monkeypatch.setattr(RestClient, "__init__", init)
    monkeypatch.setattr(_wire, "parse_request_head", parse_request_head)
    monkeypatch.setattr(_wire, "exchange", exchange)
    monkeypatch.setattr(_wire, "LineReader", line_reader)
    return calls, ports


def _one_cached_upgrade(monkeypatch):
    monkeypatch.syspath_prepend(REPO)
    import bench

    return bench.run_rolling_upgrade_benchmark(
        steps=1, warmup=0, substrate="cached", gpu_validate=False)


def test_disabled_by_environment_never_calls_wire(monkeypatch):
    calls, ports = _spy_on_wire(monkeypatch)
    monkeypatch.setenv(ENV_SWITCH, "0")
    result = _one_cached_upgrade(monkeypatch)
    assert result["upgrades_completed"] == 1
    assert ports and calls == []


def test_enabled_by_default_uses_wire_for_requests_and_watches(monkeypatch):
    calls, _ = _spy_on_wire(monkeypatch)
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    result = _one_cached_upgrade(monkeypatch)
    assert result["upgrades_completed"] == 1
    assert {"exchange", "LineReader", "parse_request_head"} <= set(calls)


def test_missing_extension_falls_back(monkeypatch):
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    monkeypatch.setitem(sys.modules, "k8s_operator_libs_amd.native._wire", None)
    import k8s_operator_libs_amd.native as native_pkg

    monkeypatch.delattr(native_pkg, "_wire", raising=False)
    handle = start_apiserver()
    client = RestClient(handle.url)
    try:
        assert client._wire is None
        client.create(_node("n1"))
        w = client.watch("v1", "Node")
        try:
            assert w._sock is None  # httpx reader
            client.patch("v1", "Node", "n1", {"metadata": {"labels": {"a": "1"}}})
            assert w.next(5.0)[0] == "MODIFIED"
        finally:
            w.stop()
    finally:
        client.close()
        handle.stop()


# ---------------------------------------------------------------------------
# apiserver side: native request-head parse, single-write responses
# ---------------------------------------------------------------------------

def test_parse_request_head():
    head = (b"PATCH /api/v1/nodes/n1?x=1 HTTP/1.1\r\nhOsT: a\r\n"
            b"content-LENGTH:  7 \r\n\r\n")
    assert _wire.parse_request_head(head + b'{"a":1}') == (
        "PATCH", "/api/v1/nodes/n1?x=1", 1, 7, False, True, len(head))
    assert _wire.parse_request_head(bytearray(head)) is not None
    assert _wire.parse_request_head(head[:-1]) is None
    assert _wire.parse_request_head(b"") is None
    assert _wire.parse_request_head(
        b"GET / HTTP/1.0\r\n\r\n") == ("GET", "/", 0, None, False, False, 18)
    assert _wire.parse_request_head(
        b"GET / HTTP/1.1\r\nConnection: close\r\n"
        b"Transfer-Encoding: chunked\r\n\r\n")[3:6] == (None, True, False)
    for bad in (b"GET /\r\n\r\n", b"GET / HTTP/1.1\nHost: a\n\n",
                b"GET / HTTP/1.1\r\nbroken\r\n\r\n",
                b"POST / HTTP/1.1\r\nContent-Length: -1\r\n\r\n",
                b"GET / HTTP/1.1\r\nX: " + b"a" * (65 * 1024)):
        with pytest.raises(ValueError):
            _wire.parse_request_head(bad)


_NODE_BODY = json.dumps(_node("n1", {"a": "1"})).encode()
_RAW_REQUESTS = [
    # (pieces sent one after another, responses expected)
    ([b"GET /api/v1/nodes/missing HTTP/1.1\r\nHost: a\r\n\r\n"], 1),
    ([b"POST /api/v1/nodes HTTP/1.1\r\nHost: a\r\nContent-Length: "
      + str(len(_NODE_BODY)).encode() + b"\r\n\r\n" + _NODE_BODY], 1),
    # head split inside a header line, body in a third piece
    ([b"PATCH /api/v1/nodes/n1 HTTP/1.1\r\nHost: a\r\nContent-Le",
      b"ngth: 36\r\n\r\n", b'{"metadata": {"labels": {"b": "2"}}}'], 1),
    # two pipelined requests in one segment
    ([b"GET /api/v1/nodes/n1 HTTP/1.1\r\nHost: a\r\n\r\n"
      b"GET /api/v1 HTTP/1.1\r\nHost: a\r\n\r\n"], 2),
    ([b"GET /api/v1/nodes HTTP/1.1\r\nhost: a\r\nExpect: 100-continue\r\n\r\n"], 1),
    ([b"BREW /pot HTTP/1.1\r\nHost: a\r\n\r\n"], 1),   # 501, then closed
]


def _read_responses(sock, count):
    """Read `count` Content-Length-framed responses (1xx skipped)."""
    out, data = [], b""
    while len(out) < count:
        while b"\r\n\r\n" not in data:
            piece = sock.recv(65536)
            if not piece:
                return out + [data]
            data += piece
        head, _, rest = data.partition(b"\r\n\r\n")
        if head.startswith(b"HTTP/1.1 100"):
            data = rest
            continue
        length = 0
        for line in head.split(b"\r\n")[1:]:
            name, _, value = line.partition(b":")
            if name.lower() == b"content-length":
                length = int(value)
        while len(rest) < length:
            rest += sock.recv(65536)
        out.append(head + b"\r\n\r\n" + rest[:length])
        data = rest[length:]
    return out


def _raw_session(url):
    import re

    host, port = url[len("http://"):].split(":")
    got = []
    with socket.create_connection((host, int(port)), timeout=5) as sock:
        sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        for pieces, count in _RAW_REQUESTS:
            for piece in pieces:
                sock.sendall(piece)
            got.extend(_read_responses(sock, count))
        assert sock.recv(16) == b""   # the 501 closed the connection
    volatile = re.compile(
        rb'Date: [^\r]*|"uid": "[^"]*"|"creationTimestamp": "[^"]*"')
    return [volatile.sub(b"", r) for r in got]


def test_threaded_apiserver_bytes_same_with_and_without_native_head(monkeypatch):
    sessions = {}
    for label in ("native", "stdlib"):
        if label == "stdlib":
            monkeypatch.setenv(ENV_SWITCH, "0")
        handle = start_apiserver()
        try:
            sessions[label] = _raw_session(handle.url)
        finally:
            handle.stop()
    assert sessions["native"] == sessions["stdlib"]
    firsts = [r.split(b"\r\n")[0] for r in sessions["native"]]
    assert firsts == [
        b"HTTP/1.1 404 Not Found", b"HTTP/1.1 201 Created", b"HTTP/1.1 200 OK",
        b"HTTP/1.1 200 OK", b"HTTP/1.1 200 OK", b"HTTP/1.1 200 OK",
        b"HTTP/1.1 501 Unsupported method ('BREW')"]
    assert b'"labels": {"a": "1", "b": "2"}' in sessions["native"][2]


def test_threaded_apiserver_honours_connection_close_and_http10():
    handle = start_apiserver()
    try:
        host, port = handle.url[len("http://"):].split(":")
        for request in (
                b"GET /api/v1 HTTP/1.1\r\nHost: a\r\nConnection: close\r\n\r\n",
                b"GET /api/v1 HTTP/1.0\r\n\r\n"):
            with socket.create_connection((host, int(port)), timeout=5) as sock:
                sock.sendall(request)
                (resp,) = _read_responses(sock, 1)
                assert resp.startswith(b"HTTP/1.1 200 OK\r\n")
                assert sock.recv(16) == b""   # closed by the server
    finally:
        handle.stop()
