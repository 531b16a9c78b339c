"""Native watch-event path: `_wire.StreamWriter` fan-out on the server,
`_wire.LinePump` and drain-on-read in the informer on the client.

The Python-free core runs stand-alone under sanitizers; the two classes run
against plain sockets; the wiring runs against the in-repo apiserver, where
the native path and the forced fallback must put the same bytes on the wire
and keep the same cache."""

import json
import os
import socket
import subprocess
import threading
import time
import types

import pytest

_wire = pytest.importorskip("k8s_operator_libs_amd.native._wire")

import k8s_operator_libs_amd.native as native_pkg  # noqa: E402
from k8s_operator_libs_amd.core import apiserver, cache, restclient  # noqa: E402
from k8s_operator_libs_amd.core.apiserver import start_apiserver  # noqa: E402
from k8s_operator_libs_amd.core.cache import CachedClient  # noqa: E402
from k8s_operator_libs_amd.core.fakecluster import FakeCluster  # noqa: E402
from k8s_operator_libs_amd.core.restclient import RestClient  # noqa: E402

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NATIVE_DIR = os.path.join(REPO, "k8s_operator_libs_amd", "native")
ENV_SWITCH = "K8S_OPERATOR_LIBS_NATIVE_WIRE"
NEVER = 2 ** 64 - 1

STREAM_HEAD = (b"HTTP/1.1 200 OK\r\nContent-Type: application/json\r\n"
               b"Connection: close\r\n\r\n")
CHUNKED_HEAD = (b"HTTP/1.1 200 OK\r\nContent-Type: application/json\r\n"
                b"Transfer-Encoding: chunked\r\n\r\n")


def _node(name, **labels):
    return {"apiVersion": "v1", "kind": "Node",
            "metadata": {"name": name, "labels": dict(labels)}}


def _until(cond, timeout=5.0):
    deadline = time.monotonic() + timeout
    while time.monotonic() < deadline:
        if cond():
            return True
        time.sleep(0.005)
    return cond()


# ---------------------------------------------------------------------------
# 1. the core, stand-alone, under ASan + UBSan and under TSan
# ---------------------------------------------------------------------------

def _no_address_randomisation():
    """Runs in the child, before the selftest is started: load it at fixed
    addresses.  The ThreadSanitizer runtime of GCC 11 knows where a process
    may have its mappings and gives up at start-up ("unexpected memory
    mapping") on hosts that randomise addresses over more bits than it
    allows for.  The checks themselves are not affected."""
    import ctypes

    ADDR_NO_RANDOMIZE = 0x0040000
    ctypes.CDLL(None).personality(ADDR_NO_RANDOMIZE)


def test_wire_stream_selftest_under_sanitizers(tmp_path):
    source = os.path.join(REPO, "tests", "native", "wire_stream_selftest.cpp")
    env = dict(os.environ)
    for name, extra in (
            ("ASAN_OPTIONS", "verify_asan_link_order=0"),
            ("UBSAN_OPTIONS", "halt_on_error=1:print_stacktrace=1"),
            ("TSAN_OPTIONS", "halt_on_error=1")):
        env[name] = ":".join(v for v in (env.get(name), extra) if v)
    for tag, flag in (("asan", "-fsanitize=address,undefined"),
                      ("tsan", "-fsanitize=thread")):
        exe = tmp_path / f"wire_stream_selftest_{tag}"
        build = subprocess.run(
            ["g++", "-std=c++17", "-O1", "-g", "-pthread", flag,
             f"-I{NATIVE_DIR}", source, "-o", str(exe)],
            capture_output=True, text=True, timeout=300,
        )
        assert build.returncode == 0, build.stderr
        # the instrumented code is the program itself: nothing is preloaded
        run = subprocess.run([str(exe)], capture_output=True, text=True,
                             timeout=120, env=env,
                             preexec_fn=_no_address_randomisation)
        assert run.returncode == 0, tag + "\n" + run.stdout + run.stderr
        assert "checks passed" in run.stdout


# ---------------------------------------------------------------------------
# 2. LinePump: framing and lifecycle over a socket pair
# ---------------------------------------------------------------------------

@pytest.fixture
def pair():
    ours, peer = socket.socketpair()
    pumps = []

    def make():
        pump = _wire.LinePump(ours.fileno())
        pumps.append(pump)
        return pump

    yield ours, peer, make
    try:
        ours.shutdown(socket.SHUT_RDWR)
    except OSError:
        pass
    for pump in pumps:
        pump.stop()
    ours.close()
    peer.close()


def _collect(pump, count, timeout=5.0):
    got = []
    deadline = time.monotonic() + timeout
    while len(got) < count and time.monotonic() < deadline:
        seen = pump.seq
        got.extend(pump.drain())
        if len(got) < count and not pump.ended:
            pump.wait(seen, deadline - time.monotonic())
    got.extend(pump.drain())
    return got


def test_linepump_until_close_lines_in_order(pair):
    ours, peer, make = pair
    pump = make()
    lines = [json.dumps({"n": i}).encode() for i in range(300)]
    peer.sendall(STREAM_HEAD + b"".join(ln + b"\n" for ln in lines) + b"tail")
    assert pump.read_head(5.0) == 200
    assert _collect(pump, 300) == lines
    assert not pump.ended
    peer.shutdown(socket.SHUT_WR)  # read-until-close: the close ends the body
    pump.wait(NEVER, 5.0)
    assert pump.ended and pump.error is None
    assert pump.drain() == [b"tail"]  # the unterminated tail is the last line
    assert pump.seq == 301


def test_linepump_chunked_one_byte_at_a_time(pair):
    ours, peer, make = pair
    pump = make()
    lines = [json.dumps({"n": i, "pad": "x" * (i % 7)}).encode()
             for i in range(12)]
    body = b"".join(ln + b"\n" for ln in lines)
    payload = CHUNKED_HEAD
    for i in range(0, len(body), 5):  # chunks cut lines anywhere
        piece = body[i:i + 5]
        payload += b"%x\r\n" % len(piece) + piece + b"\r\n"
    payload += b"0\r\n\r\n"
    for i in range(len(payload)):
        peer.sendall(payload[i:i + 1])
    assert pump.read_head(5.0) == 200
    pump.wait(NEVER, 5.0)  # the last chunk ends the stream by itself
    assert pump.ended and pump.error is None
    assert pump.drain() == lines


def test_linepump_wait_times_out_then_resumes(pair):
    ours, peer, make = pair
    pump = make()
    with pytest.raises(TimeoutError):
        pump.read_head(0.05)
    peer.sendall(STREAM_HEAD)
    assert pump.read_head(5.0) == 200
    t0 = time.monotonic()
    assert pump.wait(0, 0.1) == 0
    assert 0.09 <= time.monotonic() - t0 < 1.0
    assert pump.drain() == [] and not pump.ended
    peer.sendall(b"late\n")
    assert pump.wait(0, 5.0) == 1
    assert pump.drain() == [b"late"]


def test_linepump_wait_releases_the_gil(pair):
    ours, peer, make = pair
    pump = make()
    peer.sendall(STREAM_HEAD)
    assert pump.read_head(5.0) == 200
    count = [0]
    stop = threading.Event()

    def counter():
        while not stop.is_set():
            count[0] += 1

    t = threading.Thread(target=counter, daemon=True)
    t.start()
    try:
        before = count[0]
        assert pump.wait(0, 0.2) == 0  # nothing arrives
        advanced = count[0] - before
    finally:
        stop.set()
        t.join(5)
    # a wait that held the GIL would leave the counter where it was
    assert advanced > 1000


def test_linepump_shutdown_unblocks_wait_and_stop(pair):
    ours, peer, make = pair
    pump = make()
    peer.sendall(STREAM_HEAD + b"one\n")
    assert pump.read_head(5.0) == 200
    assert pump.wait(0, 5.0) == 1
    result = {}

    def waiter():
        t0 = time.monotonic()
        result["seq"] = pump.wait(1, 30.0)
        result["took"] = time.monotonic() - t0

    t = threading.Thread(target=waiter, daemon=True)
    t.start()
    assert _until(lambda: t.is_alive())
    t0 = time.monotonic()
    ours.shutdown(socket.SHUT_RDWR)
    pump.stop()
    t.join(5)
    assert time.monotonic() - t0 < 1.0
    assert not t.is_alive() and result["seq"] == 1 and result["took"] < 1.0
    assert pump.ended
    os.fstat(ours.fileno())  # the fd is still open, and still ours
    assert ours.fileno() >= 0
    pump.stop()  # again: harmless


def test_linepump_stop_without_shutdown_still_returns(pair):
    ours, peer, make = pair
    pump = make()
    t0 = time.monotonic()
    pump.stop()
    assert time.monotonic() - t0 < 1.0 and pump.ended


def test_linepump_malformed_chunk_sets_error(pair):
    ours, peer, make = pair
    pump = make()
    peer.sendall(CHUNKED_HEAD + b"3\r\nok\n\r\nZZ\r\nnope\r\n")
    assert pump.read_head(5.0) == 200
    pump.wait(NEVER, 5.0)
    assert pump.ended
    assert pump.error == "malformed chunked framing"
    assert pump.drain() == [b"ok"]


def test_linepump_reads_through_a_linereader(pair):
    ours, peer, make = pair
    reader = _wire.LineReader(ours.fileno())
    pump = _wire.LinePump(reader)
    try:
        peer.sendall(STREAM_HEAD + b"x\n")
        assert pump.read_head(5.0) == 200
        assert pump.wait(0, 5.0) == 1
        with pytest.raises(RuntimeError):  # the reader is the pump's now
            reader.readline(0.01)
    finally:
        ours.shutdown(socket.SHUT_RDWR)
        pump.stop()


# ---------------------------------------------------------------------------
# 3. StreamWriter
# ---------------------------------------------------------------------------

def _small_buffers(a, b):
    a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 4096)
    b.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 4096)


def _read_all(sock, until_bytes=None, timeout=10.0):
    """Read until EOF, or until `until_bytes` bytes have arrived."""
    sock.settimeout(timeout)
    data = bytearray()
    while until_bytes is None or len(data) < until_bytes:
        piece = sock.recv(1 << 16)
        if not piece:
            break
        data += piece
    return bytes(data)


def test_streamwriter_eight_threads_lines_whole_and_in_order():
    a, b = socket.socketpair()
    _small_buffers(a, b)  # so that writes do meet a full socket
    writer = _wire.StreamWriter(a.fileno())
    threads, per_thread = 8, 200
    total = 0
    lines = {}
    for t in range(threads):
        lines[t] = [b"t%d:%d:%s\n" % (t, i, b"x" * ((i * 7 + t) % 120))
                    for i in range(per_thread)]
        total += sum(len(ln) for ln in lines[t])
    received = {}
    reader = threading.Thread(
        target=lambda: received.setdefault("data", _read_all(b, total)),
        daemon=True)
    reader.start()
    results = []

    def work(t):
        results.append(all(writer.write(ln) for ln in lines[t]))

    workers = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for w in workers:
        w.start()
    for w in workers:
        w.join(10)
    reader.join(10)
    try:
        assert results == [True] * threads and not writer.dead
        got = received["data"].split(b"\n")
        assert got.pop() == b""  # every line arrived whole
        seen = {t: [] for t in range(threads)}
        for ln in got:
            seen[int(ln[1:ln.index(b":")])].append(ln + b"\n")
        assert seen == lines  # each thread's lines, in that thread's order
        assert _until(lambda: writer.pending == 0)
    finally:
        writer.close()
        a.close()
        b.close()


def test_streamwriter_backlog_accumulates_then_drains_in_order():
    a, b = socket.socketpair()
    _small_buffers(a, b)
    writer = _wire.StreamWriter(a.fileno())
    try:
        lines = [b"%06d:%s\n" % (i, b"y" * 200) for i in range(400)]
        assert all(writer.write(ln) for ln in lines)  # never blocks
        assert writer.pending > 0 and not writer.dead  # nobody is reading
        data = _read_all(b, sum(len(ln) for ln in lines))
        assert data == b"".join(lines)
        assert _until(lambda: writer.pending == 0)
        assert writer.write(b"after\n")
        assert _read_all(b, 6) == b"after\n"
    finally:
        writer.close()
        a.close()
        b.close()


def test_streamwriter_past_the_cap_is_dead_and_shut_down():
    a, b = socket.socketpair()
    _small_buffers(a, b)
    writer = _wire.StreamWriter(a.fileno(), 8192)
    try:
        line = b"z" * 999 + b"\n"
        results = [writer.write(line) for _ in range(200)]  # none raises
        assert results[0] is True and results[-1] is False
        assert results == sorted(results, reverse=True)  # True..., then False...
        assert writer.dead and writer.pending == 0
        # the socket was shut down, not closed: the peer reads whole lines up
        # to an EOF, and the fd is still ours
        data = _read_all(b)
        assert len(data) % 1000 <= 999 and data.count(b"\n") <= results.count(True)
        os.fstat(a.fileno())
        assert writer.write(b"more\n") is False
    finally:
        writer.close()
        a.close()
        b.close()


def test_streamwriter_close_detaches_and_refuses():
    a, b = socket.socketpair()
    _small_buffers(a, b)
    writer = _wire.StreamWriter(a.fileno())
    while writer.pending == 0:
        assert writer.write(b"q" * 500 + b"\n")
    writer.close()
    assert writer.dead and writer.write(b"x\n") is False
    a.close()  # nothing native may touch the fd after close()
    b.close()


def test_overflowing_sink_does_not_fail_the_mutation():
    cluster = FakeCluster()
    cluster.create(_node("n1"))
    a, b = socket.socketpair()
    _small_buffers(a, b)
    writer = _wire.StreamWriter(a.fileno(), 2048)
    watch = cluster.watch("v1", "Node")
    try:
        with cluster._lock:
            watch.set_sink(lambda t, snap: writer.write(
                cluster.event_line(t, snap)))
        for i in range(60):
            out = cluster.patch("v1", "Node", "n1", {"metadata": {
                "annotations": {"blob": "b" * 1024, "i": str(i)}}})
            assert out["metadata"]["annotations"]["i"] == str(i)
        assert writer.dead
        stored = cluster.get("v1", "Node", "n1")
        assert stored["metadata"]["annotations"]["i"] == "59"
        assert watch.events.empty()  # the sink took the queue's place
    finally:
        watch.stop()
        writer.close()
        a.close()
        b.close()


def test_failing_sink_does_not_fail_the_mutation(caplog):
    cluster = FakeCluster()
    watch = cluster.watch("v1", "Node")
    other = cluster.watch("v1", "Node")

    def sink(event_type, snapshot):
        raise RuntimeError("sink broke")

    with cluster._lock:
        watch.set_sink(sink)
    created = cluster.create(_node("n1"))
    assert created["metadata"]["resourceVersion"]
    assert other.next(1.0)[0] == "ADDED"  # later watches still get theirs
    assert "watch sink failed" in caplog.text
    watch.stop()
    other.stop()


def test_event_line_is_built_once_per_event_type(monkeypatch):
    cluster = FakeCluster()
    cluster.create(_node("n1", tier="cpu"))
    watches = [cluster.watch("v1", "Node") for _ in range(3)]
    watches.append(cluster.watch("v1", "Node", label_selector="tier=gpu"))
    got = []
    with cluster._lock:
        for w in watches:
            w.set_sink(lambda t, snap: got.append(cluster.event_line(t, snap)))
    from k8s_operator_libs_amd.core import fakecluster

    calls = []
    real_dumps = json.dumps
    monkeypatch.setattr(fakecluster.json, "dumps",
                        lambda obj, *a, **kw: (calls.append(1),
                                               real_dumps(obj, *a, **kw))[1])
    cluster.patch("v1", "Node", "n1", {"metadata": {"labels": {"tier": "gpu"}}})
    # three MODIFIED share one line, the selector watch's ADDED is its own
    assert len(got) == 4 and len(calls) == 2
    assert got[0] is got[1] is got[2]
    assert json.loads(got[0])["type"] == "MODIFIED"
    assert json.loads(got[3])["type"] == "ADDED"
    for w in watches:
        w.stop()


def test_dead_writer_ends_the_watch_on_the_server(monkeypatch):
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    monkeypatch.setattr(apiserver, "WATCH_MAX_BACKLOG", 4096)
    handle = start_apiserver()
    cluster = handle.cluster
    cluster.create(_node("n1"))
    sock = socket.socket()
    sock.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 4096)
    try:
        sock.connect(("127.0.0.1", int(handle.url.rsplit(":", 1)[1])))
        sock.sendall(b"GET /api/v1/nodes?watch=true HTTP/1.1\r\nHost: t\r\n\r\n")
        assert _until(lambda: cluster._watches.get(("v1", "Node")))
        blob = "b" * 65536
        for i in range(200):  # a reader that never reads: ~13 MB
            out = cluster.patch("v1", "Node", "n1", {"metadata": {
                "annotations": {"blob": blob, "i": str(i)}}})
            assert out["metadata"]["annotations"]["i"] == str(i)
        # the server cut the stream off (the client would re-watch) ...
        data = _read_all(sock)
        assert data.startswith(b"HTTP/1.1 200 OK\r\n")
        # ... and its stream thread ends the watch at its next tick
        assert _until(lambda: not cluster._watches.get(("v1", "Node")), 3.0)
    finally:
        sock.close()
        handle.stop()


# ---------------------------------------------------------------------------
# 4. the bytes of a watch stream: native fan-out against the fallback
# ---------------------------------------------------------------------------

def _pod(name, namespace, tier):
    return {"apiVersion": "v1", "kind": "Pod",
            "metadata": {"name": name, "namespace": namespace,
                         "labels": {"tier": tier},
                         # fixed, so two runs serialise alike
                         "uid": f"uid-{namespace}-{name}",
                         "creationTimestamp": "2024-01-01T00:00:00Z"},
            "spec": {"nodeName": "n1"}}


class _RawWatch:
    """A watch read straight off a socket, byte for byte."""

    def __init__(self, port, target):
        self.sock = socket.create_connection(("127.0.0.1", port), timeout=10)
        self.sock.sendall(f"GET {target} HTTP/1.1\r\nHost: t\r\n\r\n".encode())
        self.data = b""
        while b"\r\n\r\n" not in self.data:  # head: the watch is registered
            self._more()

    def _more(self):
        piece = self.sock.recv(1 << 16)
        assert piece, "stream ended early"
        self.data += piece

    def until(self, marker):
        """(head without its Date line, body up to the line with `marker`,
        keep-alive newlines removed: when those fall is a matter of timing)"""
        while True:
            head, _, body = self.data.partition(b"\r\n\r\n")
            lines = body.split(b"\n")
            done = [ln for ln in lines[:-1] if ln]
            if any(marker in ln for ln in done):
                break
            self._more()
        self.sock.close()
        head = b"\r\n".join(ln for ln in head.split(b"\r\n")
                            if not ln.lower().startswith(b"date:"))
        last = max(i for i, ln in enumerate(done) if marker in ln)
        return head, b"".join(ln + b"\n" for ln in done[:last + 1])


def _scripted_streams(monkeypatch, native):
    if native:
        monkeypatch.delenv(ENV_SWITCH, raising=False)
    else:
        monkeypatch.setenv(ENV_SWITCH, "0")
    handle = start_apiserver()
    port = int(handle.url.rsplit(":", 1)[1])
    cluster = handle.cluster
    client = RestClient(handle.url)
    try:
        streams = {
            "all": _RawWatch(port, "/api/v1/pods?watch=true"),
            "selector": _RawWatch(
                port, "/api/v1/pods?watch=true&labelSelector=tier%3Dgpu"),
            "namespaced": _RawWatch(
                port, "/api/v1/namespaces/ns-a/pods?watch=true"),
        }
        cluster.create(_pod("a1", "ns-a", "gpu"))
        cluster.create(_pod("b1", "ns-b", "cpu"))
        mid_rv = cluster.current_rv()
        # b1 starts matching the selector (ADDED there), a1 stops (DELETED)
        client.patch("v1", "Pod", "b1",
                     {"metadata": {"labels": {"tier": "gpu"}}}, "ns-b")
        cluster.patch("v1", "Pod", "a1",
                      {"metadata": {"labels": {"tier": "cpu"}}}, "ns-a")
        cluster.patch("v1", "Pod", "a1",
                      {"metadata": {"annotations": {"k": "v"}}}, "ns-a")
        streams["resumed"] = _RawWatch(
            port, f"/api/v1/pods?watch=true&resourceVersion={mid_rv}")
        streams["initial"] = _RawWatch(
            port, "/api/v1/pods?watch=true&sendInitialEvents=true"
                  "&resourceVersionMatch=NotOlderThan")
        cluster.delete("v1", "Pod", "b1", "ns-b")
        client.create(_pod("a2", "ns-a", "gpu"))
        cluster.patch_status("v1", "Pod", "a2", {"phase": "Running"}, "ns-a")
        cluster.create(_pod("zz-last", "ns-a", "gpu"))  # every stream sees it
        return {name: s.until(b"zz-last") for name, s in streams.items()}
    finally:
        client.close()
        handle.stop()


def test_stream_bytes_same_with_native_fanout_and_without(monkeypatch):
    made = []
    real_writer = _wire.StreamWriter

    def counting(*args):
        made.append(args)
        return real_writer(*args)

    monkeypatch.setattr(_wire, "StreamWriter", counting)
    fallback = _scripted_streams(monkeypatch, native=False)
    assert made == []
    native = _scripted_streams(monkeypatch, native=True)
    assert len(made) == 5  # one writer per stream: the native path did run
    assert set(native) == {"all", "selector", "namespaced", "resumed", "initial"}
    for name in native:
        assert native[name] == fallback[name], name
    # and the script did exercise what it set out to
    types_of = {name: [json.loads(ln)["type"] for ln in body.splitlines()]
                for name, (_, body) in native.items()}
    assert types_of["selector"] == ["ADDED", "ADDED", "DELETED", "DELETED",
                                    "ADDED", "MODIFIED", "ADDED"]
    assert len(types_of["namespaced"]) == 6
    assert types_of["resumed"][0] == "MODIFIED" and len(types_of["resumed"]) == 7
    assert types_of["initial"][:3] == ["ADDED", "ADDED", "BOOKMARK"]
    bookmark = json.loads(native["initial"][1].splitlines()[2])
    assert bookmark["object"]["metadata"]["annotations"] == {
        "k8s.io/initial-events-end": "true"}


# ---------------------------------------------------------------------------
# 5. informer coherence over the native path
# ---------------------------------------------------------------------------

@pytest.fixture
def served(monkeypatch):
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    handle = start_apiserver()
    client = RestClient(handle.url)
    cached = CachedClient(client)
    yield handle, client, cached
    cached.stop()
    client.close()
    handle.stop()


def _patch_wait_get_cycles(client, cached, names, cycles, errors):
    def work(name):
        try:
            for i in range(cycles):
                out = client.patch("v1", "Node", name,
                                   {"metadata": {"labels": {"i": str(i)}}})
                rv = out["metadata"]["resourceVersion"]
                assert cached.wait_for_resource_version(
                    "v1", "Node", name, "", rv, timeout=10.0)
                got = cached.get("v1", "Node", name)
                assert got["metadata"]["labels"]["i"] == str(i), (name, i)
                assert int(got["metadata"]["resourceVersion"]) >= int(rv)
        except BaseException as exc:  # surfaced by the caller
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads)


def test_every_get_after_the_barrier_shows_the_write(served):
    handle, client, cached = served
    names = [f"n{i}" for i in range(4)]
    for name in names:
        client.create(_node(name))
    assert len(cached.list("v1", "Node")) == 4
    inf = cached._informers[("v1", "Node")]
    assert inf._watch.direct and inf._reads_directly(inf._watch)
    errors = []
    _patch_wait_get_cycles(client, cached, names, 200, errors)
    assert not errors, errors[0]


@pytest.mark.parametrize("fanout,pump,drain", [
    (False, True, True), (True, False, False), (True, True, False),
    (False, False, False)])
def test_each_stage_can_be_switched_off(monkeypatch, fanout, pump, drain):
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    monkeypatch.setattr(apiserver, "WATCH_FANOUT", fanout)
    monkeypatch.setattr(restclient._HttpWatch, "USE_LINE_PUMP", pump)
    monkeypatch.setattr(cache._Informer, "USE_DRAIN_ON_READ", drain)
    made = {"writer": 0, "pump": 0}
    real_writer, real_pump = _wire.StreamWriter, _wire.LinePump
    monkeypatch.setattr(_wire, "StreamWriter", lambda *a: (
        made.__setitem__("writer", made["writer"] + 1), real_writer(*a))[1])
    monkeypatch.setattr(_wire, "LinePump", lambda *a: (
        made.__setitem__("pump", made["pump"] + 1), real_pump(*a))[1])
    handle = start_apiserver()
    client = RestClient(handle.url)
    cached = CachedClient(client)
    try:
        client.create(_node("n0"))
        assert cached.get("v1", "Node", "n0")
        inf = cached._informers[("v1", "Node")]
        assert inf._reads_directly(inf._watch) is (pump and drain)
        errors = []
        _patch_wait_get_cycles(client, cached, ["n0"], 20, errors)
        assert not errors, errors[0]
        assert (made["writer"] > 0) is fanout and (made["pump"] > 0) is pump
    finally:
        cached.stop()
        client.close()
        handle.stop()


def test_sync_delay_keeps_events_on_the_informer_thread(monkeypatch):
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    handle = start_apiserver()
    client = RestClient(handle.url)
    cached = CachedClient(client, sync_delay=0.05)
    try:
        client.create(_node("n0"))
        assert _until(lambda: cached.list("v1", "Node"))
        inf = cached._informers[("v1", "Node")]
        assert inf._watch.direct and not inf._reads_directly(inf._watch)
        out = client.patch("v1", "Node", "n0", {"metadata": {"labels": {"a": "1"}}})
        # the injected lag is still there: a read right after the write is stale
        assert "a" not in cached.get("v1", "Node", "n0")["metadata"]["labels"]
        assert cached.wait_for_resource_version(
            "v1", "Node", "n0", "", out["metadata"]["resourceVersion"], 5.0)
        assert cached.get("v1", "Node", "n0")["metadata"]["labels"]["a"] == "1"
    finally:
        cached.stop()
        client.close()
        handle.stop()


def test_unread_events_are_drained_at_the_idle_tick(served):
    handle, client, cached = served
    client.create(_node("n0"))
    assert cached.get("v1", "Node", "n0")
    inf = cached._informers[("v1", "Node")]
    watch = inf._watch
    assert inf._reads_directly(watch)
    before = watch.seq()
    for i in range(50):
        handle.cluster.patch("v1", "Node", "n0",
                             {"metadata": {"labels": {"i": str(i)}}})
    # nobody reads the cache; the informer thread's tick (0.2 s) must empty
    # the pump and apply the events
    assert _until(lambda: watch.seq() >= before + 50
                  and watch.lines_pending() == 0, 3.0)
    with inf._lock:
        assert inf._store[("", "n0")]["metadata"]["labels"]["i"] == "49"
    assert inf._last_rv == handle.cluster.current_rv()


class _Scripted:
    """Plays one handler per accepted connection; records each request head."""

    def __init__(self, handlers):
        self.handlers = list(handlers)
        self.requests = []
        self.release = threading.Event()
        self.errors = []
        self.listener = socket.socket()
        self.listener.bind(("127.0.0.1", 0))
        self.listener.listen(8)
        self.url = f"http://127.0.0.1:{self.listener.getsockname()[1]}"
        self.threads = [threading.Thread(target=self._accept, daemon=True)]
        self.threads[0].start()

    def _accept(self):
        for handler in self.handlers:
            try:
                conn, _ = self.listener.accept()
            except OSError:
                return
            t = threading.Thread(target=self._run, args=(handler, conn),
                                 daemon=True)
            t.start()
            self.threads.append(t)

    def _run(self, handler, conn):
        try:
            conn.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            data = b""
            while b"\r\n\r\n" not in data:
                piece = conn.recv(65536)
                if not piece:
                    return
                data += piece
            self.requests.append(data.split(b"\r\n", 1)[0].decode())
            handler(self, conn)
        except Exception as exc:
            self.errors.append(exc)
        finally:
            conn.close()

    def close(self):
        self.release.set()
        try:
            self.listener.shutdown(socket.SHUT_RDWR)
        except OSError:
            pass
        self.listener.close()
        for t in self.threads:
            t.join(5)
        assert not self.errors, self.errors


def _event(event_type, name, rv, **labels):
    obj = _node(name, **labels)
    obj["metadata"]["resourceVersion"] = str(rv)
    return json.dumps({"type": event_type, "object": obj}).encode() + b"\n"


def _initial_end(rv):
    return json.dumps({"type": "BOOKMARK", "object": {
        "kind": "Node", "apiVersion": "v1", "metadata": {
            "resourceVersion": str(rv),
            "annotations": {"k8s.io/initial-events-end": "true"}}}}
    ).encode() + b"\n"


def test_out_of_order_drop_and_410_over_a_scripted_server(monkeypatch):
    monkeypatch.delenv(ENV_SWITCH, raising=False)

    def first_stream(srv, conn):
        # initial state is empty; then x at 5, a stale x at 3, y at 6 — and
        # the server drops the stream
        conn.sendall(STREAM_HEAD + _initial_end(1)
                     + _event("ADDED", "x", 5, v="five")
                     + _event("MODIFIED", "x", 3, v="three")
                     + _event("ADDED", "y", 6))
        srv.first_sent.wait(10)

    def second_stream(srv, conn):
        conn.sendall(STREAM_HEAD + _event("MODIFIED", "y", 7, v="seven"))
        srv.expire.wait(10)
        conn.sendall(json.dumps({"type": "ERROR", "object": {
            "kind": "Status", "apiVersion": "v1", "status": "Failure",
            "reason": "Expired", "code": 410}}).encode() + b"\n")
        srv.release.wait(10)

    def relist(srv, conn):
        z = _node("z")
        z["metadata"]["resourceVersion"] = "19"
        body = json.dumps({"kind": "NodeList", "apiVersion": "v1",
                           "metadata": {"resourceVersion": "20"},
                           "items": [z]}).encode()
        conn.sendall(b"HTTP/1.1 200 OK\r\nContent-Type: application/json\r\n"
                     b"Content-Length: %d\r\n\r\n" % len(body) + body)
        srv.release.wait(10)

    def third_stream(srv, conn):
        conn.sendall(STREAM_HEAD + _event("ADDED", "w", 21))
        srv.release.wait(10)

    srv = _Scripted([first_stream, second_stream, relist, third_stream])
    srv.first_sent = threading.Event()
    srv.expire = threading.Event()
    client = RestClient(srv.url)
    cached = CachedClient(client)
    try:
        # rv 5 then rv 3 for x: the cache stays at 5
        assert cached.wait_for_resource_version("v1", "Node", "y", "", "6", 5.0)
        x = cached.get("v1", "Node", "x")
        assert x["metadata"]["resourceVersion"] == "5"
        assert x["metadata"]["labels"]["v"] == "five"
        inf = cached._informers[("v1", "Node")]
        assert inf._reads_directly(inf._watch) and inf._last_rv == "6"
        # a server drop: re-watch from the last resourceVersion, no relist
        srv.first_sent.set()
        assert cached.wait_for_resource_version("v1", "Node", "y", "", "7", 5.0)
        assert len(srv.requests) == 2
        assert "watch=true" in srv.requests[1]
        assert "resourceVersion=6" in srv.requests[1]
        assert cached.get("v1", "Node", "x")["metadata"]["resourceVersion"] == "5"
        # an in-stream 410: relist, then watch from the list's resourceVersion
        srv.expire.set()
        assert _until(lambda: len(srv.requests) == 4)
        assert srv.requests[2].startswith("GET /api/v1/nodes")
        assert "watch=true" not in srv.requests[2]
        assert "watch=true" in srv.requests[3]
        assert "resourceVersion=20" in srv.requests[3]
        assert cached.wait_for_resource_version("v1", "Node", "w", "", "21", 5.0)
        assert [n["metadata"]["name"] for n in cached.list("v1", "Node")] == [
            "w", "z"]
    finally:
        cached.stop()
        client.close()
        srv.close()


def test_next_keeps_its_contract_over_the_pump(monkeypatch):
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    handle = start_apiserver()
    client = RestClient(handle.url)
    try:
        client.create(_node("n1"))
        w = client.watch("v1", "Node", resource_version="0")
        assert w.direct and w._sock is not None and w.alive()
        assert w.next(5.0)[0] == "ADDED"
        t0 = time.monotonic()
        assert w.next(0.05) is None  # a timeout, not an early return
        assert time.monotonic() - t0 >= 0.045
        client.patch("v1", "Node", "n1", {"metadata": {"labels": {"a": "1"}}})
        client.delete("v1", "Node", "n1")
        assert [w.next(5.0)[0] for _ in range(2)] == ["MODIFIED", "DELETED"]
        w.stop()
        assert not w.alive() and w._sock is None
        assert w.next(0.01) is None
        w.stop()
    finally:
        client.close()
        handle.stop()


# ---------------------------------------------------------------------------
# 6. fallback
# ---------------------------------------------------------------------------

def _spy(monkeypatch):
    made = []
    real_writer, real_pump = _wire.StreamWriter, _wire.LinePump
    monkeypatch.setattr(_wire, "StreamWriter",
                        lambda *a: (made.append("StreamWriter"),
                                    real_writer(*a))[1])
    monkeypatch.setattr(_wire, "LinePump",
                        lambda *a: (made.append("LinePump"), real_pump(*a))[1])
    return made


def _one_round(expect_direct):
    handle = start_apiserver()
    client = RestClient(handle.url)
    cached = CachedClient(client)
    try:
        client.create(_node("n0"))
        assert cached.get("v1", "Node", "n0")
        inf = cached._informers[("v1", "Node")]
        assert inf._reads_directly(inf._watch) is expect_direct
        if not expect_direct:
            assert isinstance(inf._watch._thread, threading.Thread)
        errors = []
        _patch_wait_get_cycles(client, cached, ["n0"], 10, errors)
        assert not errors, errors[0]
        return client
    finally:
        cached.stop()
        client.close()
        handle.stop()


def test_environment_switch_off_constructs_neither_class(monkeypatch):
    made = _spy(monkeypatch)
    monkeypatch.setenv(ENV_SWITCH, "0")
    client = _one_round(expect_direct=False)
    assert client._wire is None and made == []
    monkeypatch.delenv(ENV_SWITCH)
    _one_round(expect_direct=True)
    assert {"StreamWriter", "LinePump"} <= set(made)


def test_older_extension_without_the_new_names_runs_the_old_paths(monkeypatch):
    monkeypatch.delenv(ENV_SWITCH, raising=False)
    made = _spy(monkeypatch)
    older = types.SimpleNamespace(
        exchange=_wire.exchange, LineReader=_wire.LineReader,
        parse_request_head=_wire.parse_request_head)
    monkeypatch.setattr(native_pkg, "load_wire", lambda: older)
    monkeypatch.setattr(restclient, "_load_wire", lambda: older)
    client = _one_round(expect_direct=False)
    assert client._wire is older and made == []
