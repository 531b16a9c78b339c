"""httpx-based Kubernetes REST client.

The production implementation of
:class:`~k8s_operator_libs_amd.core.client.Client` (the in-process analogue
of client-go + controller-runtime's typed client): standard apiserver REST
paths, JSON merge patches, the eviction subresource, label/field selector
query params, and a discovery call used by crdutil's wait-until-served poll.

Configuration resolution order (``from_environment``):

1. explicit ``base_url`` argument,
2. in-cluster service account
   (``/var/run/secrets/kubernetes.io/serviceaccount``),
3. ``$KUBECONFIG`` (minimal parse: current-context cluster + token/cert auth),
4. ``$KUBERNETES_MASTER`` URL (no auth — dev/test apiservers).
"""

from __future__ import annotations

import collections
import http.client as _http_client
import json
import os
from typing import Any, Dict, Optional

import httpx

from ..native import load_wire as _load_wire
from . import meta
from .client import Client
from .errors import (
    AlreadyExistsError,
    ApiError,
    BadRequestError,
    ConflictError,
    NotFoundError,
)

SA_DIR = "/var/run/secrets/kubernetes.io/serviceaccount"

# (apiVersion, kind) -> (plural, namespaced); mirrors the FakeCluster registry
_KIND_INFO = {
    ("v1", "Node"): ("nodes", False),
    ("v1", "Pod"): ("pods", True),
    ("v1", "Event"): ("events", True),
    ("v1", "Namespace"): ("namespaces", False),
    ("apps/v1", "DaemonSet"): ("daemonsets", True),
    ("apps/v1", "ControllerRevision"): ("controllerrevisions", True),
    ("apiextensions.k8s.io/v1", "CustomResourceDefinition"): (
        "customresourcedefinitions", False),
    ("maintenance.amd.com/v1alpha1", "NodeMaintenance"): ("nodemaintenances", True),
    ("coordination.k8s.io/v1", "Lease"): ("leases", True),
}


def _lower_plural(kind: str) -> str:
    """English pluralization matching apimachinery's namer conventions:
    ``NetworkPolicy`` -> ``networkpolicies``, ``Ingress`` -> ``ingresses``,
    ``Endpoints`` -> ``endpoints``.  Only a fallback — registered kinds and
    discovery (see :meth:`RestClient._kind_info`) take precedence."""
    k = kind.lower()
    if k.endswith(("ss", "x", "z", "ch", "sh")):
        return k + "es"
    if k.endswith("s"):
        return k  # already plural-looking (Endpoints)
    if k.endswith("y") and len(k) > 1 and k[-2] not in "aeiou":
        return k[:-1] + "ies"
    return k + "s"


def _pool_max_idle() -> int:
    """Idle connections worth keeping: one per thread that can be talking
    to the apiserver at the same moment.  That is the reconcile thread,
    the eviction and the drain workers (each manager bounds its own) and
    the per-phase node fan-out."""
    from ..upgrade.common_manager import CommonUpgradeManager
    from ..upgrade.drain_manager import DrainManager
    from ..upgrade.pod_manager import PodManager

    return (1 + PodManager.MAX_CONCURRENT_NODE_WORKERS
            + DrainManager.MAX_CONCURRENT_NODE_WORKERS
            + CommonUpgradeManager.MAX_PARALLEL_NODE_OPS)


class RestClient(Client):
    #: plain-HTTP requests share keep-alive connections between threads
    #: through ``_wire.Pool`` when the extension has it, so a worker thread
    #: started for one node does not dial a connection of its own; False
    #: keeps one socket per thread (``_fast_local``)
    USE_POOL = True

    def __init__(
        self,
        base_url: str,
        token: Optional[str] = None,
        verify: Any = True,
        timeout: float = 30.0,
        extra_kinds: Optional[Dict[tuple, tuple]] = None,
        retries: int = 3,
    ) -> None:
        self.base_url = base_url.rstrip("/")
        headers = {"Content-Type": "application/json"}
        if token:
            headers["Authorization"] = f"Bearer {token}"
        self._headers = dict(headers)
        self._timeout = timeout
        self._http = httpx.Client(
            base_url=self.base_url, headers=headers, verify=verify, timeout=timeout
        )
        # Plain-HTTP fast path: thread-local persistent http.client
        # connections cut ~40% off per-request latency vs the full httpx
        # stack — and request latency IS the reconcile loop's wire cost.
        # TLS endpoints (real apiservers) stay on httpx.
        self._fast_netloc = None
        self._wire = None
        self._pool = None
        if self.base_url.startswith("http://"):
            import urllib.parse

            parsed = urllib.parse.urlsplit(self.base_url)
            self._fast_netloc = (parsed.hostname, parsed.port or 80)
            self._fast_local = __import__("threading").local()
            # native wire path (plain HTTP only; TLS never takes it)
            self._wire = _load_wire()
            self._wire_heads: Dict[tuple, bytes] = {}
            if self._wire is not None and hasattr(self._wire, "Pool"):
                self._pool = self._wire.Pool(
                    *self._fast_netloc, max_idle=_pool_max_idle(),
                    connect_timeout=timeout)
        self._kinds = dict(_KIND_INFO)
        if extra_kinds:
            self._kinds.update(extra_kinds)
        self._retries = retries

    # -- plain-HTTP fast transport -------------------------------------------

    def _wire_head(self, headers=None) -> bytes:
        """The request's header block (Host, auth, content type), encoded
        once per client and per distinct override rather than per request."""
        key = tuple(sorted(headers.items())) if headers else ()
        head = self._wire_heads.get(key)
        if head is None:
            host, port = self._fast_netloc
            if ":" in host:
                host = f"[{host}]"
            hdrs = {"Host": host if port == 80 else f"{host}:{port}",
                    "Accept-Encoding": "identity"}
            hdrs.update(self._headers)
            if headers:
                hdrs.update(headers)
            head = "".join(f"{k}: {v}\r\n" for k, v in hdrs.items()).encode(
                "latin-1")
            self._wire_heads[key] = head
        return head

    def _wire_connect(self):
        import socket

        sock = socket.create_connection(self._fast_netloc,
                                        timeout=self._timeout)
        sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        return sock

    def _wire_request(self, method: str, path: str, params=None, content=None,
                      headers=None):
        """``_fast_request`` over the native extension: one send, then
        poll/recv with the GIL released and no Python-level parsing.  The
        thread-local socket stays owned here; the extension only borrows
        its fd.  Same reconnect-once behaviour as the http.client path."""
        import urllib.parse

        if params:
            path = f"{path}?{urllib.parse.urlencode(params)}"
        head = self._wire_head(headers)
        pool = self._pool if self.USE_POOL else None
        if pool is not None:
            try:
                return self._pool_request(pool, method, path, head, content)
            except _PoolClosed:
                pass  # close() won the race: as after close() without a pool
        sock = getattr(self._fast_local, "sock", None)
        for attempt in (0, 1):
            try:
                if sock is None:
                    sock = self._wire_connect()
                    self._fast_local.sock = sock
                status, data, reusable = self._wire.exchange(
                    sock.fileno(), method, path, head, content, self._timeout)
            except ValueError as exc:
                # malformed framing: the connection is unusable and the
                # request is not resent; surface it as the protocol error
                # the retry loop in _request already understands
                self._wire_drop(sock)
                raise _http_client.HTTPException(str(exc)) from exc
            except (ConnectionError, OSError):
                # keep-alive connection died (server restart/idle close):
                # reconnect once, then let the caller's retry logic own it.
                # On purpose exactly what the http.client path below does,
                # no wider: OSError covers TimeoutError, so a request that
                # timed out after it was sent is resent once there too
                # (ADVICE.md flags that resend; narrowing it is a change of
                # its own, for both paths at once).
                self._wire_drop(sock)
                sock = None
                if attempt:
                    raise
            except BaseException:
                # interrupted mid-exchange (Ctrl-C): a half-read response
                # must not be left for the next request
                self._wire_drop(sock)
                raise
            else:
                if not reusable:
                    self._wire_drop(sock)
                return _FastResponse(status, data)
        raise AssertionError("unreachable")

    def _pool_request(self, pool, method: str, path: str, head: bytes,
                      content):
        """``_wire_request`` over a connection borrowed from the client's
        pool for this one exchange.  The fd stays the pool's: it goes back
        with ``checkin`` whatever happened, and the pool keeps it only
        after a complete, reusable response.  A connection from the idle
        list that turns out dead is replaced by a fresh dial once, as the
        thread-local path reconnects once, but only for a reset or a
        broken pipe; a freshly dialled one is not retried."""
        for fresh in (False, True):
            try:
                fd, reused = pool.checkout(fresh)
            except RuntimeError as exc:
                raise _PoolClosed() from exc
            keep = False
            try:
                status, data, keep = self._wire.exchange(
                    fd, method, path, head, content, self._timeout)
            except ValueError as exc:
                # malformed framing: not resent (see _wire_request)
                raise _http_client.HTTPException(str(exc)) from exc
            except (ConnectionResetError, BrokenPipeError):
                if not reused:
                    raise
            else:
                return _FastResponse(status, data)
            finally:
                # also on timeout and on an interruption (Ctrl-C): a
                # half-read response is closed, not left for the next user
                pool.checkin(fd, keep)
        raise AssertionError("unreachable")

    def _wire_drop(self, sock) -> None:
        if sock is not None:
            try:
                sock.close()
            except Exception:
                pass
        self._fast_local.sock = None

    def _fast_request(self, method: str, path: str, params=None, content=None,
                      headers=None):
        if self._wire is not None:
            return self._wire_request(method, path, params=params,
                                      content=content, headers=headers)
        import http.client
        import urllib.parse

        if params:
            path = f"{path}?{urllib.parse.urlencode(params)}"
        conn = getattr(self._fast_local, "conn", None)
        hdrs = dict(self._headers)
        if headers:
            hdrs.update(headers)
        body = content if content is not None else None
        for attempt in (0, 1):
            if conn is None:
                conn = http.client.HTTPConnection(
                    *self._fast_netloc, timeout=self._timeout
                )
                self._fast_local.conn = conn
            try:
                conn.request(method, path, body=body, headers=hdrs)
                resp = conn.getresponse()
                data = resp.read()
                return _FastResponse(resp.status, data)
            except (http.client.HTTPException, ConnectionError, OSError):
                # keep-alive connection died (server restart/idle close):
                # reconnect once, then let the caller's retry logic own it
                try:
                    conn.close()
                except Exception:
                    pass
                conn = None
                self._fast_local.conn = None
                if attempt:
                    raise
        raise AssertionError("unreachable")

    def _request(self, method: str, path: str, **kw) -> httpx.Response:
        """Issue a request with client-go-style retries on transient failures
        (connection errors, 429/5xx).  Conflicts/NotFound/etc. surface
        immediately — the callers' optimistic-concurrency logic owns those."""
        import time as _time

        attempt = 0
        while True:
            try:
                if self._fast_netloc is not None:
                    resp = self._fast_request(method, path, **kw)
                else:
                    resp = self._http.request(method, path, **kw)
            except (httpx.ConnectError, httpx.ReadError, httpx.RemoteProtocolError,
                    httpx.ConnectTimeout, httpx.ReadTimeout,
                    _http_client.HTTPException,
                    ConnectionError, OSError) as exc:
                if attempt >= self._retries:
                    err = ApiError(f"connection to apiserver failed: {exc}")
                    err.code = 503
                    raise err from exc
            else:
                if resp.status_code not in (429, 500, 502, 503, 504) or \
                        attempt >= self._retries:
                    return resp
            attempt += 1
            _time.sleep(min(0.05 * (2 ** attempt), 1.0))

    @classmethod
    def from_environment(cls) -> "RestClient":
        token_path = os.path.join(SA_DIR, "token")
        if os.path.exists(token_path):
            with open(token_path) as fh:
                token = fh.read().strip()
            host = os.environ.get("KUBERNETES_SERVICE_HOST", "kubernetes.default.svc")
            port = os.environ.get("KUBERNETES_SERVICE_PORT", "443")
            ca = os.path.join(SA_DIR, "ca.crt")
            return cls(f"https://{host}:{port}", token=token,
                       verify=ca if os.path.exists(ca) else True)
        kubeconfig = os.environ.get("KUBECONFIG")
        if kubeconfig and os.path.exists(kubeconfig):
            return cls._from_kubeconfig(kubeconfig)
        master = os.environ.get("KUBERNETES_MASTER")
        if master:
            return cls(master, verify=False)
        raise RuntimeError(
            "no cluster configuration found (service account, $KUBECONFIG, "
            "or $KUBERNETES_MASTER)"
        )

    @classmethod
    def _from_kubeconfig(cls, path: str) -> "RestClient":
        import yaml

        with open(path) as fh:
            cfg = yaml.safe_load(fh)
        ctx_name = cfg.get("current-context")
        ctx = next(c["context"] for c in cfg["contexts"] if c["name"] == ctx_name)
        cluster = next(
            c["cluster"] for c in cfg["clusters"] if c["name"] == ctx["cluster"]
        )
        user = next(u["user"] for u in cfg["users"] if u["name"] == ctx["user"])
        token = user.get("token")
        verify: Any = cluster.get("certificate-authority", True)
        if cluster.get("insecure-skip-tls-verify"):
            verify = False
        return cls(cluster["server"], token=token, verify=verify)

    # -- path construction ----------------------------------------------------

    def _kind_info(self, api_version: str, kind: str) -> tuple:
        info = self._kinds.get((api_version, kind))
        if info is None:
            # resolve through API discovery (authoritative, like client-go's
            # RESTMapper) before falling back to English pluralization rules
            info = self._discover_kind(api_version, kind) or (_lower_plural(kind), True)
            self._kinds[(api_version, kind)] = info
        return info

    def _discover_kind(self, api_version: str, kind: str) -> Optional[tuple]:
        prefix = f"/api/{api_version}" if "/" not in api_version else f"/apis/{api_version}"
        try:
            resp = self._request("GET", prefix)
        except ApiError:
            return None
        if resp.status_code != 200:
            return None
        try:
            resources = resp.json().get("resources", [])
        except ValueError:
            return None
        for res in resources:
            if res.get("kind") == kind and "/" not in res.get("name", ""):
                return (res["name"], bool(res.get("namespaced", True)))
        return None

    def _collection_path(self, api_version: str, kind: str, namespace: str) -> str:
        plural, namespaced = self._kind_info(api_version, kind)
        prefix = f"/api/{api_version}" if "/" not in api_version else f"/apis/{api_version}"
        if namespaced and namespace:
            return f"{prefix}/namespaces/{namespace}/{plural}"
        return f"{prefix}/{plural}"

    def _object_path(self, api_version: str, kind: str, name: str, namespace: str) -> str:
        return f"{self._collection_path(api_version, kind, namespace)}/{name}"

    @staticmethod
    def _raise_for(resp: httpx.Response) -> None:
        if resp.status_code < 400:
            return
        try:
            message = resp.json().get("message", resp.text)
        except ValueError:
            message = resp.text
        if resp.status_code == 404:
            raise NotFoundError(message)
        if resp.status_code == 409:
            # AlreadyExists vs Conflict share 409; K8s status reason decides
            try:
                reason = resp.json().get("reason", "")
            except ValueError:
                reason = ""
            if reason == "AlreadyExists":
                raise AlreadyExistsError(message)
            raise ConflictError(message)
        if resp.status_code == 400:
            raise BadRequestError(message)
        if resp.status_code == 422:
            from .errors import InvalidError

            raise InvalidError(message)
        err = ApiError(message)
        err.code = resp.status_code
        raise err

    # -- Client implementation -------------------------------------------------

    def get(self, api_version, kind, name, namespace=""):
        resp = self._request("GET", self._object_path(api_version, kind, name, namespace))
        self._raise_for(resp)
        return resp.json()

    def list(self, api_version, kind, namespace=None, label_selector="", field_selector=""):
        return self.list_with_meta(
            api_version, kind, namespace=namespace,
            label_selector=label_selector, field_selector=field_selector,
        )[0]

    #: LIST chunk size (client-go reflector uses 500; 0 disables pagination)
    LIST_PAGE_SIZE = 500

    def list_with_meta(self, api_version, kind, namespace=None,
                       label_selector="", field_selector=""):
        """Chunked LIST following ``continue`` tokens (the client-go
        pager), returning all items plus the first chunk's list RV."""
        params = {}
        if label_selector:
            params["labelSelector"] = label_selector
        if field_selector:
            params["fieldSelector"] = field_selector
        if self.LIST_PAGE_SIZE:
            params["limit"] = str(self.LIST_PAGE_SIZE)
        path = self._collection_path(api_version, kind, namespace or "")
        items: list = []
        rv = None
        while True:
            resp = self._request("GET", path, params=params)
            self._raise_for(resp)
            body = resp.json()
            md = body.get("metadata") or {}
            if rv is None:
                rv = md.get("resourceVersion")
            items.extend(body.get("items", []))
            cont = md.get("continue")
            if not cont:
                return items, rv
            params["continue"] = cont

    def create(self, obj):
        api_version, kind = meta.api_version(obj), meta.kind(obj)
        path = self._collection_path(api_version, kind, meta.namespace(obj))
        resp = self._request("POST", path, content=json.dumps(obj))
        self._raise_for(resp)
        return resp.json()

    def update(self, obj):
        api_version, kind = meta.api_version(obj), meta.kind(obj)
        path = self._object_path(api_version, kind, meta.name(obj), meta.namespace(obj))
        resp = self._request("PUT", path, content=json.dumps(obj))
        self._raise_for(resp)
        return resp.json()

    def patch(self, api_version, kind, name, patch, namespace=""):
        path = self._object_path(api_version, kind, name, namespace)
        resp = self._request(
            "PATCH", path, content=json.dumps(patch),
            headers={"Content-Type": "application/merge-patch+json"},
        )
        self._raise_for(resp)
        return resp.json()

    def delete(self, api_version, kind, name, namespace="", grace_period_seconds=None):
        kw = {}
        if grace_period_seconds is not None:
            kw["content"] = json.dumps({
                "apiVersion": "v1", "kind": "DeleteOptions",
                "gracePeriodSeconds": int(grace_period_seconds),
            })
        resp = self._request(
            "DELETE", self._object_path(api_version, kind, name, namespace), **kw
        )
        self._raise_for(resp)

    def patch_status(self, api_version, kind, name, status, namespace=""):
        path = self._object_path(api_version, kind, name, namespace) + "/status"
        resp = self._request(
            "PATCH", path, content=json.dumps({"status": status}),
            headers={"Content-Type": "application/merge-patch+json"},
        )
        self._raise_for(resp)
        return resp.json()

    def evict_pod(self, name, namespace):
        path = self._object_path("v1", "Pod", name, namespace) + "/eviction"
        body = {
            "apiVersion": "policy/v1",
            "kind": "Eviction",
            "metadata": {"name": name, "namespace": namespace},
        }
        resp = self._request("POST", path, content=json.dumps(body))
        self._raise_for(resp)

    def watch(self, api_version: str, kind: str, namespace=None,
              resource_version=None, label_selector="", field_selector="",
              send_initial_events=False):
        """Open a Kubernetes watch stream (``?watch=true``) with standard
        query parameters: ``resourceVersion`` anchoring, ``labelSelector``
        filtering, namespace-scoped paths, and ``allowWatchBookmarks`` so
        the server can advance the resume point while idle.  Returns an
        object with ``next(timeout)`` / ``stop()`` like FakeCluster's Watch —
        :class:`~k8s_operator_libs_amd.core.cache.CachedClient` runs
        unchanged over REST.  An expired resume point surfaces as a
        410 ``GoneError`` (HTTP status) or an in-stream ``("ERROR", status)``
        event, both of which the informer answers with relist."""
        return _HttpWatch(self, api_version, kind, namespace=namespace,
                          resource_version=resource_version,
                          label_selector=label_selector,
                          field_selector=field_selector,
                          send_initial_events=send_initial_events)

    # -- discovery (for crdutil.wait_for_crds) ----------------------------------

    def discover_resource(self, api_version: str, plural: str) -> bool:
        prefix = f"/api/{api_version}" if "/" not in api_version else f"/apis/{api_version}"
        resp = self._request("GET", prefix)
        if resp.status_code != 200:
            return False
        for res in resp.json().get("resources", []):
            if res.get("name") == plural:
                return True
        return False

    def register_kind(self, api_version: str, kind: str, plural: str, namespaced: bool) -> None:
        self._kinds[(api_version, kind)] = (plural, namespaced)

    def close(self) -> None:
        self._http.close()
        if self._fast_netloc is not None:
            conn = getattr(self._fast_local, "conn", None)
            if conn is not None:
                try:
                    conn.close()
                except Exception:
                    pass
                self._fast_local.conn = None
            self._wire_drop(getattr(self._fast_local, "sock", None))
            pool, self._pool = self._pool, None
            if pool is not None:
                pool.close()


class _PoolClosed(Exception):
    """The client was closed while a request was on its way to the pool."""


class _FastResponse:
    """Minimal response shim matching the httpx surface `_raise_for` and
    the CRUD methods consume (status_code / json() / text)."""

    __slots__ = ("status_code", "_data")

    def __init__(self, status_code: int, data: bytes) -> None:
        self.status_code = status_code
        self._data = data

    def json(self):
        return json.loads(self._data)

    @property
    def text(self) -> str:
        return self._data.decode(errors="replace")


class _HttpWatch:
    """Streaming watch over HTTP: a reader thread feeds a queue of
    ``(event_type, object)`` tuples parsed from newline-delimited WatchEvent
    JSON — the real apiserver framing, with no custom handshake.  The
    constructor returns once the response headers arrive (the server has
    registered the watch by then); against an RV-anchored server nothing can
    be lost before that because the informer resumes from its list RV.
    ``ERROR`` and ``BOOKMARK`` events pass through to the consumer.

    On plain-HTTP endpoints with the ``_wire`` extension there is no Python
    reader thread and no queue: a ``_wire.LinePump`` thread collects the
    lines without the GIL and :meth:`next` (wait, drain, ``json.loads``)
    decodes them on the caller's thread.  A consumer that wants the events
    on a thread of its own choosing takes them with :meth:`drain_events`
    (see ``cache._Informer``)."""

    #: read plain-HTTP streams with ``_wire.LinePump`` when the extension has
    #: it; False keeps the Python reader thread over ``_wire.LineReader``
    USE_LINE_PUMP = True

    def __init__(self, client: RestClient, api_version: str, kind: str,
                 namespace=None, resource_version=None,
                 label_selector="", field_selector="",
                 send_initial_events=False) -> None:
        import queue
        import threading

        self._queue: "queue.Queue" = queue.Queue()
        self._stop = threading.Event()
        self._connected = threading.Event()
        path = client._collection_path(api_version, kind, namespace or "")
        params = {"watch": "true", "allowWatchBookmarks": "true"}
        if resource_version is not None:
            params["resourceVersion"] = str(resource_version)
        if label_selector:
            params["labelSelector"] = label_selector
        if field_selector:
            params["fieldSelector"] = field_selector
        if send_initial_events:
            params["sendInitialEvents"] = "true"
            params["resourceVersionMatch"] = "NotOlderThan"
        self._error: Optional[BaseException] = None

        def reader():
            try:
                # stream through the client's own session so TLS verification,
                # auth headers and base_url apply to watches too
                with client._http.stream(
                    "GET", path, params=params, timeout=None,
                ) as resp:
                    self._resp = resp  # stop() closes it to unblock instantly
                    if resp.status_code == 410:
                        from .errors import GoneError

                        self._error = GoneError("watch resume point expired")
                        return
                    if resp.status_code >= 400:
                        err = ApiError(f"watch rejected: HTTP {resp.status_code}")
                        err.code = resp.status_code
                        self._error = err
                        return
                    # headers received: the server has registered the watch
                    self._connected.set()
                    for line in resp.iter_lines():
                        if self._stop.is_set():
                            break
                        line = line.strip()
                        if not line:
                            continue
                        try:
                            event = json.loads(line)
                        except ValueError:
                            continue
                        self._queue.put((event.get("type"), event.get("object")))
            except Exception as exc:
                if not self._stop.is_set():
                    # stream dropped: alive() goes False and the informer
                    # layer reconnects from its last RV; no point crashing
                    import logging as _logging

                    _logging.getLogger(__name__).warning(
                        "watch stream ended: %s", exc
                    )
            finally:
                self._connected.set()  # never leave a waiter hanging

        def native_reader():
            # plain-HTTP endpoints: own socket, head and line framing parsed
            # natively with the GIL released while waiting
            import urllib.parse

            wire = client._wire
            sock = None
            try:
                sock = client._wire_connect()
                self._sock = sock  # stop() shuts it down to unblock instantly
                if self._stop.is_set():
                    return
                request = (
                    f"GET {path}?{urllib.parse.urlencode(params)} HTTP/1.1\r\n"
                ).encode("latin-1") + client._wire_head() + b"\r\n"
                sock.sendall(request)
                lines = wire.LineReader(sock.fileno())
                status = lines.read_head(client._timeout)
                if status == 410:
                    from .errors import GoneError

                    self._error = GoneError("watch resume point expired")
                    return
                if status >= 400:
                    err = ApiError(f"watch rejected: HTTP {status}")
                    err.code = status
                    self._error = err
                    return
                # headers received: the server has registered the watch
                self._connected.set()
                while not self._stop.is_set():
                    try:
                        line = lines.readline(None)
                    except EOFError:
                        break
                    if line is None:
                        continue
                    try:
                        event = json.loads(line)
                    except ValueError:
                        continue
                    self._queue.put((event.get("type"), event.get("object")))
            except Exception as exc:
                if not self._stop.is_set():
                    import logging as _logging

                    _logging.getLogger(__name__).warning(
                        "watch stream ended: %s", exc
                    )
            finally:
                self._connected.set()  # never leave a waiter hanging
                # closed only here, after readline has returned: the fd
                # cannot be reused under a blocked recv
                if sock is not None:
                    try:
                        sock.close()
                    except Exception:
                        pass

        self._sock = None
        self._resp = None
        self._pump = None
        # decoded events not yet handed out (line-pump path)
        self._ready: "collections.deque" = collections.deque()
        self._stop_lock = threading.Lock()
        wire = client._wire
        if wire is not None and client._fast_netloc is not None:
            if self.USE_LINE_PUMP and hasattr(wire, "LinePump"):
                self._open_pumped(client, wire, path, params)
                if self._error is not None:
                    raise self._error
                return
            reader = native_reader
        self._thread = threading.Thread(target=reader, daemon=True)
        self._thread.start()
        self._connected.wait(10.0)
        if self._error is not None:
            raise self._error

    def _open_pumped(self, client, wire, path, params) -> None:
        """Plain-HTTP endpoints with ``_wire.LinePump``: connect and read the
        response head here, on the caller's thread; from then on a native
        thread reads the lines and never takes the GIL."""
        import urllib.parse

        from .errors import GoneError

        sock = None
        try:
            sock = client._wire_connect()
            request = (
                f"GET {path}?{urllib.parse.urlencode(params)} HTTP/1.1\r\n"
            ).encode("latin-1") + client._wire_head() + b"\r\n"
            sock.sendall(request)
            # the reader stays the one place that frames the stream; the
            # pump's thread reads through it
            pump = wire.LinePump(wire.LineReader(sock.fileno()))
        except Exception as exc:
            self._pump_failed(sock, None, exc)
            return
        try:
            status = pump.read_head(client._timeout)
        except Exception as exc:
            self._pump_failed(sock, pump, exc)
            return
        if status == 410 or status >= 400:
            if status == 410:
                self._error = GoneError("watch resume point expired")
            else:
                self._error = ApiError(f"watch rejected: HTTP {status}")
                self._error.code = status
            self._pump_failed(sock, pump, None)
            return
        self._sock = sock
        self._pump = pump
        self._thread = _PumpThread(pump)

    def _pump_failed(self, sock, pump, exc) -> None:
        """The stream never opened: like a stream that dropped at once,
        ``alive()`` is False and the informer layer reconnects."""
        import logging as _logging
        import socket as _socket

        if exc is not None:
            _logging.getLogger(__name__).warning("watch stream ended: %s", exc)
        if sock is not None:
            try:
                sock.shutdown(_socket.SHUT_RDWR)
            except OSError:
                pass
        if pump is not None:
            pump.stop()
        if sock is not None:
            sock.close()
        self._stop.set()
        self._thread = _PumpThread(None)

    # -- line-pump path: lines are decoded on the thread that asks -------------

    @property
    def direct(self) -> bool:
        """True when events can be taken with :meth:`drain_events` on the
        consumer's own thread (the line-pump path)."""
        return self._pump is not None

    def seq(self) -> int:
        """Lines received so far; pass it to :meth:`wait_lines`.  Read it
        BEFORE :meth:`drain_events`, so a line that arrives in between ends
        the wait at once and is never slept through."""
        return self._pump.seq

    def wait_lines(self, seen_seq: int, timeout: Optional[float]) -> int:
        """Block (GIL released) until more than ``seen_seq`` lines have
        arrived, the stream has ended, or the timeout is up."""
        return self._pump.wait(seen_seq, timeout)

    def wait_ended(self, timeout: Optional[float]) -> bool:
        """Block until the stream has ended or the timeout is up."""
        self._pump.wait(_NEVER_SEQ, timeout)
        return self._pump.ended

    def ended(self) -> bool:
        return self._pump.ended

    def lines_pending(self) -> int:
        return self._pump.pending

    def drain_events(self) -> list:
        """Every event that has arrived and has not been handed out, oldest
        first, decoded here.  One consumer at a time (with :meth:`next`)."""
        out = list(self._ready)
        self._ready.clear()
        for line in self._pump.drain():
            try:
                event = json.loads(line)
            except ValueError:
                continue
            out.append((event.get("type"), event.get("object")))
        return out

    def next(self, timeout: Optional[float] = None):
        if self._pump is not None:
            return self._next_pumped(timeout)
        import queue

        try:
            return self._queue.get(timeout=timeout)
        except queue.Empty:
            return None

    def _next_pumped(self, timeout: Optional[float]):
        import time

        deadline = None if timeout is None else time.monotonic() + timeout
        ready = self._ready
        while not ready:
            seen = self._pump.seq
            ready.extend(self.drain_events())
            if ready:
                break
            remaining = None if deadline is None else deadline - time.monotonic()
            if remaining is not None and remaining <= 0:
                return None
            if self._pump.ended:
                if self._pump.pending:
                    continue  # the last lines raced the end of the stream
                # nothing will ever arrive: still honour the timeout, so a
                # polling consumer does not spin on a dropped stream
                self._stop.wait(remaining)
                return None
            self._pump.wait(seen, remaining)
        return ready.popleft()

    def stop(self) -> None:
        self._stop.set()
        sock = self._sock
        if self._pump is not None:
            import socket

            with self._stop_lock:
                sock, self._sock = self._sock, None
                if sock is None:
                    return
                try:
                    sock.shutdown(socket.SHUT_RDWR)  # wakes the pump's thread
                except OSError:
                    pass
                self._pump.stop()  # joined: the fd can no longer be in use
                sock.close()
            return
        if sock is not None:
            # wake the native reader; it closes the socket itself once it
            # has left readline
            import socket

            try:
                sock.shutdown(socket.SHUT_RDWR)
            except OSError:
                pass
        resp = self._resp
        if resp is not None:
            # close the stream so the blocked reader exits immediately
            # instead of waiting for the next keep-alive frame
            try:
                resp.close()
            except Exception:
                pass

    def alive(self) -> bool:
        """False once the HTTP stream has ended (server drop or stop)."""
        return self._thread.is_alive() and not self._stop.is_set()


#: a line count no stream reaches: LinePump.wait then returns only at the end
#: of the stream or at its timeout
_NEVER_SEQ = 2 ** 64 - 1


class _PumpThread:
    """``join`` / ``is_alive`` of ``threading.Thread`` over the native reader
    thread of a ``_wire.LinePump`` (None: it never started)."""

    def __init__(self, pump) -> None:
        self._pump = pump

    def is_alive(self) -> bool:
        return self._pump is not None and not self._pump.ended

    def join(self, timeout: Optional[float] = None) -> None:
        if self._pump is not None:
            self._pump.wait(_NEVER_SEQ, timeout)
