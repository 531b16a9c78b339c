// wire.cpp — native HTTP/1.1 wire path for the REST client and watch reader.
//
// Per-request wire overhead (request assembly, two sends, the header parse
// of the response, and the pure-Python line iteration of the watch stream)
// is where the cached-substrate reconcile loop spends its time
// (docs/performance.md).  This CPython extension does the framing natively
// on a socket the caller hands in:
//
//   exchange(fd, method, path, header_bytes, body, timeout)
//       -> (status, body_bytes, reusable)
//   Pool(host, port, max_idle, connect_timeout)
//       .checkout() -> (fd, reused), .checkin(fd, reusable)
//       keep-alive connections shared by all threads of a client: a thread
//       that lives for one request reuses what another left behind and
//       pays no dial (docs/performance.md)
//   LineReader(fd).read_head(timeout) -> status
//   LineReader(fd).readline(timeout)  -> bytes | None
//   parse_request_head(data)          -> None | (method, target, ...)
//     (the threaded apiserver's side of the same exchange)
//
// and carries a watch event from the write that caused it to the thread that
// waits for it without a Python thread in between (docs/performance.md):
//
//   StreamWriter(fd, max_backlog).write(line) -> bool
//       server side: the mutating thread sends the line itself; one native
//       thread per process drains what a full socket left behind
//   LinePump(fd | LineReader).wait(seen_seq, timeout) -> seq, .drain()
//       client side: one native thread per stream reads head and lines
//
// Rules: an fd passed in is borrowed and is never closed here, whether it
// belongs to a Python socket object or to a Pool.  The one exception to
// "never close" is the Pool: it opens its own fds and always closes them
// itself, at checkin(), close() or when it is freed, so that nobody else
// has to (or may).  Every wait is poll()+recv()/send()/connect() with the
// remaining deadline and with the GIL released; EINTR re-takes the GIL and
// runs signal handlers; the native threads never take the GIL.  Parsing
// and response framing live in wire_core.hpp, backlog, line framing and the
// pending-line queue in wire_stream.hpp (no Python, no sockets), the pool
// in wire_pool.hpp (sockets, no Python).

#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <poll.h>
#include <sys/socket.h>
#include <sys/types.h>
#include <unistd.h>

#include "wire_core.hpp"
#include "wire_pool.hpp"
#include "wire_stream.hpp"

namespace {

constexpr size_t kRecvBuf = 64 * 1024;

using Clock = std::chrono::steady_clock;

// Deadline helper: timeout < 0 means wait for ever.
struct Deadline {
  bool infinite;
  Clock::time_point at;

  explicit Deadline(double timeout_s) : infinite(timeout_s < 0) {
    if (!infinite)
      at = Clock::now() + std::chrono::duration_cast<Clock::duration>(
                              std::chrono::duration<double>(timeout_s));
  }

  // remaining milliseconds for poll(): -1 for ever, 0 when expired
  int remaining_ms() const {
    if (infinite) return -1;
    auto left = std::chrono::duration_cast<std::chrono::microseconds>(
                    at - Clock::now()).count();
    if (left <= 0) return 0;
    long long ms = (left + 999) / 1000;  // round up: never spin on 0 early
    return ms > 0x7fffffff ? 0x7fffffff : int(ms);
  }
};

// timeout argument: None -> -1 (for ever), number -> seconds (clamped >= 0)
bool parse_timeout(PyObject* obj, double* out) {
  if (obj == nullptr || obj == Py_None) {
    *out = -1.0;
    return true;
  }
  double v = PyFloat_AsDouble(obj);
  if (v == -1.0 && PyErr_Occurred()) return false;
  *out = v < 0 ? 0.0 : v;
  return true;
}

enum IoResult { kIoOk = 0, kIoTimeout = 1, kIoError = 2, kIoSignal = 3 };

// Wait until fd is ready for `events`, GIL released.  kIoSignal: a Python
// signal handler raised (exception set).
IoResult wait_fd(int fd, short events, const Deadline& dl) {
  for (;;) {
    int ms = dl.remaining_ms();
    struct pollfd p = {fd, events, 0};
    int rc, err;
    Py_BEGIN_ALLOW_THREADS
    rc = poll(&p, 1, ms);
    err = errno;
    Py_END_ALLOW_THREADS
    if (rc > 0) return kIoOk;  // readable/writable, or HUP/ERR: recv reports it
    if (rc == 0) {
      if (ms != 0 && dl.remaining_ms() != 0) continue;  // woke a hair early
      return kIoTimeout;
    }
    if (err == EINTR) {
      if (PyErr_CheckSignals() < 0) return kIoSignal;
      continue;
    }
    errno = err;
    PyErr_SetFromErrno(PyExc_OSError);
    return kIoError;
  }
}

// poll + recv into buf, both inside one GIL release.  *got = bytes read
// (0 = peer closed).
IoResult recv_some(int fd, char* buf, size_t cap, const Deadline& dl,
                   size_t* got) {
  for (;;) {
    int ms = dl.remaining_ms();
    struct pollfd p = {fd, POLLIN, 0};
    int rc, err;
    ssize_t n = -1;
    Py_BEGIN_ALLOW_THREADS
    rc = poll(&p, 1, ms);
    err = errno;
    if (rc > 0) {  // readable, or HUP/ERR: recv reports which
      n = recv(fd, buf, cap, MSG_DONTWAIT);
      err = errno;
    }
    Py_END_ALLOW_THREADS
    if (rc == 0) {
      if (ms != 0 && dl.remaining_ms() != 0) continue;  // woke a hair early
      return kIoTimeout;
    }
    if (n >= 0) {
      *got = size_t(n);
      return kIoOk;
    }
    if (rc > 0 && (err == EAGAIN || err == EWOULDBLOCK)) continue;
    if (err == EINTR) {
      if (PyErr_CheckSignals() < 0) return kIoSignal;
      continue;
    }
    errno = err;  // ECONNRESET/EPIPE map to ConnectionError subclasses
    PyErr_SetFromErrno(PyExc_OSError);
    return kIoError;
  }
}

IoResult send_all(int fd, const char* buf, size_t len, const Deadline& dl) {
  size_t off = 0;
  while (off < len) {
    ssize_t n;
    int err;
    Py_BEGIN_ALLOW_THREADS
    n = send(fd, buf + off, len - off, MSG_NOSIGNAL | MSG_DONTWAIT);
    err = errno;
    Py_END_ALLOW_THREADS
    if (n >= 0) {
      off += size_t(n);
      continue;
    }
    if (err == EAGAIN || err == EWOULDBLOCK) {
      IoResult w = wait_fd(fd, POLLOUT, dl);
      if (w != kIoOk) return w;
      continue;
    }
    if (err == EINTR) {
      if (PyErr_CheckSignals() < 0) return kIoSignal;
      continue;
    }
    errno = err;
    PyErr_SetFromErrno(PyExc_OSError);
    return kIoError;
  }
  return kIoOk;
}

PyObject* raise_wire_error(int st) {
  PyErr_SetString(PyExc_ValueError, wire::status_message(st));
  return nullptr;
}

PyObject* raise_timeout() {
  PyErr_SetString(PyExc_TimeoutError, "timed out");
  return nullptr;
}

// bytes | str | None  ->  pointer/length (str is UTF-8 encoded in place)
bool as_buffer(PyObject* obj, const char** p, Py_ssize_t* n, bool* present) {
  *present = true;
  if (obj == Py_None) {
    *p = "";
    *n = 0;
    *present = false;
    return true;
  }
  if (PyBytes_Check(obj)) {
    *p = PyBytes_AS_STRING(obj);
    *n = PyBytes_GET_SIZE(obj);
    return true;
  }
  if (PyUnicode_Check(obj)) {
    *p = PyUnicode_AsUTF8AndSize(obj, n);
    return *p != nullptr;
  }
  PyErr_SetString(PyExc_TypeError, "body must be bytes, str or None");
  return false;
}

// ---------------------------------------------------------------------------
// exchange
// ---------------------------------------------------------------------------

PyObject* py_exchange(PyObject* /*self*/, PyObject* args) {
  int fd;
  const char *method, *path, *head;
  Py_ssize_t method_len, path_len, head_len;
  PyObject *body_obj, *timeout_obj = Py_None;
  if (!PyArg_ParseTuple(args, "is#s#y#O|O", &fd, &method, &method_len, &path,
                        &path_len, &head, &head_len, &body_obj, &timeout_obj))
    return nullptr;
  const char* body;
  Py_ssize_t body_len;
  bool has_body;
  if (!as_buffer(body_obj, &body, &body_len, &has_body)) return nullptr;
  double timeout_s;
  if (!parse_timeout(timeout_obj, &timeout_s)) return nullptr;
  Deadline dl(timeout_s);

  std::string method_s(method, size_t(method_len));
  bool is_head = method_s == "HEAD";
  bool wants_length = has_body || method_s == "POST" || method_s == "PUT" ||
                      method_s == "PATCH";

  // one buffer, one send: request line + caller's header block + length + body
  std::string req;
  req.reserve(size_t(method_len + path_len + head_len + body_len) + 64);
  req.append(method_s).append(" ").append(path, size_t(path_len));
  req.append(" HTTP/1.1\r\n").append(head, size_t(head_len));
  if (wants_length)
    req.append("Content-Length: ").append(std::to_string(body_len)).append("\r\n");
  req.append("\r\n").append(body, size_t(body_len));

  IoResult io = send_all(fd, req.data(), req.size(), dl);
  if (io == kIoTimeout) return raise_timeout();
  if (io != kIoOk) return nullptr;

  wire::ResponseReader reader(is_head);
  char buf[kRecvBuf];  // on the stack: no allocation per request

  while (!reader.done()) {
    size_t got = 0;
    io = recv_some(fd, buf, sizeof buf, dl, &got);
    if (io == kIoTimeout) return raise_timeout();
    if (io != kIoOk) return nullptr;
    if (got == 0) {
      if (reader.peer_closed()) break;
      bool got_any = reader.started();
      PyErr_SetString(got_any ? PyExc_ConnectionError
                              : PyExc_ConnectionResetError,
                      got_any ? "peer closed the connection mid-response"
                              : "peer closed the connection without a response");
      return nullptr;
    }
    int st = reader.feed(buf, got);
    if (st < 0) return raise_wire_error(st);
  }

  const std::string& out = reader.body();
  PyObject* body_bytes =
      PyBytes_FromStringAndSize(out.data(), Py_ssize_t(out.size()));
  if (!body_bytes) return nullptr;
  PyObject* res = Py_BuildValue("(iNO)", reader.status(), body_bytes,
                                reader.reusable() ? Py_True : Py_False);
  return res;
}

// ---------------------------------------------------------------------------
// parse_request_head (server side)
// ---------------------------------------------------------------------------

PyObject* py_parse_request_head(PyObject* /*self*/, PyObject* arg) {
  Py_buffer view;
  if (PyObject_GetBuffer(arg, &view, PyBUF_SIMPLE) < 0) return nullptr;
  wire::HeadParser hp(wire::HeadParser::kRequest);
  size_t used = 0;
  int st = hp.feed(static_cast<const char*>(view.buf), size_t(view.len), &used);
  PyBuffer_Release(&view);
  if (st < 0) return raise_wire_error(st);
  if (st == wire::kNeedMore) Py_RETURN_NONE;
  PyObject* length;
  if (hp.has_content_length) {
    length = PyLong_FromSize_t(hp.content_length);
    if (!length) return nullptr;
  } else {
    length = Py_None;
    Py_INCREF(length);
  }
  return Py_BuildValue("(s#s#iNOOn)", hp.method.data(),
                       Py_ssize_t(hp.method.size()), hp.target.data(),
                       Py_ssize_t(hp.target.size()), hp.version_minor, length,
                       hp.chunked ? Py_True : Py_False,
                       hp.keep_alive() ? Py_True : Py_False,
                       Py_ssize_t(used));
}

// ---------------------------------------------------------------------------
// LineReader
// ---------------------------------------------------------------------------

struct LineReaderObject {
  PyObject_HEAD
  int fd;
  bool busy;  // a call is inside poll/recv with the GIL released, or a
              // LinePump's thread reads through this reader
  wire::LineFramer* framer;
  std::string* buf;  // recv buffer
};

void linereader_dealloc(LineReaderObject* self) {
  delete self->framer;
  delete self->buf;
  Py_TYPE(self)->tp_free(reinterpret_cast<PyObject*>(self));
}

int linereader_init(LineReaderObject* self, PyObject* args, PyObject* /*kw*/) {
  int fd;
  if (!PyArg_ParseTuple(args, "i", &fd)) return -1;
  if (self->framer != nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "LineReader is already initialised");
    return -1;
  }
  self->fd = fd;
  self->busy = false;
  try {
    self->framer = new wire::LineFramer();
    self->buf = new std::string(kRecvBuf, '\0');
  } catch (const std::bad_alloc&) {
    PyErr_NoMemory();
    return -1;
  }
  return 0;
}

// One poll+recv round.  Returns kIoOk (bytes consumed or the stream's end
// noted), kIoTimeout, or kIoError/kIoSignal with an exception set.
IoResult linereader_fill(LineReaderObject* self, const Deadline& dl) {
  size_t got = 0;
  self->busy = true;
  IoResult io = recv_some(self->fd, &(*self->buf)[0], self->buf->size(), dl,
                          &got);
  self->busy = false;
  if (io != kIoOk) return io;
  if (got == 0) {
    self->framer->peer_closed();
    return kIoOk;
  }
  try {
    int st = self->framer->consume(self->buf->data(), got);
    if (st < 0) {
      raise_wire_error(st);
      return kIoError;
    }
  } catch (const std::bad_alloc&) {
    PyErr_NoMemory();
    return kIoError;
  }
  return kIoOk;
}

bool linereader_enter(LineReaderObject* self) {
  if (self->framer == nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "LineReader is not initialised");
    return false;
  }
  if (self->busy) {
    PyErr_SetString(PyExc_RuntimeError,
                    "LineReader is in use by another thread");
    return false;
  }
  return true;
}

PyObject* linereader_read_head_impl(LineReaderObject* self, PyObject* args) {
  PyObject* timeout_obj = Py_None;
  if (!PyArg_ParseTuple(args, "|O", &timeout_obj)) return nullptr;
  if (!linereader_enter(self)) return nullptr;
  double timeout_s;
  if (!parse_timeout(timeout_obj, &timeout_s)) return nullptr;
  Deadline dl(timeout_s);
  while (!self->framer->head_done()) {
    if (self->framer->stream_end()) {
      PyErr_SetString(PyExc_ConnectionResetError,
                      "peer closed the connection without a response");
      return nullptr;
    }
    IoResult io = linereader_fill(self, dl);
    if (io == kIoTimeout) return raise_timeout();
    if (io != kIoOk) return nullptr;
  }
  return PyLong_FromLong(self->framer->status());
}

PyObject* linereader_readline_impl(LineReaderObject* self, PyObject* args) {
  PyObject* timeout_obj = Py_None;
  if (!PyArg_ParseTuple(args, "|O", &timeout_obj)) return nullptr;
  if (!linereader_enter(self)) return nullptr;
  double timeout_s;
  if (!parse_timeout(timeout_obj, &timeout_s)) return nullptr;
  Deadline dl(timeout_s);
  std::string line;
  for (;;) {
    int st = self->framer->next(&line);
    if (st == wire::kDone)
      return PyBytes_FromStringAndSize(line.data(), Py_ssize_t(line.size()));
    if (st < 0) return raise_wire_error(st);
    if (self->framer->stream_end()) {
      if (!self->framer->head_done()) {
        PyErr_SetString(PyExc_ConnectionResetError,
                        "peer closed the connection without a response");
        return nullptr;
      }
      PyErr_SetString(PyExc_EOFError, "stream ended");
      return nullptr;
    }
    IoResult io = linereader_fill(self, dl);
    if (io == kIoTimeout) Py_RETURN_NONE;
    if (io != kIoOk) return nullptr;
  }
}

// C++ allocation failures surface as MemoryError
PyObject* linereader_read_head(LineReaderObject* self, PyObject* args) {
  try {
    return linereader_read_head_impl(self, args);
  } catch (const std::bad_alloc&) {
    self->busy = false;
    return PyErr_NoMemory();
  }
}

PyObject* linereader_readline(LineReaderObject* self, PyObject* args) {
  try {
    return linereader_readline_impl(self, args);
  } catch (const std::bad_alloc&) {
    self->busy = false;
    return PyErr_NoMemory();
  }
}

PyObject* linereader_get_status(LineReaderObject* self, void*) {
  if (self->framer == nullptr || !self->framer->head_done()) Py_RETURN_NONE;
  return PyLong_FromLong(self->framer->status());
}

PyObject* linereader_get_chunked(LineReaderObject* self, void*) {
  if (self->framer == nullptr || !self->framer->head_done()) Py_RETURN_NONE;
  return PyBool_FromLong(self->framer->chunked());
}

PyMethodDef linereader_methods[] = {
    {"read_head", reinterpret_cast<PyCFunction>(linereader_read_head),
     METH_VARARGS,
     "read_head(timeout=None) -> status.  Consume the response head (1xx "
     "interim responses skipped); TimeoutError on deadline."},
    {"readline", reinterpret_cast<PyCFunction>(linereader_readline),
     METH_VARARGS,
     "readline(timeout=None) -> bytes | None.  Next non-blank line of the "
     "body (read-until-close, chunked or Content-Length framing); None on "
     "timeout; EOFError once the stream has ended."},
    {nullptr, nullptr, 0, nullptr},
};

PyGetSetDef linereader_getset[] = {
    {"status", reinterpret_cast<getter>(linereader_get_status), nullptr,
     "HTTP status once the head has been read, else None", nullptr},
    {"chunked", reinterpret_cast<getter>(linereader_get_chunked), nullptr,
     "True when the body uses chunked framing (None before the head)",
     nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr},
};

PyTypeObject LineReaderType = {
    PyVarObject_HEAD_INIT(nullptr, 0)
    "_wire.LineReader",           /* tp_name */
    sizeof(LineReaderObject),     /* tp_basicsize */
};

// ---------------------------------------------------------------------------
// LinePump (client side of a watch stream)
// ---------------------------------------------------------------------------

// What the pump's thread works on.  The framer and the recv buffer belong
// to the LineReader the pump holds a reference to; the thread is joined
// before that reference is dropped.
struct PumpState {
  int fd = -1;
  int wake[2] = {-1, -1};  // stop() writes, the thread polls the read end
  wire::LineFramer* framer = nullptr;
  std::string* buf = nullptr;
  wire::LineQueue queue;
};

// The reader thread: head, then lines, into the queue.  Never takes the GIL.
void pump_run(PumpState* st) {
  int error = 0;
  bool head_published = false;
  try {
    std::string line;
    for (;;) {
      struct pollfd p[2] = {{st->fd, POLLIN, 0}, {st->wake[0], POLLIN, 0}};
      if (poll(p, 2, -1) < 0) {
        if (errno == EINTR) continue;
        error = errno;
        break;
      }
      if (p[1].revents) break;  // stop()
      ssize_t n = recv(st->fd, &(*st->buf)[0], st->buf->size(), MSG_DONTWAIT);
      if (n < 0) {
        if (errno == EAGAIN || errno == EWOULDBLOCK || errno == EINTR) continue;
        error = errno;
        break;
      }
      int bad = 0;
      if (n == 0) {
        st->framer->peer_closed();
      } else {
        bad = st->framer->consume(st->buf->data(), size_t(n));
      }
      // what arrived whole before a framing error is still handed out
      if (!head_published && st->framer->head_done()) {
        st->queue.set_head(st->framer->status());
        head_published = true;
      }
      int rc;
      while ((rc = st->framer->next(&line)) == wire::kDone)
        st->queue.push(std::move(line));
      if (bad < 0 || rc < 0) {
        error = bad < 0 ? bad : rc;
        break;
      }
      if (st->framer->stream_end()) break;
    }
  } catch (const std::bad_alloc&) {
    error = ENOMEM;
  }
  st->queue.end(error);  // the thread's last use of the fd is behind it
}

struct LinePumpObject {
  PyObject_HEAD
  PyObject* reader;  // the LineReader whose framing state the thread drives
  PumpState* st;
  std::thread* thread;
  bool joined;
};

// seen_seq that no stream reaches: wait() then returns only at the end of
// the stream or at the timeout
constexpr unsigned long long kNeverSeq = ~0ULL;

void linepump_join(LinePumpObject* self, bool release_gil) {
  if (self->thread == nullptr) return;
  if (self->joined) {
    // another caller is joining, or has: the queue's end is the thread's
    // last act, so waiting for it is as good
    if (release_gil) {
      Py_BEGIN_ALLOW_THREADS
      self->st->queue.wait(kNeverSeq, -1.0);
      Py_END_ALLOW_THREADS
    } else {
      self->st->queue.wait(kNeverSeq, -1.0);
    }
    return;
  }
  self->joined = true;
  char c = 0;
  ssize_t rc = write(self->st->wake[1], &c, 1);
  (void)rc;
  if (release_gil) {
    Py_BEGIN_ALLOW_THREADS
    self->thread->join();
    Py_END_ALLOW_THREADS
  } else {
    self->thread->join();
  }
}

void linepump_dealloc(LinePumpObject* self) {
  if (self->st != nullptr) {
    linepump_join(self, false);
    delete self->thread;
    if (self->st->wake[0] >= 0) close(self->st->wake[0]);
    if (self->st->wake[1] >= 0) close(self->st->wake[1]);
    delete self->st;
  }
  Py_XDECREF(self->reader);
  Py_TYPE(self)->tp_free(reinterpret_cast<PyObject*>(self));
}

int linepump_init(LinePumpObject* self, PyObject* args, PyObject* /*kw*/) {
  PyObject* source;
  if (!PyArg_ParseTuple(args, "O", &source)) return -1;
  if (self->st != nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "LinePump is already initialised");
    return -1;
  }
  PyObject* reader;
  if (PyObject_TypeCheck(source, &LineReaderType)) {
    reader = source;
    Py_INCREF(reader);
  } else {
    reader = PyObject_CallFunctionObjArgs(
        reinterpret_cast<PyObject*>(&LineReaderType), source, nullptr);
    if (reader == nullptr) return -1;
  }
  LineReaderObject* lr = reinterpret_cast<LineReaderObject*>(reader);
  if (!linereader_enter(lr)) {
    Py_DECREF(reader);
    return -1;
  }
  PumpState* st = nullptr;
  try {
    st = new PumpState();
    st->fd = lr->fd;
    st->framer = lr->framer;
    st->buf = lr->buf;
    if (pipe2(st->wake, O_NONBLOCK | O_CLOEXEC) != 0) {
      PyErr_SetFromErrno(PyExc_OSError);
      delete st;
      Py_DECREF(reader);
      return -1;
    }
    lr->busy = true;  // for good: the reader is the thread's from now on
    self->reader = reader;
    self->st = st;
    self->joined = false;
    self->thread = new std::thread(pump_run, st);
  } catch (const std::exception&) {  // bad_alloc, or no thread to be had
    if (self->st == nullptr) {
      delete st;
      Py_DECREF(reader);
    } else {
      st->queue.end(EAGAIN);  // dealloc tidies up; nothing was started
    }
    PyErr_SetString(PyExc_RuntimeError, "LinePump could not start its thread");
    return -1;
  }
  return 0;
}

bool linepump_enter(LinePumpObject* self) {
  if (self->st == nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "LinePump is not initialised");
    return false;
  }
  return true;
}

// Run `step(seconds)` (GIL released) in slices of at most a second until
// `done()` or the deadline, looking for signals in between.  False with an
// exception set when a signal handler raised.
template <class Step, class Done>
bool linepump_wait_sliced(double timeout_s, Step step, Done done) {
  Deadline dl(timeout_s);
  for (;;) {
    int ms = dl.remaining_ms();
    double slice = ms < 0 || ms > 1000 ? 1.0 : double(ms) / 1000.0;
    Py_BEGIN_ALLOW_THREADS
    step(slice);
    Py_END_ALLOW_THREADS
    if (done() || dl.remaining_ms() == 0) return true;
    if (PyErr_CheckSignals() < 0) return false;
  }
}

PyObject* linepump_read_head(LinePumpObject* self, PyObject* args) {
  PyObject* timeout_obj = Py_None;
  if (!PyArg_ParseTuple(args, "|O", &timeout_obj)) return nullptr;
  if (!linepump_enter(self)) return nullptr;
  double timeout_s;
  if (!parse_timeout(timeout_obj, &timeout_s)) return nullptr;
  wire::LineQueue& q = self->st->queue;
  int status = 0;
  if (!linepump_wait_sliced(
          timeout_s, [&](double s) { status = q.wait_head(s); },
          [&] { return status != 0 || q.ended(); }))
    return nullptr;
  if (status != 0) return PyLong_FromLong(status);
  if (!q.ended()) return raise_timeout();
  int error = q.error();
  if (error < 0) return raise_wire_error(error);
  if (error > 0) {
    errno = error;
    return PyErr_SetFromErrno(PyExc_OSError);
  }
  PyErr_SetString(PyExc_ConnectionResetError,
                  "peer closed the connection without a response");
  return nullptr;
}

PyObject* linepump_wait(LinePumpObject* self, PyObject* args) {
  unsigned long long seen;
  PyObject* timeout_obj = Py_None;
  if (!PyArg_ParseTuple(args, "K|O", &seen, &timeout_obj)) return nullptr;
  if (!linepump_enter(self)) return nullptr;
  double timeout_s;
  if (!parse_timeout(timeout_obj, &timeout_s)) return nullptr;
  wire::LineQueue& q = self->st->queue;
  uint64_t seq = 0;
  if (!linepump_wait_sliced(
          timeout_s, [&](double s) { seq = q.wait(seen, s); },
          [&] { return seq > seen || q.ended(); }))
    return nullptr;
  return PyLong_FromUnsignedLongLong(seq);
}

PyObject* linepump_drain(LinePumpObject* self, PyObject*) {
  if (!linepump_enter(self)) return nullptr;
  try {
    std::deque<std::string> lines = self->st->queue.drain();
    PyObject* out = PyList_New(Py_ssize_t(lines.size()));
    if (!out) return nullptr;
    Py_ssize_t i = 0;
    for (const std::string& line : lines) {
      PyObject* b =
          PyBytes_FromStringAndSize(line.data(), Py_ssize_t(line.size()));
      if (!b) {
        Py_DECREF(out);
        return nullptr;
      }
      PyList_SET_ITEM(out, i++, b);
    }
    return out;
  } catch (const std::bad_alloc&) {
    return PyErr_NoMemory();
  }
}

PyObject* linepump_stop(LinePumpObject* self, PyObject*) {
  if (!linepump_enter(self)) return nullptr;
  linepump_join(self, true);
  Py_RETURN_NONE;
}

PyObject* linepump_get_seq(LinePumpObject* self, void*) {
  if (!linepump_enter(self)) return nullptr;
  return PyLong_FromUnsignedLongLong(self->st->queue.seq());
}

PyObject* linepump_get_pending(LinePumpObject* self, void*) {
  if (!linepump_enter(self)) return nullptr;
  return PyLong_FromSize_t(self->st->queue.pending());
}

PyObject* linepump_get_ended(LinePumpObject* self, void*) {
  if (!linepump_enter(self)) return nullptr;
  return PyBool_FromLong(self->st->queue.ended());
}

PyObject* linepump_get_error(LinePumpObject* self, void*) {
  if (!linepump_enter(self)) return nullptr;
  int error = self->st->queue.error();
  if (error == 0) Py_RETURN_NONE;
  return PyUnicode_FromString(error < 0 ? wire::status_message(error)
                                        : std::strerror(error));
}

PyMethodDef linepump_methods[] = {
    {"read_head", reinterpret_cast<PyCFunction>(linepump_read_head),
     METH_VARARGS,
     "read_head(timeout=None) -> status.  Wait for the response head; "
     "TimeoutError on deadline, ConnectionResetError, OSError or ValueError "
     "when the stream ended before it."},
    {"wait", reinterpret_cast<PyCFunction>(linepump_wait), METH_VARARGS,
     "wait(seen_seq, timeout=None) -> seq.  Return once more than seen_seq "
     "lines have arrived, the stream has ended, or the timeout is up.  The "
     "GIL is released while waiting; every waiter is woken."},
    {"drain", reinterpret_cast<PyCFunction>(linepump_drain), METH_NOARGS,
     "drain() -> list[bytes].  Every pending line, oldest first."},
    {"stop", reinterpret_cast<PyCFunction>(linepump_stop), METH_NOARGS,
     "stop().  End the reader thread and join it (GIL released).  On return "
     "nothing native uses the fd any more: close the socket only now."},
    {nullptr, nullptr, 0, nullptr},
};

PyGetSetDef linepump_getset[] = {
    {"seq", reinterpret_cast<getter>(linepump_get_seq), nullptr,
     "lines received so far", nullptr},
    {"pending", reinterpret_cast<getter>(linepump_get_pending), nullptr,
     "lines received and not yet drained", nullptr},
    {"ended", reinterpret_cast<getter>(linepump_get_ended), nullptr,
     "True once the stream is over: body complete, peer closed, framing "
     "error, read error or stop()", nullptr},
    {"error", reinterpret_cast<getter>(linepump_get_error), nullptr,
     "why the stream ended, None for a clean end", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr},
};

PyTypeObject LinePumpType = {
    PyVarObject_HEAD_INIT(nullptr, 0)
    "_wire.LinePump",             /* tp_name */
    sizeof(LinePumpObject),       /* tp_basicsize */
};

// ---------------------------------------------------------------------------
// StreamWriter (server side of a watch stream)
// ---------------------------------------------------------------------------

// One stream's fd and backlog, shared between its StreamWriter and the
// flusher so that neither can outlive the other's use of it.
struct Stream {
  Stream(int fd_, size_t max_backlog) : fd(fd_), buf(max_backlog) {}

  long send_some(const char* p, size_t n) const {
    for (;;) {
      ssize_t rc = send(fd, p, n, MSG_DONTWAIT | MSG_NOSIGNAL);
      if (rc >= 0) return long(rc);
      if (errno == EINTR) continue;
      if (errno == EAGAIN || errno == EWOULDBLOCK) return wire::kSendWouldBlock;
      return wire::kSendFailed;
    }
  }

  // the peer learns of a dead stream at once; the fd itself stays open
  void on_dead() {
    if (!shut.exchange(true)) shutdown(fd, SHUT_RDWR);
  }

  const int fd;
  wire::StreamBuffer buf;
  std::atomic<bool> shut{false};
};

// The process's one flusher thread: drains backlogs when their sockets
// report POLLOUT.  It never touches Python.  `mu_` is held across a flush
// and across detach(), so once detach() has returned the thread does not
// use that stream's fd again.
class Flusher {
 public:
  static Flusher& instance() {
    static Flusher* self = new Flusher();  // never destroyed: no exit races
    return *self;
  }

  // `s` has a backlog: watch its fd from now on
  bool attach(const std::shared_ptr<Stream>& s) {
    std::lock_guard<std::mutex> hold(mu_);
    if (!ensure_started()) return false;
    for (const auto& have : active_)
      if (have == s) return true;
    active_.push_back(s);
    wake();
    return true;
  }

  void detach(const std::shared_ptr<Stream>& s) {
    std::lock_guard<std::mutex> hold(mu_);
    for (size_t i = 0; i < active_.size(); ++i) {
      if (active_[i] == s) {
        active_.erase(active_.begin() + long(i));
        wake();
        break;
      }
    }
  }

 private:
  Flusher() = default;

  bool ensure_started() {  // mu_ held
    if (started_) return true;
    if (pipe2(wake_, O_NONBLOCK | O_CLOEXEC) != 0) return false;
    try {
      std::thread(&Flusher::run, this).detach();
    } catch (const std::system_error&) {
      close(wake_[0]);
      close(wake_[1]);
      return false;
    }
    started_ = true;
    return true;
  }

  void wake() {
    char c = 0;
    ssize_t rc = write(wake_[1], &c, 1);  // a full pipe is already a wake-up
    (void)rc;
  }

  void run() {
    std::vector<std::shared_ptr<Stream>> watched;
    std::vector<struct pollfd> fds;
    for (;;) {
      {
        std::lock_guard<std::mutex> hold(mu_);
        watched = active_;
      }
      fds.clear();
      fds.push_back({wake_[0], POLLIN, 0});
      for (const auto& s : watched) fds.push_back({s->fd, POLLOUT, 0});
      if (poll(fds.data(), nfds_t(fds.size()), -1) < 0) continue;  // EINTR
      if (fds[0].revents) {
        char sink[64];
        while (read(wake_[0], sink, sizeof sink) > 0) {
        }
      }
      for (size_t i = 0; i < watched.size(); ++i) {
        if (!fds[i + 1].revents) continue;
        const std::shared_ptr<Stream>& s = watched[i];
        std::lock_guard<std::mutex> hold(mu_);
        size_t at = 0;
        while (at < active_.size() && active_[at] != s) ++at;
        if (at == active_.size()) continue;  // detached while we polled
        Stream* raw = s.get();
        auto st = raw->buf.flush(
            [raw](const char* p, size_t n) { return raw->send_some(p, n); });
        if (st == wire::StreamBuffer::kQueued) continue;
        if (st == wire::StreamBuffer::kDead) raw->on_dead();
        active_.erase(active_.begin() + long(at));
      }
    }
  }

  std::mutex mu_;
  std::vector<std::shared_ptr<Stream>> active_;
  bool started_ = false;
  int wake_[2] = {-1, -1};
};

// Default backlog cap: 64 MiB.  The replay that opens a watch (resume
// history or the initial events of a whole kind) is written in one go under
// the cluster lock and has to fit; 64 MiB is also the cap on a single line
// (wire::kMaxLine), so no legal stream is refused for its first line.  A
// reader that falls further behind than that is cut off and re-watches.
constexpr size_t kDefaultMaxBacklog = wire::kMaxLine;

struct StreamWriterObject {
  PyObject_HEAD
  std::shared_ptr<Stream>* stream;
  bool closed;
};

void streamwriter_dealloc(StreamWriterObject* self) {
  if (self->stream != nullptr) {
    if (!self->closed) Flusher::instance().detach(*self->stream);
    delete self->stream;
  }
  Py_TYPE(self)->tp_free(reinterpret_cast<PyObject*>(self));
}

int streamwriter_init(StreamWriterObject* self, PyObject* args,
                      PyObject* /*kw*/) {
  int fd;
  Py_ssize_t max_backlog = Py_ssize_t(kDefaultMaxBacklog);
  if (!PyArg_ParseTuple(args, "i|n", &fd, &max_backlog)) return -1;
  if (self->stream != nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "StreamWriter is already initialised");
    return -1;
  }
  if (fd < 0 || max_backlog < 0) {
    PyErr_SetString(PyExc_ValueError, "fd and max_backlog must be >= 0");
    return -1;
  }
  try {
    self->stream = new std::shared_ptr<Stream>(
        std::make_shared<Stream>(fd, size_t(max_backlog)));
  } catch (const std::bad_alloc&) {
    PyErr_NoMemory();
    return -1;
  }
  self->closed = false;
  return 0;
}

// Never raises for a stream that cannot take the data: the caller is a
// cluster mutation that must go through whatever its watchers do.
PyObject* streamwriter_write(StreamWriterObject* self, PyObject* arg) {
  if (self->stream == nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "StreamWriter is not initialised");
    return nullptr;
  }
  Py_buffer view;
  if (PyObject_GetBuffer(arg, &view, PyBUF_SIMPLE) < 0) return nullptr;
  bool ok = false;
  if (!self->closed) {
    const std::shared_ptr<Stream>& s = *self->stream;
    Stream* raw = s.get();
    try {
      // send() is non-blocking, so the GIL stays held: releasing it would
      // invite the thread switch this path exists to avoid
      auto st = raw->buf.write(
          static_cast<const char*>(view.buf), size_t(view.len),
          [raw](const char* p, size_t n) { return raw->send_some(p, n); });
      if (st == wire::StreamBuffer::kQueued && !Flusher::instance().attach(s)) {
        raw->buf.kill();  // no flusher thread: the backlog would never drain
        st = wire::StreamBuffer::kDead;
      }
      if (st == wire::StreamBuffer::kDead) raw->on_dead();
      ok = st != wire::StreamBuffer::kDead;
    } catch (const std::bad_alloc&) {
      raw->buf.kill();
      raw->on_dead();
    }
  }
  PyBuffer_Release(&view);
  return PyBool_FromLong(ok);
}

PyObject* streamwriter_close(StreamWriterObject* self, PyObject*) {
  if (self->stream != nullptr && !self->closed) {
    self->closed = true;
    Flusher::instance().detach(*self->stream);
  }
  Py_RETURN_NONE;
}

PyObject* streamwriter_get_dead(StreamWriterObject* self, void*) {
  if (self->stream == nullptr) Py_RETURN_TRUE;
  return PyBool_FromLong(self->closed || (*self->stream)->buf.dead());
}

PyObject* streamwriter_get_pending(StreamWriterObject* self, void*) {
  if (self->stream == nullptr) return PyLong_FromLong(0);
  return PyLong_FromSize_t((*self->stream)->buf.pending());
}

PyMethodDef streamwriter_methods[] = {
    {"write", reinterpret_cast<PyCFunction>(streamwriter_write), METH_O,
     "write(data) -> bool.  Thread-safe, never blocks, never raises for a "
     "broken stream.  With nothing queued the bytes are sent on the calling "
     "thread; what the socket does not take waits in the backlog, which one "
     "native thread per process drains on POLLOUT.  Each call's bytes reach "
     "the peer contiguously.  False once the writer is dead or closed."},
    {"close", reinterpret_cast<PyCFunction>(streamwriter_close), METH_NOARGS,
     "close().  Detach from the flusher thread; on return nothing native "
     "uses the fd any more.  Unsent backlog is dropped."},
    {nullptr, nullptr, 0, nullptr},
};

PyGetSetDef streamwriter_getset[] = {
    {"dead", reinterpret_cast<getter>(streamwriter_get_dead), nullptr,
     "True after a send error, a backlog past max_backlog (the socket is "
     "then shut down, not closed) or close()", nullptr},
    {"pending", reinterpret_cast<getter>(streamwriter_get_pending), nullptr,
     "bytes waiting in the backlog", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr},
};

PyTypeObject StreamWriterType = {
    PyVarObject_HEAD_INIT(nullptr, 0)
    "_wire.StreamWriter",         /* tp_name */
    sizeof(StreamWriterObject),   /* tp_basicsize */
};

// ---------------------------------------------------------------------------
// Pool (keep-alive connections shared by every thread of a client)
// ---------------------------------------------------------------------------

struct PoolObject {
  PyObject_HEAD
  wire::Pool* pool;
};

void pool_dealloc(PoolObject* self) {
  delete self->pool;  // closes the idle fds
  Py_TYPE(self)->tp_free(reinterpret_cast<PyObject*>(self));
}

int pool_init(PoolObject* self, PyObject* args, PyObject* kw) {
  static const char* names[] = {"host", "port", "max_idle", "connect_timeout",
                                nullptr};
  const char* host;
  int port;
  Py_ssize_t max_idle = 8;
  PyObject* timeout_obj = Py_None;
  if (!PyArg_ParseTupleAndKeywords(args, kw, "si|nO",
                                   const_cast<char**>(names), &host, &port,
                                   &max_idle, &timeout_obj))
    return -1;
  if (self->pool != nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "Pool is already initialised");
    return -1;
  }
  if (port < 0 || port > 65535 || max_idle < 0) {
    PyErr_SetString(PyExc_ValueError,
                    "port must be 0..65535 and max_idle >= 0");
    return -1;
  }
  double timeout_s;
  if (!parse_timeout(timeout_obj, &timeout_s)) return -1;
  try {
    self->pool = new wire::Pool(host, port, size_t(max_idle), timeout_s);
  } catch (const std::bad_alloc&) {
    PyErr_NoMemory();
    return -1;
  }
  return 0;
}

bool pool_enter(PoolObject* self) {
  if (self->pool == nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "Pool is not initialised");
    return false;
  }
  return true;
}

// a signal interrupted the dial: take the GIL back and run the handlers
bool pool_on_eintr(void*) {
  PyGILState_STATE gil = PyGILState_Ensure();
  bool go_on = PyErr_CheckSignals() == 0;
  PyGILState_Release(gil);
  return go_on;
}

PyObject* pool_checkout_impl(PoolObject* self, PyObject* args) {
  int fresh = 0;
  if (!PyArg_ParseTuple(args, "|p", &fresh)) return nullptr;
  if (!pool_enter(self)) return nullptr;
  // the idle list first: a mutex and a zero-timeout poll, nothing to wait for
  wire::Pool::Lease lease;
  if (!fresh) lease = self->pool->take_idle();
  if (lease.fd < 0 && lease.error == wire::Pool::kOk) {
    Py_BEGIN_ALLOW_THREADS
    lease = self->pool->dial(pool_on_eintr, nullptr);
    Py_END_ALLOW_THREADS
  }
  switch (lease.error) {
    case wire::Pool::kOk:
      return Py_BuildValue("(iO)", lease.fd,
                           lease.reused ? Py_True : Py_False);
    case wire::Pool::kClosed:
      PyErr_SetString(PyExc_RuntimeError, "Pool is closed");
      return nullptr;
    case wire::Pool::kResolve: {
      PyObject* gaierror = nullptr;
      PyObject* mod = PyImport_ImportModule("socket");
      if (mod != nullptr) {
        gaierror = PyObject_GetAttrString(mod, "gaierror");
        Py_DECREF(mod);
      }
      if (gaierror == nullptr) return nullptr;
      PyObject* val = Py_BuildValue("(is)", lease.code, gai_strerror(lease.code));
      if (val != nullptr) {
        PyErr_SetObject(gaierror, val);  // an OSError subclass
        Py_DECREF(val);
      }
      Py_DECREF(gaierror);
      return nullptr;
    }
    case wire::Pool::kTimeout:
      return raise_timeout();
    case wire::Pool::kInterrupted:
      return nullptr;  // the signal handler's exception is set
    default:
      errno = lease.code;
      return PyErr_SetFromErrno(PyExc_OSError);
  }
}

PyObject* pool_checkout(PoolObject* self, PyObject* args) {
  try {
    return pool_checkout_impl(self, args);
  } catch (const std::bad_alloc&) {
    return PyErr_NoMemory();
  }
}

PyObject* pool_checkin(PoolObject* self, PyObject* args) {
  int fd, reusable;
  if (!PyArg_ParseTuple(args, "ip", &fd, &reusable)) return nullptr;
  if (!pool_enter(self)) return nullptr;
  try {
    self->pool->checkin(fd, reusable != 0);
  } catch (const std::bad_alloc&) {
    close(fd);  // the idle list could not grow: the fd is still the pool's
  }
  Py_RETURN_NONE;
}

PyObject* pool_close(PoolObject* self, PyObject*) {
  if (!pool_enter(self)) return nullptr;
  self->pool->close();
  Py_RETURN_NONE;
}

PyObject* pool_stats(PoolObject* self, PyObject*) {
  if (!pool_enter(self)) return nullptr;
  wire::PoolStats st = self->pool->stats();
  return Py_BuildValue("{s:K,s:K,s:K,s:n}", "dials",
                       static_cast<unsigned long long>(st.dials), "reuses",
                       static_cast<unsigned long long>(st.reuses),
                       "stale_discards",
                       static_cast<unsigned long long>(st.stale_discards),
                       "idle", Py_ssize_t(st.idle));
}

PyObject* pool_get_max_idle(PoolObject* self, void*) {
  if (!pool_enter(self)) return nullptr;
  return PyLong_FromSize_t(self->pool->max_idle());
}

PyObject* pool_get_closed(PoolObject* self, void*) {
  if (!pool_enter(self)) return nullptr;
  return PyBool_FromLong(self->pool->closed());
}

PyMethodDef pool_methods[] = {
    {"checkout", reinterpret_cast<PyCFunction>(pool_checkout), METH_VARARGS,
     "checkout(fresh=False) -> (fd, reused).  The most recently used idle "
     "connection that is still quiet (reused=True), else (or with fresh) a "
     "new one, dialled with the GIL released.  The fd stays the pool's: pass it to exchange() and "
     "give it back with checkin(), exactly once, never close it.  OSError "
     "(TimeoutError, socket.gaierror) when the dial fails; RuntimeError "
     "once the pool is closed."},
    {"checkin", reinterpret_cast<PyCFunction>(pool_checkin), METH_VARARGS,
     "checkin(fd, reusable).  Give a checked-out fd back.  It is kept for "
     "the next checkout() only when reusable is true (the response was "
     "complete and exchange() said reusable), the pool is open and fewer "
     "than max_idle are idle; otherwise the pool closes it."},
    {"close", reinterpret_cast<PyCFunction>(pool_close), METH_NOARGS,
     "close().  Close the idle connections; one checked out now is closed "
     "when it comes back.  checkout() raises from here on."},
    {"stats", reinterpret_cast<PyCFunction>(pool_stats), METH_NOARGS,
     "stats() -> {'dials', 'reuses', 'stale_discards', 'idle'}."},
    {nullptr, nullptr, 0, nullptr},
};

PyGetSetDef pool_getset[] = {
    {"max_idle", reinterpret_cast<getter>(pool_get_max_idle), nullptr,
     "most connections kept idle", nullptr},
    {"closed", reinterpret_cast<getter>(pool_get_closed), nullptr,
     "True after close()", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr},
};

PyTypeObject PoolType = {
    PyVarObject_HEAD_INIT(nullptr, 0)
    "_wire.Pool",                 /* tp_name */
    sizeof(PoolObject),           /* tp_basicsize */
};

// ---------------------------------------------------------------------------
// module
// ---------------------------------------------------------------------------

// C++ allocation failures inside exchange() surface as MemoryError
PyObject* py_exchange_guarded(PyObject* self, PyObject* args) {
  try {
    return py_exchange(self, args);
  } catch (const std::bad_alloc&) {
    return PyErr_NoMemory();
  }
}

PyObject* py_parse_request_head_guarded(PyObject* self, PyObject* arg) {
  try {
    return py_parse_request_head(self, arg);
  } catch (const std::bad_alloc&) {
    return PyErr_NoMemory();
  }
}

PyMethodDef wire_methods[] = {
    {"exchange", py_exchange_guarded, METH_VARARGS,
     "exchange(fd, method, path, header_bytes, body, timeout=None) -> "
     "(status, body_bytes, reusable).  One HTTP/1.1 request/response on a "
     "connected socket: the request goes out in a single send; the response "
     "is read with Content-Length, chunked or read-to-EOF framing.  "
     "reusable is False when the connection must not carry another request."},
    {"parse_request_head", py_parse_request_head_guarded, METH_O,
     "parse_request_head(data) -> None | (method, target, minor_version, "
     "content_length | None, chunked, keep_alive, head_size).  None while "
     "the head is incomplete; ValueError when it is malformed."},
    {nullptr, nullptr, 0, nullptr},
};

struct PyModuleDef wire_module = {
    PyModuleDef_HEAD_INIT, "_wire",
    "Native HTTP/1.1 framing for the REST client and the watch reader", -1,
    wire_methods,
};

}  // namespace

PyMODINIT_FUNC PyInit__wire(void) {
  LineReaderType.tp_flags = Py_TPFLAGS_DEFAULT;
  LineReaderType.tp_doc =
      "LineReader(fd): newline-delimited reader over a streaming HTTP "
      "response on a socket the caller owns (never closed here).";
  LineReaderType.tp_new = PyType_GenericNew;
  LineReaderType.tp_init = reinterpret_cast<initproc>(linereader_init);
  LineReaderType.tp_dealloc = reinterpret_cast<destructor>(linereader_dealloc);
  LineReaderType.tp_methods = linereader_methods;
  LineReaderType.tp_getset = linereader_getset;
  if (PyType_Ready(&LineReaderType) < 0) return nullptr;
  StreamWriterType.tp_flags = Py_TPFLAGS_DEFAULT;
  StreamWriterType.tp_doc =
      "StreamWriter(fd, max_backlog=64 MiB): non-blocking, thread-safe line "
      "writer over a socket the caller owns (never closed here).  The "
      "default cap holds the replay that opens a watch, which is written in "
      "one go, and equals the 64 MiB cap on a single line; a reader further "
      "behind than that is cut off and re-watches.";
  StreamWriterType.tp_new = PyType_GenericNew;
  StreamWriterType.tp_init = reinterpret_cast<initproc>(streamwriter_init);
  StreamWriterType.tp_dealloc =
      reinterpret_cast<destructor>(streamwriter_dealloc);
  StreamWriterType.tp_methods = streamwriter_methods;
  StreamWriterType.tp_getset = streamwriter_getset;
  if (PyType_Ready(&StreamWriterType) < 0) return nullptr;
  LinePumpType.tp_flags = Py_TPFLAGS_DEFAULT;
  LinePumpType.tp_doc =
      "LinePump(fd | LineReader): one native thread reads the response head "
      "and then lines from a socket the caller owns, without ever taking "
      "the GIL; consumers wait() for the line count to move and drain().  "
      "Given a LineReader, the thread reads through it and the reader is "
      "the pump's from then on.  To end it: shut the socket down, stop(), "
      "and only then close the socket.";
  LinePumpType.tp_new = PyType_GenericNew;
  LinePumpType.tp_init = reinterpret_cast<initproc>(linepump_init);
  LinePumpType.tp_dealloc = reinterpret_cast<destructor>(linepump_dealloc);
  LinePumpType.tp_methods = linepump_methods;
  LinePumpType.tp_getset = linepump_getset;
  if (PyType_Ready(&LinePumpType) < 0) return nullptr;
  PoolType.tp_flags = Py_TPFLAGS_DEFAULT;
  PoolType.tp_doc =
      "Pool(host, port, max_idle=8, connect_timeout=None): keep-alive "
      "connections to one plain-HTTP endpoint, shared by every thread.  The "
      "pool opens its sockets itself and is the only one to close them; "
      "checkout() lends an fd to one exchange() at a time.  A forked child "
      "starts with an empty pool.";
  PoolType.tp_new = PyType_GenericNew;
  PoolType.tp_init = reinterpret_cast<initproc>(pool_init);
  PoolType.tp_dealloc = reinterpret_cast<destructor>(pool_dealloc);
  PoolType.tp_methods = pool_methods;
  PoolType.tp_getset = pool_getset;
  if (PyType_Ready(&PoolType) < 0) return nullptr;
  PyObject* m = PyModule_Create(&wire_module);
  if (!m) return nullptr;
  Py_INCREF(&PoolType);
  if (PyModule_AddObject(m, "Pool",
                         reinterpret_cast<PyObject*>(&PoolType)) < 0) {
    Py_DECREF(&PoolType);
    Py_DECREF(m);
    return nullptr;
  }
  Py_INCREF(&LinePumpType);
  if (PyModule_AddObject(m, "LinePump",
                         reinterpret_cast<PyObject*>(&LinePumpType)) < 0) {
    Py_DECREF(&LinePumpType);
    Py_DECREF(m);
    return nullptr;
  }
  Py_INCREF(&StreamWriterType);
  if (PyModule_AddObject(m, "StreamWriter",
                         reinterpret_cast<PyObject*>(&StreamWriterType)) < 0) {
    Py_DECREF(&StreamWriterType);
    Py_DECREF(m);
    return nullptr;
  }
  Py_INCREF(&LineReaderType);
  if (PyModule_AddObject(m, "LineReader",
                         reinterpret_cast<PyObject*>(&LineReaderType)) < 0) {
    Py_DECREF(&LineReaderType);
    Py_DECREF(m);
    return nullptr;
  }
  return m;
}
