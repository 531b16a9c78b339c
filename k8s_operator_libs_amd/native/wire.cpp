// wire.cpp — native HTTP/1.1 wire path for the REST client and watch reader.
//
// Per-request wire overhead (request assembly, two sends, the header parse
// of the response, and the pure-Python line iteration of the watch stream)
// is where the cached-substrate reconcile loop spends its time
// (docs/performance.md).  This CPython extension does the framing natively
// on a socket the Python side owns:
//
//   exchange(fd, method, path, header_bytes, body, timeout)
//       -> (status, body_bytes, reusable)
//   LineReader(fd).read_head(timeout) -> status
//   LineReader(fd).readline(timeout)  -> bytes | None
//   parse_request_head(data)          -> None | (method, target, ...)
//     (the threaded apiserver's side of the same exchange)
//
// Rules: the fd belongs to the Python socket object and is never closed
// here; every wait is poll()+recv()/send() with the remaining deadline and
// with the GIL released; EINTR re-takes the GIL and runs signal handlers.
// Parsing lives in wire_core.hpp (no Python, no sockets).

#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <cerrno>
#include <chrono>
#include <new>
#include <string>

#include <poll.h>
#include <sys/socket.h>
#include <sys/types.h>

#include "wire_core.hpp"

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

bool status_has_no_body(int status) {
  return status == 204 || status == 304;
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

  wire::HeadParser head_parser(wire::HeadParser::kResponse);
  wire::ChunkedDecoder chunked;
  std::string out;
  enum { kHead, kLength, kChunked, kUntilClose, kComplete } phase = kHead;
  size_t remaining = 0;
  bool reusable = true;
  bool got_any = false;
  char buf[kRecvBuf];  // on the stack: no allocation per request

  while (phase != kComplete) {
    size_t got = 0;
    io = recv_some(fd, buf, sizeof buf, dl, &got);
    if (io == kIoTimeout) return raise_timeout();
    if (io != kIoOk) return nullptr;
    if (got == 0) {
      if (phase == kUntilClose) {
        phase = kComplete;
        break;
      }
      PyErr_SetString(got_any ? PyExc_ConnectionError
                              : PyExc_ConnectionResetError,
                      got_any ? "peer closed the connection mid-response"
                              : "peer closed the connection without a response");
      return nullptr;
    }
    got_any = true;
    const char* p = buf;
    size_t n = got;
    while (n > 0 && phase != kComplete) {
      size_t used = 0;
      if (phase == kHead) {
        int st = head_parser.feed(p, n, &used);
        if (st < 0) return raise_wire_error(st);
        if (st == wire::kDone) {
          int code = head_parser.status;
          if (code >= 100 && code < 200 && code != 101) {
            head_parser.reset();  // interim response: skip it
          } else {
            if (!head_parser.keep_alive()) reusable = false;
            if (is_head || status_has_no_body(code)) {
              phase = kComplete;
            } else if (head_parser.chunked) {
              phase = kChunked;
            } else if (head_parser.has_content_length) {
              remaining = head_parser.content_length;
              if (remaining == 0) {
                phase = kComplete;
              } else {
                phase = kLength;
                // cap the up-front reservation: the length is peer-supplied
                out.reserve(remaining < (size_t(1) << 26) ? remaining
                                                          : (size_t(1) << 26));
              }
            } else {
              phase = kUntilClose;
              reusable = false;
            }
          }
        }
      } else if (phase == kLength) {
        used = n < remaining ? n : remaining;
        out.append(p, used);
        remaining -= used;
        if (remaining == 0) phase = kComplete;
      } else if (phase == kChunked) {
        int st = chunked.feed(p, n, &used, &out);
        if (st < 0) return raise_wire_error(st);
        if (st == wire::kDone) phase = kComplete;
      } else {  // kUntilClose
        used = n;
        out.append(p, used);
      }
      p += used;
      n -= used;
    }
    if (n > 0) reusable = false;  // bytes past the response: do not reuse
  }

  PyObject* body_bytes =
      PyBytes_FromStringAndSize(out.data(), Py_ssize_t(out.size()));
  if (!body_bytes) return nullptr;
  PyObject* res = Py_BuildValue("(iNO)", head_parser.status, body_bytes,
                                reusable ? Py_True : Py_False);
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
  bool busy;         // a call is inside poll/recv with the GIL released
  bool head_done;
  bool stream_end;   // body complete or peer closed
  bool flushed;      // unterminated tail already handed out
  int mode;          // 0 until-close, 1 chunked, 2 content-length
  size_t remaining;  // mode 2
  wire::HeadParser* head;
  wire::ChunkedDecoder* chunked;
  wire::LineSplitter* lines;
  std::string* scratch;  // decoded chunk payload
  std::string* buf;      // recv buffer
};

void linereader_dealloc(LineReaderObject* self) {
  delete self->head;
  delete self->chunked;
  delete self->lines;
  delete self->scratch;
  delete self->buf;
  Py_TYPE(self)->tp_free(reinterpret_cast<PyObject*>(self));
}

int linereader_init(LineReaderObject* self, PyObject* args, PyObject* /*kw*/) {
  int fd;
  if (!PyArg_ParseTuple(args, "i", &fd)) return -1;
  if (self->head != nullptr) {
    PyErr_SetString(PyExc_RuntimeError, "LineReader is already initialised");
    return -1;
  }
  self->fd = fd;
  self->busy = false;
  self->head_done = false;
  self->stream_end = false;
  self->flushed = false;
  self->mode = 0;
  self->remaining = 0;
  try {
    self->head = new wire::HeadParser(wire::HeadParser::kResponse);
    self->chunked = new wire::ChunkedDecoder();
    self->lines = new wire::LineSplitter();
    self->scratch = new std::string();
    self->buf = new std::string(kRecvBuf, '\0');
  } catch (const std::bad_alloc&) {
    PyErr_NoMemory();
    return -1;
  }
  return 0;
}

// Route received bytes through head -> body framing -> line splitter.
// Returns false with a Python exception set on malformed framing.
bool linereader_consume(LineReaderObject* self, const char* p, size_t n) {
  while (n > 0) {
    size_t used = 0;
    if (!self->head_done) {
      int st = self->head->feed(p, n, &used);
      if (st < 0) {
        raise_wire_error(st);
        return false;
      }
      if (st == wire::kDone) {
        int code = self->head->status;
        if (code >= 100 && code < 200 && code != 101) {
          self->head->reset();
        } else {
          self->head_done = true;
          if (status_has_no_body(code)) {
            self->stream_end = true;
          } else if (self->head->chunked) {
            self->mode = 1;
          } else if (self->head->has_content_length) {
            self->mode = 2;
            self->remaining = self->head->content_length;
            if (self->remaining == 0) self->stream_end = true;
          } else {
            self->mode = 0;
          }
        }
      }
    } else if (self->stream_end) {
      return true;  // bytes past the body are not ours
    } else if (self->mode == 1) {
      self->scratch->clear();
      int st = self->chunked->feed(p, n, &used, self->scratch);
      self->lines->feed(self->scratch->data(), self->scratch->size());
      if (st < 0) {
        raise_wire_error(st);
        return false;
      }
      if (st == wire::kDone) self->stream_end = true;
    } else if (self->mode == 2) {
      used = n < self->remaining ? n : self->remaining;
      self->lines->feed(p, used);
      self->remaining -= used;
      if (self->remaining == 0) self->stream_end = true;
    } else {
      used = n;
      self->lines->feed(p, used);
    }
    p += used;
    n -= used;
  }
  return true;
}

// One poll+recv round.  Returns kIoOk (bytes consumed or stream_end set),
// kIoTimeout, or kIoError/kIoSignal with an exception set.
IoResult linereader_fill(LineReaderObject* self, const Deadline& dl) {
  size_t got = 0;
  self->busy = true;
  IoResult io = recv_some(self->fd, &(*self->buf)[0], self->buf->size(), dl,
                          &got);
  self->busy = false;
  if (io != kIoOk) return io;
  if (got == 0) {
    self->stream_end = true;
    return kIoOk;
  }
  try {
    if (!linereader_consume(self, self->buf->data(), got)) return kIoError;
  } catch (const std::bad_alloc&) {
    PyErr_NoMemory();
    return kIoError;
  }
  return kIoOk;
}

bool linereader_enter(LineReaderObject* self) {
  if (self->head == nullptr) {
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
  while (!self->head_done) {
    if (self->stream_end) {
      PyErr_SetString(PyExc_ConnectionResetError,
                      "peer closed the connection without a response");
      return nullptr;
    }
    IoResult io = linereader_fill(self, dl);
    if (io == kIoTimeout) return raise_timeout();
    if (io != kIoOk) return nullptr;
  }
  return PyLong_FromLong(self->head->status);
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
    int st = self->lines->next(&line);
    if (st == wire::kDone)
      return PyBytes_FromStringAndSize(line.data(), Py_ssize_t(line.size()));
    if (st < 0) return raise_wire_error(st);
    if (self->stream_end) {
      if (!self->head_done) {
        PyErr_SetString(PyExc_ConnectionResetError,
                        "peer closed the connection without a response");
        return nullptr;
      }
      if (!self->flushed) {
        self->flushed = true;
        st = self->lines->flush(&line);
        if (st == wire::kDone)
          return PyBytes_FromStringAndSize(line.data(),
                                           Py_ssize_t(line.size()));
        if (st < 0) return raise_wire_error(st);
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
  if (self->head == nullptr || !self->head_done) Py_RETURN_NONE;
  return PyLong_FromLong(self->head->status);
}

PyObject* linereader_get_chunked(LineReaderObject* self, void*) {
  if (self->head == nullptr || !self->head_done) Py_RETURN_NONE;
  return PyBool_FromLong(self->mode == 1);
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
  PyObject* m = PyModule_Create(&wire_module);
  if (!m) return nullptr;
  Py_INCREF(&LineReaderType);
  if (PyModule_AddObject(m, "LineReader",
                         reinterpret_cast<PyObject*>(&LineReaderType)) < 0) {
    Py_DECREF(&LineReaderType);
    Py_DECREF(m);
    return nullptr;
  }
  return m;
}
