// wire_pool_selftest.cpp — stand-alone checks of wire_pool.hpp and of
// wire::ResponseReader, against a loopback listener on threads of this
// program.
//
// Built with -fsanitize=address,undefined by tests/test_wire_pool_native.py
// and run as a child process; nothing is preloaded.  Every case counts the
// entries of /proc/self/fd before it starts and after its server and pool
// are gone: the two must be equal, so every fd the pool opened was closed
// by the pool.  The exchange below is the one RestClient does with
// _wire.exchange: check out, send, read with ResponseReader, check in, and
// one more try on a fresh dial when a reused connection was reset before
// it said anything.

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <dirent.h>
#include <sys/wait.h>

#include "wire_core.hpp"
#include "wire_pool.hpp"

namespace {

int g_failures = 0;
int g_checks = 0;
std::mutex g_check_mu;

#define CHECK(cond)                                                     \
  do {                                                                  \
    std::lock_guard<std::mutex> check_hold(g_check_mu);                 \
    ++g_checks;                                                         \
    if (!(cond)) {                                                      \
      ++g_failures;                                                     \
      if (g_failures < 20)                                              \
        std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,    \
                     #cond);                                            \
    }                                                                   \
  } while (0)

int count_fds() {
  DIR* d = opendir("/proc/self/fd");
  if (!d) return -1;
  int n = 0;
  while (struct dirent* e = readdir(d))
    if (e->d_name[0] != '.') ++n;
  closedir(d);
  return n - 1;  // the directory's own fd
}

std::string ok_response(const std::string& body, const char* extra = "") {
  return "HTTP/1.1 200 OK\r\n" + std::string(extra) + "Content-Length: " +
         std::to_string(body.size()) + "\r\n\r\n" + body;
}

// ---------------------------------------------------------------------------
// the server: one thread per connection, behaviour chosen by request path
// ---------------------------------------------------------------------------

class Server {
 public:
  Server() {
    listener_ = socket(AF_INET, SOCK_STREAM | SOCK_CLOEXEC, 0);
    int one = 1;
    setsockopt(listener_, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
    struct sockaddr_in addr = {};
    addr.sin_family = AF_INET;
    addr.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
    if (bind(listener_, reinterpret_cast<sockaddr*>(&addr), sizeof addr) != 0 ||
        listen(listener_, 64) != 0) {
      std::perror("listen");
      std::exit(2);
    }
    socklen_t len = sizeof addr;
    getsockname(listener_, reinterpret_cast<sockaddr*>(&addr), &len);
    port = ntohs(addr.sin_port);
    acceptor_ = std::thread([this] { accept_loop(); });
  }

  ~Server() {
    shutdown(listener_, SHUT_RDWR);  // wakes the pending accept
    acceptor_.join();
    close(listener_);
    for (auto& t : handlers_) t.join();  // each ends when its peer closed
  }

  std::vector<std::string> requests() {
    std::lock_guard<std::mutex> hold(mu_);
    return requests_;
  }

  // block until `n` connections have been closed by the server side
  void wait_server_closed(int n) {
    std::unique_lock<std::mutex> hold(mu_);
    cv_.wait_for(hold, std::chrono::seconds(5),
                 [&] { return server_closed_ >= n; });
  }

  int port = 0;
  std::atomic<int> accepts{0};

 private:
  void accept_loop() {
    for (;;) {
      int fd = accept4(listener_, nullptr, nullptr, SOCK_CLOEXEC);
      if (fd < 0) {
        if (errno == EINTR) continue;
        return;
      }
      ++accepts;
      int one = 1;
      setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
      std::lock_guard<std::mutex> hold(mu_);
      handlers_.emplace_back([this, fd] { serve(fd); });
    }
  }

  static void send_str(int fd, const std::string& s) {
    size_t off = 0;
    while (off < s.size()) {
      ssize_t n = send(fd, s.data() + off, s.size() - off, MSG_NOSIGNAL);
      if (n <= 0) return;
      off += size_t(n);
    }
  }

  void note_closed() {
    std::lock_guard<std::mutex> hold(mu_);
    ++server_closed_;
    cv_.notify_all();
  }

  void serve(int fd) {
    std::string pending;
    char buf[4096];
    for (;;) {
      size_t end;
      while ((end = pending.find("\r\n\r\n")) == std::string::npos) {
        ssize_t n = recv(fd, buf, sizeof buf, 0);
        if (n <= 0) {
          close(fd);
          return;
        }
        pending.append(buf, size_t(n));
      }
      size_t sp1 = pending.find(' ');
      size_t sp2 = pending.find(' ', sp1 + 1);
      std::string path = pending.substr(sp1 + 1, sp2 - sp1 - 1);
      pending.erase(0, end + 4);  // the requests here have no body
      {
        std::lock_guard<std::mutex> hold(mu_);
        requests_.push_back(path);
      }
      if (path == "/ok") {
        send_str(fd, ok_response("ok"));
      } else if (path == "/slow") {
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        send_str(fd, ok_response("slow"));
      } else if (path == "/once") {  // answers, then drops the connection
        send_str(fd, ok_response("once"));
        close(fd);
        note_closed();
        return;
      } else if (path == "/close") {
        send_str(fd, ok_response("bye", "Connection: close\r\n"));
        close(fd);
        note_closed();
        return;
      } else if (path == "/until-close") {
        send_str(fd, "HTTP/1.1 200 OK\r\n\r\nto the end");
        close(fd);
        note_closed();
        return;
      } else if (path == "/extra") {
        send_str(fd, ok_response("ok") + "stray");
      } else if (path == "/stall") {
        send_str(fd, "HTTP/1.1 200 OK\r\nContent-Length: 100\r\n\r\n0123456789");
      } else if (path == "/bad") {
        send_str(fd, "HTTP/1.1 200 OK\r\nContent-Length: -1\r\n\r\n");
      } else {
        send_str(fd, "HTTP/1.1 404 Not Found\r\nContent-Length: 0\r\n\r\n");
      }
    }
  }

  int listener_ = -1;
  std::thread acceptor_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::thread> handlers_;
  std::vector<std::string> requests_;
  int server_closed_ = 0;
};

// ---------------------------------------------------------------------------
// the client: what RestClient does with checkout / exchange / checkin
// ---------------------------------------------------------------------------

struct Result {
  enum Kind { kResponse, kDialFailed, kTimeout, kReset, kCutShort, kFraming };
  Kind kind = kDialFailed;
  int status = 0;
  std::string body;
  bool reusable = false;
  wire::Pool::Error pool_error = wire::Pool::kOk;
};

// one try on one fd; *silent: the connection failed before it said anything
Result exchange_on(int fd, const std::string& path, double timeout_s,
                   bool* silent) {
  Result r;
  *silent = false;
  auto deadline = std::chrono::steady_clock::now() +
                  std::chrono::duration_cast<std::chrono::milliseconds>(
                      std::chrono::duration<double>(timeout_s));
  std::string req = "GET " + path + " HTTP/1.1\r\nHost: t\r\n\r\n";
  if (send(fd, req.data(), req.size(), MSG_NOSIGNAL) !=
      ssize_t(req.size())) {
    r.kind = Result::kReset;
    *silent = true;
    return r;
  }
  wire::ResponseReader reader(false);
  char buf[4096];
  while (!reader.done()) {
    auto left = std::chrono::duration_cast<std::chrono::milliseconds>(
                    deadline - std::chrono::steady_clock::now()).count();
    struct pollfd p = {fd, POLLIN, 0};
    if (left <= 0 || poll(&p, 1, int(left)) == 0) {
      r.kind = Result::kTimeout;
      return r;
    }
    ssize_t n = recv(fd, buf, sizeof buf, MSG_DONTWAIT);
    if (n < 0) {
      if (errno == EAGAIN || errno == EINTR) continue;
      r.kind = Result::kReset;
      *silent = !reader.started();
      return r;
    }
    if (n == 0) {
      if (reader.peer_closed()) break;
      r.kind = reader.started() ? Result::kCutShort : Result::kReset;
      *silent = !reader.started();
      return r;
    }
    // exactly-sized heap copy: a reader that looks past its input trips ASan
    std::unique_ptr<char[]> piece(new char[size_t(n)]);
    std::memcpy(piece.get(), buf, size_t(n));
    if (reader.feed(piece.get(), size_t(n)) < 0) {
      r.kind = Result::kFraming;
      return r;
    }
  }
  r.kind = Result::kResponse;
  r.status = reader.status();
  r.body = reader.body();
  r.reusable = reader.reusable();
  return r;
}

Result exchange(wire::Pool& pool, const std::string& path,
                double timeout_s = 5.0) {
  Result r;
  for (int attempt = 0; attempt < 2; ++attempt) {
    wire::Pool::Lease lease = attempt ? pool.dial() : pool.checkout();
    if (lease.fd < 0) {
      r.kind = Result::kDialFailed;
      r.pool_error = lease.error;
      return r;
    }
    bool silent = false;
    r = exchange_on(lease.fd, path, timeout_s, &silent);
    pool.checkin(lease.fd, r.kind == Result::kResponse && r.reusable);
    if (!(silent && lease.reused)) break;  // a fresh dial is not retried
  }
  return r;
}

bool is_ok(const Result& r, const char* body) {
  return r.kind == Result::kResponse && r.status == 200 && r.body == body &&
         r.reusable;
}

// Runs `body(server, port)`; the fds open before and after must be as many.
template <class Fn>
void fd_neutral(const char* name, Fn body) {
  int before = count_fds();
  {
    Server srv;
    body(srv);
  }
  int after = count_fds();
  if (before != after)
    std::fprintf(stderr, "%s: %d fds before, %d after\n", name, before, after);
  CHECK(before == after);
}

// ---------------------------------------------------------------------------
// cases
// ---------------------------------------------------------------------------

void test_sequential_reuse() {
  fd_neutral("sequential", [](Server& srv) {
    wire::Pool pool("127.0.0.1", srv.port, 4, 5.0);
    for (int i = 0; i < 50; ++i) CHECK(is_ok(exchange(pool, "/ok"), "ok"));
    CHECK(srv.accepts == 1);
    wire::PoolStats st = pool.stats();
    CHECK(st.dials == 1 && st.reuses == 49 && st.stale_discards == 0);
    CHECK(st.idle == 1);
  });
}

void test_threads_share() {
  fd_neutral("threads", [](Server& srv) {
    wire::Pool pool("127.0.0.1", srv.port, 4, 5.0);
    std::vector<std::thread> threads;
    for (int t = 0; t < 8; ++t)
      threads.emplace_back([&] {
        for (int i = 0; i < 20; ++i) CHECK(is_ok(exchange(pool, "/ok"), "ok"));
      });
    for (auto& t : threads) t.join();
    CHECK(srv.accepts >= 1 && srv.accepts <= 8);
    wire::PoolStats st = pool.stats();
    CHECK(st.idle <= 4);
    CHECK(st.dials == uint64_t(srv.accepts));
    CHECK(st.dials + st.reuses == 160);
    CHECK(srv.requests().size() == 160);
  });
}

void test_peer_closes_idle_connection() {
  fd_neutral("stale", [](Server& srv) {
    wire::Pool pool("127.0.0.1", srv.port, 4, 5.0);
    CHECK(is_ok(exchange(pool, "/once"), "once"));
    CHECK(pool.stats().idle == 1);  // the response said nothing of closing
    srv.wait_server_closed(1);
    CHECK(is_ok(exchange(pool, "/ok"), "ok"));
    wire::PoolStats st = pool.stats();
    CHECK(st.dials == 2 && st.stale_discards == 1 && st.reuses == 0);
    CHECK(srv.accepts == 2);
    std::vector<std::string> want = {"/once", "/ok"};
    CHECK(srv.requests() == want);  // each request exactly once: no replay
  });
}

void test_not_pooled() {
  fd_neutral("not pooled", [](Server& srv) {
    wire::Pool pool("127.0.0.1", srv.port, 4, 5.0);
    Result r = exchange(pool, "/close");
    CHECK(r.kind == Result::kResponse && r.body == "bye" && !r.reusable);
    CHECK(pool.stats().idle == 0);
    r = exchange(pool, "/until-close");
    CHECK(r.kind == Result::kResponse && r.body == "to the end" && !r.reusable);
    CHECK(pool.stats().idle == 0);
    r = exchange(pool, "/extra");
    // the stray bytes may arrive with the response or after it; when they
    // come later the idle check at the next checkout finds them
    CHECK(r.kind == Result::kResponse && r.body == "ok");
    if (r.reusable) {
      std::this_thread::sleep_for(std::chrono::milliseconds(20));
      uint64_t before = pool.stats().stale_discards;
      CHECK(is_ok(exchange(pool, "/ok"), "ok"));
      CHECK(pool.stats().stale_discards == before + 1);
    } else {
      CHECK(pool.stats().idle == 0);
    }
    CHECK(pool.stats().reuses == 0);
  });
}

void test_failures_close_the_fd() {
  fd_neutral("failures", [](Server& srv) {
    wire::Pool pool("127.0.0.1", srv.port, 4, 5.0);
    int held = count_fds();
    Result r = exchange(pool, "/stall", 0.1);
    CHECK(r.kind == Result::kTimeout);
    CHECK(pool.stats().idle == 0);
    r = exchange(pool, "/bad");
    CHECK(r.kind == Result::kFraming);
    CHECK(pool.stats().idle == 0);
    // the server's ends close once it has seen ours close
    for (int i = 0; i < 200 && count_fds() != held; ++i)
      std::this_thread::sleep_for(std::chrono::milliseconds(5));
    CHECK(count_fds() == held);
    CHECK(is_ok(exchange(pool, "/ok"), "ok"));  // still usable
    CHECK(is_ok(exchange(pool, "/ok"), "ok"));
    CHECK(pool.stats().reuses == 1 && pool.stats().dials == 3);
  });
}

void test_max_idle() {
  fd_neutral("max_idle", [](Server& srv) {
    wire::Pool pool("127.0.0.1", srv.port, 2, 5.0);
    int base = count_fds();
    std::vector<std::thread> users;
    std::mutex mu;
    std::condition_variable cv;
    int holding = 0;
    for (int u = 0; u < 4; ++u)
      users.emplace_back([&] {
        wire::Pool::Lease lease = pool.checkout();
        CHECK(lease.fd >= 0 && !lease.reused);
        {  // all four hold a connection at the same time
          std::unique_lock<std::mutex> hold(mu);
          ++holding;
          cv.notify_all();
          cv.wait_for(hold, std::chrono::seconds(5),
                      [&] { return holding == 4; });
        }
        bool silent;
        Result r = exchange_on(lease.fd, "/ok", 5.0, &silent);
        CHECK(is_ok(r, "ok"));
        pool.checkin(lease.fd, r.reusable);
      });
    for (auto& t : users) t.join();
    CHECK(srv.accepts == 4);
    CHECK(pool.stats().idle == 2 && pool.stats().dials == 4);
    // ours: two idle; the server's: two until it sees the other two close
    for (int i = 0; i < 200 && count_fds() != base + 4; ++i)
      std::this_thread::sleep_for(std::chrono::milliseconds(5));
    CHECK(count_fds() == base + 4);
  });
}

void test_close_with_one_checked_out() {
  fd_neutral("close", [](Server& srv) {
    wire::Pool pool("127.0.0.1", srv.port, 4, 5.0);
    CHECK(is_ok(exchange(pool, "/ok"), "ok"));
    wire::Pool::Lease lent = pool.dial();
    CHECK(lent.fd >= 0);
    CHECK(pool.stats().idle == 1);
    pool.close();
    CHECK(pool.stats().idle == 0);
    bool silent;
    CHECK(is_ok(exchange_on(lent.fd, "/ok", 5.0, &silent), "ok"));  // still ours
    pool.checkin(lent.fd, true);  // closed here, not kept
    CHECK(pool.stats().idle == 0);
    CHECK(pool.checkout().error == wire::Pool::kClosed);
    CHECK(pool.dial().error == wire::Pool::kClosed);
    CHECK(exchange(pool, "/ok").pool_error == wire::Pool::kClosed);
    pool.close();  // twice is fine
  });
}

void test_dial_failures() {
  int before = count_fds();
  int dead_port;
  {
    Server srv;
    dead_port = srv.port;
  }
  {
    wire::Pool pool("127.0.0.1", dead_port, 4, 1.0);
    wire::Pool::Lease lease = pool.checkout();
    CHECK(lease.fd < 0 && lease.error == wire::Pool::kConnect &&
          lease.code == ECONNREFUSED);
  }
  CHECK(count_fds() == before);
}

void test_fork_starts_empty() {
  fd_neutral("fork", [](Server& srv) {
    wire::Pool pool("127.0.0.1", srv.port, 4, 5.0);
    CHECK(is_ok(exchange(pool, "/ok"), "ok"));
    CHECK(pool.stats().idle == 1);
    int with_idle = count_fds();
    pid_t child = fork();
    if (child == 0) {
      // the inherited idle fd is closed, and nothing else happens to it
      bool empty = pool.stats().idle == 0 && pool.stats().dials == 0;
      bool closed = count_fds() == with_idle - 1;
      _exit(empty && closed ? 0 : 1);
    }
    int status = -1;
    waitpid(child, &status, 0);
    CHECK(WIFEXITED(status) && WEXITSTATUS(status) == 0);
    // the parent's connection is untouched by the child's close
    CHECK(is_ok(exchange(pool, "/ok"), "ok"));
    CHECK(pool.stats().reuses == 1 && pool.stats().stale_discards == 0);
  });
}

// ---------------------------------------------------------------------------
// ResponseReader: every split point gives what the whole buffer gives
// ---------------------------------------------------------------------------

struct Parsed {
  int rc = 0;
  int status = 0;
  std::string body;
  bool reusable = false;
};

Parsed read_pieces(const std::vector<std::string>& pieces, bool head_request) {
  wire::ResponseReader reader(head_request);
  Parsed out;
  for (const std::string& piece : pieces) {
    if (piece.empty()) continue;
    std::unique_ptr<char[]> copy(new char[piece.size()]);
    std::memcpy(copy.get(), piece.data(), piece.size());
    out.rc = reader.feed(copy.get(), piece.size());
    if (out.rc != wire::kNeedMore) break;
  }
  out.status = reader.status();
  out.body = reader.body();
  out.reusable = reader.reusable();
  return out;
}

void test_response_reader_splits() {
  struct Case {
    std::string bytes;
    bool head_request;
    int status;
    std::string body;
  };
  const std::string chunked =
      "HTTP/1.1 201 Created\r\nTransfer-Encoding: chunked\r\n\r\n"
      "7;ext=1\r\n{\"a\": 1\r\n1\r\n,\r\n8 ; x\r\n \"b\": 2}\r\n"
      "0\r\nX-Trailer: 1\r\nX-Other: 2\r\n\r\n";
  const std::vector<Case> corpus = {
      {ok_response("{\"kind\": \"Status\"}"), false, 200, "{\"kind\": \"Status\"}"},
      {chunked, false, 201, "{\"a\": 1, \"b\": 2}"},
      {"HTTP/1.1 204 No Content\r\nX-A: b\r\n\r\n", false, 204, ""},
      {"HTTP/1.1 304 Not Modified\r\nContent-Length: 10\r\n\r\n", false, 304, ""},
      {"HTTP/1.1 200 OK\r\nContent-Length: 10\r\n\r\n", true, 200, ""},
      {"HTTP/1.1 100 Continue\r\n\r\n" + ok_response("after"), false, 200,
       "after"},
  };
  for (const Case& c : corpus) {
    Parsed whole = read_pieces({c.bytes}, c.head_request);
    CHECK(whole.rc == wire::kDone && whole.status == c.status &&
          whole.body == c.body && whole.reusable);
    for (size_t split = 1; split < c.bytes.size(); ++split) {
      Parsed two = read_pieces(
          {c.bytes.substr(0, split), c.bytes.substr(split)}, c.head_request);
      CHECK(two.rc == whole.rc && two.status == whole.status &&
            two.body == whole.body && two.reusable == whole.reusable);
    }
    std::vector<std::string> bytes;
    for (char ch : c.bytes) bytes.emplace_back(1, ch);
    Parsed single = read_pieces(bytes, c.head_request);
    CHECK(single.rc == whole.rc && single.status == whole.status &&
          single.body == whole.body && single.reusable == whole.reusable);
    // bytes past the response: same result, but not reusable, wherever cut
    std::string more = c.bytes + "HTTP/1.1 200";
    for (size_t split = 1; split <= c.bytes.size(); ++split) {
      Parsed two =
          read_pieces({more.substr(0, split), more.substr(split)}, c.head_request);
      // cut exactly at the end, the reader is done before the rest arrives
      bool sees_rest = split < c.bytes.size();
      CHECK(two.rc == wire::kDone && two.body == c.body &&
            two.reusable == !sees_rest);
    }
  }
  // read-until-close: done only when the peer closes, never reusable
  wire::ResponseReader until(false);
  std::string raw = "HTTP/1.1 200 OK\r\n\r\nabc";
  CHECK(until.feed(raw.data(), raw.size()) == wire::kNeedMore);
  CHECK(until.peer_closed() && until.done() && until.body() == "abc" &&
        !until.reusable());
  // a close in the middle of a framed body is not an end
  wire::ResponseReader cut(false);
  raw = "HTTP/1.1 200 OK\r\nContent-Length: 5\r\n\r\nab";
  CHECK(cut.feed(raw.data(), raw.size()) == wire::kNeedMore);
  CHECK(!cut.peer_closed() && !cut.done() && cut.started());
  wire::ResponseReader bad(false);
  raw = "HTTP/1.1 200 OK\r\nContent-Length: -1\r\n\r\n";
  CHECK(bad.feed(raw.data(), raw.size()) == wire::kErrBadLength);
}

}  // namespace

int main() {
  test_response_reader_splits();
  test_sequential_reuse();
  test_threads_share();
  test_peer_closes_idle_connection();
  test_not_pooled();
  test_failures_close_the_fd();
  test_max_idle();
  test_close_with_one_checked_out();
  test_dial_failures();
  test_fork_starts_empty();
  if (g_failures) {
    std::fprintf(stderr, "wire_pool selftest: %d of %d checks FAILED\n",
                 g_failures, g_checks);
    return 1;
  }
  std::printf("wire_pool selftest: %d checks passed\n", g_checks);
  return 0;
}
