// wire_pool.hpp — keep-alive connection pool shared by every thread of a
// client.  Sockets, no Python: wire.cpp wraps it as _wire.Pool, and
// tests/native/wire_pool_selftest.cpp drives it stand-alone under sanitizers.
//
// The pool dials its own connections and lends their fds out one user at a
// time: checkout() hands over the most recently used idle fd (or dials),
// checkin() takes it back when the response was complete and the connection
// may carry another request, and closes it otherwise.  Every fd the pool
// opened is closed by the pool and by nobody else; a lent fd must come back
// through checkin() exactly once.
//
// A thread that lives for one request therefore reuses a connection that
// another thread left behind, where a thread-local socket would have cost it
// a TCP handshake, an accept and a handler-thread start on the server.

#pragma once

#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <sys/types.h>
#include <unistd.h>

namespace wire {

struct PoolStats {
  uint64_t dials = 0;           // connections opened
  uint64_t reuses = 0;          // checkouts served from the idle list
  uint64_t stale_discards = 0;  // idle fds found dead at checkout
  size_t idle = 0;              // fds on the idle list now
};

class Pool {
 public:
  enum Error {
    kOk = 0,
    kClosed,       // close() has been called
    kResolve,      // getaddrinfo failed: `code` is its EAI_* value
    kConnect,      // socket/connect failed: `code` is errno
    kTimeout,      // connect_timeout ran out
    kInterrupted,  // on_eintr said stop
  };

  struct Lease {
    int fd = -1;
    bool reused = false;  // from the idle list, not freshly dialled
    Error error = kOk;
    int code = 0;
  };

  // Called when a blocking wait was interrupted by a signal; false aborts
  // the dial with kInterrupted.
  using OnEintr = bool (*)(void*);

  Pool(std::string host, int port, size_t max_idle, double connect_timeout_s)
      : host_(std::move(host)), port_(port), max_idle_(max_idle),
        // negative: no limit of the pool's own (the kernel's still holds)
        connect_timeout_s_(connect_timeout_s < 0 || connect_timeout_s > 1e6
                               ? 1e6 : connect_timeout_s),
        pid_(getpid()) {}

  ~Pool() { close(); }

  Pool(const Pool&) = delete;
  Pool& operator=(const Pool&) = delete;

  // The most recently used idle connection that is still quiet, without
  // blocking; fd -1 with kOk when there is none and the caller should dial().
  // An idle keep-alive connection has nothing to say: readable, hung up or
  // in error means the peer closed it or sent stray bytes, so it is closed
  // here, before a request is written to it, and the next one is tried.
  Lease take_idle() {
    Lease lease;
    for (;;) {
      int fd;
      {
        std::lock_guard<std::mutex> hold(mu_);
        after_fork();
        if (closed_) {
          lease.error = kClosed;
          return lease;
        }
        if (idle_.empty()) return lease;
        fd = idle_.back();
        idle_.pop_back();
      }
      struct pollfd p = {fd, POLLIN | POLLRDHUP | POLLHUP | POLLERR, 0};
      int rc = poll(&p, 1, 0);
      if (rc == 0) {
        std::lock_guard<std::mutex> hold(mu_);
        ++stats_.reuses;
        lease.fd = fd;
        lease.reused = true;
        return lease;
      }
      ::close(fd);
      std::lock_guard<std::mutex> hold(mu_);
      ++stats_.stale_discards;
    }
  }

  // Open a new connection: resolve (numeric addresses without a lookup),
  // non-blocking connect, poll against connect_timeout.  Blocks; call it
  // without any lock the caller's other threads need.
  Lease dial(OnEintr on_eintr = nullptr, void* arg = nullptr) {
    Lease lease;
    {
      std::lock_guard<std::mutex> hold(mu_);
      after_fork();
      if (closed_) {
        lease.error = kClosed;
        return lease;
      }
    }
    char service[16];
    std::snprintf(service, sizeof service, "%d", port_);
    struct addrinfo hints = {};
    hints.ai_socktype = SOCK_STREAM;
    hints.ai_flags = AI_NUMERICHOST | AI_NUMERICSERV;
    struct addrinfo* found = nullptr;
    int rc = getaddrinfo(host_.c_str(), service, &hints, &found);
    if (rc == EAI_NONAME) {  // not a numeric address: look the name up
      hints.ai_flags = AI_NUMERICSERV;
      rc = getaddrinfo(host_.c_str(), service, &hints, &found);
    }
    if (rc != 0) {
      lease.error = kResolve;
      lease.code = rc;
      return lease;
    }
    auto deadline = std::chrono::steady_clock::now() +
                    std::chrono::duration_cast<std::chrono::microseconds>(
                        std::chrono::duration<double>(connect_timeout_s_));
    lease.error = kConnect;
    lease.code = EADDRNOTAVAIL;  // an empty address list
    for (struct addrinfo* ai = found; ai != nullptr; ai = ai->ai_next) {
      int fd = socket(ai->ai_family, ai->ai_socktype | SOCK_NONBLOCK | SOCK_CLOEXEC,
                      ai->ai_protocol);
      if (fd < 0) {
        lease.code = errno;
        continue;
      }
      Error err = connect_fd(fd, ai, deadline, on_eintr, arg, &lease.code);
      if (err == kOk) {
        int one = 1;
        setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
        lease.fd = fd;
        lease.error = kOk;
        lease.code = 0;
        break;
      }
      ::close(fd);
      lease.error = err;
      if (err != kConnect) break;  // out of time or told to stop
    }
    freeaddrinfo(found);
    if (lease.fd >= 0) {
      std::lock_guard<std::mutex> hold(mu_);
      ++stats_.dials;
      if (closed_) {  // close() came while we dialled
        ::close(lease.fd);
        lease.fd = -1;
        lease.error = kClosed;
      }
    }
    return lease;
  }

  Lease checkout(OnEintr on_eintr = nullptr, void* arg = nullptr) {
    Lease lease = take_idle();
    if (lease.fd >= 0 || lease.error != kOk) return lease;
    return dial(on_eintr, arg);
  }

  // Give a lent fd back.  reusable: the response was complete and the
  // connection may carry another request; anything else (timeout, framing
  // error, interruption, `Connection: close`) closes it.  So do a closed
  // pool and an idle list already holding max_idle.
  void checkin(int fd, bool reusable) {
    if (fd < 0) return;
    {
      std::lock_guard<std::mutex> hold(mu_);
      if (reusable && !closed_ && pid_ == getpid() &&
          idle_.size() < max_idle_) {
        idle_.push_back(fd);
        return;
      }
    }
    ::close(fd);
  }

  // Close the idle fds.  An fd lent out now is closed when it comes back;
  // checkout() and dial() fail with kClosed from here on.
  void close() {
    std::vector<int> doomed;
    {
      std::lock_guard<std::mutex> hold(mu_);
      after_fork();
      closed_ = true;
      doomed.swap(idle_);
    }
    for (int fd : doomed) ::close(fd);
  }

  bool closed() {
    std::lock_guard<std::mutex> hold(mu_);
    return closed_;
  }

  PoolStats stats() {
    std::lock_guard<std::mutex> hold(mu_);
    after_fork();
    PoolStats out = stats_;
    out.idle = idle_.size();
    return out;
  }

  const std::string& host() const { return host_; }
  int port() const { return port_; }
  size_t max_idle() const { return max_idle_; }

 private:
  // mu_ held.  In a forked child the idle fds are the parent's connections:
  // close the child's copies (the parent's stay open) and start empty.
  void after_fork() {
    pid_t now = getpid();
    if (now == pid_) return;
    pid_ = now;
    for (int fd : idle_) ::close(fd);
    idle_.clear();
    stats_ = PoolStats();
  }

  static Error connect_fd(int fd, const struct addrinfo* ai,
                          std::chrono::steady_clock::time_point deadline,
                          OnEintr on_eintr, void* arg, int* code) {
    for (;;) {
      if (connect(fd, ai->ai_addr, ai->ai_addrlen) == 0) return kOk;
      if (errno == EINTR) {
        // the connect goes on in the background: wait for it below
        if (on_eintr && !on_eintr(arg)) return kInterrupted;
        break;
      }
      if (errno == EINPROGRESS) break;
      *code = errno;
      return kConnect;
    }
    for (;;) {
      auto left = std::chrono::duration_cast<std::chrono::milliseconds>(
                      deadline - std::chrono::steady_clock::now()).count();
      if (left <= 0) return kTimeout;
      struct pollfd p = {fd, POLLOUT, 0};
      int rc = poll(&p, 1, left > 0x7fffffff ? 0x7fffffff : int(left) + 1);
      if (rc < 0) {
        if (errno != EINTR) {
          *code = errno;
          return kConnect;
        }
        if (on_eintr && !on_eintr(arg)) return kInterrupted;
        continue;
      }
      if (rc == 0) continue;  // the deadline check above decides
      int soerr = 0;
      socklen_t len = sizeof soerr;
      if (getsockopt(fd, SOL_SOCKET, SO_ERROR, &soerr, &len) != 0) soerr = errno;
      if (soerr == 0) return kOk;
      *code = soerr;
      return kConnect;
    }
  }

  const std::string host_;
  const int port_;
  const size_t max_idle_;
  const double connect_timeout_s_;

  std::mutex mu_;
  pid_t pid_;
  bool closed_ = false;
  std::vector<int> idle_;  // most recently used at the back
  PoolStats stats_;
};

}  // namespace wire
