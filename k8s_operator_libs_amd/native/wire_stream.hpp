// wire_stream.hpp — Python-free, socket-free state of the watch event path.
//
// Server side: StreamBuffer is the per-stream backlog behind
// _wire.StreamWriter.  Whole lines go straight to a caller-supplied send
// function while nothing is queued; the unsent tail of a line and every
// later line wait in the backlog; a backlog past its cap marks the stream
// dead.  The send function stands in for send(2): wire.cpp supplies the real
// one.
//
// Client side: LineFramer turns the bytes of a streaming response into lines
// (it is what _wire.LineReader and _wire.LinePump read with), and LineQueue
// is the pending-line queue, with its sequence counter, between a LinePump's
// reader thread and the Python threads that consume the lines.
//
// tests/native/wire_stream_selftest.cpp drives all three stand-alone under
// AddressSanitizer + UBSan and under ThreadSanitizer.
//
// Thread safety: StreamBuffer and LineQueue may be used from any thread.
// StreamBuffer holds one mutex across the send call, which is what keeps two
// lines from interleaving, so the send function must never block.

#pragma once

#include <cerrno>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <ctime>
#include <deque>
#include <mutex>
#include <string>
#include <utility>

#include <pthread.h>

#include "wire_core.hpp"

namespace wire {

// What a send function returns instead of a byte count.
constexpr long kSendWouldBlock = -1;  // nothing accepted now, try again later
constexpr long kSendFailed = -2;      // the stream is broken for good

class StreamBuffer {
 public:
  enum Result {
    kSent,    // nothing is waiting: every accepted byte has been sent
    kQueued,  // bytes wait in the backlog: flush() when the sink has room
    kDead,    // overflow or a failed send: nothing more is accepted
  };

  explicit StreamBuffer(size_t max_backlog) : max_backlog_(max_backlog) {}

  // Accept [p, p+n) as one unit.  With an empty backlog it is offered to
  // `send` first (long send(const char*, size_t): bytes taken, or one of the
  // two constants above); whatever is left is queued behind earlier data.
  template <class SendFn>
  Result write(const char* p, size_t n, SendFn&& send) {
    std::lock_guard<std::mutex> hold(mu_);
    if (dead_) return kDead;
    if (pending_locked() == 0) {
      while (n > 0) {
        long rc = send(p, n);
        if (rc == kSendWouldBlock || rc == 0) break;
        if (rc < 0) return die();
        p += rc;
        n -= size_t(rc);
      }
      if (n == 0) return kSent;
    }
    if (n > max_backlog_ || pending_locked() > max_backlog_ - n) return die();
    if (head_ > 0 && head_ >= buf_.size() - head_) {  // compact: tail is small
      buf_.erase(0, head_);
      head_ = 0;
    }
    buf_.append(p, n);
    return kQueued;
  }

  // Offer the backlog to `send` until it is empty or the sink is full.
  template <class SendFn>
  Result flush(SendFn&& send) {
    std::lock_guard<std::mutex> hold(mu_);
    if (dead_) return kDead;
    while (head_ < buf_.size()) {
      long rc = send(buf_.data() + head_, buf_.size() - head_);
      if (rc == kSendWouldBlock || rc == 0) return kQueued;
      if (rc < 0) return die();
      head_ += size_t(rc);
    }
    buf_.clear();
    head_ = 0;
    return kSent;
  }

  // Refuse everything from now on and drop what is queued.
  void kill() {
    std::lock_guard<std::mutex> hold(mu_);
    die();
  }

  bool dead() const {
    std::lock_guard<std::mutex> hold(mu_);
    return dead_;
  }

  size_t pending() const {
    std::lock_guard<std::mutex> hold(mu_);
    return pending_locked();
  }

 private:
  size_t pending_locked() const { return buf_.size() - head_; }

  Result die() {
    dead_ = true;
    std::string().swap(buf_);
    head_ = 0;
    return kDead;
  }

  const size_t max_backlog_;
  mutable std::mutex mu_;
  std::string buf_;
  size_t head_ = 0;  // bytes of buf_ already sent
  bool dead_ = false;
};

// ---------------------------------------------------------------------------
// LineFramer: a streaming HTTP response as lines.  Received bytes go through
// the response head, then the body framing the head announced (chunked,
// Content-Length or read-until-close), then the line splitter.  Not
// thread-safe: one reader at a time (_wire.LineReader, or the thread of a
// _wire.LinePump).
// ---------------------------------------------------------------------------

class LineFramer {
 public:
  LineFramer() : head_(HeadParser::kResponse) {}

  // Route [p, p+n) through head -> body framing -> line splitter.  Returns
  // kNeedMore, or the error of malformed framing.  Bytes past the end of
  // the body are ignored.
  int consume(const char* p, size_t n) {
    while (n > 0) {
      size_t used = 0;
      if (!head_done_) {
        int st = head_.feed(p, n, &used);
        if (st < 0) return st;
        if (st == kDone) {
          int code = head_.status;
          if (code >= 100 && code < 200 && code != 101) {
            head_.reset();  // interim response: skip it
          } else {
            head_done_ = true;
            if (code == 204 || code == 304) {
              stream_end_ = true;
            } else if (head_.chunked) {
              mode_ = kChunked;
            } else if (head_.has_content_length) {
              mode_ = kLength;
              remaining_ = head_.content_length;
              if (remaining_ == 0) stream_end_ = true;
            } else {
              mode_ = kUntilClose;
            }
          }
        }
      } else if (stream_end_) {
        return kNeedMore;  // bytes past the body are not ours
      } else if (mode_ == kChunked) {
        scratch_.clear();
        int st = chunked_.feed(p, n, &used, &scratch_);
        lines_.feed(scratch_.data(), scratch_.size());
        if (st < 0) return st;
        if (st == kDone) stream_end_ = true;
      } else if (mode_ == kLength) {
        used = n < remaining_ ? n : remaining_;
        lines_.feed(p, used);
        remaining_ -= used;
        if (remaining_ == 0) stream_end_ = true;
      } else {
        used = n;
        lines_.feed(p, used);
      }
      p += used;
      n -= used;
    }
    return kNeedMore;
  }

  void peer_closed() { stream_end_ = true; }

  // Next non-blank line: kDone with *out set, kNeedMore when none is
  // complete yet, or kErrLineTooLong.  Once the stream has ended the
  // unterminated tail is handed out as a last line.
  int next(std::string* out) {
    int st = lines_.next(out);
    if (st != kNeedMore) return st;
    if (stream_end_ && head_done_ && !flushed_) {
      flushed_ = true;
      return lines_.flush(out);
    }
    return kNeedMore;
  }

  bool head_done() const { return head_done_; }
  bool stream_end() const { return stream_end_; }  // body complete or peer closed
  int status() const { return head_.status; }
  bool chunked() const { return mode_ == kChunked; }

 private:
  enum Mode { kUntilClose, kChunked, kLength };

  HeadParser head_;
  ChunkedDecoder chunked_;
  LineSplitter lines_;
  std::string scratch_;  // decoded chunk payload
  Mode mode_ = kUntilClose;
  size_t remaining_ = 0;  // kLength
  bool head_done_ = false;
  bool stream_end_ = false;
  bool flushed_ = false;  // unterminated tail already handed out
};

namespace detail {

// A condition variable whose timed waits run on CLOCK_MONOTONIC through
// pthread_cond_timedwait.  std::condition_variable's steady-clock waits use
// pthread_cond_clockwait, which the ThreadSanitizer of GCC 11 does not
// intercept (it then believes the mutex stays locked across the wait and
// reports races that are not there); this keeps the clock and stays
// checkable.
class MonotonicCond {
 public:
  MonotonicCond() {
    pthread_condattr_t attr;
    pthread_condattr_init(&attr);
    pthread_condattr_setclock(&attr, CLOCK_MONOTONIC);
    pthread_cond_init(&cond_, &attr);
    pthread_condattr_destroy(&attr);
  }
  ~MonotonicCond() { pthread_cond_destroy(&cond_); }
  MonotonicCond(const MonotonicCond&) = delete;
  MonotonicCond& operator=(const MonotonicCond&) = delete;

  void notify_all() { pthread_cond_broadcast(&cond_); }

  void wait(std::unique_lock<std::mutex>& hold) {
    pthread_cond_wait(&cond_, hold.mutex()->native_handle());
  }

  // false once `at` (CLOCK_MONOTONIC) has passed
  bool wait_until(std::unique_lock<std::mutex>& hold,
                  const struct timespec& at) {
    return pthread_cond_timedwait(&cond_, hold.mutex()->native_handle(),
                                  &at) != ETIMEDOUT;
  }

 private:
  pthread_cond_t cond_;
};

}  // namespace detail

// ---------------------------------------------------------------------------
// LineQueue: what a LinePump's reader thread hands to its consumers.  The
// producer publishes the response status, then lines, then the end of the
// stream; every push bumps a sequence counter and wakes all waiters.
// Consumers wait for the counter to pass what they have seen and drain
// everything pending at once.  Thread-safe.
// ---------------------------------------------------------------------------

class LineQueue {
 public:
  void set_head(int status) {
    std::lock_guard<std::mutex> hold(mu_);
    status_ = status;
    cv_.notify_all();
  }

  void push(std::string&& line) {
    std::lock_guard<std::mutex> hold(mu_);
    pending_.push_back(std::move(line));
    ++seq_;
    cv_.notify_all();
  }

  // End of stream: error is 0 for a clean end, a wire::Status (< 0) for
  // malformed framing, an errno (> 0) for a failed read.  The first wins.
  void end(int error) {
    std::lock_guard<std::mutex> hold(mu_);
    if (ended_) return;
    ended_ = true;
    error_ = error;
    cv_.notify_all();
  }

  // Block until the head has arrived or the stream has ended, for at most
  // timeout_s seconds (< 0: for ever).  Returns the status, 0 if there is
  // none yet.
  int wait_head(double timeout_s) {
    std::unique_lock<std::mutex> hold(mu_);
    wait_locked(hold, timeout_s, [this] { return status_ != 0 || ended_; });
    return status_;
  }

  // Block until more than `seen` lines have been pushed or the stream has
  // ended, for at most timeout_s seconds (< 0: for ever).  Returns the count.
  uint64_t wait(uint64_t seen, double timeout_s) {
    std::unique_lock<std::mutex> hold(mu_);
    wait_locked(hold, timeout_s, [&] { return seq_ > seen || ended_; });
    return seq_;
  }

  // Everything pending, oldest first.
  std::deque<std::string> drain() {
    std::deque<std::string> out;
    std::lock_guard<std::mutex> hold(mu_);
    out.swap(pending_);
    return out;
  }

  uint64_t seq() const {
    std::lock_guard<std::mutex> hold(mu_);
    return seq_;
  }

  size_t pending() const {
    std::lock_guard<std::mutex> hold(mu_);
    return pending_.size();
  }

  bool ended() const {
    std::lock_guard<std::mutex> hold(mu_);
    return ended_;
  }

  int error() const {
    std::lock_guard<std::mutex> hold(mu_);
    return error_;
  }

 private:
  template <class Pred>
  void wait_locked(std::unique_lock<std::mutex>& hold, double timeout_s,
                   Pred pred) {
    if (timeout_s < 0) {
      while (!pred()) cv_.wait(hold);
      return;
    }
    struct timespec at;
    clock_gettime(CLOCK_MONOTONIC, &at);
    double whole = std::floor(timeout_s);
    at.tv_sec += time_t(whole);
    at.tv_nsec += long((timeout_s - whole) * 1e9);
    if (at.tv_nsec >= 1000000000L) {
      at.tv_nsec -= 1000000000L;
      ++at.tv_sec;
    }
    while (!pred())
      if (!cv_.wait_until(hold, at)) return;
  }

  mutable std::mutex mu_;
  detail::MonotonicCond cv_;
  std::deque<std::string> pending_;
  uint64_t seq_ = 0;
  int status_ = 0;
  bool ended_ = false;
  int error_ = 0;
};

}  // namespace wire
