// wire_stream_selftest.cpp — stand-alone checks of wire_stream.hpp.
//
// Built and run twice by tests/test_watch_native.py, as a child process:
// once with -fsanitize=address,undefined and once with -fsanitize=thread.
//
//   LineQueue     sequence counter, wait (timeout, wake, end of stream) and
//                 drain under one producer and two consumers: every line is
//                 handed out exactly once and in order
//   StreamBuffer  direct send, partial send, flush in pieces, lines behind a
//                 backlog stay behind it, the cap (exactly full is fine, one
//                 byte more is dead), a failed send, and four writers against
//                 a sink that takes a few bytes at a time: no torn lines,
//                 each writer's lines in order
//   LineFramer    the same lines from read-until-close and from chunked
//                 framing fed a byte at a time; a malformed chunk is an error
//
// The sink below stands in for a socket: it takes at most `room` bytes and
// then reports that it would block.

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "wire_stream.hpp"

namespace {

std::atomic<int> g_failures{0};
std::atomic<int> g_checks{0};

#define CHECK(cond)                                                     \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(cond)) {                                                      \
      if (++g_failures < 20)                                            \
        std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,    \
                     #cond);                                            \
    }                                                                   \
  } while (0)

// ---------------------------------------------------------------------------
// LineQueue
// ---------------------------------------------------------------------------

void test_queue_basics() {
  wire::LineQueue q;
  CHECK(q.seq() == 0 && q.pending() == 0 && !q.ended());
  // nothing arrives: wait comes back at its timeout, unchanged
  auto t0 = std::chrono::steady_clock::now();
  CHECK(q.wait(0, 0.05) == 0);
  CHECK(std::chrono::steady_clock::now() - t0 >= std::chrono::milliseconds(45));
  CHECK(q.wait_head(0.0) == 0);
  q.set_head(200);
  CHECK(q.wait_head(-1.0) == 200);
  q.push("a");
  q.push("b");
  CHECK(q.seq() == 2 && q.pending() == 2);
  CHECK(q.wait(0, -1.0) == 2);  // already past 0: no blocking
  CHECK(q.wait(1, -1.0) == 2);
  std::deque<std::string> got = q.drain();
  CHECK(got.size() == 2 && got[0] == "a" && got[1] == "b");
  CHECK(q.pending() == 0 && q.seq() == 2);  // draining does not move seq
  CHECK(q.drain().empty());
  CHECK(q.wait(2, 0.01) == 2);  // caught up: waits, then times out
  q.end(wire::kErrBadChunk);
  q.end(0);  // the first end wins
  CHECK(q.ended() && q.error() == wire::kErrBadChunk);
  CHECK(q.wait(2, -1.0) == 2);  // ended: never blocks again
}

void test_queue_wakes_a_waiter() {
  wire::LineQueue q;
  std::atomic<bool> woke{false};
  std::thread waiter([&] {
    CHECK(q.wait(0, 10.0) == 1);
    woke = true;
  });
  std::this_thread::sleep_for(std::chrono::milliseconds(20));
  CHECK(!woke);
  q.push("x");
  waiter.join();
  CHECK(woke);
  std::thread ender([&] { CHECK(q.wait(~0ULL, 10.0) == 1); });
  std::this_thread::sleep_for(std::chrono::milliseconds(20));
  q.end(0);
  ender.join();
}

void test_queue_one_producer_two_consumers() {
  constexpr int kLines = 4000;
  wire::LineQueue q;
  std::vector<int> got[2];
  auto consume = [&](int who) {
    for (;;) {
      uint64_t seen = q.seq();  // before the drain: no line is slept through
      for (std::string& line : q.drain()) got[who].push_back(std::stoi(line));
      if (q.ended() && q.pending() == 0) return;
      q.wait(seen, 1.0);
    }
  };
  std::thread c0(consume, 0), c1(consume, 1);
  std::thread producer([&] {
    for (int i = 0; i < kLines; ++i) {
      q.push(std::to_string(i));
      if (i % 97 == 0) std::this_thread::yield();
    }
    q.end(0);
  });
  producer.join();
  c0.join();
  c1.join();
  CHECK(q.seq() == uint64_t(kLines));
  CHECK(got[0].size() + got[1].size() == size_t(kLines));
  std::vector<int> seen(kLines, 0);
  for (int who = 0; who < 2; ++who) {
    for (size_t i = 0; i < got[who].size(); ++i) {
      int v = got[who][i];
      if (v >= 0 && v < kLines) ++seen[size_t(v)];
      if (i > 0) CHECK(got[who][i - 1] < v);  // each consumer sees them in order
    }
  }
  bool exactly_once = true;
  for (int n : seen) exactly_once = exactly_once && n == 1;
  CHECK(exactly_once);
}

// ---------------------------------------------------------------------------
// StreamBuffer
// ---------------------------------------------------------------------------

struct Sink {
  std::string data;             // touched only inside send (the buffer's lock)
  std::atomic<long> room{0};    // bytes it still takes
  long piece = 1 << 20;         // at most this many per call
  bool broken = false;
  int calls = 0;

  long send(const char* p, size_t n) {
    ++calls;
    if (broken) return wire::kSendFailed;
    long r = room.load();
    if (r <= 0) return wire::kSendWouldBlock;
    long take = long(n) < r ? long(n) : r;
    if (take > piece) take = piece;
    data.append(p, size_t(take));
    room -= take;
    return take;
  }
};

using SB = wire::StreamBuffer;

void test_backlog_single_thread() {
  Sink sink;
  auto send = [&](const char* p, size_t n) { return sink.send(p, n); };
  SB buf(16);
  sink.room = 100;
  CHECK(buf.write("one\n", 4, send) == SB::kSent);
  CHECK(sink.data == "one\n" && buf.pending() == 0);
  // the sink takes 5 of 12 bytes: the tail waits
  sink.room = 5;
  CHECK(buf.write("hello world\n", 12, send) == SB::kQueued);
  CHECK(sink.data == "one\nhello" && buf.pending() == 7);
  // a line behind a backlog is not offered to the sink, even if it has room
  sink.room = 0;
  int calls = sink.calls;
  CHECK(buf.write("x\n", 2, send) == SB::kQueued);
  CHECK(sink.calls == calls && buf.pending() == 9);
  CHECK(buf.flush(send) == SB::kQueued && buf.pending() == 9);  // still full
  sink.room = 3;
  CHECK(buf.flush(send) == SB::kQueued && buf.pending() == 6);
  sink.room = 100;
  sink.piece = 2;  // in pieces of two bytes
  CHECK(buf.flush(send) == SB::kSent && buf.pending() == 0);
  CHECK(sink.data == "one\nhello world\nx\n");
  CHECK(buf.flush(send) == SB::kSent);  // nothing to do
  CHECK(!buf.dead());

  // the cap: exactly full is accepted, one byte more is not
  sink.room = 0;
  CHECK(buf.write("0123456789\n", 11, send) == SB::kQueued);
  CHECK(buf.write("abcd\n", 5, send) == SB::kQueued);
  CHECK(buf.pending() == 16);
  CHECK(buf.write("!", 1, send) == SB::kDead);
  CHECK(buf.dead() && buf.pending() == 0);
  sink.room = 100;
  CHECK(buf.write("late\n", 5, send) == SB::kDead);
  CHECK(buf.flush(send) == SB::kDead);
  CHECK(sink.data == "one\nhello world\nx\n");  // nothing torn, nothing late

  // one write larger than the cap
  SB small(4);
  sink.room = 0;
  CHECK(small.write("too long\n", 9, send) == SB::kDead);

  // what the sink took before it filled up does not count against the cap
  SB part(4);
  sink.data.clear();
  sink.room = 6;
  sink.piece = 1 << 20;
  CHECK(part.write("123456789\n", 10, send) == SB::kQueued);
  CHECK(part.pending() == 4 && sink.data == "123456");

  // a failed send, direct and from the backlog
  SB a(64), b(64);
  sink.broken = true;
  CHECK(a.write("x\n", 2, send) == SB::kDead && a.dead());
  sink.broken = false;
  sink.room = 0;
  CHECK(b.write("x\n", 2, send) == SB::kQueued);
  sink.broken = true;
  CHECK(b.flush(send) == SB::kDead && b.dead());
  SB c(64);
  c.kill();
  CHECK(c.dead());
}

void test_backlog_no_torn_lines() {
  constexpr int kWriters = 4, kLines = 600;
  Sink sink;
  sink.piece = 7;
  auto send = [&](const char* p, size_t n) { return sink.send(p, n); };
  SB buf(size_t(1) << 24);
  std::atomic<bool> done{false};
  std::thread flusher([&] {  // the socket drains in fits and starts
    unsigned step = 0;
    while (!done) {
      sink.room += long(1 + (step++ * 37) % 300);
      buf.flush(send);
      std::this_thread::yield();
    }
  });
  std::vector<std::thread> writers;
  for (int w = 0; w < kWriters; ++w) {
    writers.emplace_back([&, w] {
      for (int i = 0; i < kLines; ++i) {
        std::string line = "w" + std::to_string(w) + ":" + std::to_string(i) +
                           ":" + std::string(size_t((i * 13 + w) % 90), 'x') +
                           "\n";
        CHECK(buf.write(line.data(), line.size(), send) != SB::kDead);
      }
    });
  }
  for (auto& t : writers) t.join();
  done = true;
  flusher.join();
  sink.room = long(1) << 30;
  sink.piece = 1 << 20;
  CHECK(buf.flush(send) == SB::kSent);
  // every line whole, each writer's lines in order
  int next[kWriters] = {0, 0, 0, 0};
  size_t pos = 0, lines = 0;
  bool whole = true;
  while (pos < sink.data.size()) {
    size_t lf = sink.data.find('\n', pos);
    if (lf == std::string::npos) { whole = false; break; }
    std::string line = sink.data.substr(pos, lf - pos);
    pos = lf + 1;
    ++lines;
    int w = -1, i = -1;
    int fill = 0;
    if (std::sscanf(line.c_str(), "w%d:%d:%n", &w, &i, &fill) != 2 || w < 0 ||
        w >= kWriters) { whole = false; break; }
    std::string tail = line.substr(size_t(fill));
    if (tail != std::string(size_t((i * 13 + w) % 90), 'x') || i != next[w]) {
      whole = false;
      break;
    }
    ++next[w];
  }
  CHECK(whole);
  CHECK(lines == size_t(kWriters * kLines));
}

// ---------------------------------------------------------------------------
// LineFramer
// ---------------------------------------------------------------------------

std::vector<std::string> frame(const std::string& stream, bool bytewise,
                               int* error) {
  wire::LineFramer f;
  std::vector<std::string> out;
  std::string line;
  *error = 0;
  auto take = [&] {
    int st;
    while ((st = f.next(&line)) == wire::kDone) out.push_back(line);
    if (st < 0) *error = st;
  };
  size_t step = bytewise ? 1 : stream.size();
  for (size_t i = 0; i < stream.size() && *error == 0; i += step) {
    // an exactly-sized copy: reading past the piece trips AddressSanitizer
    std::string piece = stream.substr(i, step);
    std::vector<char> exact(piece.begin(), piece.end());
    int st = f.consume(exact.data(), exact.size());
    if (st < 0) *error = st;
    else take();
  }
  if (*error == 0) {
    f.peer_closed();
    take();
  }
  return out;
}

void test_framer() {
  const std::vector<std::string> want = {"{\"a\":1}", "{\"b\":2}", "tail"};
  std::string plain =
      "HTTP/1.1 100 Continue\r\n\r\n"
      "HTTP/1.1 200 OK\r\nConnection: close\r\n\r\n"
      "{\"a\":1}\n\n\r\n{\"b\":2}\r\ntail";
  std::string chunked =
      "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
      "5\r\n{\"a\":\r\n4\r\n1}\n\n\r\nb\r\n\r\n{\"b\":2}\r\n\r\n4\r\ntail\r\n0\r\n\r\n";
  int error = 0;
  for (bool bytewise : {false, true}) {
    CHECK(frame(plain, bytewise, &error) == want && error == 0);
    CHECK(frame(chunked, bytewise, &error) == want && error == 0);
  }
  std::string bad =
      "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
      "3\r\nok\n\r\nZZ\r\nnope\r\n";
  std::vector<std::string> got = frame(bad, true, &error);
  CHECK(error == wire::kErrBadChunk);
  CHECK(got.size() == 1 && got[0] == "ok");
  wire::LineFramer f;
  f.peer_closed();  // closed before any head: no line, no flush
  std::string line;
  CHECK(f.next(&line) == wire::kNeedMore && !f.head_done() && f.stream_end());
}

}  // namespace

int main() {
  test_queue_basics();
  test_queue_wakes_a_waiter();
  test_queue_one_producer_two_consumers();
  test_backlog_single_thread();
  test_backlog_no_torn_lines();
  test_framer();
  if (g_failures.load() != 0) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures.load(),
                 g_checks.load());
    return 1;
  }
  std::printf("%d checks passed\n", g_checks.load());
  return 0;
}
