// wire_core_selftest.cpp — stand-alone checks of the wire_core.hpp parsers.
//
// Built with -fsanitize=address,undefined by tests/test_wire_native.py and
// run as a child process.  Every canned stream is fed to its parser whole,
// split in two at EVERY byte offset, and one byte at a time; all three must
// give the same result.  Malformed streams must return their defined error
// (and, under the sanitizers, touch nothing out of bounds).
//
// The three big streams (a 65 KiB head, a head of exactly 64 KiB, a 1 MiB
// line) are NOT cut at every offset: a two-piece run copies the whole stream,
// so every offset would cost gigabytes of copying.  They are cut on a coarse
// stride, at every offset in a window around each place where a boundary bug
// could sit (the 64 KiB cap, the head's terminator, the LFs of the big
// line), and byte-at-a-time.  Every other stream is cut at every offset.
//
// Each piece is copied into an exactly-sized heap block before it is fed, so
// a parser that reads past the end of its input trips AddressSanitizer.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "wire_core.hpp"

namespace {

int g_failures = 0;
int g_checks = 0;

#define CHECK(cond)                                                     \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(cond)) {                                                      \
      ++g_failures;                                                     \
      if (g_failures < 20)                                              \
        std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,    \
                     #cond);                                            \
    }                                                                   \
  } while (0)

// How a stream is cut into pieces: [0,split) then the rest; split == npos
// means whole; step == 1 means byte-at-a-time.
struct Cut {
  size_t split;
  bool bytewise;
};

std::vector<std::string> pieces(const std::string& s, const Cut& cut) {
  std::vector<std::string> out;
  if (cut.bytewise) {
    for (char c : s) out.emplace_back(1, c);
  } else if (cut.split == std::string::npos) {
    out.push_back(s);
  } else {
    out.push_back(s.substr(0, cut.split));
    out.push_back(s.substr(cut.split));
  }
  return out;
}

// offsets where a coarse stride is topped up with every cut in +-kDenseSpan
using Dense = std::vector<size_t>;
constexpr size_t kDenseSpan = 12;

std::vector<Cut> all_cuts(const std::string& s, size_t stride = 1,
                          const Dense& dense = {}) {
  std::vector<Cut> cuts;
  cuts.push_back({std::string::npos, false});
  for (size_t i = 0; i <= s.size(); i += stride) cuts.push_back({i, false});
  for (size_t centre : dense) {
    size_t lo = centre > kDenseSpan ? centre - kDenseSpan : 0;
    size_t hi = centre + kDenseSpan < s.size() ? centre + kDenseSpan : s.size();
    for (size_t i = lo; i <= hi; ++i) cuts.push_back({i, false});
  }
  cuts.push_back({0, true});
  return cuts;
}

// exact-size heap copy of a piece (ASan red zones right behind it)
struct Exact {
  char* p;
  size_t n;
  explicit Exact(const std::string& s) : p(nullptr), n(s.size()) {
    p = static_cast<char*>(std::malloc(n ? n : 1));
    if (n) std::memcpy(p, s.data(), n);
  }
  ~Exact() { std::free(p); }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

// -- heads -------------------------------------------------------------------

struct HeadResult {
  int st = wire::kNeedMore;
  size_t consumed = 0;  // bytes of the stream that belong to the head(s)
  int status = 0;
  std::string method, target;
  int minor = -1;
  bool has_len = false;
  size_t len = 0;
  bool chunked = false, close = false, keep_alive = false;
  int interim = 0;  // 1xx responses skipped

  bool operator==(const HeadResult& o) const {
    return st == o.st && consumed == o.consumed && status == o.status &&
           method == o.method && target == o.target && minor == o.minor &&
           has_len == o.has_len && len == o.len && chunked == o.chunked &&
           close == o.close && keep_alive == o.keep_alive &&
           interim == o.interim;
  }
};

HeadResult run_head(wire::HeadParser::Kind kind, const std::string& stream,
                    const Cut& cut) {
  wire::HeadParser hp(kind);
  HeadResult r;
  for (const std::string& piece : pieces(stream, cut)) {
    Exact e(piece);
    size_t off = 0;
    while (off < e.n) {
      size_t used = 0;
      int st = hp.feed(e.p + off, e.n - off, &used);
      off += used;
      r.consumed += used;
      if (st == wire::kDone && kind == wire::HeadParser::kResponse &&
          hp.status >= 100 && hp.status < 200) {
        ++r.interim;
        hp.reset();
        continue;
      }
      r.st = st;
      if (st != wire::kNeedMore) goto finished;
    }
  }
finished:
  if (r.st == wire::kDone) {
    r.status = hp.status;
    r.method = hp.method;
    r.target = hp.target;
    r.minor = hp.version_minor;
    r.has_len = hp.has_content_length;
    r.len = hp.content_length;
    r.chunked = hp.chunked;
    r.close = hp.connection_close;
    r.keep_alive = hp.keep_alive();
  }
  return r;
}

// run under every cut; all results equal; returns the whole-feed result
HeadResult head_all_cuts(wire::HeadParser::Kind kind, const std::string& s,
                         size_t stride = 1, const Dense& dense = {}) {
  HeadResult whole = run_head(kind, s, {std::string::npos, false});
  for (const Cut& cut : all_cuts(s, stride, dense)) {
    HeadResult r = run_head(kind, s, cut);
    CHECK(r == whole);
  }
  return whole;
}

void test_response_heads() {
  const auto R = wire::HeadParser::kResponse;
  {
    std::string s = "HTTP/1.1 200 OK\r\nContent-Length: 0\r\n\r\n";
    HeadResult r = head_all_cuts(R, s);
    CHECK(r.st == wire::kDone);
    CHECK(r.status == 200 && r.has_len && r.len == 0);
    CHECK(!r.chunked && !r.close && r.keep_alive);
    CHECK(r.consumed == s.size());
  }
  {  // mixed-case names, optional whitespace, body bytes after the head
    std::string head =
        "HTTP/1.1 409 Conflict\r\ncOnTeNt-LeNgTh:   42  \r\n"
        "CONNECTION:\tClose\r\nX-Other: a:b\r\n\r\n";
    std::string s = head + "{\"kind\":\"Status\"}";
    HeadResult r = head_all_cuts(R, s);
    CHECK(r.st == wire::kDone);
    CHECK(r.status == 409 && r.has_len && r.len == 42);
    CHECK(r.close && !r.keep_alive);
    CHECK(r.consumed == head.size());
  }
  {
    std::string s =
        "HTTP/1.1 200 OK\r\ntransfer-ENCODING: gzip, Chunked\r\n\r\n";
    HeadResult r = head_all_cuts(R, s);
    CHECK(r.st == wire::kDone && r.chunked && !r.has_len);
  }
  {  // a 100-continue followed by a 200
    std::string s =
        "HTTP/1.1 100 Continue\r\n\r\n"
        "HTTP/1.1 200 OK\r\nContent-Length: 7\r\n\r\n";
    HeadResult r = head_all_cuts(R, s);
    CHECK(r.st == wire::kDone && r.interim == 1);
    CHECK(r.status == 200 && r.len == 7 && r.consumed == s.size());
  }
  {  // HTTP/1.0: no keep-alive unless asked for
    HeadResult r = head_all_cuts(R, "HTTP/1.0 200 OK\r\n\r\n");
    CHECK(r.st == wire::kDone && r.minor == 0 && !r.keep_alive);
    r = head_all_cuts(R, "HTTP/1.0 200 OK\r\nConnection: keep-alive\r\n\r\n");
    CHECK(r.st == wire::kDone && r.keep_alive);
  }
  {  // no reason phrase
    HeadResult r = head_all_cuts(R, "HTTP/1.1 204\r\n\r\n");
    CHECK(r.st == wire::kDone && r.status == 204);
  }
  // malformed
  CHECK(head_all_cuts(R, "HTTP/1.1 200 OK\r\nNoColonHere\r\n\r\n").st ==
        wire::kErrBadHead);
  CHECK(head_all_cuts(R, "HTTP/1.1 200 OK\nContent-Length: 0\n\n").st ==
        wire::kErrBadHead);
  CHECK(head_all_cuts(R, "HTTP/1.1 200 OK\r\nContent-Length: -1\r\n\r\n").st ==
        wire::kErrBadLength);
  CHECK(head_all_cuts(
            R, "HTTP/1.1 200 OK\r\nContent-Length: 99999999999999999999\r\n\r\n")
            .st == wire::kErrBadLength);
  CHECK(head_all_cuts(R, "HTTP/1.1 200 OK\r\nContent-Length: 12abc\r\n\r\n").st ==
        wire::kErrBadLength);
  CHECK(head_all_cuts(R, "HTTP/1.1 200 OK\r\nContent-Length:\r\n\r\n").st ==
        wire::kErrBadLength);
  CHECK(head_all_cuts(R,
                      "HTTP/1.1 200 OK\r\nContent-Length: 1\r\n"
                      "Content-Length: 2\r\n\r\n").st == wire::kErrBadLength);
  CHECK(head_all_cuts(R, "HTTP/2 200 OK\r\n\r\n").st == wire::kErrBadHead);
  CHECK(head_all_cuts(R, "HTTP/1.1 2x0 OK\r\n\r\n").st == wire::kErrBadHead);
  CHECK(head_all_cuts(R, "\r\n").st == wire::kErrBadHead);
  CHECK(head_all_cuts(R, "HTTP/1.1 200 OK\r\nName : v\r\n\r\n").st ==
        wire::kErrBadHead);
  {  // a 65 KiB head: refused at the cap, not truncated
    std::string s = "HTTP/1.1 200 OK\r\nX-Pad: ";
    s.append(65 * 1024, 'a');
    s += "\r\nContent-Length: 3\r\n\r\n";
    HeadResult r = head_all_cuts(R, s, 997, {0, wire::kMaxHead, s.size()});
    CHECK(r.st == wire::kErrHeadTooLarge);
    CHECK(r.consumed == wire::kMaxHead);
  }
  {  // a head of exactly 64 KiB still parses
    std::string s = "HTTP/1.1 200 OK\r\nX-Pad: ";
    std::string tail = "\r\nContent-Length: 3\r\n\r\n";
    s.append(wire::kMaxHead - s.size() - tail.size(), 'a');
    s += tail;
    HeadResult r = head_all_cuts(
        R, s, 1009, {0, s.size() - tail.size(), wire::kMaxHead});
    CHECK(s.size() == wire::kMaxHead);
    CHECK(r.st == wire::kDone && r.len == 3);
  }
  {  // incomplete head: still waiting, never an error
    HeadResult r = head_all_cuts(R, "HTTP/1.1 200 OK\r\nContent-Le");
    CHECK(r.st == wire::kNeedMore);
  }
}

void test_request_heads() {
  const auto Q = wire::HeadParser::kRequest;
  {
    std::string head =
        "PATCH /api/v1/nodes/n1?x=1 HTTP/1.1\r\nHost: 127.0.0.1:80\r\n"
        "content-length: 17\r\n\r\n";
    HeadResult r = head_all_cuts(Q, head + "{\"a\":1}");
    CHECK(r.st == wire::kDone);
    CHECK(r.method == "PATCH" && r.target == "/api/v1/nodes/n1?x=1");
    CHECK(r.minor == 1 && r.has_len && r.len == 17 && r.keep_alive);
    CHECK(r.consumed == head.size());
  }
  {
    HeadResult r =
        head_all_cuts(Q, "GET / HTTP/1.1\r\nConnection: close\r\n\r\n");
    CHECK(r.st == wire::kDone && !r.keep_alive && !r.has_len);
  }
  {
    HeadResult r = head_all_cuts(Q, "GET / HTTP/1.0\r\n\r\n");
    CHECK(r.st == wire::kDone && r.minor == 0 && !r.keep_alive);
  }
  CHECK(head_all_cuts(Q, "GET /\r\n\r\n").st == wire::kErrBadHead);
  CHECK(head_all_cuts(Q, "GET  HTTP/1.1\r\n\r\n").st == wire::kErrBadHead);
  CHECK(head_all_cuts(Q, "GET / HTTP/1.1\r\nbroken\r\n\r\n").st ==
        wire::kErrBadHead);
  CHECK(head_all_cuts(Q, "GET / HTTP/1.1\nHost: x\n\n").st == wire::kErrBadHead);
  CHECK(head_all_cuts(Q, "POST / HTTP/1.1\r\nContent-Length: -1\r\n\r\n").st ==
        wire::kErrBadLength);
}

// -- chunked body + line splitter ---------------------------------------------

struct BodyResult {
  int st = wire::kNeedMore;
  size_t consumed = 0;
  std::string payload;
  std::vector<std::string> lines;
  int line_st = wire::kNeedMore;

  bool operator==(const BodyResult& o) const {
    return st == o.st && consumed == o.consumed && payload == o.payload &&
           lines == o.lines && line_st == o.line_st;
  }
};

// chunked stream -> payload -> lines (drained after every piece, as the
// extension does)
BodyResult run_chunked(const std::string& stream, const Cut& cut) {
  wire::ChunkedDecoder dec;
  wire::LineSplitter split;
  BodyResult r;
  std::string line;
  for (const std::string& piece : pieces(stream, cut)) {
    Exact e(piece);
    std::string out;
    size_t used = 0;
    int st = dec.feed(e.p, e.n, &used, &out);
    r.consumed += used;
    r.payload += out;
    Exact payload(out);
    split.feed(payload.p, payload.n);
    int ls;
    while ((ls = split.next(&line)) == wire::kDone) r.lines.push_back(line);
    r.line_st = ls;
    r.st = st;
    if (st != wire::kNeedMore) break;
  }
  return r;
}

BodyResult chunked_all_cuts(const std::string& s, size_t stride = 1) {
  BodyResult whole = run_chunked(s, {std::string::npos, false});
  for (const Cut& cut : all_cuts(s, stride)) {
    BodyResult r = run_chunked(s, cut);
    CHECK(r == whole);
  }
  return whole;
}

std::string chunk(const std::string& data, const char* ext = "") {
  char size[32];
  std::snprintf(size, sizeof size, "%zx", data.size());
  return std::string(size) + ext + "\r\n" + data + "\r\n";
}

void test_chunked() {
  const std::string e1 = "{\"type\":\"ADDED\",\"object\":{\"n\":1}}";
  const std::string e2 = "{\"type\":\"MODIFIED\",\"object\":{\"n\":2}}";
  const std::string e3 = "{\"type\":\"DELETED\",\"object\":{\"n\":3}}";
  {
    // chunk boundaries inside a line; a size line of several hex digits (so
    // cuts fall inside it); an extension; blank keep-alive lines; trailers
    std::string pad(300, ' ');
    std::string body = chunk(e1.substr(0, 10)) +
                       chunk(e1.substr(10) + "\n" + e2.substr(0, 5), ";ext=1") +
                       chunk(e2.substr(5) + "\r\n\n\n" + pad + "\n" + e3 + "\n") +
                       "0\r\nX-Trailer: 1\r\nOther: 2\r\n\r\n";
    std::string s = body + "NEXT";  // bytes after the body are left alone
    BodyResult r = chunked_all_cuts(s);
    CHECK(r.st == wire::kDone);
    CHECK(r.consumed == body.size());
    CHECK(r.lines.size() == 3);
    if (r.lines.size() == 3) {
      CHECK(r.lines[0] == e1 && r.lines[1] == e2 && r.lines[2] == e3);
    }
  }
  {  // upper-case hex, empty body
    BodyResult r = chunked_all_cuts("A\r\n0123456789\r\n0\r\n\r\n");
    CHECK(r.st == wire::kDone && r.payload == "0123456789");
    r = chunked_all_cuts("0\r\n\r\n");
    CHECK(r.st == wire::kDone && r.payload.empty());
  }
  {  // unfinished body keeps waiting
    BodyResult r = chunked_all_cuts("5\r\nabc");
    CHECK(r.st == wire::kNeedMore && r.payload == "abc");
  }
  // malformed
  CHECK(chunked_all_cuts("zz\r\nabc\r\n0\r\n\r\n").st == wire::kErrBadChunk);
  CHECK(chunked_all_cuts("\r\n").st == wire::kErrBadChunk);
  CHECK(chunked_all_cuts("3\nabc\r\n").st == wire::kErrBadChunk);
  CHECK(chunked_all_cuts("3\r\nabcX\r\n").st == wire::kErrBadChunk);
  CHECK(chunked_all_cuts("3\r\nabc\rX").st == wire::kErrBadChunk);
  CHECK(chunked_all_cuts("3g\r\nabc\r\n").st == wire::kErrBadChunk);
  CHECK(chunked_all_cuts("fffffffffffffffff\r\nabc").st == wire::kErrBadChunk);
  CHECK(chunked_all_cuts("-1\r\n").st == wire::kErrBadChunk);
  {  // 16 hex digits fit size_t exactly on LP64: no overflow error
    wire::ChunkedDecoder dec;
    std::string out, s = "ffffffffffffffff\r\nab";
    size_t used = 0;
    int st = dec.feed(s.data(), s.size(), &used, &out);
    CHECK(sizeof(size_t) != 8 || (st == wire::kNeedMore && out == "ab"));
  }
}

// -- plain line streams --------------------------------------------------------

struct LinesResult {
  std::vector<std::string> lines;
  int st = wire::kNeedMore;
  std::string tail;
  bool has_tail = false;

  bool operator==(const LinesResult& o) const {
    return lines == o.lines && st == o.st && tail == o.tail &&
           has_tail == o.has_tail;
  }
};

LinesResult run_lines(const std::string& stream, const Cut& cut,
                      size_t max_line = wire::kMaxLine) {
  wire::LineSplitter split(max_line);
  LinesResult r;
  std::string line;
  for (const std::string& piece : pieces(stream, cut)) {
    Exact e(piece);
    split.feed(e.p, e.n);
    int st;
    while ((st = split.next(&line)) == wire::kDone) r.lines.push_back(line);
    r.st = st;
    if (st < 0) return r;
  }
  r.has_tail = split.flush(&line) == wire::kDone;
  if (r.has_tail) r.tail = line;
  return r;
}

LinesResult lines_all_cuts(const std::string& s, size_t stride = 1,
                           size_t max_line = wire::kMaxLine,
                           const Dense& dense = {}) {
  LinesResult whole = run_lines(s, {std::string::npos, false}, max_line);
  for (const Cut& cut : all_cuts(s, stride, dense)) {
    LinesResult r = run_lines(s, cut, max_line);
    CHECK(r == whole);
  }
  return whole;
}

void test_lines() {
  {  // three events in one feed, blank keep-alive lines, CRLF endings
    LinesResult r = lines_all_cuts("\n\n{\"a\":1}\n{\"b\":2}\r\n\n \n{\"c\":3}\n\n");
    CHECK(r.st == wire::kNeedMore && !r.has_tail);
    CHECK(r.lines.size() == 3);
    if (r.lines.size() == 3) {
      CHECK(r.lines[0] == "{\"a\":1}" && r.lines[1] == "{\"b\":2}" &&
            r.lines[2] == "{\"c\":3}");
    }
  }
  {  // partial line carried; unterminated tail only through flush()
    LinesResult r = lines_all_cuts("one\ntw");
    CHECK(r.lines.size() == 1 && r.has_tail && r.tail == "tw");
  }
  {  // a 1 MiB line between two short ones
    std::string big(1024 * 1024, 'x');
    std::string s = "head\n" + big + "\ntail\n";
    // dense around the LF before the big line and the LF after it
    LinesResult r = lines_all_cuts(s, 65521, wire::kMaxLine,
                                   {5, 5 + big.size(), s.size()});
    CHECK(r.lines.size() == 3);
    if (r.lines.size() == 3) {
      CHECK(r.lines[0] == "head" && r.lines[1] == big && r.lines[2] == "tail");
    }
    // byte-at-a-time over the whole MiB is covered by all_cuts' last entry
  }
  {  // the cap is an error, not a truncation (small cap: same code path)
    LinesResult r = lines_all_cuts("ok\n0123456789ABCDEF-too-long\nnext\n", 1, 16);
    CHECK(r.st == wire::kErrLineTooLong);
    CHECK(r.lines.size() == 1 && r.lines[0] == "ok");
    r = lines_all_cuts("0123456789ABCDEF\n", 1, 16);  // exactly at the cap
    CHECK(r.st == wire::kNeedMore && r.lines.size() == 1);
    // no terminator in sight and already past the cap
    r = lines_all_cuts("0123456789ABCDEFG", 1, 16);
    CHECK(r.st == wire::kErrLineTooLong);
  }
  CHECK(wire::kMaxLine == 64u * 1024u * 1024u);
  CHECK(wire::kMaxHead == 64u * 1024u);
}

}  // namespace

int main() {
  test_response_heads();
  test_request_heads();
  test_chunked();
  test_lines();
  if (g_failures) {
    std::fprintf(stderr, "wire_core selftest: %d of %d checks FAILED\n",
                 g_failures, g_checks);
    return 1;
  }
  std::printf("wire_core selftest: %d checks passed\n", g_checks);
  return 0;
}
