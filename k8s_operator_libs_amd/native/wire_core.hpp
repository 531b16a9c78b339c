// wire_core.hpp — Python-free HTTP/1.1 framing primitives.
//
// Incremental parsers over caller-supplied bytes: no Python.h, no sockets,
// no I/O.  wire.cpp wraps them for the REST client and the watch reader;
// tests/native/wire_core_selftest.cpp drives them stand-alone under
// sanitizers.  Every parser accepts its input in arbitrary pieces (down to
// one byte at a time) and gives the same result as for a single feed.
//
// Hard caps raise a defined error and never truncate:
//   - a message head larger than kMaxHead (64 KiB),
//   - a Content-Length that is non-numeric, negative or overflows size_t,
//   - a chunk size that is non-hex or overflows size_t,
//   - a single line longer than kMaxLine (64 MiB).

#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

namespace wire {

enum Status : int {
  kNeedMore = 0,  // input consumed, feed more bytes
  kDone = 1,      // element complete (head parsed / body ended / line ready)
  kErrHeadTooLarge = -1,
  kErrBadHead = -2,
  kErrBadLength = -3,
  kErrBadChunk = -4,
  kErrLineTooLong = -5,
};

inline const char* status_message(int st) {
  switch (st) {
    case kNeedMore: return "need more input";
    case kDone: return "done";
    case kErrHeadTooLarge: return "HTTP head larger than 64 KiB";
    case kErrBadHead: return "malformed HTTP head";
    case kErrBadLength: return "invalid Content-Length";
    case kErrBadChunk: return "malformed chunked framing";
    case kErrLineTooLong: return "line longer than the 64 MiB cap";
    default: return "unknown wire error";
  }
}

constexpr size_t kMaxHead = 64 * 1024;
constexpr size_t kMaxLine = 64u * 1024u * 1024u;

namespace detail {

inline char lower(char c) { return (c >= 'A' && c <= 'Z') ? char(c + 32) : c; }
inline bool is_ows(char c) { return c == ' ' || c == '\t'; }

// case-insensitive compare of [p, p+n) with a lower-case literal
inline bool ieq(const char* p, size_t n, const char* lit) {
  size_t m = std::strlen(lit);
  if (n != m) return false;
  for (size_t i = 0; i < n; ++i)
    if (lower(p[i]) != lit[i]) return false;
  return true;
}

// does the comma-separated token list [p, p+n) contain `lit` (lower-case)?
inline bool has_token(const char* p, size_t n, const char* lit) {
  size_t i = 0;
  while (i < n) {
    while (i < n && (is_ows(p[i]) || p[i] == ',')) ++i;
    size_t start = i;
    while (i < n && p[i] != ',') ++i;
    size_t end = i;
    while (end > start && is_ows(p[end - 1])) --end;
    if (ieq(p + start, end - start, lit)) return true;
  }
  return false;
}

// strict decimal size_t: digits only, at least one, no overflow
inline bool parse_size(const char* p, size_t n, size_t* out) {
  if (n == 0) return false;
  size_t v = 0;
  for (size_t i = 0; i < n; ++i) {
    if (p[i] < '0' || p[i] > '9') return false;
    size_t d = size_t(p[i] - '0');
    if (v > (SIZE_MAX - d) / 10) return false;
    v = v * 10 + d;
  }
  *out = v;
  return true;
}

}  // namespace detail

// ---------------------------------------------------------------------------
// Message head (response or request): accumulate up to CRLF CRLF, then parse.
// ---------------------------------------------------------------------------

class HeadParser {
 public:
  enum Kind { kResponse, kRequest };

  explicit HeadParser(Kind kind) : kind_(kind) { reset(); }

  void reset() {
    buf_.clear();
    line_start_ = 0;
    done_ = false;
    status = 0;
    version_minor = 1;
    method.clear();
    target.clear();
    has_content_length = false;
    content_length = 0;
    chunked = false;
    connection_close = false;
    connection_keep_alive = false;
  }

  // Consume bytes of the head from [data, data+n).  *consumed is how many of
  // them belong to the head (always n unless the head completed or failed
  // inside this piece).  Returns kNeedMore, kDone or an error.
  int feed(const char* data, size_t n, size_t* consumed) {
    size_t i = 0;
    if (done_) {
      *consumed = 0;
      return kDone;
    }
    while (i < n) {
      if (buf_.size() >= kMaxHead) {
        *consumed = i;
        return kErrHeadTooLarge;
      }
      char c = data[i++];
      buf_.push_back(c);
      if (c != '\n') continue;
      size_t end = buf_.size() - 1;  // index of the LF
      if (end == 0 || buf_[end - 1] != '\r') {
        *consumed = i;
        return kErrBadHead;  // bare LF
      }
      if (end - 1 == line_start_) {  // empty line: end of head
        *consumed = i;
        int st = parse();
        done_ = (st == kDone);
        return st;
      }
      line_start_ = end + 1;
    }
    *consumed = n;
    return kNeedMore;
  }

  // keep-alive as the server/client should treat this message
  bool keep_alive() const {
    if (version_minor >= 1) return !connection_close;
    return connection_keep_alive && !connection_close;
  }

  // response fields
  int status;
  // request fields
  std::string method;
  std::string target;
  // shared
  int version_minor;
  bool has_content_length;
  size_t content_length;
  bool chunked;
  bool connection_close;
  bool connection_keep_alive;

 private:
  int parse_version(const char* p, size_t n) {
    // "HTTP/1.x"
    if (n != 8 || std::memcmp(p, "HTTP/1.", 7) != 0) return kErrBadHead;
    if (p[7] < '0' || p[7] > '9') return kErrBadHead;
    version_minor = p[7] - '0';
    return kDone;
  }

  int parse_start_line(const char* p, size_t n) {
    if (kind_ == kResponse) {
      // HTTP/1.x SP 3DIGIT [SP reason]
      if (n < 12 || p[8] != ' ') return kErrBadHead;
      if (parse_version(p, 8) != kDone) return kErrBadHead;
      int code = 0;
      for (size_t i = 9; i < 12; ++i) {
        if (p[i] < '0' || p[i] > '9') return kErrBadHead;
        code = code * 10 + (p[i] - '0');
      }
      if (n > 12 && p[12] != ' ') return kErrBadHead;
      if (code < 100) return kErrBadHead;
      status = code;
      return kDone;
    }
    // METHOD SP target SP HTTP/1.x
    const char* sp1 = static_cast<const char*>(std::memchr(p, ' ', n));
    if (!sp1 || sp1 == p) return kErrBadHead;
    size_t rest = n - size_t(sp1 + 1 - p);
    const char* sp2 = static_cast<const char*>(std::memchr(sp1 + 1, ' ', rest));
    if (!sp2 || sp2 == sp1 + 1) return kErrBadHead;
    size_t vlen = n - size_t(sp2 + 1 - p);
    if (parse_version(sp2 + 1, vlen) != kDone) return kErrBadHead;
    method.assign(p, size_t(sp1 - p));
    target.assign(sp1 + 1, size_t(sp2 - sp1 - 1));
    return kDone;
  }

  int parse_header(const char* p, size_t n) {
    const char* colon = static_cast<const char*>(std::memchr(p, ':', n));
    if (!colon || colon == p) return kErrBadHead;
    size_t name_len = size_t(colon - p);
    // no whitespace inside or after the field name (RFC 9112 §5.1)
    for (size_t i = 0; i < name_len; ++i)
      if (detail::is_ows(p[i])) return kErrBadHead;
    const char* v = colon + 1;
    size_t vn = n - name_len - 1;
    while (vn && detail::is_ows(*v)) { ++v; --vn; }
    while (vn && detail::is_ows(v[vn - 1])) --vn;
    if (detail::ieq(p, name_len, "content-length")) {
      size_t len = 0;
      if (!detail::parse_size(v, vn, &len)) return kErrBadLength;
      if (has_content_length && len != content_length) return kErrBadLength;
      has_content_length = true;
      content_length = len;
    } else if (detail::ieq(p, name_len, "transfer-encoding")) {
      if (detail::has_token(v, vn, "chunked")) chunked = true;
    } else if (detail::ieq(p, name_len, "connection")) {
      if (detail::has_token(v, vn, "close")) connection_close = true;
      if (detail::has_token(v, vn, "keep-alive")) connection_keep_alive = true;
    }
    return kDone;
  }

  int parse() {
    const char* p = buf_.data();
    size_t total = buf_.size() - 2;  // drop the terminating empty line
    size_t pos = 0;
    bool first = true;
    while (pos < total) {
      // every line in buf_ ends in CRLF (feed() rejected bare LFs)
      const char* lf =
          static_cast<const char*>(std::memchr(p + pos, '\n', total - pos));
      size_t line_end = size_t(lf - p) - 1;  // index of the CR
      int st = first ? parse_start_line(p + pos, line_end - pos)
                     : parse_header(p + pos, line_end - pos);
      if (st != kDone) return st;
      first = false;
      pos = line_end + 2;
    }
    return first ? kErrBadHead : kDone;
  }

  Kind kind_;
  std::string buf_;
  size_t line_start_;
  bool done_;
};

// ---------------------------------------------------------------------------
// Chunked transfer-coding decoder.
// ---------------------------------------------------------------------------

class ChunkedDecoder {
 public:
  ChunkedDecoder() { reset(); }

  void reset() {
    state_ = kSizeFirst;
    remaining_ = 0;
    meta_len_ = 0;
    trailer_line_len_ = 0;
  }

  // Decode from [data, data+n), appending payload bytes to *out.  *consumed
  // is n unless the body ended (kDone) or failed inside this piece.
  int feed(const char* data, size_t n, size_t* consumed, std::string* out) {
    size_t i = 0;
    while (i < n) {
      if (state_ == kData) {
        size_t take = n - i < remaining_ ? n - i : remaining_;
        out->append(data + i, take);
        i += take;
        remaining_ -= take;
        if (remaining_ == 0) state_ = kDataCR;
        continue;
      }
      if (state_ == kEnd) break;
      char c = data[i++];
      switch (state_) {
        case kSizeFirst:
        case kSize: {
          int d = hex(c);
          if (d >= 0) {
            if (remaining_ > (SIZE_MAX >> 4)) return fail(consumed, i);
            remaining_ = (remaining_ << 4) | size_t(d);
            state_ = kSize;
          } else if (state_ == kSizeFirst) {
            return fail(consumed, i);  // a size line starts with a hex digit
          } else if (c == '\r') {
            state_ = kSizeLF;
          } else if (c == ';' || detail::is_ows(c)) {
            state_ = kExt;
          } else {
            return fail(consumed, i);
          }
          if (++meta_len_ > kMaxHead) return fail(consumed, i);
          break;
        }
        case kExt:  // chunk extensions are ignored
          if (c == '\r') state_ = kSizeLF;
          else if (c == '\n') return fail(consumed, i);
          if (++meta_len_ > kMaxHead) return fail(consumed, i);
          break;
        case kSizeLF:
          if (c != '\n') return fail(consumed, i);
          meta_len_ = 0;
          if (remaining_ == 0) {
            state_ = kTrailer;
            trailer_line_len_ = 0;
          } else {
            state_ = kData;
          }
          break;
        case kDataCR:
          if (c != '\r') return fail(consumed, i);
          state_ = kDataLF;
          break;
        case kDataLF:
          if (c != '\n') return fail(consumed, i);
          state_ = kSizeFirst;
          break;
        case kTrailer:
          if (c == '\r') state_ = kTrailerLF;
          else if (c == '\n') return fail(consumed, i);
          else ++trailer_line_len_;
          if (++meta_len_ > kMaxHead) return fail(consumed, i);
          break;
        case kTrailerLF:
          if (c != '\n') return fail(consumed, i);
          if (trailer_line_len_ == 0) {
            state_ = kEnd;
          } else {
            state_ = kTrailer;
            trailer_line_len_ = 0;
          }
          break;
        default:
          return fail(consumed, i);
      }
    }
    *consumed = i;
    return state_ == kEnd ? kDone : kNeedMore;
  }

  bool done() const { return state_ == kEnd; }

 private:
  enum State {
    kSizeFirst, kSize, kExt, kSizeLF, kData, kDataCR, kDataLF,
    kTrailer, kTrailerLF, kEnd, kFailed,
  };

  static int hex(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
  }

  int fail(size_t* consumed, size_t i) {
    state_ = kFailed;
    *consumed = i;
    return kErrBadChunk;
  }

  State state_;
  size_t remaining_;
  size_t meta_len_;  // bytes of size line / trailers since the last data
  size_t trailer_line_len_;
};

// ---------------------------------------------------------------------------
// One whole response to one request: head (interim 1xx responses skipped),
// then the body by Content-Length, chunked or read-until-close framing.
// ---------------------------------------------------------------------------

class ResponseReader {
 public:
  // head_request: the request was a HEAD, so the response carries no body
  explicit ResponseReader(bool head_request)
      : head_(HeadParser::kResponse), head_request_(head_request) {}

  // Consume bytes as they arrive.  kNeedMore, kDone (status/body/reusable
  // are final) or an error.  Bytes past the end of the response are not
  // consumed; they make the connection not reusable.
  int feed(const char* p, size_t n) {
    if (n > 0) started_ = true;
    while (n > 0 && phase_ != kComplete) {
      size_t used = 0;
      if (phase_ == kHead) {
        int st = head_.feed(p, n, &used);
        if (st < 0) return st;
        if (st == kDone) on_head();
      } else if (phase_ == kLength) {
        used = n < remaining_ ? n : remaining_;
        body_.append(p, used);
        remaining_ -= used;
        if (remaining_ == 0) phase_ = kComplete;
      } else if (phase_ == kChunked) {
        int st = chunked_.feed(p, n, &used, &body_);
        if (st < 0) return st;
        if (st == kDone) phase_ = kComplete;
      } else {  // kUntilClose
        used = n;
        body_.append(p, used);
      }
      p += used;
      n -= used;
    }
    if (n > 0) reusable_ = false;  // bytes past the response: do not reuse
    return phase_ == kComplete ? kDone : kNeedMore;
  }

  // The peer closed the connection.  True when that ends the response (a
  // read-until-close body); false when it cut the response short.
  bool peer_closed() {
    if (phase_ == kUntilClose) phase_ = kComplete;
    return phase_ == kComplete;
  }

  bool done() const { return phase_ == kComplete; }
  bool started() const { return started_; }  // any byte of a response seen
  int status() const { return head_.status; }
  bool reusable() const { return reusable_; }
  std::string& body() { return body_; }

 private:
  static bool status_has_no_body(int status) {
    return status == 204 || status == 304;
  }

  void on_head() {
    int code = head_.status;
    if (code >= 100 && code < 200 && code != 101) {
      head_.reset();  // interim response: skip it
      return;
    }
    if (!head_.keep_alive()) reusable_ = false;
    if (head_request_ || status_has_no_body(code)) {
      phase_ = kComplete;
    } else if (head_.chunked) {
      phase_ = kChunked;
    } else if (head_.has_content_length) {
      remaining_ = head_.content_length;
      if (remaining_ == 0) {
        phase_ = kComplete;
      } else {
        phase_ = kLength;
        // cap the up-front reservation: the length is peer-supplied
        body_.reserve(remaining_ < (size_t(1) << 26) ? remaining_
                                                     : (size_t(1) << 26));
      }
    } else {
      phase_ = kUntilClose;
      reusable_ = false;
    }
  }

  enum Phase { kHead, kLength, kChunked, kUntilClose, kComplete };

  HeadParser head_;
  ChunkedDecoder chunked_;
  std::string body_;
  Phase phase_ = kHead;
  size_t remaining_ = 0;
  bool head_request_;
  bool reusable_ = true;
  bool started_ = false;
};

// ---------------------------------------------------------------------------
// Line splitter: complete LF-terminated lines, blank ones skipped, a partial
// line carried across feeds.
// ---------------------------------------------------------------------------

class LineSplitter {
 public:
  explicit LineSplitter(size_t max_line = kMaxLine)
      : max_line_(max_line), pos_(0), scan_(0) {}

  void feed(const char* data, size_t n) {
    if (pos_ > 0 && pos_ == buf_.size()) {
      buf_.clear();
      pos_ = scan_ = 0;
    }
    buf_.append(data, n);
  }

  // Next non-blank line with surrounding whitespace (the CR included)
  // stripped.  kDone: *out holds the line; kNeedMore: no complete line yet;
  // kErrLineTooLong: the pending line exceeds the cap.
  int next(std::string* out) {
    for (;;) {
      const char* base = buf_.data();
      const char* lf = scan_ < buf_.size()
          ? static_cast<const char*>(
                std::memchr(base + scan_, '\n', buf_.size() - scan_))
          : nullptr;
      if (!lf) {
        scan_ = buf_.size();
        if (buf_.size() - pos_ > max_line_) return kErrLineTooLong;
        if (pos_ > 0) {  // compact so the buffer holds only the partial line
          buf_.erase(0, pos_);
          scan_ -= pos_;
          pos_ = 0;
        }
        return kNeedMore;
      }
      size_t end = size_t(lf - base);
      size_t start = pos_;
      pos_ = scan_ = end + 1;
      if (end - start > max_line_) return kErrLineTooLong;
      if (strip(base, start, end, out)) return kDone;
    }
  }

  // At end of stream: the unterminated tail, if it is not blank.
  int flush(std::string* out) {
    size_t start = pos_, end = buf_.size();
    pos_ = scan_ = end;
    if (end - start > max_line_) return kErrLineTooLong;
    return strip(buf_.data(), start, end, out) ? kDone : kNeedMore;
  }

  size_t pending() const { return buf_.size() - pos_; }

 private:
  static bool is_space(char c) {
    return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\f' ||
           c == '\v';
  }

  static bool strip(const char* base, size_t start, size_t end,
                    std::string* out) {
    while (start < end && is_space(base[start])) ++start;
    while (end > start && is_space(base[end - 1])) --end;
    if (start == end) return false;
    out->assign(base + start, end - start);
    return true;
  }

  size_t max_line_;
  std::string buf_;
  size_t pos_;   // start of the first unreturned byte
  size_t scan_;  // no LF in [pos_, scan_)
};

}  // namespace wire
