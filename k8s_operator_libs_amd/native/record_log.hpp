// record_log.hpp — the capped mismatch log of the checks that record what they
// found: records of type R in device memory behind one claim counter.  The
// counter is a word of the check's own block of 64-bit counters, which the
// log owns, so counters and claims come back in one download.  Like the
// holders it is built from, a log lives for one call.

#pragma once

#include <vector>

#include "hip_util.hpp"
#include "validator_problems.hpp"

template <typename R>
struct RecordLogView {
  unsigned long long* claims;
  R* records;
  uint32_t cap;
};

// `make()` gives the record; it runs only for a claim that got a slot
template <typename R, typename Make>
__device__ __forceinline__ void record_log_claim(const RecordLogView<R>& log,
                                                 Make make) {
  const unsigned long long slot = atomicAdd(log.claims, 1ull);
  if (slot < log.cap) log.records[slot] = make();  // past the cap: dropped
}

template <typename R>
class RecordLog {
 public:
  // `capacity` records and `ctl_words` counters, zeroed; the claim counter is
  // word `claim_word` of them
  RecordLog(size_t capacity, size_t ctl_words, size_t claim_word)
      : ctl_(ctl_words), records_(capacity), claim_word_(claim_word) {
    ctl_.fill(0);
    records_.fill(0);
  }
  unsigned long long* ctl() const { return ctl_.get(); }
  RecordLogView<R> view(size_t cap) const {
    return {ctl_.get() + claim_word_, records_.get(), (uint32_t)cap};
  }

  struct Collected {
    std::vector<unsigned long long> ctl;  // every counter of the block
    uint64_t claims;
    std::vector<R> records;  // the first min(claims, cap)
  };
  // After a synchronise.  `rezero` clears the counters for a next phase.
  Collected collect(size_t cap, bool rezero = false) {
    Collected c{std::vector<unsigned long long>(ctl_.size()), 0, {}};
    ctl_.download(c.ctl.data(), c.ctl.size());
    c.claims = c.ctl[claim_word_];
    c.records.resize(record_log_kept(c.claims, cap));
    if (!c.records.empty()) records_.download(c.records.data(), c.records.size());
    if (rezero) ctl_.fill(0);
    return c;
  }

 private:
  DeviceBuf<unsigned long long> ctl_;
  DeviceBuf<R> records_;
  size_t claim_word_;
};
