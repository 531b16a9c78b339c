// hostlink_problems_selftest.cpp — stand-alone checks of the host side of the
// host-link data-integrity check (native/hostlink_problems.hpp).
//
// Built with -fsanitize=address,undefined by tests/test_host_link_native.py and
// run as a child process, so the host fill, verify, plan and slot-compare
// loops run under the sanitizers on exactly sized heap buffers.  Copies are
// done here with memcpy, which stands in for a faultless link; deliberately
// wrong copies (shifted, one byte short, one byte long, not done at all) must
// each be caught by the whole-slot compare.

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "validator_problems.hpp"

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

template <typename F>
bool throws_invalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

void test_seed_rule_and_fill() {
  // splitmix64's first output for state 0 is the hash of word 0 under seed 1
  CHECK(hbm_pattern_value(kHbmPatternHash, 1, 0) == 0xE220A8397B1DCDAFull);
  CHECK(hostlink_seed(1, 0, 0) == 1 && hostlink_seed(1, 2, 5) == 38);
  CHECK(hostlink_data_phase(kHostlinkD2h) == kHostlinkH2d);
  CHECK(hostlink_data_phase(kHostlinkZcWrite) == kHostlinkZcRead);
  CHECK(hostlink_data_phase(kHostlinkDuplex) == kHostlinkDuplex);
  CHECK(hostlink_data_inverted(kHostlinkD2h) && !hostlink_data_inverted(kHostlinkH2d));
  CHECK(hostlink_kind_phases(kHostlinkPageable) == 0x23u);
  CHECK(hostlink_kind_phases(kHostlinkRegistered) == 0x3Fu);
  CHECK(hostlink_kind_phases(kHostlinkPinned) == 0x7Fu);

  const uint64_t n = 1031, first = 77;
  std::vector<uint64_t> buf(n);
  hostlink_fill(buf.data(), first, n, 9, false);
  for (uint64_t k = 0; k < n; ++k)
    CHECK(buf[k] == hbm_pattern_value(kHbmPatternHash, 9, first + k));
  HostlinkTally clean;
  hostlink_verify(buf.data(), first, n, 9, false, -1, 1, 4, clean);
  CHECK(clean.compared == n && clean.errors == 0 && clean.records.empty());

  // the hook changes the comparison only: got is the buffer's word
  HostlinkTally hooked;
  hostlink_verify(buf.data(), first, n, 9, false, (int64_t)first + 5, 1ull << 40, 4,
                  hooked);
  CHECK(hooked.compared == n && hooked.errors == 1 && hooked.records.size() == 1);
  CHECK(hooked.records[0].word == first + 5 && hooked.records[0].got == buf[5]);
  CHECK((hooked.records[0].expected ^ hooked.records[0].got) == 1ull << 40);
  CHECK(hooked.xor_or == 1ull << 40);
  // a hook word outside the compared range does nothing
  HostlinkTally outside;
  hostlink_verify(buf.data(), first, n, 9, false, (int64_t)(first + n), 1, 4, outside);
  CHECK(outside.errors == 0);

  // a transfer that did not happen: the inverse is expected, every bit differs
  HostlinkTally stale;
  hostlink_verify(buf.data(), first, n, 9, true, -1, 1, 4, stale);
  CHECK(stale.compared == n && stale.errors == n && stale.xor_or == ~0ull);
  CHECK(stale.records.size() == 4 && stale.dropped == n - 4);
  HostlinkTally capless;
  hostlink_verify(buf.data(), first, n, 9, true, -1, 1, 0, capless);
  CHECK(capless.records.empty() && capless.dropped == n && capless.errors == n);

  hostlink_fill(buf.data(), first, n, 9, true);
  HostlinkTally inverted;
  hostlink_verify(buf.data(), first, n, 9, true, -1, 1, 4, inverted);
  CHECK(inverted.errors == 0);
  // another seed's words never pass
  HostlinkTally other;
  hostlink_verify(buf.data(), first, n, 10, true, -1, 1, 0, other);
  CHECK(other.errors == n);
}

void test_plan() {
  const HostlinkPlan plan = hostlink_plan();
  CHECK(plan.cases.size() == 464 && kHostlinkCases == 464);
  CHECK(plan.slot_bytes % 4096 == 0 && plan.slot_bytes == kHostlinkSlotBytes);
  CHECK(plan.guard >= 64);
  std::set<std::tuple<int, size_t, size_t, size_t>> seen;
  std::set<size_t> lens;
  for (size_t i = 0; i < plan.cases.size(); ++i) {
    const HostlinkCase& c = plan.cases[i];
    CHECK(c.index == (int)i);
    CHECK(c.direction == (i < 232 ? 0 : 1));
    seen.insert(std::make_tuple(c.direction, c.len, c.src_off, c.dst_off));
    lens.insert(c.len);
    CHECK(c.len >= 1);
    CHECK(c.src_pos() >= 64 && c.dst_pos() >= 64);
    CHECK(c.src_pos() + c.len + 64 <= plan.slot_bytes);
    CHECK(c.dst_pos() + c.len + 64 <= plan.slot_bytes);
  }
  CHECK(seen.size() == 464);  // every (direction, length, offset pair) once
  CHECK(lens.size() == 29 && *lens.begin() == 1 && *lens.rbegin() == 65537);
}

// the link of this program: a faultless copy of a case into dst
void copy_case(std::vector<uint8_t>& dst, const std::vector<uint8_t>& src,
               const HostlinkCase& c, long shift_dst, long extra_len) {
  std::memcpy(dst.data() + c.dst_pos() + shift_dst, src.data() + c.src_pos(),
              (size_t)((long)c.len + extra_len));
}

void test_slot_compare() {
  const HostlinkPlan plan = hostlink_plan();
  const uint64_t src_seed = hostlink_seed(3, 1, kHostlinkUnaligned);
  const uint64_t bg_seed = hostlink_seed(3, 1, kHostlinkBackground);
  // the largest case at the largest offsets, the smallest, one in the middle,
  // in both directions
  std::vector<int> picks;
  for (const HostlinkCase& c : plan.cases)
    if ((c.len == 65537 && c.src_off == 129) || (c.len == 1 && c.src_off == 63) ||
        (c.len == 4097 && c.src_off == 1 && c.dst_off == 2))
      picks.push_back(c.index);
  CHECK(picks.size() == 6);
  for (const int idx : picks) {
    const HostlinkCase& c = plan.cases[(size_t)idx];
    // exactly sized heap buffers: a byte outside a slot is a sanitizer report
    std::vector<uint8_t> src(plan.slot_bytes), dst(plan.slot_bytes);
    hostlink_slot_fill(src.data(), src_seed, c.index);
    CHECK(src[9] == hostlink_slot_byte(src_seed, c.index, 9));
    CHECK(src[plan.slot_bytes - 1] ==
          hostlink_slot_byte(src_seed, c.index, plan.slot_bytes - 1));

    const auto compare = [&](uint8_t poison, size_t cap) {
      HostlinkSlotTally t;
      hostlink_slot_compare(dst.data(), c, src_seed, bg_seed, poison, cap, t);
      CHECK(t.compared == plan.slot_bytes);
      return t;
    };
    const auto reset = [&] { hostlink_slot_fill(dst.data(), bg_seed, c.index); };

    reset();
    copy_case(dst, src, c, 0, 0);
    CHECK(compare(0, 8).errors == 0);
    // independent of the expected-image helper: the payload is the source's
    // bytes and the neighbours are the background's
    CHECK(dst[c.dst_pos()] == src[c.src_pos()]);
    CHECK(dst[c.dst_pos() + c.len - 1] == src[c.src_pos() + c.len - 1]);
    CHECK(dst[c.dst_pos() - 1] == hostlink_slot_byte(bg_seed, c.index, c.dst_pos() - 1));
    CHECK(dst[c.dst_pos() + c.len] ==
          hostlink_slot_byte(bg_seed, c.index, c.dst_pos() + c.len));

    // the hook: one error at the first payload byte, memory untouched
    const HostlinkSlotTally hooked = compare(0x10, 8);
    CHECK(hooked.errors == 1 && hooked.records.size() == 1);
    CHECK(hooked.records[0].offset == c.dst_pos());
    CHECK(hooked.records[0].case_index == c.index);
    CHECK(hooked.records[0].got == src[c.src_pos()]);
    CHECK((hooked.records[0].expected ^ hooked.records[0].got) == 0x10);

    // a copy that did not happen
    reset();
    const HostlinkSlotTally none = compare(0, 0);
    CHECK(none.errors > 0 && none.errors <= c.len && none.records.empty());
    CHECK(none.dropped == none.errors);
    if (c.len >= 4097) CHECK(none.errors > c.len - c.len / 64);

    // deliberately wrong copies: each must be a mismatch
    reset();
    copy_case(dst, src, c, 1, 0);  // starts one byte late
    CHECK(compare(0, 8).errors > 0);
    reset();
    copy_case(dst, src, c, -1, 0);  // starts one byte early
    CHECK(compare(0, 8).errors > 0);
    reset();
    copy_case(dst, src, c, 0, 1);  // one byte too many
    {
      const HostlinkSlotTally t = compare(0, 8);
      const bool same = src[c.src_pos() + c.len] ==
                        hostlink_slot_byte(bg_seed, c.index, c.dst_pos() + c.len);
      CHECK(t.errors == (same ? 0u : 1u));
      if (!same) CHECK(t.records[0].offset == c.dst_pos() + c.len);
    }
    reset();
    copy_case(dst, src, c, 0, -1);  // one byte too few
    {
      const HostlinkSlotTally t = compare(0, 8);
      const bool same = src[c.src_pos() + c.len - 1] ==
                        hostlink_slot_byte(bg_seed, c.index, c.dst_pos() + c.len - 1);
      CHECK(t.errors == (same ? 0u : 1u));
      if (!same) CHECK(t.records[0].offset == c.dst_pos() + c.len - 1);
    }
  }
  // over every case, a too-long and a too-short copy are caught wherever the
  // byte at stake differs between source and background: that must be nearly
  // always (a hash byte agrees by chance once in 256)
  int blind = 0;
  for (const HostlinkCase& c : plan.cases) {
    blind += hostlink_slot_byte(src_seed, c.index, c.src_pos() + c.len) ==
             hostlink_slot_byte(bg_seed, c.index, c.dst_pos() + c.len);
    blind += hostlink_slot_byte(src_seed, c.index, c.src_pos() + c.len - 1) ==
             hostlink_slot_byte(bg_seed, c.index, c.dst_pos() + c.len - 1);
  }
  CHECK(blind <= 16);
}

void test_atomics() {
  const uint64_t seed = 0xDEADBEEFCAFEF00Dull;
  const uint64_t threads = 256, host_adds = 128;
  const int reps = 3;
  const HostlinkAtomExpected e = hostlink_atom_expected(seed, threads, reps, host_adds);
  CHECK(e.add32.size() == 64 && e.add64.size() == 64);
  // brute force, per cell
  for (int c = 0; c < 64; ++c) {
    uint32_t s32 = 0;
    uint64_t s64 = 0;
    for (uint64_t id = 0; id < threads; ++id)
      for (int r = 0; r < reps; ++r)
        if ((int)((id + r) % 64) == c) {
          s32 += hostlink_atom_vals(seed, id, r).add32;
          s64 += hostlink_atom_vals(seed, id, r).add64;
        }
    CHECK(e.device32[c] == s32 && e.device64[c] == s64);
    for (uint64_t j = 0; j < host_adds; ++j)
      if ((int)(j % 64) == c) {
        s32 += hostlink_atom_vals(seed, kHostlinkHostId + j, 0).add32;
        s64 += hostlink_atom_vals(seed, kHostlinkHostId + j, 0).add64;
      }
    CHECK(e.add32[c] == s32 && e.add64[c] == s64);
  }
  // the operand is the hash of the pinned kind's atomics seed
  const HostlinkAtomVals v = hostlink_atom_vals(seed, 5, 2);
  CHECK(v.add32 == (uint32_t)hbm_pattern_value(kHbmPatternHash, seed + 6, 2 * 82));
  CHECK(v.add64 == hbm_pattern_value(kHbmPatternHash, seed + 6, 2 * 82 + 1));
  CHECK(hostlink_atom_items(256) == 128 + 2 + 256 + 320 + 16 + 2);
}

void test_validation() {
  HostlinkShape ok{1 << 20, {0, 1, 2}, 0, 0, 2, 4096, 64, 0, -1, -1, -1, 1};
  hostlink_validate(ok);
  const auto bad = [&](auto&& change) {
    HostlinkShape s = ok;
    change(s);
    return throws_invalid([&] { hostlink_validate(s); });
  };
  CHECK(bad([](HostlinkShape& s) { s.nbytes = 4100; }));
  CHECK(bad([](HostlinkShape& s) { s.nbytes = 4088; }));
  CHECK(bad([](HostlinkShape& s) { s.nbytes = (1ull << 30) + 8; }));
  CHECK(bad([](HostlinkShape& s) { s.kinds.clear(); }));
  CHECK(bad([](HostlinkShape& s) { s.blocks = -1; }));
  CHECK(bad([](HostlinkShape& s) { s.atomics_blocks = -1; }));
  CHECK(bad([](HostlinkShape& s) { s.reps = 0; }));
  CHECK(bad([](HostlinkShape& s) { s.reps = 17; }));
  CHECK(bad([](HostlinkShape& s) { s.host_adds = 65; }));
  CHECK(bad([](HostlinkShape& s) { s.max_records = -1; }));
  CHECK(bad([](HostlinkShape& s) { s.max_records = 4097; }));
  CHECK(bad([](HostlinkShape& s) { s.poison_mask = 1u << 7; }));
  CHECK(bad([](HostlinkShape& s) { s.poison_kind = 3; }));
  CHECK(bad([](HostlinkShape& s) { s.poison_word = 1 << 17; }));
  CHECK(bad([](HostlinkShape& s) { s.poison_case = 464; }));
  CHECK(bad([](HostlinkShape& s) { s.poison_mask = 1; }));  // no poison_word
  CHECK(bad([](HostlinkShape& s) { s.poison_mask = 32; }));  // no poison_case
  CHECK(bad([](HostlinkShape& s) {
    s.poison_mask = 32;
    s.poison_case = 0;
    s.poison_xor = 256;
  }));
  CHECK(!bad([](HostlinkShape& s) { s.nbytes = 4096; }));
  CHECK(!bad([](HostlinkShape& s) {
    s.poison_mask = 0x7F;
    s.poison_word = 0;
    s.poison_case = 463;
  }));
  CHECK(throws_invalid([] { hostlink_kind_list({}); }));
  CHECK(throws_invalid([] { hostlink_kind_list({"pinned", "pinned"}); }));
  CHECK(throws_invalid([] { hostlink_kind_list({"mapped"}); }));
  CHECK(hostlink_kind_list({"pageable", "pinned"}) == (std::vector<int>{2, 0}));
}

}  // namespace

int main() {
  test_seed_rule_and_fill();
  test_plan();
  test_slot_compare();
  test_atomics();
  test_validation();
  if (g_failures) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("%d checks passed\n", g_checks);
  return 0;
}
