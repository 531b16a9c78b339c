// hostlink_problems.hpp — the exact problems of the host-link data-integrity
// check (host_link_check in gpu_validator.hip): what every word of a host or
// device buffer must hold after each phase, the plan of unaligned copies with
// the expected image of every destination slot, and the operands and totals of
// the system-scope atomics.
//
// Included from validator_problems.hpp (it needs hbm_pattern_value and
// VALIDATOR_HD); plain C++17 like the rest of it, so
// tests/native/hostlink_problems_selftest.cpp drives it stand-alone under
// AddressSanitizer + UBSan.  The host loops are single-threaded on purpose:
// the check measures a link, not the host's memory bandwidth.
//
// Seed rule: phase p of memory kind k uses the hash pattern with seed
// `seed + 16 * k + p`, so any expected word is
// hbm_pattern_value(kHbmPatternHash, seed + 16 * k + p, word).  Inverses are
// computed from the pattern, never from data read.

#pragma once

constexpr int kHostlinkKinds = 3;
constexpr int kHostlinkPinned = 0, kHostlinkRegistered = 1, kHostlinkPageable = 2;
static const char* const kHostlinkKindNames[kHostlinkKinds] = {
    "pinned", "registered", "pageable"};

constexpr int kHostlinkPhases = 7;
constexpr int kHostlinkH2d = 0, kHostlinkD2h = 1, kHostlinkZcRead = 2,
              kHostlinkZcWrite = 3, kHostlinkDuplex = 4, kHostlinkUnaligned = 5,
              kHostlinkAtomics = 6;
static const char* const kHostlinkPhaseNames[kHostlinkPhases] = {
    "h2d", "d2h", "zc_read", "zc_write", "duplex", "unaligned", "atomics"};
// seed slot of the background a destination slot holds before an unaligned copy
constexpr int kHostlinkBackground = 8;

constexpr uint64_t kHostlinkMinBytes = 4096, kHostlinkMaxBytes = 1ull << 30;
constexpr int kHostlinkMaxReps = 16;
constexpr int kHostlinkMaxRecords = 4096;
constexpr int kHostlinkMaxBlocks = 1 << 16;
constexpr int kHostlinkMaxAtomBlocks = 4096;
constexpr int kHostlinkMaxHostAdds = 1 << 20;

VALIDATOR_HD inline uint64_t hostlink_seed(uint64_t seed, int kind, int phase) {
  return seed + 16ull * (uint64_t)kind + (uint64_t)phase;
}

// Which pattern the words compared in a phase belong to, and whether they are
// its inverse: d2h brings back what the h2d kernel inverted, zc_write stores
// the inverse of what zc_read compared.
VALIDATOR_HD inline int hostlink_data_phase(int phase) {
  return phase == kHostlinkD2h ? kHostlinkH2d
         : phase == kHostlinkZcWrite ? kHostlinkZcRead : phase;
}
VALIDATOR_HD inline bool hostlink_data_inverted(int phase) {
  return phase == kHostlinkD2h || phase == kHostlinkZcWrite;
}

inline int hostlink_kind_index(const std::string& name) {
  for (int k = 0; k < kHostlinkKinds; ++k)
    if (name == kHostlinkKindNames[k]) return k;
  throw std::invalid_argument(
      "host_link_check: kinds are 'pinned', 'registered' and 'pageable', not '" +
      name + "'");
}

// phases a kind runs, as a bit mask: pageable memory has no device pointer
inline unsigned hostlink_kind_phases(int kind) {
  if (kind == kHostlinkPageable)
    return 1u << kHostlinkH2d | 1u << kHostlinkD2h | 1u << kHostlinkUnaligned;
  if (kind == kHostlinkRegistered) return 0x3Fu;
  return 0x7Fu;
}

// ---------------------------------------------------------------------------
// Word buffers: fill and exact verify
// ---------------------------------------------------------------------------

// dst[k] = pattern(pseed, first_word + k), inverted or not
inline void hostlink_fill(uint64_t* dst, uint64_t first_word, uint64_t n,
                          uint64_t pseed, bool inverted) {
  const uint64_t inv = inverted ? ~0ull : 0ull;
  for (uint64_t k = 0; k < n; ++k)
    dst[k] = hbm_pattern_value(kHbmPatternHash, pseed, first_word + k) ^ inv;
}

struct HostlinkWordRecord {
  uint64_t word, expected, got;
};

// what one comparison pass found; `cap` records are kept, the rest counted
struct HostlinkTally {
  uint64_t compared = 0, errors = 0, xor_or = 0, dropped = 0;
  std::vector<HostlinkWordRecord> records;
};

// Compare src[k] with the pattern word first_word + k.  The poison hook is
// data only: poison_xor goes into the expected value of word poison_word
// (-1: off) and never into memory, so `got` is what the buffer holds.
inline void hostlink_verify(const uint64_t* src, uint64_t first_word, uint64_t n,
                            uint64_t pseed, bool inverted, int64_t poison_word,
                            uint64_t poison_xor, size_t cap, HostlinkTally& t) {
  const uint64_t inv = inverted ? ~0ull : 0ull;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t w = first_word + k;
    uint64_t expected = hbm_pattern_value(kHbmPatternHash, pseed, w) ^ inv;
    if (poison_word >= 0 && w == (uint64_t)poison_word) expected ^= poison_xor;
    const uint64_t got = src[k];
    ++t.compared;
    if (got == expected) continue;
    ++t.errors;
    t.xor_or |= got ^ expected;
    if (t.records.size() < cap)
      t.records.push_back({w, expected, got});
    else
      ++t.dropped;
  }
}

// ---------------------------------------------------------------------------
// The unaligned copy plan.  A case copies `len` bytes from byte
// guard + src_off of the source slot to byte guard + dst_off of the
// destination slot.  Every slot has the same size: a 4 KiB multiple that holds
// the guard, the largest payload at the largest offset, and 64 free bytes
// behind it.  The source slot of case c holds the bytes (little-endian) of the
// hash words c * slot_words + j of the phase's seed, the destination slot the
// same words of the background seed; after the copy the whole destination slot
// is compared, so one byte too many, too few or one byte off is a mismatch.
// ---------------------------------------------------------------------------

constexpr int kHostlinkLengths = 29, kHostlinkOffsets = 8;
constexpr int kHostlinkLength[kHostlinkLengths] = {
    1,   2,   3,   4,   5,   7,    8,    9,    15,    16,    17,   31, 32, 33, 63,
    64,  65,  127, 128, 129, 255,  256,  257,  4095,  4096,  4097,
    65535, 65536, 65537};
constexpr int kHostlinkOffset[kHostlinkOffsets][2] = {  // {src_off, dst_off}
    {0, 0}, {1, 0}, {0, 1}, {3, 3}, {1, 2}, {2, 3}, {63, 65}, {129, 7}};
constexpr int kHostlinkCasesPerDirection = kHostlinkLengths * kHostlinkOffsets;
constexpr int kHostlinkCases = 2 * kHostlinkCasesPerDirection;  // 464
constexpr size_t kHostlinkGuard = 128;
constexpr size_t kHostlinkTailGuard = 64;
constexpr size_t kHostlinkSlotBytes =
    (kHostlinkGuard + 65537 + 129 + kHostlinkTailGuard + 4095) / 4096 * 4096;
constexpr size_t kHostlinkSlotWords = kHostlinkSlotBytes / 8;
static const char* const kHostlinkDirectionNames[2] = {"h2d", "d2h"};

struct HostlinkCase {
  int index, direction;  // 0: host to device, 1: device to host
  size_t len, src_off, dst_off;
  size_t src_pos() const { return kHostlinkGuard + src_off; }  // in the slot
  size_t dst_pos() const { return kHostlinkGuard + dst_off; }
};

struct HostlinkPlan {
  size_t slot_bytes = kHostlinkSlotBytes, guard = kHostlinkGuard;
  std::vector<HostlinkCase> cases;
};

inline HostlinkPlan hostlink_plan() {
  HostlinkPlan p;
  p.cases.reserve(kHostlinkCases);
  for (int d = 0; d < 2; ++d)
    for (int l = 0; l < kHostlinkLengths; ++l)
      for (int o = 0; o < kHostlinkOffsets; ++o)
        p.cases.push_back({(int)p.cases.size(), d, (size_t)kHostlinkLength[l],
                           (size_t)kHostlinkOffset[o][0],
                           (size_t)kHostlinkOffset[o][1]});
  return p;
}

// byte j of the slot image of case c under pseed
inline uint8_t hostlink_slot_byte(uint64_t pseed, int c, size_t j) {
  const uint64_t w = hbm_pattern_value(
      kHbmPatternHash, pseed, (uint64_t)c * kHostlinkSlotWords + j / 8);
  return (uint8_t)(w >> (8 * (j % 8)));
}

// the whole slot image of case c under pseed
inline void hostlink_slot_fill(uint8_t* slot, uint64_t pseed, int c) {
  for (size_t w = 0; w < kHostlinkSlotWords; ++w) {
    const uint64_t v = hbm_pattern_value(kHbmPatternHash, pseed,
                                         (uint64_t)c * kHostlinkSlotWords + w);
    for (int b = 0; b < 8; ++b) slot[8 * w + b] = (uint8_t)(v >> (8 * b));
  }
}

// what the destination slot of `c` must hold after the copy
inline std::vector<uint8_t> hostlink_slot_expected(const HostlinkCase& c,
                                                   uint64_t src_seed,
                                                   uint64_t bg_seed) {
  std::vector<uint8_t> e(kHostlinkSlotBytes);
  hostlink_slot_fill(e.data(), bg_seed, c.index);
  for (size_t j = 0; j < c.len; ++j)
    e[c.dst_pos() + j] = hostlink_slot_byte(src_seed, c.index, c.src_pos() + j);
  return e;
}

struct HostlinkByteRecord {
  int case_index;
  size_t offset;  // in the destination slot
  uint8_t expected, got;
};

struct HostlinkSlotTally {
  uint64_t compared = 0, errors = 0, xor_or = 0, dropped = 0;
  std::vector<HostlinkByteRecord> records;
};

// Compare a whole destination slot.  poison (0: off) goes into the expected
// value of the first payload byte, never into memory.
inline void hostlink_slot_compare(const uint8_t* dst, const HostlinkCase& c,
                                  uint64_t src_seed, uint64_t bg_seed,
                                  uint8_t poison, size_t cap,
                                  HostlinkSlotTally& t) {
  std::vector<uint8_t> e = hostlink_slot_expected(c, src_seed, bg_seed);
  e[c.dst_pos()] ^= poison;
  for (size_t j = 0; j < kHostlinkSlotBytes; ++j) {
    ++t.compared;
    if (dst[j] == e[j]) continue;
    ++t.errors;
    t.xor_or |= (uint64_t)(uint8_t)(dst[j] ^ e[j]) << (8 * (j % 8));
    if (t.records.size() < cap)
      t.records.push_back({c.index, j, e[j], dst[j]});
    else
      ++t.dropped;
  }
}

// ---------------------------------------------------------------------------
// System-scope atomics on pinned host memory: fetch-add, swap and
// compare-and-swap only (the three PCIe AtomicOps), 32 and 64 bit, integers
// modulo 2^32 and 2^64.
// ---------------------------------------------------------------------------

constexpr int kHostlinkAtomCells = 64;   // one 128-byte line each
constexpr int kHostlinkAtomBlock = 64;   // one wave: its lanes hit 64 lines
constexpr int kHostlinkClaimCells = 8;
constexpr uint64_t kHostlinkHostId = 1ull << 40;  // ids of the host's own adds

struct HostlinkAtomVals {
  uint32_t add32;
  uint64_t add64;
};

// what thread `id` adds in repetition `r` (r < 16); host add j is thread
// kHostlinkHostId + j, repetition 0
VALIDATOR_HD inline HostlinkAtomVals hostlink_atom_vals(uint64_t seed, uint64_t id,
                                                        uint32_t r) {
  const uint64_t s = hostlink_seed(seed, kHostlinkPinned, kHostlinkAtomics);
  const uint64_t n = id * 16 + r;
  HostlinkAtomVals v;
  v.add32 = (uint32_t)hbm_pattern_value(kHbmPatternHash, s, 2 * n);
  v.add64 = hbm_pattern_value(kHbmPatternHash, s, 2 * n + 1);
  return v;
}

struct HostlinkAtomExpected {
  std::vector<uint32_t> add32, device32, host32;
  std::vector<uint64_t> add64, device64, host64;
};

// cells after `threads` device threads ran `reps` repetitions and the host
// made `host_adds` adds: thread id hits cell (id + r) % 64, host add j cell
// j % 64
inline HostlinkAtomExpected hostlink_atom_expected(uint64_t seed, uint64_t threads,
                                                   int reps, uint64_t host_adds) {
  HostlinkAtomExpected e;
  e.device32.assign(kHostlinkAtomCells, 0u);
  e.host32.assign(kHostlinkAtomCells, 0u);
  e.device64.assign(kHostlinkAtomCells, 0ull);
  e.host64.assign(kHostlinkAtomCells, 0ull);
  for (uint64_t id = 0; id < threads; ++id)
    for (int r = 0; r < reps; ++r) {
      const size_t c = (size_t)((id + (uint64_t)r) % kHostlinkAtomCells);
      const HostlinkAtomVals v = hostlink_atom_vals(seed, id, (uint32_t)r);
      e.device32[c] += v.add32;
      e.device64[c] += v.add64;
    }
  for (uint64_t j = 0; j < host_adds; ++j) {
    const size_t c = (size_t)(j % kHostlinkAtomCells);
    const HostlinkAtomVals v = hostlink_atom_vals(seed, kHostlinkHostId + j, 0);
    e.host32[c] += v.add32;
    e.host64[c] += v.add64;
  }
  e.add32.resize(kHostlinkAtomCells);
  e.add64.resize(kHostlinkAtomCells);
  for (int c = 0; c < kHostlinkAtomCells; ++c) {
    e.add32[c] = e.device32[c] + e.host32[c];
    e.add64[c] = e.device64[c] + e.host64[c];
  }
  return e;
}

// items the host compares in the atomics phase: 2 x 64 add cells, the ticket
// counter, the out-of-range ticket count, `threads` seen slots, the
// threads + 64 values of the swap multiset, 8 claim/confirm pairs and one
// winner count per width
inline uint64_t hostlink_atom_items(uint64_t threads) {
  return 2ull * kHostlinkAtomCells + 2 + threads + (threads + kHostlinkAtomCells) +
         2ull * kHostlinkClaimCells + 2;
}

// ---------------------------------------------------------------------------
// Argument rules of host_link_check, checked before the first HIP call
// ---------------------------------------------------------------------------

struct HostlinkShape {
  uint64_t nbytes;
  std::vector<int> kinds;
  int blocks, atomics_blocks, reps;
  int64_t host_adds;
  int max_records;
  unsigned poison_mask;
  int poison_kind;
  int64_t poison_word, poison_case;
  uint64_t poison_xor;
};

inline std::vector<int> hostlink_kind_list(const std::vector<std::string>& names) {
  if (names.empty())
    throw std::invalid_argument("host_link_check: kinds must not be empty");
  std::vector<int> kinds;
  for (const std::string& n : names) {
    const int k = hostlink_kind_index(n);
    if (std::find(kinds.begin(), kinds.end(), k) != kinds.end())
      throw std::invalid_argument("host_link_check: kind '" + n + "' given twice");
    kinds.push_back(k);
  }
  return kinds;
}

inline void hostlink_validate(const HostlinkShape& s) {
  const std::string who = "host_link_check: ";
  if (s.nbytes % 8 != 0 || s.nbytes < kHostlinkMinBytes ||
      s.nbytes > kHostlinkMaxBytes)
    throw std::invalid_argument(
        who + "nbytes must be a multiple of 8 in [4 KiB, 1 GiB]");
  if (s.kinds.empty()) throw std::invalid_argument(who + "kinds must not be empty");
  if (s.blocks < 0 || s.blocks > kHostlinkMaxBlocks)
    throw std::invalid_argument(who + "blocks must be in [0, 65536]");
  if (s.atomics_blocks < 0 || s.atomics_blocks > kHostlinkMaxAtomBlocks)
    throw std::invalid_argument(who + "atomics_blocks must be in [0, 4096]");
  if (s.reps < 1 || s.reps > kHostlinkMaxReps)
    throw std::invalid_argument(who + "reps must be in [1, 16]");
  if (s.host_adds < 0 || s.host_adds > kHostlinkMaxHostAdds ||
      s.host_adds % kHostlinkAtomCells != 0)
    throw std::invalid_argument(
        who + "host_adds must be a multiple of 64 in [0, 2^20]");
  if (s.max_records < 0 || s.max_records > kHostlinkMaxRecords)
    throw std::invalid_argument(who + "max_records must be in [0, 4096]");
  if (s.poison_mask >> kHostlinkPhases)
    throw std::invalid_argument(who + "poison_mask has one bit per phase: 7 bits");
  if (s.poison_kind < -1 || s.poison_kind >= kHostlinkKinds)
    throw std::invalid_argument(who + "poison_kind is -1 or a kind index below 3");
  if (s.poison_word < -1 || s.poison_word >= (int64_t)(s.nbytes / 8))
    throw std::invalid_argument(who + "poison_word is -1 or a word of the buffer");
  if (s.poison_case < -1 || s.poison_case >= kHostlinkCases)
    throw std::invalid_argument(who + "poison_case is -1 or a plan case below 464");
  if ((s.poison_mask & 0x1Fu) && s.poison_word < 0)
    throw std::invalid_argument(who + "poison bits 0 to 4 need a poison_word");
  if ((s.poison_mask & 1u << kHostlinkUnaligned) && s.poison_case < 0)
    throw std::invalid_argument(who + "poison bit 5 needs a poison_case");
  if (s.poison_mask && s.poison_xor == 0)
    throw std::invalid_argument(who + "poison_xor must be non-zero");
  // the unaligned phase compares bytes, the add_u32 cell 32 bits
  if ((s.poison_mask & 1u << kHostlinkUnaligned) && (uint8_t)s.poison_xor == 0)
    throw std::invalid_argument(who + "poison bit 5 uses the low byte of poison_xor");
  if ((s.poison_mask & 1u << kHostlinkAtomics) && (uint32_t)s.poison_xor == 0)
    throw std::invalid_argument(
        who + "poison bit 6 uses the low 32 bits of poison_xor");
}
