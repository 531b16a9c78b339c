// lds_problems_selftest.cpp — stand-alone checks of the generators of the LDS
// data-integrity check (native/lds_problems.hpp).
//
// Built with -fsanitize=address,undefined by tests/test_lds_problems_native.py
// and run as a child process, so the index arithmetic of the generators runs
// under the sanitizers.  Beyond that it asserts only what can be stated
// without the code under test: every address is inside the 160 KiB array and
// aligned as its instruction needs, every layout covers every byte exactly
// once, every permutation is one, the per-cell totals equal a brute-force sum
// over all threads, and published splitmix64 values.

#include <cstdint>
#include <cstdio>
#include <set>
#include <stdexcept>
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

const uint64_t kSeeds[] = {0ull, 1ull, 0xDEADBEEFCAFEF00Dull, ~0ull};

void test_constants_and_index() {
  CHECK(kLdsWords == 40960 && kLdsBytes == 163840);
  CHECK(kLdsChunks * kLdsChunkWords == kLdsWords);
  CHECK(kLdsChunks % 4 == 0);
  CHECK(kLdsTrBlocks == 1280 && kLdsTrBlocks % 16 == 0);
  // splitmix64 of state 0 after one step (published first output for seed 0)
  CHECK(hbm_pattern_value(kHbmPatternHash, 1, 0) == 0xE220A8397B1DCDAFull);
  // the fields of an index do not overlap at their largest values
  std::set<uint64_t> seen;
  const uint32_t blocks[] = {0, 1, kLdsMaxBlocks - 1};
  const uint32_t reps[] = {0, 1, kLdsMaxReps - 1};
  const uint32_t subs[] = {0, 1, kLdsMaxPasses, 31};
  const uint32_t words[] = {0, 1, kLdsWords - 1, 65535};
  for (uint32_t b : blocks)
    for (uint32_t r : reps)
      for (uint32_t s : subs)
        for (uint32_t w : words) CHECK(seen.insert(lds_index(b, r, s, w)).second);
}

void test_pattern() {
  for (uint64_t seed : kSeeds)
    for (int passes : {1, 3, kLdsMaxPasses}) {
      // checker by word parity, whatever the seed
      CHECK(lds_pattern_word(seed, passes, 3, 2, passes, 0) == 0xAAAAAAAAu);
      CHECK(lds_pattern_word(seed, passes, 3, 2, passes, 40959) == 0x55555555u);
      const std::vector<uint32_t> a = lds_pattern_image(seed, passes, 0, 0, 0);
      const std::vector<uint32_t> b = lds_pattern_image(seed, passes, 1, 0, 0);
      CHECK(a.size() == (size_t)kLdsWords && a != b);
      // every data bit takes both values somewhere in a hash image
      uint32_t ones = 0, zeros = 0;
      for (uint32_t v : a) {
        ones |= v;
        zeros |= ~v;
      }
      CHECK(ones == ~0u && zeros == ~0u);
    }
  // three different widths per pattern; over three patterns every width in
  // every role
  for (int pat = 0; pat <= kLdsMaxPasses; ++pat) {
    std::set<int> w;
    for (int step = 0; step < 3; ++step) {
      const int width = lds_pattern_width(pat, step);
      CHECK(width >= 0 && width < 3);
      w.insert(width);
    }
    CHECK(w.size() == 3);
  }
  for (int step = 0; step < 3; ++step) {
    std::set<int> w;
    for (int pat = 0; pat < 3; ++pat) w.insert(lds_pattern_width(pat, step));
    CHECK(w.size() == 3);
  }
}

void test_subword() {
  int bytes = 0;
  for (uint32_t w = 0; w < (uint32_t)kLdsWords; ++w) bytes += lds_subword_bytes(w);
  CHECK(bytes == kLdsWords / 2);
  for (int bank = 0; bank < 64; ++bank) {  // every bank sees both kinds
    CHECK(lds_subword_bytes((uint32_t)bank));
    CHECK(!lds_subword_bytes((uint32_t)bank + 256u));
  }
}

void test_transpose() {
  for (int layout = 0; layout < 2; ++layout) {
    const int R = kLdsTrRowBlocks[layout];
    CHECK((32 * R) % 8 == 0);  // the row stride is a multiple of 8 bytes
    std::vector<int> cover(kLdsBytes, 0), recv(kLdsBytes / 2, 0);
    for (uint32_t b = 0; b < (uint32_t)kLdsTrBlocks; ++b)
      for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t off = lds_tr_lane_offset(R, b, i);
        CHECK(off % 8 == 0 && off + 8 <= (uint32_t)kLdsBytes);
        if (off + 8 <= (uint32_t)kLdsBytes)
          for (int k = 0; k < 8; ++k) ++cover[off + k];
        // lane 4q+p addresses row q, columns 4p .. 4p+3
        CHECK(off == lds_tr_row_offset(R, b, i >> 2) + 8 * (i & 3));
        for (uint32_t q = 0; q < 4; ++q) {
          const uint32_t e = lds_tr_expected_elem(R, b, i, q);
          CHECK(e < (uint32_t)kLdsBytes / 2);
          if (e < (uint32_t)kLdsBytes / 2) ++recv[e];
          // row q of the block, column i
          CHECK(2 * e == lds_tr_row_offset(R, b, q) + 2 * i);
        }
      }
    bool once = true;
    for (int c : cover) once = once && c == 1;
    for (int c : recv) once = once && c == 1;
    CHECK(once);  // every byte addressed once, every element received once
    // rows of a block are one stride apart
    CHECK(lds_tr_row_offset(R, 7, 1) - lds_tr_row_offset(R, 7, 0) == 32u * R);
  }
  CHECK(lds_tr_lane_offset(5, kLdsTrBlocks - 1, 15) + 8 == (uint32_t)kLdsBytes);
  for (uint64_t seed : kSeeds) {
    const uint32_t w = lds_tr_word(seed, 2, 1, 77);
    CHECK(lds_tr_elem(seed, 2, 1, 154) == (w & 0xFFFFu));
    CHECK(lds_tr_elem(seed, 2, 1, 155) == (w >> 16));
  }
}

void test_dma() {
  const uint32_t blocks[] = {0, 1, 2, 511, kLdsMaxBlocks - 1};
  const uint32_t reps[] = {0, 1, 2, kLdsMaxReps - 1};
  for (uint32_t b : blocks)
    for (uint32_t r : reps) {
      std::vector<int> used(kLdsWords, 0);
      bool identity = true, ok = true;
      for (uint32_t w = 0; w < (uint32_t)kLdsWords; ++w) {
        const uint32_t s = lds_dma_src_index(b, r, w);
        ok = ok && s < (uint32_t)kLdsWords;
        if (s < (uint32_t)kLdsWords) ++used[s];
        identity = identity && s == w;
        if (lds_dma_wide(r, w / kLdsChunkWords)) {
          // a 16-byte piece: aligned source, four words kept together
          ok = ok && (s & 3u) == (w & 3u);
          ok = ok && s - (s & 3u) == lds_dma_src_index(b, r, w - (w & 3u));
        }
      }
      CHECK(ok);
      CHECK(!identity);
      bool once = true;
      for (int c : used) once = once && c == 1;
      CHECK(once);  // a permutation of the source buffer
      const std::vector<uint32_t> img = lds_dma_image(1, b, r);
      CHECK(img.size() == (size_t)kLdsWords);
    }
  // differs per workgroup and per repetition
  CHECK(lds_dma_src_index(0, 0, 5) != lds_dma_src_index(1, 0, 5));
  CHECK(lds_dma_src_index(0, 0, 5) != lds_dma_src_index(0, 1, 5));
  int wide = 0;
  for (uint32_t c = 0; c < (uint32_t)kLdsChunks; ++c) {
    wide += lds_dma_wide(0, c);
    CHECK(lds_dma_wide(0, c) != lds_dma_wide(1, c));
  }
  CHECK(wide == kLdsChunks / 2);
}

void test_atomics() {
  // cells: inside the array, 8-byte aligned, not overlapping
  std::set<uint32_t> words;
  for (uint32_t c = 0; c < (uint32_t)kLdsAtomCells; ++c) {
    const uint32_t base = lds_atom_cell_base(c);
    CHECK(base % 2 == 0 && (base + kLdsCellAdd64) % 2 == 0);
    CHECK(base + kLdsCellConfirm < (uint32_t)kLdsWords);
    for (int f = 0; f <= kLdsCellConfirm; ++f) CHECK(words.insert(base + f).second);
  }
  CHECK(lds_atom_cell_base(kLdsAtomCells - 1) > 3u * kLdsWords / 4);  // the top too
  for (uint64_t seed : kSeeds) {
    const uint32_t block = 17, rep = 3;
    // brute force over every thread and step
    std::vector<LdsAtomCell> want(kLdsAtomCells,
                                  LdsAtomCell{0ull, 0u, 0u, ~0u, 0u, 0u, ~0u, 0, 0});
    for (uint32_t tid = 0; tid < (uint32_t)kLdsBlock; ++tid)
      for (uint32_t step = 0; step < (uint32_t)kLdsAtomSteps; ++step) {
        const LdsAtomVals v = lds_atom_vals(seed, block, rep, tid, step);
        CHECK(v.addf >= -8 && v.addf <= 8);
        LdsAtomCell& e = want[(tid + step) % kLdsAtomCells];
        e.add32 += v.add32;
        e.add64 += v.add64;
        e.addf += v.addf;
        e.addf_abs += v.addf < 0 ? -v.addf : v.addf;
        e.max32 = std::max(e.max32, v.mm);
        e.min32 = std::min(e.min32, v.mm);
        e.x ^= v.x;
        e.o |= v.o;
        e.a &= v.a;
      }
    const LdsAtomExpected got = lds_atom_expected(seed, block, rep);
    for (int c = 0; c < kLdsAtomCells; ++c) {
      CHECK(got.add32[c] == want[c].add32 && got.add64[c] == want[c].add64);
      CHECK(got.addf[c] == want[c].addf && got.addf_abs[c] == want[c].addf_abs);
      CHECK(got.max32[c] == want[c].max32 && got.min32[c] == want[c].min32);
      CHECK(got.x[c] == want[c].x && got.o[c] == want[c].o && got.a[c] == want[c].a);
      CHECK(got.addf_abs[c] <= kLdsF32Bound);  // every f32 sum order is exact
    }
  }
}

void test_permute() {
  for (uint64_t seed : kSeeds)
    for (uint32_t step = 0; step < (uint32_t)kLdsPermSteps; ++step)
      for (uint32_t wave = 0; wave < 4; ++wave) {
        const uint32_t map = lds_perm_map(seed, 9, 1, step, wave);
        CHECK((map & 1u) == 1u && (map & 63u) == (map & 0xFFu) && (map >> 8) < 64);
        std::set<uint32_t> image;
        for (uint32_t l = 0; l < 64; ++l) {
          const uint32_t to = lds_perm_sigma(map, l);
          CHECK(to < 64);
          image.insert(to);
          CHECK(lds_perm_sigma_inv(map, to) == l);
        }
        CHECK(image.size() == 64);
      }
  // every odd multiplier has its inverse
  for (uint32_t m = 1; m < 64; m += 2)
    for (uint32_t add : {0u, 5u, 63u})
      for (uint32_t l = 0; l < 64; ++l)
        CHECK(lds_perm_sigma_inv(m | add << 8, lds_perm_sigma(m | add << 8, l)) == l);
  CHECK(lds_perm_map(1, 0, 0, 0, 0) != lds_perm_map(1, 0, 0, 1, 0));
}

void test_counts_and_validation() {
  CHECK(lds_phase_items(kLdsPhasePattern, 3) == 8ull * kLdsWords);
  CHECK(lds_phase_items(kLdsPhaseSubword, 3) == 163840ull);
  CHECK(lds_phase_items(kLdsPhaseTranspose, 3) == 2ull * 81920);
  CHECK(lds_phase_items(kLdsPhaseDma, 3) == 40960ull);
  CHECK(lds_phase_items(kLdsPhaseAtomics, 3) == 640ull);
  CHECK(lds_phase_items(kLdsPhasePermute, 3) == 4096ull);
  CHECK(throws_invalid([] { lds_phase_items(6, 1); }));

  std::vector<int64_t> offs(64);
  for (int l = 0; l < 64; ++l) offs[l] = 8 * l;
  lds_tr_tile_validate(256, offs);  // exactly fits: 64 x 8 = 512 bytes
  lds_tr_tile_validate(81920, offs);
  CHECK(throws_invalid([&] { lds_tr_tile_validate(255, offs); }));
  CHECK(throws_invalid([&] { lds_tr_tile_validate(81921, offs); }));
  CHECK(throws_invalid([&] { lds_tr_tile_validate(2, offs); }));
  std::vector<int64_t> bad = offs;
  bad[5] = 44;
  CHECK(throws_invalid([&] { lds_tr_tile_validate(256, bad); }));
  bad = offs;
  bad[0] = -8;
  CHECK(throws_invalid([&] { lds_tr_tile_validate(256, bad); }));
  bad = offs;
  bad[63] = 163840;
  CHECK(throws_invalid([&] { lds_tr_tile_validate(81920, bad); }));
  bad = offs;
  bad[63] = (int64_t)1 << 40;
  CHECK(throws_invalid([&] { lds_tr_tile_validate(81920, bad); }));
  bad.pop_back();
  CHECK(throws_invalid([&] { lds_tr_tile_validate(256, bad); }));
}

}  // namespace

int main() {
  test_constants_and_index();
  test_pattern();
  test_subword();
  test_transpose();
  test_dma();
  test_atomics();
  test_permute();
  test_counts_and_validation();
  if (g_failures) {
    std::fprintf(stderr, "%d of %d checks FAILED\n", g_failures, g_checks);
    return 1;
  }
  std::printf("%d checks passed\n", g_checks);
  return 0;
}
