// lds_problems.hpp — the exact problems of the LDS data-integrity check
// (lds_integrity_kernel in gpu_validator.hip): what every one of the 40960
// words of a CU's Local Data Share must hold after each step of the six
// phases, and what the LDS atomic ALU and the permute crossbar must return.
//
// Included from validator_problems.hpp (it needs hbm_pattern_value and
// VALIDATOR_HD); plain C++17 like the rest of it, so
// tests/native/lds_problems_selftest.cpp drives it stand-alone under
// AddressSanitizer + UBSan.  Every value is a pure function of (seed, phase
// key, workgroup, repetition, sub-step, word index): the kernel, the host
// reference and the tests' numpy all derive it from the same definition.

#pragma once

constexpr int kLdsWords = 40960;             // 160 KiB, all of a CU's LDS
constexpr int kLdsBytes = kLdsWords * 4;
constexpr int kLdsBlock = 256;               // four waves, one per SIMD
constexpr int kLdsChunkWords = 256;          // 1 KiB: one dwordx4 wave-instruction
constexpr int kLdsChunks = kLdsWords / kLdsChunkWords;  // 160
constexpr int kLdsPhases = 6;
constexpr int kLdsPhasePattern = 0, kLdsPhaseSubword = 1, kLdsPhaseTranspose = 2,
              kLdsPhaseDma = 3, kLdsPhaseAtomics = 4, kLdsPhasePermute = 5;
static const char* const kLdsPhaseNames[kLdsPhases] = {
    "pattern", "subword", "transpose", "dma", "atomics", "permute"};
constexpr int kLdsMaxPasses = 16;
constexpr int kLdsMaxReps = 4096;
constexpr int kLdsMaxBlocks = 1 << 16;
constexpr int kLdsMaxRecords = 64;

constexpr uint64_t kLdsKeyPattern = 0x4C44535F50415454ull,  // "LDS_PATT"
                   kLdsKeySubword = 0x4C44535F53554257ull,
                   kLdsKeyTranspose = 0x4C44535F54523136ull,
                   kLdsKeyDma = 0x4C44535F444D4153ull,
                   kLdsKeyAtom1 = 0x4C44535F41544D31ull,
                   kLdsKeyAtom2 = 0x4C44535F41544D32ull,
                   kLdsKeyPermVal = 0x4C44535F5045524Dull,
                   kLdsKeyPermMap = 0x4C44535F50455250ull;

// index of one value: block < 2^16, rep < 2^12, sub < 2^5, word < 2^16
VALIDATOR_HD inline uint64_t lds_index(uint32_t block, uint32_t rep, uint32_t sub,
                                       uint32_t word) {
  return ((((uint64_t)block << 12 | rep) << 5 | sub) << 16) | word;
}
VALIDATOR_HD inline uint64_t lds_hash(uint64_t seed, uint64_t key, uint32_t block,
                                      uint32_t rep, uint32_t sub, uint32_t word) {
  return hbm_pattern_value(kHbmPatternHash, seed ^ key,
                           lds_index(block, rep, sub, word));
}

// --- bit 0, pattern --------------------------------------------------------
// patterns 0 .. passes-1 are hash patterns, pattern `passes` is the checker
VALIDATOR_HD inline uint32_t lds_pattern_word(uint64_t seed, int passes,
                                              uint32_t block, uint32_t rep,
                                              int pat, uint32_t w) {
  if (pat >= passes) return (w & 1u) ? 0x55555555u : 0xAAAAAAAAu;
  return (uint32_t)lds_hash(seed, kLdsKeyPattern, block, rep, (uint32_t)pat, w);
}
// access width of step 0 (fill), 1 (verify p, write ~p), 2 (verify ~p) of
// pattern `pat`: 0 = b32, 1 = b64, 2 = b128
VALIDATOR_HD inline int lds_pattern_width(int pat, int step) {
  return (pat + step) % 3;
}

// --- bit 1, subword --------------------------------------------------------
VALIDATOR_HD inline uint32_t lds_subword_word(uint64_t seed, uint32_t block,
                                              uint32_t rep, uint32_t w) {
  return (uint32_t)lds_hash(seed, kLdsKeySubword, block, rep, 0, w);
}
// even 1 KiB chunks are assembled from four byte stores, odd ones from two
// 16-bit stores
VALIDATOR_HD inline bool lds_subword_bytes(uint32_t w) {
  return ((w / kLdsChunkWords) & 1u) == 0;
}

// --- bit 2, transpose ------------------------------------------------------
// The array holds 81920 16-bit elements, element e in half e & 1 of word e / 2.
// A block is 4 rows x 16 columns; a row of the image is 32 * R bytes and holds
// R blocks side by side (R = 2: 64-byte rows, R = 5: 160-byte rows, a 128-byte
// row padded by 32), four rows make a tile.  Both images tile the whole array:
// 1280 blocks of 128 bytes each.
constexpr int kLdsTrBlocks = kLdsBytes / 128;   // 1280
constexpr int kLdsTrRowBlocks[2] = {2, 5};
VALIDATOR_HD inline uint32_t lds_tr_word(uint64_t seed, uint32_t block,
                                         uint32_t rep, uint32_t w) {
  return (uint32_t)lds_hash(seed, kLdsKeyTranspose, block, rep, 0, w);
}
VALIDATOR_HD inline uint32_t lds_tr_elem(uint64_t seed, uint32_t block,
                                         uint32_t rep, uint32_t e) {
  return (lds_tr_word(seed, block, rep, e >> 1) >> (16 * (e & 1u))) & 0xFFFFu;
}
// byte offset of row q, column 0 of block b
VALIDATOR_HD inline uint32_t lds_tr_row_offset(int R, uint32_t b, uint32_t q) {
  return (b / R) * 128u * R + q * 32u * R + (b % R) * 32u;
}
// The documented lane map: lane 4q+p of a 16-lane group supplies the address
// of row q, columns 4p .. 4p+3; lane i receives column i, row q in element q.
VALIDATOR_HD inline uint32_t lds_tr_lane_offset(int R, uint32_t b, uint32_t i) {
  return lds_tr_row_offset(R, b, i >> 2) + 8u * (i & 3u);
}
VALIDATOR_HD inline uint32_t lds_tr_expected_elem(int R, uint32_t b, uint32_t i,
                                                  uint32_t q) {
  return lds_tr_row_offset(R, b, q) / 2u + i;  // element index
}

// --- bit 3, dma ------------------------------------------------------------
// One source buffer of kLdsWords words per run.  A 1 KiB chunk c of LDS is
// filled either by one 16-byte-per-lane load (lane l lands at words 4l .. 4l+3
// of the chunk) or by four 4-byte-per-lane loads (load j, lane l lands at word
// 64j + l): destination = wave-uniform base + lane x size.  The source of
// every destination word is permuted per workgroup and repetition.
VALIDATOR_HD inline uint32_t lds_dma_src_word(uint64_t seed, uint32_t j) {
  return (uint32_t)lds_hash(seed, kLdsKeyDma, 0, 0, 0, j);
}
VALIDATOR_HD inline bool lds_dma_wide(uint32_t rep, uint32_t chunk) {
  return ((chunk + rep) & 1u) == 0;
}
VALIDATOR_HD inline uint32_t lds_dma_src_index(uint32_t block, uint32_t rep,
                                               uint32_t w) {
  const uint32_t c = w / kLdsChunkWords, in = w % kLdsChunkWords;
  const uint32_t sc = (c + 1u + block * 7u + rep * 13u) % kLdsChunks;
  uint32_t sin;
  if (lds_dma_wide(rep, c))  // 16-byte pieces keep their four words together
    sin = 4u * (((in >> 2) * 5u + 3u + block + rep) & 63u) + (in & 3u);
  else
    sin = (in * 37u + 11u + block + rep) & 255u;
  return sc * kLdsChunkWords + sin;
}

// --- bit 4, atomics --------------------------------------------------------
constexpr int kLdsAtomCells = 64;
constexpr int kLdsAtomSteps = 4;
constexpr int kLdsAtomChecks = 10;  // compared values per cell
constexpr int64_t kLdsF32Bound = 1ll << 23;
// word offsets of a cell's fields
constexpr int kLdsCellAdd32 = 0, kLdsCellAddF = 1, kLdsCellAdd64 = 2,
              kLdsCellMax = 4, kLdsCellMin = 5, kLdsCellXor = 6, kLdsCellOr = 7,
              kLdsCellAnd = 8, kLdsCellClaim = 9, kLdsCellConfirm = 10;
// the cells are spread over the whole array and over four bank groups
VALIDATOR_HD inline uint32_t lds_atom_cell_base(uint32_t c) {
  return c * 640u + (c & 3u) * 16u;
}

struct LdsAtomVals {
  uint64_t add64;
  uint32_t add32, mm, x, o, a;
  int addf;  // integer in [-8, 8], added as f32
};
// what thread `tid` applies to cell (tid + step) % 64 in step `step`
VALIDATOR_HD inline LdsAtomVals lds_atom_vals(uint64_t seed, uint32_t block,
                                              uint32_t rep, uint32_t tid,
                                              uint32_t step) {
  const uint64_t h1 = lds_hash(seed, kLdsKeyAtom1, block, rep, step, tid);
  const uint64_t h2 = lds_hash(seed, kLdsKeyAtom2, block, rep, step, tid);
  LdsAtomVals v;
  v.add32 = (uint32_t)h1;
  v.addf = (int)((h1 >> 32) % 17) - 8;
  v.add64 = h2;
  v.mm = (uint32_t)(h1 >> 13);
  v.x = (uint32_t)(h2 >> 20);
  v.o = 1u << ((h2 >> 8) & 31);
  v.a = ~(1u << ((h2 >> 16) & 31));
  return v;
}

struct LdsAtomCell {
  uint64_t add64;
  uint32_t add32, max32, min32, x, o, a;
  int addf, addf_abs;
};
// totals of cell c after the 256 threads ran kLdsAtomSteps steps
VALIDATOR_HD inline LdsAtomCell lds_atom_expected_cell(uint64_t seed,
                                                       uint32_t block,
                                                       uint32_t rep, uint32_t c) {
  LdsAtomCell e = {0ull, 0u, 0u, ~0u, 0u, 0u, ~0u, 0, 0};
  for (uint32_t step = 0; step < (uint32_t)kLdsAtomSteps; ++step)
    for (uint32_t k = 0; k < (uint32_t)(kLdsBlock / kLdsAtomCells); ++k) {
      const uint32_t tid =
          ((c + kLdsAtomCells - step % kLdsAtomCells) % kLdsAtomCells) +
          kLdsAtomCells * k;
      const LdsAtomVals v = lds_atom_vals(seed, block, rep, tid, step);
      e.add32 += v.add32;
      e.add64 += v.add64;
      e.addf += v.addf;
      e.addf_abs += v.addf < 0 ? -v.addf : v.addf;
      e.max32 = v.mm > e.max32 ? v.mm : e.max32;
      e.min32 = v.mm < e.min32 ? v.mm : e.min32;
      e.x ^= v.x;
      e.o |= v.o;
      e.a &= v.a;
    }
  return e;
}

// --- bit 5, permute --------------------------------------------------------
constexpr int kLdsPermSteps = 8;
VALIDATOR_HD inline uint32_t lds_perm_value(uint64_t seed, uint32_t block,
                                            uint32_t rep, uint32_t step,
                                            uint32_t tid) {
  return (uint32_t)lds_hash(seed, kLdsKeyPermVal, block, rep, step, tid);
}
// lane permutation of wave `wave` in step `step`: sigma(l) = (mul * l + add) % 64
// with an odd mul; returns mul | add << 8
VALIDATOR_HD inline uint32_t lds_perm_map(uint64_t seed, uint32_t block,
                                          uint32_t rep, uint32_t step,
                                          uint32_t wave) {
  const uint64_t h = lds_hash(seed, kLdsKeyPermMap, block, rep, step, wave);
  return (((uint32_t)h & 63u) | 1u) | ((uint32_t)(h >> 8) & 63u) << 8;
}
VALIDATOR_HD inline uint32_t lds_perm_sigma(uint32_t map, uint32_t l) {
  return ((map & 63u) * l + (map >> 8)) & 63u;
}
// sigma^-1: the multiplier's inverse mod 64 by Newton steps
VALIDATOR_HD inline uint32_t lds_perm_sigma_inv(uint32_t map, uint32_t l) {
  const uint32_t m = map & 63u;
  uint32_t inv = m;  // correct to 3 bits for an odd m
  inv *= 2u - m * inv;
  inv *= 2u - m * inv;
  return (inv * (l + 64u - (map >> 8))) & 63u;
}

// ---------------------------------------------------------------------------
// Host only
// ---------------------------------------------------------------------------

// items one workgroup compares per repetition, by phase: 32-bit words, and
// for subword also the bytes and halves of its read-back, for transpose the
// 16-bit elements of both images, for atomics the values of every cell, for
// permute the values received
inline uint64_t lds_phase_items(int phase, int passes) {
  switch (phase) {
    case kLdsPhasePattern: return (uint64_t)(passes + 1) * 2 * kLdsWords;
    // every word once, then 4 bytes of one half of the words and 2 halves of
    // the other half
    case kLdsPhaseSubword: return (uint64_t)kLdsWords * 4;
    // 81920 elements under each of the two row strides
    case kLdsPhaseTranspose: return (uint64_t)kLdsWords * 4;
    case kLdsPhaseDma: return (uint64_t)kLdsWords;
    case kLdsPhaseAtomics: return (uint64_t)kLdsAtomCells * kLdsAtomChecks;
    case kLdsPhasePermute: return (uint64_t)kLdsBlock * kLdsPermSteps * 2;
  }
  throw std::invalid_argument("lds_phase_items: phase out of range");
}

struct LdsAtomExpected {
  std::vector<uint32_t> add32, max32, min32, x, o, a;
  std::vector<uint64_t> add64;
  std::vector<int64_t> addf, addf_abs;
};
inline LdsAtomExpected lds_atom_expected(uint64_t seed, uint32_t block,
                                         uint32_t rep) {
  LdsAtomExpected e;
  for (uint32_t c = 0; c < (uint32_t)kLdsAtomCells; ++c) {
    const LdsAtomCell k = lds_atom_expected_cell(seed, block, rep, c);
    // enforced, not assumed: below 2^23 every partial sum is an exact f32
    if ((int64_t)k.addf_abs > kLdsF32Bound)
      throw std::invalid_argument(
          "lds_integrity: the f32 operands of cell " + std::to_string(c) +
          " sum to a magnitude above 2^23");
    e.add32.push_back(k.add32);
    e.add64.push_back(k.add64);
    e.addf.push_back(k.addf);
    e.addf_abs.push_back(k.addf_abs);
    e.max32.push_back(k.max32);
    e.min32.push_back(k.min32);
    e.x.push_back(k.x);
    e.o.push_back(k.o);
    e.a.push_back(k.a);
  }
  return e;
}

inline std::vector<uint32_t> lds_pattern_image(uint64_t seed, int passes,
                                               uint32_t block, uint32_t rep,
                                               int pat) {
  std::vector<uint32_t> v(kLdsWords);
  for (uint32_t w = 0; w < (uint32_t)kLdsWords; ++w)
    v[w] = lds_pattern_word(seed, passes, block, rep, pat, w);
  return v;
}
inline std::vector<uint32_t> lds_subword_image(uint64_t seed, uint32_t block,
                                               uint32_t rep) {
  std::vector<uint32_t> v(kLdsWords);
  for (uint32_t w = 0; w < (uint32_t)kLdsWords; ++w)
    v[w] = lds_subword_word(seed, block, rep, w);
  return v;
}
inline std::vector<uint32_t> lds_tr_image(uint64_t seed, uint32_t block,
                                          uint32_t rep) {
  std::vector<uint32_t> v(kLdsWords);
  for (uint32_t w = 0; w < (uint32_t)kLdsWords; ++w)
    v[w] = lds_tr_word(seed, block, rep, w);
  return v;
}
inline std::vector<uint32_t> lds_dma_source(uint64_t seed) {
  std::vector<uint32_t> v(kLdsWords);
  for (uint32_t j = 0; j < (uint32_t)kLdsWords; ++j) v[j] = lds_dma_src_word(seed, j);
  return v;
}
inline std::vector<uint32_t> lds_dma_image(uint64_t seed, uint32_t block,
                                           uint32_t rep) {
  const std::vector<uint32_t> src = lds_dma_source(seed);
  std::vector<uint32_t> v(kLdsWords);
  for (uint32_t w = 0; w < (uint32_t)kLdsWords; ++w)
    v[w] = src.at(lds_dma_src_index(block, rep, w));
  return v;
}

// every argument of lds_tr_tile is validated here, before the first HIP call
inline void lds_tr_tile_validate(size_t image_elems,
                                 const std::vector<int64_t>& lane_byte_offsets) {
  if (image_elems < 4 || image_elems > (size_t)kLdsBytes / 2)
    throw std::invalid_argument(
        "lds_tr_tile: the image holds 4 to 81920 16-bit elements");
  if (lane_byte_offsets.size() != 64)
    throw std::invalid_argument("lds_tr_tile: one byte offset per lane, 64 in all");
  for (int64_t off : lane_byte_offsets) {
    if (off < 0 || off % 8 != 0)
      throw std::invalid_argument(
          "lds_tr_tile: every lane offset is a non-negative multiple of 8 bytes");
    if ((uint64_t)off + 8 > (uint64_t)image_elems * 2)
      throw std::invalid_argument(
          "lds_tr_tile: a lane's 8 bytes end beyond the image");
  }
}
