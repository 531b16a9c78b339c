// validator_problems_selftest.cpp — stand-alone checks of the GPU validator's
// problem generators (native/validator_problems.hpp).
//
// Built with -fsanitize=address,undefined by
// tests/test_validator_problems_native.py and run as a child process, so the
// index and bit-packing arithmetic of the generators runs under the
// sanitizers.  Beyond that it asserts only what can be stated without the
// code under test: documented table sizes and layouts, codes decoded by the
// decoders written here from the format definitions, expected tiles
// recomputed in double precision, and published splitmix64 values.  The host
// side of a launch's results lives there too and is checked on hand-built
// tables: the per-unit tally of a sweep, the digest grouping of the
// vector-ALU sweep, the kept count of a record log and the range checks.

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// --- decoders written from the format definitions -------------------------

// OCP minifloat: sign, ebits exponent bits with `bias`, mbits mantissa bits
double ref_minifloat(int ebits, int mbits, int bias, unsigned code) {
  const int e = (code >> mbits) & ((1u << ebits) - 1);
  const int m = code & ((1u << mbits) - 1);
  const bool neg = (code >> (ebits + mbits)) & 1u;
  const double v = e == 0 ? std::ldexp((double)m, 1 - bias - mbits)
                          : std::ldexp((double)((1 << mbits) + m), e - bias - mbits);
  return neg ? -v : v;
}
double ref_e4m3(unsigned code) { return ref_minifloat(4, 3, 7, code); }

// the five MX element formats by cbsz / blgp code: bits, ebits, mbits, bias
const int kRefMx[5][4] = {
    {8, 4, 3, 7}, {8, 5, 2, 15}, {6, 2, 3, 1}, {6, 3, 2, 3}, {4, 2, 1, 1}};
double ref_mx(int fmt, unsigned code) {
  return ref_minifloat(kRefMx[fmt][1], kRefMx[fmt][2], kRefMx[fmt][3], code);
}
double ref_e8m0(unsigned code) { return std::ldexp(1.0, (int)code - 127); }

float ref_bits_to_f32(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
uint32_t ref_f32_to_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// bits [pos, pos + width) of a little-endian string of 32-bit words
unsigned ref_field(const uint32_t* words, int pos, int width) {
  unsigned v = 0;
  for (int b = 0; b < width; ++b)
    v |= ((words[(pos + b) >> 5] >> ((pos + b) & 31)) & 1u) << b;
  return v;
}

// 16 x K by K x 16 (or m x k by k x n) product in double
std::vector<double> ref_product(const std::vector<double>& a,
                                const std::vector<double>& b, int M, int N, int K) {
  std::vector<double> d((size_t)M * N, 0.0);
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) d[m * N + n] += a[m * K + k] * b[k * N + n];
  return d;
}

std::vector<double> to_double(const std::vector<float>& v) {
  return std::vector<double>(v.begin(), v.end());
}

// --- e4m3 codec ------------------------------------------------------------

void test_e4m3() {
  // every integer e4m3 holds exactly (3 mantissa bits: all of -16..16)
  for (int v = -16; v <= 16; ++v) {
    const uint8_t c = encode_e4m3fn_nearest((float)v);
    CHECK((c & 0x7F) != 0x7F);
    CHECK(ref_e4m3(c) == (double)v);
  }
  for (unsigned c = 0; c < 256; ++c)
    if ((c & 0x7F) != 0x7F) CHECK((double)decode_e4m3fn((uint8_t)c) == ref_e4m3(c));
}

// --- per-CU coverage problems and their table -------------------------------

double cov_ref_decode(int dt, uint32_t enc) {
  if (dt == 0) return ref_bits_to_f32(enc);
  if (dt == 1) return ref_bits_to_f32(enc << 16);
  return ref_e4m3(enc);
}

void test_cov() {
  const std::vector<uint32_t> tab = cov_build_table();
  // 4 sets x 64 lanes x (2 f32 + 8 bf16 + 4 fp8 operand words + 12 expected)
  CHECK(tab.size() == (size_t)4 * 64 * 26);
  CHECK(kCovRecWords == 26);
  for (int s = 0; s < 4; ++s) {
    CovProblem pr[3] = {cov_problem(s, 0), cov_problem(s, 1), cov_problem(s, 2)};
    for (int dt = 0; dt < 3; ++dt) {
      const CovProblem& p = pr[dt];
      const int K = dt == 0 ? 4 : 32;
      CHECK(p.k == K);
      CHECK(p.a_enc.size() == (size_t)16 * K && p.b_enc.size() == (size_t)16 * K);
      CHECK(p.a_dec.size() == (size_t)16 * K && p.b_dec.size() == (size_t)16 * K);
      CHECK(p.d.size() == 256);
      if (p.a_enc.size() != (size_t)16 * K || p.a_dec.size() != p.a_enc.size() ||
          p.b_enc.size() != p.a_enc.size() || p.b_dec.size() != p.a_enc.size() ||
          p.d.size() != 256)
        return;
      for (int i = 0; i < 16 * K; ++i) {
        CHECK((double)p.a_dec[i] == cov_ref_decode(dt, p.a_enc[i]));
        CHECK((double)p.b_dec[i] == cov_ref_decode(dt, p.b_enc[i]));
        CHECK(std::fabs(p.a_dec[i]) <= 8.f && std::fabs(p.b_dec[i]) <= 8.f);
        CHECK(p.a_dec[i] == std::floor(p.a_dec[i]));
      }
      const std::vector<double> want =
          ref_product(to_double(p.a_dec), to_double(p.b_dec), 16, 16, K);
      for (int i = 0; i < 256; ++i) CHECK((double)p.d[i] == want[i]);
    }
    if (tab.size() != (size_t)4 * 64 * 26) continue;
    // the documented fragment layout of every lane record
    for (int l = 0; l < 64; ++l) {
      const uint32_t* r = &tab[(size_t)(s * 64 + l) * 26];
      const int lo = l & 15, hi = l >> 4;
      CHECK(r[0] == pr[0].a_enc[lo * 4 + hi]);
      CHECK(r[1] == pr[0].b_enc[hi * 16 + lo]);
      for (int i = 0; i < 8; ++i) {
        const int k = hi * 8 + i;
        CHECK(ref_field(r + 2, 16 * i, 16) == pr[1].a_enc[lo * 32 + k]);
        CHECK(ref_field(r + 6, 16 * i, 16) == pr[1].b_enc[k * 16 + lo]);
        CHECK(ref_field(r + 10, 8 * i, 8) == pr[2].a_enc[lo * 32 + k]);
        CHECK(ref_field(r + 12, 8 * i, 8) == pr[2].b_enc[k * 16 + lo]);
      }
      for (int t = 0; t < 3; ++t)
        for (int q = 0; q < 4; ++q)
          CHECK(r[14 + t * 4 + q] ==
                ref_f32_to_bits(pr[t].d[(hi * 4 + q) * 16 + lo]));
    }
  }
}

// --- MX problems and their table -------------------------------------------

// documented C/D maps: where register r of lane l sits in the m x n tile
int mx_ref_d_index(int shape, int l, int r) {
  if (shape == 0) return ((l >> 4) * 4 + r) * 16 + (l & 15);
  return ((r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31);
}

void check_mx_problem(const MxProblem& p, int set, int fa, int fb, int shape) {
  const int M = shape == 0 ? 16 : 32, N = M, K = shape == 0 ? 128 : 64, KB = K / 32;
  CHECK(p.set == set && p.fa == fa && p.fb == fb && p.shape == shape);
  CHECK(p.m == M && p.n == N && p.k == K && p.kblocks == KB);
  CHECK(p.sel_a >= 0 && p.sel_a < 4 && p.sel_b >= 0 && p.sel_b < 4);
  CHECK(p.a_codes.size() == (size_t)M * K && p.b_codes.size() == (size_t)K * N);
  CHECK(p.a_scales.size() == (size_t)M * KB && p.b_scales.size() == (size_t)KB * N);
  CHECK(p.d.size() == (size_t)M * N);
  CHECK(p.a_words.size() == 512 && p.b_words.size() == 512);
  CHECK(p.a_scale_words.size() == 64 && p.b_scale_words.size() == 64);
  CHECK(p.log2_span <= 20.0);
  if (p.a_codes.size() != (size_t)M * K || p.b_codes.size() != (size_t)K * N ||
      p.a_scales.size() != (size_t)M * KB || p.b_scales.size() != (size_t)KB * N ||
      p.d.size() != (size_t)M * N || p.a_words.size() != 512 ||
      p.b_words.size() != 512 || p.a_scale_words.size() != 64 ||
      p.b_scale_words.size() != 64 || p.sel_a < 0 || p.sel_a > 3 || p.sel_b < 0 ||
      p.sel_b > 3)
    return;

  // expected tile == sum of decoded element x decoded scale products; with
  // S/q <= 2^20 every partial sum is exact in double
  std::vector<double> a((size_t)M * K), b((size_t)K * N);
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < K; ++k)
      a[m * K + k] = ref_mx(fa, p.a_codes[m * K + k]) *
                     ref_e8m0(p.a_scales[m * KB + k / 32]);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n)
      b[k * N + n] = ref_mx(fb, p.b_codes[k * N + n]) *
                     ref_e8m0(p.b_scales[(k / 32) * N + n]);
  const std::vector<double> want = ref_product(a, b, M, N, K);
  for (int i = 0; i < M * N; ++i) CHECK((double)p.d[i] == want[i]);

  // the documented fragment layout: lane l holds row / col l % M, lane group
  // g = l / M; element j sits at bits [w*j, w*j + w); 8-bit lanes hold two
  // runs of 16, the narrower formats are K-contiguous; unused words are zero
  const int wa = kRefMx[fa][0], wb = kRefMx[fb][0];
  for (int l = 0; l < 64; ++l) {
    const int rc = l % M, g = l / M;
    for (int j = 0; j < 32; ++j) {
      const int ka = wa == 8 ? (K / 2) * (j >> 4) + 16 * g + (j & 15) : 32 * g + j;
      const int kb = wb == 8 ? (K / 2) * (j >> 4) + 16 * g + (j & 15) : 32 * g + j;
      CHECK(ref_field(&p.a_words[l * 8], wa * j, wa) == p.a_codes[rc * K + ka]);
      CHECK(ref_field(&p.b_words[l * 8], wb * j, wb) == p.b_codes[kb * N + rc]);
    }
    for (int w = wa; w < 8; ++w) CHECK(p.a_words[l * 8 + w] == 0);
    for (int w = wb; w < 8; ++w) CHECK(p.b_words[l * 8 + w] == 0);
    // lane group g supplies the scale of K block g in the op_sel byte
    CHECK(((p.a_scale_words[l] >> (8 * p.sel_a)) & 0xFF) == p.a_scales[rc * KB + g]);
    CHECK(((p.b_scale_words[l] >> (8 * p.sel_b)) & 0xFF) == p.b_scales[g * N + rc]);
  }

  const std::vector<uint32_t> rec = mx_tile_record(p);
  CHECK(rec.size() == (size_t)64 * 18);
  if (rec.size() != (size_t)64 * 18) return;
  for (int l = 0; l < 64; ++l) {
    CHECK(std::memcmp(&rec[l * 18], &p.a_words[l * 8], 32) == 0);
    CHECK(std::memcmp(&rec[l * 18 + 8], &p.b_words[l * 8], 32) == 0);
    CHECK(rec[l * 18 + 16] == p.a_scale_words[l]);
    CHECK(rec[l * 18 + 17] == p.b_scale_words[l]);
  }
}

// the sweep's ten problems: format pair and shape, as documented
const int kRefProb[10][3] = {{0, 0, 0}, {1, 1, 0}, {2, 2, 0}, {3, 3, 0}, {4, 4, 0},
                             {0, 4, 0}, {4, 2, 0}, {3, 1, 0}, {4, 4, 1}, {0, 0, 1}};

void test_mx() {
  const std::vector<uint32_t> tab = mx_build_table();
  // 5 sets x 10 problems x 64 lanes x (16 operand + 2 scale + 16 expected)
  CHECK(tab.size() == (size_t)5 * 10 * 64 * 34);
  CHECK(kMxRecWords == 34 && kMxTileRecWords == 18);
  bool in_sweep[5][5][2] = {};
  for (int s = 0; s < 5; ++s)
    for (int i = 0; i < 10; ++i) {
      const int fa = kRefProb[i][0], fb = kRefProb[i][1], sh = kRefProb[i][2];
      CHECK(kMxProbFa[i] == fa && kMxProbFb[i] == fb && kMxProbShape[i] == sh);
      in_sweep[fa][fb][sh] = true;
      const MxProblem p = mx_problem(s, fa, fb, sh);  // must not throw
      check_mx_problem(p, s, fa, fb, sh);
      if (tab.size() != (size_t)5 * 10 * 64 * 34 || p.a_words.size() != 512 ||
          p.b_words.size() != 512 || p.d.size() != (size_t)p.m * p.n)
        continue;
      for (int l = 0; l < 64; ++l) {
        const uint32_t* r = &tab[(size_t)((s * 10 + i) * 64 + l) * 34];
        CHECK(std::memcmp(r, &p.a_words[l * 8], 32) == 0);
        CHECK(std::memcmp(r + 8, &p.b_words[l * 8], 32) == 0);
        CHECK(r[16] == p.a_scale_words[l] && r[17] == p.b_scale_words[l]);
        for (int q = 0; q < 16; ++q)
          CHECK(r[18 + q] == (q < (sh == 0 ? 4 : 16)
                                  ? ref_f32_to_bits(p.d[mx_ref_d_index(sh, l, q)])
                                  : 0u));
      }
    }
  // every other combination: a problem, or a domain_error where the pair's
  // alphabets cannot meet the exactness bound (by design)
  int built = 0, refused = 0;
  for (int s = 0; s < 5; ++s)
    for (int fa = 0; fa < 5; ++fa)
      for (int fb = 0; fb < 5; ++fb)
        for (int sh = 0; sh < 2; ++sh) {
          if (in_sweep[fa][fb][sh]) continue;
          try {
            const MxProblem p = mx_problem(s, fa, fb, sh);
            check_mx_problem(p, s, fa, fb, sh);
            ++built;
          } catch (const std::domain_error&) {
            ++refused;
          }
        }
  CHECK(built + refused == 5 * (5 * 5 * 2 - 10));
  std::printf("mx: %d other combinations built, %d refused\n", built, refused);
  // arguments out of range are refused before anything is indexed
  for (int bad = 0; bad < 4; ++bad) {
    bool threw = false;
    try {
      mx_problem(bad == 0 ? 5 : 0, bad == 1 ? 5 : 0, bad == 2 ? -1 : 0,
                 bad == 3 ? 2 : 0);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw);
  }
}

void test_mx_burn_seed() {
  for (int f : {4, 0}) {  // e2m1, e4m3
    const std::vector<uint32_t> seed = mx_burn_seed(f);
    CHECK(seed.size() == (size_t)64 * 16 + 1);
    if (seed.size() != (size_t)64 * 16 + 1) continue;
    // both scales 2^-20 in every byte: E8M0 code 127 - 20
    CHECK(seed[64 * 16] == 0x6B6B6B6Bu);
    const int w = kRefMx[f][0];
    for (int l = 0; l < 64; ++l)
      for (int h = 0; h < 2; ++h) {
        const uint32_t* words = &seed[l * 16 + h * 8];
        for (int j = 0; j < 32; ++j) {
          const double v = ref_mx(f, ref_field(words, w * j, w));
          CHECK(v != 0.0 && std::isfinite(v) && std::fabs(v) <= 448.0);
        }
        for (int i = w; i < 8; ++i) CHECK(words[i] == 0);
      }
  }
}

// --- single-wave smoke tiles -------------------------------------------------

template <typename T, typename Decode>
void check_smoke(const SmokeTile<T>& t, int K, Decode decode) {
  CHECK(t.k == K);
  CHECK(t.a_enc.size() == (size_t)16 * K && t.b_enc.size() == (size_t)16 * K);
  CHECK(t.a_dec.size() == (size_t)16 * K && t.b_dec.size() == (size_t)16 * K);
  CHECK(t.ref.size() == 256);
  if (t.a_enc.size() != (size_t)16 * K || t.b_enc.size() != (size_t)16 * K ||
      t.a_dec.size() != (size_t)16 * K || t.b_dec.size() != (size_t)16 * K ||
      t.ref.size() != 256)
    return;
  for (int i = 0; i < 16 * K; ++i) {
    CHECK((double)t.a_dec[i] == decode(t.a_enc[i]));
    CHECK((double)t.b_dec[i] == decode(t.b_enc[i]));
  }
  // A and B are unrelated and neither is constant
  CHECK(t.a_dec != t.b_dec);
  CHECK(t.a_dec[0] != t.a_dec[1] && t.b_dec[0] != t.b_dec[1]);
  // a K-step fmaf chain rounds once per step: |ref - exact| <= K u S (1 + u)^K
  // with u = 2^-24 and S the sum of |a b| of that output
  const std::vector<double> a = to_double(t.a_dec), b = to_double(t.b_dec);
  const std::vector<double> want = ref_product(a, b, 16, 16, K);
  for (int m = 0; m < 16; ++m)
    for (int n = 0; n < 16; ++n) {
      double S = 0.0;
      for (int k = 0; k < K; ++k) S += std::fabs(a[m * K + k] * b[k * 16 + n]);
      const double bound = 1.001 * K * std::ldexp(1.0, -24) * S;
      CHECK(std::fabs((double)t.ref[m * 16 + n] - want[m * 16 + n]) <= bound);
    }
}

void test_smoke() {
  const auto bf16 = [](uint16_t v) { return (double)ref_bits_to_f32((uint32_t)v << 16); };
  check_smoke(smoke_f32_problem(), 4, [](float v) { return (double)v; });
  check_smoke(smoke_bf16_problem(), 32, bf16);
  check_smoke(smoke_bf16_tile_problem(), 32, bf16);
  const SmokeTile<uint8_t> q = smoke_fp8_problem();
  check_smoke(q, 32, [](uint8_t v) { return ref_e4m3(v); });
  for (uint8_t c : q.a_enc) CHECK((c & 0x7F) != 0x7F);
  for (uint8_t c : q.b_enc) CHECK((c & 0x7F) != 0x7F);
  // the two bf16 problems are different problems
  CHECK(smoke_bf16_problem().a_enc != smoke_bf16_tile_problem().a_enc);

  // an element of either bf16 problem is the nearest bf16 of its formula:
  // within half a bf16 ulp (at most 2^-8 relative) of it
  const SmokeTile<uint16_t> t = smoke_bf16_tile_problem();
  for (int i = 0; i < 16 * 32; ++i) {
    const double want = (double)(0.07f * (float)((i * 13) % 41) - 1.2f);
    CHECK(std::fabs((double)t.a_dec[i] - want) <= std::ldexp(std::fabs(want), -8));
  }
  const SmokeTile<uint16_t> c = smoke_bf16_problem();
  for (int i = 0; i < 16 * 32; ++i) {
    const double want = (double)(0.03f * (float)((i * 3) % 29) - 0.4f);
    CHECK(std::fabs((double)c.a_dec[i] - want) <= std::ldexp(std::fabs(want), -8));
  }

  // the burn-in seed truncates: never above its f32 value, less than one
  // bf16 ulp (2^-7 relative) below it
  const std::vector<uint16_t> seed = bf16_burn_seed();
  CHECK(seed.size() == 256);
  for (size_t i = 0; i < seed.size(); ++i) {
    const double f = (double)(0.001f + 0.00001f * (float)(i % 17));
    const double v = bf16(seed[i]);
    CHECK(v <= f && v > f * (1.0 - std::ldexp(1.0, -7)));
  }

  CHECK(max_abs_err({1.f, 2.f, -3.f}, {1.f, 2.5f, -1.f}) == 2.0);
  CHECK(max_abs_err({1.f}, {1.f}) == 0.0);
}

// --- HBM pattern and cross-XCD generators -----------------------------------

void test_patterns() {
  // checker: 0xAAAA.. on even indices, 0x5555.. on odd ones, seed ignored
  CHECK(hbm_pattern_value(kHbmPatternChecker, 7, 0) == 0xAAAAAAAAAAAAAAAAull);
  CHECK(hbm_pattern_value(kHbmPatternChecker, 7, 1) == 0x5555555555555555ull);
  CHECK(hbm_pattern_value(kHbmPatternChecker, 7, 1ull << 62) == 0xAAAAAAAAAAAAAAAAull);
  // hash: the splitmix64 finaliser of i + seed * golden; seeds 1, 2, 3 at
  // index 0 are the first three outputs of splitmix64 from state 0
  CHECK(hbm_pattern_value(kHbmPatternHash, 1, 0) == 0xE220A8397B1DCDAFull);
  CHECK(hbm_pattern_value(kHbmPatternHash, 2, 0) == 0x6E789E6AA1B965F4ull);
  CHECK(hbm_pattern_value(kHbmPatternHash, 3, 0) == 0x06C45D188009454Full);
  CHECK(hbm_pattern_value(kHbmPatternHash, 1, 1) == 0x910A2DEC89025CC1ull);
  CHECK(hbm_pattern_value(kHbmPatternHash, 1, 1ull << 62) == 0x00AA50EA8E0FA9EBull);
  CHECK(hbm_pattern_value(kHbmPatternHash, 0, 5) == 0xB6BF613DBEBB45DCull);

  // [reps][blocks][slab_lines]
  CHECK(xf_line_index(32, 8, 1, 2, 3) == (1u * 32 + 2) * 8 + 3);
  CHECK(xf_line_index(1024, 32, 63, 1023, 31) == (63ull * 1024 + 1023) * 32 + 31);
  // static words: the hash under seed ^ "STATIC_X"; payload: seed + round,
  // round -1 being the initial upload
  CHECK(kXfStaticKey == 0x5354415449435F58ull);
  CHECK(xf_static_word(1, 7) == 0xDD66779232EEAAD9ull);
  CHECK(xf_payload_word(1, -1, 5) == 0xB6BF613DBEBB45DCull);
  CHECK(xf_payload_word(1, 1, 0) == 0x6E789E6AA1B965F4ull);
}

bool atom_expected_throws(uint64_t threads, int reps, int cells) {
  try {
    xf_atom_expected(1, threads, reps, cells);
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

void test_atomics() {
  for (uint64_t id = 0; id < 4096; ++id) {
    const XfAtomVals v = xf_atom_vals(1, id, (uint32_t)(id % 64));
    CHECK(v.addf >= -8 && v.addf <= 8);
    CHECK(__builtin_popcount(v.o) <= 1 && __builtin_popcount(v.a) >= 31);
  }
  const XfAtomExpected e = xf_atom_expected(1, 512, 3, 5);
  CHECK(e.add32.size() == 5 && e.x.size() == 5 && e.o.size() == 5 && e.a.size() == 5);
  CHECK(e.add64.size() == 5 && e.max64.size() == 5 && e.min64.size() == 5);
  CHECK(e.addf.size() == 5);
  int64_t mag = 0;
  for (size_t c = 0; c < e.addf.size(); ++c) {
    mag += e.addf[c] < 0 ? -e.addf[c] : e.addf[c];
    if (c < e.min64.size() && c < e.max64.size()) CHECK(e.min64[c] <= e.max64[c]);
  }
  CHECK(mag <= 8 * 512 * 3);

  // The 2^23 bound on a cell's sum of f32 magnitudes.  An operand is at most
  // 8, so 64 reps of up to 2^23 / (8 * 64) = 16384 threads on one cell can
  // never reach it, whatever the hash gives:
  CHECK(!atom_expected_throws(512, 64, 1));
  CHECK(!atom_expected_throws(16384, 64, 1));
  // Operands are uniform on -8..8: mean magnitude 72/17, standard deviation
  // 2.47.  N = 64 * threads of them sum to N * 72/17 on average, which passes
  // 2^23 at 30948 threads; 31076 is the smallest count whose expected sum
  // lies ten standard deviations (10 * 2.47 * sqrt(N)) above the bound.
  CHECK(atom_expected_throws(31076, 64, 1));
}

// planes of a sweep, sized exactly: ASan sees a read past any of them
struct Planes {
  int simds;
  std::vector<uint32_t> v;
  explicit Planes(int s) : simds(s), v((size_t)4 * kCovKeys * s, 0u) {}
  void set(int key, int simd, uint32_t waves, uint32_t fail, uint32_t hw,
           uint32_t xcc) {
    const size_t n = (size_t)kCovKeys * simds, at = (size_t)key * simds + simd;
    v[at] = waves, v[n + at] = fail, v[2 * n + at] = hw, v[3 * n + at] = xcc;
  }
};

void test_tally() {
  for (int simds : {4, 1}) {  // the sweeps' form and the per-key (LDS) form
    Planes p(simds);
    CovTally t = cov_tally(p.v.data(), 2, simds);
    CHECK(t.units.empty() && t.cus_covered == 0 && t.slots_covered == 0);
    CHECK(t.waves_run == 0 && t.failed_slots == 0 && !t.complete);

    // cus = 2: key 0x000 whole, key 0x101 without its last SIMD
    for (int s = 0; s < simds; ++s) p.set(0x000, s, 1, 0, 0, 0);
    for (int s = 0; s + 1 < simds; ++s) p.set(0x101, s, 1, 0, 0, 0);
    t = cov_tally(p.v.data(), 2, simds);
    if (simds == 4) {
      CHECK(t.cus_covered == 2 && t.slots_covered == 7 && !t.complete);
    } else {
      CHECK(t.cus_covered == 1 && t.slots_covered == 1 && !t.complete);
    }
    p.set(0x101, simds - 1, 1, 0, 0, 0);
    t = cov_tally(p.v.data(), 2, simds);
    CHECK(t.cus_covered == 2 && t.slots_covered == 2 * simds && t.complete);
    CHECK(t.waves_run == 2 * simds && t.failed_slots == 0);
    CHECK(t.units.size() == (size_t)2 * simds);
    CHECK(!cov_tally(p.v.data(), 3, simds).complete);

    // one slot: counts, and the raw words carried through
    Planes q(simds);
    q.set(0x2A5, simds - 1, 3, 0b101u, 0xCAFE0123u, 0x80000002u);
    t = cov_tally(q.v.data(), 1, simds);
    CHECK(t.waves_run == 3 && t.failed_slots == 1 && t.units.size() == 1);
    if (t.units.size() == 1) {
      const CovUnit& u = t.units[0];
      CHECK(u.key == 0x2A5 && u.simd == simds - 1 && u.waves == 3);
      CHECK(u.fail_mask == 0b101u && u.hw_id_raw == 0xCAFE0123u);
      CHECK(u.xcc_id_raw == 0x80000002u);
    }

    // the last slot of the planes
    Planes l(simds);
    l.set(kCovKeys - 1, simds - 1, 2, 0, 7, 9);
    t = cov_tally(l.v.data(), 1, simds);
    CHECK(t.units.size() == 1 && t.cus_covered == 1 && t.waves_run == 2);
    if (t.units.size() == 1) {
      CHECK(t.units[0].key == kCovKeys - 1 && t.units[0].simd == simds - 1);
      CHECK(t.units[0].hw_id_raw == 7 && t.units[0].xcc_id_raw == 9);
    }
  }
}

void test_digest_grouping() {
  const int W = 3;  // slot + 1 | two digests
  const std::vector<uint64_t> recs = {
      0, 1, 1,                            // never written: skipped
      (uint64_t)kCovSlots + 1, 2, 2,      // above the slots: skipped
      6, 10, 11,                          // slot 5
      6, 10, 11,                          // the same tuple again: one entry
      6, 10, 12,                          // another tuple: kept, second
      6, 9, 11,                           // and a third, in first-seen order
      (uint64_t)kCovSlots, 3, 4,          // the last slot
  };
  const auto by_slot = valu_group_digests(recs.data(), recs.size() / W, W);
  CHECK(by_slot.size() == (size_t)kCovSlots);
  size_t filled = 0;
  for (const auto& s : by_slot) filled += !s.empty();
  CHECK(filled == 2);
  using T = std::vector<uint64_t>;
  CHECK(by_slot[5].size() == 3);
  if (by_slot[5].size() == 3) {
    CHECK(by_slot[5][0] == (T{10, 11}) && by_slot[5][1] == (T{10, 12}));
    CHECK(by_slot[5][2] == (T{9, 11}));
  }
  CHECK(by_slot[kCovSlots - 1].size() == 1);
  if (by_slot[kCovSlots - 1].size() == 1) CHECK(by_slot[kCovSlots - 1][0] == (T{3, 4}));
  CHECK(valu_group_digests(recs.data(), 0, W)[5].empty());
}

bool range_throws(long v, long lo, long hi, const char* want) {
  try {
    require_range("some_check", "reps", v, lo, hi);
  } catch (const std::invalid_argument& e) {
    return std::strcmp(e.what(), want) == 0;
  }
  return false;
}

void test_record_log_and_ranges() {
  // kept = min(claims, cap); what a check reports as dropped is its own
  // count minus kept
  CHECK(record_log_kept(0, 64) == 0);
  CHECK(record_log_kept(64, 64) == 64);
  CHECK(record_log_kept(69, 64) == 64 && 69 - record_log_kept(69, 64) == 5);
  // a later phase of the host-link check, the room used up before it
  CHECK(record_log_kept(3, 0) == 0 && 3 - record_log_kept(3, 0) == 3);
  CHECK(record_log_kept(~0ull, 4096) == 4096);

  CHECK(range_throws(0, 1, 4096, "some_check: reps must be in [1, 4096]"));
  CHECK(range_throws(64, -1, 63, "some_check: reps must be in [-1, 63]"));
  CHECK(!range_throws(1, 1, 4096, "") && !range_throws(4096, 1, 4096, ""));
  for (int key : {-2, kCovKeys}) {
    bool threw = false;
    try {
      require_poison_key("some_check", key);
    } catch (const std::invalid_argument& e) {
      threw = std::strcmp(e.what(), "some_check: poison_key out of range") == 0;
    }
    CHECK(threw);
  }
  require_poison_key("some_check", -1);
  require_poison_key("some_check", kCovKeys - 1);
}

}  // namespace

int main() {
  test_tally();
  test_digest_grouping();
  test_record_log_and_ranges();
  test_e4m3();
  test_cov();
  test_mx();
  test_mx_burn_seed();
  test_smoke();
  test_patterns();
  test_atomics();
  if (g_failures) {
    std::fprintf(stderr, "validator_problems selftest: %d of %d checks FAILED\n",
                 g_failures, g_checks);
    return 1;
  }
  std::printf("validator_problems selftest: %d checks passed\n", g_checks);
  return 0;
}
