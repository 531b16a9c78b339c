// validator_problems.hpp — the exact problems of gpu_validator.hip: operand
// generators, codecs, packed per-lane tables, expected results, and the
// records and constants the kernels share with them.
//
// Plain C++17: no HIP and no Python header, so
// tests/native/validator_problems_selftest.cpp drives all of it stand-alone
// under AddressSanitizer + UBSan.  The functions the kernels call as well are
// marked VALIDATOR_HD.  The generators of the LDS data-integrity check are in
// lds_problems.hpp, those of the host-link check in hostlink_problems.hpp and
// those of the vector-ALU check in valu_problems.hpp, all included at the end.

#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define VALIDATOR_HD __host__ __device__
#else
#define VALIDATOR_HD
#endif

// ---------------------------------------------------------------------------
// Bit helpers and the OCP e4m3fn codec
// ---------------------------------------------------------------------------

inline uint32_t f32_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
// round to nearest even
inline uint16_t to_bf16(float f) {
  const uint32_t u = f32_bits(f);
  return (uint16_t)((u + 0x7FFF + ((u >> 16) & 1)) >> 16);
}
inline float from_bf16(uint16_t v) {
  uint32_t u = (uint32_t)v << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

inline float decode_e4m3fn(uint8_t u) {
  int s = (u >> 7) & 1;
  int e = (u >> 3) & 0xF;
  int m = u & 7;
  float v;
  if (e == 0) {
    v = (float)m / 8.0f * (1.0f / 64.0f);  // subnormal: 2^-6 scale
  } else if (e == 15 && m == 7) {
    v = 0.0f;  // NaN code; never produced by our encoder
  } else {
    v = (1.0f + (float)m / 8.0f) * std::ldexp(1.0f, e - 7);
  }
  return s ? -v : v;
}

inline uint8_t encode_e4m3fn_nearest(float f) {
  // exact nearest-representable search over the 256-code table (fine for a
  // smoke test; avoids re-deriving RNE tie rules)
  uint8_t best = 0;
  float best_err = 1e30f;
  for (int u = 0; u < 256; ++u) {
    if ((u & 0x7F) == 0x7F) continue;  // NaN codes
    float err = std::fabs(decode_e4m3fn((uint8_t)u) - f);
    if (err < best_err) {
      best_err = err;
      best = (uint8_t)u;
    }
  }
  return best;
}

// ---------------------------------------------------------------------------
// Single-wave smoke tiles: 16 x K by K x 16, row-major.  Each generator
// returns the operands as the kernel reads them, the f32 values they decode
// to, and the reference tile: a k-ordered fmaf chain over the decoded values
// (guide: bitwise equal to the f32 MFMA).  The four operand formulas differ
// on purpose; all are asymmetric so transposed writes can't pass.
// ---------------------------------------------------------------------------

template <typename T>
struct SmokeTile {
  int k = 0;
  std::vector<T> a_enc, b_enc;
  std::vector<float> a_dec, b_dec, ref;  // 16xK, Kx16, 16x16
};

// element i of A is enc(gen_a(i)), likewise B
template <typename T, typename Enc, typename Dec, typename GenA, typename GenB>
inline SmokeTile<T> smoke_tile(int K, Enc enc, Dec dec, GenA gen_a, GenB gen_b) {
  SmokeTile<T> t;
  t.k = K;
  t.a_enc.resize(16 * K);
  t.b_enc.resize(16 * K);
  t.a_dec.resize(16 * K);
  t.b_dec.resize(16 * K);
  t.ref.resize(16 * 16);
  for (int i = 0; i < 16 * K; ++i) {
    t.a_dec[i] = dec(t.a_enc[i] = enc(gen_a(i)));
    t.b_dec[i] = dec(t.b_enc[i] = enc(gen_b(i)));
  }
  for (int m = 0; m < 16; ++m)
    for (int n = 0; n < 16; ++n) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k)
        acc = fmaf(t.a_dec[m * K + k], t.b_dec[k * 16 + n], acc);
      t.ref[m * 16 + n] = acc;
    }
  return t;
}

inline SmokeTile<float> smoke_f32_problem() {
  const auto same = [](float f) { return f; };
  return smoke_tile<float>(
      4, same, same, [](int i) { return 0.01f * (float)(i % 37) - 0.15f; },
      [](int i) { return 0.02f * (float)((i * 7) % 23) - 0.2f; });
}

// mfma_bf16_check
inline SmokeTile<uint16_t> smoke_bf16_problem() {
  return smoke_tile<uint16_t>(
      32, to_bf16, from_bf16,
      [](int i) { return 0.03f * (float)((i * 3) % 29) - 0.4f; },
      [](int i) { return 0.015f * (float)((i * 11) % 31) - 0.2f; });
}

// mfma_bf16_tile: wider values, checked in Python against an fp32 reference
inline SmokeTile<uint16_t> smoke_bf16_tile_problem() {
  return smoke_tile<uint16_t>(
      32, to_bf16, from_bf16,
      [](int i) { return 0.07f * (float)((i * 13) % 41) - 1.2f; },
      [](int i) { return 0.05f * (float)((i * 17) % 37) - 0.8f; });
}

inline SmokeTile<uint8_t> smoke_fp8_problem() {
  return smoke_tile<uint8_t>(
      32, encode_e4m3fn_nearest, decode_e4m3fn,
      [](int i) { return 0.05f * (float)((i * 5) % 23) - 0.5f; },
      [](int i) { return 0.03f * (float)((i * 7) % 19) - 0.25f; });
}

inline double max_abs_err(const std::vector<float>& got,
                          const std::vector<float>& ref) {
  double max_err = 0.0;
  for (size_t i = 0; i < ref.size(); ++i)
    max_err = std::max(max_err, (double)std::fabs(got[i] - ref[i]));
  return max_err;
}

// 256 bf16 around 1e-3 so the burn-in accumulators stay finite; truncated,
// not rounded
inline std::vector<uint16_t> bf16_burn_seed() {
  std::vector<uint16_t> seed(256);
  for (int i = 0; i < 256; ++i)
    seed[i] = (uint16_t)(f32_bits(0.001f + 0.00001f * (float)(i % 17)) >> 16);
  return seed;
}

// ---------------------------------------------------------------------------
// Per-CU coverage sweep problems.  Operands are small integers (|v| <= 8,
// exact in f32, bf16 and e4m3), so every K=32 dot product is an integer
// <= 2048 and exact in f32 in any summation order.
// ---------------------------------------------------------------------------

constexpr int kCovSets = 4;  // operand sets per repetition

// Per-lane record of one operand set, already in MFMA fragment order (the
// layouts documented on the three smoke kernels), packed by the host.
struct CovLaneRec {
  uint32_t f32_a, f32_b;        // A[l&15][l>>4], B[l>>4][l&15]
  uint32_t bf16_a[4], bf16_b[4];  // 8 bf16: A[l&15][(l>>4)*8+i], B[(l>>4)*8+i][l&15]
  uint32_t fp8_a[2], fp8_b[2];  // 8 e4m3, same geometry as bf16
  uint32_t exp[3][4];           // expected D[(l>>4)*4+r][l&15] bits per dtype
};
constexpr int kCovRecWords = sizeof(CovLaneRec) / sizeof(uint32_t);

// Integer operand generators: |v| <= 8, A and B unrelated (a transposed
// fragment cannot pass), every (set, dtype) pair a different pattern.
inline int cov_a_val(int set, int dt, int m, int k) {
  return (m * 3 + k * 5 + set * 7 + dt * 2 + (m * k) % 5) % 17 - 8;
}
inline int cov_b_val(int set, int dt, int k, int n) {
  return (k * 7 + n * 11 + set * 13 + dt * 4 + 3 + (k * n) % 7) % 17 - 8;
}

// One (set, dtype) problem: encoded operands, their decoded f32 values and
// the expected tile, which is computed in integers from the intended values
// (not from the decoded ones, so an encoding that fails to round-trip shows).
struct CovProblem {
  int k;
  std::vector<uint32_t> a_enc, b_enc;  // f32 bits / bf16 / e4m3 code per element
  std::vector<float> a_dec, b_dec, d;  // row-major 16xK, Kx16, 16x16
};

static const char* const kCovDtypeNames[3] = {"f32", "bf16", "fp8"};

inline CovProblem cov_problem(int set, int dt) {
  CovProblem p;
  p.k = dt == 0 ? 4 : 32;
  const int K = p.k;
  std::vector<int> a(16 * K), b(K * 16);
  for (int m = 0; m < 16; ++m)
    for (int k = 0; k < K; ++k) a[m * K + k] = cov_a_val(set, dt, m, k);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < 16; ++n) b[k * 16 + n] = cov_b_val(set, dt, k, n);
  auto encode = [dt](int v, uint32_t* enc, float* dec) {
    const float f = (float)v;
    if (dt == 0) {
      *enc = f32_bits(f);
      *dec = f;
    } else if (dt == 1) {
      const uint16_t h = to_bf16(f);
      *enc = h;
      *dec = from_bf16(h);
    } else {
      const uint8_t q = encode_e4m3fn_nearest(f);
      *enc = q;
      *dec = decode_e4m3fn(q);
    }
  };
  p.a_enc.resize(16 * K);
  p.a_dec.resize(16 * K);
  p.b_enc.resize(K * 16);
  p.b_dec.resize(K * 16);
  for (int i = 0; i < 16 * K; ++i) encode(a[i], &p.a_enc[i], &p.a_dec[i]);
  for (int i = 0; i < K * 16; ++i) encode(b[i], &p.b_enc[i], &p.b_dec[i]);
  p.d.resize(256);
  for (int m = 0; m < 16; ++m)
    for (int n = 0; n < 16; ++n) {
      int acc = 0;
      for (int k = 0; k < K; ++k) acc += a[m * K + k] * b[k * 16 + n];
      p.d[m * 16 + n] = (float)acc;
    }
  return p;
}

// Pack every set into per-lane fragment records for the kernel:
// kCovSets x 64 lanes x kCovRecWords.
inline std::vector<uint32_t> cov_build_table() {
  std::vector<uint32_t> tab((size_t)kCovSets * 64 * kCovRecWords, 0u);
  for (int s = 0; s < kCovSets; ++s) {
    CovProblem pr[3] = {cov_problem(s, 0), cov_problem(s, 1), cov_problem(s, 2)};
    for (int l = 0; l < 64; ++l) {
      CovLaneRec rec;
      std::memset(&rec, 0, sizeof(rec));
      const int lo = l & 15, hi = l >> 4;
      rec.f32_a = pr[0].a_enc[lo * 4 + hi];
      rec.f32_b = pr[0].b_enc[hi * 16 + lo];
      for (int i = 0; i < 8; ++i) {
        const int k = hi * 8 + i;
        rec.bf16_a[i / 2] |= pr[1].a_enc[lo * 32 + k] << (16 * (i & 1));
        rec.bf16_b[i / 2] |= pr[1].b_enc[k * 16 + lo] << (16 * (i & 1));
        rec.fp8_a[i / 4] |= pr[2].a_enc[lo * 32 + k] << (8 * (i & 3));
        rec.fp8_b[i / 4] |= pr[2].b_enc[k * 16 + lo] << (8 * (i & 3));
      }
      for (int t = 0; t < 3; ++t)
        for (int r = 0; r < 4; ++r)
          rec.exp[t][r] = f32_bits(pr[t].d[(hi * 4 + r) * 16 + lo]);
      std::memcpy(&tab[(size_t)(s * 64 + l) * kCovRecWords], &rec, sizeof(rec));
    }
  }
  return tab;
}

// ---------------------------------------------------------------------------
// MX block-scaled problems; the formats, the fragment layout and the
// exactness argument are documented on the MX kernels in gpu_validator.hip.
// ---------------------------------------------------------------------------

constexpr int kMxFormats = 5;
constexpr int kMxSets = 5;
constexpr int kMxSpanBoundLog2 = 20;

struct MxFormat {
  const char* name;
  int bits, ebits, mbits, bias;
  int unit;      // alphabet values are mags[i] * 2^unit
  int n_mags;
  int mags[16];  // both signs of each are used
  bool zero;     // plus zero
};

// Alphabets: both signs, every mantissa bit pattern, at least three exponent
// values, magnitudes small enough for the span bound.  e2m1: all 15 values.
static const MxFormat kMxFmt[kMxFormats] = {
    {"e4m3", 8, 4, 3, 7, -3, 13, {1, 2, 3, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16}, false},
    {"e5m2", 8, 5, 2, 15, -2, 11, {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14}, false},
    {"e2m3", 6, 2, 3, 1, -3, 16,
     {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, false},
    {"e3m2", 6, 3, 2, 3, -4, 12, {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16}, false},
    {"e2m1", 4, 2, 1, 1, -1, 7, {1, 2, 3, 4, 6, 8, 12}, true},
};

// A code as (-1)^sign * mant * 2^exp; NaN / Inf codes are not finite.
struct MxParts {
  bool finite;
  int sign, mant, exp;
};

inline MxParts mx_decode_parts(int fmt, unsigned code) {
  const MxFormat& f = kMxFmt[fmt];
  const int e = (code >> f.mbits) & ((1 << f.ebits) - 1);
  const int m = code & ((1 << f.mbits) - 1);
  MxParts p{true, (int)((code >> (f.bits - 1)) & 1u), 0, 0};
  if (fmt == 0 && e == 15 && m == 7) p.finite = false;  // e4m3 NaN
  if (fmt == 1 && e == 31) p.finite = false;            // e5m2 Inf / NaN
  if (e == 0) {
    p.mant = m;  // subnormal
    p.exp = 1 - f.bias - f.mbits;
  } else {
    p.mant = (1 << f.mbits) + m;
    p.exp = e - f.bias - f.mbits;
  }
  return p;
}

inline double mx_decode(int fmt, unsigned code) {
  const MxParts p = mx_decode_parts(fmt, code);
  const double v = std::ldexp((double)p.mant, p.exp);
  return p.sign ? -v : v;
}

// Exact encoder of n * 2^unit: throws when no finite code has that value.
inline uint8_t mx_encode_exact(int fmt, int n, int unit) {
  if (n == 0) return 0;
  const int mag = n < 0 ? -n : n;
  for (unsigned code = 0; code < (1u << kMxFmt[fmt].bits); ++code) {
    const MxParts p = mx_decode_parts(fmt, code);
    if (!p.finite || p.mant == 0 || p.sign != (n < 0)) continue;
    const int d = p.exp - unit;
    if (d >= 0 ? (d < 24 && (p.mant << d) == mag)
               : (-d < 24 && (mag << -d) == p.mant))
      return (uint8_t)code;
  }
  throw std::domain_error(std::string("mx_encode_exact: ") + kMxFmt[fmt].name +
                          " cannot represent " + std::to_string(n) + " * 2^" +
                          std::to_string(unit));
}

// E8M0: 2^(code - 127); 0xFF is NaN and never produced.
inline uint8_t mx_encode_e8m0(int exp) {
  if (exp < -127 || exp > 127)
    throw std::domain_error("mx_encode_e8m0: 2^" + std::to_string(exp) +
                            " has no E8M0 code");
  return (uint8_t)(exp + 127);
}
inline double mx_decode_e8m0(uint8_t code) {
  return std::ldexp(1.0, (int)code - 127);
}

// op_sel byte of the scale VGPR, per set: A and B use different bytes
constexpr int mx_sel_a(int set) { return set & 3; }
constexpr int mx_sel_b(int set) { return set == 0 ? 0 : 1 + (set % 3); }
// scale exponents per set are base + one of three offsets: set 0 uniform, 1
// and 2 near one, 3 far apart, 4 a wider spread that takes S/q near the bound
static const int kMxScaleBaseA[kMxSets] = {0, -1, 2, 20, -2};
static const int kMxScaleBaseB[kMxSets] = {0, 0, -3, -21, -1};
static const int kMxScaleSpread[kMxSets][3] = {
    {0, 0, 0}, {0, 1, 2}, {0, 1, 2}, {0, 1, 2}, {0, 1, 3}};

struct MxProblem {
  int set, fa, fb, shape;  // shape 0: 16x16x128, 1: 32x32x64
  int m, n, k, kblocks, sel_a, sel_b;
  std::vector<uint8_t> a_codes, b_codes;    // row-major m x k, k x n
  std::vector<uint8_t> a_scales, b_scales;  // row-major m x kblocks, kblocks x n
  std::vector<float> d;                     // expected, row-major m x n
  double log2_span;                         // achieved log2(S / q)
  std::vector<uint32_t> a_words, b_words;   // 64 lanes x 8 operand words
  std::vector<uint32_t> a_scale_words, b_scale_words;  // 64 lanes
};

inline const char* mx_shape_name(int shape) {
  return shape == 0 ? "16x16x128" : "32x32x64";
}

// K index of element j of a lane in lane group g (see the layout comment)
inline int mx_lane_k(int bits, int K, int g, int j) {
  return bits == 8 ? (K / 2) * (j >> 4) + 16 * g + (j & 15) : 32 * g + j;
}

// One lane's 32 elements of row / col `codes` (K elements, `stride` apart):
// element j at bits [w*j, w*j + w) of 8 words
inline void mx_pack_lane(int bits, int K, int g, const uint8_t* codes,
                         size_t stride, uint32_t* words) {
  for (int i = 0; i < 8; ++i) words[i] = 0;
  for (int j = 0; j < 32; ++j) {
    const uint32_t c = codes[mx_lane_k(bits, K, g, j) * stride];
    const int pos = j * bits, w = pos >> 5, off = pos & 31;
    words[w] |= c << off;
    if (off + bits > 32) words[w + 1] |= c >> (32 - off);
  }
}

inline int mx_ctz(int64_t v) {
  int z = 0;
  while ((v & 1) == 0) {
    v >>= 1;
    ++z;
  }
  return z;
}

inline MxProblem mx_problem(int set, int fa, int fb, int shape) {
  if (set < 0 || set >= kMxSets)
    throw std::invalid_argument("mx_problem: set out of range");
  if (fa < 0 || fa >= kMxFormats || fb < 0 || fb >= kMxFormats)
    throw std::invalid_argument("mx_problem: unknown format");
  if (shape != 0 && shape != 1)
    throw std::invalid_argument("mx_problem: unknown shape");
  MxProblem p;
  p.set = set;
  p.fa = fa;
  p.fb = fb;
  p.shape = shape;
  p.m = p.n = shape == 0 ? 16 : 32;
  p.k = shape == 0 ? 128 : 64;
  p.kblocks = p.k / 32;
  p.sel_a = mx_sel_a(set);
  p.sel_b = mx_sel_b(set);
  const int M = p.m, N = p.n, K = p.k, KB = p.kblocks;

  auto alphabet = [](int fmt) {
    const MxFormat& f = kMxFmt[fmt];
    std::vector<int> v;
    for (int i = 0; i < f.n_mags; ++i) {
      v.push_back(f.mags[i]);
      v.push_back(-f.mags[i]);
    }
    if (f.zero) v.push_back(0);
    return v;
  };
  const std::vector<int> al_a = alphabet(fa), al_b = alphabet(fb);
  const int ua = kMxFmt[fa].unit, ub = kMxFmt[fb].unit;

  // intended values (integers in units of 2^ua, 2^ub) and scale exponents;
  // A and B are unrelated patterns and every (set, pair, shape) differs
  std::vector<int> a(M * K), b(K * N), sa(M * KB), sb(KB * N);
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < K; ++k)
      a[m * K + k] = al_a[(m * 3 + k * 5 + set * 7 + fa * 2 + fb * 3 +
                           shape * 11 + (m * k) % 5) % (int)al_a.size()];
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n)
      b[k * N + n] = al_b[(k * 7 + n * 11 + set * 13 + fb * 4 + fa * 5 +
                           shape * 3 + 3 + (k * n) % 7) % (int)al_b.size()];
  // neighbouring rows / cols and neighbouring kblocks get different scales
  // (set 0 is uniform: it checks the operand maps on their own)
  for (int m = 0; m < M; ++m)
    for (int kb = 0; kb < KB; ++kb)
      sa[m * KB + kb] =
          kMxScaleBaseA[set] + kMxScaleSpread[set][(m + 2 * kb + set) % 3];
  for (int kb = 0; kb < KB; ++kb)
    for (int n = 0; n < N; ++n)
      sb[kb * N + n] =
          kMxScaleBaseB[set] + kMxScaleSpread[set][(2 * n + kb + set + 1) % 3];

  // encode; an operand that does not round-trip throws
  p.a_codes.resize(M * K);
  p.b_codes.resize(K * N);
  p.a_scales.resize(M * KB);
  p.b_scales.resize(KB * N);
  for (int i = 0; i < M * K; ++i) {
    p.a_codes[i] = mx_encode_exact(fa, a[i], ua);
    if (mx_decode(fa, p.a_codes[i]) != std::ldexp((double)a[i], ua))
      throw std::domain_error("mx_problem: A operand does not round-trip");
  }
  for (int i = 0; i < K * N; ++i) {
    p.b_codes[i] = mx_encode_exact(fb, b[i], ub);
    if (mx_decode(fb, p.b_codes[i]) != std::ldexp((double)b[i], ub))
      throw std::domain_error("mx_problem: B operand does not round-trip");
  }
  for (int i = 0; i < M * KB; ++i) {
    p.a_scales[i] = mx_encode_e8m0(sa[i]);
    if (mx_decode_e8m0(p.a_scales[i]) != std::ldexp(1.0, sa[i]))
      throw std::domain_error("mx_problem: A scale does not round-trip");
  }
  for (int i = 0; i < KB * N; ++i) {
    p.b_scales[i] = mx_encode_e8m0(sb[i]);
    if (mx_decode_e8m0(p.b_scales[i]) != std::ldexp(1.0, sb[i]))
      throw std::domain_error("mx_problem: B scale does not round-trip");
  }

  // expected tile in 64-bit fixed point with unit 2^e_min, from the intended
  // integers and exponents (never from decoded floats)
  int e_min = INT32_MAX;
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n)
      for (int kb = 0; kb < KB; ++kb)
        e_min = std::min(e_min, ua + ub + sa[m * KB + kb] + sb[kb * N + n]);
  int q_exp = INT32_MAX;  // log2 of q
  int64_t s_max = 0;      // S in units of 2^e_min
  p.d.resize(M * N);
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) {
      int64_t acc = 0, abs_sum = 0;
      for (int k = 0; k < K; ++k) {
        const int64_t prod = (int64_t)a[m * K + k] * b[k * N + n];
        if (prod == 0) continue;
        const int e = ua + ub + sa[m * KB + k / 32] + sb[(k / 32) * N + n];
        if (e - e_min > 30) throw std::domain_error("mx_problem: scale spread");
        acc += prod * ((int64_t)1 << (e - e_min));
        abs_sum += (prod < 0 ? -prod : prod) * ((int64_t)1 << (e - e_min));
        q_exp = std::min(q_exp, e + mx_ctz(prod));
      }
      s_max = std::max(s_max, abs_sum);
      const double want = std::ldexp((double)acc, e_min);
      p.d[m * N + n] = (float)want;
      if ((double)p.d[m * N + n] != want)
        throw std::domain_error("mx_problem: expected value is not an f32");
    }
  if (s_max == 0) throw std::domain_error("mx_problem: empty tile");
  p.log2_span = std::log2((double)s_max) + (double)(e_min - q_exp);
  if (p.log2_span > (double)kMxSpanBoundLog2)
    throw std::domain_error(
        std::string("mx_problem: S/q = 2^") + std::to_string(p.log2_span) +
        " exceeds the exactness bound for " + kMxFmt[fa].name + " x " +
        kMxFmt[fb].name + " " + mx_shape_name(shape) + " set " +
        std::to_string(set));

  // per-lane fragments; the three scale bytes op_sel does not pick hold valid
  // scales that would give another answer
  p.a_words.resize(64 * 8);
  p.b_words.resize(64 * 8);
  p.a_scale_words.resize(64);
  p.b_scale_words.resize(64);
  for (int l = 0; l < 64; ++l) {
    const int rc = l % M, kb = l / M;
    mx_pack_lane(kMxFmt[fa].bits, K, kb, &p.a_codes[rc * K], 1,
                 &p.a_words[l * 8]);
    mx_pack_lane(kMxFmt[fb].bits, K, kb, &p.b_codes[rc], (size_t)N,
                 &p.b_words[l * 8]);
    const uint32_t ca = p.a_scales[rc * KB + kb], cb = p.b_scales[kb * N + rc];
    uint32_t wa = 0, wb = 0;
    for (int i = 0; i < 4; ++i) {
      wa |= (i == p.sel_a ? ca : ca + 3 + i) << (8 * i);
      wb |= (i == p.sel_b ? cb : cb + 3 + i) << (8 * i);
    }
    p.a_scale_words[l] = wa;
    p.b_scale_words[l] = wb;
  }
  return p;
}

// The sweep's problems per set: five same-format pairs and three mixed pairs
// (cbsz != blgp) on 16x16x128, then e2m1 and e4m3 on 32x32x64.
constexpr int kMxProbs = 10;
constexpr int kMxProbFa[kMxProbs] = {0, 1, 2, 3, 4, 0, 4, 3, 4, 0};
constexpr int kMxProbFb[kMxProbs] = {0, 1, 2, 3, 4, 4, 2, 1, 4, 0};
constexpr int kMxProbShape[kMxProbs] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1};
constexpr int kMxProbBit[kMxProbs] = {0, 1, 2, 3, 4, 5, 5, 5, 6, 6};

// Per-lane records: the single tile reads a[8] b[8] sa sb, the sweep the same
// followed by exp[16] (16x16 problems use exp[0..3]).
constexpr int kMxTileRecWords = 18;
constexpr int kMxRecWords = 34;

// Accumulator registers per lane, and where register r of lane l sits in the
// row-major m x n tile (the dtype-independent C/D maps).
inline int mx_lane_regs(int shape) { return shape == 0 ? 4 : 16; }
inline int mx_d_index(int shape, int l, int r) {
  return shape == 0
             ? ((l >> 4) * 4 + r) * 16 + (l & 15)
             : ((r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31);
}

// the kMxTileRecWords operand and scale words of lane l
inline void mx_lane_operands(const MxProblem& p, int l, uint32_t* r) {
  std::memcpy(r, &p.a_words[l * 8], 32);
  std::memcpy(r + 8, &p.b_words[l * 8], 32);
  r[16] = p.a_scale_words[l];
  r[17] = p.b_scale_words[l];
}

// 64 lanes x kMxTileRecWords
inline std::vector<uint32_t> mx_tile_record(const MxProblem& p) {
  std::vector<uint32_t> rec((size_t)64 * kMxTileRecWords);
  for (int l = 0; l < 64; ++l)
    mx_lane_operands(p, l, &rec[(size_t)l * kMxTileRecWords]);
  return rec;
}

// kMxSets x kMxProbs x 64 lanes x kMxRecWords
inline std::vector<uint32_t> mx_build_table() {
  std::vector<uint32_t> tab((size_t)kMxSets * kMxProbs * 64 * kMxRecWords, 0u);
  for (int s = 0; s < kMxSets; ++s)
    for (int i = 0; i < kMxProbs; ++i) {
      const MxProblem p =
          mx_problem(s, kMxProbFa[i], kMxProbFb[i], kMxProbShape[i]);
      for (int l = 0; l < 64; ++l) {
        uint32_t* r = &tab[(size_t)((s * kMxProbs + i) * 64 + l) * kMxRecWords];
        mx_lane_operands(p, l, r);
        for (int q = 0; q < mx_lane_regs(p.shape); ++q)
          r[18 + q] = f32_bits(p.d[mx_d_index(p.shape, l, q)]);
      }
    }
  return tab;
}

// Burn-in seed: 64 lanes x {a[8], b[8]} of non-zero alphabet codes of format
// f, then the scale word (2^-20 in every byte).
inline std::vector<uint32_t> mx_burn_seed(int f) {
  const MxFormat& mf = kMxFmt[f];
  std::vector<uint32_t> seed(64 * 16 + 1);
  for (int l = 0; l < 64; ++l)
    for (int h = 0; h < 2; ++h) {
      uint8_t codes[128];  // one row: only the lane's own 32 are read
      for (int j = 0; j < 128; ++j) {
        const int mag = mf.mags[(l * 7 + j * 3 + h * 5) % mf.n_mags];
        codes[j] = mx_encode_exact(f, (l + j + h) % 3 == 0 ? -mag : mag, mf.unit);
      }
      mx_pack_lane(mf.bits, 128, l >> 4, codes, 1, &seed[l * 16 + h * 8]);
    }
  seed[64 * 16] = 0x01010101u * mx_encode_e8m0(-20);
  return seed;
}

// ---------------------------------------------------------------------------
// HBM pattern (hash or checker) of a logical 64-bit word index: the one
// definition shared by the kernels and the host reference.
// ---------------------------------------------------------------------------

constexpr int kHbmPatternHash = 0, kHbmPatternChecker = 1;

VALIDATOR_HD inline uint64_t hbm_pattern_value(int pattern, uint64_t seed,
                                               uint64_t i) {
  if (pattern == kHbmPatternChecker)
    return (i & 1ull) ? 0x5555555555555555ull : 0xAAAAAAAAAAAAAAAAull;
  uint64_t z = i + seed * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---------------------------------------------------------------------------
// Cross-XCD check: the words of the hand-off slabs and the operands of the
// atomics sweep, shared by the kernels and the host.
// ---------------------------------------------------------------------------

constexpr uint64_t kXfStaticKey = 0x5354415449435F58ull;
constexpr uint64_t kXfAtomKey1 = 0x41544F4D31ull, kXfAtomKey2 = 0x41544F4D32ull,
                   kXfAtomKey3 = 0x41544F4D33ull;
constexpr int64_t kXfF32Bound = 1ll << 23;

VALIDATOR_HD inline uint64_t xf_static_word(uint64_t seed, uint64_t idx) {
  return hbm_pattern_value(kHbmPatternHash, seed ^ kXfStaticKey, idx);
}
// round -1 is the initial upload
VALIDATOR_HD inline uint64_t xf_payload_word(uint64_t seed, int64_t round,
                                             uint64_t idx) {
  return hbm_pattern_value(kHbmPatternHash, seed + (uint64_t)round, idx);
}
VALIDATOR_HD inline uint64_t xf_line_index(uint32_t blocks, uint32_t slab_lines,
                                           uint32_t rep, uint32_t block,
                                           uint32_t line) {
  return ((uint64_t)rep * blocks + block) * slab_lines + line;
}

struct XfAtomVals {
  uint64_t add64, mm;
  uint32_t add32, x, o, a;
  int addf;  // integer in [-8, 8], added as f32
};

// The one generator shared by the kernel and the host: what thread `id` adds
// in repetition `rep`.  or/and operands are mostly neutral so the cells do
// not saturate.
VALIDATOR_HD inline XfAtomVals xf_atom_vals(uint64_t seed, uint64_t id,
                                            uint32_t rep) {
  const uint64_t n = id * 64 + rep;
  const uint64_t h1 = hbm_pattern_value(kHbmPatternHash, seed ^ kXfAtomKey1, n);
  const uint64_t h2 = hbm_pattern_value(kHbmPatternHash, seed ^ kXfAtomKey2, n);
  const uint64_t h3 = hbm_pattern_value(kHbmPatternHash, seed ^ kXfAtomKey3, n);
  XfAtomVals v;
  v.add32 = (uint32_t)h1;
  v.addf = (int)((h1 >> 32) % 17) - 8;
  v.add64 = h2;
  v.mm = h3;
  v.x = (uint32_t)(h1 >> 20);
  v.o = ((h2 >> 40) & 1023) == 0 ? 1u << ((h2 >> 8) & 31) : 0u;
  v.a = ((h2 >> 50) & 1023) == 0 ? ~(1u << ((h2 >> 16) & 31)) : ~0u;
  return v;
}

// Expected cell contents after `threads` threads ran `reps` repetitions.
struct XfAtomExpected {
  std::vector<uint32_t> add32, x, o, a;
  std::vector<uint64_t> add64, max64, min64;
  std::vector<int64_t> addf;
};

inline XfAtomExpected xf_atom_expected(uint64_t seed, uint64_t threads, int reps,
                                       int cells) {
  XfAtomExpected e;
  e.add32.assign(cells, 0u);
  e.x.assign(cells, 0u);
  e.o.assign(cells, 0u);
  e.a.assign(cells, ~0u);
  e.add64.assign(cells, 0ull);
  e.max64.assign(cells, 0ull);
  e.min64.assign(cells, ~0ull);
  e.addf.assign(cells, 0);
  std::vector<int64_t> mag(cells, 0);
  for (uint64_t id = 0; id < threads; ++id)
    for (int rep = 0; rep < reps; ++rep) {
      const size_t c = (size_t)((id + (uint64_t)rep) % (uint64_t)cells);
      const XfAtomVals v = xf_atom_vals(seed, id, (uint32_t)rep);
      e.add32[c] += v.add32;
      e.add64[c] += v.add64;
      e.addf[c] += v.addf;
      mag[c] += v.addf < 0 ? -v.addf : v.addf;
      e.max64[c] = std::max(e.max64[c], v.mm);
      e.min64[c] = std::min(e.min64[c], v.mm);
      e.x[c] ^= v.x;
      e.o[c] |= v.o;
      e.a[c] &= v.a;
    }
  // enforced, not assumed: below 2^23 every partial sum is an exact f32
  for (int c = 0; c < cells; ++c)
    if (mag[c] > kXfF32Bound)
      throw std::invalid_argument(
          "xcd_fabric: the f32 operands of cell " + std::to_string(c) +
          " sum to a magnitude of " + std::to_string(mag[c]) +
          " > 2^23; use more cells or fewer reps");
  return e;
}

// ---------------------------------------------------------------------------
// What the host does with the tables a launch leaves behind: argument range
// checks, the per-unit tally of a whole-device sweep, the digest grouping of
// the vector-ALU sweep and the kept / dropped split of a capped record log.
// ---------------------------------------------------------------------------

constexpr int kCovKeys = 4096;           // placement keys: 4 XCC bits + 8 HW_ID bits
constexpr int kCovSlots = kCovKeys * 4;  // x 4 SIMDs

// the range checks whose message is the same in every check
inline void require_range(const std::string& who, const char* name, long value,
                          long lo, long hi) {
  if (value < lo || value > hi)
    throw std::invalid_argument(who + ": " + name + " must be in [" +
                                std::to_string(lo) + ", " + std::to_string(hi) + "]");
}
inline void require_poison_key(const std::string& who, int poison_key) {
  if (poison_key < -1 || poison_key >= kCovKeys)
    throw std::invalid_argument(who + ": poison_key out of range");
}

// One unit that ran at least one wave (simds == 4) or workgroup (simds == 1).
struct CovUnit {
  int key, simd;
  uint32_t waves, fail_mask, hw_id_raw, xcc_id_raw;
};
struct CovTally {
  int cus_covered = 0, slots_covered = 0, failed_slots = 0;
  long waves_run = 0;
  bool complete = false;  // every CU of the device, and every SIMD of each
  std::vector<CovUnit> units;
};

// `planes` is waves | fail | hw_id | xcc_id, each kCovKeys * simds words, entry
// key * simds + simd.  The whole-device sweeps keep one entry per SIMD
// (simds == 4), the LDS check one per CU (simds == 1).
inline CovTally cov_tally(const uint32_t* planes, int cus, int simds) {
  const int n = kCovKeys * simds;
  const uint32_t* waves = planes;
  CovTally t;
  for (int key = 0; key < kCovKeys; ++key) {
    bool any = false;
    for (int s = 0; s < simds; ++s) {
      const int slot = key * simds + s;
      if (waves[slot] == 0) continue;
      any = true;
      ++t.slots_covered;
      t.units.push_back({key, s, waves[slot], planes[n + slot],
                         planes[2 * n + slot], planes[3 * n + slot]});
      t.waves_run += waves[slot];
      t.failed_slots += planes[n + slot] != 0;
    }
    t.cus_covered += any;
  }
  t.complete = t.cus_covered >= cus && t.slots_covered >= simds * cus;
  return t;
}

// Wave records [slot + 1 | digests...] of rec_words words each -> per slot the
// distinct digest tuples in first-seen order.  A first word of 0 (never
// written) or above kCovSlots is skipped.
inline std::vector<std::vector<std::vector<uint64_t>>> valu_group_digests(
    const uint64_t* recs, size_t n_recs, int rec_words) {
  std::vector<std::vector<std::vector<uint64_t>>> by_slot(kCovSlots);
  for (size_t i = 0; i < n_recs; ++i) {
    const uint64_t* wr = recs + i * (size_t)rec_words;
    if (wr[0] == 0 || wr[0] > (uint64_t)kCovSlots) continue;
    std::vector<uint64_t> tuple(wr + 1, wr + rec_words);
    auto& seen = by_slot[wr[0] - 1];
    if (std::find(seen.begin(), seen.end(), tuple) == seen.end()) seen.push_back(tuple);
  }
  return by_slot;
}

// records a log of `cap` slots holds after `claims` claims; the rest were dropped
inline size_t record_log_kept(uint64_t claims, size_t cap) {
  return (size_t)std::min<uint64_t>(claims, (uint64_t)cap);
}

// ---------------------------------------------------------------------------
// LDS data-integrity check: its generators live in a header of their own.
// ---------------------------------------------------------------------------

#include "lds_problems.hpp"

// ---------------------------------------------------------------------------
// Host-link data-integrity check: likewise.
// ---------------------------------------------------------------------------

#include "hostlink_problems.hpp"

// ---------------------------------------------------------------------------
// Vector-ALU check: likewise.
// ---------------------------------------------------------------------------

#include "valu_problems.hpp"
