// valu_problems.hpp — the exact problems of the vector-ALU check
// (valu_coverage_kernel in gpu_validator.hip): the one table of instructions,
// the generator of their operands and the host reference of their results.
//
// Included from validator_problems.hpp (it needs hbm_pattern_value and the MX
// code tables); plain C++17, host only, no HIP include, so
// tests/native/valu_problems_selftest.cpp drives it stand-alone under
// AddressSanitizer + UBSan.
//
// Every op takes three 64-bit operands a, b, c per lane and gives one 64-bit
// result per lane; narrower operands sit in the low word(s), packed pairs in
// (low word, high word).  One record of the device table is
//   a_lo a_hi b_lo b_hi c_lo c_hi expected_lo expected_hi
// for one (op, set, lane).  Values come from splitmix64 and are then shaped
// per op; valu_check_constraints throws when a shaped value or a result
// breaks a stated condition.  No NaN or infinity is ever an input or an
// expected result.
//
// The reference assumes what hipcc's default mode gives the device: round to
// nearest even, subnormals kept for f32, f16 and f64.

#pragma once

constexpr int kValuSets = 4;                  // operand sets per op
constexpr int kValuRecWords = 8;
constexpr int kValuGroups = 7;
constexpr int kValuGroupF32 = 0, kValuGroupF64 = 1, kValuGroupF16 = 2,
              kValuGroupInt = 3, kValuGroupConvert = 4, kValuGroupCrosslane = 5,
              kValuGroupConsensus = 6;
static const char* const kValuGroupNames[kValuGroups] = {
    "f32", "f64", "f16", "int", "convert", "crosslane", "consensus"};
constexpr int kValuMaxRecords = 64;
constexpr uint64_t kValuKey = 0x56414C555F4F5053ull;  // "VALU_OPS"

// What an op computes.  The device's valu_eval<KIND, IMM> and valu_ref_lane /
// valu_ref_wave below are the two implementations of this list.
enum ValuKind : int {
  // f32
  kVkFmaF32, kVkAddF32, kVkMulF32, kVkPkFmaF32, kVkPkAddF32, kVkPkMulF32,
  kVkMinF32, kVkMaxF32, kVkMed3F32, kVkLdexpF32, kVkFrexpMantF32, kVkRndneF32,
  // f64
  kVkFmaF64, kVkAddF64, kVkMulF64, kVkLdexpF64,
  // f16
  kVkPkFmaF16, kVkPkAddF16, kVkPkMulF16, kVkDot2F16, kVkDot2Bf16,
  // int
  kVkMadU64U32, kVkMulHiU32, kVkMulLoU32, kVkMulI24, kVkAddU64, kVkSubU64,
  kVkLshlB32, kVkLshrB32, kVkAshrI32, kVkLshlB64, kVkLshrB64, kVkAshrI64,
  kVkBfeU32, kVkBfiB32, kVkPermB32, kVkAlignbitB32, kVkSadU8, kVkBcntU32,
  kVkFfbhU32, kVkBfrevB32, kVkBitop3B32, kVkDot4I8, kVkDot4U8, kVkCmpSelect,
  // convert
  kVkCvtF16F32, kVkCvtPkBf16F32, kVkCvtI32F32, kVkCvtU32F32, kVkCvtF32I32,
  kVkCvtF32U32, kVkCvtPkFp8F32, kVkCvtPkBf8F32, kVkCvtF32Fp8, kVkCvtF32Bf8,
  kVkCvtScalePkF32Fp4, kVkCvtScalePkFp4F32,
  // crosslane
  kVkDpp, kVkReadlane, kVkReadfirstlane, kVkPermlane16Swap, kVkPermlane32Swap,
  kVkMbcnt, kVkCmpMask,
  // consensus
  kVkExpF32, kVkLogF32, kVkRcpF32, kVkRsqF32, kVkSqrtF32, kVkSinF32, kVkCosF32,
  kVkRcpF64, kVkRsqF64, kVkCvtSrFp8F32, kVkPrngB32,
};

// DPP ops: IMM = dpp_ctrl | variant << 12.  Variant 0: row_mask 0xF,
// bank_mask 0xF, bound_ctrl off.  Variant 1: row_mask 0xD, bank_mask 0x7,
// bound_ctrl on, so `old` shows in row 1 and in bank 3 of every row.
constexpr int kValuDppV1 = 1 << 12;
constexpr int kValuDppRowMask[2] = {0xF, 0xD};
constexpr int kValuDppBankMask[2] = {0xF, 0x7};
constexpr int kValuReadLanes[4] = {5, 23, 40, 62};

struct ValuOp {
  const char* name;  // the instruction, plus its immediate where one varies
  int group, kind, imm;
};

#define VALU_DPP2(X, text, ctrl)                                        \
  X("v_mov_b32_dpp " text, kValuGroupCrosslane, kVkDpp, (ctrl))         \
  X("v_mov_b32_dpp " text " row_mask:0xd bank_mask:0x7 bound_ctrl:1",   \
    kValuGroupCrosslane, kVkDpp, (ctrl) | kValuDppV1)

// X(name, group, kind, imm): the one table shared by the kernel, the
// reference, the mismatch records and valu_probe.
#define VALU_OPS(X)                                                            \
  X("v_fma_f32", kValuGroupF32, kVkFmaF32, 0)                                  \
  X("v_add_f32", kValuGroupF32, kVkAddF32, 0)                                  \
  X("v_mul_f32", kValuGroupF32, kVkMulF32, 0)                                  \
  X("v_pk_fma_f32", kValuGroupF32, kVkPkFmaF32, 0)                             \
  X("v_pk_add_f32", kValuGroupF32, kVkPkAddF32, 0)                             \
  X("v_pk_mul_f32", kValuGroupF32, kVkPkMulF32, 0)                             \
  X("v_min_f32", kValuGroupF32, kVkMinF32, 0)                                  \
  X("v_max_f32", kValuGroupF32, kVkMaxF32, 0)                                  \
  X("v_med3_f32", kValuGroupF32, kVkMed3F32, 0)                                \
  X("v_ldexp_f32", kValuGroupF32, kVkLdexpF32, 0)                              \
  X("v_frexp_mant_f32", kValuGroupF32, kVkFrexpMantF32, 0)                     \
  X("v_rndne_f32", kValuGroupF32, kVkRndneF32, 0)                              \
  X("v_fma_f64", kValuGroupF64, kVkFmaF64, 0)                                  \
  X("v_add_f64", kValuGroupF64, kVkAddF64, 0)                                  \
  X("v_mul_f64", kValuGroupF64, kVkMulF64, 0)                                  \
  X("v_ldexp_f64", kValuGroupF64, kVkLdexpF64, 0)                              \
  X("v_pk_fma_f16", kValuGroupF16, kVkPkFmaF16, 0)                             \
  X("v_pk_add_f16", kValuGroupF16, kVkPkAddF16, 0)                             \
  X("v_pk_mul_f16", kValuGroupF16, kVkPkMulF16, 0)                             \
  X("v_dot2c_f32_f16", kValuGroupF16, kVkDot2F16, 0)                           \
  X("v_dot2c_f32_bf16", kValuGroupF16, kVkDot2Bf16, 0)                         \
  X("v_mad_u64_u32", kValuGroupInt, kVkMadU64U32, 0)                           \
  X("v_mul_hi_u32", kValuGroupInt, kVkMulHiU32, 0)                             \
  X("v_mul_lo_u32", kValuGroupInt, kVkMulLoU32, 0)                             \
  X("v_mul_i32_i24", kValuGroupInt, kVkMulI24, 0)                              \
  X("v_add_co_u32+v_addc_co_u32", kValuGroupInt, kVkAddU64, 0)                 \
  X("v_sub_co_u32+v_subb_co_u32", kValuGroupInt, kVkSubU64, 0)                 \
  X("v_lshlrev_b32", kValuGroupInt, kVkLshlB32, 0)                             \
  X("v_lshrrev_b32", kValuGroupInt, kVkLshrB32, 0)                             \
  X("v_ashrrev_i32", kValuGroupInt, kVkAshrI32, 0)                             \
  X("v_lshlrev_b64", kValuGroupInt, kVkLshlB64, 0)                             \
  X("v_lshrrev_b64", kValuGroupInt, kVkLshrB64, 0)                             \
  X("v_ashrrev_i64", kValuGroupInt, kVkAshrI64, 0)                             \
  X("v_bfe_u32", kValuGroupInt, kVkBfeU32, 0)                                  \
  X("v_bfi_b32", kValuGroupInt, kVkBfiB32, 0)                                  \
  X("v_perm_b32", kValuGroupInt, kVkPermB32, 0)                                \
  X("v_alignbit_b32", kValuGroupInt, kVkAlignbitB32, 0)                        \
  X("v_sad_u8", kValuGroupInt, kVkSadU8, 0)                                    \
  X("v_bcnt_u32_b32", kValuGroupInt, kVkBcntU32, 0)                            \
  X("v_ffbh_u32", kValuGroupInt, kVkFfbhU32, 0)                                \
  X("v_bfrev_b32", kValuGroupInt, kVkBfrevB32, 0)                              \
  X("v_bitop3_b32 bitop3:0x96", kValuGroupInt, kVkBitop3B32, 0x96)             \
  X("v_bitop3_b32 bitop3:0xe8", kValuGroupInt, kVkBitop3B32, 0xE8)             \
  X("v_bitop3_b32 bitop3:0xca", kValuGroupInt, kVkBitop3B32, 0xCA)             \
  X("v_bitop3_b32 bitop3:0x1b", kValuGroupInt, kVkBitop3B32, 0x1B)             \
  X("v_dot4_i32_i8", kValuGroupInt, kVkDot4I8, 0)                              \
  X("v_dot4_u32_u8", kValuGroupInt, kVkDot4U8, 0)                              \
  X("v_cmp_lt_i32+v_cndmask_b32", kValuGroupInt, kVkCmpSelect, 0)              \
  X("v_cvt_f16_f32", kValuGroupConvert, kVkCvtF16F32, 0)                       \
  X("v_cvt_pk_bf16_f32", kValuGroupConvert, kVkCvtPkBf16F32, 0)                \
  X("v_cvt_i32_f32", kValuGroupConvert, kVkCvtI32F32, 0)                       \
  X("v_cvt_u32_f32", kValuGroupConvert, kVkCvtU32F32, 0)                       \
  X("v_cvt_f32_i32", kValuGroupConvert, kVkCvtF32I32, 0)                       \
  X("v_cvt_f32_u32", kValuGroupConvert, kVkCvtF32U32, 0)                       \
  X("v_cvt_pk_fp8_f32 word_sel:0", kValuGroupConvert, kVkCvtPkFp8F32, 0)       \
  X("v_cvt_pk_fp8_f32 word_sel:1", kValuGroupConvert, kVkCvtPkFp8F32, 1)       \
  X("v_cvt_pk_bf8_f32 word_sel:0", kValuGroupConvert, kVkCvtPkBf8F32, 0)       \
  X("v_cvt_pk_bf8_f32 word_sel:1", kValuGroupConvert, kVkCvtPkBf8F32, 1)       \
  X("v_cvt_f32_fp8 byte_sel:0", kValuGroupConvert, kVkCvtF32Fp8, 0)            \
  X("v_cvt_f32_fp8 byte_sel:1", kValuGroupConvert, kVkCvtF32Fp8, 1)            \
  X("v_cvt_f32_fp8 byte_sel:2", kValuGroupConvert, kVkCvtF32Fp8, 2)            \
  X("v_cvt_f32_fp8 byte_sel:3", kValuGroupConvert, kVkCvtF32Fp8, 3)            \
  X("v_cvt_f32_bf8 byte_sel:0", kValuGroupConvert, kVkCvtF32Bf8, 0)            \
  X("v_cvt_f32_bf8 byte_sel:1", kValuGroupConvert, kVkCvtF32Bf8, 1)            \
  X("v_cvt_f32_bf8 byte_sel:2", kValuGroupConvert, kVkCvtF32Bf8, 2)            \
  X("v_cvt_f32_bf8 byte_sel:3", kValuGroupConvert, kVkCvtF32Bf8, 3)            \
  X("v_cvt_scalef32_pk_f32_fp4 byte_sel:0", kValuGroupConvert,                 \
    kVkCvtScalePkF32Fp4, 0)                                                    \
  X("v_cvt_scalef32_pk_f32_fp4 byte_sel:1", kValuGroupConvert,                 \
    kVkCvtScalePkF32Fp4, 1)                                                    \
  X("v_cvt_scalef32_pk_f32_fp4 byte_sel:2", kValuGroupConvert,                 \
    kVkCvtScalePkF32Fp4, 2)                                                    \
  X("v_cvt_scalef32_pk_f32_fp4 byte_sel:3", kValuGroupConvert,                 \
    kVkCvtScalePkF32Fp4, 3)                                                    \
  X("v_cvt_scalef32_pk_fp4_f32 byte_sel:0", kValuGroupConvert,                 \
    kVkCvtScalePkFp4F32, 0)                                                    \
  X("v_cvt_scalef32_pk_fp4_f32 byte_sel:1", kValuGroupConvert,                 \
    kVkCvtScalePkFp4F32, 1)                                                    \
  X("v_cvt_scalef32_pk_fp4_f32 byte_sel:2", kValuGroupConvert,                 \
    kVkCvtScalePkFp4F32, 2)                                                    \
  X("v_cvt_scalef32_pk_fp4_f32 byte_sel:3", kValuGroupConvert,                 \
    kVkCvtScalePkFp4F32, 3)                                                    \
  VALU_DPP2(X, "quad_perm:[1,0,3,2]", 0xB1)                                       \
  VALU_DPP2(X, "quad_perm:[3,3,0,1]", 0x4F)                                       \
  VALU_DPP2(X, "row_shl:1", 0x101)                                                \
  VALU_DPP2(X, "row_shl:15", 0x10F)                                               \
  VALU_DPP2(X, "row_shr:1", 0x111)                                                \
  VALU_DPP2(X, "row_shr:15", 0x11F)                                               \
  VALU_DPP2(X, "row_ror:1", 0x121)                                                \
  VALU_DPP2(X, "row_ror:15", 0x12F)                                               \
  VALU_DPP2(X, "wave_shl:1", 0x130)                                               \
  VALU_DPP2(X, "wave_rol:1", 0x134)                                               \
  VALU_DPP2(X, "wave_shr:1", 0x138)                                               \
  VALU_DPP2(X, "wave_ror:1", 0x13C)                                               \
  VALU_DPP2(X, "row_mirror", 0x140)                                               \
  VALU_DPP2(X, "row_half_mirror", 0x141)                                          \
  VALU_DPP2(X, "row_bcast:15", 0x142)                                             \
  VALU_DPP2(X, "row_bcast:31", 0x143)                                             \
  X("v_readlane_b32", kValuGroupCrosslane, kVkReadlane, 0)                     \
  X("v_readfirstlane_b32", kValuGroupCrosslane, kVkReadfirstlane, 0)           \
  X("v_permlane16_swap_b32", kValuGroupCrosslane, kVkPermlane16Swap, 0)        \
  X("v_permlane32_swap_b32", kValuGroupCrosslane, kVkPermlane32Swap, 0)        \
  X("v_mbcnt_lo_u32_b32+v_mbcnt_hi_u32_b32", kValuGroupCrosslane, kVkMbcnt, 0) \
  X("v_cmp_lt_u32 (64-bit mask)", kValuGroupCrosslane, kVkCmpMask, 0)          \
  X("v_exp_f32", kValuGroupConsensus, kVkExpF32, 0)                            \
  X("v_log_f32", kValuGroupConsensus, kVkLogF32, 0)                            \
  X("v_rcp_f32", kValuGroupConsensus, kVkRcpF32, 0)                            \
  X("v_rsq_f32", kValuGroupConsensus, kVkRsqF32, 0)                            \
  X("v_sqrt_f32", kValuGroupConsensus, kVkSqrtF32, 0)                          \
  X("v_sin_f32", kValuGroupConsensus, kVkSinF32, 0)                            \
  X("v_cos_f32", kValuGroupConsensus, kVkCosF32, 0)                            \
  X("v_rcp_f64", kValuGroupConsensus, kVkRcpF64, 0)                            \
  X("v_rsq_f64", kValuGroupConsensus, kVkRsqF64, 0)                            \
  X("v_cvt_sr_fp8_f32", kValuGroupConsensus, kVkCvtSrFp8F32, 0)                \
  X("v_prng_b32", kValuGroupConsensus, kVkPrngB32, 0)

#define VALU_X_ENTRY(n, g, k, i) {n, g, k, i},
static const ValuOp kValuOpTable[] = {VALU_OPS(VALU_X_ENTRY)};
#undef VALU_X_ENTRY
#define VALU_X_KIND(n, g, k, i) k,
constexpr int kValuOpKind[] = {VALU_OPS(VALU_X_KIND)};
#undef VALU_X_KIND
#define VALU_X_IMM(n, g, k, i) i,
constexpr int kValuOpImm[] = {VALU_OPS(VALU_X_IMM)};
#undef VALU_X_IMM
#define VALU_X_GROUP(n, g, k, i) g,
constexpr int kValuOpGroup[] = {VALU_OPS(VALU_X_GROUP)};
#undef VALU_X_GROUP
constexpr int kValuOps = sizeof(kValuOpKind) / sizeof(int);
constexpr int kValuConsOps = 11;
constexpr int kValuExactOps = kValuOps - kValuConsOps;  // the table's head
static_assert(kValuOpGroup[kValuExactOps - 1] != kValuGroupConsensus &&
                  kValuOpGroup[kValuExactOps] == kValuGroupConsensus,
              "the consensus ops are the last kValuConsOps of VALU_OPS");
// every lane of a wave runs every input of a consensus op: one set's worth
constexpr int kValuConsInputs = 64;
static_assert(kValuConsInputs <= kValuSets * 64, "inputs fit the op's records");

inline int valu_op_index(const std::string& name) {
  for (int i = 0; i < kValuOps; ++i)
    if (name == kValuOpTable[i].name) return i;
  throw std::invalid_argument("valu: unknown op '" + name + "'");
}

// compares one lane makes per repetition, per group
inline uint64_t valu_items_per_lane(int group) {
  uint64_t n = 0;
  for (int i = 0; i < kValuOps; ++i)
    if (kValuOpGroup[i] == group)
      n += group == kValuGroupConsensus ? kValuConsInputs : kValuSets;
  return n;
}
// ... and one wave
inline uint64_t valu_items(int group) { return 64 * valu_items_per_lane(group); }

// ---------------------------------------------------------------------------
// Bit helpers
// ---------------------------------------------------------------------------

inline uint32_t valu_lo(uint64_t v) { return (uint32_t)v; }
inline uint32_t valu_hi(uint64_t v) { return (uint32_t)(v >> 32); }
inline uint64_t valu_pack(uint32_t lo, uint32_t hi) {
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
inline float valu_f32(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline double valu_f64(uint64_t u) {
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}
inline uint64_t valu_f64_bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}
inline bool valu_f32_finite(uint32_t u) { return ((u >> 23) & 0xFFu) != 0xFFu; }
inline bool valu_f64_finite(uint64_t u) { return ((u >> 52) & 0x7FFu) != 0x7FFu; }
inline bool valu_f16_finite(uint32_t h) { return ((h >> 10) & 0x1Fu) != 0x1Fu; }

// A small float format: sign, ebits, mbits, bias; IEEE-like subnormals.  The
// largest finite code's magnitude bits are `max_code` (e4m3fn: 0x7E, its top
// exponent holds values; e2m1: 0x7, no infinity at all).
struct ValuFmt {
  int ebits, mbits, bias;
  uint32_t max_code;
};
constexpr ValuFmt kValuFmtF16 = {5, 10, 15, 0x7BFF};
constexpr ValuFmt kValuFmtBf16 = {8, 7, 127, 0x7F7F};
constexpr ValuFmt kValuFmtE4m3 = {4, 3, 7, 0x7E};
constexpr ValuFmt kValuFmtE5m2 = {5, 2, 15, 0x7B};
constexpr ValuFmt kValuFmtE2m1 = {2, 1, 1, 0x7};

// An exact binary value: (-1)^neg * n * 2^e2.
struct ValuExact {
  bool neg;
  unsigned __int128 n;
  int e2;
};

inline ValuExact valu_decode(const ValuFmt& f, uint32_t code) {
  const uint32_t e = (code >> f.mbits) & ((1u << f.ebits) - 1u);
  const uint32_t m = code & ((1u << f.mbits) - 1u);
  ValuExact v;
  v.neg = ((code >> (f.ebits + f.mbits)) & 1u) != 0;
  if (e == 0) {
    v.n = m;
    v.e2 = 1 - f.bias - f.mbits;
  } else {
    v.n = (1u << f.mbits) + m;
    v.e2 = (int)e - f.bias - f.mbits;
  }
  return v;
}
inline ValuExact valu_exact_f32(uint32_t u) {
  return valu_decode(ValuFmt{8, 23, 127, 0x7F7FFFFFu}, u);
}
inline double valu_exact_to_double(const ValuExact& v) {  // exact for n < 2^53
  const double d = std::ldexp((double)(uint64_t)v.n, v.e2);
  return v.neg ? -d : d;
}

// The project's own integer round-to-nearest-even: one rounding of an exact
// value to format f, subnormals kept.  Throws when the rounded value is beyond
// the largest finite code: the caller's operands broke their range condition.
inline uint32_t valu_rne(const ValuFmt& f, const ValuExact& v) {
  const uint32_t sign = (v.neg ? 1u : 0u) << (f.ebits + f.mbits);
  if (v.n == 0) return sign;
  int p = 0;
  while ((v.n >> p) > 1) ++p;
  const int emin = 1 - f.bias;
  const int top = p + v.e2;  // exponent of the leading bit
  int q = (top < emin ? emin : top) - f.mbits;  // exponent of the result's ulp
  const int shift = q - v.e2;
  unsigned __int128 m;
  if (shift <= 0) {
    m = v.n << -shift;
  } else if (shift > 126) {
    m = 0;
  } else {
    m = v.n >> shift;
    const unsigned __int128 rem = v.n & (((unsigned __int128)1 << shift) - 1);
    const unsigned __int128 half = (unsigned __int128)1 << (shift - 1);
    if (rem > half || (rem == half && (m & 1))) ++m;
  }
  if (m == ((unsigned __int128)2 << f.mbits)) {
    m >>= 1;
    ++q;
  }
  uint32_t code;
  if (m < ((unsigned __int128)1 << f.mbits))
    code = (uint32_t)m;  // subnormal or zero
  else
    code = ((uint32_t)(q + f.mbits + f.bias) << f.mbits) |
           ((uint32_t)m - (1u << f.mbits));
  if (q + f.mbits + f.bias >= (1 << f.ebits) || code > f.max_code)
    throw std::domain_error("valu_rne: result beyond the largest finite value");
  return sign | code;
}

// a * b + c of three exact values, exactly
inline ValuExact valu_exact_fma(const ValuExact& a, const ValuExact& b,
                                const ValuExact& c) {
  const int ep = a.e2 + b.e2;
  const int e = ep < c.e2 ? ep : c.e2;
  if (ep - e > 64 || c.e2 - e > 64)
    throw std::domain_error("valu_exact_fma: exponents too far apart");
  __int128 p = (__int128)(a.n * b.n) << (ep - e);
  if (a.neg != b.neg) p = -p;
  __int128 s = (__int128)c.n << (c.e2 - e);
  if (c.neg) s = -s;
  const __int128 r = p + s;
  ValuExact out;
  // an exact zero sum of opposite signs is +0 under RNE; of equal signs, theirs
  out.neg = r < 0 || (r == 0 && (a.neg != b.neg) && c.neg);
  out.n = (unsigned __int128)(r < 0 ? -r : r);
  out.e2 = e;
  return out;
}
constexpr ValuExact kValuExactOne = {false, 1, 0};

inline uint32_t valu_f16_fma(uint32_t a, uint32_t b, uint32_t c) {
  return valu_rne(kValuFmtF16,
                  valu_exact_fma(valu_decode(kValuFmtF16, a),
                                 valu_decode(kValuFmtF16, b),
                                 valu_decode(kValuFmtF16, c)));
}
inline uint32_t valu_f16_add(uint32_t a, uint32_t b) {
  return valu_rne(kValuFmtF16,
                  valu_exact_fma(valu_decode(kValuFmtF16, a), kValuExactOne,
                                 valu_decode(kValuFmtF16, b)));
}
inline uint32_t valu_f16_mul(uint32_t a, uint32_t b) {
  ValuExact z = {false, 0, 0};
  // a * b + (zero of the product's sign) keeps the sign of an exact zero
  z.neg = valu_decode(kValuFmtF16, a).neg != valu_decode(kValuFmtF16, b).neg;
  return valu_rne(kValuFmtF16, valu_exact_fma(valu_decode(kValuFmtF16, a),
                                              valu_decode(kValuFmtF16, b), z));
}

// Separate multiply and add must not be contracted into an fma: HIP compiles
// host code with -ffp-contract=fast as well.
#if defined(__clang__)
#define VALU_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VALU_NO_CONTRACT
#endif
inline float valu_mul_rn(float a, float b) {
  VALU_NO_CONTRACT
  volatile float r = a * b;
  return r;
}
inline float valu_add_rn(float a, float b) {
  VALU_NO_CONTRACT
  volatile float r = a + b;
  return r;
}
inline double valu_mul_rn(double a, double b) {
  VALU_NO_CONTRACT
  volatile double r = a * b;
  return r;
}
inline double valu_add_rn(double a, double b) {
  VALU_NO_CONTRACT
  volatile double r = a + b;
  return r;
}

inline float valu_med3(float a, float b, float c) {
  const float lo = std::fmin(a, b), hi = std::fmax(a, b);
  return std::fmax(lo, std::fmin(hi, c));
}

// v_perm_b32: byte i of the result is picked by byte i of the selector from
// the eight bytes {a, b} (b is bytes 0..3, a is bytes 4..7); 0x0C gives 0x00.
// The sign-replicating selectors 8..11 and the 0xFF ones are not used.
inline uint32_t valu_perm(uint32_t a, uint32_t b, uint32_t sel) {
  const uint64_t src = valu_pack(b, a);
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t s = (sel >> (8 * i)) & 0xFFu;
    if (s > 7 && s != 0x0C)
      throw std::invalid_argument("valu: v_perm_b32 selector byte outside 0..7, 0x0c");
    const uint32_t byte = s == 0x0C ? 0u : (uint32_t)(src >> (8 * s)) & 0xFFu;
    r |= byte << (8 * i);
  }
  return r;
}

inline uint32_t valu_bitop3(uint32_t a, uint32_t b, uint32_t c, int table) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) {
    const int idx = (int)(((a >> i) & 1u) << 2 | ((b >> i) & 1u) << 1 | ((c >> i) & 1u));
    r |= (uint32_t)((table >> idx) & 1) << i;
  }
  return r;
}

inline bool valu_pow2_f32(uint32_t u) {  // a normal power of two, positive
  return (u >> 31) == 0 && (u & 0x7FFFFFu) == 0 && ((u >> 23) & 0xFFu) != 0 &&
         valu_f32_finite(u);
}
// x / scale for a power-of-two scale, exactly
inline ValuExact valu_unscale(uint32_t x, uint32_t scale) {
  ValuExact v = valu_exact_f32(x);
  v.e2 -= (int)((scale >> 23) & 0xFFu) - 127;
  return v;
}

// ---------------------------------------------------------------------------
// The reference of one lane-wise op.  Throws std::invalid_argument when an
// operand is outside what the op is checked on (valu_probe validates with
// it), std::domain_error from valu_rne when a result leaves its range.
// ---------------------------------------------------------------------------

inline void valu_need(bool ok, const char* what) {
  if (!ok) throw std::invalid_argument(std::string("valu: ") + what);
}

inline uint64_t valu_ref_lane(int kind, int imm, uint64_t a, uint64_t b, uint64_t c) {
  const uint32_t al = valu_lo(a), ah = valu_hi(a), bl = valu_lo(b), bh = valu_hi(b),
                 cl = valu_lo(c), ch = valu_hi(c);
  auto fin32 = [](uint32_t u) { valu_need(valu_f32_finite(u), "f32 operand is Inf or NaN"); };
  auto fin64 = [](uint64_t u) { valu_need(valu_f64_finite(u), "f64 operand is Inf or NaN"); };
  auto fin16x2 = [](uint32_t u) {
    valu_need(valu_f16_finite(u & 0xFFFFu) && valu_f16_finite(u >> 16),
              "f16 operand is Inf or NaN");
  };
  auto out32 = [](float f) {
    const uint32_t u = f32_bits(f);
    if (!valu_f32_finite(u)) throw std::domain_error("valu: f32 result is Inf or NaN");
    return u;
  };
  auto out64 = [](double d) {
    const uint64_t u = valu_f64_bits(d);
    if (!valu_f64_finite(u)) throw std::domain_error("valu: f64 result is Inf or NaN");
    return u;
  };
  switch (kind) {
    case kVkFmaF32:
      fin32(al), fin32(bl), fin32(cl);
      return out32(std::fmaf(valu_f32(al), valu_f32(bl), valu_f32(cl)));
    case kVkAddF32:
      fin32(al), fin32(bl);
      return out32(valu_add_rn(valu_f32(al), valu_f32(bl)));
    case kVkMulF32:
      fin32(al), fin32(bl);
      return out32(valu_mul_rn(valu_f32(al), valu_f32(bl)));
    case kVkPkFmaF32:
      fin32(al), fin32(bl), fin32(cl), fin32(ah), fin32(bh), fin32(ch);
      return valu_pack(out32(std::fmaf(valu_f32(al), valu_f32(bl), valu_f32(cl))),
                       out32(std::fmaf(valu_f32(ah), valu_f32(bh), valu_f32(ch))));
    case kVkPkAddF32:
      fin32(al), fin32(bl), fin32(ah), fin32(bh);
      return valu_pack(out32(valu_add_rn(valu_f32(al), valu_f32(bl))),
                       out32(valu_add_rn(valu_f32(ah), valu_f32(bh))));
    case kVkPkMulF32:
      fin32(al), fin32(bl), fin32(ah), fin32(bh);
      return valu_pack(out32(valu_mul_rn(valu_f32(al), valu_f32(bl))),
                       out32(valu_mul_rn(valu_f32(ah), valu_f32(bh))));
    case kVkMinF32:
    case kVkMaxF32:
    case kVkMed3F32: {
      fin32(al), fin32(bl), fin32(cl);
      const float x = valu_f32(al), y = valu_f32(bl), z = valu_f32(cl);
      // which of two equal values (+0 / -0 included) comes out is not claimed
      valu_need(x != y && (kind != kVkMed3F32 || (x != z && y != z)),
                "min / max / med3 operands must differ in value");
      if (kind == kVkMinF32) return out32(std::fmin(x, y));
      if (kind == kVkMaxF32) return out32(std::fmax(x, y));
      return out32(valu_med3(x, y, z));
    }
    case kVkLdexpF32:
      fin32(al);
      valu_need((int32_t)bl >= -300 && (int32_t)bl <= 300, "ldexp exponent beyond +-300");
      return out32(std::ldexp(valu_f32(al), (int)(int32_t)bl));
    case kVkFrexpMantF32: {
      fin32(al);
      int e;
      return out32(std::frexp(valu_f32(al), &e));
    }
    case kVkRndneF32:
      fin32(al);
      return out32(std::nearbyint(valu_f32(al)));
    case kVkFmaF64:
      fin64(a), fin64(b), fin64(c);
      return out64(std::fma(valu_f64(a), valu_f64(b), valu_f64(c)));
    case kVkAddF64:
      fin64(a), fin64(b);
      return out64(valu_add_rn(valu_f64(a), valu_f64(b)));
    case kVkMulF64:
      fin64(a), fin64(b);
      return out64(valu_mul_rn(valu_f64(a), valu_f64(b)));
    case kVkLdexpF64:
      fin64(a);
      valu_need((int32_t)bl >= -2200 && (int32_t)bl <= 2200, "ldexp exponent beyond +-2200");
      return out64(std::ldexp(valu_f64(a), (int)(int32_t)bl));
    case kVkPkFmaF16:
      fin16x2(al), fin16x2(bl), fin16x2(cl);
      return valu_f16_fma(al & 0xFFFFu, bl & 0xFFFFu, cl & 0xFFFFu) |
             valu_f16_fma(al >> 16, bl >> 16, cl >> 16) << 16;
    case kVkPkAddF16:
      fin16x2(al), fin16x2(bl);
      return valu_f16_add(al & 0xFFFFu, bl & 0xFFFFu) |
             valu_f16_add(al >> 16, bl >> 16) << 16;
    case kVkPkMulF16:
      fin16x2(al), fin16x2(bl);
      return valu_f16_mul(al & 0xFFFFu, bl & 0xFFFFu) |
             valu_f16_mul(al >> 16, bl >> 16) << 16;
    case kVkDot2F16:
    case kVkDot2Bf16: {
      // small integers only: every partial sum is exact in any order and at
      // any internal width, so the undocumented rounding plays no part
      const ValuFmt& f = kind == kVkDot2F16 ? kValuFmtF16 : kValuFmtBf16;
      double v[5];
      const uint32_t codes[4] = {al & 0xFFFFu, al >> 16, bl & 0xFFFFu, bl >> 16};
      for (int i = 0; i < 4; ++i) {
        valu_need(((codes[i] >> f.mbits) & ((1u << f.ebits) - 1u)) !=
                      (1u << f.ebits) - 1u, "dot2 operand is Inf or NaN");
        v[i] = valu_exact_to_double(valu_decode(f, codes[i]));
      }
      fin32(cl);
      v[4] = valu_f32(cl);
      for (double x : v)
        valu_need(x == std::nearbyint(x) && std::fabs(x) <= 64.0,
                  "dot2 operands must be integers of magnitude <= 64");
      return f32_bits((float)(v[0] * v[2] + v[1] * v[3] + v[4]));
    }
    case kVkMadU64U32: return (uint64_t)al * bl + c;
    case kVkMulHiU32: return (uint32_t)(((uint64_t)al * bl) >> 32);
    case kVkMulLoU32: return (uint32_t)((uint64_t)al * bl);
    case kVkMulI24: {
      const int64_t x = (int32_t)(al << 8) >> 8, y = (int32_t)(bl << 8) >> 8;
      return (uint32_t)(uint64_t)(x * y);
    }
    case kVkAddU64: return a + b;
    case kVkSubU64: return a - b;
    case kVkLshlB32: return al << (bl & 31u);
    case kVkLshrB32: return al >> (bl & 31u);
    case kVkAshrI32: return (uint32_t)((int32_t)al >> (bl & 31u));
    case kVkLshlB64: return a << (bl & 63u);
    case kVkLshrB64: return a >> (bl & 63u);
    case kVkAshrI64: return (uint64_t)((int64_t)a >> (bl & 63u));
    case kVkBfeU32: {
      const uint32_t off = bl & 31u, width = cl & 31u;
      return width == 0 ? 0u : (al >> off) & ((1u << width) - 1u);
    }
    case kVkBfiB32: return (al & bl) | (~al & cl);
    case kVkPermB32: return valu_perm(al, bl, cl);
    case kVkAlignbitB32: return (uint32_t)(valu_pack(bl, al) >> (cl & 31u));
    case kVkSadU8: {
      uint32_t s = cl;
      for (int i = 0; i < 4; ++i) {
        const int x = (al >> (8 * i)) & 0xFF, y = (bl >> (8 * i)) & 0xFF;
        s += (uint32_t)(x > y ? x - y : y - x);
      }
      return s;
    }
    case kVkBcntU32: {
      uint32_t n = bl;
      for (int i = 0; i < 32; ++i) n += (al >> i) & 1u;
      return n;
    }
    case kVkFfbhU32: {
      uint32_t n = 0;
      while (n < 32 && !((al >> (31 - n)) & 1u)) ++n;
      return n;  // 32 for zero
    }
    case kVkBfrevB32: {
      uint32_t r = 0;
      for (int i = 0; i < 32; ++i) r |= ((al >> i) & 1u) << (31 - i);
      return r;
    }
    case kVkBitop3B32: return valu_bitop3(al, bl, cl, imm);
    case kVkDot4I8: {
      uint32_t s = cl;
      for (int i = 0; i < 4; ++i)
        s += (uint32_t)((int32_t)(int8_t)(al >> (8 * i)) * (int32_t)(int8_t)(bl >> (8 * i)));
      return s;
    }
    case kVkDot4U8: {
      uint32_t s = cl;
      for (int i = 0; i < 4; ++i) s += ((al >> (8 * i)) & 0xFFu) * ((bl >> (8 * i)) & 0xFFu);
      return s;
    }
    case kVkCmpSelect: return (int32_t)al < (int32_t)bl ? cl : ch;
    case kVkCvtF16F32:
      fin32(al);
      return valu_rne(kValuFmtF16, valu_exact_f32(al));
    case kVkCvtPkBf16F32:
      fin32(al), fin32(ah);
      return valu_rne(kValuFmtBf16, valu_exact_f32(al)) |
             valu_rne(kValuFmtBf16, valu_exact_f32(ah)) << 16;
    case kVkCvtI32F32: {
      fin32(al);
      const float x = valu_f32(al);
      valu_need(x >= -2147483648.0f && x < 2147483648.0f, "f32 -> i32 out of range");
      return (uint32_t)(int32_t)x;
    }
    case kVkCvtU32F32: {
      fin32(al);
      const float x = valu_f32(al);
      valu_need((al >> 31) == 0 && x < 4294967296.0f, "f32 -> u32 out of range");
      return (uint32_t)x;
    }
    case kVkCvtF32I32: return f32_bits((float)(int32_t)al);
    case kVkCvtF32U32: return f32_bits((float)al);
    case kVkCvtPkFp8F32:
    case kVkCvtPkBf8F32: {
      fin32(al), fin32(ah);
      const bool fp8 = kind == kVkCvtPkFp8F32;
      const float lim = fp8 ? 448.0f : 57344.0f;
      valu_need(std::fabs(valu_f32(al)) <= lim && std::fabs(valu_f32(ah)) <= lim,
                "fp8 / bf8 input beyond the largest finite value");
      const ValuFmt& f = fp8 ? kValuFmtE4m3 : kValuFmtE5m2;
      const uint32_t pair = valu_rne(f, valu_exact_f32(al)) |
                            valu_rne(f, valu_exact_f32(ah)) << 8;
      return imm ? (cl & 0x0000FFFFu) | pair << 16 : (cl & 0xFFFF0000u) | pair;
    }
    case kVkCvtF32Fp8:
    case kVkCvtF32Bf8: {
      const uint32_t code = (al >> (8 * imm)) & 0xFFu;
      if (kind == kVkCvtF32Fp8)
        valu_need((code & 0x7Fu) != 0x7Fu, "fp8 code is NaN");
      else
        valu_need((code & 0x7Cu) != 0x7Cu, "bf8 code is Inf or NaN");
      return f32_bits((float)valu_exact_to_double(
          valu_decode(kind == kVkCvtF32Fp8 ? kValuFmtE4m3 : kValuFmtE5m2, code)));
    }
    case kVkCvtScalePkF32Fp4: {
      valu_need(valu_pow2_f32(bl), "fp4 scale must be a normal power of two");
      const uint32_t byte = (al >> (8 * imm)) & 0xFFu;
      uint32_t r[2];
      for (int i = 0; i < 2; ++i) {
        ValuExact v = valu_decode(kValuFmtE2m1, (byte >> (4 * i)) & 0xFu);
        v.e2 += (int)((bl >> 23) & 0xFFu) - 127;
        r[i] = out32((float)valu_exact_to_double(v));
        valu_need(v.n == 0 || ((r[i] >> 23) & 0xFFu) != 0, "fp4 * scale is subnormal");
      }
      return valu_pack(r[0], r[1]);
    }
    case kVkCvtScalePkFp4F32: {
      fin32(al), fin32(ah);
      valu_need(valu_pow2_f32(bl), "fp4 scale must be a normal power of two");
      uint32_t nib[2];
      const uint32_t x[2] = {al, ah};
      for (int i = 0; i < 2; ++i) {
        const ValuExact v = valu_unscale(x[i], bl);
        const int ex = (int)((bl >> 23) & 0xFFu) - 127;
        valu_need(std::fabs(std::ldexp((double)valu_f32(x[i]), -ex)) <= 6.0,
                  "|x / scale| beyond 6");
        nib[i] = valu_rne(kValuFmtE2m1, v);
      }
      const uint32_t byte = nib[0] | nib[1] << 4;
      return (cl & ~(0xFFu << (8 * imm))) | byte << (8 * imm);
    }
    default:
      throw std::invalid_argument("valu: op has no lane-wise reference");
  }
}

// ---------------------------------------------------------------------------
// Cross-lane: the lane-permutation model.  dpp_source gives the lane a DPP
// control reads from, or -1 where the source is invalid (the result is then
// 0 under bound_ctrl, `old` otherwise).  A row is 16 lanes, a bank 4.
//
//   quad_perm [p0 p1 p2 p3]   lane l reads lane (l & ~3) | p[l & 3]
//   row_shl:n                 l + n, invalid past the end of the row
//   row_shr:n                 l - n, invalid before the start of the row
//   row_ror:n                 row base + ((l % 16) - n) mod 16
//   wave_shl:1 / wave_rol:1   l + 1, lane 63 invalid / reads lane 0
//   wave_shr:1 / wave_ror:1   l - 1, lane 0 invalid / reads lane 63
//   row_mirror                row base + 15 - l % 16
//   row_half_mirror           half-row base + 7 - l % 8
//   row_bcast:15              rows 1..3 read the last lane of the row before;
//                             row 0 reads itself (a plain move, never invalid)
//   row_bcast:31              rows 2 and 3 read lane 31; rows 0 and 1 read
//                             themselves
// ---------------------------------------------------------------------------

inline int valu_dpp_source(int ctrl, int l) {
  const int row = l & ~15, r = l & 15;
  if (ctrl <= 0xFF) return (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3);
  if (ctrl >= 0x101 && ctrl <= 0x10F) return r + (ctrl & 15) < 16 ? l + (ctrl & 15) : -1;
  if (ctrl >= 0x111 && ctrl <= 0x11F) return r >= (ctrl & 15) ? l - (ctrl & 15) : -1;
  if (ctrl >= 0x121 && ctrl <= 0x12F) return row | ((r - (ctrl & 15)) & 15);
  switch (ctrl) {
    case 0x130: return l < 63 ? l + 1 : -1;
    case 0x134: return (l + 1) & 63;
    case 0x138: return l > 0 ? l - 1 : -1;
    case 0x13C: return (l - 1) & 63;
    case 0x140: return row | (15 - r);
    case 0x141: return (l & ~7) | (7 - (l & 7));
    case 0x142: return l >= 16 ? row - 1 : l;
    case 0x143: return l >= 32 ? 31 : l;
  }
  throw std::invalid_argument("valu: unknown dpp_ctrl");
}

// The reference of one op over a whole wave: 64 lanes of a, b, c in, 64
// results out.  Lane-wise ops go through valu_ref_lane.
inline void valu_ref_wave(int op, const uint64_t* a, const uint64_t* b,
                          const uint64_t* c, uint64_t* out) {
  const int kind = kValuOpKind[op], imm = kValuOpImm[op];
  if (kValuOpGroup[op] == kValuGroupConsensus)
    throw std::invalid_argument("valu: consensus ops have no host reference");
  switch (kind) {
    case kVkDpp: {
      const int ctrl = imm & 0xFFF, v = imm >> 12;
      for (int l = 0; l < 64; ++l) {
        const bool enabled = ((kValuDppRowMask[v] >> (l >> 4)) & 1) &&
                             ((kValuDppBankMask[v] >> ((l >> 2) & 3)) & 1);
        const int src = valu_dpp_source(ctrl, l);
        const uint32_t old = valu_lo(b[l]);
        out[l] = !enabled ? old : src >= 0 ? valu_lo(a[src]) : v ? 0u : old;
      }
      return;
    }
    case kVkReadlane:
      for (int l = 0; l < 64; ++l) out[l] = valu_lo(a[kValuReadLanes[l & 3]]);
      return;
    case kVkReadfirstlane:
      for (int l = 0; l < 64; ++l) out[l] = valu_lo(a[0]);
      return;
    case kVkPermlane16Swap:
      // rows 1 and 3 of vdst (a) swap with rows 0 and 2 of src (b)
      for (int l = 0; l < 64; ++l) {
        const bool odd = (l >> 4) & 1;
        out[l] = odd ? valu_pack(valu_lo(b[l - 16]), valu_lo(b[l]))
                     : valu_pack(valu_lo(a[l]), valu_lo(a[l + 16]));
      }
      return;
    case kVkPermlane32Swap:
      // lanes 32..63 of vdst (a) swap with lanes 0..31 of src (b)
      for (int l = 0; l < 64; ++l)
        out[l] = l >= 32 ? valu_pack(valu_lo(b[l - 32]), valu_lo(b[l]))
                         : valu_pack(valu_lo(a[l]), valu_lo(a[l + 32]));
      return;
    case kVkMbcnt:
      for (int l = 0; l < 64; ++l) {
        uint32_t n = valu_lo(b[l]);
        for (int i = 0; i < l; ++i) n += (uint32_t)((a[l] >> i) & 1u);
        out[l] = n;
      }
      return;
    case kVkCmpMask: {
      uint64_t mask = 0;
      for (int l = 0; l < 64; ++l)
        mask |= (uint64_t)(valu_lo(a[l]) < valu_lo(b[l])) << l;
      for (int l = 0; l < 64; ++l) out[l] = mask;
      return;
    }
    default:
      for (int l = 0; l < 64; ++l) out[l] = valu_ref_lane(kind, imm, a[l], b[l], c[l]);
  }
}

// Operand checks of a consensus op (valu_probe validates with it): no NaN in,
// and inputs on which the raw instruction returns a finite number.
inline void valu_check_consensus_operand(int kind, uint64_t a, uint64_t b) {
  (void)b;
  const uint32_t al = valu_lo(a);
  const float x = valu_f32(al);
  switch (kind) {
    case kVkExpF32:
      valu_need(valu_f32_finite(al) && std::fabs(x) <= 120.0f, "v_exp_f32 input beyond +-120");
      return;
    case kVkLogF32: case kVkRsqF32: case kVkRcpF32:
      valu_need(valu_f32_finite(al) && ((al >> 23) & 0xFFu) != 0 &&
                    (kind == kVkRcpF32 || x > 0.0f),
                "input must be a normal number (positive for log / rsq)");
      valu_need(std::fabs(x) < 1e30f && std::fabs(x) > 1e-30f, "input magnitude outside 1e-30..1e30");
      return;
    case kVkSqrtF32:
      valu_need(valu_f32_finite(al) && (x > 0.0f || al == 0), "v_sqrt_f32 input negative");
      return;
    case kVkSinF32: case kVkCosF32:
      valu_need(valu_f32_finite(al) && std::fabs(x) <= 256.0f, "sin / cos input beyond +-256 revolutions");
      return;
    case kVkRcpF64: case kVkRsqF64: {
      const double d = valu_f64(a);
      valu_need(valu_f64_finite(a) && std::fabs(d) > 1e-300 && std::fabs(d) < 1e300 &&
                    (kind == kVkRcpF64 || d > 0.0),
                "f64 input must be a normal number (positive for rsq)");
      return;
    }
    case kVkCvtSrFp8F32:
      valu_need(valu_f32_finite(al) && std::fabs(x) <= 448.0f, "fp8 input beyond 448");
      return;
    default:
      return;
  }
}

// ---------------------------------------------------------------------------
// The generator
// ---------------------------------------------------------------------------

inline uint64_t valu_rand(int op, int set, int lane, int k) {
  return hbm_pattern_value(kHbmPatternHash, kValuKey,
                           (((uint64_t)op << 8 | (uint64_t)set) << 8 | (uint64_t)lane) << 4 | (uint64_t)k);
}

// a finite f32 with exponent in [emin, emax]; one in four has a short mantissa
inline uint32_t valu_gen_f32(uint64_t r, int emin, int emax) {
  const uint32_t sign = (uint32_t)(r & 1u);
  const int e = emin + (int)((r >> 1) % (uint64_t)(emax - emin + 1));
  uint32_t mant = (uint32_t)(r >> 40) & 0x7FFFFFu;
  if (((r >> 20) & 3u) == 0) mant &= 0x700000u;
  if (e < -126) return sign << 31 | (mant >> (-126 - e)) | 1u;  // subnormal
  return sign << 31 | (uint32_t)(e + 127) << 23 | mant;
}
inline uint64_t valu_gen_f64(uint64_t r, int emin, int emax) {
  const uint64_t sign = r & 1u;
  const int e = emin + (int)((r >> 1) % (uint64_t)(emax - emin + 1));
  uint64_t mant = (r >> 11) & 0xFFFFFFFFFFFFFull;
  if (((r >> 8) & 3u) == 0) mant &= 0xE000000000000ull;
  if (e < -1022) return sign << 63 | (mant >> (-1022 - e)) | 1u;
  return sign << 63 | (uint64_t)(e + 1023) << 52 | mant;
}
inline uint32_t valu_gen_f16(uint64_t r, int emin, int emax) {
  const uint32_t sign = (uint32_t)(r & 1u);
  const int e = emin + (int)((r >> 1) % (uint64_t)(emax - emin + 1));
  uint32_t mant = (uint32_t)(r >> 40) & 0x3FFu;
  if (((r >> 20) & 3u) == 0) mant &= 0x380u;
  if (e < -14) return sign << 15 | (mant >> (-14 - e)) | 1u;
  return sign << 15 | (uint32_t)(e + 15) << 10 | mant;
}
inline uint32_t valu_gen_f16x2(uint64_t r, int emin, int emax) {
  return valu_gen_f16(r, emin, emax) | valu_gen_f16(r * 0x9E3779B97F4A7C15ull >> 3, emin, emax) << 16;
}
// an integer in [-8, 8] as f16 / bf16 / f32 bits
inline uint32_t valu_small_int(uint64_t r, const ValuFmt* f) {
  const int v = (int)(r % 17u) - 8;
  const ValuExact e = {v < 0, (unsigned __int128)(v < 0 ? -v : v), 0};
  return f ? valu_rne(*f, e) : f32_bits((float)v);
}

constexpr uint32_t kF32One = 0x3F800000u, kF32NegZero = 0x80000000u;
inline uint32_t valu_f32_pow2(int e) { return (uint32_t)(e + 127) << 23; }

struct ValuOperands {
  uint64_t a, b, c;
};

// The pinned records of the floating groups (set 0, lanes 0..4): an exact
// tie, a subnormal result, signed zeros, and the triple on which fused and
// unfused multiply-add differ.
inline bool valu_pinned_f32(int kind, int lane, ValuOperands& o) {
  const uint32_t t = kF32One | 0x800u;   // 1 + 2^-12
  switch (kind) {
    case kVkFmaF32: case kVkPkFmaF32: {
      const uint32_t rec[5][3] = {
          {t, t, 0},                                       // 1 + 2^-11 + 2^-24: tie
          {valu_f32_pow2(-100), valu_f32_pow2(-30), 0x00000200u},  // subnormal
          {kF32NegZero, 0x40A00000u, 0},                   // -0 * 5 + 0 = +0
          {kF32NegZero, 0x40A00000u, kF32NegZero},         // -0 * 5 - 0 = -0
          {t, t, 0xBF801000u}};  // - (1 + 2^-11): fused 2^-24, unfused 0
      if (lane >= 5) return false;
      o = {valu_pack(rec[lane][0], rec[4 - lane][0]), valu_pack(rec[lane][1], rec[4 - lane][1]),
           valu_pack(rec[lane][2], rec[4 - lane][2])};
      return true;
    }
    case kVkAddF32: case kVkPkAddF32: {
      const uint32_t rec[4][2] = {{kF32One, valu_f32_pow2(-24)},       // tie -> 1
                                  {valu_f32_pow2(-126), 0x80400000u},   // 2^-126 - 2^-127
                                  {kF32NegZero, 0},
                                  {kF32NegZero, kF32NegZero}};
      if (lane >= 4) return false;
      o = {valu_pack(rec[lane][0], rec[3 - lane][0]), valu_pack(rec[lane][1], rec[3 - lane][1]), 0};
      return true;
    }
    case kVkMulF32: case kVkPkMulF32: {
      const uint32_t rec[4][2] = {{t, t},
                                  {valu_f32_pow2(-100), valu_f32_pow2(-30) | 0x400000u},
                                  {kF32NegZero, 0x40A00000u},
                                  {0x00000003u, 0x3F000000u}};  // 3 ulp / 2: tie, subnormal
      if (lane >= 4) return false;
      o = {valu_pack(rec[lane][0], rec[3 - lane][0]), valu_pack(rec[lane][1], rec[3 - lane][1]), 0};
      return true;
    }
    case kVkLdexpF32:
      // (1 + 2^-23) * 2^-127: a tie between two subnormals; -0 stays -0
      if (lane == 0) { o = {kF32One | 1u, (uint32_t)-127, 0}; return true; }
      if (lane == 1) { o = {kF32NegZero, 12u, 0}; return true; }
      if (lane == 2) { o = {0x00000005u, 30u, 0}; return true; }
      return false;
    case kVkFrexpMantF32:
      if (lane == 0) { o = {0x00000005u, 0, 0}; return true; }
      if (lane == 1) { o = {kF32NegZero, 0, 0}; return true; }
      return false;
    case kVkRndneF32: {
      const uint32_t rec[5] = {0x40200000u /* 2.5 */, 0xBF000000u /* -0.5 */, kF32NegZero,
                               0x40600000u /* 3.5 */, 0x00000001u};
      if (lane >= 5) return false;
      o = {rec[lane], 0, 0};
      return true;
    }
    case kVkMinF32: case kVkMaxF32: case kVkMed3F32:
      if (lane == 0) { o = {kF32NegZero, 0x00000001u, 0x80000001u}; return true; }
      return false;
  }
  return false;
}

inline bool valu_pinned_f64(int kind, int lane, ValuOperands& o) {
  const uint64_t one = 0x3FF0000000000000ull, nz = 0x8000000000000000ull;
  const uint64_t t = one | (1ull << 25);  // 1 + 2^-27: square is a tie
  if (lane >= 3) return false;
  switch (kind) {
    case kVkFmaF64: case kVkMulF64: {
      const uint64_t rec[3][3] = {{t, t, 0},
                                  {0x0000000000000003ull, 0x3FE0000000000000ull, 0},
                                  {nz, 0x4014000000000000ull, kind == kVkFmaF64 && lane == 2 ? nz : 0}};
      o = {rec[lane][0], rec[lane][1], rec[lane][2]};
      return true;
    }
    case kVkAddF64: {
      const uint64_t rec[3][2] = {{one, 0x3CA0000000000000ull},  // 1 + 2^-53: tie
                                  {0x0010000000000000ull, 0x8008000000000000ull},
                                  {nz, 0}};
      o = {rec[lane][0], rec[lane][1], 0};
      return true;
    }
    case kVkLdexpF64:
      if (lane == 0) { o = {one | 1ull, (uint32_t)-1023, 0}; return true; }
      if (lane == 1) { o = {nz, 5u, 0}; return true; }
      return false;
  }
  return false;
}

inline bool valu_pinned_f16(int kind, int lane, ValuOperands& o) {
  // low halves pinned, high halves a second pinned record
  const uint32_t one = 0x3C00u, nz = 0x8000u, five = 0x4500u;
  if (lane >= 3) return false;
  switch (kind) {
    case kVkPkFmaF16: {
      // (1 + 2^-5)(1 + 2^-6) = 1 + 2^-5 + 2^-6 + 2^-11: tie
      const uint32_t rec[3][3] = {{one | 0x20u, one | 0x10u, 0},
                                  {0x1400u /* 2^-10 */, 0x1600u /* 1.5 * 2^-10 */, 0x0001u},
                                  {nz, five, nz}};
      o = {rec[lane][0] | rec[2 - lane][0] << 16, rec[lane][1] | rec[2 - lane][1] << 16,
           rec[lane][2] | rec[2 - lane][2] << 16};
      return true;
    }
    case kVkPkAddF16: {
      const uint32_t rec[3][2] = {{one, 0x1000u /* 2^-11 */}, {0x0400u, 0x8200u}, {nz, 0}};
      o = {rec[lane][0] | rec[2 - lane][0] << 16, rec[lane][1] | rec[2 - lane][1] << 16, 0};
      return true;
    }
    case kVkPkMulF16: {
      const uint32_t rec[3][2] = {{one | 0x20u, one | 0x10u}, {0x0003u, 0x3800u /* 0.5 */}, {nz, five}};
      o = {rec[lane][0] | rec[2 - lane][0] << 16, rec[lane][1] | rec[2 - lane][1] << 16, 0};
      return true;
    }
  }
  return false;
}

inline uint32_t valu_f32_from_double(double d) { return f32_bits((float)d); }

// inputs of the fp8 / bf8 encoders: codes, midpoints between neighbouring
// codes (exact ties), subnormal targets and arbitrary in-range values
inline uint32_t valu_gen_fp8_input(uint64_t r, const ValuFmt& f) {
  const uint32_t top = f.max_code;
  const uint32_t code = (uint32_t)((r >> 8) % (top + 1u));
  const double lo = valu_exact_to_double(valu_decode(f, code));
  const double hi = valu_exact_to_double(valu_decode(f, code < top ? code + 1 : code));
  double v;
  switch (r & 3u) {
    case 0: v = lo; break;
    case 1: v = (lo + hi) / 2; break;                      // tie
    default: v = lo + (hi - lo) * (double)((r >> 40) & 0xFFFFu) / 65536.0;
  }
  const uint32_t bits = valu_f32_from_double(v);
  return bits | (uint32_t)((r >> 7) & 1u) << 31;
}

inline ValuOperands valu_operands(int op, int set, int lane) {
  const int kind = kValuOpKind[op];
  const uint64_t r0 = valu_rand(op, set, lane, 0), r1 = valu_rand(op, set, lane, 1),
                 r2 = valu_rand(op, set, lane, 2), r3 = valu_rand(op, set, lane, 3),
                 r4 = valu_rand(op, set, lane, 4), r5 = valu_rand(op, set, lane, 5);
  ValuOperands o = {r0, r1, r2};
  if (set == 0) {
    if (kValuOpGroup[op] == kValuGroupF32 && valu_pinned_f32(kind, lane, o)) return o;
    if (kValuOpGroup[op] == kValuGroupF64 && valu_pinned_f64(kind, lane, o)) return o;
    if (kValuOpGroup[op] == kValuGroupF16 && valu_pinned_f16(kind, lane, o)) return o;
  }
  // set 3 of the f32 / f64 ops works at the bottom of the exponent range
  const int lo32 = set == 3 ? -140 : -12, hi32 = set == 3 ? -100 : 12;
  switch (kind) {
    case kVkFmaF32: case kVkPkFmaF32:
      // products near the addend, so cancellation and ties are common
      o.a = valu_pack(valu_gen_f32(r0, -12, 12), valu_gen_f32(r3, -12, 12));
      o.b = valu_pack(valu_gen_f32(r1, set == 3 ? -135 : -12, set == 3 ? -120 : 12),
                      valu_gen_f32(r4, -12, 12));
      o.c = valu_pack(valu_gen_f32(r2, set == 3 ? -140 : -20, set == 3 ? -110 : 20),
                      valu_gen_f32(r5, -20, 20));
      break;
    case kVkAddF32: case kVkPkAddF32:
      o.a = valu_pack(valu_gen_f32(r0, lo32, hi32), valu_gen_f32(r3, -12, 12));
      o.b = valu_pack(valu_gen_f32(r1, lo32, hi32), valu_gen_f32(r4, -12, 12));
      break;
    case kVkMulF32: case kVkPkMulF32:
      o.a = valu_pack(valu_gen_f32(r0, -12, 12), valu_gen_f32(r3, -12, 12));
      o.b = valu_pack(valu_gen_f32(r1, lo32, hi32), valu_gen_f32(r4, -12, 12));
      break;
    case kVkMinF32: case kVkMaxF32: case kVkMed3F32:
      o.a = valu_gen_f32(r0, lo32, hi32);
      o.b = valu_gen_f32(r1, lo32, hi32) ^ 2u;
      o.c = valu_gen_f32(r2, lo32, hi32) ^ 4u;
      if (o.a == o.b) o.b ^= 0x10u;
      if (o.c == o.a || o.c == o.b) o.c ^= 0x20u;
      if (o.c == o.a || o.c == o.b) o.c ^= 0x40u;
      break;
    case kVkLdexpF32:
      o.a = valu_gen_f32(r0, -20, 20);
      o.b = (uint32_t)((int)(r1 % 61u) - 30 - (set == 3 ? 125 : 0));
      break;
    case kVkFrexpMantF32:
      o.a = valu_gen_f32(r0, set == 3 ? -149 : -60, set == 3 ? -120 : 60);
      break;
    case kVkRndneF32:
      o.a = valu_gen_f32(r0, -3, 24);
      if ((r1 & 3u) == 0)  // n + 0.5: tie
        o.a = f32_bits((float)((int)(r1 >> 8 & 0xFFFF) - 32768) + 0.5f);
      break;
    case kVkFmaF64:
      o.a = valu_gen_f64(r0, -12, 12);
      o.b = valu_gen_f64(r1, set == 3 ? -1040 : -12, set == 3 ? -1020 : 12);
      o.c = valu_gen_f64(r2, set == 3 ? -1060 : -20, set == 3 ? -1010 : 20);
      break;
    case kVkAddF64:
      o.a = valu_gen_f64(r0, set == 3 ? -1070 : -12, set == 3 ? -1015 : 12);
      o.b = valu_gen_f64(r1, set == 3 ? -1070 : -12, set == 3 ? -1015 : 12);
      break;
    case kVkMulF64:
      o.a = valu_gen_f64(r0, -12, 12);
      o.b = valu_gen_f64(r1, set == 3 ? -1070 : -12, set == 3 ? -1015 : 12);
      break;
    case kVkLdexpF64:
      o.a = valu_gen_f64(r0, -20, 20);
      o.b = (uint32_t)((int)(r1 % 61u) - 30 - (set == 3 ? 1040 : 0));
      break;
    case kVkPkFmaF16:
      o.a = valu_gen_f16x2(r0, -5, 5);
      o.b = valu_gen_f16x2(r1, set == 3 ? -14 : -5, set == 3 ? -8 : 5);
      o.c = valu_gen_f16x2(r2, set == 3 ? -20 : -8, set == 3 ? -10 : 8);
      break;
    case kVkPkAddF16:
      o.a = valu_gen_f16x2(r0, set == 3 ? -22 : -6, set == 3 ? -12 : 6);
      o.b = valu_gen_f16x2(r1, set == 3 ? -22 : -6, set == 3 ? -12 : 6);
      break;
    case kVkPkMulF16:
      o.a = valu_gen_f16x2(r0, -5, 5);
      o.b = valu_gen_f16x2(r1, set == 3 ? -20 : -5, set == 3 ? -8 : 5);
      break;
    case kVkDot2F16: case kVkDot2Bf16: {
      const ValuFmt* f = kind == kVkDot2F16 ? &kValuFmtF16 : &kValuFmtBf16;
      o.a = valu_small_int(r0, f) | valu_small_int(r0 >> 16, f) << 16;
      o.b = valu_small_int(r1, f) | valu_small_int(r1 >> 16, f) << 16;
      o.c = valu_small_int(r2, nullptr);
      break;
    }
    case kVkMulI24: case kVkMulHiU32: case kVkMulLoU32: case kVkMadU64U32:
      // a quarter of the lanes multiply all-ones style values: carries
      if ((r3 & 3u) == 0) o.a |= 0xFFFF0000FFFF0000ull, o.b |= 0xFF00FF00FF00FF00ull;
      break;
    case kVkAddU64: case kVkSubU64:
      // long carry / borrow chains through the word boundary
      if ((r3 & 1u) == 0) o.a |= 0x0000FFFFFFFF0000ull;
      if ((r3 & 2u) == 0) o.b = (o.b & 0xFFFF00000000FFFFull) | 0x0000000000010000ull;
      break;
    case kVkLshlB32: case kVkLshrB32: case kVkAshrI32:
      o.b = (r1 & 7u) == 0 ? (r1 >> 8 & 1u) * 31u : r1 & 31u;
      break;
    case kVkLshlB64: case kVkLshrB64: case kVkAshrI64:
      o.b = (r1 & 7u) == 0 ? ((r1 >> 8 & 2u) ? 32u : 0u) + ((r1 >> 8 & 1u) ? 31u : 0u) : r1 & 63u;
      break;
    case kVkPermB32: {
      uint32_t sel = 0;
      for (int i = 0; i < 4; ++i) {
        const uint32_t s = (uint32_t)(r2 >> (8 * i)) & 15u;
        sel |= (s < 8 ? s : s < 10 ? 0x0Cu : s & 7u) << (8 * i);
      }
      o.c = sel;
      break;
    }
    case kVkFfbhU32:
      o.a = (uint32_t)r0 >> (r1 % 33u == 32 ? 31 : r1 % 33u);
      if (r1 % 33u == 32) o.a = 0;
      break;
    case kVkCmpSelect:
      if ((r3 & 3u) == 0) o.b = (o.b & ~0xFFFFFFFFull) | valu_lo(o.a);  // equal: not less
      break;
    case kVkCvtF16F32: {
      o.a = valu_gen_f32(r0, set == 3 ? -26 : -14, set == 3 ? -13 : 15);
      if ((r1 & 3u) == 0) o.a = (valu_lo(o.a) & 0xFFFFE000u) | 0x1000u;  // tie
      break;
    }
    case kVkCvtPkBf16F32: {
      uint32_t x = valu_gen_f32(r0, set == 3 ? -140 : -30, set == 3 ? -120 : 30);
      uint32_t y = valu_gen_f32(r1, -30, 30);
      if ((r2 & 3u) == 0) x = (x & 0xFFFF0000u) | 0x8000u;  // tie
      if ((r2 & 12u) == 0) y = (y & 0xFFFF0000u) | 0x8000u;
      o.a = valu_pack(x, y);
      break;
    }
    case kVkCvtI32F32:
      o.a = valu_gen_f32(r0, -3, 30);
      break;
    case kVkCvtU32F32:
      o.a = valu_gen_f32(r0, -3, 31) & 0x7FFFFFFFu;
      break;
    case kVkCvtF32I32: case kVkCvtF32U32:
      // above 2^24 the conversion rounds; 2^24 + 1 style values are ties
      if ((r1 & 3u) == 0) o.a = (valu_lo(o.a) & 0xFFFFFF00u) | 0x80u;
      if ((r1 & 12u) == 0) o.a = valu_lo(o.a) >> (r1 >> 8 & 31u);
      break;
    case kVkCvtPkFp8F32: case kVkCvtPkBf8F32: {
      const ValuFmt& f = kind == kVkCvtPkFp8F32 ? kValuFmtE4m3 : kValuFmtE5m2;
      o.a = valu_pack(valu_gen_fp8_input(r0, f), valu_gen_fp8_input(r1, f));
      break;
    }
    case kVkCvtF32Fp8: case kVkCvtF32Bf8: {
      // set * 64 + lane walks all 256 codes; NaN (and Inf) codes step aside
      const int imm = kValuOpImm[op];
      uint32_t code = (uint32_t)(set * 64 + lane);
      const bool bad = kind == kVkCvtF32Fp8 ? (code & 0x7Fu) == 0x7Fu : (code & 0x7Cu) == 0x7Cu;
      if (bad) code &= 0x83u;
      o.a = (valu_lo(r0) & ~(0xFFu << (8 * imm))) | code << (8 * imm);
      break;
    }
    case kVkCvtScalePkF32Fp4: {
      // lane walks the 16 codes in both nibbles
      const int imm = kValuOpImm[op];
      const uint32_t byte = (uint32_t)(lane & 15) | (uint32_t)((lane >> 2) + 4 * set & 15) << 4;
      o.a = (valu_lo(r0) & ~(0xFFu << (8 * imm))) | byte << (8 * imm);
      o.b = valu_f32_pow2((int)(r1 % 41u) - 20);
      break;
    }
    case kVkCvtScalePkFp4F32: {
      const int ex = (int)(r1 % 41u) - 20;
      uint32_t x[2];
      const uint64_t rr[2] = {r0, r3};
      for (int i = 0; i < 2; ++i) {
        const uint32_t bits = valu_gen_fp8_input(rr[i], kValuFmtE2m1);
        x[i] = f32_bits(std::ldexp(valu_f32(bits), ex));
      }
      o.a = valu_pack(x[0], x[1]);
      o.b = valu_f32_pow2(ex);
      break;
    }
    case kVkMbcnt:
      o.b = valu_lo(r1) & 0xFFFFu;
      break;
    case kVkCmpMask:
      if ((r3 & 3u) == 0) o.b = o.a;
      break;
    // consensus inputs: one per (set, lane)
    case kVkExpF32:
      o.a = valu_gen_f32(r0, -10, 5);
      break;
    case kVkLogF32: case kVkRsqF32: case kVkSqrtF32:
      o.a = valu_gen_f32(r0, -60, 60) & 0x7FFFFFFFu;
      break;
    case kVkRcpF32:
      o.a = valu_gen_f32(r0, -60, 60);
      break;
    case kVkSinF32: case kVkCosF32:
      o.a = valu_gen_f32(r0, -12, 7);
      break;
    case kVkRcpF64:
      o.a = valu_gen_f64(r0, -300, 300);
      break;
    case kVkRsqF64:
      o.a = valu_gen_f64(r0, -300, 300) & 0x7FFFFFFFFFFFFFFFull;
      break;
    case kVkCvtSrFp8F32:
      o.a = valu_gen_fp8_input(r0, kValuFmtE4m3);
      break;
    default:
      break;  // raw 64-bit random words
  }
  return o;
}

struct ValuProblem {
  // [set * 64 + lane]; a consensus op has its kValuConsInputs inputs instead
  std::vector<uint64_t> a, b, c, expected;
};

// Operands and expected words of one op; consensus ops get no `expected`.
// Throws when an operand or a result breaks its op's condition.
inline ValuProblem valu_problem(int op) {
  if (op < 0 || op >= kValuOps) throw std::invalid_argument("valu: op index out of range");
  ValuProblem p;
  const bool consensus = kValuOpGroup[op] == kValuGroupConsensus;
  const size_t n = consensus ? (size_t)kValuConsInputs : (size_t)kValuSets * 64;
  p.a.resize(n), p.b.resize(n), p.c.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const ValuOperands o = valu_operands(op, (int)(i / 64), (int)(i % 64));
    p.a[i] = o.a, p.b[i] = o.b, p.c[i] = o.c;
  }
  if (consensus) {
    for (size_t i = 0; i < n; ++i)
      valu_check_consensus_operand(kValuOpKind[op], p.a[i], p.b[i]);
    return p;
  }
  p.expected.resize(n);
  for (int s = 0; s < kValuSets; ++s)
    valu_ref_wave(op, &p.a[s * 64], &p.b[s * 64], &p.c[s * 64], &p.expected[s * 64]);
  return p;
}

// The device table: kValuOps x kValuSets x 64 records of kValuRecWords words
// (a consensus op uses the first kValuConsInputs of its records).
inline std::vector<uint32_t> valu_build_table() {
  std::vector<uint32_t> tab((size_t)kValuOps * kValuSets * 64 * kValuRecWords, 0u);
  for (int op = 0; op < kValuOps; ++op) {
    const ValuProblem p = valu_problem(op);
    for (size_t i = 0; i < p.a.size(); ++i) {
      uint32_t* r = &tab[((size_t)op * kValuSets * 64 + i) * kValuRecWords];
      r[0] = valu_lo(p.a[i]), r[1] = valu_hi(p.a[i]);
      r[2] = valu_lo(p.b[i]), r[3] = valu_hi(p.b[i]);
      r[4] = valu_lo(p.c[i]), r[5] = valu_hi(p.c[i]);
      if (!p.expected.empty())
        r[6] = valu_lo(p.expected[i]), r[7] = valu_hi(p.expected[i]);
    }
  }
  return tab;
}

// hash(op, input index, result bits) of the consensus digests: splitmix64
// finaliser.  The device folds the same function; a digest is the wrapping
// sum over all inputs of an op, so the order of the inputs does not matter.
VALIDATOR_HD inline uint64_t valu_digest_term(uint32_t op, uint32_t index, uint64_t bits) {
  uint64_t z = bits + ((uint64_t)op << 32 | index) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
