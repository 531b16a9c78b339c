// valu_problems_selftest.cpp — stand-alone checks of the generator and host
// reference of the vector-ALU check (native/valu_problems.hpp).
//
// Built with -fsanitize=address,undefined by tests/test_valu_problems_native.py
// and run as a child process, so the generator, the integer rounder and the
// lane-permutation model run under the sanitizers.  Beyond that it asserts
// what can be stated without the code under test: hand-computed roundings,
// the triple on which fused and unfused multiply-add differ, that every
// permutation is one, that no record holds a NaN or an infinity, and that a
// violated constraint throws.

#include <cstdint>
#include <cstdio>
#include <set>
#include <stdexcept>
#include <string>
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

template <typename E, typename F>
bool throws(F f) {
  try {
    f();
  } catch (const E&) {
    return true;
  }
  return false;
}

int op_of(const char* name) { return valu_op_index(name); }

uint64_t lane_ref(const char* name, uint64_t a, uint64_t b, uint64_t c) {
  const int op = op_of(name);
  return valu_ref_lane(kValuOpKind[op], kValuOpImm[op], a, b, c);
}

void test_table() {
  CHECK(kValuOps == (int)(sizeof(kValuOpTable) / sizeof(kValuOpTable[0])));
  std::set<std::string> names;
  for (int i = 0; i < kValuOps; ++i) {
    CHECK(names.insert(kValuOpTable[i].name).second);
    CHECK(kValuOpTable[i].group == kValuOpGroup[i]);
    CHECK(op_of(kValuOpTable[i].name) == i);
    // groups are contiguous and in bit order
    if (i) CHECK(kValuOpGroup[i] >= kValuOpGroup[i - 1]);
  }
  CHECK(kValuOpGroup[0] == 0 && kValuOpGroup[kValuOps - 1] == kValuGroups - 1);
  CHECK(throws<std::invalid_argument>([] { valu_op_index("v_nonesuch"); }));
  uint64_t items = 0;
  for (int g = 0; g < kValuGroups; ++g) {
    CHECK(valu_items(g) > 0 && valu_items(g) % 64 == 0);
    items += valu_items(g);
  }
  CHECK(items == 64ull * ((uint64_t)kValuExactOps * kValuSets +
                          (uint64_t)kValuConsOps * kValuConsInputs));
  CHECK(valu_build_table().size() ==
        (size_t)kValuOps * kValuSets * 64 * kValuRecWords);
}

void test_rounder() {
  // f16: 1 + 2^-11 is a tie -> 1 (even); 1 + 3 * 2^-11 is a tie -> 1 + 2^-9
  CHECK(valu_rne(kValuFmtF16, ValuExact{false, 2049, -11}) == 0x3C00u);
  CHECK(valu_rne(kValuFmtF16, ValuExact{false, 2051, -11}) == 0x3C02u);
  CHECK(valu_rne(kValuFmtF16, ValuExact{true, 4097, -12}) == 0xBC00u);   // below the tie
  CHECK(valu_rne(kValuFmtF16, ValuExact{false, 4099, -12}) == 0x3C01u);  // above it
  // subnormals: 2^-24 is the smallest, 2^-25 a tie -> 0, 3 * 2^-25 a tie -> 2^-23
  CHECK(valu_rne(kValuFmtF16, ValuExact{false, 1, -24}) == 0x0001u);
  CHECK(valu_rne(kValuFmtF16, ValuExact{false, 1, -25}) == 0x0000u);
  CHECK(valu_rne(kValuFmtF16, ValuExact{true, 3, -25}) == 0x8002u);
  // the largest subnormal rounds up into the smallest normal
  CHECK(valu_rne(kValuFmtF16, ValuExact{false, 2047, -25}) == 0x0400u);
  CHECK(valu_rne(kValuFmtF16, ValuExact{false, 65504, 0}) == 0x7BFFu);
  CHECK(throws<std::domain_error>(
      [] { valu_rne(kValuFmtF16, ValuExact{false, 65520, 0}); }));
  CHECK(valu_rne(kValuFmtF16, ValuExact{true, 0, 0}) == 0x8000u);
  // bf16 of 1 + 2^-8 (tie -> 1) and 1 + 3 * 2^-8 (tie -> 1 + 2^-6)
  CHECK(valu_rne(kValuFmtBf16, valu_exact_f32(0x3F808000u)) == 0x3F80u);
  CHECK(valu_rne(kValuFmtBf16, valu_exact_f32(0x3F818000u)) == 0x3F82u);
  // e4m3: 448 is the largest; 17 is a tie between 16 and 18 -> 16; 2^-10 is a
  // tie between 0 and the smallest subnormal 2^-9 -> 0
  CHECK(valu_rne(kValuFmtE4m3, ValuExact{false, 448, 0}) == 0x7Eu);
  CHECK(valu_rne(kValuFmtE4m3, ValuExact{false, 17, 0}) == 0x58u);
  CHECK(valu_rne(kValuFmtE4m3, ValuExact{false, 19, 0}) == 0x5Au);
  CHECK(valu_rne(kValuFmtE4m3, ValuExact{true, 1, -10}) == 0x80u);
  CHECK(valu_rne(kValuFmtE4m3, ValuExact{false, 3, -10}) == 0x02u);
  CHECK(throws<std::domain_error>(
      [] { valu_rne(kValuFmtE4m3, ValuExact{false, 480, 0}); }));
  // e5m2: 57344 is the largest; 5 * 2^-17 is a subnormal tie -> 2^-15
  CHECK(valu_rne(kValuFmtE5m2, ValuExact{false, 57344, 0}) == 0x7Bu);
  CHECK(valu_rne(kValuFmtE5m2, ValuExact{false, 5, -18}) == 0x01u);
  // e2m1: 0 0.5 1 1.5 2 3 4 6; 2.5 -> 2, 3.5 -> 4, 5 -> 4, 0.25 -> 0, 0.75 -> 1
  CHECK(valu_rne(kValuFmtE2m1, ValuExact{false, 5, -1}) == 0x4u);
  CHECK(valu_rne(kValuFmtE2m1, ValuExact{false, 7, -1}) == 0x6u);
  CHECK(valu_rne(kValuFmtE2m1, ValuExact{false, 5, 0}) == 0x6u);
  CHECK(valu_rne(kValuFmtE2m1, ValuExact{false, 1, -2}) == 0x0u);
  CHECK(valu_rne(kValuFmtE2m1, ValuExact{true, 3, -2}) == 0xAu);
  CHECK(valu_rne(kValuFmtE2m1, ValuExact{false, 6, 0}) == 0x7u);
  // every code of every small format decodes and re-encodes to itself
  const ValuFmt* fmts[] = {&kValuFmtF16, &kValuFmtE4m3, &kValuFmtE5m2, &kValuFmtE2m1};
  for (const ValuFmt* f : fmts)
    for (uint32_t code = 0; code <= f->max_code; ++code) {
      CHECK(valu_rne(*f, valu_decode(*f, code)) == code);
      const uint32_t neg = code | 1u << (f->ebits + f->mbits);
      CHECK(valu_rne(*f, valu_decode(*f, neg)) == neg);
    }
}

void test_fused_versus_unfused() {
  // a = b = 1 + 2^-12, c = -(1 + 2^-11): a * b = 1 + 2^-11 + 2^-24 exactly.
  // Fused gives 2^-24; the separate multiply rounds to 1 + 2^-11 (a tie, to
  // even) and the add then gives +0.  The reference must keep the two apart
  // whatever the compiler's contraction default is.
  const uint32_t a = 0x3F800800u, b = 0x3F800800u, c = 0xBF801000u;
  CHECK(lane_ref("v_fma_f32", a, b, c) == 0x33800000u);
  const uint64_t prod = lane_ref("v_mul_f32", a, b, 0);
  CHECK(prod == 0x3F801000u);
  CHECK(lane_ref("v_add_f32", prod, c, 0) == 0x00000000u);
  CHECK(f32_bits(valu_add_rn(valu_mul_rn(valu_f32(a), valu_f32(b)), valu_f32(c))) == 0u);
  // the pinned record of the sweep holds this triple
  const ValuOperands o = valu_operands(op_of("v_fma_f32"), 0, 4);
  CHECK(valu_lo(o.a) == a && valu_lo(o.b) == b && valu_lo(o.c) == c);
  // f64 likewise: (1 + 2^-27)^2 = 1 + 2^-26 + 2^-54, a tie -> 1 + 2^-26
  const uint64_t t = 0x3FF0000002000000ull;
  CHECK(lane_ref("v_mul_f64", t, t, 0) == 0x3FF0000004000000ull);
  CHECK(lane_ref("v_fma_f64", t, t, 0xBFF0000004000000ull) == 0x3C90000000000000ull);
  // f16, by the integer path: (1 + 2^-5)(1 + 2^-6) is a tie -> even
  CHECK(lane_ref("v_pk_mul_f16", 0x3C20u, 0x3C10u, 0) == 0x3C30u);
  CHECK(lane_ref("v_pk_fma_f16", 0x3C20u, 0x3C10u, 0xBC30u) == 0x1000u);  // 2^-11 left
  CHECK(lane_ref("v_pk_add_f16", 0x8000u, 0x0000u, 0) == 0x0000u);        // -0 + 0 = +0
  CHECK(lane_ref("v_pk_add_f16", 0x8000u, 0x8000u, 0) == 0x8000u);
  CHECK(lane_ref("v_pk_mul_f16", 0x8000u, 0x4500u, 0) == 0x8000u);        // -0 * 5 = -0
}

void test_integer_ops() {
  CHECK(lane_ref("v_mad_u64_u32", 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFFFFFFFFFull) ==
        0xFFFFFFFE00000000ull);
  CHECK(lane_ref("v_mul_hi_u32", 0xFFFFFFFFu, 0xFFFFFFFFu, 0) == 0xFFFFFFFEu);
  CHECK(lane_ref("v_mul_i32_i24", 0x00FFFFFFu, 0x00000002u, 0) == 0xFFFFFFFEu);  // -1 * 2
  CHECK(lane_ref("v_bfe_u32", 0xABCD1234u, 8, 12) == 0xD12u);
  CHECK(lane_ref("v_bfe_u32", 0xABCD1234u, 8, 0) == 0u);
  CHECK(lane_ref("v_bfi_b32", 0x0000FFFFu, 0x12345678u, 0x9ABCDEF0u) == 0x9ABC5678u);
  CHECK(lane_ref("v_perm_b32", 0x44556677u, 0x00112233u, 0x0C070400u) == 0x00447733u);
  CHECK(throws<std::invalid_argument>(
      [] { lane_ref("v_perm_b32", 1, 2, 0x00000008u); }));
  CHECK(lane_ref("v_alignbit_b32", 0x00000001u, 0x80000000u, 31) == 0x00000003u);
  CHECK(lane_ref("v_sad_u8", 0x00FF10F0u, 0xFF000FF1u, 5) == 5u + 255 + 255 + 1 + 1);
  CHECK(lane_ref("v_ffbh_u32", 0, 0, 0) == 32u && lane_ref("v_ffbh_u32", 1, 0, 0) == 31u);
  CHECK(lane_ref("v_bfrev_b32", 0x00000001u, 0, 0) == 0x80000000u);
  CHECK(lane_ref("v_bitop3_b32 bitop3:0x96", 0xF0u, 0xCCu, 0xAAu) == 0x96u);
  CHECK(lane_ref("v_bitop3_b32 bitop3:0xca", 0xF0u, 0xCCu, 0xAAu) == 0xCAu);
  CHECK(lane_ref("v_dot4_i32_i8", 0x80FF0102u, 0x7F020304u, 10) ==
        (uint32_t)(10 + (-128 * 127) + (-1 * 2) + 1 * 3 + 2 * 4));
  CHECK(lane_ref("v_dot4_u32_u8", 0x80FF0102u, 0x7F020304u, 10) ==
        10u + 128 * 127 + 255 * 2 + 3 + 8);
  CHECK(lane_ref("v_ashrrev_i64", 0x8000000000000000ull, 63, 0) == ~0ull);
}

void test_conversions() {
  CHECK(lane_ref("v_cvt_f32_fp8 byte_sel:2", 0x007E0000u, 0, 0) == f32_bits(448.0f));
  CHECK(lane_ref("v_cvt_f32_fp8 byte_sel:0", 0x81u, 0, 0) == f32_bits(-0.001953125f));
  CHECK(lane_ref("v_cvt_f32_bf8 byte_sel:3", 0x7B000000u, 0, 0) == f32_bits(57344.0f));
  // NaN / Inf codes are refused, as valu_probe refuses them
  CHECK(throws<std::invalid_argument>(
      [] { lane_ref("v_cvt_f32_fp8 byte_sel:0", 0x7Fu, 0, 0); }));
  CHECK(throws<std::invalid_argument>(
      [] { lane_ref("v_cvt_f32_bf8 byte_sel:1", 0x7C00u, 0, 0); }));
  // 17 and 19 are ties of e4m3; word_sel 1 keeps the low half of `old`
  CHECK(lane_ref("v_cvt_pk_fp8_f32 word_sel:1",
                 valu_pack(f32_bits(17.0f), f32_bits(-19.0f)), 0, 0xAAAA5555u) == 0xDA585555u);
  CHECK(lane_ref("v_cvt_pk_fp8_f32 word_sel:0",
                 valu_pack(f32_bits(17.0f), f32_bits(-19.0f)), 0, 0xAAAA5555u) == 0xAAAADA58u);
  CHECK(throws<std::invalid_argument>([] {
    lane_ref("v_cvt_pk_fp8_f32 word_sel:0", valu_pack(f32_bits(449.0f), 0), 0, 0);
  }));
  CHECK(throws<std::invalid_argument>([] {
    lane_ref("v_cvt_pk_bf8_f32 word_sel:0", valu_pack(0, f32_bits(-57345.0f)), 0, 0);
  }));
  // fp4: codes 0x7 (6) and 0x9 (-0.5) scaled by 2^3
  CHECK(lane_ref("v_cvt_scalef32_pk_f32_fp4 byte_sel:1", 0x00009700u, f32_bits(8.0f), 0) ==
        valu_pack(f32_bits(48.0f), f32_bits(-4.0f)));
  // 20 / 8 = 2.5 -> 2 (code 4), -28 / 8 = -3.5 -> -4 (code 0xE)
  CHECK(lane_ref("v_cvt_scalef32_pk_fp4_f32 byte_sel:3",
                 valu_pack(f32_bits(20.0f), f32_bits(-28.0f)), f32_bits(8.0f),
                 0x11223344u) == 0xE4223344u);
  CHECK(throws<std::invalid_argument>([] {
    lane_ref("v_cvt_scalef32_pk_fp4_f32 byte_sel:0", valu_pack(f32_bits(7.0f), 0),
             f32_bits(1.0f), 0);
  }));
  CHECK(throws<std::invalid_argument>([] {
    lane_ref("v_cvt_scalef32_pk_fp4_f32 byte_sel:0", 0, f32_bits(3.0f), 0);
  }));
  CHECK(lane_ref("v_cvt_f16_f32", 0x3F801000u, 0, 0) == 0x3C00u);  // tie -> even
  CHECK(lane_ref("v_cvt_f16_f32", 0x33800000u, 0, 0) == 0x0001u);  // 2^-24
  CHECK(lane_ref("v_cvt_f32_u32", 0x01000001u, 0, 0) == 0x4B800000u);  // 2^24 + 1: tie
  CHECK(throws<std::invalid_argument>(
      [] { lane_ref("v_cvt_i32_f32", f32_bits(3e9f), 0, 0); }));
}

void test_nan_is_refused() {
  const uint32_t nan32 = 0x7FC00000u, inf32 = 0x7F800000u;
  CHECK(throws<std::invalid_argument>([&] { lane_ref("v_fma_f32", nan32, 1, 1); }));
  CHECK(throws<std::invalid_argument>([&] { lane_ref("v_add_f32", 1, inf32, 0); }));
  CHECK(throws<std::invalid_argument>(
      [] { lane_ref("v_fma_f64", 0x7FF8000000000000ull, 0, 0); }));
  CHECK(throws<std::invalid_argument>([] { lane_ref("v_pk_add_f16", 0x7E00u, 0, 0); }));
  // a result that overflows is refused too
  CHECK(throws<std::domain_error>(
      [] { lane_ref("v_mul_f32", 0x7F000000u, 0x7F000000u, 0); }));
  CHECK(throws<std::domain_error>([] { lane_ref("v_pk_mul_f16", 0x7BFFu, 0x7BFFu, 0); }));
  // which of two equal values min / max return is not claimed
  CHECK(throws<std::invalid_argument>(
      [] { lane_ref("v_min_f32", 0x80000000u, 0x00000000u, 0); }));
  // dot2 operands must be small integers
  CHECK(throws<std::invalid_argument>(
      [] { lane_ref("v_dot2c_f32_f16", 0x3C003800u, 0x3C003C00u, 0); }));  // 0.5
  CHECK(throws<std::invalid_argument>([] {
    valu_check_consensus_operand(kVkLogF32, 0x80000000u | 0x3F800000u, 0);
  }));
  CHECK(throws<std::invalid_argument>(
      [] { valu_check_consensus_operand(kVkCvtSrFp8F32, f32_bits(500.0f), 0); }));
}

void test_lane_model() {
  // every control with all sources valid is a map into 0..63; the rotations,
  // mirrors and quad_perm [1,0,3,2] are permutations
  const int perms[] = {0xB1, 0x121, 0x12F, 0x134, 0x13C, 0x140, 0x141};
  for (int ctrl : perms) {
    std::set<int> seen;
    for (int l = 0; l < 64; ++l) {
      const int s = valu_dpp_source(ctrl, l);
      CHECK(s >= 0 && s < 64);
      seen.insert(s);
    }
    CHECK(seen.size() == 64);
  }
  for (int l = 0; l < 64; ++l) {
    CHECK(valu_dpp_source(0x101, l) == ((l & 15) == 15 ? -1 : l + 1));
    CHECK(valu_dpp_source(0x11F, l) == ((l & 15) == 15 ? l - 15 : -1));
    CHECK(valu_dpp_source(0x130, l) == (l == 63 ? -1 : l + 1));
    CHECK(valu_dpp_source(0x138, l) == (l == 0 ? -1 : l - 1));
  }
  CHECK(throws<std::invalid_argument>([] { valu_dpp_source(0x150, 0); }));
  // the swaps move every value exactly once
  std::vector<uint64_t> a(64), b(64), c(64, 0), out(64);
  for (int l = 0; l < 64; ++l) a[l] = 100 + l, b[l] = 200 + l;
  for (const char* name : {"v_permlane16_swap_b32", "v_permlane32_swap_b32"}) {
    valu_ref_wave(op_of(name), a.data(), b.data(), c.data(), out.data());
    std::multiset<uint32_t> in, got;
    for (int l = 0; l < 64; ++l) {
      in.insert(valu_lo(a[l])), in.insert(valu_lo(b[l]));
      got.insert(valu_lo(out[l])), got.insert(valu_hi(out[l]));
    }
    CHECK(in == got);
  }
  valu_ref_wave(op_of("v_permlane32_swap_b32"), a.data(), b.data(), c.data(), out.data());
  CHECK(out[0] == valu_pack(100, 132) && out[40] == valu_pack(208, 240));
  CHECK(throws<std::invalid_argument>([&] {
    valu_ref_wave(op_of("v_exp_f32"), a.data(), b.data(), c.data(), out.data());
  }));
}

void test_records() {
  // no record of the sweep holds a NaN or an infinity, in or out; generating
  // them does not throw
  for (int op = 0; op < kValuOps; ++op) {
    const ValuProblem p = valu_problem(op);
    CHECK(p.a.size() == (kValuOpGroup[op] == kValuGroupConsensus
                             ? (size_t)kValuConsInputs : (size_t)kValuSets * 64));
    CHECK(p.expected.empty() == (kValuOpGroup[op] == kValuGroupConsensus));
    const int g = kValuOpGroup[op], kind = kValuOpKind[op];
    for (size_t i = 0; i < p.expected.size(); ++i) {
      if (g == kValuGroupF32) {
        CHECK(valu_f32_finite(valu_lo(p.expected[i])));
        CHECK(valu_f32_finite(valu_lo(p.a[i])));
      }
      if (g == kValuGroupF64) CHECK(valu_f64_finite(p.expected[i]));
      if (kind == kVkPkFmaF16 || kind == kVkPkAddF16 || kind == kVkPkMulF16)
        CHECK(valu_f16_finite(valu_lo(p.expected[i]) & 0xFFFFu) &&
              valu_f16_finite(valu_lo(p.expected[i]) >> 16));
    }
  }
  // the digest term is the splitmix64 finaliser: published value for state 0
  CHECK(valu_digest_term(0, 0, 0x9E3779B97F4A7C15ull) == 0xE220A8397B1DCDAFull);
}

}  // namespace

int main() {
  test_table();
  test_rounder();
  test_fused_versus_unfused();
  test_integer_ops();
  test_conversions();
  test_nan_is_refused();
  test_lane_model();
  test_records();
  if (g_failures) {
    std::fprintf(stderr, "%d of %d checks failed\n", g_failures, g_checks);
    return 1;
  }
  std::printf("%d checks passed\n", g_checks);
  return 0;
}
