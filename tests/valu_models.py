"""Models of the vector-ALU check's ops, written for the tests from IEEE-754,
the OCP 8-bit / MX definitions and the ISA text, never by calling the native
reference: `fractions.Fraction` with its own round-to-nearest-even rounder,
its own e4m3 / e5m2 / e2m1 coders and its own lane-permutation functions.
Shared by test_valu_check_cpu.py (against `valu_reference()`) and
test_valu_check.py (against the hardware, through `valu_probe`)."""

import json
import math
from fractions import Fraction

F32 = (8, 23, 127)
F64 = (11, 52, 1023)
F16 = (5, 10, 15)
BF16 = (8, 7, 127)
E4M3 = (4, 3, 7)
E5M2 = (5, 2, 15)
E2M1 = (2, 1, 1)


def decode(fmt, code):
    """Code -> Fraction, or None for Inf / NaN (OCP: e4m3 has one NaN and no
    Inf, e2m1 has neither)."""
    ebits, mbits, bias = fmt
    sign = -1 if (code >> (ebits + mbits)) & 1 else 1
    e = (code >> mbits) & ((1 << ebits) - 1)
    m = code & ((1 << mbits) - 1)
    if fmt == E4M3:
        if e == 15 and m == 7:
            return None
    elif fmt != E2M1 and e == (1 << ebits) - 1:
        return None
    if e == 0:
        return sign * Fraction(m, 1 << mbits) * Fraction(2) ** (1 - bias)
    return sign * (1 + Fraction(m, 1 << mbits)) * Fraction(2) ** (e - bias)


def is_tie(fmt, x):
    """Is the exact value x halfway between two neighbours of fmt?"""
    ebits, mbits, bias = fmt
    if x == 0:
        return False
    mag = abs(x)
    e = max(math.floor(math.log2(mag)) if mag >= Fraction(2) ** (1 - bias) else 1 - bias,
            1 - bias)
    while Fraction(2) ** e > mag and e > 1 - bias:
        e -= 1
    while Fraction(2) ** (e + 1) <= mag:
        e += 1
    q = mag / Fraction(2) ** (e - mbits)
    return q.denominator == 2


def rne(fmt, x, neg_zero=False):
    """Round the exact Fraction x to fmt, nearest even, subnormals kept; the
    sign of a zero result is the sign of x, or `neg_zero` for an exact 0."""
    ebits, mbits, bias = fmt
    top = ebits + mbits
    if x == 0:
        return (1 << top) if neg_zero else 0
    sign = (1 << top) if x < 0 else 0
    mag = abs(x)
    emin = 1 - bias
    e = emin
    while Fraction(2) ** (e + 1) <= mag:
        e += 1
    q = mag / Fraction(2) ** (e - mbits)  # in units of the ulp at e
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    if n == 2 << mbits:
        n >>= 1
        e += 1
    if n < 1 << mbits:
        return sign | n
    return sign | ((e + bias) << mbits) | (n - (1 << mbits))


def fma_bits(fmt, a, b, c):
    x, y, z = decode(fmt, a), decode(fmt, b), decode(fmt, c)
    top = fmt[0] + fmt[1]
    pneg = ((a >> top) ^ (b >> top)) & 1
    cneg = (c >> top) & 1
    return rne(fmt, x * y + z, neg_zero=bool(pneg and cneg))


def add_bits(fmt, a, b):
    top = fmt[0] + fmt[1]
    return rne(fmt, decode(fmt, a) + decode(fmt, b),
               neg_zero=bool((a >> top) & (b >> top) & 1))


def mul_bits(fmt, a, b):
    top = fmt[0] + fmt[1]
    return rne(fmt, decode(fmt, a) * decode(fmt, b),
               neg_zero=bool(((a >> top) ^ (b >> top)) & 1))


def lo(v):
    return v & 0xFFFFFFFF


def hi(v):
    return v >> 32


def pack(l, h):
    return l | (h << 32)


def h0(v):
    return v & 0xFFFF


def h1(v):
    return (v >> 16) & 0xFFFF


def s32(v):
    return v - (1 << 32) if v & 0x80000000 else v


def bitop3(a, b, c, table):
    r = 0
    for i in range(32):
        idx = ((a >> i) & 1) << 2 | ((b >> i) & 1) << 1 | ((c >> i) & 1)
        r |= ((table >> idx) & 1) << i
    return r


def perm(a, b, sel):
    src = pack(b, a)
    r = 0
    for i in range(4):
        s = (sel >> (8 * i)) & 0xFF
        assert s <= 7 or s == 0x0C
        r |= (0 if s == 0x0C else (src >> (8 * s)) & 0xFF) << (8 * i)
    return r


def frexp_mant(x):
    if x == 0:
        return x
    mag = abs(x)
    while mag >= 1:
        mag /= 2
    while mag < Fraction(1, 2):
        mag *= 2
    return mag if x > 0 else -mag


def round_half_even(x):
    n = math.floor(x)
    rem = x - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return n


def scale_exp(bits):
    assert bits & 0x807FFFFF == 0 and 0 < (bits >> 23) < 255, "scale is no power of two"
    return (bits >> 23) - 127


def byte_insert(old, byte, sel):
    return (old & ~(0xFF << (8 * sel)) & 0xFFFFFFFF) | (byte << (8 * sel))


def lane_model(name, a, b, c):
    """One lane of one lane-wise op, from the definitions."""
    base, _, imm = name.partition(" ")
    sel = int(imm.split(":")[1], 0) if ":" in imm else 0
    al, ah, bl, bh, cl, ch = lo(a), hi(a), lo(b), hi(b), lo(c), hi(c)
    m32 = 0xFFFFFFFF
    if base == "v_fma_f32":
        return fma_bits(F32, al, bl, cl)
    if base == "v_add_f32":
        return add_bits(F32, al, bl)
    if base == "v_mul_f32":
        return mul_bits(F32, al, bl)
    if base == "v_pk_fma_f32":
        return pack(fma_bits(F32, al, bl, cl), fma_bits(F32, ah, bh, ch))
    if base == "v_pk_add_f32":
        return pack(add_bits(F32, al, bl), add_bits(F32, ah, bh))
    if base == "v_pk_mul_f32":
        return pack(mul_bits(F32, al, bl), mul_bits(F32, ah, bh))
    if base in ("v_min_f32", "v_max_f32", "v_med3_f32"):
        vals = sorted([(decode(F32, v), v) for v in ((al, bl, cl) if base == "v_med3_f32"
                                                       else (al, bl))])
        assert len({v[0] for v in vals}) == len(vals), "operands must differ in value"
        return vals[{"v_min_f32": 0, "v_max_f32": -1, "v_med3_f32": 1}[base]][1]
    if base == "v_ldexp_f32":
        return rne(F32, decode(F32, al) * Fraction(2) ** s32(bl), neg_zero=bool(al >> 31))
    if base == "v_frexp_mant_f32":
        return rne(F32, frexp_mant(decode(F32, al)), neg_zero=bool(al >> 31))
    if base == "v_rndne_f32":
        return rne(F32, Fraction(round_half_even(decode(F32, al))), neg_zero=bool(al >> 31)) \
            | (al & 0x80000000)
    if base == "v_fma_f64":
        return fma_bits(F64, a, b, c)
    if base == "v_add_f64":
        return add_bits(F64, a, b)
    if base == "v_mul_f64":
        return mul_bits(F64, a, b)
    if base == "v_ldexp_f64":
        return rne(F64, decode(F64, a) * Fraction(2) ** s32(bl), neg_zero=bool(a >> 63))
    if base == "v_pk_fma_f16":
        return fma_bits(F16, h0(al), h0(bl), h0(cl)) | fma_bits(F16, h1(al), h1(bl), h1(cl)) << 16
    if base == "v_pk_add_f16":
        return add_bits(F16, h0(al), h0(bl)) | add_bits(F16, h1(al), h1(bl)) << 16
    if base == "v_pk_mul_f16":
        return mul_bits(F16, h0(al), h0(bl)) | mul_bits(F16, h1(al), h1(bl)) << 16
    if base in ("v_dot2c_f32_f16", "v_dot2c_f32_bf16"):
        f = F16 if base.endswith("_f16") else BF16
        return rne(F32, decode(f, h0(al)) * decode(f, h0(bl))
                   + decode(f, h1(al)) * decode(f, h1(bl)) + decode(F32, cl))
    if base == "v_mad_u64_u32":
        return (al * bl + c) & (2 ** 64 - 1)
    if base == "v_mul_hi_u32":
        return (al * bl) >> 32
    if base == "v_mul_lo_u32":
        return (al * bl) & m32
    if base == "v_mul_i32_i24":
        sx = lambda v: (v & 0xFFFFFF) - (1 << 24 if v & 0x800000 else 0)  # noqa: E731
        return (sx(al) * sx(bl)) & m32
    if base == "v_add_co_u32+v_addc_co_u32":
        return (a + b) & (2 ** 64 - 1)
    if base == "v_sub_co_u32+v_subb_co_u32":
        return (a - b) & (2 ** 64 - 1)
    if base == "v_lshlrev_b32":
        return (al << (bl & 31)) & m32
    if base == "v_lshrrev_b32":
        return al >> (bl & 31)
    if base == "v_ashrrev_i32":
        return (s32(al) >> (bl & 31)) & m32
    if base == "v_lshlrev_b64":
        return (a << (bl & 63)) & (2 ** 64 - 1)
    if base == "v_lshrrev_b64":
        return a >> (bl & 63)
    if base == "v_ashrrev_i64":
        return ((a - (1 << 64 if a >> 63 else 0)) >> (bl & 63)) & (2 ** 64 - 1)
    if base == "v_bfe_u32":
        return (al >> (bl & 31)) & ((1 << (cl & 31)) - 1)
    if base == "v_bfi_b32":
        return (al & bl) | (~al & cl & m32)
    if base == "v_perm_b32":
        return perm(al, bl, cl)
    if base == "v_alignbit_b32":
        return (pack(bl, al) >> (cl & 31)) & m32
    if base == "v_sad_u8":
        return (cl + sum(abs(((al >> s) & 0xFF) - ((bl >> s) & 0xFF))
                         for s in (0, 8, 16, 24))) & m32
    if base == "v_bcnt_u32_b32":
        return (bin(al).count("1") + bl) & m32
    if base == "v_ffbh_u32":
        return 32 - al.bit_length()
    if base == "v_bfrev_b32":
        return int(format(al, "032b")[::-1], 2)
    if base == "v_bitop3_b32":
        return bitop3(al, bl, cl, sel)
    if base in ("v_dot4_i32_i8", "v_dot4_u32_u8"):
        sx = (lambda v: v - 256 if v & 0x80 else v) if base.endswith("i8") else (lambda v: v)
        return (cl + sum(sx((al >> s) & 0xFF) * sx((bl >> s) & 0xFF)
                         for s in (0, 8, 16, 24))) & m32
    if base == "v_cmp_lt_i32+v_cndmask_b32":
        return cl if s32(al) < s32(bl) else ch
    if base == "v_cvt_f16_f32":
        return rne(F16, decode(F32, al), neg_zero=bool(al >> 31))
    if base == "v_cvt_pk_bf16_f32":
        return rne(BF16, decode(F32, al), bool(al >> 31)) | rne(BF16, decode(F32, ah), bool(ah >> 31)) << 16
    if base in ("v_cvt_i32_f32", "v_cvt_u32_f32"):
        x = decode(F32, al)
        n = math.floor(abs(x)) * (1 if x >= 0 else -1)  # toward zero
        assert (-2 ** 31 <= n < 2 ** 31) if base == "v_cvt_i32_f32" else (0 <= n < 2 ** 32)
        return n & m32
    if base == "v_cvt_f32_i32":
        return rne(F32, Fraction(s32(al)))
    if base == "v_cvt_f32_u32":
        return rne(F32, Fraction(al))
    if base in ("v_cvt_pk_fp8_f32", "v_cvt_pk_bf8_f32"):
        f, limit = (E4M3, 448) if "fp8" in base else (E5M2, 57344)
        x, y = decode(F32, al), decode(F32, ah)
        assert abs(x) <= limit and abs(y) <= limit, "fp8 input out of range"
        pair = rne(f, x, bool(al >> 31)) | rne(f, y, bool(ah >> 31)) << 8
        return (cl & 0xFFFF) | pair << 16 if sel else (cl & 0xFFFF0000) | pair
    if base in ("v_cvt_f32_fp8", "v_cvt_f32_bf8"):
        f = E4M3 if "fp8" in base else E5M2
        code = (al >> (8 * sel)) & 0xFF
        v = decode(f, code)
        assert v is not None, "NaN / Inf code"
        return rne(F32, v, neg_zero=bool(code >> 7))
    if base == "v_cvt_scalef32_pk_f32_fp4":
        byte = (al >> (8 * sel)) & 0xFF
        s = Fraction(2) ** scale_exp(bl)
        out = [rne(F32, decode(E2M1, n) * s, neg_zero=bool(n >> 3)) for n in (byte & 15, byte >> 4)]
        return pack(out[0], out[1])
    if base == "v_cvt_scalef32_pk_fp4_f32":
        s = Fraction(2) ** scale_exp(bl)
        nib = []
        for bits in (al, ah):
            x = decode(F32, bits) / s
            assert abs(x) <= 6, "|x / scale| > 6"
            nib.append(rne(E2M1, x, neg_zero=bool(bits >> 31)))
        return byte_insert(cl, nib[0] | nib[1] << 4, sel)
    raise KeyError(name)


# lane permutations, from the ISA text; None = no valid source
def dpp_source(ctrl, l):
    row, r = l & ~15, l & 15
    if ctrl.startswith("quad_perm:"):
        p = json.loads(ctrl.split(":")[1])
        return (l & ~3) | p[l & 3]
    kind, _, n = ctrl.partition(":")
    n = int(n) if n else 0
    if kind == "row_shl":
        return l + n if r + n < 16 else None
    if kind == "row_shr":
        return l - n if r >= n else None
    if kind == "row_ror":
        return row | ((r - n) % 16)
    if kind == "wave_shl":
        return l + 1 if l < 63 else None
    if kind == "wave_rol":
        return (l + 1) % 64
    if kind == "wave_shr":
        return l - 1 if l > 0 else None
    if kind == "wave_ror":
        return (l - 1) % 64
    if kind == "row_mirror":
        return row | (15 - r)
    if kind == "row_half_mirror":
        return (l & ~7) | (7 - (l & 7))
    if kind == "row_bcast" and n == 15:
        return row - 1 if l >= 16 else l
    if kind == "row_bcast" and n == 31:
        return 31 if l >= 32 else l
    raise KeyError(ctrl)


def wave_model(name, a, b, c):
    """64 lanes of one op."""
    if name.startswith("v_mov_b32_dpp "):
        parts = name.split(" ")[1:]
        ctrl = parts[0]
        row_mask, bank_mask, bound = 0xF, 0xF, False
        for p in parts[1:]:
            k, v = p.split(":")
            if k == "row_mask":
                row_mask = int(v, 0)
            elif k == "bank_mask":
                bank_mask = int(v, 0)
            elif k == "bound_ctrl":
                bound = bool(int(v, 0))
        out = []
        for l in range(64):
            enabled = (row_mask >> (l >> 4)) & 1 and (bank_mask >> ((l >> 2) & 3)) & 1
            src = dpp_source(ctrl, l)
            old = lo(b[l])
            out.append(old if not enabled else lo(a[src]) if src is not None
                       else 0 if bound else old)
        return out
    if name == "v_readlane_b32":
        return [lo(a[(5, 23, 40, 62)[l & 3]]) for l in range(64)]
    if name == "v_readfirstlane_b32":
        return [lo(a[0])] * 64
    if name == "v_permlane16_swap_b32":
        # rows 1, 3 of the first register swap with rows 0, 2 of the second
        return [pack(lo(b[l - 16]), lo(b[l])) if (l >> 4) & 1 else pack(lo(a[l]), lo(a[l + 16]))
                for l in range(64)]
    if name == "v_permlane32_swap_b32":
        return [pack(lo(b[l - 32]), lo(b[l])) if l >= 32 else pack(lo(a[l]), lo(a[l + 32]))
                for l in range(64)]
    if name == "v_mbcnt_lo_u32_b32+v_mbcnt_hi_u32_b32":
        return [(lo(b[l]) + bin(a[l] & ((1 << l) - 1)).count("1")) & 0xFFFFFFFF
                for l in range(64)]
    if name == "v_cmp_lt_u32 (64-bit mask)":
        mask = sum(1 << l for l in range(64) if lo(a[l]) < lo(b[l]))
        return [mask] * 64
    return [lane_model(name, a[l], b[l], c[l]) for l in range(64)]
