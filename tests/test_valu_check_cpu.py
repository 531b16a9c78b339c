"""CPU tests of the vector-ALU check: the pure verdict (`summarize_valu`), the
report wiring against a stub native module, and `valu_reference()` (host
only) against models written here, from IEEE-754 / OCP / the ISA text, never
by calling the native ones: `fractions.Fraction` with its own RNE rounder for
the floating ops, its own e4m3 / e5m2 / e2m1 coders and its own
lane-permutation functions."""

import importlib
import json
import struct
import sys
from fractions import Fraction

import pytest

from k8s_operator_libs_amd.validation import (
    gpu_health,
    gpu_health_check,
    load_native_validator,
    summarize_valu,
    valu_check,
)

# the package exports the function `valu_check` under the module's own name
valu_module = importlib.import_module("k8s_operator_libs_amd.validation.valu_check")

XCCS, CUS_PER_XCC = 2, 3
BITS = ["f32", "f64", "f16", "int", "convert", "crosslane", "consensus"]
CONS_OPS = ["v_exp_f32", "v_rcp_f64", "v_prng_b32"]
GOOD = (0x1111, 0x2222, 0x3333)
ITEMS = [10, 20, 30, 40, 50, 60, 70]
REPS = 2


def _key(xcc, se, sh, cu):
    return (xcc << 8) | (se << 5) | (sh << 4) | cu


def _raw(skip_slots=(), fail=None, digests=None, compute_units=XCCS * CUS_PER_XCC,
         compared_delta=None, records=()):
    """A fully covered synthetic device minus ``skip_slots`` ((key, simd)
    pairs); ``fail`` maps (key, simd) -> fail_mask, ``digests`` maps (key,
    simd) -> the list of digest tuples that slot reports."""
    fail, digests = fail or {}, digests or {}
    units = []
    for xcc in range(XCCS):
        for cu in range(CUS_PER_XCC):
            key = _key(xcc, se=cu % 2, sh=0, cu=cu)
            for simd in range(4):
                if (key, simd) in skip_slots:
                    continue
                units.append({
                    "key": key, "xcc": xcc, "hw_bits": key & 0xFF,
                    "simd": simd, "waves": 2,
                    "fail_mask": fail.get((key, simd), 0),
                    "digests": [list(t) for t in digests.get((key, simd), [GOOD])],
                })
    waves = 2 * len(units)
    compared = [waves * REPS * n for n in ITEMS]
    for g, d in (compared_delta or {}).items():
        compared[g] += d
    return {
        "compute_units": compute_units,
        "cus_covered": len({u["key"] for u in units}),
        "simd_slots_covered": len(units),
        "waves_run": waves,
        "rounds": 1,
        "failed_slots": sum(1 for u in units if u["fail_mask"]),
        "units": units,
        "elapsed_ms": 2.5,
        "reps": REPS,
        "compared": compared,
        "items": list(ITEMS),
        "consensus_ops": list(CONS_OPS),
        "records": list(records),
        "records_dropped": 0,
        "error_count": len(records),
    }


ALL_SLOTS = [(_key(x, c % 2, 0, c), s) for x in range(XCCS) for c in range(CUS_PER_XCC)
             for s in range(4)]


# -- summarize_valu -----------------------------------------------------------


def test_fail_bits_are_the_documented_seven():
    assert list(valu_module.FAIL_BITS) == BITS


def test_summary_healthy_full_coverage():
    s = summarize_valu(_raw())
    assert s["healthy"] is True
    assert s["compute_units"] == 6 and s["cus_covered"] == 6
    assert s["simd_slots_covered"] == 24
    assert s["failing_units"] == [] and s["short_groups"] == []
    assert s["consensus_digests"] == dict(zip(CONS_OPS, GOOD))
    assert s["compared"] == s["compared_expected"] == [48 * REPS * n for n in ITEMS]
    assert s["failing_ops"] == [] and s["error_count"] == 0
    assert s["records_dropped"] == 0
    assert s["elapsed_ms"] == 2.5 and s["rounds"] == 1
    assert "units" not in s and "records" not in s


@pytest.mark.parametrize("bit,name", list(enumerate(BITS)))
def test_summary_decodes_each_fail_bit(bit, name):
    key = _key(1, se=1, sh=0, cu=1)
    s = summarize_valu(_raw(fail={(key, 2): 1 << bit}))
    assert s["healthy"] is False
    assert len(s["failing_units"]) == 1
    unit = s["failing_units"][0]
    assert (unit["xcc"], unit["se"], unit["sh"], unit["cu"]) == (1, 1, 0, 1)
    assert unit["simd"] == 2 and unit["key"] == key
    assert unit["failed"] == [name]


def test_summary_decodes_combined_mask_in_bit_order():
    key = _key(0, se=0, sh=0, cu=0)
    s = summarize_valu(_raw(fail={(key, 0): 0x7F, (key, 3): 0x54}))
    assert [u["failed"] for u in s["failing_units"]] == [
        BITS, ["f16", "convert", "consensus"]]
    assert [u["simd"] for u in s["failing_units"]] == [0, 3]


def test_summary_missing_cu_is_unhealthy():
    gone = _key(0, se=1, sh=0, cu=1)
    s = summarize_valu(_raw(skip_slots={(gone, i) for i in range(4)}))
    assert s["healthy"] is False
    assert s["uncovered_cus"] == 1 and s["cus_covered"] == 5
    assert s["failing_units"] == [] and s["short_groups"] == []


def test_summary_three_simd_cu_is_unhealthy():
    key = _key(1, se=0, sh=0, cu=0)
    s = summarize_valu(_raw(skip_slots={(key, 3)}))
    assert s["cus_covered"] == 6 and s["simd_slots_covered"] == 23
    assert s["healthy"] is False and s["failing_units"] == []


def test_one_deviant_digest_fails_only_that_slot_with_consensus():
    slot = (_key(1, se=0, sh=0, cu=2), 1)
    s = summarize_valu(_raw(digests={slot: [(0x1111, 0x2223, 0x3333)]}))
    assert s["healthy"] is False
    assert s["consensus_digests"] == dict(zip(CONS_OPS, GOOD))
    assert [(u["key"], u["simd"], u["failed"]) for u in s["failing_units"]] == [
        (slot[0], slot[1], ["consensus"])]


def test_deviant_digest_joins_the_bits_the_kernel_set():
    slot = (_key(0, se=1, sh=0, cu=1), 0)
    s = summarize_valu(_raw(fail={slot: 0x09}, digests={slot: [(1, 2, 3)]}))
    assert [u["failed"] for u in s["failing_units"]] == [["f32", "int", "consensus"]]
    # the kernel's own bit 6 is not listed twice
    s = summarize_valu(_raw(fail={slot: 0x40}, digests={slot: [(1, 2, 3)]}))
    assert [u["failed"] for u in s["failing_units"]] == [["consensus"]]


def test_slot_holding_two_tuples_fails():
    slot = (_key(0, se=0, sh=0, cu=0), 3)
    s = summarize_valu(_raw(digests={slot: [GOOD, (0x1111, 0x2222, 0x3334)]}))
    assert s["healthy"] is False
    assert s["consensus_digests"] == dict(zip(CONS_OPS, GOOD))
    assert [(u["key"], u["simd"], u["failed"]) for u in s["failing_units"]] == [
        (slot[0], slot[1], ["consensus"])]


def test_slot_without_a_digest_record_fails():
    slot = (_key(0, se=0, sh=0, cu=0), 3)
    s = summarize_valu(_raw(digests={slot: []}))
    assert s["healthy"] is False
    assert [u["failed"] for u in s["failing_units"]] == [["consensus"]]


def test_three_against_three_has_no_majority():
    # a 2 x 3 CU device seen on one SIMD per CU: six slots, split evenly at
    # one op; the other ops still have their majority
    keep = [(_key(x, c % 2, 0, c), 0) for x in range(XCCS) for c in range(CUS_PER_XCC)]
    skip = set(ALL_SLOTS) - set(keep)
    other = (0x1111, 0x9999, 0x3333)
    s = summarize_valu(_raw(skip_slots=skip, digests={k: [other] for k in keep[:3]}))
    assert s["healthy"] is False
    assert s["consensus_digests"] == {"v_exp_f32": 0x1111, "v_rcp_f64": None,
                                      "v_prng_b32": 0x3333}
    # the same split on a fully covered device, as the only defect
    half = ALL_SLOTS[:12]
    s = summarize_valu(_raw(digests={k: [other] for k in half}))
    assert s["cus_covered"] == 6 and s["simd_slots_covered"] == 24
    assert s["consensus_digests"]["v_rcp_f64"] is None
    assert s["healthy"] is False


def test_short_count_is_unhealthy_with_zero_errors():
    s = summarize_valu(_raw(compared_delta={4: -64}))
    assert s["healthy"] is False
    assert s["short_groups"] == ["convert"]
    assert s["failing_units"] == [] and s["error_count"] == 0
    s = summarize_valu(_raw(compared_delta={0: -1, 6: +1}))
    assert s["short_groups"] == ["f32", "consensus"] and s["healthy"] is False
    raw = _raw()
    raw["compared"] = raw["compared"][:6]
    assert summarize_valu(raw)["short_groups"] == ["consensus"]


def test_failing_ops_come_from_the_records():
    key = _key(0, 0, 0, 0)
    recs = [
        {"key": key, "simd": 1, "group": "f32", "op": "v_fma_f32", "set": 0, "lane": 3,
         "rep": 0, "expected": 1, "got": 0},
        {"key": key, "simd": 1, "group": "convert", "op": "v_cvt_pk_fp8_f32 word_sel:1",
         "set": 2, "lane": 9, "rep": 0, "expected": 5, "got": 4},
        {"key": key, "simd": 1, "group": "f32", "op": "v_fma_f32", "set": 1, "lane": 3,
         "rep": 0, "expected": 1, "got": 0},
    ]
    raw = _raw(fail={(key, 1): 0x11}, records=recs)
    raw["records_dropped"] = 7
    raw["error_count"] = 10
    s = summarize_valu(raw)
    assert s["failing_ops"] == ["v_cvt_pk_fp8_f32 word_sel:1", "v_fma_f32"]
    assert s["error_count"] == 10 and s["records_dropped"] == 7
    assert s["healthy"] is False
    # errors counted but no slot marked: still unhealthy
    raw = _raw()
    raw["error_count"] = 1
    assert summarize_valu(raw)["healthy"] is False


# -- health-report wiring -----------------------------------------------------


class _StubNative:
    """Healthy stand-in for the native module; the sweep's result is settable."""

    def __init__(self, raw):
        self.raw = raw
        self.calls = []

    def device_probe(self, device):
        return {"gcn_arch": "gfx950:sramecc+:xnack-", "compute_units": 6,
                "device_count": 1}

    def mfma_f32_check(self, device):
        return 0.0

    def mfma_bf16_check(self, device):
        return 0.0

    def hbm_bandwidth_gbps(self, device, buf_mib, iters):
        return 5000.0

    def lds_roundtrip_check(self, device):
        return True

    def valu_coverage_check(self, device, **kw):
        self.calls.append((device, kw))
        return self.raw


TODAYS_CHECK_KEYS = {
    "smi", "device", "arch_ok", "mfma_f32_max_err", "mfma_bf16_max_err",
    "hbm_bandwidth_gbps", "lds_ok", "xgmi_ok",
}


def _install_stub(monkeypatch, stub):
    monkeypatch.setattr(gpu_health, "load_native_validator", lambda: stub)
    monkeypatch.setattr(
        gpu_health, "smi_probe", lambda: {"tool": None, "ok": False, "raw": ""})


def test_health_report_without_valu_never_calls_it(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS
    assert report["healthy"] is True
    assert gpu_health_check(require_gpu=True, valu=False) == report
    assert stub.calls == []


def test_health_report_valu_adds_one_key_and_gates(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, valu=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS | {"valu"}
    v = report["checks"]["valu"]
    assert v["healthy"] is True and v["cus_covered"] == 6
    assert "units" not in v and "records" not in v
    assert report["healthy"] is True
    assert stub.calls == [(0, {})]

    slot = (_key(0, se=1, sh=0, cu=1), 1)
    stub.raw = _raw(digests={slot: [(1, 2, 3)]})
    report = gpu_health_check(require_gpu=True, valu=True)
    assert report["healthy"] is False
    assert report["checks"]["valu"]["failing_units"][0]["failed"] == ["consensus"]
    # everything else is still fine: only the sweep gates it
    assert gpu_health_check(require_gpu=True)["healthy"] is True
    stub.raw = _raw(compared_delta={1: -1})
    assert gpu_health_check(require_gpu=True, valu=True)["healthy"] is False


def test_main_maps_the_valu_flag(monkeypatch, capsys):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    monkeypatch.setattr(sys, "argv", ["gpu_health"])
    assert gpu_health.main() == 0
    assert "valu" not in json.loads(capsys.readouterr().out)["checks"]
    assert stub.calls == []
    monkeypatch.setattr(sys, "argv", ["gpu_health", "--valu"])
    assert gpu_health.main() == 0
    assert "valu" in json.loads(capsys.readouterr().out)["checks"]
    assert len(stub.calls) == 1
    stub.raw = _raw(fail={(_key(0, 0, 0, 0), 0): 4})
    assert gpu_health.main() == 1


def test_python_wrapper_summarizes_and_keeps_units_and_records(monkeypatch):
    stub = _StubNative(_raw())
    monkeypatch.setattr(valu_module, "load_native_validator", lambda: stub)
    out = valu_check(0, reps=2, poison_mask=64)
    assert stub.calls == [(0, {"reps": 2, "poison_mask": 64})]
    assert out["healthy"] is True
    assert len(out["units"]) == 24 and out["records"] == []
    monkeypatch.setattr(valu_module, "load_native_validator", lambda: None)
    with pytest.raises(gpu_health.GpuHealthError):
        valu_check(0)


# -- valu_reference() against models written here ------------------------------

from valu_models import (  # noqa: E402
    BF16, E2M1, E4M3, E5M2, F16, F32, F64, decode, h0, h1, hi, is_tie, lo, rne,
    scale_exp, wave_model,
)


@pytest.fixture(scope="module")
def reference():
    native = load_native_validator()
    if native is None:
        pytest.skip("native validator not built and not buildable here")
    return native.valu_reference()


def _exact_ops(reference):
    return [op for op in reference["ops"] if op["expected"] is not None]


def test_reference_shape(reference):
    assert reference["groups"] == BITS
    assert reference["sets"] * reference["lanes"] == 256
    names = [op["name"] for op in reference["ops"]]
    assert len(set(names)) == len(names)
    per_group = {g: 0 for g in BITS}
    for op in reference["ops"]:
        assert len(op["a"]) == len(op["b"]) == len(op["c"]) == (
            reference["consensus_inputs"] if op["group"] == "consensus" else 256)
        assert (op["expected"] is None) == (op["group"] == "consensus")
        per_group[op["group"]] += (reference["consensus_inputs"]
                                   if op["group"] == "consensus" else reference["sets"])
    assert reference["items"] == [64 * per_group[g] for g in BITS]
    for required in (
            "v_fma_f32", "v_pk_fma_f32", "v_med3_f32", "v_ldexp_f32", "v_rndne_f32",
            "v_fma_f64", "v_pk_fma_f16", "v_dot2c_f32_bf16", "v_mad_u64_u32",
            "v_perm_b32", "v_sad_u8", "v_dot4_i32_i8", "v_cvt_pk_bf16_f32",
            "v_cvt_pk_fp8_f32 word_sel:1", "v_cvt_f32_bf8 byte_sel:3",
            "v_cvt_scalef32_pk_fp4_f32 byte_sel:2", "v_mov_b32_dpp row_bcast:31",
            "v_permlane16_swap_b32", "v_permlane32_swap_b32", "v_readlane_b32",
            "v_exp_f32", "v_rsq_f64", "v_cvt_sr_fp8_f32", "v_prng_b32"):
        assert required in names
    assert len([n for n in names if n.startswith("v_bitop3_b32")]) >= 4


def test_reference_expected_words_match_the_models(reference):
    for op in _exact_ops(reference):
        for s in range(reference["sets"]):
            sl = slice(64 * s, 64 * s + 64)
            want = wave_model(op["name"], op["a"][sl], op["b"][sl], op["c"][sl])
            assert op["expected"][sl] == want, (op["name"], s)


def _floats_of(op):
    """(format, code) of every floating input and output of a record list."""
    name = op["name"].split(" ")[0]
    for i in range(256):
        a, b, c, e = op["a"][i], op["b"][i], op["c"][i], op["expected"][i]
        if op["group"] == "f32":
            words = [lo(a), lo(e)]
            if name not in ("v_ldexp_f32", "v_frexp_mant_f32", "v_rndne_f32"):
                words.append(lo(b))
            if name in ("v_fma_f32", "v_pk_fma_f32", "v_med3_f32"):
                words.append(lo(c))
            if name.startswith("v_pk_"):
                words += [hi(a), hi(b), hi(e)] + ([hi(c)] if "fma" in name else [])
            for w in words:
                yield F32, w
        elif op["group"] == "f64":
            yield F64, a
            yield F64, e
            if name != "v_ldexp_f64":
                yield F64, b
            if name == "v_fma_f64":
                yield F64, c
        elif name.startswith("v_pk_") and name.endswith("_f16"):
            for w in (a, b, e) + ((c,) if "fma" in name else ()):
                yield F16, h0(lo(w))
                yield F16, h1(lo(w))


@pytest.mark.parametrize("group", ["f32", "f64", "f16"])
def test_floating_groups_hold_no_nan_and_all_special_cases(reference, group):
    ops = [op for op in _exact_ops(reference) if op["group"] == group]
    subnormal = signed_zero = False
    for op in ops:
        for fmt, code in _floats_of(op):
            v = decode(fmt, code)
            assert v is not None, (op["name"], hex(code))
            ebits, mbits, _ = fmt
            if v == 0 and code >> (ebits + mbits):
                signed_zero = True
            if v != 0 and (code >> mbits) & ((1 << ebits) - 1) == 0:
                subnormal = True
    assert subnormal and signed_zero
    # an exact tie: the exact result of a multiply / add / fma lies halfway
    fmt = {"f32": F32, "f64": F64, "f16": F16}[group]
    ties = 0
    for op in ops:
        name = op["name"]
        if not any(k in name for k in ("fma", "add", "mul")):
            continue
        for i in range(256):
            a, b, c = op["a"][i], op["b"][i], op["c"][i]
            if fmt == F16:
                a, b, c = h0(lo(a)), h0(lo(b)), h0(lo(c))
            elif fmt == F32:
                a, b, c = lo(a), lo(b), lo(c)
            x, y, z = decode(fmt, a), decode(fmt, b), decode(fmt, c)
            exact = x * y + z if "fma" in name else x + y if "add" in name else x * y
            ties += is_tie(fmt, exact)
    assert ties >= 1


def test_dot2_partial_sums_are_exact(reference):
    for op in _exact_ops(reference):
        if not op["name"].startswith("v_dot2c"):
            continue
        f = F16 if op["name"].endswith("_f16") else BF16
        for i in range(256):
            a, b, c = lo(op["a"][i]), lo(op["b"][i]), lo(op["c"][i])
            vals = [decode(f, h0(a)), decode(f, h1(a)), decode(f, h0(b)), decode(f, h1(b)),
                    decode(F32, c)]
            # small integers: every partial sum, in any order and at any
            # internal width of at least 11 bits, is exact
            assert all(v is not None and v.denominator == 1 and abs(v) <= 8 for v in vals)
            for part in (vals[0] * vals[2], vals[1] * vals[3], vals[4],
                         vals[0] * vals[2] + vals[1] * vals[3],
                         vals[0] * vals[2] + vals[4], vals[1] * vals[3] + vals[4]):
                assert abs(part) < 2 ** 10


def test_fp8_records_respect_their_ranges(reference):
    seen_codes = {"fp8": set(), "bf8": set()}
    fp4_codes = set()
    selects = set()
    ties = {"fp8": 0, "bf8": 0, "fp4": 0}
    subnormal_targets = {"fp8": 0, "bf8": 0}
    for op in _exact_ops(reference):
        base, _, imm = op["name"].partition(" ")
        if not base.startswith("v_cvt_"):
            continue
        sel = int(imm.split(":")[1], 0) if ":" in imm else 0
        kind = "fp8" if "fp8" in base else "bf8"
        fmt, limit = (E4M3, 448) if kind == "fp8" else (E5M2, 57344)
        if base in ("v_cvt_pk_fp8_f32", "v_cvt_pk_bf8_f32"):
            selects.add((base, sel))
            for i in range(256):
                for w in (lo(op["a"][i]), hi(op["a"][i])):
                    x = decode(F32, w)
                    assert x is not None and abs(x) <= limit
                    ties[kind] += is_tie(fmt, x)
                    subnormal_targets[kind] += 0 < abs(x) < Fraction(2) ** (1 - fmt[2])
        elif base in ("v_cvt_f32_fp8", "v_cvt_f32_bf8"):
            selects.add((base, sel))
            for i in range(256):
                code = (lo(op["a"][i]) >> (8 * sel)) & 0xFF
                assert decode(fmt, code) is not None
                seen_codes[kind].add((sel, code))
        elif base == "v_cvt_scalef32_pk_f32_fp4":
            selects.add((base, sel))
            for i in range(256):
                byte = (lo(op["a"][i]) >> (8 * sel)) & 0xFF
                fp4_codes.add((sel, byte & 15))
                fp4_codes.add((sel, byte >> 4))
                scale_exp(lo(op["b"][i]))
        elif base == "v_cvt_scalef32_pk_fp4_f32":
            selects.add((base, sel))
            for i in range(256):
                s = Fraction(2) ** scale_exp(lo(op["b"][i]))
                for w in (lo(op["a"][i]), hi(op["a"][i])):
                    x = decode(F32, w) / s
                    assert abs(x) <= 6
                    ties["fp4"] += is_tie(E2M1, x)
    # every non-NaN code through every byte select; all 16 fp4 codes likewise
    for sel in range(4):
        assert {c for s, c in seen_codes["fp8"] if s == sel} == {
            c for c in range(256) if c & 0x7F != 0x7F}
        assert {c for s, c in seen_codes["bf8"] if s == sel} == {
            c for c in range(256) if c & 0x7C != 0x7C}
        assert {c for s, c in fp4_codes if s == sel} == set(range(16))
    assert {("v_cvt_pk_fp8_f32", 0), ("v_cvt_pk_fp8_f32", 1), ("v_cvt_pk_bf8_f32", 0),
            ("v_cvt_pk_bf8_f32", 1)} <= selects
    assert all(n > 0 for n in ties.values()), ties
    assert all(n > 0 for n in subnormal_targets.values()), subnormal_targets


def test_conversion_records_hold_ties_and_subnormal_targets(reference):
    ops = {op["name"]: op for op in _exact_ops(reference)}
    for name, fmt, words in (("v_cvt_f16_f32", F16, (lo,)),
                             ("v_cvt_pk_bf16_f32", BF16, (lo, hi))):
        xs = [decode(F32, w(v)) for v in ops[name]["a"] for w in words]
        assert all(x is not None for x in xs)
        assert any(is_tie(fmt, x) for x in xs)
        assert any(0 < abs(x) < Fraction(2) ** (1 - fmt[2]) for x in xs)


def test_models_agree_with_struct_on_plain_cases():
    # the test's own rounder against the platform's IEEE conversions
    for x in (1.0, -2.5, 1e-40, 3.4e38, 0.1, 2.0 ** -149, 65504.0, 1e-7):
        bits = struct.unpack("<I", struct.pack("<f", x))[0]
        assert rne(F32, Fraction(x)) == bits
        assert decode(F32, bits) == Fraction(struct.unpack("<f", struct.pack("<f", x))[0])
    for x in (1.0, 0.1, 65504.0, 6e-8, 1e-5, 1 + 2 ** -11, 1 + 3 * 2 ** -11):
        bits = struct.unpack("<H", struct.pack("<e", x))[0]
        assert rne(F16, Fraction(x)) == bits
    assert is_tie(F16, 1 + Fraction(1, 2 ** 11)) and not is_tie(F16, 1 + Fraction(1, 2 ** 10))
    assert is_tie(E2M1, Fraction(5, 2)) and is_tie(E4M3, Fraction(17))
    assert rne(E4M3, Fraction(17)) == 0x58 and rne(E2M1, Fraction(-7, 2)) == 0xE
    assert decode(E4M3, 0x7E) == 448 and decode(E4M3, 0x7F) is None
    assert decode(E5M2, 0x7B) == 57344 and decode(E5M2, 0x7C) is None
