"""CPU-side tests for the MX block-scaled matrix check.

``summarize_mx_matrix`` is pure, so it is driven with hand-built raw tables of
a small synthetic device (2 XCCs x 3 CUs).  The health-report wiring is
checked against a stub native module.  The host-generated problems
(``mx_reference()``: raw operand codes, raw E8M0 scale codes, packed lane
words, expected tiles) are checked against decoders and a packer written here
from the OCP MX definitions, never by calling the native ones."""

import math

import numpy as np
import pytest

from k8s_operator_libs_amd.validation import (
    gpu_health,
    gpu_health_check,
    load_native_validator,
    mx_matrix,
    summarize_mx_matrix,
)

XCCS, CUS_PER_XCC = 2, 3
BITS = ["e4m3", "e5m2", "e2m3", "e3m2", "e2m1", "mixed", "shape32"]


def _key(xcc, se, sh, cu):
    return (xcc << 8) | (se << 5) | (sh << 4) | cu


def _raw(skip_slots=(), fail=None, compute_units=XCCS * CUS_PER_XCC):
    """A fully covered synthetic device minus ``skip_slots`` ((key, simd)
    pairs); ``fail`` maps (key, simd) -> fail_mask."""
    fail = fail or {}
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
                })
    keys = {u["key"] for u in units}
    return {
        "compute_units": compute_units,
        "cus_covered": len(keys),
        "simd_slots_covered": len(units),
        "waves_run": 2 * len(units),
        "rounds": 1,
        "failed_slots": sum(1 for u in units if u["fail_mask"]),
        "units": units,
        "elapsed_ms": 0.5,
    }


# -- summarize_mx_matrix ------------------------------------------------------


def test_summary_healthy_full_coverage():
    s = summarize_mx_matrix(_raw())
    assert s["healthy"] is True
    assert s["compute_units"] == 6
    assert s["cus_covered"] == 6
    assert s["simd_slots_covered"] == 24
    assert s["per_xcc"] == {0: 3, 1: 3}
    assert s["uncovered_cus"] == 0
    assert s["failing_units"] == []
    assert s["rounds"] == 1
    assert s["elapsed_ms"] == 0.5
    assert "units" not in s


def test_fail_bits_are_the_documented_seven():
    assert list(mx_matrix.FAIL_BITS) == BITS


@pytest.mark.parametrize("bit,name", list(enumerate(BITS)))
def test_summary_decodes_each_fail_bit(bit, name):
    key = _key(1, se=1, sh=0, cu=1)
    s = summarize_mx_matrix(_raw(fail={(key, 2): 1 << bit}))
    assert s["healthy"] is False
    assert s["cus_covered"] == 6 and s["simd_slots_covered"] == 24
    assert len(s["failing_units"]) == 1
    unit = s["failing_units"][0]
    assert (unit["xcc"], unit["se"], unit["sh"], unit["cu"]) == (1, 1, 0, 1)
    assert unit["simd"] == 2
    assert unit["key"] == key
    assert unit["failed"] == [name]


def test_summary_decodes_combined_mask_in_bit_order():
    key = _key(0, se=0, sh=0, cu=0)
    s = summarize_mx_matrix(_raw(fail={(key, 0): 0x7F, (key, 3): 0x54}))
    assert [u["failed"] for u in s["failing_units"]] == [
        BITS, ["e2m3", "e2m1", "shape32"],
    ]
    assert [u["simd"] for u in s["failing_units"]] == [0, 3]


def test_summary_missing_cu_is_unhealthy():
    gone = _key(0, se=1, sh=0, cu=1)
    s = summarize_mx_matrix(_raw(skip_slots={(gone, i) for i in range(4)}))
    assert s["healthy"] is False
    assert s["uncovered_cus"] == 1
    assert s["cus_covered"] == 5
    assert s["per_xcc"] == {0: 2, 1: 3}
    assert s["failing_units"] == []


def test_summary_three_simd_cu_is_unhealthy():
    key = _key(1, se=0, sh=0, cu=0)
    s = summarize_mx_matrix(_raw(skip_slots={(key, 3)}))
    assert s["cus_covered"] == 6
    assert s["uncovered_cus"] == 0
    assert s["simd_slots_covered"] == 23
    assert s["healthy"] is False


def test_summary_more_keys_than_cus_is_unhealthy():
    s = summarize_mx_matrix(_raw(compute_units=5))
    assert s["cus_covered"] == 6
    assert s["healthy"] is False


# -- health-report wiring -----------------------------------------------------


class _StubNative:
    """Healthy stand-in for the native module; the MX results are settable."""

    def __init__(self, mx_raw):
        self.mx_raw = mx_raw
        self.tflops = {"e2m1": 8000.0, "e4m3": 4000.0}
        self.mx_calls = []
        self.tf_calls = []

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

    def mx_coverage_check(self, device, **kw):
        self.mx_calls.append((device, kw))
        return self.mx_raw

    def mx_throughput_tflops(self, device, fmt, iters):
        self.tf_calls.append((device, fmt, iters))
        return self.tflops[fmt]


TODAYS_CHECK_KEYS = {
    "smi", "device", "arch_ok", "mfma_f32_max_err", "mfma_bf16_max_err",
    "hbm_bandwidth_gbps", "lds_ok", "xgmi_ok",
}


def _install_stub(monkeypatch, stub):
    monkeypatch.setattr(gpu_health, "load_native_validator", lambda: stub)
    monkeypatch.setattr(
        gpu_health, "smi_probe", lambda: {"tool": None, "ok": False, "raw": ""}
    )


def test_health_report_without_mx_is_unchanged(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True)
    assert set(report) == {"healthy", "checks"}
    assert set(report["checks"]) == TODAYS_CHECK_KEYS
    assert report["healthy"] is True
    assert stub.mx_calls == [] and stub.tf_calls == []
    assert gpu_health_check(require_gpu=True, mx=False) == report


def test_health_report_mx_adds_exactly_one_key(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, mx=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS | {"mx_matrix"}
    mx = report["checks"]["mx_matrix"]
    assert mx["healthy"] is True and mx["cus_covered"] == 6
    assert "units" not in mx
    assert mx["throughput_tflops"] == {"e2m1": 8000.0, "e4m3": 4000.0}
    assert report["healthy"] is True
    assert len(stub.mx_calls) == 1
    assert [c[1] for c in stub.tf_calls] == ["e2m1", "e4m3"]


def test_health_report_failing_unit_alone_flips_healthy(monkeypatch):
    key = _key(0, se=1, sh=0, cu=1)
    stub = _StubNative(_raw(fail={(key, 1): 1 << 4}))
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, mx=True)
    assert report["healthy"] is False
    mx = report["checks"]["mx_matrix"]
    assert mx["failing_units"][0]["failed"] == ["e2m1"]
    assert "units" not in mx
    assert all(tf >= gpu_health.MFMA_MIN_TFLOPS
               for tf in mx["throughput_tflops"].values())
    # everything else is still fine: only the sweep gates it
    assert gpu_health_check(require_gpu=True)["healthy"] is True

    stub.mx_raw = _raw(skip_slots={(key, 0)})
    assert gpu_health_check(require_gpu=True, mx=True)["healthy"] is False


@pytest.mark.parametrize("fmt", ["e2m1", "e4m3"])
def test_health_report_slow_throughput_alone_flips_healthy(monkeypatch, fmt):
    stub = _StubNative(_raw())
    stub.tflops[fmt] = gpu_health.MFMA_MIN_TFLOPS - 1.0
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, mx=True)
    assert report["checks"]["mx_matrix"]["healthy"] is True
    assert report["checks"]["mx_matrix"]["failing_units"] == []
    assert report["healthy"] is False
    stub.tflops[fmt] = gpu_health.MFMA_MIN_TFLOPS
    assert gpu_health_check(require_gpu=True, mx=True)["healthy"] is True


def test_main_maps_the_mx_flag(monkeypatch, capsys):
    import json
    import sys

    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    monkeypatch.setattr(sys, "argv", ["gpu_health"])
    assert gpu_health.main() == 0
    assert "mx_matrix" not in json.loads(capsys.readouterr().out)["checks"]
    monkeypatch.setattr(sys, "argv", ["gpu_health", "--mx"])
    assert gpu_health.main() == 0
    assert "mx_matrix" in json.loads(capsys.readouterr().out)["checks"]
    stub.tflops["e4m3"] = 10.0
    assert gpu_health.main() == 1


def test_python_wrapper_summarizes_and_keeps_units(monkeypatch):
    stub = _StubNative(_raw())
    monkeypatch.setattr(mx_matrix, "load_native_validator", lambda: stub)
    out = mx_matrix.mx_matrix_check(0, reps=2, poison_mask=64)
    assert stub.mx_calls == [(0, {"reps": 2, "poison_mask": 64})]
    assert out["healthy"] is True
    assert len(out["units"]) == 24
    monkeypatch.setattr(mx_matrix, "load_native_validator", lambda: None)
    with pytest.raises(gpu_health.GpuHealthError):
        mx_matrix.mx_matrix_check(0)


# -- mx_reference() against independent decoders ------------------------------

# OCP MX element formats: (bits, exponent bits, mantissa bits, bias)
FORMATS = {
    "e4m3": (8, 4, 3, 7),
    "e5m2": (8, 5, 2, 15),
    "e2m3": (6, 2, 3, 1),
    "e3m2": (6, 3, 2, 3),
    "e2m1": (4, 2, 1, 1),
}
SHAPES = {"16x16x128": (16, 16, 128), "32x32x64": (32, 32, 64)}
SAME_16 = [(f, f, "16x16x128") for f in FORMATS]
MIXED_16 = [("e4m3", "e2m1", "16x16x128"), ("e2m1", "e2m3", "16x16x128")]
SHAPE_32 = [("e2m1", "e2m1", "32x32x64"), ("e4m3", "e4m3", "32x32x64")]


def _fields(fmt, code):
    bits, ebits, mbits, _ = FORMATS[fmt]
    assert 0 <= code < (1 << bits)
    return (code >> (bits - 1), (code >> mbits) & ((1 << ebits) - 1),
            code & ((1 << mbits) - 1))


def decode_element(fmt, code):
    """OCP MX v1.0 element value (float64, exact); NaN/Inf codes -> None."""
    _, _, mbits, bias = FORMATS[fmt]
    s, e, m = _fields(fmt, code)
    if fmt == "e4m3" and e == 15 and m == 7:
        return None
    if fmt == "e5m2" and e == 31:
        return None
    if e == 0:
        v = math.ldexp(m, 1 - bias - mbits)
    else:
        v = math.ldexp((1 << mbits) + m, e - bias - mbits)
    return -v if s else v


def decode_scale(code):
    assert 0 <= code <= 254, "E8M0 0xFF is NaN"
    return math.ldexp(1.0, code - 127)


def lane_k(bits, k_total, group, j):
    """K index of element j of a lane in lane group ``group`` (the layout in
    validation/README.md, found on hardware): 6-bit and 4-bit lanes hold 32
    consecutive k; an 8-bit lane holds 16 from each half of K."""
    if bits == 8:
        return (k_total // 2) * (j >> 4) + 16 * group + (j & 15)
    return 32 * group + j


def pack_lane(bits, codes):
    """32 elements -> 8 words: element j at bits [bits*j, bits*j + bits) of the
    little-endian string, the words past it zero."""
    big = 0
    for j, c in enumerate(codes):
        big |= int(c) << (bits * j)
    return [(big >> (32 * w)) & 0xFFFFFFFF for w in range(8)]


@pytest.fixture(scope="module")
def reference():
    native = load_native_validator()
    if native is None:
        pytest.skip("native validator not built and not buildable here")
    return native.mx_reference()


class _Problem:
    def __init__(self, raw):
        self.raw = raw
        self.set, self.fa, self.fb = raw["set"], raw["fmt_a"], raw["fmt_b"]
        self.shape = raw["shape"]
        self.m, self.n, self.k = SHAPES[self.shape]
        assert (raw["m"], raw["n"], raw["k"]) == (self.m, self.n, self.k)
        self.kb = self.k // 32
        self.a_codes = np.array(raw["a_codes"]).reshape(self.m, self.k)
        self.b_codes = np.array(raw["b_codes"]).reshape(self.k, self.n)
        self.a_scales = np.array(raw["a_scales"]).reshape(self.m, self.kb)
        self.b_scales = np.array(raw["b_scales"]).reshape(self.kb, self.n)
        self.d = np.array(raw["d"], dtype=np.float32).reshape(self.m, self.n)
        dec_a = np.vectorize(lambda c: decode_element(self.fa, c), otypes=[float])
        dec_b = np.vectorize(lambda c: decode_element(self.fb, c), otypes=[float])
        dec_s = np.vectorize(decode_scale, otypes=[float])
        # every element times the scale of its (row, kblock) / (kblock, col)
        self.a = dec_a(self.a_codes) * np.repeat(dec_s(self.a_scales), 32, axis=1)
        self.b = dec_b(self.b_codes) * np.repeat(dec_s(self.b_scales), 32, axis=0)

    @property
    def ident(self):
        return (self.set, self.fa, self.fb, self.shape)


@pytest.fixture(scope="module")
def problems(reference):
    return [_Problem(p) for p in reference["problems"]]


def test_reference_lists_the_required_problems(reference, problems):
    assert reference["sets"] >= 2
    idents = {p.ident for p in problems}
    assert len(idents) == len(problems)
    for s in range(reference["sets"]):
        for fa, fb, shape in SAME_16 + MIXED_16 + SHAPE_32:
            assert (s, fa, fb, shape) in idents


def test_reference_has_no_nan_or_inf_codes(problems):
    for p in problems:
        for fmt, codes in ((p.fa, p.a_codes), (p.fb, p.b_codes)):
            for c in np.unique(codes):
                assert decode_element(fmt, int(c)) is not None, (p.ident, c)
        for scales in (p.a_scales, p.b_scales):
            assert scales.min() >= 0 and scales.max() <= 254


def test_reference_alphabets_cover_the_format(problems):
    for p in problems:
        for fmt, codes in ((p.fa, p.a_codes), (p.fb, p.b_codes)):
            _, _, mbits, _ = FORMATS[fmt]
            fields = [_fields(fmt, int(c)) for c in np.unique(codes)]
            assert {s for s, _, _ in fields} == {0, 1}, p.ident
            assert {m for _, _, m in fields} == set(range(1 << mbits)), p.ident
            assert len({e for _, e, _ in fields}) >= 3, p.ident
            if fmt == "e2m1":
                values = {decode_element(fmt, int(c)) for c in np.unique(codes)}
                assert values == {0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                                  -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0}


def test_reference_expected_tile_is_the_exact_product(problems):
    for p in problems:
        want = p.a @ p.b  # float64: exact here, see the span test
        assert np.array_equal(want.astype(np.float32), p.d), p.ident
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        # asymmetric: transposing a fragment or the output cannot pass
        assert not np.array_equal(p.a, p.b.T), p.ident
        assert not np.array_equal(p.d, p.d.T), p.ident
        assert np.abs(p.d).max() < 2.0 ** 16  # moderate, far scales included


def _log2_span(p):
    """log2(S / q) recomputed from the decoded operands in exact integers."""
    prods = []
    for m in range(p.m):
        prods.append(p.a[m][:, None] * p.b)  # k x n scaled products of row m
    prods = np.stack(prods)  # m x k x n, each exact in float64
    nz = np.abs(prods[prods != 0])
    mant, exp = np.frexp(nz)  # nz = mant * 2^exp, mant in [0.5, 1)
    ints = (mant * 2.0 ** 53).astype(np.int64)
    tz = np.array([(int(v) & -int(v)).bit_length() - 1 for v in np.unique(ints)])
    tz_of = dict(zip(np.unique(ints).tolist(), tz.tolist()))
    q_exp = min(e - 53 + tz_of[i] for i, e in zip(ints.tolist(), exp.tolist()))
    s = np.abs(prods).sum(axis=1).max()
    return math.log2(s) - q_exp


def test_reference_span_is_within_the_claimed_bound(reference, problems):
    bound = reference["span_bound_log2"]
    assert bound <= 24  # any-order exactness in f32
    for p in problems:
        got = _log2_span(p)
        assert got == pytest.approx(p.raw["log2_span"], abs=1e-9), p.ident
        assert got <= bound, p.ident


def test_reference_problems_are_pairwise_different(problems):
    for i, p in enumerate(problems):
        for q in problems[i + 1:]:
            if p.shape != q.shape:
                continue
            assert not np.array_equal(p.a, q.a), (p.ident, q.ident)
            assert not np.array_equal(p.b, q.b), (p.ident, q.ident)
            assert not np.array_equal(p.d, q.d), (p.ident, q.ident)


def test_reference_scales_differ_between_neighbouring_blocks(reference, problems):
    far = set()
    for p in problems:
        if p.set == 0:
            # the uniform set: operand maps on their own
            assert len(np.unique(p.a_scales)) == 1
            assert len(np.unique(p.b_scales)) == 1
            continue
        assert np.all(p.a_scales[1:, :] != p.a_scales[:-1, :]), p.ident  # rows
        assert np.all(p.a_scales[:, 1:] != p.a_scales[:, :-1]), p.ident  # kblocks
        assert np.all(p.b_scales[:, 1:] != p.b_scales[:, :-1]), p.ident  # cols
        assert np.all(p.b_scales[1:, :] != p.b_scales[:-1, :]), p.ident  # kblocks
        if p.a_scales.min() >= 127 + 16 and p.b_scales.max() <= 127 - 16:
            far.add(p.set)
    assert far, "no set with scale bases far from 127 in opposite directions"


def test_reference_scale_words_select_one_byte(problems):
    sels = set()
    for p in problems:
        sa, sb = p.raw["op_sel_a"], p.raw["op_sel_b"]
        sels.add((sa, sb))
        for lane in range(64):
            rc, kb = lane % p.m, lane // p.m
            for word, sel, code in (
                (p.raw["a_scale_words"][lane], sa, p.a_scales[rc, kb]),
                (p.raw["b_scale_words"][lane], sb, p.b_scales[kb, rc]),
            ):
                by = [(word >> (8 * i)) & 0xFF for i in range(4)]
                assert by[sel] == code
                for i in range(4):
                    if i != sel:
                        assert by[i] != code and by[i] <= 254
    assert len({a for a, _ in sels}) > 1 and len({b for _, b in sels}) > 1
    assert any(a != b for a, b in sels)


@pytest.mark.parametrize("fmt", ["e2m3", "e2m1", "e4m3"])
def test_packed_lane_words_match_the_documented_layout(problems, fmt):
    bits = FORMATS[fmt][0]
    checked = 0
    for p in problems:
        if p.fa != fmt and p.fb != fmt:
            continue
        a_words = np.array(p.raw["a_words"]).reshape(64, 8)
        b_words = np.array(p.raw["b_words"]).reshape(64, 8)
        for lane in range(64):
            rc, group = lane % p.m, lane // p.m
            ks = [lane_k(bits, p.k, group, j) for j in range(32)]
            if p.fa == fmt:
                assert a_words[lane].tolist() == pack_lane(bits, p.a_codes[rc, ks])
                checked += 1
            if p.fb == fmt:
                assert b_words[lane].tolist() == pack_lane(bits, p.b_codes[ks, rc])
                checked += 1
        # 32 elements of `bits` bits fill `bits` words; the rest are zero
        if p.fa == fmt:
            assert not a_words[:, bits:].any()
    assert checked >= 128


def test_lane_k_covers_every_k_exactly_once():
    for bits in (8, 6, 4):
        for k_total, groups in ((128, 4), (64, 2)):
            ks = [lane_k(bits, k_total, g, j)
                  for g in range(groups) for j in range(32)]
            assert sorted(ks) == list(range(k_total))
    # an 8-bit lane: words 0..3 from the first half of K, 4..7 from the second
    assert [lane_k(8, 128, 1, j) for j in (0, 15, 16, 31)] == [16, 31, 80, 95]
    assert [lane_k(8, 64, 1, j) for j in (0, 15, 16, 31)] == [16, 31, 48, 63]


def test_pack_lane_crosses_word_boundaries():
    # element 5 of a 6-bit string sits at bits 30..35: both words get a part
    words = pack_lane(6, [0] * 5 + [0b101011] + [0] * 26)
    assert words[0] == (0b11 << 30) and words[1] == 0b1010
    assert pack_lane(4, [0xA, 0x5] + [0] * 30)[0] == 0x5A
