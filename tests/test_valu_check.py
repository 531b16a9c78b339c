"""The vector-ALU check on a real MI355X.

Single instructions are probed on one wave and compared bit for bit against
models written for the tests (`valu_models.py`: Fractions, own coders, own
lane maps): these probes are what pin the cross-lane maps, a wrong map cannot
reproduce them.  The sweep must reach every CU and SIMD, count every compare,
end with one digest tuple on every slot, and the data-only poison hook proves
that each of the seven comparisons is live and attributed to the unit that
produced it.  Nothing depends on timing."""

import numpy as np
import pytest

from valu_models import (
    E2M1, E4M3, E5M2, F32, decode, is_tie, lane_model, lo, pack, rne, wave_model,
)

pytestmark = pytest.mark.gpu

BITS = ["f32", "f64", "f16", "int", "convert", "crosslane", "consensus"]

# Largest error of the raw transcendentals against float64, in ulps of the
# f32 result, measured on an MI355X over TRANSCENDENTAL_INPUTS (see
# docs/performance.md); the bound of the sanity test is twice that plus one.
MEASURED_ULPS = {
    "v_exp_f32": 0.71,
    "v_log_f32": 1.00,
    "v_rcp_f32": 0.72,
    "v_rsq_f32": 0.77,
    "v_sqrt_f32": 0.81,
    "v_sin_f32": 3.63,
}


@pytest.fixture(scope="module")
def native():
    import os

    from k8s_operator_libs_amd.validation import GpuHealthError, load_native_validator

    mod = load_native_validator()
    if mod is None:
        if not os.path.exists("/dev/kfd"):
            # CPU-only machine running an unfiltered `pytest tests/`: skip.
            # On a real GPU box a missing native extension stays a HARD
            # failure.
            pytest.skip("no GPU on this machine (missing /dev/kfd)")
        raise GpuHealthError(
            "native validator must be present on a GPU box - refusing to skip"
        )
    return mod


@pytest.fixture(scope="module")
def clean(native):
    from k8s_operator_libs_amd.validation import valu_check

    return valu_check(0)


@pytest.fixture(scope="module")
def reference(native):
    return native.valu_reference()


def _probe(native, name, a, b=None, c=None):
    zero = [0] * 64
    return native.valu_probe(0, name, list(a), list(b or zero), list(c or zero))


def _f32(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


# -- the sweep ----------------------------------------------------------------


def test_default_run_is_healthy_and_counted(clean, reference):
    assert clean["healthy"] is True, (clean["failing_units"][:4], clean["failing_ops"],
                                     clean["short_groups"], clean["records"][:4])
    assert clean["cus_covered"] == clean["compute_units"]
    assert clean["simd_slots_covered"] == 4 * clean["compute_units"]
    assert clean["reps"] == 4  # the default
    assert clean["compared"] == clean["compared_expected"]
    assert clean["compared_expected"] == [
        clean["waves_run"] * clean["reps"] * n for n in reference["items"]]
    assert all(n > 0 for n in clean["compared"])
    assert clean["error_count"] == 0 and clean["records"] == []
    tuples = {tuple(t) for u in clean["units"] for t in u["digests"]}
    assert all(len(u["digests"]) == 1 for u in clean["units"])
    assert len(tuples) == 1
    assert list(clean["consensus_digests"].values()) == list(next(iter(tuples)))
    print("valu default run: rounds", clean["rounds"], "elapsed_ms", clean["elapsed_ms"])


def test_second_run_gives_the_same_digests(native, clean):
    from k8s_operator_libs_amd.validation import valu_check

    again = valu_check(0, reps=1)
    assert again["healthy"] is True
    assert again["consensus_digests"] == clean["consensus_digests"]
    assert None not in again["consensus_digests"].values()


def test_poisoned_cu_fails_alone_with_all_seven_names(native, clean, reference):
    from k8s_operator_libs_amd.validation import valu_check

    key = clean["units"][len(clean["units"]) // 2]["key"]
    out = valu_check(0, reps=1, poison_key=key, poison_mask=0x7F)
    assert out["healthy"] is False
    covered = sorted((u["key"], u["simd"]) for u in out["units"] if u["key"] == key)
    assert len(covered) == 4
    assert sorted((u["key"], u["simd"]) for u in out["failing_units"]) == covered
    assert all(u["failed"] == BITS for u in out["failing_units"])
    # only the comparison was poisoned: what the hardware computed is the
    # unpoisoned reference value
    ops = {op["name"]: op for op in reference["ops"]}
    assert out["records"] and out["error_count"] >= len(out["records"])
    assert out["records_dropped"] == out["error_count"] - len(out["records"])
    for r in out["records"]:
        assert r["key"] == key
        want = ops[r["op"]]["expected"][64 * r["set"] + r["lane"]]
        assert r["got"] == want and r["expected"] == want ^ 1
    assert out["short_groups"] == []


def test_poison_all_fails_every_slot_with_the_six_exact_names(native, clean):
    from k8s_operator_libs_amd.validation import valu_check

    out = valu_check(0, reps=1, poison_all=True, poison_mask=0x3F)
    assert out["healthy"] is False
    assert len(out["failing_units"]) == 4 * clean["compute_units"]
    assert all(u["failed"] == BITS[:6] for u in out["failing_units"])
    assert out["consensus_digests"] == clean["consensus_digests"]


def test_poison_all_with_the_consensus_bit_raises(native):
    with pytest.raises(ValueError):
        native.valu_coverage_check(0, poison_all=True, poison_mask=0x40)
    with pytest.raises(ValueError):
        native.valu_coverage_check(0, poison_all=True, poison_mask=0x7F)


def test_full_report_carries_the_check(native):
    from k8s_operator_libs_amd.validation import gpu_health_check

    report = gpu_health_check(valu=True, require_gpu=True)
    assert report["healthy"] is True
    v = report["checks"]["valu"]
    assert v["healthy"] is True and v["short_groups"] == []
    assert "units" not in v and "records" not in v


# -- single instructions ---------------------------------------------------------


def test_probe_validates_before_it_runs(native):
    zero = [0] * 64
    with pytest.raises(ValueError):
        native.valu_probe(0, "v_nonesuch", zero, zero, zero)
    with pytest.raises(ValueError):
        native.valu_probe(0, "v_fma_f32", zero[:63], zero, zero)
    with pytest.raises(ValueError):  # an fp8 NaN code
        native.valu_probe(0, "v_cvt_f32_fp8 byte_sel:1", [0x7F00] * 64, zero, zero)
    with pytest.raises(ValueError):  # beyond the largest finite e4m3
        native.valu_probe(0, "v_cvt_pk_fp8_f32 word_sel:0", [_f32(449.0)] * 64, zero, zero)
    with pytest.raises(ValueError):  # a NaN input
        native.valu_probe(0, "v_fma_f32", [0x7FC00000] * 64, zero, zero)


def test_probe_fma_subnormal_and_tie_results(native):
    one, t = 0x3F800000, 0x3F800800  # 1, 1 + 2^-12
    triples = [
        (t, t, 0),                      # 1 + 2^-11 + 2^-24: tie -> even
        (t, t, 0xBF801000),             # fused: 2^-24 is left
        (0x0D800000, 0x30800000, 0x00000200),  # 2^-100 * 2^-30 + subnormal
        (0x00000003, 0x3F000000, 0),    # 1.5 ulp: a tie between subnormals
        (0x00000003, 0x3F000000, 0x00000001),
        (0x80000000, 0x40A00000, 0),    # -0 * 5 + 0 = +0
        (0x80000000, 0x40A00000, 0x80000000),  # -0
        (one | 1, 0x3F000001, 0x33800000),
        (0x00800000, 0x3F7FFFFF, 0),    # just below the smallest normal
        (0x7F7FFFFF, 0x3F800000, 0xF3000000),
    ]
    rows = [triples[l % len(triples)] for l in range(64)]
    a, b, c = ([r[i] for r in rows] for i in range(3))
    for name in ("v_fma_f32",):
        got = _probe(native, name, a, b, c)
        assert got == [lane_model(name, a[l], b[l], c[l]) for l in range(64)]
    got = _probe(native, "v_pk_fma_f32", [pack(x, y) for x, y in zip(a, a[::-1])],
                 [pack(x, y) for x, y in zip(b, b[::-1])],
                 [pack(x, y) for x, y in zip(c, c[::-1])])
    assert got == [pack(lane_model("v_fma_f32", a[l], b[l], c[l]),
                        lane_model("v_fma_f32", a[63 - l], b[63 - l], c[63 - l]))
                   for l in range(64)]
    # the separate multiply and add stay separate on the device as well
    prod = _probe(native, "v_mul_f32", a, b)
    assert prod == [lane_model("v_mul_f32", a[l], b[l], 0) for l in range(64)]
    assert prod[1] == 0x3F801000
    assert _probe(native, "v_add_f32", prod, c)[1] == 0


@pytest.mark.parametrize("kind,fmt", [("fp8", E4M3), ("bf8", E5M2)])
def test_probe_decodes_every_non_nan_code(native, kind, fmt):
    codes = [c for c in range(256) if decode(fmt, c) is not None]
    assert len(codes) == (254 if kind == "fp8" else 248)
    for sel in range(4):
        for i in range(0, 256, 64):
            chunk = [codes[min(i + l, len(codes) - 1)] for l in range(64)]
            a = [(0xA5A5A5A5 & ~(0xFF << (8 * sel))) | c << (8 * sel) for c in chunk]
            got = _probe(native, f"v_cvt_f32_{kind} byte_sel:{sel}", a)
            assert got == [rne(F32, decode(fmt, c), neg_zero=bool(c >> 7)) for c in chunk]


def test_probe_decodes_all_fp4_codes(native):
    for sel in range(4):
        bytes_ = [(l & 15) | ((l * 7 + 3) & 15) << 4 for l in range(64)]
        a = [(0x5A5A5A5A & ~(0xFF << (8 * sel))) | v << (8 * sel) for v in bytes_]
        scales = [_f32(2.0 ** ((l % 9) - 4)) for l in range(64)]
        name = f"v_cvt_scalef32_pk_f32_fp4 byte_sel:{sel}"
        got = _probe(native, name, a, scales)
        assert {v & 15 for v in bytes_} == {v >> 4 for v in bytes_} == set(range(16))
        assert got == [lane_model(name, a[l], scales[l], 0) for l in range(64)]


def test_probe_fp8_and_fp4_encode_ties(native):
    for kind, fmt, top in (("fp8", E4M3, 0x7E), ("bf8", E5M2, 0x7B)):
        # the midpoint of every pair of neighbouring codes, both signs
        mids = []
        for code in range(top):
            m = (decode(fmt, code) + decode(fmt, code + 1)) / 2
            assert is_tie(fmt, m)
            mids += [m, -m]
        for sel in (0, 1):
            name = f"v_cvt_pk_{kind}_f32 word_sel:{sel}"
            for i in range(0, len(mids), 64):
                xs = [mids[min(i + l, len(mids) - 1)] for l in range(64)]
                ys = xs[::-1]
                a = [pack(_f32(float(x)), _f32(float(y))) for x, y in zip(xs, ys)]
                old = [0x13572468] * 64
                got = _probe(native, name, a, None, old)
                assert got == [lane_model(name, a[l], 0, old[l]) for l in range(64)]
    halves = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.5, 6.0, 0.0]
    for sel in range(4):
        name = f"v_cvt_scalef32_pk_fp4_f32 byte_sel:{sel}"
        ex = [(l % 7) - 3 for l in range(64)]
        a = [pack(_f32(halves[l % 10] * 2.0 ** ex[l]),
                  _f32(-halves[(l + 3) % 10] * 2.0 ** ex[l])) for l in range(64)]
        b = [_f32(2.0 ** e) for e in ex]
        old = [0x89ABCDEF] * 64
        got = _probe(native, name, a, b, old)
        assert got == [lane_model(name, a[l], b[l], old[l]) for l in range(64)]
    assert is_tie(E2M1, decode(F32, _f32(2.5)))


def test_probe_cross_lane_maps(native, reference):
    # distinct, recognisable values: the source's lane in the low byte
    src = [0x51000000 | l * 0x010101 for l in range(64)]
    old = [0x0D000000 | l * 0x010101 for l in range(64)]
    names = [op["name"] for op in reference["ops"] if op["group"] == "crosslane"]
    dpp = [n for n in names if n.startswith("v_mov_b32_dpp ")]
    assert len(dpp) == 32
    for name in dpp + ["v_readlane_b32", "v_readfirstlane_b32",
                       "v_permlane16_swap_b32", "v_permlane32_swap_b32"]:
        got = _probe(native, name, src, old)
        assert got == wave_model(name, src, old, [0] * 64), name
    masks = [0xF0F0F0F0F0F0F0F0 ^ (l * 0x0101010101010101) for l in range(64)]
    name = "v_mbcnt_lo_u32_b32+v_mbcnt_hi_u32_b32"
    assert _probe(native, name, masks, list(range(64))) == wave_model(
        name, masks, list(range(64)), [0] * 64)
    name = "v_cmp_lt_u32 (64-bit mask)"
    x = [(l * 37) % 64 for l in range(64)]
    assert _probe(native, name, x, [32] * 64) == wave_model(name, x, [32] * 64, [0] * 64)


def test_probe_matches_the_reference_records(native, reference):
    # set 0 of every exact op, as generated: ties, subnormals and signed zeros
    for op in reference["ops"]:
        if op["expected"] is None:
            continue
        got = _probe(native, op["name"], op["a"][:64], op["b"][:64], op["c"][:64])
        assert got == op["expected"][:64], op["name"]


# -- transcendental sanity -------------------------------------------------------

N = 1024
POS = np.exp2(np.linspace(-20, 20, N)).astype(np.float32)
# v_log_f32 near 1 gives a result near 0, where an error of one ulp of the
# *input* is many ulps of the result: the normal-range claim leaves it out
LOG_IN = POS[np.abs(POS - 1) > 0.25][:960]
# v_sin_f32 takes revolutions; away from the zero crossings for the same reason
TRANSCENDENTAL_INPUTS = {
    "v_exp_f32": (np.linspace(-20, 20, N).astype(np.float32), np.exp2),
    "v_log_f32": (LOG_IN, np.log2),
    "v_rcp_f32": (POS, lambda x: 1.0 / x),
    "v_rsq_f32": (POS, lambda x: 1.0 / np.sqrt(x)),
    "v_sqrt_f32": (POS, np.sqrt),
    "v_sin_f32": (np.linspace(0.02, 0.48, N).astype(np.float32),
                  lambda x: np.sin(2 * np.pi * x)),
}


@pytest.mark.parametrize("name", list(TRANSCENDENTAL_INPUTS))
def test_transcendentals_make_sense(native, name):
    xs, fn = TRANSCENDENTAL_INPUTS[name]
    assert len(xs) % 64 == 0
    got = []
    for i in range(0, len(xs), 64):
        a = [int(v) for v in xs[i:i + 64].view(np.uint32)]
        got += [lo(v) for v in _probe(native, name, a)]
    got = np.array(got, dtype=np.uint32).view(np.float32).astype(np.float64)
    want = fn(xs.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(got - want) / ulp))
    print(name, "largest error in ulps:", worst)
    assert worst <= 2 * MEASURED_ULPS[name] + 1
