"""MX block-scaled matrix path on a real MI355X.

Single tiles are verified bit for bit against decoders written here from the
OCP MX definitions (the assumed fragment and scale-byte maps are confirmed by
outcome: a wrong map cannot reproduce these tiles).  The sweep must reach
every CU and SIMD the device reports, and the data-only poison hook proves
that each of the seven comparisons is live and attributed to the unit that
produced it.  Nothing depends on timing beyond the project's existing
throughput floor."""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPS = 2
MAX_ROUNDS = 8
BITS = ["e4m3", "e5m2", "e2m3", "e3m2", "e2m1", "mixed", "shape32"]
FAR_SET = 3  # scale bases 2^+20 / 2^-21
WIDE_SET = 4  # widest scale spread: S/q closest to the generator's bound

# (bits, exponent bits, mantissa bits, bias) per OCP MX element format
FORMATS = {
    "e4m3": (8, 4, 3, 7),
    "e5m2": (8, 5, 2, 15),
    "e2m3": (6, 2, 3, 1),
    "e3m2": (6, 3, 2, 3),
    "e2m1": (4, 2, 1, 1),
}
TILES = (
    [(f, f, "16x16x128") for f in FORMATS]
    + [("e4m3", "e2m1", "16x16x128"), ("e2m1", "e2m3", "16x16x128"),
       ("e3m2", "e5m2", "16x16x128")]
    + [("e2m1", "e2m1", "32x32x64"), ("e4m3", "e4m3", "32x32x64")]
)


@pytest.fixture(scope="module")
def native():
    import os

    from k8s_operator_libs_amd.validation import GpuHealthError, load_native_validator

    mod = load_native_validator()
    if mod is None:
        if not os.path.exists("/dev/kfd"):
            # CPU-only machine running an unfiltered `pytest tests/`: skip.
            # On a real GPU box (ROCm kfd present) a missing native
            # extension stays a HARD failure — a silent skip there would
            # green-wash the exact fallback the driver checks for.
            pytest.skip("no GPU on this machine (missing /dev/kfd)")
        raise GpuHealthError(
            "native validator must be present on a GPU box - refusing to skip"
        )
    return mod


@pytest.fixture(scope="module")
def clean(native):
    from k8s_operator_libs_amd.validation import mx_matrix_check

    return mx_matrix_check(0, reps=REPS, max_rounds=MAX_ROUNDS)


def _decode(fmt, code):
    _, ebits, mbits, bias = FORMATS[fmt]
    bits = FORMATS[fmt][0]
    s = code >> (bits - 1)
    e = (code >> mbits) & ((1 << ebits) - 1)
    m = code & ((1 << mbits) - 1)
    assert not (fmt == "e4m3" and e == 15 and m == 7)
    assert not (fmt == "e5m2" and e == 31)
    if e == 0:
        v = math.ldexp(m, 1 - bias - mbits)
    else:
        v = math.ldexp((1 << mbits) + m, e - bias - mbits)
    return -v if s else v


def _numpy_tile(t):
    m, n, k = t["m"], t["n"], t["k"]
    dec_a = np.vectorize(lambda c: _decode(t["fmt_a"], c), otypes=[float])
    dec_b = np.vectorize(lambda c: _decode(t["fmt_b"], c), otypes=[float])
    a = dec_a(np.array(t["a_codes"]).reshape(m, k))
    b = dec_b(np.array(t["b_codes"]).reshape(k, n))
    sa = np.ldexp(1.0, np.array(t["a_scales"]).reshape(m, k // 32) - 127)
    sb = np.ldexp(1.0, np.array(t["b_scales"]).reshape(k // 32, n) - 127)
    want = (a * np.repeat(sa, 32, axis=1)) @ (b * np.repeat(sb, 32, axis=0))
    return want.astype(np.float32)


@pytest.mark.parametrize("mx_set", [0, FAR_SET, WIDE_SET],
                         ids=["set0", "far", "wide"])
@pytest.mark.parametrize("fmt_a,fmt_b,shape", TILES,
                         ids=[f"{a}x{b}-{s}" for a, b, s in TILES])
def test_single_tile_is_bit_exact(native, fmt_a, fmt_b, shape, mx_set):
    t = native.mx_mfma_tile(0, fmt_a, fmt_b, shape, mx_set)
    assert (t["fmt_a"], t["fmt_b"], t["shape"], t["set"]) == (
        fmt_a, fmt_b, shape, mx_set)
    want = _numpy_tile(t)
    got = np.array(t["d_gpu"], dtype=np.float32).reshape(t["m"], t["n"])
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(  # noqa: T201 (figures before the asserts)
        f"{fmt_a}x{fmt_b} {shape} set={mx_set} log2_span={t['log2_span']:.2f} "
        f"mismatching={bad}/{got.size} max_abs={np.abs(want).max()}"
    )
    assert np.abs(want).max() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the host's own fixed-point tile agrees with both
    assert np.array_equal(
        np.array(t["d"], dtype=np.float32).reshape(t["m"], t["n"]), want)


def test_clean_sweep_covers_every_cu_and_simd(native, clean):
    cus = native.device_probe(0)["compute_units"]
    print(  # noqa: T201 (figures before the asserts)
        f"cus={cus} covered={clean['cus_covered']} "
        f"slots={clean['simd_slots_covered']} rounds={clean['rounds']} "
        f"per_xcc={clean['per_xcc']} elapsed_ms={clean['elapsed_ms']:.3f} "
        f"failing={clean['failing_units'][:4]}"
    )
    assert clean["compute_units"] == cus
    assert clean["cus_covered"] == cus
    assert clean["simd_slots_covered"] == 4 * cus
    assert sum(clean["per_xcc"].values()) == cus
    assert clean["uncovered_cus"] == 0
    assert 1 <= clean["rounds"] <= MAX_ROUNDS
    assert clean["failing_units"] == []
    assert clean["healthy"] is True


@pytest.mark.parametrize("bit,name", list(enumerate(BITS)), ids=BITS)
def test_each_comparison_is_live(native, clean, bit, name):
    from k8s_operator_libs_amd.validation import mx_matrix_check

    out = mx_matrix_check(0, reps=REPS, max_rounds=MAX_ROUNDS,
                          poison_all=True, poison_mask=1 << bit)
    assert out["healthy"] is False
    assert out["cus_covered"] == clean["cus_covered"]
    assert out["simd_slots_covered"] == clean["simd_slots_covered"]
    assert len(out["failing_units"]) == len(out["units"])
    assert all(u["fail_mask"] == 1 << bit for u in out["units"])
    assert all(u["failed"] == [name] for u in out["failing_units"])


def test_poisoned_cu_is_the_only_one_named(native, clean):
    from k8s_operator_libs_amd.validation import mx_matrix_check

    keys = sorted({u["key"] for u in clean["units"]})
    victim = keys[len(keys) // 2]  # from the middle, not the first
    out = mx_matrix_check(0, reps=REPS, max_rounds=MAX_ROUNDS,
                          poison_key=victim, poison_mask=1 << BITS.index("e2m3"))
    assert out["healthy"] is False
    assert {u["key"] for u in out["failing_units"]} == {victim}
    assert all(u["failed"] == ["e2m3"] for u in out["failing_units"])
    victim_simds = {u["simd"] for u in out["units"] if u["key"] == victim}
    assert {u["simd"] for u in out["failing_units"]} == victim_simds
    for u in out["units"]:
        if u["key"] != victim:
            assert u["fail_mask"] == 0, u
    assert out["cus_covered"] == clean["cus_covered"]
    assert out["simd_slots_covered"] == clean["simd_slots_covered"]


def test_health_report_carries_mx_matrix(native):
    from k8s_operator_libs_amd.validation import gpu_health_check

    report = gpu_health_check(require_gpu=True, mx=True,
                              bw_buf_mib=128, bw_iters=2)
    mx = report["checks"]["mx_matrix"]
    print(f"mx_matrix={mx}")  # noqa: T201 (figures before the asserts)
    assert report["healthy"], report
    assert mx["healthy"] is True
    assert mx["cus_covered"] == report["checks"]["device"]["compute_units"]
    assert set(mx["throughput_tflops"]) == {"e2m1", "e4m3"}
    assert "units" not in mx

    plain = gpu_health_check(require_gpu=True, bw_buf_mib=128, bw_iters=2)
    assert "mx_matrix" not in plain["checks"]


@pytest.mark.parametrize("fmt", ["e2m1", "e4m3"])
def test_mx_throughput_exceeds_the_bf16_floor(native, fmt):
    from k8s_operator_libs_amd.validation.gpu_health import MFMA_MIN_TFLOPS

    tflops = native.mx_throughput_tflops(0, fmt, 20000)
    print(f"mx {fmt} throughput = {tflops:.1f} TFLOP/s")  # noqa: T201
    assert tflops > MFMA_MIN_TFLOPS
