"""Per-CU coverage sweep on a real MI355X.

The clean sweep must reach every CU and SIMD the device reports; the
data-only poison hook then proves that each of the four comparisons is live
and that a failure is attributed to the unit that produced it.  Nothing
here depends on timing: ``elapsed_ms`` is reported, never asserted."""

import pytest

pytestmark = pytest.mark.gpu

REPS = 4
MAX_ROUNDS = 8
BITS = {"f32": 1, "bf16": 2, "fp8": 4, "lds": 8}


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
    from k8s_operator_libs_amd.validation import cu_coverage_check

    return cu_coverage_check(0, reps=REPS, max_rounds=MAX_ROUNDS)


def _keys(summary):
    return sorted({u["key"] for u in summary["units"]})


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


def test_poisoned_cu_is_the_only_one_named(native, clean):
    from k8s_operator_libs_amd.validation import cu_coverage_check

    keys = _keys(clean)
    victim = keys[len(keys) // 2]  # from the middle, not the first
    out = cu_coverage_check(0, reps=REPS, max_rounds=MAX_ROUNDS,
                            poison_key=victim, poison_mask=BITS["bf16"])
    assert out["healthy"] is False
    assert {u["key"] for u in out["failing_units"]} == {victim}
    assert all(u["failed"] == ["bf16"] for u in out["failing_units"])
    # every SIMD of the victim that ran a wave failed, nothing else did
    victim_simds = {u["simd"] for u in out["units"] if u["key"] == victim}
    assert {u["simd"] for u in out["failing_units"]} == victim_simds
    for u in out["units"]:
        if u["key"] != victim:
            assert u["fail_mask"] == 0, u
    # the hook changes comparisons only, never coverage
    assert out["cus_covered"] == clean["cus_covered"]
    assert out["simd_slots_covered"] == clean["simd_slots_covered"]


@pytest.mark.parametrize("name", ["f32", "bf16", "fp8", "lds"])
def test_each_comparison_is_live(native, clean, name):
    from k8s_operator_libs_amd.validation import cu_coverage_check

    out = cu_coverage_check(0, reps=REPS, max_rounds=MAX_ROUNDS,
                            poison_all=True, poison_mask=BITS[name])
    assert out["healthy"] is False
    assert out["simd_slots_covered"] == clean["simd_slots_covered"]
    assert len(out["failing_units"]) == len(out["units"])
    assert all(u["fail_mask"] == BITS[name] for u in out["units"])
    assert all(u["failed"] == [name] for u in out["failing_units"])


def test_health_report_carries_coverage(native):
    from k8s_operator_libs_amd.validation import gpu_health_check

    report = gpu_health_check(require_gpu=True, coverage=True,
                              bw_buf_mib=128, bw_iters=2)
    assert report["healthy"], report
    cov = report["checks"]["cu_coverage"]
    assert cov["healthy"] is True
    assert cov["cus_covered"] == report["checks"]["device"]["compute_units"]
    assert "units" not in cov

    plain = gpu_health_check(require_gpu=True, bw_buf_mib=128, bw_iters=2)
    assert "cu_coverage" not in plain["checks"]
