"""CPU-side tests for the per-CU coverage sweep.

``summarize_cu_coverage`` is pure, so it is driven with hand-built raw
tables of a small synthetic device (2 XCCs x 3 CUs).  The health-report
wiring is checked against a stub native module, and the host-computed
operand/expected tables are checked against numpy."""

import numpy as np
import pytest

from k8s_operator_libs_amd.validation import (
    cu_coverage,
    gpu_health,
    gpu_health_check,
    load_native_validator,
    summarize_cu_coverage,
)

XCCS, CUS_PER_XCC = 2, 3


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
        "elapsed_ms": 0.25,
    }


def test_summary_healthy_full_coverage():
    s = summarize_cu_coverage(_raw())
    assert s["healthy"] is True
    assert s["compute_units"] == 6
    assert s["cus_covered"] == 6
    assert s["simd_slots_covered"] == 24
    assert s["uncovered_cus"] == 0
    assert s["failing_units"] == []
    assert s["rounds"] == 1
    assert s["elapsed_ms"] == 0.25
    assert "units" not in s


def test_summary_per_xcc_counts():
    s = summarize_cu_coverage(_raw())
    assert s["per_xcc"] == {0: 3, 1: 3}
    assert sum(s["per_xcc"].values()) == s["cus_covered"]
    # drop one whole CU of XCC 1
    gone = _key(1, se=0, sh=0, cu=2)
    s = summarize_cu_coverage(_raw(skip_slots={(gone, i) for i in range(4)}))
    assert s["per_xcc"] == {0: 3, 1: 2}


@pytest.mark.parametrize("bit,name", [(1, "f32"), (2, "bf16"), (4, "fp8"), (8, "lds")])
def test_summary_decodes_each_fail_bit(bit, name):
    key = _key(1, se=1, sh=0, cu=1)
    s = summarize_cu_coverage(_raw(fail={(key, 2): bit}))
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
    s = summarize_cu_coverage(_raw(fail={(key, 0): 0xF, (key, 3): 0xA}))
    assert [u["failed"] for u in s["failing_units"]] == [
        ["f32", "bf16", "fp8", "lds"], ["bf16", "lds"],
    ]
    assert [u["simd"] for u in s["failing_units"]] == [0, 3]


def test_summary_missing_cu_is_unhealthy():
    gone = _key(0, se=1, sh=0, cu=1)
    s = summarize_cu_coverage(_raw(skip_slots={(gone, i) for i in range(4)}))
    assert s["healthy"] is False
    assert s["uncovered_cus"] == 1
    assert s["cus_covered"] == 5
    assert s["failing_units"] == []


def test_summary_three_simd_cu_is_unhealthy():
    key = _key(1, se=0, sh=0, cu=0)
    s = summarize_cu_coverage(_raw(skip_slots={(key, 3)}))
    assert s["cus_covered"] == 6
    assert s["uncovered_cus"] == 0
    assert s["simd_slots_covered"] == 23
    assert s["healthy"] is False


def test_summary_more_keys_than_cus_is_unhealthy():
    # a wrong placement-key layout shows up as a count mismatch, loudly
    s = summarize_cu_coverage(_raw(compute_units=5))
    assert s["cus_covered"] == 6
    assert s["healthy"] is False


class _StubNative:
    """Healthy stand-in for the native module; the sweep result is settable."""

    def __init__(self, coverage_raw):
        self.coverage_raw = coverage_raw
        self.coverage_calls = []

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

    def cu_coverage_check(self, device, **kw):
        self.coverage_calls.append((device, kw))
        return self.coverage_raw


TODAYS_CHECK_KEYS = {
    "smi", "device", "arch_ok", "mfma_f32_max_err", "mfma_bf16_max_err",
    "hbm_bandwidth_gbps", "lds_ok", "xgmi_ok",
}


def _install_stub(monkeypatch, stub):
    monkeypatch.setattr(gpu_health, "load_native_validator", lambda: stub)
    # keep the smi tools (a subprocess per report) out of these tests
    monkeypatch.setattr(
        gpu_health, "smi_probe", lambda: {"tool": None, "ok": False, "raw": ""}
    )


def test_health_report_without_coverage_is_unchanged(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True)
    assert set(report) == {"healthy", "checks"}
    assert set(report["checks"]) == TODAYS_CHECK_KEYS
    assert report["healthy"] is True
    assert stub.coverage_calls == []
    assert gpu_health_check(require_gpu=True, coverage=False) == report


def test_health_report_coverage_adds_key_and_gates(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, coverage=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS | {"cu_coverage"}
    cov = report["checks"]["cu_coverage"]
    assert cov["healthy"] is True and cov["cus_covered"] == 6
    assert "units" not in cov
    assert report["healthy"] is True
    assert len(stub.coverage_calls) == 1

    key = _key(0, se=1, sh=0, cu=1)
    stub.coverage_raw = _raw(fail={(key, 1): 4})
    report = gpu_health_check(require_gpu=True, coverage=True)
    assert report["healthy"] is False
    assert report["checks"]["cu_coverage"]["failing_units"][0]["failed"] == ["fp8"]
    # everything else is still fine: only the sweep gates it
    assert gpu_health_check(require_gpu=True)["healthy"] is True

    stub.coverage_raw = _raw(skip_slots={(key, 0)})
    assert gpu_health_check(require_gpu=True, coverage=True)["healthy"] is False


def test_python_wrapper_summarizes_and_keeps_units(monkeypatch):
    stub = _StubNative(_raw())
    monkeypatch.setattr(cu_coverage, "load_native_validator", lambda: stub)
    out = cu_coverage.cu_coverage_check(0, reps=2, poison_mask=2)
    assert stub.coverage_calls == [(0, {"reps": 2, "poison_mask": 2})]
    assert out["healthy"] is True
    assert len(out["units"]) == 24
    monkeypatch.setattr(cu_coverage, "load_native_validator", lambda: None)
    with pytest.raises(gpu_health.GpuHealthError):
        cu_coverage.cu_coverage_check(0)


@pytest.fixture(scope="module")
def reference():
    native = load_native_validator()
    if native is None:
        pytest.skip("native validator not built and not buildable here")
    return native.cu_coverage_reference()


def _tiles(reference, dtype):
    m, n = reference["m"], reference["n"]
    for entry in reference[dtype]:
        k = entry["k"]
        a = np.array(entry["a"], dtype=np.float32).reshape(m, k)
        b = np.array(entry["b"], dtype=np.float32).reshape(k, n)
        d = np.array(entry["d"], dtype=np.float32).reshape(m, n)
        yield a, b, d


@pytest.mark.parametrize("dtype,k", [("f32", 4), ("bf16", 32), ("fp8", 32)])
def test_reference_tables_against_numpy(reference, dtype, k):
    assert reference["sets"] >= 4
    assert len(reference[dtype]) == reference["sets"]
    seen = []
    for a, b, d in _tiles(reference, dtype):
        assert a.shape == (16, k) and b.shape == (k, 16)
        # operands decoded from their f32 / bf16 / e4m3 encodings are still
        # the small integers they were generated as
        for op in (a, b):
            assert np.array_equal(op, np.round(op))
            assert np.abs(op).max() <= 8
            assert len(np.unique(op)) > 8  # more than a couple of bit patterns
        # exact in any order: float64 accumulate equals the f32 table bitwise
        want = a.astype(np.float64) @ b.astype(np.float64)
        assert np.abs(want).max() <= 2048
        assert np.array_equal(want.astype(np.float32), d)
        # asymmetric: transposing a fragment or the output cannot pass
        assert not np.array_equal(a, b.T)
        assert not np.array_equal(d, d.T)
        seen.append((a, b, d))
    for i in range(len(seen)):
        for j in range(i + 1, len(seen)):
            for x, y in zip(seen[i], seen[j]):
                assert not np.array_equal(x, y)


def test_reference_dtypes_use_different_patterns(reference):
    bf16 = [a for a, _, _ in _tiles(reference, "bf16")]
    fp8 = [a for a, _, _ in _tiles(reference, "fp8")]
    for x, y in zip(bf16, fp8):
        assert not np.array_equal(x, y)
