"""CPU-side tests for the HBM data-integrity check.

The host-only pattern reference is checked against a numpy ``uint64``
re-implementation written from the formulas, the native entry point's
argument validation is exercised without a device, ``summarize_hbm_integrity``
is driven with hand-built raw tables, and the health-report and CLI wiring is
checked against a stub native module."""

import numpy as np
import pytest

from k8s_operator_libs_amd.validation import (
    gpu_health,
    gpu_health_check,
    hbm_integrity,
    load_native_validator,
    summarize_hbm_integrity,
)

MASK = (1 << 64) - 1


def np_pattern(pattern, seed, first_word, count, inverted=False):
    """value(pattern, seed, i) for i in [first_word, first_word + count),
    all arithmetic mod 2^64."""
    i = np.arange(count, dtype=np.uint64) + np.uint64(first_word)
    if pattern == "checker":
        out = np.where(i & np.uint64(1), np.uint64(0x5555555555555555),
                       np.uint64(0xAAAAAAAAAAAAAAAA))
    else:
        with np.errstate(over="ignore"):
            z = i + np.uint64((seed * 0x9E3779B97F4A7C15) & MASK)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            out = z ^ (z >> np.uint64(31))
    return ~out if inverted else out


@pytest.fixture(scope="module")
def native():
    mod = load_native_validator()
    if mod is None:
        pytest.skip("native validator not built and not buildable here")
    return mod


@pytest.mark.parametrize("pattern", ["hash", "checker"])
@pytest.mark.parametrize("seed", [1, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("inverted", [False, True])
@pytest.mark.parametrize("first_word", [0, 2**32 - 8])
def test_reference_against_numpy(native, pattern, seed, inverted, first_word):
    got = native.hbm_pattern_reference(pattern, seed, first_word, 16, inverted)
    want = np_pattern(pattern, seed, first_word, 16, inverted)
    assert len(got) == 16
    assert all(isinstance(v, int) and 0 <= v <= MASK for v in got)
    assert got == [int(v) for v in want]


def test_reference_known_answers(native):
    # splitmix64's first output from state 0 is the hash of (seed 1, word 0)
    assert native.hbm_pattern_reference("hash", 1, 0, 1) == [0xE220A8397B1DCDAF]
    assert native.hbm_pattern_reference("checker", 7, 0, 2) == [
        0xAAAAAAAAAAAAAAAA, 0x5555555555555555,
    ]
    assert native.hbm_pattern_reference("checker", 7, 1, 1, inverted=True) == [
        0xAAAAAAAAAAAAAAAA,
    ]


@pytest.mark.parametrize("seed", [1, 0xDEADBEEFCAFEF00D])
def test_hash_words_distinct_and_every_bit_toggles(native, seed):
    words = native.hbm_pattern_reference("hash", seed, 0, 4096)
    assert words == [int(v) for v in np_pattern("hash", seed, 0, 4096)]
    assert len(set(words)) == 4096
    ones = zeros = 0
    for w in words:
        ones |= w
        zeros |= ~w & MASK
    assert ones == MASK and zeros == MASK


def test_reference_limits(native):
    assert len(native.hbm_pattern_reference("hash", 1, 5, 65536)) == 65536
    assert native.hbm_pattern_reference("hash", 1, 5, 0) == []
    with pytest.raises(ValueError):
        native.hbm_pattern_reference("hash", 1, 0, 65537)
    with pytest.raises(ValueError):
        native.hbm_pattern_reference("walking_ones", 1, 0, 4)


@pytest.mark.parametrize("kw", [
    {"nbytes": 1024 + 4},
    {"nbytes": 1024, "chunk_bytes": 0},
    {"nbytes": 1024, "chunk_bytes": 100},
    {"nbytes": 1024, "passes": 0},
    {"nbytes": 1024, "passes": 17},
    {"nbytes": 1024, "max_records": 0},
    {"nbytes": 1024, "max_records": 4097},
    {"nbytes": 1024, "poison_word": 3, "poison_xor": 0},
    {"nbytes": 1024, "poison_word": -2},
    {"nbytes": 1024, "poison_phase": 4},  # passes=1 + checker: phases 0..3
    {"nbytes": 1024, "checker": False, "poison_phase": 2},
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_arguments_are_validated_before_any_device_call(native, kw):
    # std::invalid_argument -> ValueError; a HIP failure would be RuntimeError
    with pytest.raises(ValueError):
        native.hbm_pattern_check(0, **kw)


WORDS = 1000
CHUNK_WORDS = 400


def _record(word, phase, expected, flip):
    return {
        "word": word, "byte_offset": 8 * word, "chunk": word // CHUNK_WORDS,
        "phase": phase, "expected": expected, "got": expected ^ flip,
    }


def _raw(records=(), error_count=None, verified_short=0, records_dropped=0,
         beyond_cache=False):
    records = list(records)
    xor_or = 0
    for r in records:
        xor_or |= r["expected"] ^ r["got"]
    phases = []
    verify_index = 0
    for p, (pattern, seed) in enumerate([("hash", 1), ("checker", 0)]):
        for k, kind in enumerate(("fill", "verify_invert", "verify")):
            phases.append({
                "index": 3 * p + k, "pattern": pattern, "seed": seed,
                "kind": kind,
                "verify_index": None if kind == "fill" else verify_index,
                "ms": 1.0, "gbps": 100.0 * (k + 1) + 10.0 * p,
            })
            verify_index += kind != "fill"
    return {
        "bytes": 8 * WORDS, "words": WORDS, "first_word": 0,
        "chunks": [
            {"index": 0, "first_word": 0, "bytes": 3200},
            {"index": 1, "first_word": 400, "bytes": 3200},
            {"index": 2, "first_word": 800, "bytes": 1600},
        ],
        "phases": phases,
        "words_verified": 4 * WORDS - verified_short,
        "words_expected": 4 * WORDS,
        "error_count": len(records) if error_count is None else error_count,
        "xor_or": xor_or,
        "records": records,
        "records_dropped": records_dropped,
        "elapsed_ms": 6.0,
        "beyond_cache": beyond_cache,
    }


def test_summary_clean():
    s = summarize_hbm_integrity(_raw())
    assert s["healthy"] is True
    assert s["error_count"] == 0
    assert s["flipped_bits"] == []
    assert s["failing_words"] == []
    assert s["records_dropped"] == 0
    assert s["recorded_errors_per_chunk"] == {}
    assert s["words_verified"] == s["words_expected"] == 4 * WORDS
    assert s["bytes"] == 8 * WORDS and s["words"] == WORDS and s["chunks"] == 3
    assert s["beyond_cache"] is False
    assert summarize_hbm_integrity(_raw(beyond_cache=True))["beyond_cache"] is True
    # median over the two patterns' phases of each kind
    assert s["gbps_median"] == {
        "fill": 105.0, "verify_invert": 205.0, "verify": 305.0,
    }
    assert s["elapsed_ms"] == 6.0
    assert "records" not in s and "phases" not in s


@pytest.mark.parametrize("k", [0, 37, 63])
def test_summary_single_bit_record(k):
    s = summarize_hbm_integrity(_raw([_record(123, 1, 0x0123456789ABCDEF, 1 << k)]))
    assert s["healthy"] is False
    assert s["error_count"] == 1
    assert s["flipped_bits"] == [k]
    assert len(s["failing_words"]) == 1
    w = s["failing_words"][0]
    assert (w["word"], w["byte_offset"], w["chunk"], w["phase"]) == (123, 984, 0, 1)
    assert w["flipped_bits"] == [k]
    assert w["expected"] ^ w["got"] == 1 << k
    assert s["recorded_errors_per_chunk"] == {0: 1}


def test_summary_multi_bit_records_sorted_with_own_bits():
    recs = [
        _record(900, 0, MASK, (1 << 5) | (1 << 40)),
        _record(401, 3, 0, 1 << 63),
        _record(401, 2, 0, (1 << 0) | (1 << 1) | (1 << 2)),
    ]
    s = summarize_hbm_integrity(_raw(recs))
    assert s["healthy"] is False
    assert s["flipped_bits"] == [0, 1, 2, 5, 40, 63]
    assert [(w["word"], w["phase"]) for w in s["failing_words"]] == [
        (401, 2), (401, 3), (900, 0),
    ]
    assert [w["flipped_bits"] for w in s["failing_words"]] == [
        [0, 1, 2], [63], [5, 40],
    ]
    assert s["recorded_errors_per_chunk"] == {1: 2, 2: 1}


def test_summary_short_coverage_is_unhealthy_with_zero_errors():
    s = summarize_hbm_integrity(_raw(verified_short=1))
    assert s["error_count"] == 0 and s["failing_words"] == []
    assert s["words_verified"] == s["words_expected"] - 1
    assert s["healthy"] is False


def test_summary_errors_without_records_is_unhealthy():
    s = summarize_hbm_integrity(_raw(error_count=3))
    assert s["failing_words"] == []
    assert s["error_count"] == 3
    assert s["healthy"] is False


def test_summary_records_without_errors_is_unhealthy():
    s = summarize_hbm_integrity(_raw([_record(7, 0, 5, 4)], error_count=0))
    assert s["error_count"] == 0
    assert len(s["failing_words"]) == 1
    assert s["healthy"] is False


def test_summary_carries_records_dropped():
    recs = [_record(w, 0, 0, 2) for w in range(4)]
    s = summarize_hbm_integrity(_raw(recs, error_count=10, records_dropped=6))
    assert s["records_dropped"] == 6
    assert s["error_count"] == 10
    assert len(s["failing_words"]) == 4
    assert s["healthy"] is False


class _StubNative:
    """Healthy stand-in for the native module; the pattern result is settable."""

    def __init__(self, hbm_raw):
        self.hbm_raw = hbm_raw
        self.hbm_calls = []

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

    def hbm_pattern_check(self, device, nbytes, **kw):
        self.hbm_calls.append((device, nbytes, kw))
        return self.hbm_raw


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


def test_health_report_without_memory_is_unchanged(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True)
    assert set(report) == {"healthy", "checks"}
    assert set(report["checks"]) == TODAYS_CHECK_KEYS
    assert report["healthy"] is True
    assert gpu_health_check(require_gpu=True, memory=False) == report
    # a size alone does not switch the check on
    assert gpu_health_check(require_gpu=True, memory_mib=64) == report
    assert stub.hbm_calls == []


def test_health_report_memory_adds_key_and_gates(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, memory=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS | {"hbm_integrity"}
    mem = report["checks"]["hbm_integrity"]
    assert mem["healthy"] is True
    assert "records" not in mem and "phases" not in mem
    assert report["healthy"] is True
    assert stub.hbm_calls == [(0, 4096 * 2**20, {})]  # the default size

    stub.hbm_raw = _raw([_record(5, 2, 0xAAAAAAAAAAAAAAAA, 1 << 9)])
    report = gpu_health_check(require_gpu=True, memory=True, memory_mib=64)
    assert report["healthy"] is False
    mem = report["checks"]["hbm_integrity"]
    assert mem["flipped_bits"] == [9]
    assert mem["failing_words"][0]["word"] == 5
    assert "records" not in mem and "phases" not in mem
    assert stub.hbm_calls[-1] == (0, 64 * 2**20, {})
    # everything else is still fine: only the memory check gates it
    assert gpu_health_check(require_gpu=True)["healthy"] is True

    stub.hbm_raw = _raw(verified_short=1)
    assert gpu_health_check(require_gpu=True, memory=True)["healthy"] is False


@pytest.mark.parametrize("argv,calls", [
    (["gpu_health"], []),
    (["gpu_health", "--memory"], [(0, 4096 * 2**20, {})]),
    (["gpu_health", "--memory", "--memory-mib=64"], [(0, 64 * 2**20, {})]),
    (["gpu_health", "--memory-mib=64"], [(0, 67108864, {})]),
    (["gpu_health", "--memory", "--memory-mib=0"], [(0, 0, {})]),
], ids=["plain", "memory", "memory+mib", "mib-implies-memory", "all-free"])
def test_main_maps_memory_flags(monkeypatch, capsys, argv, calls):
    import json
    import sys

    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    monkeypatch.setattr(sys, "argv", argv)
    assert gpu_health.main() == 0
    assert stub.hbm_calls == calls
    printed = json.loads(capsys.readouterr().out)
    assert ("hbm_integrity" in printed["checks"]) == bool(calls)

    stub.hbm_raw = _raw(error_count=1)
    if calls:
        assert gpu_health.main() == 1


def test_python_wrapper_converts_mib_and_keeps_raw_lists(monkeypatch):
    stub = _StubNative(_raw([_record(9, 0, 1, 1)]))
    monkeypatch.setattr(hbm_integrity, "load_native_validator", lambda: stub)
    out = hbm_integrity.hbm_integrity_check(0, mib=1.5, passes=2, max_records=8)
    assert stub.hbm_calls == [(0, 1572864, {"passes": 2, "max_records": 8})]
    assert out["healthy"] is False
    assert out["records"] == stub.hbm_raw["records"]
    assert len(out["phases"]) == 6
    hbm_integrity.hbm_integrity_check(0, mib=(3 * 2**20 + 8) / 2**20)
    assert stub.hbm_calls[-1][1] == 3 * 2**20 + 8
    with pytest.raises(ValueError):
        hbm_integrity.hbm_integrity_check(0, mib=-1)
    monkeypatch.setattr(hbm_integrity, "load_native_validator", lambda: None)
    with pytest.raises(gpu_health.GpuHealthError):
        hbm_integrity.hbm_integrity_check(0)
