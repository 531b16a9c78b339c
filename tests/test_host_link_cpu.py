"""Host-link data-integrity check, the parts that need no GPU: the unaligned
copy plan, the atomics reference against a pure-Python re-implementation of
its formulas, argument validation before any HIP call, the pure verdict on
hand-built raw tables, and the health-report and CLI wiring against a stub
native module."""

import copy
import json
import sys

import pytest

from k8s_operator_libs_amd.validation import (
    gpu_health,
    gpu_health_check,
    host_link,
    load_native_validator,
    summarize_host_link,
)

MASK = (1 << 64) - 1
LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128,
           129, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537]
OFFSETS = [(0, 0), (1, 0), (0, 1), (3, 3), (1, 2), (2, 3), (63, 65), (129, 7)]
SLOT_BYTES = 69632
WORDS = 131073


@pytest.fixture(scope="module")
def native():
    mod = load_native_validator()
    if mod is None:
        pytest.skip("native validator not built and not buildable here")
    return mod


# ---- the plan ---------------------------------------------------------------

def test_plan_has_every_length_with_every_offset_pair_both_ways(native):
    plan = native.host_link_plan()
    cases = plan["cases"]
    assert len(cases) == 464
    assert [c["case"] for c in cases] == list(range(464))
    for direction in ("h2d", "d2h"):
        got = sorted((c["len"], c["src_off"], c["dst_off"])
                     for c in cases if c["direction"] == direction)
        want = sorted((n, s, d) for n in LENGTHS for (s, d) in OFFSETS)
        assert got == want
    assert plan["slot_bytes"] == SLOT_BYTES
    assert plan["slot_bytes"] % 4096 == 0
    assert plan["slot_bytes"] >= 65537 + 129 + 2 * 64


def test_plan_cases_fit_their_slot_with_guard_bytes(native):
    plan = native.host_link_plan()
    for c in plan["cases"]:
        assert c["src_pos"] == plan["guard"] + c["src_off"]
        assert c["dst_pos"] == plan["guard"] + c["dst_off"]
        for pos in (c["src_pos"], c["dst_pos"]):
            assert pos >= 64, c
            assert pos + c["len"] + 64 <= plan["slot_bytes"], c


# ---- the atomics reference against the formulas ------------------------------

def py_hash(seed, i):
    """splitmix64 finaliser of (i + seed * golden ratio), mod 2^64."""
    z = (i + seed * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def py_atom_vals(seed, ident, rep):
    """Operands of thread ``ident`` in repetition ``rep``: words 2n and 2n + 1,
    n = 16 * ident + rep, of the pinned kind's atomics seed (seed + 6)."""
    n = 16 * ident + rep
    s = (seed + 6) & MASK
    return py_hash(s, 2 * n) & 0xFFFFFFFF, py_hash(s, 2 * n + 1)


def py_reference(seed, threads, reps, host_adds):
    add32, add64 = [0] * 64, [0] * 64
    for ident in range(threads):
        for rep in range(reps):
            a, b = py_atom_vals(seed, ident, rep)
            cell = (ident + rep) % 64
            add32[cell] = (add32[cell] + a) & 0xFFFFFFFF
            add64[cell] = (add64[cell] + b) & MASK
    for j in range(host_adds):
        a, b = py_atom_vals(seed, (1 << 40) + j, 0)
        add32[j % 64] = (add32[j % 64] + a) & 0xFFFFFFFF
        add64[j % 64] = (add64[j % 64] + b) & MASK
    return add32, add64


@pytest.mark.parametrize("seed,threads,reps,host_adds", [
    (1, 256, 2, 4096), (0x5EED, 64, 1, 0), (MASK, 320, 16, 64), (7, 0, 3, 128),
])
def test_reference_equals_the_formulas(native, seed, threads, reps, host_adds):
    ref = native.host_link_reference(seed, threads, reps, host_adds)
    add32, add64 = py_reference(seed, threads, reps, host_adds)
    assert list(ref["add32"]) == add32
    assert list(ref["add64"]) == add64
    assert [(d + h) & 0xFFFFFFFF for d, h in
            zip(ref["device_add32"], ref["host_add32"])] == add32
    assert [(d + h) & MASK for d, h in
            zip(ref["device_add64"], ref["host_add64"])] == add64
    assert ref["items"] == 2 * threads + 212


def test_words_come_from_the_hbm_reference(native):
    # the seed rule: phase p of kind k is the hash pattern of seed + 16k + p
    for kind, phase in ((0, 0), (1, 4), (2, 5)):
        got = native.hbm_pattern_reference("hash", 9 + 16 * kind + phase, 5, 3, False)
        assert list(got) == [py_hash(9 + 16 * kind + phase, 5 + k) for k in range(3)]


# ---- argument validation, before any HIP call --------------------------------

@pytest.mark.parametrize("kw", [
    {"nbytes": 4100}, {"nbytes": 4088}, {"nbytes": 0}, {"nbytes": (1 << 30) + 8},
    {"kinds": []}, {"kinds": ["mapped"]}, {"kinds": ["pinned", "pinned"]},
    {"blocks": -1}, {"atomics_blocks": -1}, {"reps": 0}, {"reps": 17},
    {"host_adds": -64}, {"host_adds": 100},
    {"max_records": -1}, {"max_records": 4097},
    {"poison_mask": 1 << 7}, {"poison_kind": 3}, {"poison_kind": -2},
    {"poison_word": -2}, {"poison_word": 1 << 17, "nbytes": 1 << 20},
    {"poison_case": 464}, {"poison_case": -2},
    {"poison_mask": 1}, {"poison_mask": 32},
    {"poison_mask": 1, "poison_word": 0, "poison_xor": 0},
    {"poison_mask": 32, "poison_case": 0, "poison_xor": 256},
    {"poison_mask": 64, "poison_xor": 1 << 32},
])
def test_bad_arguments_raise_value_error_without_a_gpu(native, kw):
    kw = dict(kw)
    nbytes = kw.pop("nbytes", 1 << 20)
    with pytest.raises(ValueError):
        native.host_link_check(0, nbytes, **kw)


def test_reference_validates_its_arguments(native):
    for kw in ({"reps": 0}, {"reps": 17}, {"host_adds": 1}, {"threads": 1 << 20}):
        with pytest.raises(ValueError):
            native.host_link_reference(**kw)


# ---- the pure verdict on hand-built raw tables -------------------------------

def _phase(compared, expected=None, errors=0, gbps=10.0):
    return {"compared": compared,
            "expected": compared if expected is None else expected,
            "errors": errors, "elapsed_ms": 1.0, "link_ms": 0.5, "gbps": gbps}


def _raw(kinds=("pinned", "registered", "pageable"), atomics=True, threads=256):
    lo = WORDS // 2
    full = {
        "h2d": _phase(WORDS), "d2h": _phase(WORDS), "zc_read": _phase(WORDS),
        "zc_write": _phase(WORDS), "duplex": _phase(lo + (WORDS - lo)),
        "unaligned": _phase(464 * SLOT_BYTES),
        "atomics": _phase(2 * threads + 212),
    }
    names = {
        "pinned": ["h2d", "d2h", "zc_read", "zc_write", "duplex", "unaligned"]
                  + (["atomics"] if atomics else []),
        "registered": ["h2d", "d2h", "zc_read", "zc_write", "duplex", "unaligned"],
        "pageable": ["h2d", "d2h", "unaligned"],
    }
    out_kinds = {}
    for kind in kinds:
        table = {"fail_mask": 0,
                 "phases": {p: copy.deepcopy(full[p]) for p in names[kind]}}
        if kind != "pageable":
            table["duplex_overlap"] = True
        out_kinds[kind] = table
    return {
        "bytes": 8 * WORDS, "words": WORDS, "seed": 1, "blocks": 8,
        "plan_cases": 464, "slot_bytes": SLOT_BYTES, "kinds": out_kinds,
        "fail_mask": 0, "error_count": 0, "xor_or": 0, "records": [],
        "records_dropped": 0, "atomics_supported": atomics,
        "atomics": {"threads": threads} if atomics else None,
        "elapsed_ms": 12.5,
    }


def _word_record(kind, phase, word, bit, side="host"):
    return {"kind": kind, "phase": phase, "side": side, "word": word,
            "byte_offset": 8 * word, "expected": 0xF0 ^ (1 << bit), "got": 0xF0,
            "flipped_bits": [bit]}


def _fail(raw, kind, phase, records, errors=None, dropped=0):
    raw = copy.deepcopy(raw)
    errors = len(records) + dropped if errors is None else errors
    bit = host_link.PHASES.index(phase)
    raw["kinds"][kind]["phases"][phase]["errors"] = errors
    raw["kinds"][kind]["fail_mask"] |= 1 << bit
    raw["fail_mask"] |= 1 << bit
    raw["error_count"] += errors
    raw["records"] += records
    raw["records_dropped"] += dropped
    return raw


def test_summary_clean_is_healthy():
    s = summarize_host_link(_raw())
    assert s["healthy"] is True and s["consistent"] is True
    assert s["failing_phases"] == {"pinned": [], "registered": [], "pageable": []}
    assert s["failing_words"] == [] and s["failing_cases"] == []
    assert s["failing_atomics"] == []
    assert s["atomics_supported"] is True
    assert set(s["rates_gbps"]["pageable"]) == {"h2d", "d2h", "unaligned"}
    assert "atomics" not in s["rates_gbps"]["pinned"]
    assert "records" not in s
    assert s["duplex_overlap"] == {"pinned": True, "registered": True}


@pytest.mark.parametrize("kind,phase", [
    ("pinned", "h2d"), ("pinned", "atomics"), ("registered", "duplex"),
    ("pageable", "unaligned"),
])
def test_summary_short_count_is_unhealthy_with_zero_errors(kind, phase):
    raw = _raw()
    raw["kinds"][kind]["phases"][phase]["compared"] -= 1
    s = summarize_host_link(raw)
    assert s["error_count"] == 0
    assert s["healthy"] is False
    assert s["short_phases"][kind] == [phase]
    assert s["failing_phases"][kind] == []


def test_summary_errors_in_one_kind_only():
    recs = [_word_record("registered", "zc_write", 384, 9),
            _word_record("registered", "zc_write", 128, 3)]
    s = summarize_host_link(_fail(_raw(), "registered", "zc_write", recs))
    assert s["healthy"] is False and s["consistent"] is True
    assert s["failing_phases"] == {"pinned": [], "registered": ["zc_write"],
                                   "pageable": []}
    assert [w["word"] for w in s["failing_words"]] == [128, 384]   # sorted
    assert s["failing_words"][0]["flipped_bits"] == [3]
    assert s["failing_words"][1]["byte_offset"] == 8 * 384
    assert s["error_count"] == 2


def test_summary_names_failing_cases_and_atomics():
    case = {"kind": "pageable", "phase": "unaligned", "side": "host", "case": 237,
            "direction": "d2h", "src_off": 1, "dst_off": 2, "len": 1,
            "byte_offset": 130, "expected": 0x41, "got": 0x40, "flipped_bits": [0]}
    atom = {"kind": "pinned", "phase": "atomics", "side": "host",
            "comparison": "add_u32", "op": "add_u32", "cell": 0,
            "expected": 6, "got": 7}
    raw = _fail(_fail(_raw(), "pageable", "unaligned", [case]),
                "pinned", "atomics", [atom])
    s = summarize_host_link(raw)
    assert s["healthy"] is False and s["consistent"] is True
    assert s["failing_cases"] == [{
        "kind": "pageable", "case": 237, "direction": "d2h", "src_off": 1,
        "dst_off": 2, "len": 1, "byte_offset": 130, "expected": 0x41,
        "got": 0x40, "flipped_bits": [0]}]
    assert s["failing_atomics"] == [{"comparison": "add_u32", "op": "add_u32",
                                     "cell": 0, "expected": 6, "got": 7}]
    assert s["failing_words"] == []
    assert s["fail_mask"] == (1 << 5) | (1 << 6)


def test_summary_atomics_unsupported_is_healthy_and_flagged():
    s = summarize_host_link(_raw(atomics=False))
    assert s["healthy"] is True
    assert s["atomics_supported"] is False
    assert "atomics" not in s["compared"]["pinned"]
    # a table that claims support but ran no atomics phase is not clean
    raw = _raw(atomics=False)
    raw["atomics_supported"] = True
    assert summarize_host_link(raw)["healthy"] is False
    # and one that ran the phase without support contradicts itself
    raw = _raw(atomics=True)
    raw["atomics_supported"] = False
    assert summarize_host_link(raw)["healthy"] is False


def test_summary_records_dropped_handling():
    recs = [_word_record("pinned", "d2h", w, 1) for w in range(4)]
    raw = _fail(_raw(), "pinned", "d2h", recs, dropped=96)
    s = summarize_host_link(raw)
    assert s["error_count"] == 100 and s["records_dropped"] == 96
    assert len(s["failing_words"]) == 4
    assert s["healthy"] is False and s["consistent"] is True
    # the cap at zero: errors and a dropped count, no record
    raw = _fail(_raw(), "pinned", "h2d", [], dropped=1)
    s = summarize_host_link(raw)
    assert s["failing_words"] == [] and s["records_dropped"] == 1
    assert s["healthy"] is False and s["consistent"] is True
    # contradictions: errors that the phases do not account for, records
    # without errors
    raw = _raw()
    raw["error_count"] = 1
    s = summarize_host_link(raw)
    assert s["consistent"] is False and s["healthy"] is False
    raw = _raw()
    raw["records"] = [_word_record("pinned", "d2h", 0, 0)]
    s = summarize_host_link(raw)
    assert s["consistent"] is False and s["healthy"] is False


def test_summary_subset_of_kinds_and_wrong_plan():
    assert summarize_host_link(_raw(kinds=("pageable",)))["healthy"] is True
    raw = _raw()
    raw["plan_cases"] = 463
    assert summarize_host_link(raw)["healthy"] is False
    raw = _raw()
    del raw["kinds"]["registered"]["phases"]["zc_read"]   # a phase that never ran
    assert summarize_host_link(raw)["healthy"] is False
    raw = _raw()
    raw["kinds"] = {}
    assert summarize_host_link(raw)["healthy"] is False


# ---- health report and CLI against a stub native module ----------------------

class _StubNative:
    def __init__(self, link_raw):
        self.link_raw = link_raw
        self.link_calls = []

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

    def host_link_check(self, device, nbytes, **kw):
        self.link_calls.append((device, nbytes, kw))
        return self.link_raw


TODAYS_CHECK_KEYS = {
    "smi", "device", "arch_ok", "mfma_f32_max_err", "mfma_bf16_max_err",
    "hbm_bandwidth_gbps", "lds_ok", "xgmi_ok",
}


def _install_stub(monkeypatch, stub):
    monkeypatch.setattr(gpu_health, "load_native_validator", lambda: stub)
    monkeypatch.setattr(
        gpu_health, "smi_probe", lambda: {"tool": None, "ok": False, "raw": ""}
    )


def test_health_report_default_never_calls_the_check(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS
    assert report["healthy"] is True
    assert gpu_health_check(require_gpu=True, hostlink=False) == report
    assert stub.link_calls == []


def test_health_report_hostlink_adds_key_and_gates_both_ways(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, hostlink=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS | {"host_link"}
    summary = report["checks"]["host_link"]
    assert summary["healthy"] is True
    assert "records" not in summary and "phases" not in summary
    assert report["healthy"] is True
    assert stub.link_calls == [(0, 64 << 20, {})]

    stub.link_raw = _fail(_raw(), "pinned", "h2d",
                          [_word_record("pinned", "h2d", 5, 0, "device")])
    report = gpu_health_check(require_gpu=True, hostlink=True)
    assert report["healthy"] is False
    assert report["checks"]["host_link"]["failing_words"][0]["word"] == 5
    # everything else is still fine: only the host-link check gates it
    assert gpu_health_check(require_gpu=True)["healthy"] is True

    stub.link_raw = _raw()
    stub.link_raw["kinds"]["pageable"]["phases"]["d2h"]["compared"] -= 1
    assert gpu_health_check(require_gpu=True, hostlink=True)["healthy"] is False

    stub.link_raw = _raw()
    stub.link_calls.clear()
    assert gpu_health_check(require_gpu=True, hostlink=True,
                            hostlink_mib=1)["healthy"] is True
    assert stub.link_calls == [(0, 1 << 20, {})]


@pytest.mark.parametrize("argv,calls", [
    (["gpu_health"], []),
    (["gpu_health", "--hostlink"], [(0, 64 << 20, {})]),
    (["gpu_health", "--hostlink-mib=8"], [(0, 8 << 20, {})]),
    (["gpu_health", "--hostlink", "--hostlink-mib=0.5"], [(0, 1 << 19, {})]),
    (["gpu_health", "--memory-not", "--hostlink"], [(0, 64 << 20, {})]),
], ids=["plain", "hostlink", "mib-implies", "both", "among-others"])
def test_main_maps_hostlink_flags(monkeypatch, capsys, argv, calls):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    monkeypatch.setattr(sys, "argv", argv)
    assert gpu_health.main() == 0
    assert stub.link_calls == calls
    printed = json.loads(capsys.readouterr().out)
    assert ("host_link" in printed["checks"]) == bool(calls)

    stub.link_raw = _fail(_raw(), "pinned", "d2h",
                          [_word_record("pinned", "d2h", 1, 1)])
    if calls:
        assert gpu_health.main() == 1


def test_python_wrapper_passes_keywords_and_keeps_raw_lists(monkeypatch):
    raw = _fail(_raw(), "pinned", "d2h", [_word_record("pinned", "d2h", 1, 1)])
    stub = _StubNative(raw)
    monkeypatch.setattr(host_link, "load_native_validator", lambda: stub)
    out = host_link.host_link_check(0, mib=2, reps=1, poison_mask=2)
    assert stub.link_calls == [(0, 2 << 20, {"reps": 1, "poison_mask": 2})]
    assert out["healthy"] is False
    assert out["records"] == raw["records"]
    assert out["phases"]["pageable"] == raw["kinds"]["pageable"]["phases"]
    assert out["atomics"] == raw["atomics"]
    monkeypatch.setattr(host_link, "load_native_validator", lambda: None)
    with pytest.raises(gpu_health.GpuHealthError):
        host_link.host_link_check(0)
