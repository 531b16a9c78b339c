"""CPU-side tests for the cross-XCD hand-off and atomics check.

The host-only reference is checked against a numpy ``uint64`` re-implementation
written from the formulas (slab words and every atomic total, including the
u64 wrap-around and the f32 sums), the f32 bound and the argument validation
are exercised without a device, ``summarize_xcd_fabric`` is driven with
hand-built raw tables, and the health-report and CLI wiring is checked against
a stub native module."""

import copy

import numpy as np
import pytest

from k8s_operator_libs_amd.validation import (
    gpu_health,
    gpu_health_check,
    load_native_validator,
    summarize_xcd_fabric,
    xcd_fabric,
)

MASK = (1 << 64) - 1
STATIC_KEY = 0x5354415449435F58
ATOM_KEYS = (0x41544F4D31, 0x41544F4D32, 0x41544F4D33)
U = np.uint64


def np_hash(seed, i):
    """splitmix64 finaliser of (i + seed * golden ratio), mod 2^64."""
    i = np.asarray(i, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = i + U((seed * 0x9E3779B97F4A7C15) & MASK)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def np_line(seed, blocks, slab_lines, round_, rep, block, line):
    """(first word index, header words 0-7, payload words 8-15) of one line."""
    first = (((rep * blocks + block) * slab_lines) + line) * 16
    idx = np.arange(8, dtype=np.uint64) + U(first)
    header = np_hash(seed ^ STATIC_KEY, idx)
    payload = np_hash((seed + round_) & MASK, idx + U(8))
    return first, [int(v) for v in header], [int(v) for v in payload]


def np_atomics(seed, threads, reps, cells):
    """Every cell total after `threads` threads ran `reps` repetitions: thread
    i, repetition r hits cell (i + r) % cells."""
    ids = np.repeat(np.arange(threads, dtype=np.uint64), reps)
    rep = np.tile(np.arange(reps, dtype=np.uint64), threads)
    n = ids * U(64) + rep
    cell = ((ids + rep) % U(cells)).astype(np.int64)
    h1, h2, h3 = (np_hash(seed ^ k, n) for k in ATOM_KEYS)
    add32 = (h1 & U(0xFFFFFFFF)).astype(np.uint32)
    addf = ((h1 >> U(32)) % U(17)).astype(np.int64) - 8
    xor = ((h1 >> U(20)) & U(0xFFFFFFFF)).astype(np.uint32)
    one = np.uint32(1)
    or_ = np.where(((h2 >> U(40)) & U(1023)) == 0,
                   one << ((h2 >> U(8)) & U(31)).astype(np.uint32),
                   np.uint32(0)).astype(np.uint32)
    and_ = np.where(((h2 >> U(50)) & U(1023)) == 0,
                    ~(one << ((h2 >> U(16)) & U(31)).astype(np.uint32)),
                    np.uint32(0xFFFFFFFF)).astype(np.uint32)
    out = {
        "add_u32": np.zeros(cells, np.uint32),
        "add_u64": np.zeros(cells, np.uint64),
        "add_f32": np.zeros(cells, np.int64),
        "max_u64": np.zeros(cells, np.uint64),
        "min_u64": np.full(cells, MASK, np.uint64),
        "xor_u32": np.zeros(cells, np.uint32),
        "or_u32": np.zeros(cells, np.uint32),
        "and_u32": np.full(cells, 0xFFFFFFFF, np.uint32),
    }
    with np.errstate(over="ignore"):
        np.add.at(out["add_u32"], cell, add32)
        np.add.at(out["add_u64"], cell, h2)
    np.add.at(out["add_f32"], cell, addf)
    np.maximum.at(out["max_u64"], cell, h3)
    np.minimum.at(out["min_u64"], cell, h3)
    np.bitwise_xor.at(out["xor_u32"], cell, xor)
    np.bitwise_or.at(out["or_u32"], cell, or_)
    np.bitwise_and.at(out["and_u32"], cell, and_)
    magnitude = np.zeros(cells, np.int64)
    np.add.at(magnitude, cell, np.abs(addf))
    result = {k: [int(v) for v in arr] for k, arr in out.items()}
    result["add_f32"] = [float(v) for v in out["add_f32"]]
    return result, int(magnitude.max())


@pytest.fixture(scope="module")
def native():
    mod = load_native_validator()
    if mod is None:
        pytest.skip("native validator not built and not buildable here")
    return mod


@pytest.mark.parametrize("seed", [1, 0xDEADBEEFCAFEF00D, MASK])
@pytest.mark.parametrize("where", [
    # blocks, group, slab_lines, reps, round, rep, block, line
    (2, 2, 1, 1, 0, 0, 0, 0),
    (2, 2, 1, 1, -1, 0, 1, 0),
    (6, 2, 1, 3, 1, 2, 5, 0),
    (496, 16, 8, 8, 7, 7, 495, 7),
    (9, 3, 5, 2, 63, 1, 4, 3),
])
def test_reference_lines_against_numpy(native, seed, where):
    blocks, group, slab_lines, reps, round_, rep, block, line = where
    ref = native.xcd_fabric_reference(
        blocks, seed=seed, reps=reps, group=group, slab_lines=slab_lines,
        round=round_, rep=rep, block=block, line=line)
    first, header, payload = np_line(seed, blocks, slab_lines, round_, rep,
                                     block, line)
    assert ref["first_word"] == first
    assert ref["header"] == header
    assert ref["payload"] == payload
    groups = blocks // group
    assert (ref["member"], ref["group_index"]) == (block // groups, block % groups)
    assert ref["atomics"] is None
    # header and payload never coincide, and the payload moves every round
    assert set(header).isdisjoint(payload)
    if round_ >= 0:
        prev = native.xcd_fabric_reference(
            blocks, seed=seed, reps=reps, group=group, slab_lines=slab_lines,
            round=round_ - 1, rep=rep, block=block, line=line)
        assert prev["header"] == header
        assert set(prev["payload"]).isdisjoint(payload)


def test_reference_known_answer(native):
    # splitmix64's first output from state 0 is the hash of (seed 1, word 0);
    # word 8 of line 0 in round 0 with seed 1 is hash(1, 8)
    ref = native.xcd_fabric_reference(2, seed=1, reps=1, group=2, slab_lines=1)
    assert ref["payload"][0] == int(np_hash(1, [8])[0])
    assert int(np_hash(1, [0])[0]) == 0xE220A8397B1DCDAF
    assert ref["header"][0] == int(np_hash(1 ^ STATIC_KEY, [0])[0])


@pytest.mark.parametrize("seed,threads,reps,cells", [
    (1, 512, 1, 64),
    (0x5EED, 2048, 8, 64),
    (0xDEADBEEFCAFEF00D, 1536, 2, 7),
    (7, 4096, 64, 4096),
    (3, 300, 5, 1),
])
def test_reference_atomic_totals_against_numpy(native, seed, threads, reps, cells):
    ref = native.xcd_fabric_reference(
        2, seed=seed, reps=reps, group=2, slab_lines=1, cells=cells,
        threads=threads)["atomics"]
    want, magnitude = np_atomics(seed, threads, reps, cells)
    assert magnitude <= 2**23
    assert set(ref) == set(want)
    for op in want:
        assert list(ref[op]) == want[op], op
    # every f32 total is an integer that f32 holds exactly
    assert all(float(np.float32(v)) == v for v in ref["add_f32"])


def test_reference_u64_add_wraps(native):
    # 4096 adds of full-width words into one cell: the exact sum is far
    # beyond 2^64 and the reference keeps it modulo 2^64
    threads, reps = 1024, 4
    ids = np.repeat(np.arange(threads, dtype=np.uint64), reps)
    rep = np.tile(np.arange(reps, dtype=np.uint64), threads)
    h2 = np_hash(5 ^ ATOM_KEYS[1], ids * U(64) + rep)
    exact = sum(int(v) for v in h2)
    assert exact > 100 * 2**64
    ref = native.xcd_fabric_reference(2, seed=5, reps=reps, group=2,
                                      slab_lines=1, cells=1, threads=threads)
    assert ref["atomics"]["add_u64"] == [exact & MASK]


def test_f32_bound_is_enforced(native):
    # 2^18 threads x 64 reps into one cell: about 7e7 > 2^23
    _, magnitude = np_atomics(9, 2**12, 64, 1)
    assert magnitude * 64 > 2**23  # 2^18 threads carry 64x this
    with pytest.raises(ValueError, match="2\\^23"):
        native.xcd_fabric_reference(2, seed=9, reps=64, group=2, slab_lines=1,
                                    cells=1, threads=2**18)
    # just enough cells and the same work is accepted
    ok = native.xcd_fabric_reference(2, seed=9, reps=64, group=2, slab_lines=1,
                                     cells=64, threads=2**15)
    assert len(ok["atomics"]["add_f32"]) == 64


@pytest.mark.parametrize("kw", [
    {"reps": 0}, {"reps": 65},
    {"group": 1}, {"group": 65},
    {"slab_lines": 0}, {"slab_lines": 33},
    {"cells": 0}, {"cells": 4097},
    {"blocks": -16}, {"blocks": 24}, {"group": 3, "blocks": 8},
    {"blocks": 1040},
    {"max_rounds": 1}, {"max_rounds": 65},
    {"max_records": 0}, {"max_records": 4097},
    {"poison_mask": 1 << 9},
    {"poison_pair": -2}, {"poison_pair": 256},
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_arguments_are_validated_before_any_device_call(native, kw):
    # std::invalid_argument -> ValueError; a HIP failure would be RuntimeError
    with pytest.raises(ValueError):
        native.xcd_fabric_check(0, **kw)


@pytest.mark.parametrize("kw", [
    {"blocks": 0}, {"blocks": 3}, {"reps": 0}, {"group": 1},
    {"slab_lines": 33}, {"cells": 0}, {"round": -2}, {"round": 64},
    {"rep": 1}, {"block": 2}, {"line": 1}, {"threads": 2**22 + 1},
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_reference_arguments_are_validated(native, kw):
    args = {"blocks": 2, "reps": 1, "group": 2, "slab_lines": 1}
    args.update(kw)
    blocks = args.pop("blocks")
    with pytest.raises(ValueError):
        native.xcd_fabric_reference(blocks, **args)


# ---- summarize_xcd_fabric on hand-built raw tables -------------------------

ROUNDS, REPS, GROUP, GROUPS, SLAB = 2, 2, 2, 3, 4
EPISODES = ROUNDS * REPS * GROUPS
LINES = EPISODES * GROUP * SLAB
CELLS = 4
OPS = ("add_u32", "add_u64", "add_f32", "max_u64", "min_u64", "xor_u32",
       "or_u32", "and_u32")


def _raw(xccs=(0, 1)):
    """A clean raw table: every pair of `xccs` covered, lines split evenly."""
    n = len(xccs) ** 2
    assert LINES % n == 0
    pairs = [{"writer_xcc": w, "reader_xcc": r, "words": 8 * LINES // n,
              "lines": LINES // n, "extra_lines": 0, "errors": 0}
             for w in xccs for r in xccs]
    totals = {op: [c + 1 for c in range(CELLS)] for op in OPS}
    totals["add_f32"] = [float(c) for c in range(CELLS)]
    adders = [0] * 16
    for x in xccs:
        adders[x] = 8
    return {
        "compute_units": 4, "seed": 1, "reps": REPS, "group": GROUP,
        "groups": GROUPS, "blocks": GROUP * GROUPS, "slab_lines": SLAB,
        "cells": CELLS, "rounds": ROUNDS, "max_rounds": 8,
        "round_ms": [0.5, 0.25],
        "episodes_completed": EPISODES, "episodes_expected": EPISODES,
        "lines_verified": LINES, "lines_expected": LINES,
        "extra_lines_verified": 0,
        "header_lines_verified": LINES * GROUP,
        "header_lines_expected": LINES * GROUP,
        "payload_errors": 0, "header_errors": 0, "error_count": 0,
        "ticket_counter_errors": 0, "tickets_out_of_range": 0,
        "writer_xcc_out_of_range": 0,
        "pairs": pairs, "pairs_covered": n, "xcc_seen": len(xccs),
        "xcc_ids": list(xccs), "writes_per_xcc": [0] * 16,
        "records": [], "records_dropped": 0,
        "atomics": {
            "workgroups": 8, "threads": 2048, "totals": totals,
            "expected": copy.deepcopy(totals), "mismatches": [],
            "ticket_counter": 2048, "tickets_expected": 2048,
            "tickets_missing": 0, "tickets_out_of_range": 0,
            "claims": [1, 2, 3, 4], "confirms": [1, 2, 3, 4],
            "adders_per_xcc": adders, "ms": 0.25,
        },
        "elapsed_ms": 1.0,
    }


def _record(kind="payload", writer=0, reader=1, stale=False):
    return {
        "round": 1, "rep": 0, "group": 2, "member": 1, "block": 5, "line": 3,
        "word": 9 if kind == "payload" else 2,
        "writer_xcc": writer if kind == "payload" else None,
        "reader_xcc": reader, "kind": kind, "expected": 0x1234,
        "got": 0x1235, "stale": stale,
    }


def _with_payload_error(raw, writer=0, reader=1, stale=False):
    raw["records"].append(_record("payload", writer, reader, stale))
    raw["payload_errors"] += 1
    raw["error_count"] += 1
    for p in raw["pairs"]:
        if (p["writer_xcc"], p["reader_xcc"]) == (writer, reader):
            p["errors"] += 1
    return raw


def test_summary_clean():
    s = summarize_xcd_fabric(_raw())
    assert s["healthy"] is True and s["consistent"] is True
    assert s["cross_xcd"] is True
    assert (s["xcc_seen"], s["pairs_covered"], s["pairs_expected"]) == (2, 4, 4)
    assert s["rounds"] == ROUNDS and s["elapsed_ms"] == 1.0
    assert s["episodes_completed"] == s["episodes_expected"] == EPISODES
    assert s["lines_verified"] == s["lines_expected"] == LINES
    assert s["failing_pairs"] == [] and s["failing_atomics"] == []
    assert s["failing_comparisons"] == [] and s["stale_records"] == 0
    assert s["atomics_ok"] is True and s["tickets_ok"] is True
    assert set(s["per_xcc"]) == {0, 1}
    assert s["per_xcc"][0] == {
        "lines_written": LINES // 2, "lines_read": LINES // 2,
        "errors_as_writer": 0, "errors_as_reader": 0, "adder_waves": 8,
    }
    assert "records" not in s and "pairs" not in s and "atomics" not in s


def test_summary_single_xcc_passes_but_is_not_cross_xcd():
    s = summarize_xcd_fabric(_raw(xccs=(3,)))
    assert s["healthy"] is True
    assert s["cross_xcd"] is False
    assert (s["xcc_seen"], s["pairs_covered"]) == (1, 1)
    assert set(s["per_xcc"]) == {3}


def test_summary_payload_error_names_its_pair():
    s = summarize_xcd_fabric(_with_payload_error(_raw(), 0, 1, stale=True))
    assert s["healthy"] is False and s["consistent"] is True
    assert s["failing_pairs"] == [
        {"writer_xcc": 0, "reader_xcc": 1, "lines": LINES // 4, "errors": 1},
    ]
    assert s["failing_comparisons"] == ["payload"]
    assert s["stale_records"] == 1
    assert s["per_xcc"][0]["errors_as_writer"] == 1
    assert s["per_xcc"][1]["errors_as_reader"] == 1
    assert s["per_xcc"][1]["errors_as_writer"] == 0


def test_summary_header_error():
    raw = _raw()
    raw["records"].append(_record("header", reader=1))
    raw["header_errors"] = raw["error_count"] = 1
    s = summarize_xcd_fabric(raw)
    assert s["healthy"] is False and s["consistent"] is True
    assert s["failing_comparisons"] == ["header"]
    assert s["failing_pairs"] == [] and s["stale_records"] == 0


@pytest.mark.parametrize("comparison,op", [
    ("add_u32", "add_u32"), ("add_u64", "add_u64"), ("add_f32", "add_f32"),
    ("minmax", "max_u64"), ("minmax", "min_u64"), ("bitwise", "xor_u32"),
    ("bitwise", "or_u32"), ("bitwise", "and_u32"), ("cas", "cas"),
    ("tickets", "tickets"),
])
def test_summary_each_atomic_defect(comparison, op):
    raw = _raw()
    raw["atomics"]["mismatches"].append(
        {"comparison": comparison, "op": op, "cell": 2, "expected": 3, "got": 2})
    s = summarize_xcd_fabric(raw)
    assert s["healthy"] is False and s["atomics_ok"] is False
    assert s["failing_comparisons"] == [comparison]
    assert s["failing_atomics"] == raw["atomics"]["mismatches"]
    assert s["failing_pairs"] == []


@pytest.mark.parametrize("key,value", [
    ("tickets_missing", 1), ("tickets_out_of_range", 1), ("ticket_counter", 2047),
])
def test_summary_each_ticket_defect(key, value):
    raw = _raw()
    raw["atomics"][key] = value
    s = summarize_xcd_fabric(raw)
    assert s["healthy"] is False
    assert s["tickets_ok"] is False and s["atomics_ok"] is False
    assert s["failing_comparisons"] == ["tickets"]


@pytest.mark.parametrize("key", [
    "ticket_counter_errors", "tickets_out_of_range", "writer_xcc_out_of_range",
])
def test_summary_each_handoff_counter_defect(key):
    raw = _raw()
    raw[key] = 1
    s = summarize_xcd_fabric(raw)
    assert s["healthy"] is False and s[key] == 1


def test_summary_missing_episode_is_unhealthy_with_zero_errors():
    raw = _raw()
    raw["episodes_completed"] -= 1
    raw["lines_verified"] -= GROUP * SLAB
    raw["pairs"][0]["lines"] -= GROUP * SLAB
    s = summarize_xcd_fabric(raw)
    assert s["error_count"] == 0 and s["consistent"] is True
    assert s["episodes_completed"] == s["episodes_expected"] - 1
    assert s["healthy"] is False


def test_summary_short_header_coverage_is_unhealthy():
    raw = _raw()
    raw["header_lines_verified"] -= 1
    assert summarize_xcd_fabric(raw)["healthy"] is False


def test_summary_uncovered_pair_is_unhealthy():
    raw = _raw()
    gone = raw["pairs"].pop()  # (1, 1) never verified; its lines went to (0, 0)
    raw["pairs"][0]["lines"] += gone["lines"]
    raw["pairs_covered"] = 3
    s = summarize_xcd_fabric(raw)
    assert s["consistent"] is True and s["error_count"] == 0
    assert (s["pairs_covered"], s["pairs_expected"]) == (3, 4)
    assert s["healthy"] is False


def test_summary_pair_covered_by_extra_lines_only():
    # a pair that only a neighbour-group look reached still counts as covered,
    # and its lines are no part of lines_verified
    raw = _raw()
    moved = raw["pairs"][3]["lines"]
    raw["pairs"][3]["lines"] = 0
    raw["pairs"][3]["extra_lines"] = 5
    raw["pairs"][0]["lines"] += moved
    raw["extra_lines_verified"] = 5
    s = summarize_xcd_fabric(raw)
    assert s["consistent"] is True and s["healthy"] is True
    assert s["extra_lines_verified"] == 5
    assert s["per_xcc"][1]["lines_read"] == LINES // 4 + 5
    raw["extra_lines_verified"] = 4  # the table shows five
    s = summarize_xcd_fabric(raw)
    assert s["consistent"] is False and s["healthy"] is False


def test_summary_a_single_round_is_unhealthy():
    raw = _raw()
    raw["rounds"] = 1
    assert summarize_xcd_fabric(raw)["healthy"] is False


def test_summary_no_xcc_seen_is_unhealthy():
    raw = _raw()
    raw.update(pairs=[], pairs_covered=0, xcc_seen=0, lines_verified=0,
               lines_expected=0, episodes_completed=0, episodes_expected=0)
    s = summarize_xcd_fabric(raw)
    assert s["healthy"] is False and s["cross_xcd"] is False


def test_summary_missing_atomics_is_unhealthy():
    raw = _raw()
    raw["atomics"] = {}
    assert summarize_xcd_fabric(raw)["healthy"] is False


def test_summary_errors_without_records_is_unhealthy():
    raw = _raw()
    raw["payload_errors"] = raw["error_count"] = 2
    raw["pairs"][1]["errors"] = 2
    s = summarize_xcd_fabric(raw)
    assert s["consistent"] is False and s["healthy"] is False


def test_summary_records_without_errors_is_unhealthy():
    raw = _raw()
    raw["records"].append(_record())
    s = summarize_xcd_fabric(raw)
    assert s["error_count"] == 0
    assert s["consistent"] is False and s["healthy"] is False
    assert s["failing_comparisons"] == ["payload"]


def test_summary_pair_table_that_contradicts_the_counters_is_unhealthy():
    raw = _raw()
    raw["xcc_seen"] = 1
    raw["pairs_covered"] = 1  # the table shows four
    s = summarize_xcd_fabric(raw)
    assert s["consistent"] is False and s["healthy"] is False
    raw = _with_payload_error(_raw())
    raw["pairs"][1]["errors"] = 0  # counter says one, no pair owns it
    s = summarize_xcd_fabric(raw)
    assert s["consistent"] is False and s["healthy"] is False


# ---- health report and CLI against a stub native module --------------------

class _StubNative:
    """Healthy stand-in for the native module; the fabric result is settable."""

    def __init__(self, fabric_raw):
        self.fabric_raw = fabric_raw
        self.fabric_calls = []

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

    def xcd_fabric_check(self, device, **kw):
        self.fabric_calls.append((device, kw))
        return self.fabric_raw


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


def test_health_report_without_fabric_is_unchanged(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True)
    assert set(report) == {"healthy", "checks"}
    assert set(report["checks"]) == TODAYS_CHECK_KEYS
    assert "xcd_fabric" not in report["checks"]
    assert report["healthy"] is True
    assert gpu_health_check(require_gpu=True, fabric=False) == report
    assert stub.fabric_calls == []


def test_health_report_fabric_adds_key_and_gates(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, fabric=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS | {"xcd_fabric"}
    fab = report["checks"]["xcd_fabric"]
    assert fab["healthy"] is True and fab["cross_xcd"] is True
    assert "records" not in fab and "atomics" not in fab
    assert report["healthy"] is True
    assert stub.fabric_calls == [(0, {})]

    stub.fabric_raw = _with_payload_error(_raw(), 1, 0)
    report = gpu_health_check(require_gpu=True, fabric=True)
    assert report["healthy"] is False
    fab = report["checks"]["xcd_fabric"]
    assert [(p["writer_xcc"], p["reader_xcc"]) for p in fab["failing_pairs"]] == [(1, 0)]
    # everything else is still fine: only the fabric check gates it
    assert gpu_health_check(require_gpu=True)["healthy"] is True

    stub.fabric_raw = _raw()
    stub.fabric_raw["episodes_completed"] -= 1
    assert gpu_health_check(require_gpu=True, fabric=True)["healthy"] is False


@pytest.mark.parametrize("argv,calls", [
    (["gpu_health"], []),
    (["gpu_health", "--fabric"], [(0, {})]),
    (["gpu_health", "--deep-not", "--fabric"], [(0, {})]),
], ids=["plain", "fabric", "fabric-among-others"])
def test_main_maps_fabric_flag(monkeypatch, capsys, argv, calls):
    import json
    import sys

    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    monkeypatch.setattr(sys, "argv", argv)
    assert gpu_health.main() == 0
    assert stub.fabric_calls == calls
    printed = json.loads(capsys.readouterr().out)
    assert ("xcd_fabric" in printed["checks"]) == bool(calls)

    stub.fabric_raw = _with_payload_error(_raw())
    if calls:
        assert gpu_health.main() == 1


def test_python_wrapper_passes_keywords_and_keeps_raw_lists(monkeypatch):
    stub = _StubNative(_with_payload_error(_raw()))
    monkeypatch.setattr(xcd_fabric, "load_native_validator", lambda: stub)
    out = xcd_fabric.xcd_fabric_check(0, reps=2, poison_mask=1)
    assert stub.fabric_calls == [(0, {"reps": 2, "poison_mask": 1})]
    assert out["healthy"] is False
    assert out["records"] == stub.fabric_raw["records"]
    assert out["pairs"] == stub.fabric_raw["pairs"]
    assert out["atomics"]["threads"] == 2048
    monkeypatch.setattr(xcd_fabric, "load_native_validator", lambda: None)
    with pytest.raises(gpu_health.GpuHealthError):
        xcd_fabric.xcd_fabric_check(0)
