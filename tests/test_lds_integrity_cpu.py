"""CPU-side tests for the LDS data-integrity check.

``summarize_lds_integrity`` is driven with hand-built raw tables of a small
synthetic device, the health-report and CLI wiring is checked against a stub
native module, the host-only reference is compared with numpy written here
from the documented rules (the native generators never produce an
expectation), and the argument validation is exercised without a device."""

import copy

import numpy as np
import pytest

from k8s_operator_libs_amd.validation import (
    gpu_health,
    gpu_health_check,
    lds_integrity,
    load_native_validator,
    summarize_lds_integrity,
)

MASK = (1 << 64) - 1
U = np.uint64
PHASES = ("pattern", "subword", "transpose", "dma", "atomics", "permute")
WORDS = 40960
XCCS, CUS_PER_XCC = 2, 3

KEY_PATTERN = 0x4C44535F50415454
KEY_SUBWORD = 0x4C44535F53554257
KEY_TRANSPOSE = 0x4C44535F54523136
KEY_DMA = 0x4C44535F444D4153
KEY_ATOM1 = 0x4C44535F41544D31
KEY_ATOM2 = 0x4C44535F41544D32
KEY_PERM_VAL = 0x4C44535F5045524D
KEY_PERM_MAP = 0x4C44535F50455250


# ---- summarize_lds_integrity on hand-built raw tables ----------------------

def _key(xcc, se, sh, cu):
    return (xcc << 8) | (se << 5) | (sh << 4) | cu


def _items(passes):
    return {"pattern": (passes + 1) * 2 * WORDS, "subword": 4 * WORDS,
            "transpose": 4 * WORDS, "dma": WORDS, "atomics": 640,
            "permute": 4096}


def _raw(skip_keys=(), fail=None, compute_units=XCCS * CUS_PER_XCC, reps=2,
         passes=3):
    fail = fail or {}
    units = []
    for xcc in range(XCCS):
        for cu in range(CUS_PER_XCC):
            key = _key(xcc, se=cu % 2, sh=0, cu=cu)
            if key in skip_keys:
                continue
            units.append({"key": key, "xcc": xcc, "hw_bits": key & 0xFF,
                          "workgroups": 2, "fail_mask": fail.get(key, 0),
                          "hw_id_raw": (key & 0xFF) << 8, "xcc_id_raw": xcc})
    blocks = 2 * compute_units
    expected = {p: blocks * reps * n for p, n in _items(passes).items()}
    return {
        "compute_units": compute_units, "cus_covered": len(units), "rounds": 1,
        "blocks": blocks, "lds_bytes": 163840, "units": units,
        "phase_words_verified": dict(expected),
        "phase_words_expected": dict(expected),
        "error_count": 0, "xor_or": 0, "records": [], "records_dropped": 0,
        "elapsed_ms": 1.5,
    }


def _record(key, word, expected, got, phase="pattern", block=0, rep=0):
    return {"key": key, "block": block, "rep": rep, "phase": phase, "detail": 0,
            "word": word, "expected": expected, "got": got}


def _with_records(raw, records, dropped=0):
    raw = copy.deepcopy(raw)
    raw["records"] = records
    raw["error_count"] = len(records) + dropped
    raw["records_dropped"] = dropped
    masks = {}
    for r in records:
        masks[r["key"]] = masks.get(r["key"], 0) | (1 << PHASES.index(r["phase"]))
        raw["xor_or"] |= r["expected"] ^ r["got"]
    for u in raw["units"]:
        u["fail_mask"] |= masks.get(u["key"], 0)
    return raw


def test_summary_clean_is_healthy():
    s = summarize_lds_integrity(_raw())
    assert s["healthy"] is True and s["consistent"] is True
    assert s["cus_covered"] == s["compute_units"] == 6
    assert s["uncovered_cus"] == 0
    assert s["per_xcc"] == {0: 3, 1: 3}
    assert s["failing_units"] == [] and s["failing_words"] == []
    assert s["suspect_banks"] == [] and s["errors_per_bank"] == {}
    assert s["short_phases"] == []
    assert s["lds_bytes"] == 163840
    assert "units" not in s and "records" not in s


def test_summary_one_cu_missing_is_unhealthy():
    s = summarize_lds_integrity(_raw(skip_keys={_key(0, 1, 0, 1)}))
    assert s["healthy"] is False
    assert s["uncovered_cus"] == 1 and s["cus_covered"] == 5
    assert s["per_xcc"] == {0: 2, 1: 3}


@pytest.mark.parametrize("phase", PHASES)
def test_summary_short_count_is_unhealthy_with_zero_errors(phase):
    raw = _raw()
    raw["phase_words_verified"][phase] -= 1
    s = summarize_lds_integrity(raw)
    assert s["error_count"] == 0
    assert s["short_phases"] == [phase]
    assert s["healthy"] is False


def test_summary_fail_mask_bits_become_phase_names():
    key_a, key_b = _key(0, 0, 0, 0), _key(1, 1, 0, 1)
    raw = _raw(fail={key_a: 0b000101, key_b: 0b111010})
    raw["error_count"] = 7
    raw["records_dropped"] = 7
    s = summarize_lds_integrity(raw)
    assert s["healthy"] is False
    assert [(u["key"], u["failed"]) for u in s["failing_units"]] == [
        (key_a, ["pattern", "transpose"]),
        (key_b, ["subword", "dma", "atomics", "permute"]),
    ]
    unit = s["failing_units"][1]
    assert (unit["xcc"], unit["se"], unit["sh"], unit["cu"]) == (1, 1, 0, 1)


def test_summary_records_in_one_bank_name_that_bank():
    key = _key(1, 0, 0, 2)
    words = [17, 17 + 64, 17 + 64 * 300, 17 + 64 * 639]
    recs = [_record(key, w, 0xFFFF0000, 0xFFFF0000 ^ (1 << (w % 7)),
                    phase="pattern" if i % 2 else "subword")
            for i, w in enumerate(words)]
    s = summarize_lds_integrity(_with_records(_raw(), recs))
    assert s["healthy"] is False
    assert s["suspect_banks"] == [17]
    assert s["errors_per_bank"] == {17: 4}
    assert [w["word"] for w in s["failing_words"]] == sorted(words)
    assert all(w["bank"] == 17 for w in s["failing_words"])
    assert [w["byte_offset"] for w in s["failing_words"]] == [4 * w for w in sorted(words)]
    assert [u["key"] for u in s["failing_units"]] == [key]


def test_summary_one_bit_across_banks_names_no_bank():
    key = _key(0, 0, 0, 2)
    words = [3, 200, 4097, 40959]
    recs = [_record(key, w, 0x12345678, 0x12345678 ^ (1 << 21)) for w in words]
    s = summarize_lds_integrity(_with_records(_raw(), recs))
    assert s["suspect_banks"] == []
    assert s["flipped_bits"] == [21]
    assert all(w["flipped_bits"] == [21] for w in s["failing_words"])
    assert s["errors_per_bank"] == {w % 64: 1 for w in words}
    assert s["xor_or"] == 1 << 21


def test_summary_bank_of_a_non_memory_phase_is_not_suspect():
    key = _key(0, 0, 0, 0)
    recs = [_record(key, 5, 1, 0, phase="permute")]
    s = summarize_lds_integrity(_with_records(_raw(), recs))
    assert s["suspect_banks"] == []
    assert s["errors_per_bank"] == {5: 1}


def test_summary_records_dropped_handling():
    key = _key(0, 0, 0, 0)
    recs = [_record(key, w, 2, 3) for w in range(64)]
    ok = summarize_lds_integrity(_with_records(_raw(), recs, dropped=1000))
    assert ok["consistent"] is True and ok["healthy"] is False
    assert ok["records_dropped"] == 1000 and ok["error_count"] == 1064
    # dropped records that the error counter does not account for
    bad = _with_records(_raw(), recs, dropped=1000)
    bad["records_dropped"] = 999
    assert summarize_lds_integrity(bad)["consistent"] is False
    # errors with neither records nor drops, and records without errors
    raw = _raw()
    raw["error_count"] = 3
    s = summarize_lds_integrity(raw)
    assert s["consistent"] is False and s["healthy"] is False
    raw = _with_records(_raw(), recs[:1])
    raw["error_count"] = 0
    raw["records_dropped"] = -1
    s = summarize_lds_integrity(raw)
    assert s["consistent"] is False and s["healthy"] is False


def test_summary_smaller_lds_is_unhealthy():
    raw = _raw()
    raw["lds_bytes"] = 65536
    assert summarize_lds_integrity(raw)["healthy"] is False


# ---- health report and CLI against a stub native module --------------------

class _StubNative:
    def __init__(self, lds_raw):
        self.lds_raw = lds_raw
        self.lds_calls = []

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

    def lds_integrity_check(self, device, **kw):
        self.lds_calls.append((device, kw))
        return self.lds_raw


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
    assert gpu_health_check(require_gpu=True, lds=False) == report
    assert stub.lds_calls == []


def test_health_report_lds_adds_key_and_gates_both_ways(monkeypatch):
    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    report = gpu_health_check(require_gpu=True, lds=True)
    assert set(report["checks"]) == TODAYS_CHECK_KEYS | {"lds_integrity"}
    summary = report["checks"]["lds_integrity"]
    assert summary["healthy"] is True
    assert "units" not in summary and "records" not in summary
    assert report["healthy"] is True
    assert stub.lds_calls == [(0, {})]

    key = _key(1, 0, 0, 0)
    stub.lds_raw = _with_records(_raw(), [_record(key, 40959, 5, 4)])
    report = gpu_health_check(require_gpu=True, lds=True)
    assert report["healthy"] is False
    assert report["checks"]["lds_integrity"]["failing_units"][0]["key"] == key
    # everything else is still fine: only the LDS check gates it
    assert gpu_health_check(require_gpu=True)["healthy"] is True

    stub.lds_raw = _raw()
    stub.lds_raw["phase_words_verified"]["dma"] -= 1
    assert gpu_health_check(require_gpu=True, lds=True)["healthy"] is False


@pytest.mark.parametrize("argv,calls", [
    (["gpu_health"], []),
    (["gpu_health", "--lds"], [(0, {})]),
    (["gpu_health", "--coverage-not", "--lds"], [(0, {})]),
], ids=["plain", "lds", "lds-among-others"])
def test_main_maps_lds_flag(monkeypatch, capsys, argv, calls):
    import json
    import sys

    stub = _StubNative(_raw())
    _install_stub(monkeypatch, stub)
    monkeypatch.setattr(sys, "argv", argv)
    assert gpu_health.main() == 0
    assert stub.lds_calls == calls
    printed = json.loads(capsys.readouterr().out)
    assert ("lds_integrity" in printed["checks"]) == bool(calls)

    stub.lds_raw = _with_records(_raw(), [_record(_key(0, 0, 0, 0), 1, 1, 0)])
    if calls:
        assert gpu_health.main() == 1


def test_python_wrapper_passes_keywords_and_keeps_raw_lists(monkeypatch):
    stub = _StubNative(_with_records(_raw(), [_record(_key(0, 0, 0, 0), 1, 1, 0)]))
    monkeypatch.setattr(lds_integrity, "load_native_validator", lambda: stub)
    out = lds_integrity.lds_integrity_check(0, reps=1, poison_mask=1)
    assert stub.lds_calls == [(0, {"reps": 1, "poison_mask": 1})]
    assert out["healthy"] is False
    assert out["records"] == stub.lds_raw["records"]
    assert out["units"] == stub.lds_raw["units"]
    monkeypatch.setattr(lds_integrity, "load_native_validator", lambda: None)
    with pytest.raises(gpu_health.GpuHealthError):
        lds_integrity.lds_integrity_check(0)


# ---- the host-only reference against numpy ---------------------------------

@pytest.fixture(scope="module")
def native():
    mod = load_native_validator()
    if mod is None:
        pytest.skip("native validator not built and not buildable here")
    return mod


def np_hash(seed, i):
    """splitmix64 finaliser of (i + seed * golden ratio), mod 2^64."""
    i = np.asarray(i, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = i + U((seed * 0x9E3779B97F4A7C15) & MASK)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def np_value(seed, key, block, rep, sub, word):
    """64-bit value of (block, rep, sub, word) under a phase key: the index
    packs block | rep (12 bits) | sub (5 bits) | word (16 bits)."""
    word = np.asarray(word, dtype=np.uint64)
    idx = U((((block << 12) | rep) << 5 | sub) << 16) | word
    return np_hash(seed ^ key, idx)


def np_words(seed, key, block, rep, sub=0, n=WORDS):
    return (np_value(seed, key, block, rep, sub, np.arange(n)) & U(0xFFFFFFFF)
            ).astype(np.uint32)


CASES = [(1, 0, 0, 3), (0xDEADBEEFCAFEF00D, 511, 1, 1), (MASK, 7, 4095, 16),
         (5, 65535, 2, 2)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"b{c[1]}r{c[2]}p{c[3]}")
def ref(request, native):
    seed, block, rep, passes = request.param
    return request.param, native.lds_integrity_reference(
        seed=seed, block=block, rep=rep, passes=passes)


def test_reference_pattern_images(ref):
    (seed, block, rep, passes), r = ref
    assert r["lds_words"] == WORDS
    assert tuple(r["phases"]) == PHASES
    assert len(r["pattern_images"]) == passes + 1
    for pat in range(passes):
        want = np_words(seed, KEY_PATTERN, block, rep, sub=pat)
        assert np.array_equal(np.array(r["pattern_images"][pat], np.uint32), want)
    checker = np.where(np.arange(WORDS) % 2 == 0, 0xAAAAAAAA, 0x55555555)
    assert np.array_equal(np.array(r["pattern_images"][passes]), checker)
    # three different widths per pattern, rotated by one per pattern
    names = ["b32", "b64", "b128"]
    for pat, widths in enumerate(r["pattern_widths"]):
        assert list(widths) == [names[(pat + k) % 3] for k in range(3)]
    if passes >= 3:
        for role in range(3):
            assert {w[role] for w in r["pattern_widths"][:3]} == set(names)


def test_reference_subword_image(ref):
    (seed, block, rep, _), r = ref
    want = np_words(seed, KEY_SUBWORD, block, rep)
    assert np.array_equal(np.array(r["subword_image"], np.uint32), want)


def test_reference_dma_image_from_the_destination_rule(ref):
    """Destination = wave-uniform base + lane x size, source permuted: replay
    every wave-instruction of the fill into an empty image."""
    (seed, block, rep, _), r = ref
    src = np_words(seed, KEY_DMA, 0, 0)
    assert np.array_equal(np.array(r["dma_source"], np.uint32), src)
    image = np.full(WORDS, -1, dtype=np.int64)
    lanes = np.arange(64)
    for chunk in range(160):
        src_chunk = (chunk + 1 + block * 7 + rep * 13) % 160
        base = chunk * 256
        if (chunk + rep) % 2 == 0:
            # one 16-byte load: lane l brings source piece (5 l + 3 + block +
            # rep) % 64 of the source chunk to words 4l .. 4l+3
            piece = (lanes * 5 + 3 + block + rep) % 64
            for k in range(4):
                image[base + 4 * lanes + k] = src[src_chunk * 256 + 4 * piece + k]
        else:
            # four 4-byte loads: load j, lane l lands at word 64 j + l
            for j in range(4):
                dst = 64 * j + lanes
                image[base + dst] = src[src_chunk * 256
                                        + (dst * 37 + 11 + block + rep) % 256]
    assert (image >= 0).all()
    assert np.array_equal(np.array(r["dma_image"], np.int64), image)
    # the source really is permuted
    assert not np.array_equal(image, src.astype(np.int64))


def tr_decode(image_u16, lane_byte_offsets):
    """The documented map of ds_read_b64_tr_b16, written from the prose: in a
    group of 16 lanes, lane 4q+p supplies the address of row q, columns 4p ..
    4p+3; lane i receives column i of the four rows, row q in element q."""
    out = np.zeros((64, 4), dtype=np.int64)
    for group in range(4):
        rows = np.zeros((4, 16), dtype=np.int64)
        for q in range(4):
            for p in range(4):
                first = lane_byte_offsets[16 * group + 4 * q + p] // 2
                rows[q, 4 * p:4 * p + 4] = image_u16[first:first + 4]
        for i in range(16):
            out[16 * group + i] = rows[:, i]
    return out


def test_reference_transposed_block(ref):
    (seed, block, rep, _), r = ref
    words = np_words(seed, KEY_TRANSPOSE, block, rep)
    assert np.array_equal(np.array(r["transpose_image"], np.uint32), words)
    # element e is half e & 1 of word e // 2
    elems = np.stack([words & 0xFFFF, words >> 16], axis=1).reshape(-1)
    t = r["transpose"]
    assert t["row_stride_bytes"] == 160 and t["first_block"] == 1276
    offs = list(t["lane_byte_offsets"])
    # 160-byte rows, five blocks a row, four rows a tile; blocks 1276..1279
    for lane, off in enumerate(offs):
        b, i = 1276 + lane // 16, lane % 16
        assert off == (b // 5) * 640 + (i // 4) * 160 + (b % 5) * 32 + 8 * (i % 4)
        assert off % 8 == 0 and off + 8 <= 163840
    assert max(offs) + 8 == 163840
    assert np.array_equal(np.array(t["lanes"], np.int64), tr_decode(elems, offs))


def test_reference_atomic_totals_and_f32_bound(ref):
    (seed, block, rep, _), r = ref
    a = r["atomics"]
    cells, steps = a["cells"], a["steps"]
    assert (cells, steps) == (64, 4)
    tid = np.repeat(np.arange(256, dtype=np.uint64), steps)
    step = np.tile(np.arange(steps, dtype=np.uint64), 256)
    cell = ((tid + step) % U(cells)).astype(np.int64)
    h1 = np.array([int(np_value(seed, KEY_ATOM1, block, rep, int(s), int(t)))
                   for t, s in zip(tid, step)], dtype=np.uint64)
    h2 = np.array([int(np_value(seed, KEY_ATOM2, block, rep, int(s), int(t)))
                   for t, s in zip(tid, step)], dtype=np.uint64)
    one = np.uint32(1)
    add32 = (h1 & U(0xFFFFFFFF)).astype(np.uint32)
    addf = ((h1 >> U(32)) % U(17)).astype(np.int64) - 8
    mm = ((h1 >> U(13)) & U(0xFFFFFFFF)).astype(np.uint32)
    xor = ((h2 >> U(20)) & U(0xFFFFFFFF)).astype(np.uint32)
    or_ = (one << ((h2 >> U(8)) & U(31)).astype(np.uint32)).astype(np.uint32)
    and_ = (~(one << ((h2 >> U(16)) & U(31)).astype(np.uint32))).astype(np.uint32)
    out = {
        "add_u32": np.zeros(cells, np.uint32), "add_u64": np.zeros(cells, np.uint64),
        "add_f32": np.zeros(cells, np.int64), "max_u32": np.zeros(cells, np.uint32),
        "min_u32": np.full(cells, 0xFFFFFFFF, np.uint32),
        "xor_u32": np.zeros(cells, np.uint32), "or_u32": np.zeros(cells, np.uint32),
        "and_u32": np.full(cells, 0xFFFFFFFF, np.uint32),
    }
    with np.errstate(over="ignore"):
        np.add.at(out["add_u32"], cell, add32)
        np.add.at(out["add_u64"], cell, h2)
    np.add.at(out["add_f32"], cell, addf)
    np.maximum.at(out["max_u32"], cell, mm)
    np.minimum.at(out["min_u32"], cell, mm)
    np.bitwise_xor.at(out["xor_u32"], cell, xor)
    np.bitwise_or.at(out["or_u32"], cell, or_)
    np.bitwise_and.at(out["and_u32"], cell, and_)
    for op, want in out.items():
        assert [int(v) for v in a[op]] == [int(v) for v in want], op
    magnitude = np.zeros(cells, np.int64)
    np.add.at(magnitude, cell, np.abs(addf))
    assert [int(v) for v in a["add_f32_abs_sum"]] == [int(v) for v in magnitude]
    # every order of addition is exact in f32
    assert a["f32_bound"] == 1 << 23
    assert int(magnitude.max()) <= a["f32_bound"]
    assert -8 <= int(addf.min()) and int(addf.max()) <= 8


def test_reference_permute_expectations(ref):
    (seed, block, rep, _), r = ref
    assert len(r["permute"]) == 8
    lanes = np.arange(64)
    for step, e in enumerate(r["permute"]):
        values = np_words(seed, KEY_PERM_VAL, block, rep, sub=step, n=256)
        assert np.array_equal(np.array(e["values"], np.uint32), values)
        pulled = np.zeros(256, np.uint32)
        pushed = np.zeros(256, np.uint32)
        for wave in range(4):
            h = int(np_value(seed, KEY_PERM_MAP, block, rep, step, wave))
            mul, add = (h & 63) | 1, (h >> 8) & 63
            sigma = (mul * lanes + add) % 64
            assert sorted(sigma) == list(range(64))
            assert list(e["sigma"][64 * wave:64 * wave + 64]) == list(sigma)
            v = values[64 * wave:64 * wave + 64]
            # ds_bpermute: lane l reads lane sigma(l); ds_permute: lane l
            # writes to lane sigma(l)
            pulled[64 * wave:64 * wave + 64] = v[sigma]
            pushed[64 * wave + sigma] = v
        assert np.array_equal(np.array(e["bpermute"], np.uint32), pulled)
        assert np.array_equal(np.array(e["permute"], np.uint32), pushed)
    assert r["permute"][0]["sigma"] != r["permute"][1]["sigma"]


# ---- argument validation, before any HIP call ------------------------------

@pytest.mark.parametrize("kw", [
    {"reps": 0}, {"reps": 4097}, {"passes": 0}, {"passes": 17},
    {"max_rounds": 0}, {"max_rounds": 65}, {"blocks": -1},
    {"poison_mask": 1 << 6}, {"poison_key": 4096}, {"poison_word": 40960},
    {"poison_word": -2}, {"poison_xor": 0}, {"poison_xor": 1 << 32},
])
def test_bad_arguments_raise_value_error_without_a_gpu(native, kw):
    with pytest.raises(ValueError):
        native.lds_integrity_check(0, **kw)


def test_reference_validates_its_arguments(native):
    for kw in ({"passes": 17}, {"rep": 4096}, {"block": -1}, {"block": 65536}):
        with pytest.raises(ValueError):
            native.lds_integrity_reference(**kw)


@pytest.mark.parametrize("image,offsets", [
    (list(range(256)), [8 * i + 4 for i in range(64)]),   # misaligned
    (list(range(256)), [8 * i for i in range(63)]),       # 63 lanes
    (list(range(256)), [8 * i for i in range(63)] + [512]),    # past the end
    (list(range(256)), [-8] + [8 * i for i in range(63)]),
    ([1, 2], [0] * 64),                                   # image too small
    ([0] * 81921, [0] * 64),                              # image above 160 KiB
], ids=["misaligned", "lanes", "bounds", "negative", "small", "large"])
def test_tr_tile_validates_on_the_host(native, image, offsets):
    with pytest.raises(ValueError):
        native.lds_tr_tile(0, image, offsets)
