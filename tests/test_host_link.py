"""Host-link data-integrity check on a real MI355X.

A clean run must compare every word of every phase of every memory kind and
find nothing; the data-only poison hook then proves that each phase is live,
that a failing word or copy case is named exactly, and that a record's ``got``
is what really crossed the link (it equals the host reference of the pattern).

Shape A is 1 MiB + 8 bytes, 131073 words: only the scalar tail reaches the
last word, the byte-store and 16-bit-store chunks of the zero-copy write are
present, and with ``blocks=8`` (2048 threads over 65536 vectors) the
zero-copy kernels run their unrolled body, the remainder loop and the tail.

Which pattern a phase compares follows the check's phase table: ``d2h`` brings
back the inverse that the ``h2d`` kernel wrote (seed slot 0), ``zc_write``
stores the inverse of what ``zc_read`` compared (seed slot 2).  Nothing here
depends on timing: rates are printed, never asserted."""

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
A_BYTES = MIB + 8
A_WORDS = 131073
LO = A_WORDS // 2
SEED = 0x5EED
BIT = 1 << 37
KINDS = ["pinned", "registered", "pageable"]
PHASES = ["h2d", "d2h", "zc_read", "zc_write", "duplex", "unaligned", "atomics"]
KIND_PHASES = {"pinned": PHASES[:6], "registered": PHASES[:6],
               "pageable": ["h2d", "d2h", "unaligned"]}
# phase -> (seed slot of the pattern compared, compared with its inverse)
DATA = {0: (0, False), 1: (0, True), 2: (2, False), 3: (2, True), 4: (4, False)}
ATOM_BLOCKS = 4
THREADS = ATOM_BLOCKS * 64
REPS = 2
HOST_ADDS = 4096


@pytest.fixture(scope="module")
def native():
    import os

    from k8s_operator_libs_amd.validation import GpuHealthError, load_native_validator

    mod = load_native_validator()
    if mod is None:
        if not os.path.exists("/dev/kfd"):
            # CPU-only machine running an unfiltered `pytest tests/`: skip.
            # On a real GPU box (ROCm kfd present) a missing native
            # extension stays a HARD failure.
            pytest.skip("no GPU on this machine (missing /dev/kfd)")
        raise GpuHealthError(
            "native validator must be present on a GPU box - refusing to skip"
        )
    return mod


def run_a(native, **kw):
    from k8s_operator_libs_amd.validation import summarize_host_link

    kw.setdefault("kinds", KINDS)
    raw = native.host_link_check(0, A_BYTES, seed=SEED, blocks=8,
                                 atomics_blocks=ATOM_BLOCKS, reps=REPS,
                                 host_adds=HOST_ADDS, **kw)
    return raw, summarize_host_link(raw)


@pytest.fixture(scope="module")
def plan(native):
    return native.host_link_plan()


@pytest.fixture(scope="module")
def clean(native):
    """One clean run of shape A over all three kinds, shared and not changed."""
    return run_a(native)


def expected_counts(plan, kind, atomics):
    want = {
        "h2d": A_WORDS, "d2h": A_WORDS, "zc_read": A_WORDS, "zc_write": A_WORDS,
        "duplex": A_WORDS // 2 + (A_WORDS - A_WORDS // 2),
        "unaligned": 464 * plan["slot_bytes"],
    }
    out = {p: want[p] for p in KIND_PHASES[kind]}
    if kind == "pinned" and atomics:
        # 2 x 64 add cells, counter, out-of-range count, `threads` seen slots,
        # threads + 64 swap values, 2 x 8 claim pairs, 2 winner counts
        out["atomics"] = 128 + 2 + THREADS + (THREADS + 64) + 16 + 2
    return out


def compared_counts(raw):
    return {k: {p: v["compared"] for p, v in t["phases"].items()}
            for k, t in raw["kinds"].items()}


def word_reference(native, kind, phase, word):
    slot, inverted = DATA[phase]
    return native.hbm_pattern_reference(
        "hash", SEED + 16 * KINDS.index(kind) + slot, word, 1, inverted)[0]


def test_clean_run_compares_everything_in_all_three_kinds(native, plan, clean):
    raw, summary = clean
    for kind, table in raw["kinds"].items():
        for phase, v in table["phases"].items():
            print(f"{kind:10s} {phase:9s} {v['gbps']:8.3f} GB/s "
                  f"link {v['link_ms']:8.3f} ms  phase {v['elapsed_ms']:8.3f} ms")
        print(kind, "duplex_overlap", table.get("duplex_overlap"))
    print("total ms", raw["elapsed_ms"], "atomics", raw["atomics_supported"])

    assert raw["error_count"] == 0 and raw["records"] == []
    assert raw["records_dropped"] == 0 and raw["fail_mask"] == 0
    assert raw["xor_or"] == 0
    assert raw["words"] == A_WORDS and raw["plan_cases"] == 464
    assert list(raw["kinds"]) == KINDS
    for kind in KINDS:
        want = expected_counts(plan, kind, raw["atomics_supported"])
        phases = raw["kinds"][kind]["phases"]
        assert list(phases) == list(want)
        for phase, n in want.items():
            assert phases[phase]["expected"] == n, (kind, phase)
            assert phases[phase]["compared"] == n, (kind, phase)
            assert phases[phase]["errors"] == 0, (kind, phase)
    assert list(raw["kinds"]["pageable"]["phases"]) == ["h2d", "d2h", "unaligned"]
    assert summary["healthy"] is True and summary["consistent"] is True
    assert summary["failing_phases"] == {k: [] for k in KINDS}


@pytest.mark.parametrize("kind,bit,word,side", [
    ("pinned", 0, 77, "device"),
    ("pinned", 1, 131072, "host"),
    ("pinned", 2, 77, "device"),
    ("pinned", 3, 77, "host"),
    ("pinned", 4, LO - 1, "device"),
    ("pinned", 4, LO, "host"),
    ("registered", 0, 131072, "device"),
    ("pageable", 1, 0, "host"),
], ids=lambda v: str(v))
def test_each_word_phase_is_live(native, clean, kind, bit, word, side):
    raw, summary = run_a(native, poison_mask=1 << bit,
                         poison_kind=KINDS.index(kind), poison_word=word,
                         poison_xor=BIT)
    assert raw["error_count"] == 1 and raw["records_dropped"] == 0
    assert raw["fail_mask"] == 1 << bit and raw["xor_or"] == BIT
    for k in KINDS:
        assert raw["kinds"][k]["fail_mask"] == ((1 << bit) if k == kind else 0)
        for phase, v in raw["kinds"][k]["phases"].items():
            assert v["errors"] == (1 if (k, phase) == (kind, PHASES[bit]) else 0)
    assert len(raw["records"]) == 1
    r = raw["records"][0]
    assert (r["kind"], r["phase"], r["side"]) == (kind, PHASES[bit], side)
    assert r["word"] == word and r["byte_offset"] == 8 * word
    assert r["got"] == word_reference(native, kind, bit, word), r
    assert r["expected"] ^ r["got"] == BIT
    assert r["flipped_bits"] == [37]
    # the hook changes comparisons only: coverage is what the clean run had
    assert compared_counts(raw) == compared_counts(clean[0])
    assert summary["healthy"] is False
    assert summary["failing_phases"][kind] == [PHASES[bit]]
    assert summary["failing_words"][0]["word"] == word


@pytest.mark.parametrize("bit", [2, 3], ids=["zc_read", "zc_write"])
@pytest.mark.parametrize("word", [0, 128, 384, 131071, 131072],
                         ids=["first", "byte-chunk", "short-chunk", "last-vector",
                              "scalar-tail"])
def test_zero_copy_positions(native, word, bit):
    """What the kernel read or wrote at a 16-byte, a byte-assembled, a
    16-bit-assembled, the last vector and the scalar-tail word is the host
    reference's word."""
    raw, _ = run_a(native, kinds=["pinned"], poison_mask=1 << bit,
                   poison_word=word, poison_xor=BIT)
    assert raw["error_count"] == 1 and len(raw["records"]) == 1
    r = raw["records"][0]
    assert (r["phase"], r["word"]) == (PHASES[bit], word)
    assert r["side"] == ("device" if bit == 2 else "host")
    assert r["got"] == word_reference(native, "pinned", bit, word), r
    assert r["expected"] ^ r["got"] == BIT
    phases = raw["kinds"]["pinned"]["phases"]
    assert phases[PHASES[bit]]["compared"] == A_WORDS
    assert [p for p, v in phases.items() if v["errors"]] == [PHASES[bit]]


@pytest.mark.parametrize("kind,direction,length,offs", [
    ("pinned", "h2d", 65537, (129, 7)),
    ("pinned", "d2h", 4097, (63, 65)),
    ("registered", "h2d", 1, (1, 2)),
    ("pageable", "d2h", 33, (3, 3)),
], ids=lambda v: str(v))
def test_unaligned_case_is_named(native, plan, clean, kind, direction, length, offs):
    case = next(c for c in plan["cases"]
                if (c["direction"], c["len"], c["src_off"], c["dst_off"])
                == (direction, length, *offs))
    raw, summary = run_a(native, poison_mask=1 << 5, poison_kind=KINDS.index(kind),
                         poison_case=case["case"], poison_xor=0x21)
    assert raw["plan_cases"] == 464
    assert raw["error_count"] == 1 and raw["fail_mask"] == 1 << 5
    assert len(raw["records"]) == 1
    r = raw["records"][0]
    assert (r["kind"], r["phase"], r["side"]) == (kind, "unaligned", "host")
    assert r["case"] == case["case"] and r["direction"] == direction
    assert (r["src_off"], r["dst_off"], r["len"]) == (*offs, length)
    assert r["byte_offset"] == case["dst_pos"]
    # got is the source slot's byte at src_pos: byte j of the slot of case c is
    # byte j % 8 of hash word c * slot_words + j // 8 of seed slot 5
    j = case["src_pos"]
    w = native.hbm_pattern_reference(
        "hash", SEED + 16 * KINDS.index(kind) + 5,
        case["case"] * (plan["slot_bytes"] // 8) + j // 8, 1, False)[0]
    assert r["got"] == (w >> (8 * (j % 8))) & 0xFF, r
    assert r["expected"] ^ r["got"] == 0x21
    assert compared_counts(raw) == compared_counts(clean[0])
    assert summary["healthy"] is False
    assert summary["failing_phases"][kind] == ["unaligned"]
    assert summary["failing_cases"][0]["case"] == case["case"]
    assert summary["failing_cases"][0]["len"] == length


def _atomics_or_skip(raw):
    if not raw["atomics_supported"]:
        pytest.skip("atomics_supported is false: the device reports no native "
                    "host atomics, the phase was skipped")
    return raw["atomics"]


def test_atomics_are_exact(native, clean):
    raw, summary = clean
    a = _atomics_or_skip(raw)
    ref = native.host_link_reference(SEED, THREADS, REPS, HOST_ADDS)
    assert a["threads"] == THREADS and a["reps"] == REPS
    assert list(a["add32"]) == list(ref["add32"])
    assert list(a["add64"]) == list(ref["add64"])
    assert a["ticket_counter"] == THREADS
    assert a["tickets_out_of_range"] == 0 and a["seen_holes"] == 0
    assert a["swap_mismatches"] == 0
    assert a["winners32"] == 8 and a["winners64"] == 8
    for width in ("32", "64"):
        claims, confirms = a["claim" + width], a["confirm" + width]
        assert list(claims) == list(confirms)
        assert all(1 <= c <= THREADS for c in claims)
        # the winner of cell k is some thread id with id % 8 == k
        assert [(c - 1) % 8 for c in claims] == list(range(8))
    ph = raw["kinds"]["pinned"]["phases"]["atomics"]
    assert ph["compared"] == ph["expected"] == ref["items"] and ph["errors"] == 0
    assert summary["failing_atomics"] == []


def test_atomics_phase_is_live(native, clean):
    _atomics_or_skip(clean[0])
    raw, summary = run_a(native, kinds=["pinned"], poison_mask=1 << 6,
                         poison_xor=0x40)
    ref = native.host_link_reference(SEED, THREADS, REPS, HOST_ADDS)
    assert raw["error_count"] == 1 and raw["fail_mask"] == 1 << 6
    assert len(raw["records"]) == 1
    r = raw["records"][0]
    assert (r["kind"], r["phase"]) == ("pinned", "atomics")
    assert (r["comparison"], r["op"], r["cell"]) == ("add_u32", "add_u32", 0)
    assert r["got"] == ref["add32"][0]
    assert r["expected"] == ref["add32"][0] ^ 0x40
    ph = raw["kinds"]["pinned"]["phases"]
    assert [p for p, v in ph.items() if v["errors"]] == ["atomics"]
    assert ph["atomics"]["compared"] == ph["atomics"]["expected"]
    assert summary["healthy"] is False
    assert summary["failing_atomics"][0]["op"] == "add_u32"


def test_record_cap_at_zero_counts_and_drops(native):
    raw, summary = run_a(native, kinds=["pinned"], max_records=0, poison_mask=1,
                         poison_word=9, poison_xor=BIT)
    assert raw["error_count"] == 1
    assert raw["records"] == []
    assert raw["records_dropped"] == 1
    assert raw["fail_mask"] == 1
    assert summary["healthy"] is False and summary["consistent"] is True


def test_health_report_gates_on_host_link(native):
    from k8s_operator_libs_amd.validation import gpu_health_check

    report = gpu_health_check(require_gpu=True, hostlink=True, hostlink_mib=1,
                              bw_buf_mib=128, bw_iters=2)
    link = report["checks"]["host_link"]
    print({k: v for k, v in link.items() if k in ("rates_gbps", "elapsed_ms")})
    assert report["healthy"] is True and link["healthy"] is True
    assert link["bytes"] == MIB and link["kinds"] == KINDS
    assert "records" not in link and "phases" not in link
    plain = gpu_health_check(require_gpu=True, bw_buf_mib=128, bw_iters=2)
    assert "host_link" not in plain["checks"]
    assert plain["healthy"] is True
