"""LDS data-integrity check on a real MI355X.

A clean run must cover every CU with all 160 KiB, compare exactly as many
items per phase as the shape implies and find nothing.  The data-only poison
hook then proves that each phase's comparison is live, that a failure is named
by phase, CU, word and bank, and that what the kernel wrote at the bottom, in
the middle and at the very top of LDS equals the host reference (a record's
``got`` is real LDS content).  The single-wave probe pins the lane map of
``ds_read_b64_tr_b16`` against a transposer written here.  Nothing depends on
timing: times are printed, never asserted."""

import numpy as np
import pytest

from k8s_operator_libs_amd.validation import (
    gpu_health_check,
    summarize_lds_integrity,
)

pytestmark = pytest.mark.gpu

SEED = 0x1D5
PHASES = ("pattern", "subword", "transpose", "dma", "atomics", "permute")
WORDS = 40960
SMALL = {"blocks": 2, "reps": 1, "passes": 1, "max_rounds": 1}


@pytest.fixture(scope="module")
def native():
    import os

    from k8s_operator_libs_amd.validation import GpuHealthError, load_native_validator

    if not os.path.exists("/dev/kfd"):
        # CPU-only machine running an unfiltered `pytest tests/`: skip, also
        # where the extension is built (it cross-compiles without a GPU).
        pytest.skip("no GPU on this machine (missing /dev/kfd)")
    mod = load_native_validator()
    if mod is None:
        # On a real GPU box (ROCm kfd present) a missing native extension
        # stays a HARD failure — a silent skip there would green-wash the
        # exact fallback the driver checks for.
        raise GpuHealthError(
            "native validator must be present on a GPU box - refusing to skip"
        )
    return mod


def run(native, **kw):
    kw.setdefault("seed", SEED)
    raw = native.lds_integrity_check(0, **kw)
    summary = summarize_lds_integrity(raw)
    print(  # noqa: T201 (figures for the log, never asserted)
        f"lds_integrity {kw}: healthy={summary['healthy']} rounds={raw['rounds']} "
        f"blocks={raw['blocks']} cus={raw['cus_covered']}/{raw['compute_units']} "
        f"errors={raw['error_count']} dropped={raw['records_dropped']} "
        f"elapsed_ms={raw['elapsed_ms']:.3f}")
    return raw, summary


def items_expected(workgroups, reps, passes):
    """Items compared by `workgroups` workgroups, from the shape alone: every
    word twice per pattern (passes + the checker); every word once plus four
    bytes of one half and two halves of the other half of the words; 81920
    16-bit elements under two row strides; every word once; ten values in 64
    cells; two values per thread in eight steps."""
    per_rep = {
        "pattern": (passes + 1) * 2 * WORDS,
        "subword": WORDS + 4 * (WORDS // 2) + 2 * (WORDS // 2),
        "transpose": 2 * 81920,
        "dma": WORDS,
        "atomics": 64 * 10,
        "permute": 256 * 8 * 2,
    }
    return {p: workgroups * reps * n for p, n in per_rep.items()}


@pytest.fixture(scope="module")
def clean_default(native):
    """One clean run of the default shape, shared and left unchanged."""
    return run(native)


def test_clean_default_run_covers_every_cu_with_all_of_lds(clean_default):
    raw, s = clean_default
    assert raw["lds_bytes"] == 163840
    assert raw["error_count"] == 0 and raw["records"] == []
    assert raw["cus_covered"] == raw["compute_units"]
    assert s["cus_covered"] == s["compute_units"]  # recounted from the units
    assert raw["blocks"] == 2 * raw["compute_units"]
    want = items_expected(raw["blocks"] * raw["rounds"], reps=2, passes=3)
    assert dict(raw["phase_words_expected"]) == want
    assert dict(raw["phase_words_verified"]) == want
    assert sum(u["workgroups"] for u in raw["units"]) == raw["blocks"] * raw["rounds"]
    assert all(u["fail_mask"] == 0 for u in raw["units"])
    assert s["healthy"] is True


@pytest.mark.parametrize("bit", range(6), ids=PHASES)
def test_one_poison_bit_names_exactly_its_phase(native, bit):
    raw, s = run(native, poison_all=True, poison_mask=1 << bit, **SMALL)
    assert s["healthy"] is False
    assert len(s["failing_units"]) == len(raw["units"]) >= 1
    assert all(u["failed"] == [PHASES[bit]] for u in s["failing_units"])
    assert {r["phase"] for r in raw["records"]} == {PHASES[bit]}
    assert raw["error_count"] > 0
    assert raw["records_dropped"] == raw["error_count"] - len(raw["records"])
    assert raw["xor_or"] == 1
    # the counts are still complete
    want = items_expected(2, reps=1, passes=1)
    assert dict(raw["phase_words_verified"]) == want
    assert dict(raw["phase_words_expected"]) == want


@pytest.mark.parametrize("word", [0, 16384, 40959])
def test_poison_word_reaches_the_bottom_middle_and_top_of_lds(native, word):
    """Word 16384 is the first one no other check touches, 40959 the last."""
    xor = 0x00F00F01
    raw, s = run(native, poison_all=True, poison_mask=1, poison_word=word,
                 poison_xor=xor, **SMALL)
    assert s["healthy"] is False
    # two workgroups x (one hash pattern + the checker) x two verifying steps
    assert raw["error_count"] == len(raw["records"]) == 8
    assert raw["records_dropped"] == 0
    assert raw["xor_or"] == xor
    assert {w["word"] for w in s["failing_words"]} == {word}
    assert all(w["bank"] == word % 64 and w["byte_offset"] == 4 * word
               for w in s["failing_words"])
    assert s["suspect_banks"] == [word % 64]
    refs = {}
    for r in raw["records"]:
        assert r["phase"] == "pattern" and r["word"] == word
        assert r["expected"] ^ r["got"] == xor
        ref = refs.setdefault(
            (r["block"], r["rep"]),
            native.lds_integrity_reference(seed=SEED, block=r["block"],
                                           rep=r["rep"], passes=1))
        pattern, step = divmod(r["detail"], 4)
        image = ref["pattern_images"][pattern][word]
        # step 1 reads p, step 2 reads ~p: real memory content either way
        assert step in (1, 2)
        assert r["got"] == (image if step == 1 else image ^ 0xFFFFFFFF)
    assert {r["detail"] for r in raw["records"]} == {1, 2, 5, 6}


def test_poison_key_fails_only_that_cu(native, clean_default):
    units = clean_default[0]["units"]
    key = units[len(units) // 2]["key"]
    raw, s = run(native, poison_key=key, poison_mask=1 << 5)
    assert [u["key"] for u in s["failing_units"]] == [key]
    assert s["failing_units"][0]["failed"] == ["permute"]
    assert {r["key"] for r in raw["records"]} == {key}
    assert s["cus_covered"] == s["compute_units"]
    assert s["healthy"] is False


def tr_decode(image_u16, lane_byte_offsets):
    """Independent of the native code, from the documented map: in a group of
    16 lanes, lane 4q+p supplies the address of row q, columns 4p .. 4p+3;
    lane i receives column i of the four rows, row q in element q."""
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


def tr_offsets(base, stride, blocks_per_row):
    """Four blocks, one per 16-lane group, of an image with `stride`-byte rows
    that holds `blocks_per_row` blocks side by side, from byte `base`."""
    offs = []
    for lane in range(64):
        block, i = lane // 16, lane % 16
        offs.append(base + (block // blocks_per_row) * 4 * stride
                    + (i // 4) * stride + (block % blocks_per_row) * 32
                    + 8 * (i % 4))
    return offs


@pytest.mark.parametrize("layout", ["rows64_at_base", "padded72", "top_of_lds"])
def test_tr_tile_matches_an_independent_transposer(native, layout):
    rng = np.random.default_rng(7)
    if layout == "rows64_at_base":
        image = rng.permutation(65536)[:4096]
        offs = tr_offsets(0, 64, 2)
    elif layout == "padded72":
        # 64-byte rows padded by 8 bytes, blocks from byte 1800 on
        image = rng.permutation(65536)[:4096]
        offs = tr_offsets(1800, 72, 2)
    else:
        # 81920 elements cannot all differ in 16 bits: the top 65536 do, and
        # every address of the read lies in the last 512 bytes; the fourth
        # block ends at byte 163839
        image = np.concatenate([np.arange(16384), rng.permutation(65536)])
        offs = tr_offsets(163840 - 512, 64, 2)
        assert max(offs) + 8 == 163840
    assert all(o % 8 == 0 for o in offs)
    got = np.array(native.lds_tr_tile(0, [int(v) for v in image], offs))
    want = tr_decode(image, offs)
    assert got.shape == (64, 4)
    assert np.array_equal(got, want)
    assert len(np.unique(want)) == 256  # distinct values: no lucky match


def test_gpu_health_check_with_lds(native):
    report = gpu_health_check(0, bw_buf_mib=64.0, bw_iters=2, require_gpu=True,
                              lds=True)
    summary = report["checks"]["lds_integrity"]
    assert summary["healthy"] is True
    assert summary["cus_covered"] == summary["compute_units"]
    assert summary["lds_bytes"] == 163840
    assert summary["error_count"] == 0
    assert "units" not in summary and "records" not in summary
    assert report["healthy"] is True
