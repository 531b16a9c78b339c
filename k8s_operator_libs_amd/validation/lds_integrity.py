"""LDS data-integrity check: all 160 KiB on every CU (opt-in).

Every GEMM, attention and MoE kernel on an MI355X stages every operand
through the Local Data Share, and the other checks touch at most 64 KiB of it
with one access width and one value per word.  The native
``lds_integrity_check`` puts one workgroup on a CU that claims the whole
160 KiB and runs six phases over it, each with its own ``fail_mask`` bit and
its own counter of compared items:

- ``pattern``: moving inversions over all 40960 words (hash patterns and a
  checker; fill, verify and invert, verify) in ``b32``, ``b64`` and ``b128``
  accesses, every word verified by another wave than the one that wrote it;
- ``subword``: every word assembled over its inverse from ``ds_write_b8`` /
  ``ds_write_b16`` stores of different waves, verified whole and read back
  with ``ds_read_u8`` / ``ds_read_u16`` (the byte enables);
- ``transpose``: the whole array read with ``ds_read_b64_tr_b16`` under two
  row strides;
- ``dma``: the whole array filled by direct global->LDS loads
  (``global_load_lds_dword`` / ``_dwordx4``) from permuted source addresses;
- ``atomics``: the LDS atomic ALU (add u32 / u64 / f32, max, min, xor, or,
  and, compare-and-swap);
- ``permute``: the ``ds_bpermute_b32`` / ``ds_permute_b32`` crossbar.

This module turns the raw result into a verdict.  Comparisons are exact and
coverage is counted, not trusted: a run that compared fewer items than it
should, or missed a compute unit, is unhealthy even with zero errors.

Placement-key caveat: as in :mod:`.cu_coverage` the key
``XCC_ID[3:0] << 8 | HW_ID[15:8]`` is opaque; the ``se`` / ``sh`` / ``cu``
labels decoded from it are for humans only and the verdict counts distinct
keys against the device's compute-unit count.
"""

from __future__ import annotations

from typing import Any, Dict, List

from .cu_coverage import _failed_names, decode_key
from .gpu_health import load_native_validator, require_native_validator

# fail_mask / poison_mask bits, in bit order
PHASES = ("pattern", "subword", "transpose", "dma", "atomics", "permute")
LDS_BYTES = 163840
LDS_BANKS = 64
# phases whose record ``word`` is a word of the array written and read back
# as data, so that its bank says something about the memory
_MEMORY_PHASES = ("pattern", "subword")


def _flipped_bits(xor: int) -> List[int]:
    return [b for b in range(64) if (xor >> b) & 1]


def summarize_lds_integrity(raw: Dict[str, Any]) -> Dict[str, Any]:
    """Pure function: raw native result -> summary with a ``healthy`` verdict.

    ``healthy`` holds only with zero errors and no records, every phase's
    compared-item count equal to the expected one, every compute unit covered,
    no unit with a non-zero ``fail_mask`` and ``records_dropped`` equal to the
    errors that found no record slot.
    """
    compute_units = int(raw["compute_units"])
    units = [dict(u) for u in raw.get("units", [])]
    records = [dict(r) for r in raw.get("records", [])]
    error_count = int(raw["error_count"])
    records_dropped = int(raw.get("records_dropped", 0))
    verified = {p: int(raw["phase_words_verified"][p]) for p in PHASES}
    expected = {p: int(raw["phase_words_expected"][p]) for p in PHASES}

    keys = {int(u["key"]) for u in units}
    cus_covered = len(keys)
    per_xcc: Dict[int, int] = {}
    for key in keys:
        xcc = decode_key(key)["xcc"]
        per_xcc[xcc] = per_xcc.get(xcc, 0) + 1

    failing_units = []
    for u in sorted(units, key=lambda u: int(u["key"])):
        mask = int(u["fail_mask"])
        if not mask:
            continue
        entry = decode_key(int(u["key"]))
        entry.update(key=int(u["key"]), failed=_failed_names(mask, PHASES))
        failing_units.append(entry)

    failing_words = sorted(
        (
            {
                "key": int(r["key"]),
                "block": int(r["block"]),
                "rep": int(r["rep"]),
                "phase": str(r["phase"]),
                "word": int(r["word"]),
                "bank": int(r["word"]) % LDS_BANKS,
                "byte_offset": 4 * int(r["word"]),
                "expected": int(r["expected"]),
                "got": int(r["got"]),
                "flipped_bits": _flipped_bits(int(r["expected"]) ^ int(r["got"])),
            }
            for r in records
        ),
        key=lambda w: (w["key"], w["word"], w["phase"], w["rep"], w["block"]),
    )
    errors_per_bank: Dict[int, int] = {}
    for w in failing_words:
        errors_per_bank[w["bank"]] = errors_per_bank.get(w["bank"], 0) + 1

    # a bank is suspect when it holds all recorded memory mismatches of a unit
    banks_by_unit: Dict[int, set] = {}
    for w in failing_words:
        if w["phase"] in _MEMORY_PHASES:
            banks_by_unit.setdefault(w["key"], set()).add(w["bank"])
    suspect_banks = sorted(
        {next(iter(b)) for b in banks_by_unit.values() if len(b) == 1}
    )
    flipped = sorted({b for w in failing_words for b in w["flipped_bits"]})

    short_phases = [p for p in PHASES if verified[p] != expected[p]]
    consistent = (
        (error_count == 0) == (not records)
        and records_dropped == error_count - len(records)
        and (error_count == 0) == (not failing_units)
    )
    healthy = (
        consistent
        and error_count == 0
        and not records
        and not failing_units
        and not short_phases
        and cus_covered == compute_units
        and int(raw.get("lds_bytes", 0)) == LDS_BYTES
    )
    return {
        "healthy": bool(healthy),
        "consistent": bool(consistent),
        "compute_units": compute_units,
        "cus_covered": cus_covered,
        "uncovered_cus": max(0, compute_units - cus_covered),
        "per_xcc": dict(sorted(per_xcc.items())),
        "rounds": int(raw.get("rounds", 0)),
        "blocks": int(raw.get("blocks", 0)),
        "lds_bytes": int(raw.get("lds_bytes", 0)),
        "phase_words_verified": verified,
        "phase_words_expected": expected,
        "short_phases": short_phases,
        "error_count": error_count,
        "xor_or": int(raw.get("xor_or", 0)),
        "flipped_bits": flipped,
        "failing_units": failing_units,
        "failing_words": failing_words,
        "errors_per_bank": dict(sorted(errors_per_bank.items())),
        "suspect_banks": suspect_banks,
        "records_dropped": records_dropped,
        "elapsed_ms": float(raw.get("elapsed_ms", 0.0)),
    }


def lds_integrity_check(device: int = 0, **kw: Any) -> Dict[str, Any]:
    """Run the native LDS check on ``device`` and summarize it.

    Keyword arguments go to the native ``lds_integrity_check`` (``reps``,
    ``passes``, ``max_rounds``, ``seed``, ``blocks`` and the data-only test
    hook ``poison_key`` / ``poison_mask`` / ``poison_all`` / ``poison_word`` /
    ``poison_xor``).  The summary additionally carries the raw ``units`` and
    ``records``.  A missing native validator is an error: there is no
    fallback for this check.
    """
    native = require_native_validator(load_native_validator)
    raw = native.lds_integrity_check(device, **kw)
    summary = summarize_lds_integrity(raw)
    summary["units"] = [dict(u) for u in raw["units"]]
    summary["records"] = [dict(r) for r in raw["records"]]
    return summary


__all__: List[str] = ["PHASES", "lds_integrity_check", "summarize_lds_integrity"]
