"""Whole-device per-CU coverage sweep (opt-in).

The quick MFMA smokes launch one wave, i.e. one matrix pipe out of the
1024 on an MI355X.  The native ``cu_coverage_check`` sweep runs the f32,
bf16 and fp8 MFMA tiles plus an LDS round trip in every wave of a grid that
fills the device, compares bit-exactly (integer operands, no tolerance) and
records the outcome per placement slot that each wave reads from its own
hardware registers.  This module turns that raw table into a verdict.

Placement-key caveat: the key is ``XCC_ID[3:0] << 8 | HW_ID[15:8]`` and is
treated as **opaque**.  The ``se`` / ``sh`` / ``cu`` fields decoded from it
follow the gfx9 ``HW_ID`` layout and are labels for humans only; nothing in
the verdict depends on them.  What carries the verdict is counting: the
number of distinct keys must equal the device's compute-unit count and the
number of distinct (key, SIMD) slots must be four times that.  A wrong
layout assumption, a harvested part or a partition mode therefore shows up
as a count mismatch (unhealthy), never as coverage that was not achieved.
"""

from __future__ import annotations

from typing import Any, Dict, List, Sequence

from .gpu_health import load_native_validator, require_native_validator

SIMDS_PER_CU = 4

# fail_mask bits, in bit order
FAIL_BITS = ("f32", "bf16", "fp8", "lds")
FAIL_F32, FAIL_BF16, FAIL_FP8, FAIL_LDS = 1, 2, 4, 8


def decode_key(key: int) -> Dict[str, int]:
    """Split a placement key into human-readable labels (gfx9 HW_ID layout:
    cu = HW_ID[11:8], sh = HW_ID[12], se = HW_ID[15:13]).  Labels only."""
    hw_bits = key & 0xFF
    return {
        "xcc": (key >> 8) & 0xF,
        "se": (hw_bits >> 5) & 0x7,
        "sh": (hw_bits >> 4) & 0x1,
        "cu": hw_bits & 0xF,
    }


def _failed_names(mask: int, fail_bits: Sequence[str]) -> List[str]:
    return [name for bit, name in enumerate(fail_bits) if mask & (1 << bit)]


def summarize_cu_coverage(raw: Dict[str, Any]) -> Dict[str, Any]:
    """Pure function: raw native result -> summary with a ``healthy`` verdict.

    Coverage is recounted from ``raw["units"]`` (one entry per covered slot)
    rather than trusted from the raw counters.  ``healthy`` holds only when no
    slot has a non-zero ``fail_mask``, every compute unit was seen and every
    one of them was seen on all four SIMDs.
    """
    return summarize_sweep(raw, FAIL_BITS)


def summarize_sweep(raw: Dict[str, Any], fail_bits: Sequence[str]) -> Dict[str, Any]:
    """The verdict of a whole-device sweep whose ``fail_mask`` bits are named,
    in bit order, by ``fail_bits`` (shared with :mod:`.mx_matrix`)."""
    compute_units = int(raw["compute_units"])
    units = [dict(u) for u in raw.get("units", [])]

    simds_by_key: Dict[int, set] = {}
    for u in units:
        simds_by_key.setdefault(int(u["key"]), set()).add(int(u["simd"]))
    cus_covered = len(simds_by_key)
    simd_slots_covered = sum(len(s) for s in simds_by_key.values())

    per_xcc: Dict[int, int] = {}
    for key in simds_by_key:
        xcc = decode_key(key)["xcc"]
        per_xcc[xcc] = per_xcc.get(xcc, 0) + 1

    failing_units = []
    for u in sorted(units, key=lambda u: (int(u["key"]), int(u["simd"]))):
        mask = int(u["fail_mask"])
        if not mask:
            continue
        entry = decode_key(int(u["key"]))
        entry.update(
            key=int(u["key"]), simd=int(u["simd"]), failed=_failed_names(mask, fail_bits)
        )
        failing_units.append(entry)

    healthy = (
        not failing_units
        and cus_covered == compute_units
        and simd_slots_covered == SIMDS_PER_CU * compute_units
    )
    return {
        "healthy": bool(healthy),
        "compute_units": compute_units,
        "cus_covered": cus_covered,
        "simd_slots_covered": simd_slots_covered,
        "per_xcc": dict(sorted(per_xcc.items())),
        "failing_units": failing_units,
        "uncovered_cus": max(0, compute_units - cus_covered),
        "rounds": int(raw.get("rounds", 0)),
        "elapsed_ms": float(raw.get("elapsed_ms", 0.0)),
    }


def cu_coverage_check(device: int = 0, **kw: Any) -> Dict[str, Any]:
    """Run the native sweep on ``device`` and summarize it.

    Keyword arguments go to the native ``cu_coverage_check`` (``reps``,
    ``max_rounds``, and the data-only test hook ``poison_key`` /
    ``poison_mask`` / ``poison_all``).  The summary additionally carries the
    raw per-slot list as ``units``.  A missing native validator is an error:
    there is no fallback for this check.
    """
    native = require_native_validator(load_native_validator)
    raw = native.cu_coverage_check(device, **kw)
    summary = summarize_cu_coverage(raw)
    summary["units"] = [dict(u) for u in raw["units"]]
    return summary
