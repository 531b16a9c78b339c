"""Whole-device sweep of the vector ALU (opt-in).

Every other sweep uses the VALU only to compare what another unit produced:
a SIMD whose ``v_fma_f32`` or fp8 converter is wrong in one lane passes all of
them.  The native ``valu_coverage_check`` runs, in every wave of a grid that
fills the device, a fixed table of vector instructions over host-generated
operands: f32 / f64 / f16 arithmetic, integer and bit ops, conversions (f16,
bf16, fp8, bf8, fp4) and cross-lane ops (DPP, ``v_readlane``,
``v_permlane16/32_swap``) are compared bit-exactly against a host reference;
the raw transcendentals, stochastic rounding and ``v_prng_b32`` have no host
expectation and must give the same bits on every SIMD of the device.  Every
compare is counted, and the count is checked.  This module turns the raw
per-slot table into a verdict; placement keys are the opaque keys of
:mod:`.cu_coverage` and are counted the same way.  See
``validation/README.md`` for the exactness conditions and for what the check
does not prove.
"""

from __future__ import annotations

from collections import Counter
from typing import Any, Dict, List, Optional, Tuple

from .cu_coverage import decode_key, summarize_sweep
from .gpu_health import load_native_validator, require_native_validator

# fail_mask bits, in bit order
FAIL_BITS = ("f32", "f64", "f16", "int", "convert", "crosslane", "consensus")
CONSENSUS = "consensus"


def _strict_majority(values: List[int]) -> Optional[int]:
    """The value more than half of ``values`` hold, or None."""
    if not values:
        return None
    value, count = Counter(values).most_common(1)[0]
    return value if 2 * count > len(values) else None


def summarize_valu(raw: Dict[str, Any]) -> Dict[str, Any]:
    """Pure function: raw native result -> summary with a ``healthy`` verdict.

    Builds on :func:`.cu_coverage.summarize_sweep` (coverage recounted from
    ``raw["units"]``, ``failing_units`` named by :data:`FAIL_BITS`) and adds:

    - the consensus: per consensus op, the digest a **strict majority** of the
      covered slots hold (``consensus_digests[op]``; ``None`` and unhealthy
      when there is none).  A slot holding a digest tuple that differs from the
      majority at any op gets ``consensus`` in its ``failed`` list; a slot that
      holds two tuples differs with at least one of them;
    - the count: ``compared[g]`` must equal ``waves_run * reps * items[g]`` for
      every group, else the run is unhealthy even with zero errors and the
      groups are listed in ``short_groups``;
    - ``failing_ops`` (instruction names from the mismatch records),
      ``error_count``, ``records_dropped`` and ``elapsed_ms`` (never judged).
    """
    summary = summarize_sweep(raw, FAIL_BITS)
    units = [dict(u) for u in raw.get("units", [])]
    ops = [str(o) for o in raw.get("consensus_ops", [])]

    # one vote per (slot, tuple): a slot with two tuples votes with both
    tuples: List[Tuple[Tuple[int, int], Tuple[int, ...]]] = []
    for u in units:
        slot = (int(u["key"]), int(u["simd"]))
        for t in u.get("digests", []):
            tuples.append((slot, tuple(int(v) for v in t)))
    consensus: Dict[str, Optional[int]] = {}
    for i, op in enumerate(ops):
        consensus[op] = _strict_majority([t[i] for _, t in tuples if i < len(t)])
    no_majority = [op for op in ops if consensus[op] is None]

    deviant = set()
    for slot, t in tuples:
        if len(t) != len(ops) or any(
            consensus[op] is not None and t[i] != consensus[op]
            for i, op in enumerate(ops)
        ):
            deviant.add(slot)
    # a covered slot without any digest record reported nothing to agree with
    for u in units:
        if not u.get("digests"):
            deviant.add((int(u["key"]), int(u["simd"])))

    failing = {(e["key"], e["simd"]): e for e in summary["failing_units"]}
    for slot in deviant:
        entry = failing.get(slot)
        if entry is None:
            entry = decode_key(slot[0])
            entry.update(key=slot[0], simd=slot[1], failed=[])
            failing[slot] = entry
        if CONSENSUS not in entry["failed"]:
            entry["failed"].append(CONSENSUS)
    failing_units = [failing[s] for s in sorted(failing)]

    waves_run = int(raw.get("waves_run", 0))
    reps = int(raw.get("reps", 0))
    compared = [int(v) for v in raw.get("compared", [])]
    items = [int(v) for v in raw.get("items", [])]
    expected = [waves_run * reps * n for n in items]
    short_groups = [
        name
        for g, name in enumerate(FAIL_BITS)
        if g >= len(compared) or g >= len(expected) or compared[g] != expected[g]
    ]

    records = [dict(r) for r in raw.get("records", [])]
    failing_ops = sorted({str(r["op"]) for r in records})
    error_count = int(raw.get("error_count", 0))

    summary["failing_units"] = failing_units
    summary["healthy"] = bool(
        summary["healthy"]
        and not failing_units
        and not no_majority
        and not short_groups
        and error_count == 0
        and waves_run > 0
    )
    summary.update(
        waves_run=waves_run,
        reps=reps,
        compared=compared,
        compared_expected=expected,
        short_groups=short_groups,
        consensus_digests=consensus,
        failing_ops=failing_ops,
        error_count=error_count,
        records_dropped=int(raw.get("records_dropped", 0)),
    )
    return summary


def valu_check(device: int = 0, **kw: Any) -> Dict[str, Any]:
    """Run the native vector-ALU sweep on ``device`` and summarize it.

    Keyword arguments go to the native ``valu_coverage_check`` (``reps``,
    ``max_rounds``, and the data-only test hook ``poison_key`` /
    ``poison_mask`` / ``poison_all``).  The summary additionally carries the
    raw per-slot list as ``units`` and the mismatch records as ``records``.  A
    missing native validator is an error: there is no fallback for this check.
    """
    native = require_native_validator(load_native_validator)
    raw = native.valu_coverage_check(device, **kw)
    summary = summarize_valu(raw)
    summary["units"] = [dict(u) for u in raw["units"]]
    summary["records"] = [dict(r) for r in raw["records"]]
    return summary
