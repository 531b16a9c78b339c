"""Host-link data-integrity check (opt-in).

Every other check stays on the package; the only bytes that come back are
small result tables.  The native ``host_link_check`` compares what crosses the
path between host memory and the device, the path the driver owns: pinning,
IOMMU and GART mappings, the copy engines, userptr registration and PCIe
AtomicOps.  Per memory kind (``pinned``: ``hipHostMalloc``; ``registered``:
ordinary pages under ``hipHostRegister``; ``pageable``: ``malloc``) a hash
pattern goes host to device and back, is read and written by a kernel through
the buffer's device pointer (16-byte, byte and 16-bit stores), is copied in
both directions at once, and crosses in 464 short copies at odd offsets and
lengths whose whole destination slots are compared; on pinned memory
system-scope fetch-add, swap and compare-and-swap run while the host thread
adds to the same cells.  Comparison is exact, and what each phase compared is
counted and checked here: a phase that compared less than it covers is
unhealthy, not clean.  This module turns the raw result into a verdict.

Stale content is always another seed's hash words, so a transfer that did not
happen shows as words with about half their bits flipped; a stuck or coupled
data bit shows in ``flipped_bits``; a copy that wrote one byte too many, too
few or one byte off shows in ``failing_cases`` with the offset inside the slot.

Rates are reported (``rates_gbps``) and never judged.  When the device does
not report native host atomics the atomics phase is skipped and the summary
says ``atomics_supported: False``; nothing is claimed about them then.
"""

from __future__ import annotations

from typing import Any, Dict, List

from .gpu_health import load_native_validator, require_native_validator
from .hbm_integrity import flipped_bits, mib_to_bytes

MIB = 1 << 20
KINDS = ("pinned", "registered", "pageable")
PHASES = ("h2d", "d2h", "zc_read", "zc_write", "duplex", "unaligned", "atomics")
# pageable memory has no device pointer; atomics run on pinned memory only
KIND_PHASES = {
    "pinned": PHASES,
    "registered": PHASES[:6],
    "pageable": ("h2d", "d2h", "unaligned"),
}
PLAN_CASES = 464


def summarize_host_link(raw: Dict[str, Any]) -> Dict[str, Any]:
    """Pure function: raw native result -> summary with a ``healthy`` verdict.

    ``healthy`` holds only when the error counter is zero, no mismatch was
    recorded or dropped, every kind ran exactly the phases it has and every
    phase compared exactly what it covers.  A raw table that contradicts
    itself (errors without a failing phase, phase errors that do not add up)
    is unhealthy too.  A skipped atomics phase on a device without native host
    atomics is not a fault: it is flagged in ``atomics_supported``.
    """
    records = [dict(r) for r in raw.get("records", [])]
    error_count = int(raw["error_count"])
    atomics_supported = bool(raw.get("atomics_supported", False))
    kinds = {str(k): dict(v) for k, v in dict(raw["kinds"]).items()}

    failing_phases: Dict[str, List[str]] = {}
    short_phases: Dict[str, List[str]] = {}
    rates: Dict[str, Dict[str, float]] = {}
    compared: Dict[str, Dict[str, int]] = {}
    phase_errors = 0
    shape_ok = bool(kinds)
    for kind, table in kinds.items():
        phases = {str(p): dict(v) for p, v in dict(table["phases"]).items()}
        want = [p for p in KIND_PHASES.get(kind, ())
                if p != "atomics" or atomics_supported]
        shape_ok = shape_ok and list(phases) == want
        failing_phases[kind] = [p for p, v in phases.items() if int(v["errors"])]
        short_phases[kind] = [
            p for p, v in phases.items()
            if int(v["compared"]) != int(v["expected"])
        ]
        rates[kind] = {p: float(v.get("gbps", 0.0)) for p, v in phases.items()
                       if p != "atomics"}
        compared[kind] = {p: int(v["compared"]) for p, v in phases.items()}
        phase_errors += sum(int(v["errors"]) for v in phases.values())

    failing_words = sorted(
        (
            {
                "kind": str(r["kind"]),
                "phase": str(r["phase"]),
                "side": str(r["side"]),
                "word": int(r["word"]),
                "byte_offset": int(r["byte_offset"]),
                "expected": int(r["expected"]),
                "got": int(r["got"]),
                "flipped_bits": flipped_bits(int(r["expected"]) ^ int(r["got"])),
            }
            for r in records if "word" in r
        ),
        key=lambda r: (KINDS.index(r["kind"]) if r["kind"] in KINDS else 99,
                       PHASES.index(r["phase"]) if r["phase"] in PHASES else 99,
                       r["word"]),
    )
    failing_cases = sorted(
        (
            {
                "kind": str(r["kind"]),
                "case": int(r["case"]),
                "direction": str(r["direction"]),
                "src_off": int(r["src_off"]),
                "dst_off": int(r["dst_off"]),
                "len": int(r["len"]),
                "byte_offset": int(r["byte_offset"]),
                "expected": int(r["expected"]),
                "got": int(r["got"]),
                "flipped_bits": flipped_bits(int(r["expected"]) ^ int(r["got"])),
            }
            for r in records if "case" in r
        ),
        key=lambda r: (r["kind"], r["case"], r["byte_offset"]),
    )
    failing_atomics = sorted(
        (
            {
                "comparison": str(r["comparison"]),
                "op": str(r["op"]),
                "cell": int(r["cell"]),
                "expected": int(r["expected"]),
                "got": int(r["got"]),
            }
            for r in records if "comparison" in r
        ),
        key=lambda r: (r["op"], r["cell"]),
    )

    consistent = (
        shape_ok
        and phase_errors == error_count
        and (error_count == 0) == (not records
                                   and not int(raw.get("records_dropped", 0)))
        and (int(raw.get("fail_mask", 0)) == 0) == (error_count == 0)
    )
    healthy = (
        consistent
        and error_count == 0
        and not records
        and not any(short_phases.values())
        and int(raw.get("plan_cases", 0)) == PLAN_CASES
    )
    return {
        "healthy": bool(healthy),
        "consistent": bool(consistent),
        "bytes": int(raw["bytes"]),
        "kinds": list(kinds),
        "error_count": error_count,
        "fail_mask": int(raw.get("fail_mask", 0)),
        "xor_or": int(raw.get("xor_or", 0)),
        "flipped_bits": flipped_bits(int(raw.get("xor_or", 0))),
        "failing_phases": failing_phases,
        "short_phases": short_phases,
        "compared": compared,
        "failing_words": failing_words,
        "failing_cases": failing_cases,
        "failing_atomics": failing_atomics,
        "records_dropped": int(raw.get("records_dropped", 0)),
        "plan_cases": int(raw.get("plan_cases", 0)),
        "rates_gbps": rates,
        "duplex_overlap": {
            kind: bool(table["duplex_overlap"])
            for kind, table in kinds.items() if "duplex_overlap" in table
        },
        "atomics_supported": atomics_supported,
        "elapsed_ms": float(raw.get("elapsed_ms", 0.0)),
    }


def host_link_check(device: int = 0, mib: float = 64.0, **kw: Any) -> Dict[str, Any]:
    """Run the native host-link check with ``mib`` MiB per buffer on ``device``
    and summarize it.

    Keyword arguments go to the native ``host_link_check`` (``seed``,
    ``kinds``, ``blocks``, ``atomics_blocks``, ``reps``, ``host_adds``,
    ``max_records`` and the data-only test hook ``poison_mask`` /
    ``poison_kind`` / ``poison_word`` / ``poison_case`` / ``poison_xor``).  The
    summary additionally carries the raw ``records``, ``phases`` per kind and
    the ``atomics`` tables.  A missing native validator is an error: there is
    no fallback for this check.
    """
    native = require_native_validator(load_native_validator)
    raw = native.host_link_check(device, mib_to_bytes(mib), **kw)
    summary = summarize_host_link(raw)
    summary["records"] = [dict(r) for r in raw["records"]]
    summary["phases"] = {
        str(kind): {str(p): dict(v) for p, v in dict(table["phases"]).items()}
        for kind, table in dict(raw["kinds"]).items()
    }
    summary["atomics"] = dict(raw["atomics"]) if raw.get("atomics") else None
    return summary


__all__: List[str] = ["host_link_check", "summarize_host_link"]
