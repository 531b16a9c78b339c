"""HBM data-integrity check (opt-in).

``hbm_bandwidth_gbps`` times a copy and never looks at what arrived.  The
native ``hbm_pattern_check`` writes a pattern that is a pure function of each
64-bit word's logical index over a region of device memory, reads it back,
writes the inverse, and reads that back (moving inversions), comparing
exactly.  Every phase covers the whole region before the next one starts, so
for a region larger than the caches the reads are served by HBM.  The words
compared are counted on the device and the count is checked here: a verify
phase that skipped part of the region is unhealthy, not clean.  This module
turns the raw result into a verdict.

What a mismatch means: a stuck or coupled data bit shows in ``flipped_bits``;
an address-decoding or page-mapping fault shows as words that hold another
index's value (many flipped bits, the ``hash`` pattern differs everywhere).

ECC caveat: on a part with ECC an uncorrectable error surfaces as a fault of
the process, not as a flipped bit here, and correctable errors are repaired
silently; the RAS counters that count them are not read by this check.

Cache caveat: ``beyond_cache`` is true only when the region exceeds 512 MiB,
twice the 256 MiB Infinity Cache.  Below that the check exercises the caches
as much as HBM, and says so.
"""

from __future__ import annotations

import statistics
from typing import Any, Dict, List

from .gpu_health import load_native_validator, require_native_validator

MIB = 1 << 20
PHASE_KINDS = ("fill", "verify_invert", "verify")


def flipped_bits(mask: int) -> List[int]:
    """Bit positions set in a 64-bit xor mask, ascending."""
    return [bit for bit in range(64) if (int(mask) >> bit) & 1]


def mib_to_bytes(mib: float) -> int:
    """MiB -> a byte count the native check accepts (a multiple of 8).
    ``0`` stays ``0``: all free memory minus the native reserve."""
    if mib < 0:
        raise ValueError("memory size in MiB must not be negative")
    return (int(mib * MIB) // 8) * 8


def summarize_hbm_integrity(raw: Dict[str, Any]) -> Dict[str, Any]:
    """Pure function: raw native result -> summary with a ``healthy`` verdict.

    ``healthy`` holds only when the error counter is zero, no mismatch was
    recorded and the device compared exactly as many words as the verify
    phases cover.  A raw table that contradicts itself (errors without
    records, records without errors) is therefore unhealthy too.
    """
    records = [dict(r) for r in raw.get("records", [])]
    error_count = int(raw["error_count"])
    words_verified = int(raw["words_verified"])
    words_expected = int(raw["words_expected"])

    failing_words = []
    per_chunk: Dict[int, int] = {}
    for r in sorted(records, key=lambda r: (int(r["word"]), int(r["phase"]))):
        entry = {
            "word": int(r["word"]),
            "byte_offset": int(r["byte_offset"]),
            "chunk": int(r["chunk"]),
            "phase": int(r["phase"]),
            "expected": int(r["expected"]),
            "got": int(r["got"]),
            "flipped_bits": flipped_bits(int(r["expected"]) ^ int(r["got"])),
        }
        failing_words.append(entry)
        per_chunk[entry["chunk"]] = per_chunk.get(entry["chunk"], 0) + 1

    by_kind: Dict[str, List[float]] = {}
    for ph in raw.get("phases", []):
        by_kind.setdefault(str(ph["kind"]), []).append(float(ph["gbps"]))
    gbps_median = {
        kind: statistics.median(by_kind[kind])
        for kind in PHASE_KINDS if kind in by_kind
    }

    healthy = (
        error_count == 0
        and not records
        and words_verified == words_expected
    )
    return {
        "healthy": bool(healthy),
        "bytes": int(raw["bytes"]),
        "words": int(raw["words"]),
        "chunks": len(raw.get("chunks", [])),
        "words_verified": words_verified,
        "words_expected": words_expected,
        "error_count": error_count,
        "xor_or": int(raw.get("xor_or", 0)),
        "flipped_bits": flipped_bits(int(raw.get("xor_or", 0))),
        "failing_words": failing_words,
        "records_dropped": int(raw.get("records_dropped", 0)),
        # only as far as the (capped) records show them
        "recorded_errors_per_chunk": dict(sorted(per_chunk.items())),
        "beyond_cache": bool(raw.get("beyond_cache", False)),
        "gbps_median": gbps_median,
        "elapsed_ms": float(raw.get("elapsed_ms", 0.0)),
    }


def hbm_integrity_check(device: int = 0, mib: float = 1024.0, **kw: Any) -> Dict[str, Any]:
    """Run the native pattern test over ``mib`` MiB of ``device`` (``0``: all
    free memory minus a 2 GiB reserve) and summarize it.

    Keyword arguments go to the native ``hbm_pattern_check`` (``chunk_bytes``,
    ``passes``, ``seed``, ``checker``, ``first_word``, ``max_records`` and the
    data-only test hook ``poison_word`` / ``poison_stride`` / ``poison_xor`` /
    ``poison_phase``).  The summary additionally carries the raw ``records``
    and ``phases``.  A missing native validator is an error: there is no
    fallback for this check.
    """
    native = require_native_validator(load_native_validator)
    raw = native.hbm_pattern_check(device, mib_to_bytes(mib), **kw)
    summary = summarize_hbm_integrity(raw)
    summary["records"] = [dict(r) for r in raw["records"]]
    summary["phases"] = [dict(p) for p in raw["phases"]]
    return summary
