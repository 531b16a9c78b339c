"""Cross-XCD hand-off and device-scope atomics check (opt-in).

An MI355X is eight XCDs whose L2s are not coherent with each other.  A word
written on one XCD reaches a reader on another only through an agent-scope
release on the writer (L2 write-back), an agent-scope acquire on the reader
(L1 invalidate) and the fabric and memory-side atomics between them.  Split-K
reductions, stream-K and collective kernels stand on exactly that path, and
every other check of the validator stays inside one XCD.

The native ``xcd_fabric_check`` runs two kernels, neither of which ever waits
for another workgroup:

- the hand-off sweep: groups of workgroups each write a slab of a pattern,
  release it and draw a ticket; the last arriver of a group acquires and
  verifies every slab of the group exactly, and with them the slabs of up to
  two neighbour groups whose previous episode it finds complete at one look
  (``extra_lines``: counted, but no number of them is expected).  Each
  verified line is counted under its ``(writer_xcc, reader_xcc)`` pair, and
  rounds repeat (at least two) until every pair of the XCCs seen has been
  covered.  The payload is
  not reset between rounds, so a hand-off that did not happen reads the
  previous round's value and its record is flagged ``stale``;
- the atomics sweep: every thread of a whole-device grid adds, maximises,
  minimises, xors, ors and ands hash-derived values into shared cells at
  agent scope, draws a ticket from one counter and contends once for a CAS
  claim.  The host recomputes every total with the same generator.

This module turns the raw result into a verdict.  Coverage is counted, not
trusted: a run that lost an episode, verified fewer lines than it should or
left a pair uncovered is unhealthy, not clean.

Single-XCC caveat: on a partition that exposes one XCC the check still runs
and must still pass, but it proves nothing about the fabric; ``cross_xcd`` is
false then and the report says so.
"""

from __future__ import annotations

from typing import Any, Dict, List

from .gpu_health import load_native_validator, require_native_validator

# poison_mask bit -> the comparison it moves
POISON_COMPARISONS = (
    "payload", "header", "add_u32", "add_u64", "add_f32", "minmax",
    "bitwise", "tickets", "cas",
)


def summarize_xcd_fabric(raw: Dict[str, Any]) -> Dict[str, Any]:
    """Pure function: raw native result -> summary with a ``healthy`` verdict.

    ``healthy`` holds only with zero errors, no records, every episode
    completed, every line verified, every ``(writer, reader)`` pair of the
    XCCs seen covered, at least one XCC seen, and every atomic total, ticket
    and claim exact.  A raw table that contradicts itself (errors without
    records or the reverse, pair errors that do not add up to the payload
    error counter, a pair count that its own table does not show) is
    unhealthy too.
    """
    records = [dict(r) for r in raw.get("records", [])]
    pairs = [dict(p) for p in raw.get("pairs", [])]
    atomics = dict(raw.get("atomics") or {})
    error_count = int(raw["error_count"])
    payload_errors = int(raw.get("payload_errors", 0))
    header_errors = int(raw.get("header_errors", 0))
    episodes_completed = int(raw["episodes_completed"])
    episodes_expected = int(raw["episodes_expected"])
    lines_verified = int(raw["lines_verified"])
    lines_expected = int(raw["lines_expected"])
    extra_lines = int(raw.get("extra_lines_verified", 0))
    header_verified = int(raw.get("header_lines_verified", 0))
    header_expected = int(raw.get("header_lines_expected", 0))
    pairs_covered = int(raw["pairs_covered"])
    xcc_seen = int(raw["xcc_seen"])
    rounds = int(raw.get("rounds", 0))

    failing_pairs = sorted(
        (
            {
                "writer_xcc": int(p["writer_xcc"]),
                "reader_xcc": int(p["reader_xcc"]),
                "lines": int(p["lines"]) + int(p.get("extra_lines", 0)),
                "errors": int(p["errors"]),
            }
            for p in pairs if int(p["errors"]) != 0
        ),
        key=lambda p: (p["writer_xcc"], p["reader_xcc"]),
    )
    per_xcc: Dict[int, Dict[str, int]] = {}

    def xcc_entry(xcc: int) -> Dict[str, int]:
        return per_xcc.setdefault(int(xcc), {
            "lines_written": 0, "lines_read": 0, "errors_as_writer": 0,
            "errors_as_reader": 0, "adder_waves": 0,
        })

    for p in pairs:
        w, r = xcc_entry(p["writer_xcc"]), xcc_entry(p["reader_xcc"])
        lines = int(p["lines"]) + int(p.get("extra_lines", 0))
        w["lines_written"] += lines
        w["errors_as_writer"] += int(p["errors"])
        r["lines_read"] += lines
        r["errors_as_reader"] += int(p["errors"])
    for xcc, waves in enumerate(atomics.get("adders_per_xcc", [])):
        if int(waves):
            xcc_entry(xcc)["adder_waves"] = int(waves)

    mismatches = [dict(m) for m in atomics.get("mismatches", [])]
    failing_atomics = sorted(
        mismatches, key=lambda m: (str(m["op"]), int(m["cell"]))
    )
    tickets_ok = (
        int(atomics.get("tickets_missing", 0)) == 0
        and int(atomics.get("tickets_out_of_range", 0)) == 0
        and int(atomics.get("ticket_counter", -1))
        == int(atomics.get("tickets_expected", -2))
    )
    atomics_ok = bool(atomics) and not mismatches and tickets_ok

    failing = {str(m["comparison"]) for m in mismatches}
    failing.update(str(r["kind"]) for r in records)
    if payload_errors:
        failing.add("payload")
    if header_errors:
        failing.add("header")
    if atomics and not tickets_ok:
        failing.add("tickets")

    consistent = (
        (error_count == 0) == (not records)
        and error_count == payload_errors + header_errors
        and sum(int(p["errors"]) for p in pairs) == payload_errors
        and sum(
            1 for p in pairs
            if int(p["lines"]) + int(p.get("extra_lines", 0)) > 0
        ) == pairs_covered
        and sum(int(p["lines"]) for p in pairs) == lines_verified
        and sum(int(p.get("extra_lines", 0)) for p in pairs) == extra_lines
    )
    healthy = (
        consistent
        and error_count == 0
        and not records
        and episodes_completed == episodes_expected
        and lines_verified == lines_expected
        and header_verified == header_expected
        and int(raw.get("ticket_counter_errors", 0)) == 0
        and int(raw.get("tickets_out_of_range", 0)) == 0
        and int(raw.get("writer_xcc_out_of_range", 0)) == 0
        and xcc_seen >= 1
        and pairs_covered == xcc_seen * xcc_seen
        and rounds >= 2
        and atomics_ok
    )
    return {
        "healthy": bool(healthy),
        "consistent": bool(consistent),
        "cross_xcd": xcc_seen > 1,
        "xcc_seen": xcc_seen,
        "pairs_covered": pairs_covered,
        "pairs_expected": xcc_seen * xcc_seen,
        "rounds": rounds,
        "blocks": int(raw.get("blocks", 0)),
        "groups": int(raw.get("groups", 0)),
        "episodes_completed": episodes_completed,
        "episodes_expected": episodes_expected,
        "lines_verified": lines_verified,
        "lines_expected": lines_expected,
        "extra_lines_verified": extra_lines,
        "header_lines_verified": header_verified,
        "header_lines_expected": header_expected,
        "error_count": error_count,
        "payload_errors": payload_errors,
        "header_errors": header_errors,
        "ticket_counter_errors": int(raw.get("ticket_counter_errors", 0)),
        "tickets_out_of_range": int(raw.get("tickets_out_of_range", 0)),
        "writer_xcc_out_of_range": int(raw.get("writer_xcc_out_of_range", 0)),
        "failing_pairs": failing_pairs,
        "failing_atomics": failing_atomics,
        "failing_comparisons": sorted(failing),
        "stale_records": sum(1 for r in records if r.get("stale")),
        "records_dropped": int(raw.get("records_dropped", 0)),
        "atomics_ok": bool(atomics_ok),
        "tickets_ok": bool(tickets_ok),
        "per_xcc": dict(sorted(per_xcc.items())),
        "elapsed_ms": float(raw.get("elapsed_ms", 0.0)),
    }


def xcd_fabric_check(device: int = 0, **kw: Any) -> Dict[str, Any]:
    """Run the native cross-XCD check on ``device`` and summarize it.

    Keyword arguments go to the native ``xcd_fabric_check`` (``reps``,
    ``group``, ``slab_lines``, ``cells``, ``blocks``, ``max_rounds``, ``seed``,
    ``max_records`` and the data-only test hook ``poison_mask`` /
    ``poison_pair``).  The summary additionally carries the raw ``records``,
    ``pairs`` and ``atomics``.  A missing native validator is an error: there
    is no fallback for this check.
    """
    native = require_native_validator(load_native_validator)
    raw = native.xcd_fabric_check(device, **kw)
    summary = summarize_xcd_fabric(raw)
    summary["records"] = [dict(r) for r in raw["records"]]
    summary["pairs"] = [dict(p) for p in raw["pairs"]]
    summary["atomics"] = dict(raw["atomics"])
    return summary


__all__: List[str] = [
    "POISON_COMPARISONS", "summarize_xcd_fabric", "xcd_fabric_check",
]
