"""Whole-device sweep of the MX block-scaled matrix path (opt-in).

CDNA4's ``v_mfma_scale_f32_16x16x128_f8f6f4`` / ``_32x32x64_`` take OCP MX
operands (e4m3, e5m2, e2m3, e3m2, e2m1) with one E8M0 scale per 32-element K
block.  It is the path MXFP4 / MXFP6 / MXFP8 serving runs on and it has its
own 6-bit and 4-bit unpackers and scale application, which the f32 / bf16 /
fp8 tiles of :mod:`.cu_coverage` never touch.  The native
``mx_coverage_check`` sweep issues, in every wave of a grid that fills the
device, the five same-format pairs and three mixed pairs on 16x16x128 plus
e2m1 and e4m3 on 32x32x64, over operand sets whose scales differ between
neighbouring rows, columns and K blocks, and compares bit-exactly: operands
and scales are chosen so that every summation order gives the same f32 (see
``validation/README.md`` for the condition).  This module turns the raw
per-slot table into a verdict; placement keys are the opaque keys of
:mod:`.cu_coverage` and are counted the same way.
"""

from __future__ import annotations

from typing import Any, Dict

from .cu_coverage import summarize_sweep
from .gpu_health import load_native_validator, require_native_validator

# fail_mask bits, in bit order: one per same-format pair on 16x16x128, one for
# the mixed pairs (cbsz != blgp), one for the 32x32x64 shape
FAIL_BITS = ("e4m3", "e5m2", "e2m3", "e3m2", "e2m1", "mixed", "shape32")

# formats of the burn-in, reported as mx_matrix["throughput_tflops"]
THROUGHPUT_FORMATS = ("e2m1", "e4m3")
THROUGHPUT_ITERS = 20000


def summarize_mx_matrix(raw: Dict[str, Any]) -> Dict[str, Any]:
    """Pure function: raw native result -> summary with a ``healthy`` verdict.

    Coverage is recounted from ``raw["units"]`` (one entry per covered slot)
    rather than trusted from the raw counters.  ``healthy`` holds only when no
    slot has a non-zero ``fail_mask``, every compute unit was seen and every
    one of them was seen on all four SIMDs.  Each entry of ``failing_units``
    names the unit (labels from ``cu_coverage.decode_key``) and, in
    ``failed``, the bits of :data:`FAIL_BITS` it failed.
    """
    return summarize_sweep(raw, FAIL_BITS)


def mx_matrix_check(device: int = 0, **kw: Any) -> Dict[str, Any]:
    """Run the native MX sweep on ``device`` and summarize it.

    Keyword arguments go to the native ``mx_coverage_check`` (``reps``,
    ``max_rounds``, and the data-only test hook ``poison_key`` /
    ``poison_mask`` / ``poison_all``).  The summary additionally carries the
    raw per-slot list as ``units``.  A missing native validator is an error:
    there is no fallback for this check.
    """
    native = require_native_validator(load_native_validator)
    raw = native.mx_coverage_check(device, **kw)
    summary = summarize_mx_matrix(raw)
    summary["units"] = [dict(u) for u in raw["units"]]
    return summary
