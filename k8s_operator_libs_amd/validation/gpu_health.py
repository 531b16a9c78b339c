"""GPU health-check implementation (see package docstring)."""

from __future__ import annotations

import importlib
import json
import os
import shutil
import subprocess
from typing import Any, Dict

# Acceptance thresholds for an MI355X node.
MFMA_F32_MAX_ERR = 1e-6       # exact fmaf-chain numerics: effectively zero
MFMA_BF16_MAX_ERR = 5e-2      # bf16 inputs, f32 accumulate, K=32
MFMA_FP8_MAX_ERR = 5e-2       # OCP e4m3 inputs, f32 accumulate
HBM_MIN_GBPS = 1000.0         # far below the ~6000 GB/s measured copy BW,
                              # catches catastrophically degraded memory
MFMA_MIN_TFLOPS = 1000.0      # deep mode: half the bf16 issue-rate floor,
                              # catches down-clocked / power-capped parts


class GpuHealthError(RuntimeError):
    pass


def _gpu_present() -> bool:
    if shutil.which("rocm-smi") or shutil.which("amd-smi"):
        return os.path.exists("/dev/kfd")
    return os.path.exists("/dev/kfd")


def load_native_validator():
    """Import the native extension, building it on the fly if necessary.

    On a machine with an AMD GPU a missing/unbuildable extension raises
    GpuHealthError — validation must never silently fall back.
    On CPU-only machines returns None.
    """
    try:
        return importlib.import_module(
            "k8s_operator_libs_amd.native._gpu_validator"
        )
    except ImportError as exc:
        try:
            from ..native import build as native_build

            native_build.build()
            return importlib.import_module(
                "k8s_operator_libs_amd.native._gpu_validator"
            )
        except Exception as build_exc:
            if _gpu_present():
                raise GpuHealthError(
                    f"native GPU validator unavailable on a GPU machine: "
                    f"import error={exc}; build error={build_exc}"
                ) from build_exc
            return None


def require_native_validator(load=load_native_validator):
    """The native extension for a check that cannot run without it:
    GpuHealthError where `load` gives None.  A wrapper module passes its own
    binding of load_native_validator, the name a caller may have replaced."""
    native = load()
    if native is None:
        raise GpuHealthError("no native GPU validator available")
    return native


def smi_probe() -> Dict[str, Any]:
    """amd-smi / rocm-smi process probe: is the driver loaded and are
    devices enumerated?  Returns {'tool': ..., 'ok': bool, 'raw': ...}."""
    for tool, args in (("amd-smi", ["list", "--json"]), ("rocm-smi", ["--json"])):
        path = shutil.which(tool)
        if not path:
            continue
        try:
            out = subprocess.run(
                [path, *args], capture_output=True, text=True, timeout=30
            )
            ok = out.returncode == 0
            raw: Any = out.stdout.strip()
            try:
                raw = json.loads(raw)
            except (ValueError, TypeError):
                pass
            return {"tool": tool, "ok": ok, "raw": raw}
        except (subprocess.TimeoutExpired, OSError) as exc:
            return {"tool": tool, "ok": False, "raw": str(exc)}
    return {"tool": None, "ok": False, "raw": "no amd-smi/rocm-smi found"}


def gpu_health_check(
    device: int = 0,
    *,
    bw_buf_mib: float = 512.0,
    bw_iters: int = 5,
    require_gpu: bool = False,
    deep: bool = False,
    coverage: bool = False,
    memory: bool = False,
    memory_mib: float = 4096.0,
    mx: bool = False,
    fabric: bool = False,
    lds: bool = False,
    hostlink: bool = False,
    hostlink_mib: float = 64.0,
    valu: bool = False,
) -> Dict[str, Any]:
    """Full node GPU health check.  Returns a report dict with a top-level
    ``healthy`` verdict; raises GpuHealthError when ``require_gpu`` and no
    usable GPU/native validator is present.  ``coverage`` adds the
    whole-device per-CU sweep (see :mod:`.cu_coverage`) and gates the verdict
    on it.  ``memory`` adds the HBM pattern test over ``memory_mib`` MiB
    (``0``: all free memory; see :mod:`.hbm_integrity`) and gates on it too.
    ``mx`` adds the whole-device sweep of the MX block-scaled matrix path and
    its e2m1 / e4m3 burn-in (see :mod:`.mx_matrix`); the verdict is gated on
    the sweep and on each throughput reaching ``MFMA_MIN_TFLOPS``.  ``fabric``
    adds the cross-XCD hand-off and device-scope atomics check (see
    :mod:`.xcd_fabric`) and gates on it.  ``lds`` adds the LDS data-integrity
    check over all 160 KiB of every CU (see :mod:`.lds_integrity`) and gates on
    it.  ``hostlink`` adds the host-link data-integrity check with
    ``hostlink_mib`` MiB per buffer (DMA copies, zero-copy access and
    system-scope atomics on host memory; see :mod:`.host_link`) and gates on it
    as well.  ``valu`` adds the whole-device vector-ALU sweep (exact
    arithmetic, conversions and cross-lane ops, transcendentals by consensus;
    see :mod:`.valu_check`) and gates on it."""
    report: Dict[str, Any] = {"healthy": False, "checks": {}}
    report["checks"]["smi"] = smi_probe()

    native = load_native_validator()
    if native is None:
        if require_gpu:
            raise GpuHealthError("no native GPU validator available")
        report["reason"] = "no GPU present; native checks skipped"
        return report

    probe = native.device_probe(device)
    report["checks"]["device"] = probe
    arch_ok = "gfx950" in probe.get("gcn_arch", "")
    report["checks"]["arch_ok"] = arch_ok

    mfma_f32_err = native.mfma_f32_check(device)
    mfma_bf16_err = native.mfma_bf16_check(device)
    report["checks"]["mfma_f32_max_err"] = mfma_f32_err
    report["checks"]["mfma_bf16_max_err"] = mfma_bf16_err

    bw = native.hbm_bandwidth_gbps(device, bw_buf_mib, bw_iters)
    report["checks"]["hbm_bandwidth_gbps"] = bw

    lds_ok = native.lds_roundtrip_check(device)
    report["checks"]["lds_ok"] = lds_ok

    deep_ok = True
    if deep:
        # deep mode: fp8 matrix path + sustained matrix-core burn-in
        fp8_err = native.mfma_fp8_check(device)
        tflops = native.mfma_throughput_tflops(device, 100000)
        report["checks"]["mfma_fp8_max_err"] = fp8_err
        report["checks"]["mfma_throughput_tflops"] = tflops
        deep_ok = fp8_err <= MFMA_FP8_MAX_ERR and tflops >= MFMA_MIN_TFLOPS

    coverage_ok = True
    if coverage:
        # opt-in: MFMA + LDS on every CU and SIMD, attributed per unit
        from .cu_coverage import summarize_cu_coverage

        summary = summarize_cu_coverage(native.cu_coverage_check(device))
        report["checks"]["cu_coverage"] = summary
        coverage_ok = summary["healthy"]

    memory_ok = True
    if memory:
        # opt-in: moving-inversions pattern test, summary without raw records
        from .hbm_integrity import mib_to_bytes, summarize_hbm_integrity

        mem = summarize_hbm_integrity(
            native.hbm_pattern_check(device, mib_to_bytes(memory_mib))
        )
        report["checks"]["hbm_integrity"] = mem
        memory_ok = mem["healthy"]

    mx_ok = True
    if mx:
        # opt-in: MX block-scaled MFMA on every CU and SIMD + MX burn-in.  The
        # floor is the bf16 one: an MX path slower than bf16 is broken
        # whatever its true peak is
        from .mx_matrix import (
            THROUGHPUT_FORMATS,
            THROUGHPUT_ITERS,
            summarize_mx_matrix,
        )

        mx_summary = summarize_mx_matrix(native.mx_coverage_check(device))
        mx_summary["throughput_tflops"] = {
            fmt: native.mx_throughput_tflops(device, fmt, THROUGHPUT_ITERS)
            for fmt in THROUGHPUT_FORMATS
        }
        report["checks"]["mx_matrix"] = mx_summary
        mx_ok = mx_summary["healthy"] and all(
            tf >= MFMA_MIN_TFLOPS
            for tf in mx_summary["throughput_tflops"].values()
        )

    fabric_ok = True
    if fabric:
        # opt-in: agent-scope release/acquire hand-offs between XCDs and
        # device-scope atomics, summary without raw records
        from .xcd_fabric import summarize_xcd_fabric

        fab = summarize_xcd_fabric(native.xcd_fabric_check(device))
        report["checks"]["xcd_fabric"] = fab
        fabric_ok = fab["healthy"]

    lds_integrity_ok = True
    if lds:
        # opt-in: all 160 KiB of LDS on every CU, summary without raw units or
        # records
        from .lds_integrity import summarize_lds_integrity

        lds_summary = summarize_lds_integrity(native.lds_integrity_check(device))
        report["checks"]["lds_integrity"] = lds_summary
        lds_integrity_ok = lds_summary["healthy"]

    host_link_ok = True
    if hostlink:
        # opt-in: what crosses the host link compared exactly, summary without
        # raw records
        from .hbm_integrity import mib_to_bytes
        from .host_link import summarize_host_link

        link = summarize_host_link(
            native.host_link_check(device, mib_to_bytes(hostlink_mib))
        )
        report["checks"]["host_link"] = link
        host_link_ok = link["healthy"]

    valu_ok = True
    if valu:
        # opt-in: the vector ALU on every CU and SIMD, summary without raw
        # units or records
        from .valu_check import summarize_valu

        valu_summary = summarize_valu(native.valu_coverage_check(device))
        report["checks"]["valu"] = valu_summary
        valu_ok = valu_summary["healthy"]

    # multi-GPU nodes: verify every xGMI peer link is up
    xgmi_ok = True
    if probe.get("device_count", 1) > 1:
        links = native.xgmi_p2p_probe(device, 64.0, 3)
        report["checks"]["xgmi_links"] = [dict(l) for l in links]
        xgmi_ok = all(l.get("accessible") for l in links)
    report["checks"]["xgmi_ok"] = xgmi_ok

    report["healthy"] = bool(
        arch_ok
        and mfma_f32_err <= MFMA_F32_MAX_ERR
        and mfma_bf16_err <= MFMA_BF16_MAX_ERR
        and bw >= HBM_MIN_GBPS
        and lds_ok
        and xgmi_ok
        and deep_ok
        and coverage_ok
        and memory_ok
        and mx_ok
        and fabric_ok
        and lds_integrity_ok
        and host_link_ok
        and valu_ok
    )
    return report


def main() -> int:
    """CLI entry point for use inside a validation pod.  Pass ``--deep`` for
    the fp8 + burn-in checks, ``--coverage`` for the per-CU sweep and
    ``--memory`` for the HBM pattern test (``--memory-mib=N`` sets its size
    and implies it; ``N=0`` means all free memory) and ``--mx`` for the MX
    block-scaled matrix sweep and burn-in, ``--fabric`` for the cross-XCD
    hand-off and atomics check, ``--lds`` for the LDS data-integrity check and
    ``--hostlink`` for the host-link data-integrity check (``--hostlink-mib=N``
    sets its buffer size and implies it) and ``--valu`` for the vector-ALU
    sweep."""
    import sys

    sized_kw: Dict[str, Any] = {}
    for arg in sys.argv[1:]:
        if arg == "--memory":
            sized_kw["memory"] = True
        elif arg.startswith("--memory-mib="):
            sized_kw["memory"] = True
            sized_kw["memory_mib"] = float(arg.split("=", 1)[1])
        elif arg == "--hostlink":
            sized_kw["hostlink"] = True
        elif arg.startswith("--hostlink-mib="):
            sized_kw["hostlink"] = True
            sized_kw["hostlink_mib"] = float(arg.split("=", 1)[1])
    report = gpu_health_check(
        require_gpu=True,
        deep="--deep" in sys.argv,
        coverage="--coverage" in sys.argv,
        mx="--mx" in sys.argv,
        fabric="--fabric" in sys.argv,
        lds="--lds" in sys.argv,
        valu="--valu" in sys.argv,
        **sized_kw,
    )
    print(json.dumps(report, indent=2, default=str))  # noqa: T201 (CLI/build output)
    return 0 if report["healthy"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
