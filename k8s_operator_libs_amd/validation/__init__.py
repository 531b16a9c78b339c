"""AMD GPU node health validation.

The AMD-native replacement for the NVML-based validator pods the reference
orchestrates: after a driver bump, a validation pod on each MI355X node runs
:func:`gpu_health_check` and reports Ready only when the GPU stack is sane.
The upgrade state machine's ValidationManager gates uncordon on that
readiness (BASELINE.json north_star).

Layers:
- :func:`smi_probe` — amd-smi / rocm-smi process-level probe (driver loaded,
  devices enumerated);
- the native ``_gpu_validator`` HIP extension — device probe, MFMA matrix
  core smoke tests (f32-exact and bf16), HBM streaming bandwidth, LDS
  integrity.  **Fails loudly if the extension is missing on a GPU machine**:
  a silent fallback would let a broken driver pass validation;
- :func:`cu_coverage_check` — opt-in whole-device sweep: the f32 / bf16 / fp8
  matrix paths and LDS on every CU and SIMD, with failures attributed to the
  unit that produced them (:func:`summarize_cu_coverage` is the pure verdict);
- :func:`hbm_integrity_check` — opt-in moving-inversions pattern test over a
  region of HBM: exact comparison, coverage counted, failing words recorded
  (:func:`summarize_hbm_integrity` is the pure verdict);
- :func:`mx_matrix_check` — opt-in whole-device sweep of the MX block-scaled
  matrix path (``v_mfma_scale_f32_*_f8f6f4``: e4m3, e5m2, e2m3, e3m2 and e2m1
  operands with E8M0 block scales, both shapes, mixed pairs), bit-exact, with
  failures attributed per unit (:func:`summarize_mx_matrix` is the pure
  verdict);
- :func:`xcd_fabric_check` — opt-in cross-XCD check: wait-free last-arriver
  hand-offs (agent-scope release, ticket, acquire) between workgroups on
  different XCDs and a device-scope atomics sweep, exact, coverage counted,
  failures attributed per (writer, reader) XCC pair
  (:func:`summarize_xcd_fabric` is the pure verdict);
- :func:`lds_integrity_check` — opt-in LDS data-integrity check: all 160 KiB
  of every CU through moving inversions in ``b32`` / ``b64`` / ``b128``,
  sub-word stores, ``ds_read_b64_tr_b16``, direct global->LDS loads, the LDS
  atomic ALU and the permute crossbar, exact, coverage counted, failures
  attributed per CU, word and bank (:func:`summarize_lds_integrity` is the
  pure verdict);
- :func:`host_link_check` — opt-in host-link data-integrity check: DMA copies
  in both directions, zero-copy kernel access, duplex and unaligned copies on
  pinned, registered and pageable host memory and system-scope atomics on
  pinned memory, exact, coverage counted, failing words and copy cases
  recorded (:func:`summarize_host_link` is the pure verdict);
- :func:`valu_check` — opt-in whole-device sweep of the vector ALU: f32 / f64 /
  f16 arithmetic, integer and bit ops, conversions (f16, bf16, fp8, bf8, fp4)
  and cross-lane ops bit-exact against a host reference, raw transcendentals
  by consensus of all SIMDs, every compare counted, failures attributed per
  unit and instruction (:func:`summarize_valu` is the pure verdict).
"""

from .gpu_health import (  # noqa: F401
    GpuHealthError,
    gpu_health_check,
    load_native_validator,
    smi_probe,
)
from .cu_coverage import (  # noqa: F401
    cu_coverage_check,
    summarize_cu_coverage,
)
from .hbm_integrity import (  # noqa: F401
    hbm_integrity_check,
    summarize_hbm_integrity,
)
from .host_link import (  # noqa: F401
    host_link_check,
    summarize_host_link,
)
from .lds_integrity import (  # noqa: F401
    lds_integrity_check,
    summarize_lds_integrity,
)
from .mx_matrix import (  # noqa: F401
    mx_matrix_check,
    summarize_mx_matrix,
)
from .valu_check import (  # noqa: F401
    summarize_valu,
    valu_check,
)
from .xcd_fabric import (  # noqa: F401
    summarize_xcd_fabric,
    xcd_fabric_check,
)
