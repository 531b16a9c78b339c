// gpu_validator.hip — native MI355X (gfx950) node health validator.
//
// AMD-native replacement for the NVML-based validation pods the reference
// orchestrates ("validation pods run amd-smi/rocm-smi health
// checks instead of NVML validators").  A validation pod on an MI355X node
// runs these checks after a driver bump; the ValidationManager gates
// uncordon on the pod reporting Ready.
//
// Checks:
//   device_probe()        — device properties (arch, CUs, LDS, HBM)
//   mfma_f32_check()      — v_mfma_f32_16x16x4_f32 tile vs exact CPU fmaf
//                           chain (matrix cores, exact f32 numerics)
//   mfma_bf16_check()     — v_mfma_f32_16x16x32_bf16 tile vs CPU reference
//                           (the production-dtype matrix path)
//   mfma_fp8_check()      — v_mfma_f32_16x16x32_fp8_fp8 (OCP e4m3) tile
//   mfma_throughput_tflops() — sustained bf16 matrix-core burn-in
//   hbm_bandwidth_gbps()  — nontemporal streaming copy (sweep-tuned, ~6 TB/s)
//   lds_roundtrip_check() — LDS store/load/barrier integrity
//   xgmi_p2p_probe()      — peer reachability + p2p bandwidth per xGMI link
//   cu_coverage_check()   — f32/bf16/fp8 MFMA + LDS on every CU and SIMD,
//                           exact, attributed per unit (opt-in sweep)
//   hbm_pattern_check()   — moving-inversions pattern test over a region of
//                           HBM, exact, failing words recorded (opt-in)
//   mx_coverage_check()   — the MX block-scaled path (v_mfma_scale_f32_*_f8f6f4:
//                           e4m3, e5m2, e2m3, e3m2, e2m1 with E8M0 scales, both
//                           shapes, mixed pairs) on every CU and SIMD, exact,
//                           attributed per unit (opt-in sweep)
//   mx_mfma_tile()        — one scaled MFMA, raw codes + GPU tile returned
//   mx_throughput_tflops() — sustained e2m1 / e4m3 MX burn-in
//   xcd_fabric_check()    — hand-offs between workgroups on different XCDs
//                           (agent-scope release, ticket, acquire) and every
//                           device-scope atomic, exact, attributed per
//                           (writer, reader) XCC pair (opt-in)
//   lds_integrity_check() — all 160 KiB of LDS on every CU: moving inversions
//                           in b32 / b64 / b128, byte and 16-bit stores,
//                           ds_read_b64_tr_b16, direct global->LDS loads, LDS
//                           atomics and ds_bpermute / ds_permute, exact,
//                           attributed per CU and word (opt-in)
//   lds_tr_tile()         — one ds_read_b64_tr_b16, raw elements returned
//   valu_coverage_check() — the vector ALU on every CU and SIMD: f32 / f64 /
//                           f16 arithmetic, integer, conversions (bf16, fp8,
//                           bf8, fp4) and cross-lane ops bit-exact against a
//                           host reference, transcendentals by consensus of
//                           all SIMDs, compares counted (opt-in sweep)
//   valu_probe()          — one vector instruction on one wave, raw results
//   host_link_check()     — what crosses the host link: DMA copies both ways,
//                           zero-copy kernel access, duplex and unaligned
//                           copies, system-scope atomics on pinned, registered
//                           and pageable host memory, exact, failing words and
//                           copy cases recorded (opt-in)
//
// This file holds the kernels, the HIP host drivers, the py::dict conversion
// and the module table.  Device memory and events are owned by the holders in
// hip_util.hpp (DeviceBuf<T>, HostBuf, RegisteredBuf, Stream, EventTimer);
// the capped mismatch log of the checks is record_log.hpp, the bounded
// relaunch of a whole-device sweep and its unit dicts are sweep.hpp, and the
// tally of what a launch left behind is plain C++ next to the problems;
// the exact problems the checks run (operands, codecs, packed tables, expected results, and the records and
// constants shared with the kernels) are plain C++ in validator_problems.hpp.
//
// Built standalone with hipcc (no torch linkage) via pybind11; the .so lives
// in-tree so it travels to GPU nodes with the package.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cmath>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "hip_util.hpp"
#include "record_log.hpp"
#include "sweep.hpp"
#include "validator_problems.hpp"

namespace py = pybind11;

// ---------------------------------------------------------------------------
// MFMA f32 smoke: one wave computes D = A·B + C for a 16x16 tile, K=4,
// using v_mfma_f32_16x16x4_f32.  Lane layout (cdna_hip_programming.md §3):
//   A operand: lane l supplies A[l&15][l>>4]        (one f32)
//   B operand: lane l supplies B[l>>4][l&15]        (one f32)
//   C/D:       lane l, reg r -> row=(l>>4)*4+r, col=l&15
// ---------------------------------------------------------------------------

using f32x4 = __attribute__((ext_vector_type(4))) float;

__global__ void mfma_f32_16x16x4_kernel(const float* __restrict__ A,
                                        const float* __restrict__ B,
                                        float* __restrict__ D) {
#if defined(__gfx950__)
  int lane = threadIdx.x;   // one wave of 64
  float a = A[(lane & 15) * 4 + (lane >> 4)];   // A is 16x4 row-major
  float b = B[(lane >> 4) * 16 + (lane & 15)];  // B is 4x16 row-major
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  for (int r = 0; r < 4; ++r) {
    int row = (lane >> 4) * 4 + r;
    int col = lane & 15;
    D[row * 16 + col] = c[r];
  }
#endif
}

// ---------------------------------------------------------------------------
// MFMA bf16 smoke: v_mfma_f32_16x16x32_bf16, one wave, D = A·B.
// Per cdna_hip_programming.md §3 each lane holds 8 bf16 of A and B (4 VGPRs)
// and 4 f32 of C/D; C/D layout is dtype-independent (row=(l>>4)*4+r,
// col=l&15).  A (16x32): lane l supplies A[l&15][(l>>4)*8 + i];
// B (32x16): lane l supplies B[(l>>4)*8 + i][l&15].
// ---------------------------------------------------------------------------

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

__global__ void mfma_bf16_16x16x32_kernel(const __bf16* __restrict__ A,
                                          const __bf16* __restrict__ B,
                                          float* __restrict__ D) {
#if defined(__gfx950__)
  int lane = threadIdx.x;
  bf16x8 a, b;
  for (int i = 0; i < 8; ++i) {
    int k = (lane >> 4) * 8 + i;
    a[i] = A[(lane & 15) * 32 + k];   // A is 16x32 row-major
    b[i] = B[k * 16 + (lane & 15)];   // B is 32x16 row-major
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  for (int r = 0; r < 4; ++r) {
    int row = (lane >> 4) * 4 + r;
    int col = lane & 15;
    D[row * 16 + col] = c[r];
  }
#endif
}

// ---------------------------------------------------------------------------
// MFMA fp8 (OCP e4m3fn) smoke: v_mfma_f32_16x16x32_fp8_fp8, one wave.
// Same fragment geometry as the bf16 K=32 shape (8 elements per lane,
// packed into one i64 operand; C/D layout is dtype-independent).
// Validates the fp8 matrix path the serving stack depends on.
// ---------------------------------------------------------------------------

__global__ void mfma_fp8_16x16x32_kernel(const uint8_t* __restrict__ A,
                                         const uint8_t* __restrict__ B,
                                         float* __restrict__ D) {
#if defined(__gfx950__)
  int lane = threadIdx.x;
  uint64_t a = 0, b = 0;
  for (int i = 0; i < 8; ++i) {
    int k = (lane >> 4) * 8 + i;
    a |= (uint64_t)A[(lane & 15) * 32 + k] << (8 * i);  // A is 16x32
    b |= (uint64_t)B[k * 16 + (lane & 15)] << (8 * i);  // B is 32x16
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((long)a, (long)b, c, 0, 0, 0);
  for (int r = 0; r < 4; ++r) {
    D[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = c[r];
  }
#endif
}

// ---------------------------------------------------------------------------
// Matrix-core throughput burn-in: sustained back-to-back
// v_mfma_f32_16x16x32_bf16 with 4 independent accumulators per wave
// (the guide's issue-rate recipe: >=2 independent accumulators reach the
// issue rate; floor throughput ~2075 TF on bf16).  Catches down-clocked,
// power-capped or partially-fused parts that pass the numerics smoke.
// ---------------------------------------------------------------------------

__global__ void mfma_burn_kernel(const __bf16* __restrict__ seed,
                                 float* __restrict__ out, int iters) {
#if defined(__gfx950__)
  int lane = threadIdx.x & 63;
  bf16x8 a, b;
  for (int i = 0; i < 8; ++i) {
    a[i] = seed[(lane * 8 + i) & 255];
    b[i] = seed[(lane * 8 + i + 128) & 255];
  }
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  f32x4 acc2 = {0, 0, 0, 0}, acc3 = {0, 0, 0, 0};
  for (int i = 0; i < iters; ++i) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc1, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc2, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc3, 0, 0, 0);
  }
  float sink = acc0[0] + acc1[1] + acc2[2] + acc3[3];
  size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  out[tid] = sink;  // keep the loop alive
#endif
}

static double mfma_throughput_tflops(int device, int iters) {
  HIP_CHECK(hipSetDevice(device));
  const std::vector<uint16_t> hseed = bf16_burn_seed();
  const int block = 256, grid = 1024;  // 4096 waves = 4 per SIMD
  DeviceBuf<uint16_t> dseed(hseed.size());
  DeviceBuf<float> dout((size_t)block * grid);
  dseed.upload(hseed.data(), hseed.size());
  auto launch = [&](int n) {
    hipLaunchKernelGGL(mfma_burn_kernel, dim3(grid), dim3(block), 0, 0,
                       (const __bf16*)dseed.get(), dout.get(), n);
  };
  launch(1000);  // warmup
  HIP_CHECK(hipDeviceSynchronize());
  EventTimer timer;
  const float ms = timer.time_ms([&] { launch(iters); });
  const double waves = (double)grid * block / 64.0;
  const double flop = waves * (double)iters * 4.0 * (16.0 * 16.0 * 32.0 * 2.0);
  return flop / 1e12 / ((double)ms / 1e3);
}

// ---------------------------------------------------------------------------
// HBM streaming-copy bandwidth.  Tuned via experiments/bw_sweep.hip on
// MI355X: nontemporal 16-byte loads/stores (bypass-cache streaming hints),
// 2x unrolled grid-stride, block=512, grid up to 131072 -> 6.0 TB/s
// (95% of the 6.29 TB/s measured float4-copy ceiling,
// MI355X_MICROARCH.md) vs 4.6 TB/s for a plain 256x8192 grid-stride copy.
// ---------------------------------------------------------------------------

typedef float vfloat4 __attribute__((ext_vector_type(4)));

__global__ void bw_copy_kernel(const float4* __restrict__ src4,
                               float4* __restrict__ dst4, size_t n) {
  const vfloat4* __restrict__ src = reinterpret_cast<const vfloat4*>(src4);
  vfloat4* __restrict__ dst = reinterpret_cast<vfloat4*>(dst4);
  size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + stride < n; i += 2 * stride) {
    vfloat4 a = __builtin_nontemporal_load(&src[i]);
    vfloat4 b = __builtin_nontemporal_load(&src[i + stride]);
    __builtin_nontemporal_store(a, &dst[i]);
    __builtin_nontemporal_store(b, &dst[i + stride]);
  }
  for (; i < n; i += stride) dst[i] = src[i];
}

// ---------------------------------------------------------------------------
// LDS integrity: stage a block through LDS with a permutation and read back.
// ---------------------------------------------------------------------------

__global__ void lds_roundtrip_kernel(const float* __restrict__ in,
                                     float* __restrict__ out, int n) {
  __shared__ float lds[1024];
  int tid = threadIdx.x;
  int base = blockIdx.x * 1024;
  for (int i = tid; i < 1024; i += blockDim.x) {
    lds[(i * 5 + 7) & 1023] = in[base + i] * 2.0f;
  }
  __syncthreads();
  for (int i = tid; i < 1024; i += blockDim.x) {
    out[base + i] = lds[(i * 5 + 7) & 1023];
  }
  (void)n;
}

// ---------------------------------------------------------------------------
// Host-side checks
// ---------------------------------------------------------------------------

static py::dict device_probe(int device) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  py::dict d;
  d["name"] = std::string(prop.name);
  d["gcn_arch"] = std::string(prop.gcnArchName);
  d["compute_units"] = prop.multiProcessorCount;
  d["lds_per_block_kb"] = (int)(prop.sharedMemPerBlock / 1024);
  d["hbm_total_gb"] = (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0);
  d["clock_mhz"] = prop.clockRate / 1000;
  d["warp_size"] = prop.warpSize;
  int count = 0;
  HIP_CHECK(hipGetDeviceCount(&count));
  d["device_count"] = count;
  return d;
}

// One wave runs one of the three smoke kernels on a 16xK by Kx16 problem and
// returns the 16x16 tile.  T is the host type of an encoded element, KT the
// type the kernel reads it as.
template <typename T, typename KT>
static std::vector<float> run_single_wave_tile(
    const std::vector<T>& a, const std::vector<T>& b,
    void (*kernel)(const KT*, const KT*, float*)) {
  static_assert(sizeof(T) == sizeof(KT), "encoded element size");
  DeviceBuf<T> dA(a.size()), dB(b.size());
  DeviceBuf<float> dD(16 * 16);
  dA.upload(a.data(), a.size());
  dB.upload(b.data(), b.size());
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, 0,
                     reinterpret_cast<const KT*>(dA.get()),
                     reinterpret_cast<const KT*>(dB.get()), dD.get());
  HIP_CHECK(hipGetLastError());
  std::vector<float> d(dD.size());
  dD.download(d.data(), d.size());
  return d;
}

static double mfma_f32_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const SmokeTile<float> t = smoke_f32_problem();
  return max_abs_err(
      run_single_wave_tile(t.a_enc, t.b_enc, mfma_f32_16x16x4_kernel), t.ref);
}

static double mfma_bf16_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const SmokeTile<uint16_t> t = smoke_bf16_problem();
  return max_abs_err(
      run_single_wave_tile(t.a_enc, t.b_enc, mfma_bf16_16x16x32_kernel), t.ref);
}

static double mfma_fp8_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const SmokeTile<uint8_t> t = smoke_fp8_problem();
  return max_abs_err(
      run_single_wave_tile(t.a_enc, t.b_enc, mfma_fp8_16x16x32_kernel), t.ref);
}

static py::dict mfma_bf16_tile(int device) {
  // Run the bf16 MFMA tile and return decoded inputs + GPU output so Python
  // tests can verify against an independent fp32 reference (e.g. torch).
  HIP_CHECK(hipSetDevice(device));
  const SmokeTile<uint16_t> t = smoke_bf16_tile_problem();
  py::dict out;
  out["m"] = 16;
  out["n"] = 16;
  out["k"] = t.k;
  out["a"] = t.a_dec;  // bf16-quantized values as f32, row-major MxK
  out["b"] = t.b_dec;  // row-major KxN
  // GPU MFMA result, row-major MxN
  out["d"] = run_single_wave_tile(t.a_enc, t.b_enc, mfma_bf16_16x16x32_kernel);
  return out;
}

static double hbm_bandwidth_gbps(int device, double buf_mib, int iters) {
  HIP_CHECK(hipSetDevice(device));
  size_t bytes = (size_t)(buf_mib * 1024.0 * 1024.0);
  size_t n = bytes / sizeof(float4);
  bytes = n * sizeof(float4);
  DeviceBuf<float4> src(n), dst(n);
  src.fill(1);
  // sweep-tuned launch shape (see header comment): block 512, grid scaled to
  // ~2 float4 per thread, capped at the sweep's best 131072
  int block = 512;
  long want = (long)(n / (2 * (size_t)block)) + 1;
  int grid = (int)std::min<long>(131072, std::max<long>(1024, want));
  auto launch = [&] {
    hipLaunchKernelGGL(bw_copy_kernel, dim3(grid), dim3(block), 0, 0, src.get(),
                       dst.get(), n);
  };
  EventTimer timer;
  launch();  // warmup
  HIP_CHECK(hipDeviceSynchronize());
  const float ms = timer.time_ms([&] {
    for (int i = 0; i < iters; ++i) launch();
  });
  // read + write
  double gb = 2.0 * (double)bytes * iters / 1e9;
  return gb / ((double)ms / 1e3);
}

static bool lds_roundtrip_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const int blocks = 512, n = blocks * 1024;
  std::vector<float> hin(n), hout(n);
  for (int i = 0; i < n; ++i) hin[i] = (float)(i % 977) * 0.5f;
  DeviceBuf<float> din(n), dout(n);
  din.upload(hin.data(), n);
  hipLaunchKernelGGL(lds_roundtrip_kernel, dim3(blocks), dim3(256), 0, 0,
                     din.get(), dout.get(), n);
  HIP_CHECK(hipGetLastError());
  dout.download(hout.data(), n);
  for (int i = 0; i < n; ++i)
    if (hout[i] != hin[i] * 2.0f) return false;
  return true;
}

// ---------------------------------------------------------------------------
// xGMI peer-to-peer probe: on multi-GPU nodes check that every peer of
// `device` is reachable and measure the p2p copy bandwidth over the xGMI
// links (7 point-to-point links x ~153 GB/s per MI355X GPU).  The AMD-native
// analogue of the reference's OFED/NIC validation surface.
// ---------------------------------------------------------------------------

static py::list xgmi_p2p_probe(int device, double buf_mib, int iters) {
  py::list out;
  int count = 0;
  HIP_CHECK(hipGetDeviceCount(&count));
  size_t bytes = (size_t)(buf_mib * 1024.0 * 1024.0);
  for (int peer = 0; peer < count; ++peer) {
    if (peer == device) continue;
    py::dict entry;
    entry["peer"] = peer;
    int can = 0;
    HIP_CHECK(hipDeviceCanAccessPeer(&can, device, peer));
    entry["accessible"] = (bool)can;
    if (!can) {
      out.append(entry);
      continue;
    }
    HIP_CHECK(hipSetDevice(device));
    hipError_t en = hipDeviceEnablePeerAccess(peer, 0);
    if (en != hipSuccess && en != hipErrorPeerAccessAlreadyEnabled) {
      entry["error"] = std::string(hipGetErrorString(en));
      out.append(entry);
      continue;
    }
    // dst lives on the peer: it is freed below while the peer is selected.
    // Only when something throws does its destructor free it under whichever
    // device is current.
    DeviceBuf<uint8_t> dst;
    {
      HIP_CHECK(hipSetDevice(device));
      DeviceBuf<uint8_t> src(bytes);
      src.fill(1);
      HIP_CHECK(hipSetDevice(peer));
      dst = DeviceBuf<uint8_t>(bytes);
      HIP_CHECK(hipSetDevice(device));
      EventTimer timer;
      auto copy = [&] {
        HIP_CHECK(hipMemcpyPeer(dst.get(), peer, src.get(), device, bytes));
      };
      copy();  // warmup
      HIP_CHECK(hipDeviceSynchronize());
      const float ms = timer.time_ms([&] {
        for (int i = 0; i < iters; ++i) copy();
      });
      entry["bandwidth_gbps"] = ((double)bytes * iters / 1e9) / ((double)ms / 1e3);
    }
    HIP_CHECK(hipSetDevice(peer));
    dst.reset();
    HIP_CHECK(hipSetDevice(device));
    out.append(entry);
  }
  return out;
}


// ---------------------------------------------------------------------------
// Per-CU coverage sweep.  The single-wave MFMA smokes above exercise one
// matrix pipe of 1024; this sweep runs the f32 / bf16 / fp8 tiles and an LDS
// round trip in every wave of a grid sized to fill the device, and records
// the result per (XCC, CU, SIMD) as the wave itself reads its placement from
// HW_REG_HW_ID / HW_REG_XCC_ID.
//
// Operands are small integers (|v| <= 8, exact in f32, bf16 and e4m3), so
// every K=32 dot product is an integer <= 2048 and exact in f32 in any
// summation order: the comparison is bitwise, with no tolerance.
//
// Placement key (opaque; the field names are labels for humans only):
//   key  = XCC_ID[3:0] << 8 | HW_ID[15:8]     (gfx9: cu[11:8] sh[12] se[15:13])
//   simd = HW_ID[5:4]
//   slot = key * 4 + simd                      -> 4096 * 4 = 16384 slots
// The bit layout is an assumption; the host validates it by outcome (distinct
// keys == multiProcessorCount, distinct slots == 4x that), never by trust.
//
// Every workgroup does a fixed amount of work and exits: no spins, no grid
// barrier, no co-residency requirement.  The 64 KiB LDS claim caps a CU at
// two workgroups (160 KiB / 64 KiB), so a grid of 2 x CUs that outlives the
// launch skew is co-resident and lands two workgroups on every CU.  That only
// makes one round the normal case; the host relaunches (bounded) otherwise.
// ---------------------------------------------------------------------------

constexpr unsigned kCovFailF32 = 1u, kCovFailBf16 = 2u, kCovFailFp8 = 4u,
                   kCovFailLds = 8u;

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

// second bound = waves per SIMD: two workgroups must fit on one CU
__global__ void __launch_bounds__(kCovBlock, kCovBlocksPerCu)
cu_coverage_kernel(const uint32_t* tab, uint32_t* __restrict__ slot_waves,
                   uint32_t* __restrict__ slot_fail,
                   uint32_t* __restrict__ slot_hw_id,
                   uint32_t* __restrict__ slot_xcc_id, int reps, int poison_key,
                   unsigned poison_mask, int poison_all) {
#if defined(__gfx950__)
  __shared__ uint32_t lds[kCovLdsWords];
  const uint32_t hw_id = __builtin_amdgcn_s_getreg(kCovHwRegHwId);
  const uint32_t xcc_id = __builtin_amdgcn_s_getreg(kCovHwRegXccId);
  const uint32_t key = ((xcc_id & 0xFu) << 8) | ((hw_id >> 8) & 0xFFu);
  const uint32_t simd = (hw_id >> 4) & 3u;

  // test hook: data only, flips one bit of the *expected* values
  const unsigned pm = (poison_all || (int)key == poison_key) ? poison_mask : 0u;
  const uint32_t px[3] = {(pm >> 0) & 1u, (pm >> 1) & 1u, (pm >> 2) & 1u};
  const uint32_t px_lds = (pm >> 3) & 1u;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  unsigned fail = 0;

  for (int rep = 0; rep < reps; ++rep) {
#pragma unroll 1
    for (int s = 0; s < kCovSets; ++s) {
      // volatile: operands and expected values are re-read from global memory
      // every repetition, so neither the MFMAs nor the compares can be hoisted
      const volatile uint32_t* p = tab + (size_t)(s * 64 + lane) * kCovRecWords;
      const float fa = __uint_as_float(p[0]);
      const float fb = __uint_as_float(p[1]);
      u32x4 ba, bb;
      for (int i = 0; i < 4; ++i) {
        ba[i] = p[2 + i];
        bb[i] = p[6 + i];
      }
      const uint64_t qa = (uint64_t)p[10] | ((uint64_t)p[11] << 32);
      const uint64_t qb = (uint64_t)p[12] | ((uint64_t)p[13] << 32);

      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      f32x4 d[3];
      d[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, fb, zero, 0, 0, 0);
      d[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          __builtin_bit_cast(bf16x8, ba), __builtin_bit_cast(bf16x8, bb), zero,
          0, 0, 0);
      d[2] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((long)qa, (long)qb,
                                                        zero, 0, 0, 0);
      for (int t = 0; t < 3; ++t)
        for (int r = 0; r < 4; ++r) {
          const uint32_t want = p[14 + t * 4 + r] ^ px[t];
          if (__float_as_uint(d[t][r]) != want) fail |= 1u << t;
        }
    }

    // LDS: permuted write, barrier, read back words another wave wrote
    const uint32_t seed =
        (uint32_t)rep * 0x9E3779B9u + (uint32_t)blockIdx.x * 0x85EBCA6Bu;
#pragma unroll 4
    for (int i = tid; i < kCovLdsWords; i += kCovBlock)
      lds[(i * 5 + 7) & (kCovLdsWords - 1)] = ((uint32_t)i * 2654435761u) ^ seed;
    __syncthreads();
#pragma unroll 4
    for (int i = tid; i < kCovLdsWords; i += kCovBlock) {
      const int j = kCovLdsWords - 1 - i;  // written by thread 255 - tid
      const uint32_t want = (((uint32_t)j * 2654435761u) ^ seed) ^ px_lds;
      if (lds[(j * 5 + 7) & (kCovLdsWords - 1)] != want) fail |= kCovFailLds;
    }
    __syncthreads();
  }

  // wave-wide OR of the per-lane masks, then one lane records the wave
  unsigned wave_fail = 0;
  for (int b = 0; b < 4; ++b)
    if (__ballot((fail >> b) & 1u) != 0) wave_fail |= 1u << b;
  if (lane == 0) {
    const uint32_t slot = key * 4u + simd;  // < kCovSlots by the masks above
    atomicAdd(&slot_waves[slot], 1u);
    if (wave_fail) atomicOr(&slot_fail[slot], wave_fail);
    slot_hw_id[slot] = hw_id;    // raw registers, kept as evidence should the
    slot_xcc_id[slot] = xcc_id;  // layout assumption ever fail its check
  }
#endif
}

static py::dict cu_coverage_reference() {
  // host only: no HIP call
  py::dict out;
  out["sets"] = kCovSets;
  out["m"] = 16;
  out["n"] = 16;
  for (int t = 0; t < 3; ++t) {
    py::list per_set;
    for (int s = 0; s < kCovSets; ++s) {
      CovProblem p = cov_problem(s, t);
      py::dict e;
      e["k"] = p.k;
      e["a"] = p.a_dec;  // decoded from the encoded operand, row-major 16xK
      e["b"] = p.b_dec;  // row-major Kx16
      e["d"] = p.d;      // expected tile, row-major 16x16
      per_set.append(e);
    }
    out[kCovDtypeNames[t]] = per_set;
  }
  return out;
}

// The host side of cu_coverage_check and mx_coverage_check, whose kernels take
// the same arguments: validation before the first HIP call, then the sweep.
using CovSweepKernel = void (*)(const uint32_t*, uint32_t*, uint32_t*, uint32_t*,
                                uint32_t*, int, int, unsigned, int);
static py::dict cov_sweep_check(const std::string& who, CovSweepKernel kernel,
                                int mask_bits, const std::vector<uint32_t>& tab,
                                int device, int reps, int max_rounds,
                                int poison_key, unsigned poison_mask,
                                bool poison_all) {
  cov_validate(who, reps, max_rounds, poison_key, poison_mask, mask_bits);
  const int cus = cov_select_device(who, device);
  return cov_sweep_dict(cov_run_sweep(
      cus, max_rounds, tab, [&](int, uint32_t* d_tab, uint32_t* slots) {
        hipLaunchKernelGGL(kernel, dim3(kCovBlocksPerCu * cus), dim3(kCovBlock), 0,
                           0, d_tab, slots, slots + kCovSlots, slots + 2 * kCovSlots,
                           slots + 3 * kCovSlots, reps, poison_key, poison_mask,
                           poison_all ? 1 : 0);
      }));
}

static py::dict cu_coverage_check(int device, int reps, int max_rounds,
                                  int poison_key, unsigned poison_mask,
                                  bool poison_all) {
  return cov_sweep_check("cu_coverage_check", cu_coverage_kernel, 4,
                         cov_build_table(), device, reps, max_rounds, poison_key,
                         poison_mask, poison_all);
}

// ---------------------------------------------------------------------------
// MX block-scaled matrix path: v_mfma_scale_f32_16x16x128_f8f6f4 and
// v_mfma_scale_f32_32x32x64_f8f6f4 with OCP MX operands (e4m3, e5m2, e2m3,
// e3m2, e2m1) and one E8M0 scale per 32-element K block.  The 6-bit / 4-bit
// unpackers and the scale application are hardware the bf16 / fp8 tiles never
// touch, so they get their own exact problems, single-tile entry point,
// whole-device sweep and burn-in.
//
// Format index == the instruction's cbsz / blgp code:
//   0 e4m3   1 e5m2   2 e2m3   3 e3m2   4 e2m1
//
// Fragment layout, confirmed on an MI355X by the exact single-tile tests (a
// wrong map cannot reproduce those tiles; see validation/README.md).  Lane l
// supplies A row / B col l % M and 32 elements; with g = l / M (M = 16: four
// lane groups, M = 32: two) element j = 0..31 of the lane is
//   6-bit and 4-bit formats:  k = 32*g + j              (K-contiguous)
//   8-bit formats:            k = (K/2)*(j>>4) + 16*g + (j&15)
// i.e. an 8-bit lane holds two runs of 16: words 0..3 from the first half of
// K and words 4..7 from the second.  Element j sits at bits [w*j, w*j + w) of
// the lane's little-endian operand string (w = 8: 8 words; w = 6: words 0..5,
// 6 and 7 zero; w = 4: words 0..3, 4..7 zero).  One byte of a scale VGPR per
// lane and operand, picked by op_sel: lane group g supplies the scale of K
// block g (k in [32*g, 32*g + 32)) of its row / col for every format, so for
// an 8-bit operand it is not the lane that holds those elements.  C/D use
// the dtype-independent maps:
//   16x16: row = (l>>4)*4 + r, col = l&15
//   32x32: row = (r&3) + 8*(r>>2) + 4*(l>>5), col = l&31            r = 0..15
//
// Exactness.  Every operand is a small integer times a power of two and every
// scale is a power of two, so each scaled product is an integer multiple of
// q, the largest power of two that divides all of them.  With S the largest
// sum of |a*b*sa*sb| over the outputs, any summation order is exact in f32
// when S/q <= 2^24.  How wide the hardware aligns scaled products internally
// is not documented, so the generator keeps S/q <= 2^kMxSpanBoundLog2 and
// throws otherwise; the comparison is bitwise, with no tolerance.
// ---------------------------------------------------------------------------

constexpr int kMxFailBits = 7;  // e4m3 e5m2 e2m3 e3m2 e2m1 mixed shape32

using i32x8 = __attribute__((ext_vector_type(8))) int;
using f32x16 = __attribute__((ext_vector_type(16))) float;

#if defined(__gfx950__)
template <int FA, int FB, int OA, int OB>
__device__ __forceinline__ f32x4 mx16(i32x8 a, i32x8 b, f32x4 c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, OA,
                                                          sa, OB, sb);
}
template <int FA, int FB, int OA, int OB>
__device__ __forceinline__ f32x16 mx32(i32x8 a, i32x8 b, f32x16 c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, FA, FB, OA,
                                                         sa, OB, sb);
}
#endif

// Single tile: one wave, one instruction.  rec = 64 lanes x {a[8], b[8], sa,
// sb}; out = 64 lanes x 16 accumulator registers (4 used by 16x16).  The
// format pair is a run-time argument, so every cbsz / blgp pair has a case.
#define MX_TILE_CASE(FN, FA, FB)                                            \
  case FA * kMxFormats + FB:                                                \
    d = FN<FA, FB, mx_sel_a(SET), mx_sel_b(SET)>(a, b, d, sa, sb);          \
    break;
#define MX_TILE_ROW(FN, FA)                                                 \
  MX_TILE_CASE(FN, FA, 0) MX_TILE_CASE(FN, FA, 1) MX_TILE_CASE(FN, FA, 2)   \
  MX_TILE_CASE(FN, FA, 3) MX_TILE_CASE(FN, FA, 4)
#define MX_TILE_CASES(FN)                                                   \
  MX_TILE_ROW(FN, 0) MX_TILE_ROW(FN, 1) MX_TILE_ROW(FN, 2)                  \
  MX_TILE_ROW(FN, 3) MX_TILE_ROW(FN, 4)

template <int SHAPE, int SET>
__global__ void mx_tile_kernel(const uint32_t* __restrict__ rec,
                               float* __restrict__ out, int pair) {
#if defined(__gfx950__)
  const int lane = threadIdx.x;  // one wave of 64
  const uint32_t* p = rec + lane * kMxTileRecWords;
  i32x8 a, b;
  for (int i = 0; i < 8; ++i) {
    a[i] = (int)p[i];
    b[i] = (int)p[8 + i];
  }
  const int sa = (int)p[16], sb = (int)p[17];
  if constexpr (SHAPE == 0) {
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    switch (pair) { MX_TILE_CASES(mx16) }
    for (int r = 0; r < 4; ++r) out[lane * 16 + r] = d[r];
  } else {
    f32x16 d = {0.f};
    switch (pair) { MX_TILE_CASES(mx32) }
    for (int r = 0; r < 16; ++r) out[lane * 16 + r] = d[r];
  }
#endif
}

static int mx_format_index(const std::string& name) {
  for (int f = 0; f < kMxFormats; ++f)
    if (name == kMxFmt[f].name) return f;
  throw std::invalid_argument("unknown MX format '" + name +
                              "' (e4m3, e5m2, e2m3, e3m2, e2m1)");
}
static int mx_shape_index(const std::string& name) {
  for (int s = 0; s < 2; ++s)
    if (name == mx_shape_name(s)) return s;
  throw std::invalid_argument("unknown MX shape '" + name +
                              "' (16x16x128, 32x32x64)");
}

static py::dict mx_problem_dict(const MxProblem& p) {
  py::dict e;
  e["set"] = p.set;
  e["fmt_a"] = std::string(kMxFmt[p.fa].name);
  e["fmt_b"] = std::string(kMxFmt[p.fb].name);
  e["shape"] = std::string(mx_shape_name(p.shape));
  e["m"] = p.m;
  e["n"] = p.n;
  e["k"] = p.k;
  e["op_sel_a"] = p.sel_a;
  e["op_sel_b"] = p.sel_b;
  e["a_codes"] = std::vector<int>(p.a_codes.begin(), p.a_codes.end());
  e["b_codes"] = std::vector<int>(p.b_codes.begin(), p.b_codes.end());
  e["a_scales"] = std::vector<int>(p.a_scales.begin(), p.a_scales.end());
  e["b_scales"] = std::vector<int>(p.b_scales.begin(), p.b_scales.end());
  e["d"] = p.d;
  e["log2_span"] = p.log2_span;
  e["a_words"] = p.a_words;  // 64 lanes x 8, as packed for the instruction
  e["b_words"] = p.b_words;
  e["a_scale_words"] = p.a_scale_words;
  e["b_scale_words"] = p.b_scale_words;
  return e;
}

static py::dict mx_reference() {
  // host only: no HIP call
  py::dict out;
  out["sets"] = kMxSets;
  out["span_bound_log2"] = kMxSpanBoundLog2;
  py::list problems;
  for (int s = 0; s < kMxSets; ++s)
    for (int i = 0; i < kMxProbs; ++i)
      problems.append(mx_problem_dict(
          mx_problem(s, kMxProbFa[i], kMxProbFb[i], kMxProbShape[i])));
  out["problems"] = problems;
  return out;
}

template <int SHAPE>
static void mx_tile_launch(int set, const uint32_t* rec, float* out, int pair) {
  // set is in [0, kMxSets): mx_problem has validated it
  static void (*const kKernels[kMxSets])(const uint32_t*, float*, int) = {
      mx_tile_kernel<SHAPE, 0>, mx_tile_kernel<SHAPE, 1>, mx_tile_kernel<SHAPE, 2>,
      mx_tile_kernel<SHAPE, 3>, mx_tile_kernel<SHAPE, 4>};
  hipLaunchKernelGGL(kKernels[set], dim3(1), dim3(64), 0, 0, rec, out, pair);
}

static py::dict mx_mfma_tile(int device, const std::string& fmt_a,
                             const std::string& fmt_b, const std::string& shape,
                             int set) {
  // Run one scaled MFMA and return the raw problem + the GPU tile so Python
  // tests can verify against independent decoders.
  const int fa = mx_format_index(fmt_a), fb = mx_format_index(fmt_b);
  const int sh = mx_shape_index(shape);
  const MxProblem p = mx_problem(set, fa, fb, sh);  // validates set
  const std::vector<uint32_t> rec = mx_tile_record(p);
  HIP_CHECK(hipSetDevice(device));
  DeviceBuf<uint32_t> d_rec(rec.size());
  DeviceBuf<float> d_out(64 * 16);
  d_rec.upload(rec.data(), rec.size());
  d_out.fill(0xFF);
  if (sh == 0)
    mx_tile_launch<0>(set, d_rec.get(), d_out.get(), fa * kMxFormats + fb);
  else
    mx_tile_launch<1>(set, d_rec.get(), d_out.get(), fa * kMxFormats + fb);
  HIP_CHECK(hipGetLastError());
  std::vector<float> regs(d_out.size());
  d_out.download(regs.data(), regs.size());
  std::vector<float> d_gpu((size_t)p.m * p.n);
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < mx_lane_regs(sh); ++r)
      d_gpu[mx_d_index(sh, l, r)] = regs[l * 16 + r];
  py::dict out = mx_problem_dict(p);
  out["d_gpu"] = d_gpu;  // GPU result, row-major m x n
  return out;
}

// Whole-device MX sweep, built like cu_coverage_kernel: same grid, launch
// bounds, 64 KiB LDS claim, placement key and slot scheme, fixed work per
// workgroup.  Per-lane record of one (set, problem): a[8] b[8] sa sb exp[16]
// (16x16 problems use exp[0..3]).

template <int SET, int P>
__device__ __forceinline__ unsigned mx_cov_problem(const uint32_t* tab, int lane,
                                                   unsigned pm) {
  unsigned fail = 0;
#if defined(__gfx950__)
  constexpr int FA = kMxProbFa[P], FB = kMxProbFb[P], BIT = kMxProbBit[P];
  // volatile: operands and expected values are re-read from global memory
  // every repetition, so neither the MFMA nor the compare can be hoisted
  const uint32_t* rec =
      tab + (size_t)((SET * kMxProbs + P) * 64 + lane) * kMxRecWords;
  // opaque to the optimizer: otherwise the address of every word of every
  // record is loop-invariant, gets hoisted out of the repetition loop and
  // spills; this way each record is one base plus immediate offsets
  asm volatile("" : "+v"(rec));
  const volatile uint32_t* p = rec;
  i32x8 a, b;
  for (int i = 0; i < 8; ++i) {
    a[i] = (int)p[i];
    b[i] = (int)p[8 + i];
  }
  const int sa = (int)p[16], sb = (int)p[17];
  const uint32_t px = (pm >> BIT) & 1u;  // test hook: flips an expected bit
  if constexpr (kMxProbShape[P] == 0) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 d = mx16<FA, FB, mx_sel_a(SET), mx_sel_b(SET)>(a, b, zero, sa, sb);
    for (int r = 0; r < 4; ++r)
      if (__float_as_uint(d[r]) != (p[18 + r] ^ px)) fail = 1u << BIT;
  } else {
    const f32x16 zero = {0.f};
    const f32x16 d = mx32<FA, FB, mx_sel_a(SET), mx_sel_b(SET)>(a, b, zero, sa, sb);
    for (int r = 0; r < 16; ++r)
      if (__float_as_uint(d[r]) != (p[18 + r] ^ px)) fail = 1u << BIT;
  }
#endif
  return fail;
}

template <int SET>
__device__ __forceinline__ unsigned mx_cov_set(const uint32_t* tab, int lane,
                                               unsigned pm) {
  return mx_cov_problem<SET, 0>(tab, lane, pm) | mx_cov_problem<SET, 1>(tab, lane, pm) |
         mx_cov_problem<SET, 2>(tab, lane, pm) | mx_cov_problem<SET, 3>(tab, lane, pm) |
         mx_cov_problem<SET, 4>(tab, lane, pm) | mx_cov_problem<SET, 5>(tab, lane, pm) |
         mx_cov_problem<SET, 6>(tab, lane, pm) | mx_cov_problem<SET, 7>(tab, lane, pm) |
         mx_cov_problem<SET, 8>(tab, lane, pm) | mx_cov_problem<SET, 9>(tab, lane, pm);
}
static_assert(kMxProbs == 10 && kMxSets == 5, "mx_cov_set / mx_coverage_kernel");

__global__ void __launch_bounds__(kCovBlock, kCovBlocksPerCu)
mx_coverage_kernel(const uint32_t* tab, uint32_t* __restrict__ slot_waves,
                   uint32_t* __restrict__ slot_fail,
                   uint32_t* __restrict__ slot_hw_id,
                   uint32_t* __restrict__ slot_xcc_id, int reps, int poison_key,
                   unsigned poison_mask, int poison_all) {
#if defined(__gfx950__)
  __shared__ uint32_t lds[kCovLdsWords];  // the claim that keeps 2 per CU
  const uint32_t hw_id = __builtin_amdgcn_s_getreg(kCovHwRegHwId);
  const uint32_t xcc_id = __builtin_amdgcn_s_getreg(kCovHwRegXccId);
  const uint32_t key = ((xcc_id & 0xFu) << 8) | ((hw_id >> 8) & 0xFFu);
  const uint32_t simd = (hw_id >> 4) & 3u;
  const unsigned pm = (poison_all || (int)key == poison_key) ? poison_mask : 0u;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  unsigned fail = 0;
#pragma unroll 1
  for (int rep = 0; rep < reps; ++rep) {
    fail |= mx_cov_set<0>(tab, lane, pm);
    fail |= mx_cov_set<1>(tab, lane, pm);
    fail |= mx_cov_set<2>(tab, lane, pm);
    fail |= mx_cov_set<3>(tab, lane, pm);
    fail |= mx_cov_set<4>(tab, lane, pm);
  }

  // the masks pass through LDS once (neighbouring lanes swap theirs), which
  // keeps the static claim alive; the wave-wide OR below makes it a no-op
  lds[tid * 64] = fail;  // tid < 256: index < kCovLdsWords
  __syncthreads();
  fail |= lds[(tid ^ 1) * 64];

  unsigned wave_fail = 0;
  for (int b = 0; b < kMxFailBits; ++b)
    if (__ballot((fail >> b) & 1u) != 0) wave_fail |= 1u << b;
  if (lane == 0) {
    const uint32_t slot = key * 4u + simd;  // < kCovSlots by the masks above
    atomicAdd(&slot_waves[slot], 1u);
    if (wave_fail) atomicOr(&slot_fail[slot], wave_fail);
    slot_hw_id[slot] = hw_id;
    slot_xcc_id[slot] = xcc_id;
  }
#endif
}

static py::dict mx_coverage_check(int device, int reps, int max_rounds,
                                  int poison_key, unsigned poison_mask,
                                  bool poison_all) {
  return cov_sweep_check("mx_coverage_check", mx_coverage_kernel, kMxFailBits,
                         mx_build_table(), device, reps, max_rounds, poison_key,
                         poison_mask, poison_all);
}

// MX burn-in: the analogue of mfma_burn_kernel on 16x16x128, e2m1 or e4m3,
// four independent accumulators per wave.  Operands are non-zero alphabet
// codes; both scales are 2^-20, so the accumulators stay finite.
template <int FMT>
__global__ void mx_burn_kernel(const uint32_t* __restrict__ seed,
                               float* __restrict__ out, int iters) {
#if defined(__gfx950__)
  const int lane = threadIdx.x & 63;
  i32x8 a, b;
  for (int i = 0; i < 8; ++i) {
    a[i] = (int)seed[lane * 16 + i];
    b[i] = (int)seed[lane * 16 + 8 + i];
  }
  const int sc = (int)seed[64 * 16];
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  f32x4 acc2 = {0, 0, 0, 0}, acc3 = {0, 0, 0, 0};
  for (int i = 0; i < iters; ++i) {
    acc0 = mx16<FMT, FMT, 0, 0>(a, b, acc0, sc, sc);
    acc1 = mx16<FMT, FMT, 0, 0>(a, b, acc1, sc, sc);
    acc2 = mx16<FMT, FMT, 0, 0>(a, b, acc2, sc, sc);
    acc3 = mx16<FMT, FMT, 0, 0>(a, b, acc3, sc, sc);
  }
  const float sink = acc0[0] + acc1[1] + acc2[2] + acc3[3];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  out[tid] = sink;  // keep the loop alive
#endif
}

static double mx_throughput_tflops(int device, const std::string& fmt, int iters) {
  const int f = mx_format_index(fmt);
  if (f != 0 && f != 4)
    throw std::invalid_argument("mx_throughput_tflops: fmt must be e2m1 or e4m3");
  if (iters < 1 || iters > 10000000)
    throw std::invalid_argument("mx_throughput_tflops: iters must be in [1, 1e7]");
  const std::vector<uint32_t> hseed = mx_burn_seed(f);
  const int block = 256, grid = 512;  // 2048 waves = 2 per SIMD, 4 chains each
  HIP_CHECK(hipSetDevice(device));
  DeviceBuf<uint32_t> d_seed(hseed.size());
  DeviceBuf<float> d_out((size_t)block * grid);
  d_seed.upload(hseed.data(), hseed.size());
  auto launch = [&](int n) {
    hipLaunchKernelGGL(f == 4 ? mx_burn_kernel<4> : mx_burn_kernel<0>, dim3(grid),
                       dim3(block), 0, 0, d_seed.get(), d_out.get(), n);
  };
  launch(1000);  // warmup
  HIP_CHECK(hipDeviceSynchronize());
  EventTimer timer;
  const float ms = timer.time_ms([&] { launch(iters); });
  const double waves = (double)grid * block / 64.0;
  const double flop = waves * (double)iters * 4.0 * (16.0 * 16.0 * 128.0 * 2.0);
  return flop / 1e12 / ((double)ms / 1e3);
}

// ---------------------------------------------------------------------------
// HBM data-integrity check: a moving-inversions pattern test over a region of
// device memory that is allocated in chunks.  Every pattern runs three phases
// over the whole region (all chunks) before the next phase starts:
//   fill           write p
//   verify_invert  read, compare with p, write ~p to the same address
//   verify         read, compare with ~p
// so that for a region larger than the caches each read is served by HBM.
// The written ~p is computed from the pattern, never from the data read.
//
// A pattern is a pure function of the region's logical 64-bit word index, so
// an aliased or mis-decoded address reads back another index's word:
//   hash     splitmix64 finaliser of (i + seed * golden ratio): every data
//            bit toggles, no two nearby or power-of-two-distant words agree
//   checker  0xAAAA.. for even i, 0x5555.. for odd i (seed ignored)
//
// Comparison is exact.  A lane counts the words it compared; each workgroup
// adds its total to one of kHbmShards counters once, at its end, and the host
// checks coverage by summing them (counted, not trusted).  Only a mismatching
// lane touches the error counter, the xor mask and the capped record buffer.
// Every kernel does a fixed amount of work and exits: no spins, no waits
// between workgroups.
//
// The poison hook is data only: it XORs a mask into the *expected* value of
// the selected words and never alters memory, so a record's `got` is what the
// fill kernel really wrote.
// ---------------------------------------------------------------------------

constexpr int kHbmFill = 0, kHbmVerifyInvert = 1, kHbmVerify = 2;
constexpr int kHbmBlock = 512;            // bw_copy_kernel's sweep-tuned shape
constexpr int kHbmShards = 1024;          // compared-word counters, one line each
constexpr int kHbmShardStride = 16;       // in uint64: 128 bytes apart
constexpr int kHbmMaxRecords = 4096;
constexpr int kHbmMaxPasses = 16;
constexpr size_t kHbmReferenceMax = 65536;
constexpr uint64_t kHbmReserveBytes = 2ull << 30;
constexpr uint64_t kHbmBeyondCacheBytes = 512ull << 20;  // 2 x Infinity Cache

using u64x2 = __attribute__((ext_vector_type(2))) uint64_t;

struct HbmRecord {
  uint64_t word, phase, expected, got;
};

// Device-side result block: [0] error count, [1] xor mask, [2] record claims.
constexpr int kHbmCtlErrors = 0, kHbmCtlXor = 1, kHbmCtlClaims = 2,
              kHbmCtlWords = 4;

struct HbmLaunch {
  uint64_t* buf;        // this chunk
  uint64_t nwords;      // words in this chunk
  uint64_t base;        // logical index of the chunk's first word
  uint64_t seed;
  uint64_t poison_xor;
  uint64_t poison_stride;
  int64_t poison_word;  // -1: the hook is off for this launch
  unsigned long long* ctl;
  unsigned long long* shards;
  HbmRecord* records;
  uint32_t max_records;
  uint32_t verify_index;
  int pattern;
};

// test hook: data only, returns the mask to XOR into the expected value.
// Callers test a.poison_word >= 0 first (uniform), so a normal run pays one
// scalar branch per loop iteration and never the 64-bit modulo.
__device__ __forceinline__ uint64_t hbm_poison(const HbmLaunch& a, uint64_t i) {
  const uint64_t w = (uint64_t)a.poison_word;
  if (i < w) return 0;
  if (a.poison_stride == 0) return i == w ? a.poison_xor : 0;
  return (i - w) % a.poison_stride == 0 ? a.poison_xor : 0;
}

// got ^ expected for word i; zero when the word is right
__device__ __forceinline__ uint64_t hbm_diff(const HbmLaunch& a, uint64_t i,
                                             uint64_t got, uint64_t inv) {
  uint64_t x = got ^ hbm_pattern_value(a.pattern, a.seed, i) ^ inv;
  if (a.poison_word >= 0) x ^= hbm_poison(a, i);
  return x;
}

// the rare path: count the mismatch and claim a record slot
__device__ __forceinline__ void hbm_report(const HbmLaunch& a, uint64_t i,
                                        uint64_t got, uint64_t x, uint32_t& bad,
                                        uint64_t& bad_xor) {
  if (x == 0) return;
  ++bad;
  bad_xor |= x;
  record_log_claim(
      RecordLogView<HbmRecord>{&a.ctl[kHbmCtlClaims], a.records, a.max_records},
      [&] { return HbmRecord{i, a.verify_index, got ^ x, got}; });
}

// kind: kHbmFill / kHbmVerifyInvert / kHbmVerify.  16-byte nontemporal
// accesses, 2x unrolled grid-stride as in bw_copy_kernel; one thread handles
// the odd last word of a chunk with plain scalar accesses.  The hot loop is
// straight-line: the four differences of an iteration are ORed and only a
// non-zero OR enters the reporting path.  A lane's counters are 32-bit: the
// grid is never smaller than 2^19 threads.
template <int kind>
__global__ void __launch_bounds__(kHbmBlock) hbm_pattern_kernel(HbmLaunch a) {
  __shared__ uint32_t wave_compared[kHbmBlock / 64];
  u64x2* __restrict__ v = reinterpret_cast<u64x2*>(a.buf);
  const uint64_t nvec = a.nwords >> 1;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // what a verify kernel expects to read, and what a writing kernel stores
  const uint64_t inv = kind == kHbmVerify ? ~0ull : 0ull;
  const uint64_t winv = kind == kHbmVerifyInvert ? ~0ull : 0ull;
  uint32_t compared = 0, bad = 0;
  uint64_t bad_xor = 0;

  uint64_t i = tid;
  for (; i + stride < nvec; i += 2 * stride) {
    const uint64_t w0 = a.base + 2 * i, w1 = a.base + 2 * (i + stride);
    if (kind != kHbmFill) {
      const u64x2 g0 = __builtin_nontemporal_load(&v[i]);
      const u64x2 g1 = __builtin_nontemporal_load(&v[i + stride]);
      const uint64_t x0 = hbm_diff(a, w0, g0[0], inv);
      const uint64_t x1 = hbm_diff(a, w0 + 1, g0[1], inv);
      const uint64_t x2 = hbm_diff(a, w1, g1[0], inv);
      const uint64_t x3 = hbm_diff(a, w1 + 1, g1[1], inv);
      compared += 4;
      if ((x0 | x1 | x2 | x3) != 0) {
        hbm_report(a, w0, g0[0], x0, bad, bad_xor);
        hbm_report(a, w0 + 1, g0[1], x1, bad, bad_xor);
        hbm_report(a, w1, g1[0], x2, bad, bad_xor);
        hbm_report(a, w1 + 1, g1[1], x3, bad, bad_xor);
      }
    }
    if (kind != kHbmVerify) {
      u64x2 p0, p1;
      p0[0] = hbm_pattern_value(a.pattern, a.seed, w0) ^ winv;
      p0[1] = hbm_pattern_value(a.pattern, a.seed, w0 + 1) ^ winv;
      p1[0] = hbm_pattern_value(a.pattern, a.seed, w1) ^ winv;
      p1[1] = hbm_pattern_value(a.pattern, a.seed, w1 + 1) ^ winv;
      __builtin_nontemporal_store(p0, &v[i]);
      __builtin_nontemporal_store(p1, &v[i + stride]);
    }
  }
  for (; i < nvec; i += stride) {
    const uint64_t w0 = a.base + 2 * i;
    if (kind != kHbmFill) {
      const u64x2 g0 = __builtin_nontemporal_load(&v[i]);
      const uint64_t x0 = hbm_diff(a, w0, g0[0], inv);
      const uint64_t x1 = hbm_diff(a, w0 + 1, g0[1], inv);
      compared += 2;
      if ((x0 | x1) != 0) {
        hbm_report(a, w0, g0[0], x0, bad, bad_xor);
        hbm_report(a, w0 + 1, g0[1], x1, bad, bad_xor);
      }
    }
    if (kind != kHbmVerify) {
      u64x2 p0;
      p0[0] = hbm_pattern_value(a.pattern, a.seed, w0) ^ winv;
      p0[1] = hbm_pattern_value(a.pattern, a.seed, w0 + 1) ^ winv;
      __builtin_nontemporal_store(p0, &v[i]);
    }
  }
  if ((a.nwords & 1ull) && tid == 0) {  // scalar tail: the odd last word
    const uint64_t t = a.nwords - 1;
    if (kind != kHbmFill) {
      const uint64_t got = a.buf[t];
      ++compared;
      hbm_report(a, a.base + t, got, hbm_diff(a, a.base + t, got, inv), bad,
                 bad_xor);
    }
    if (kind != kHbmVerify)
      a.buf[t] = hbm_pattern_value(a.pattern, a.seed, a.base + t) ^ winv;
  }

  if (kind != kHbmFill) {
    if (bad != 0) {  // on a mismatch, and only then
      atomicAdd(&a.ctl[kHbmCtlErrors], (unsigned long long)bad);
      atomicOr(&a.ctl[kHbmCtlXor], (unsigned long long)bad_xor);
    }
    // workgroup total of compared words -> one add to this block's shard
    uint32_t sum = compared;
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) wave_compared[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long total = 0;
      for (int w = 0; w < kHbmBlock / 64; ++w) total += wave_compared[w];
      atomicAdd(&a.shards[(blockIdx.x & (kHbmShards - 1)) * kHbmShardStride],
                total);
    }
  }
}

static int hbm_pattern_id(const std::string& name) {
  if (name == "hash") return kHbmPatternHash;
  if (name == "checker") return kHbmPatternChecker;
  throw std::invalid_argument("hbm pattern must be 'hash' or 'checker'");
}

static std::vector<uint64_t> hbm_pattern_reference(const std::string& pattern,
                                                   uint64_t seed,
                                                   uint64_t first_word,
                                                   size_t count, bool inverted) {
  // host only: no HIP call
  const int id = hbm_pattern_id(pattern);
  if (count > kHbmReferenceMax)
    throw std::invalid_argument("hbm_pattern_reference: count is at most 65536");
  std::vector<uint64_t> out(count);
  for (size_t k = 0; k < count; ++k) {
    const uint64_t v = hbm_pattern_value(id, seed, first_word + k);
    out[k] = inverted ? ~v : v;
  }
  return out;
}

// The result tables of hbm_pattern_kernel and of the host-link kernels built
// like it: the control block with the record log, and the sharded counters.
struct HbmTables {
  RecordLog<HbmRecord> log;
  DeviceBuf<unsigned long long> shards{(size_t)kHbmShards * kHbmShardStride};
  explicit HbmTables(int max_records)
      : log((size_t)std::max(1, max_records), kHbmCtlWords, kHbmCtlClaims) {
    shards.fill(0);
  }
  void attach(HbmLaunch& a, size_t cap) const {
    const RecordLogView<HbmRecord> v = log.view(cap);
    a.ctl = log.ctl();
    a.shards = shards.get();
    a.records = v.records;
    a.max_records = v.cap;
  }
  // after a synchronise: the words the kernels counted; `rezero` for a next phase
  uint64_t words_compared(bool rezero = false) {
    std::vector<unsigned long long> sh(shards.size());
    shards.download(sh.data(), sh.size());
    uint64_t n = 0;
    for (int s = 0; s < kHbmShards; ++s) n += sh[(size_t)s * kHbmShardStride];
    if (rezero) shards.fill(0);
    return n;
  }
};

struct HbmChunk {
  DeviceBuf<uint64_t> buf;
  uint64_t first_word = 0;  // logical
  uint64_t words = 0;
};

static void hbm_launch(int kind, const HbmLaunch& a) {
  // bw_copy_kernel's launch shape: ~2 vectors per thread, grid in [1024, 131072]
  const uint64_t nvec = a.nwords >> 1;
  const long want = (long)(nvec / (2 * (uint64_t)kHbmBlock)) + 1;
  const int grid = (int)std::min<long>(131072, std::max<long>(1024, want));
  static void (*const kKernels[3])(HbmLaunch) = {  // indexed by kind
      hbm_pattern_kernel<kHbmFill>, hbm_pattern_kernel<kHbmVerifyInvert>,
      hbm_pattern_kernel<kHbmVerify>};
  hipLaunchKernelGGL(kKernels[kind], dim3(grid), dim3(kHbmBlock), 0, 0, a);
  HIP_CHECK(hipGetLastError());
}

static py::dict hbm_pattern_check(int device, uint64_t nbytes,
                                  uint64_t chunk_bytes, int passes,
                                  uint64_t seed, bool checker,
                                  uint64_t first_word, int max_records,
                                  int64_t poison_word, uint64_t poison_stride,
                                  uint64_t poison_xor, int poison_phase) {
  // every argument is validated before the first HIP call
  if (nbytes % 8 != 0)
    throw std::invalid_argument("hbm_pattern_check: nbytes must be a multiple of 8");
  if (chunk_bytes == 0 || chunk_bytes % 8 != 0)
    throw std::invalid_argument(
        "hbm_pattern_check: chunk_bytes must be a positive multiple of 8");
  require_range("hbm_pattern_check", "passes", passes, 1, kHbmMaxPasses);
  require_range("hbm_pattern_check", "max_records", max_records, 1, kHbmMaxRecords);
  if (first_word > (1ull << 62) || nbytes > (1ull << 62))
    throw std::invalid_argument("hbm_pattern_check: region out of the index range");
  const int n_patterns = passes + (checker ? 1 : 0);
  const int n_verify = 2 * n_patterns;
  if (poison_word < -1)
    throw std::invalid_argument("hbm_pattern_check: poison_word is -1 or an index");
  if (poison_word >= 0 && poison_xor == 0)
    throw std::invalid_argument(
        "hbm_pattern_check: poison_xor must be non-zero with a poison_word");
  if (poison_phase < -1 || poison_phase >= n_verify)
    throw std::invalid_argument("hbm_pattern_check: poison_phase out of range");

  HIP_CHECK(hipSetDevice(device));
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t usable =
      free_b > kHbmReserveBytes ? (uint64_t)free_b - kHbmReserveBytes : 0;
  if (nbytes == 0) {
    nbytes = usable & ~7ull;
    if (nbytes == 0)
      throw std::runtime_error(
          "hbm_pattern_check: no free device memory beyond the 2 GiB reserve");
  } else if (nbytes > usable) {
    throw std::runtime_error(
        "hbm_pattern_check: request exceeds free device memory minus the 2 GiB "
        "reserve (" + std::to_string(nbytes) + " > " + std::to_string(usable) + ")");
  }
  const uint64_t words = nbytes / 8;
  const uint64_t chunk_words = chunk_bytes / 8;

  // a chunk that cannot be allocated raises: never silently test less
  std::vector<HbmChunk> chunks;
  chunks.reserve((size_t)((words + chunk_words - 1) / chunk_words));
  for (uint64_t off = 0; off < words; off += chunk_words) {
    chunks.emplace_back();
    HbmChunk& c = chunks.back();
    c.first_word = first_word + off;
    c.words = std::min(chunk_words, words - off);
    c.buf = DeviceBuf<uint64_t>((size_t)c.words);
  }

  HbmTables tables(max_records);
  EventTimer timer;

  static const char* const kKindNames[3] = {"fill", "verify_invert", "verify"};
  py::list phases;
  double elapsed_ms = 0.0;
  int phase_index = 0, verify_index = 0;
  for (int p = 0; p < n_patterns; ++p) {
    const bool is_hash = p < passes;
    const uint64_t pseed = is_hash ? seed + (uint64_t)p : 0;
    for (int kind = kHbmFill; kind <= kHbmVerify; ++kind) {
      const bool verifies = kind != kHbmFill;
      const bool poisoned = verifies && poison_word >= 0 &&
                            (poison_phase < 0 || poison_phase == verify_index);
      const float ms = timer.time_ms([&] {
        for (const HbmChunk& c : chunks) {
          HbmLaunch a;
          a.buf = c.buf.get();
          a.nwords = c.words;
          a.base = c.first_word;
          a.seed = pseed;
          a.poison_xor = poison_xor;
          a.poison_stride = poison_stride;
          a.poison_word = poisoned ? poison_word : -1;
          tables.attach(a, (size_t)max_records);
          a.verify_index = (uint32_t)verify_index;
          a.pattern = is_hash ? kHbmPatternHash : kHbmPatternChecker;
          hbm_launch(kind, a);
        }
      });
      elapsed_ms += ms;
      // bytes the phase really moves: verify_invert reads and writes
      const double moved = (kind == kHbmVerifyInvert ? 2.0 : 1.0) * (double)nbytes;
      py::dict ph;
      ph["index"] = phase_index++;
      ph["pattern"] = is_hash ? "hash" : "checker";
      ph["seed"] = pseed;
      ph["kind"] = kKindNames[kind];
      if (verifies)
        ph["verify_index"] = verify_index++;
      else
        ph["verify_index"] = py::none();
      ph["ms"] = (double)ms;
      ph["gbps"] = ms > 0.f ? moved / 1e9 / ((double)ms / 1e3) : 0.0;
      phases.append(ph);
    }
  }

  const auto log = tables.log.collect((size_t)max_records);
  const uint64_t words_verified = tables.words_compared();

  py::list chunk_list;
  for (size_t c = 0; c < chunks.size(); ++c) {
    py::dict e;
    e["index"] = c;
    e["first_word"] = chunks[c].first_word;
    e["bytes"] = chunks[c].words * 8;
    chunk_list.append(e);
  }
  py::list records;
  for (const HbmRecord& r : log.records) {
    py::dict e;
    e["word"] = r.word;
    e["byte_offset"] = 8 * (r.word - first_word);
    e["chunk"] = (r.word - first_word) / chunk_words;
    e["phase"] = r.phase;
    e["expected"] = r.expected;
    e["got"] = r.got;
    records.append(e);
  }
  py::dict out;
  out["bytes"] = nbytes;
  out["words"] = words;
  out["first_word"] = first_word;
  out["chunks"] = chunk_list;
  out["phases"] = phases;
  out["words_verified"] = words_verified;
  out["words_expected"] = words * (uint64_t)n_verify;
  out["error_count"] = log.ctl[kHbmCtlErrors];
  out["xor_or"] = log.ctl[kHbmCtlXor];
  out["records"] = records;
  out["records_dropped"] = log.claims - (uint64_t)log.records.size();
  out["elapsed_ms"] = elapsed_ms;
  out["beyond_cache"] = nbytes > kHbmBeyondCacheBytes;
  return out;
}

// ---------------------------------------------------------------------------
// Cross-XCD hand-off and device-scope atomics check.  The eight XCDs' L2s are
// not coherent with each other: a word written on one XCD reaches a reader on
// another only through an agent-scope release on the writer (L2 write-back),
// an agent-scope acquire on the reader (L1 invalidate) and the memory-side
// atomics between them.  Two kernels exercise exactly that path; every
// workgroup does a fixed amount of work and exits, nobody waits for anybody.
//
// Hand-off sweep (xcd_handoff_kernel): the wait-free last-arriver protocol of
// a split-K reduction with a pattern in place of partial sums.  group x G
// workgroups; block b is member b / G of group b % G.  A 128-byte line is 16
// 64-bit words: words 0-7 are static (host-filled once with
// hash(seed ^ kXfStaticKey, idx), never written again), words 8-15 carry the
// payload hash(seed + round, idx); idx is the word's index in the slab buffer
// [reps][blocks][slab_lines][16].  Per rep a block
//   1. reads and verifies the static halves of every line of its group's slabs
//      (a real check that also leaves every line in this CU's L1 and this
//      XCD's L2, so a later acquire has something to invalidate),
//   2. writes the payload halves of its own slab and its XCC_ID,
//   3. drains, releases at agent scope and draws a ticket,
//   4. and, if it drew group - 1, acquires at agent scope and verifies every
//      payload half of the group exactly.
// The payload is not reset between rounds: what a broken hand-off reads is
// the previous round's hash(seed + round - 1, idx); the upload is round -1.
//
// Which member arrives last decides the reader XCC of an episode.  Left to
// the dispatcher that is heavily skewed: in a given launch the same few XCDs
// arrive last in almost every group (measured: one XCC was the reader in 0 of
// 1984 episodes of a run), and pairs stay uncovered for many rounds.  So
// member (rep + round) % group of every episode idles for a fixed few
// microseconds before it draws its ticket and every other member idles as
// long after drawing its own: each block spends the same time per rep, and
// the late member, and with it the reader XCC, rotates through the group.
// This is a fixed delay, not a wait on anybody, and like the odd G it only
// speeds coverage up: the verdict counts what happened and never relies on it.
//
// A (writer, reader) pair can only occur inside a group, and a group of fewer
// members than there are XCCs (or a grid of a handful of blocks) never spans
// them all.  So before its acquire a reducer looks once, with a compare-and-
// swap that changes nothing, at the previous repetition's ticket counter of
// up to kXfExtraGroups neighbour groups.  A counter that already holds all
// its tickets proves that every member of that episode has released its slab,
// so the reducer's acquire covers those slabs too and it verifies them as
// well; a counter that does not is left alone.  One look, no loop.  These
// extra lines are counted apart (no number of them is expected, so
// lines_verified == lines_expected keeps its meaning) and count towards
// pair coverage; their mismatches are errors like any other.
//
// Atomics sweep (xcd_atomics_kernel): 2 x CUs workgroups add, max, min, xor,
// or and and hash-derived values into `cells` 128-byte lines at agent scope,
// draw one ticket each from a single counter and contend once for a CAS
// claim.  Every total is recomputed on the host with the same generator; the
// f32 operands are integers with a per-cell sum of magnitudes of at most 2^23,
// enforced by the generator, so every order of addition is exact.
//
// Counted, not trusted: ticket counters, episodes, verified words and tickets
// are all counted on the device and compared on the host.  Every index that
// derives from a returned atomic is range-checked before it is an address.
// The poison hook is data only: it XORs bit 0 into the *expected* value.
// ---------------------------------------------------------------------------

constexpr int kXfBlock = 256;
constexpr int kXfLineWords = 16;           // 64-bit words per 128-byte line
constexpr int kXfHalfWords = 8;
constexpr int kXfTicketStride = 32;        // in uint32: one counter per line
constexpr int kXfXccs = 16;                // XCC_ID[3:0]
constexpr int kXfMaxRecords = 4096;
constexpr int kXfMaxBlocks = 1024;
constexpr int kXfStaggerSleeps = 2;        // x s_sleep(127), 64 clocks each unit
constexpr unsigned kXfPoisonPayload = 1u << 0, kXfPoisonHeader = 1u << 1,
                   kXfPoisonAdd32 = 1u << 2, kXfPoisonAdd64 = 1u << 3,
                   kXfPoisonAddF32 = 1u << 4, kXfPoisonMinMax = 1u << 5,
                   kXfPoisonBitwise = 1u << 6, kXfPoisonTickets = 1u << 7,
                   kXfPoisonCas = 1u << 8;
constexpr int kXfPoisonBits = 9;
constexpr uint32_t kXfKindPayload = 0, kXfKindHeader = 1;

// Device-side counters of the hand-off sweep.
constexpr int kXfCtlPayloadErrors = 0, kXfCtlHeaderErrors = 1, kXfCtlClaims = 2,
              kXfCtlEpisodes = 3, kXfCtlHeaderWords = 4, kXfCtlTicketRange = 5,
              kXfCtlWriterRange = 6, kXfCtlWords = 8;
// LDS of the hand-off kernel, one object: the ticket and neighbour-mask
// broadcast, the header words, then per writer XCC the payload words compared
// in the episode's own group, mismatching, and compared in neighbour groups.
constexpr int kXfShTicket = 0, kXfShMask = 1, kXfShHeader = 2, kXfShWords = 3,
              kXfShErrors = 3 + kXfXccs, kXfShExtra = 3 + 2 * kXfXccs,
              kXfShSize = 3 + 3 * kXfXccs;
constexpr int kXfPairWords = 0, kXfPairErrors = 1, kXfPairExtra = 2,
              kXfPairPlanes = 3;
constexpr uint32_t kXfExtraGroups = 2;     // neighbour groups a reducer may add

struct XfRecord {
  uint32_t round, rep, group, member, line, word, writer_xcc, reader_xcc, kind,
      extra;
  uint64_t expected, got;
};

struct XfHandoff {
  uint64_t* slab;
  uint32_t* tickets;       // [reps][G], kXfTicketStride apart
  uint32_t* writer_xcc;    // [reps][blocks]
  unsigned long long* ctl;
  unsigned long long* pair;  // [3][16][16]: words | mismatching | extra words
  XfRecord* records;
  uint64_t seed;
  uint32_t round, reps, group, G, slab_lines, max_records, poison_mask;
  int poison_pair;
};

// the rare path: claim a record slot, as hbm_report does
__device__ __forceinline__ void xf_report(const XfHandoff& a, uint32_t rep,
                                          uint32_t group, uint32_t member,
                                          uint32_t line, uint32_t word,
                                          uint32_t wx, uint32_t rx, uint32_t kind,
                                          uint32_t extra, uint64_t expected,
                                          uint64_t got) {
  const XfRecord r = {a.round, rep, group, member, line, word, wx, rx, kind, extra,
                      expected, got};
  record_log_claim(
      RecordLogView<XfRecord>{&a.ctl[kXfCtlClaims], a.records, a.max_records},
      [&] { return r; });
}

// All waves of a reducer compare every payload half of group `vg` at
// repetition `vrep` with plain 16-byte loads; `plane` is where the compared
// words are counted (the episode's own group, or a neighbour group).
__device__ __forceinline__ void xf_verify_group(const XfHandoff& a, uint32_t* sh,
                                                int plane, uint32_t extra,
                                                uint32_t vrep, uint32_t vg,
                                                uint32_t rx,
                                                uint32_t& writer_range) {
  const uint32_t blocks = a.group * a.G;
  const uint32_t slab_vecs = a.slab_lines * 4;
  const uint32_t group_vecs = a.group * slab_vecs;
  for (uint32_t v = threadIdx.x; v < group_vecs; v += kXfBlock) {
    const uint32_t m = v / slab_vecs, rem = v % slab_vecs;
    const uint32_t line = rem >> 2, w = kXfHalfWords + (rem & 3) * 2;
    const uint32_t blk = vg + m * a.G;
    const uint32_t wx = a.writer_xcc[(size_t)vrep * blocks + blk];
    const uint64_t idx =
        xf_line_index(blocks, a.slab_lines, vrep, blk, line) * kXfLineWords + w;
    const u64x2 got = *reinterpret_cast<const u64x2*>(a.slab + idx);
    if (wx >= (uint32_t)kXfXccs) {  // guarded before it indexes anything
      if ((rem & 3) == 0 && line == 0) ++writer_range;
      continue;
    }
    // test hook: data only, flips bit 0 of the *expected* words
    const uint64_t px =
        ((a.poison_mask & kXfPoisonPayload) &&
         (a.poison_pair < 0 || (uint32_t)a.poison_pair == ((wx << 4) | rx)))
            ? 1ull : 0ull;
    uint32_t bad = 0;
    for (int k = 0; k < 2; ++k) {
      const uint64_t want = xf_payload_word(a.seed, a.round, idx + k) ^ px;
      if (got[k] != want) {
        ++bad;
        xf_report(a, vrep, vg, m, line, w + k, wx, rx, kXfKindPayload, extra,
                  want, got[k]);
      }
    }
    atomicAdd(&sh[plane + wx], 2u);
    if (bad) atomicAdd(&sh[kXfShErrors + wx], bad);
  }
}

// The j-th neighbour group of episode (round, rep, g): never g itself, and a
// different one every repetition and round.  Needs G > 1.
__device__ __forceinline__ uint32_t xf_neighbour(const XfHandoff& a, uint32_t rep,
                                                 uint32_t g, uint32_t j) {
  return (g + 1 + (j + kXfExtraGroups * (rep + a.round)) % (a.G - 1)) % a.G;
}

// A fixed idle time of a few microseconds, the same for every caller.
__device__ __forceinline__ void xf_stagger() {
  for (int i = 0; i < kXfStaggerSleeps; ++i) __builtin_amdgcn_s_sleep(127);
}

__global__ void __launch_bounds__(kXfBlock) xcd_handoff_kernel(XfHandoff a) {
#if defined(__gfx950__)
  __shared__ uint32_t sh[kXfShSize];
  const uint32_t tid = threadIdx.x;
  const uint32_t rx = __builtin_amdgcn_s_getreg(kCovHwRegXccId) & (kXfXccs - 1);
  const uint32_t blocks = a.group * a.G;  // the host launches exactly this grid
  const uint32_t b = blockIdx.x;
  const uint32_t member = b / a.G, g = b % a.G;
  const uint32_t slab_vecs = a.slab_lines * 4;  // 16-byte vectors per half slab
  const uint32_t group_vecs = a.group * slab_vecs;
  // test hook: data only, flips bit 0 of the *expected* words
  const uint64_t px_header =
      ((a.poison_mask & kXfPoisonHeader) &&
       (a.poison_pair < 0 ||
        (uint32_t)(a.poison_pair & (kXfXccs - 1)) == rx))
          ? 1ull : 0ull;
  uint32_t episodes = 0, ticket_range = 0, writer_range = 0, header_bad = 0,
           header_words = 0;

  if (tid < kXfShSize) sh[tid] = 0;
  __syncthreads();

  for (uint32_t rep = 0; rep < a.reps; ++rep) {
    // 1. pre-touch: the static halves of the whole group, nobody writes them
    for (uint32_t v = tid; v < group_vecs; v += kXfBlock) {
      const uint32_t m = v / slab_vecs, rem = v % slab_vecs;
      const uint32_t line = rem >> 2, w = (rem & 3) * 2;
      const uint64_t idx =
          xf_line_index(blocks, a.slab_lines, rep, g + m * a.G, line) *
              kXfLineWords + w;
      const u64x2 got = *reinterpret_cast<const u64x2*>(a.slab + idx);
      header_words += 2;
      for (int k = 0; k < 2; ++k) {
        const uint64_t want = xf_static_word(a.seed, idx + k) ^ px_header;
        if (got[k] != want) {
          ++header_bad;
          // a static word has no device writer: writer_xcc is 0xFFFFFFFF
          xf_report(a, rep, g, m, line, w + k, 0xFFFFFFFFu, rx, kXfKindHeader,
                    0u, want, got[k]);
        }
      }
    }

    // 2. write the payload halves of this block's own slab, and who wrote it
    if (tid < slab_vecs) {
      const uint32_t line = tid >> 2, w = kXfHalfWords + (tid & 3) * 2;
      const uint64_t idx =
          xf_line_index(blocks, a.slab_lines, rep, b, line) * kXfLineWords + w;
      u64x2 p;
      p[0] = xf_payload_word(a.seed, a.round, idx);
      p[1] = xf_payload_word(a.seed, a.round, idx + 1);
      *reinterpret_cast<u64x2*>(a.slab + idx) = p;
    }
    if (tid == 0) a.writer_xcc[(size_t)rep * blocks + b] = rx;

    // 3. release and ticket: every wave drains its stores, one lane writes the
    // L2 back, waits for that itself, and only then draws the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // stagger (see above): one member per episode idles before its ticket,
      // the others after theirs, so nobody falls behind from rep to rep
      const bool late = member == (rep + a.round) % a.group;
      if (late) xf_stagger();
      const uint32_t t = __hip_atomic_fetch_add(
          &a.tickets[((size_t)rep * a.G + g) * kXfTicketStride], 1u,
          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!late) xf_stagger();
      if (t == a.group - 1) {  // 4. the last arriver acquires for the workgroup
        // one look, no loop: a neighbour group whose previous episode already
        // holds all its tickets has released all its slabs, so the acquire
        // below covers them too; one that does not is simply left out
        uint32_t mask = 0;
        if (rep > 0 && a.G > 1) {
          const uint32_t n = a.G - 1 < kXfExtraGroups ? a.G - 1 : kXfExtraGroups;
          for (uint32_t j = 0; j < n; ++j) {
            const uint32_t g2 = xf_neighbour(a, rep, g, j);
            if (atomicCAS(&a.tickets[((size_t)(rep - 1) * a.G + g2) *
                                     kXfTicketStride],
                          a.group, a.group) == a.group)
              mask |= 1u << j;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        sh[kXfShMask] = mask;
      }
      sh[kXfShTicket] = t;
    }
    __syncthreads();
    const uint32_t ticket = sh[kXfShTicket];
    if (ticket >= a.group) {  // never used for anything but this count
      if (tid == 0) ++ticket_range;
      continue;
    }
    if (ticket != a.group - 1) continue;  // everyone else goes on

    xf_verify_group(a, sh, kXfShWords, 0u, rep, g, rx, writer_range);
    const uint32_t mask = sh[kXfShMask];
    for (uint32_t j = 0; j < kXfExtraGroups; ++j)
      if (mask & (1u << j))
        xf_verify_group(a, sh, kXfShExtra, 1u, rep - 1,
                        xf_neighbour(a, rep, g, j), rx, writer_range);
    if (tid == 0) ++episodes;
  }

  // one flush per workgroup: its reader XCC is the same for every episode
  atomicAdd(&sh[kXfShHeader], header_words);
  if (header_bad)
    atomicAdd(&a.ctl[kXfCtlHeaderErrors], (unsigned long long)header_bad);
  if (writer_range)
    atomicAdd(&a.ctl[kXfCtlWriterRange], (unsigned long long)writer_range);
  __syncthreads();
  if (tid < (uint32_t)kXfXccs) {
    const uint32_t words = sh[kXfShWords + tid], errs = sh[kXfShErrors + tid];
    const uint32_t extra = sh[kXfShExtra + tid];
    constexpr int kPlane = kXfXccs * kXfXccs;
    const uint32_t at = tid * kXfXccs + rx;
    if (words)
      atomicAdd(&a.pair[kXfPairWords * kPlane + at], (unsigned long long)words);
    if (extra)
      atomicAdd(&a.pair[kXfPairExtra * kPlane + at], (unsigned long long)extra);
    if (errs) {
      atomicAdd(&a.pair[kXfPairErrors * kPlane + at], (unsigned long long)errs);
      atomicAdd(&a.ctl[kXfCtlPayloadErrors], (unsigned long long)errs);
    }
  }
  if (tid == 0) {
    atomicAdd(&a.ctl[kXfCtlHeaderWords], (unsigned long long)sh[kXfShHeader]);
    if (episodes)
      atomicAdd(&a.ctl[kXfCtlEpisodes], (unsigned long long)episodes);
    if (ticket_range)
      atomicAdd(&a.ctl[kXfCtlTicketRange], (unsigned long long)ticket_range);
  }
#endif
}

// One target of the atomics sweep: every operand on the same 128-byte line.
struct alignas(128) XfCell {
  unsigned long long add64, max64, min64;
  uint32_t add32;
  float addf;
  uint32_t x, o, a, claim, confirm;
};
static_assert(sizeof(XfCell) == 128, "one cell per 128-byte line");

constexpr int kXfActlTicketRange = 0, kXfActlWords = 2;

struct XfAtomics {
  XfCell* cells;
  uint32_t* ticket;        // one counter on its own line
  uint32_t* seen;          // [total]
  uint32_t* adders;        // [16] waves per XCC
  unsigned long long* ctl;
  uint64_t seed;
  uint32_t reps, ncells, total;
};

__global__ void __launch_bounds__(kXfBlock) xcd_atomics_kernel(XfAtomics a) {
#if defined(__gfx950__)
  const uint32_t id = blockIdx.x * kXfBlock + threadIdx.x;
  if (id >= a.total) return;  // the host launches exactly total threads
  for (uint32_t rep = 0; rep < a.reps; ++rep) {
    XfCell* c = &a.cells[(id + rep) % a.ncells];
    const XfAtomVals v = xf_atom_vals(a.seed, id, rep);
    __hip_atomic_fetch_add(&c->add32, v.add32, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&c->add64, (unsigned long long)v.add64,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsafeAtomicAdd(&c->addf, (float)v.addf);  // the hardware f32 add
    __hip_atomic_fetch_max(&c->max64, (unsigned long long)v.mm, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(&c->min64, (unsigned long long)v.mm, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_xor(&c->x, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_or(&c->o, v.o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_and(&c->a, v.a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // returning add: a ticket is an index only after its range check
  const uint32_t t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
  if (t < a.total)
    a.seen[t] = id + 1;
  else
    atomicAdd(&a.ctl[kXfActlTicketRange], 1ull);
  // single-shot CAS: one attempt, the winner confirms
  XfCell* k = &a.cells[id % a.ncells];
  if (atomicCAS(&k->claim, 0u, id + 1) == 0u) k->confirm = id + 1;
  if ((threadIdx.x & 63) == 0)
    atomicAdd(&a.adders[__builtin_amdgcn_s_getreg(kCovHwRegXccId) & (kXfXccs - 1)],
              1u);
#endif
}

struct XfShape {
  int reps, group, slab_lines, cells, blocks, max_rounds, max_records;
  unsigned poison_mask;
  int poison_pair;
};

// every argument is validated here, before the first HIP call
static void xf_validate(const std::string& who, const XfShape& s) {
  require_range(who, "reps", s.reps, 1, 64);
  require_range(who, "group", s.group, 2, 64);
  require_range(who, "slab_lines", s.slab_lines, 1, 32);
  require_range(who, "cells", s.cells, 1, 4096);
  if (s.blocks < 0 || s.blocks > kXfMaxBlocks ||
      (s.blocks > 0 && s.blocks % s.group != 0))
    throw std::invalid_argument(
        who + ": blocks must be 0 (derive from the device) or a positive "
              "multiple of group, at most 1024");
  require_range(who, "max_rounds", s.max_rounds, 2, 64);
  require_range(who, "max_records", s.max_records, 1, kXfMaxRecords);
  if (s.poison_mask >= (1u << kXfPoisonBits))
    throw std::invalid_argument(who + ": poison_mask has 9 bits");
  if (s.poison_pair < -1 || s.poison_pair > 0xFF)
    throw std::invalid_argument(
        who + ": poison_pair is -1 or writer_xcc << 4 | reader_xcc");
}

static py::dict xf_expected_dict(const XfAtomExpected& e) {
  py::dict d;
  d["add_u32"] = e.add32;
  d["add_u64"] = e.add64;
  std::vector<double> f(e.addf.begin(), e.addf.end());
  d["add_f32"] = f;
  d["max_u64"] = e.max64;
  d["min_u64"] = e.min64;
  d["xor_u32"] = e.x;
  d["or_u32"] = e.o;
  d["and_u32"] = e.a;
  return d;
}

// host only: no HIP call
static py::dict xcd_fabric_reference(int blocks, uint64_t seed, int reps,
                                     int group, int slab_lines, int cells,
                                     int round, int rep, int block, int line,
                                     uint64_t threads) {
  const XfShape s = {reps, group, slab_lines, cells, blocks, 2, 1, 0u, -1};
  xf_validate("xcd_fabric_reference", s);
  if (blocks < 1)
    throw std::invalid_argument("xcd_fabric_reference: blocks must be given");
  require_range("xcd_fabric_reference", "round", round, -1, 63);
  if (rep < 0 || rep >= reps || block < 0 || block >= blocks || line < 0 ||
      line >= slab_lines)
    throw std::invalid_argument(
        "xcd_fabric_reference: rep, block or line out of the shape");
  if (threads > (1ull << 22))
    throw std::invalid_argument("xcd_fabric_reference: threads is at most 2^22");
  const uint64_t first =
      xf_line_index((uint32_t)blocks, (uint32_t)slab_lines, (uint32_t)rep,
                    (uint32_t)block, (uint32_t)line) * kXfLineWords;
  std::vector<uint64_t> header(kXfHalfWords), payload(kXfHalfWords);
  for (int w = 0; w < kXfHalfWords; ++w) {
    header[w] = xf_static_word(seed, first + w);
    payload[w] = xf_payload_word(seed, round, first + kXfHalfWords + w);
  }
  py::dict out;
  out["first_word"] = first;
  out["header"] = header;
  out["payload"] = payload;
  out["member"] = block / (blocks / group);
  out["group_index"] = block % (blocks / group);
  if (threads > 0)
    out["atomics"] = xf_expected_dict(xf_atom_expected(seed, threads, reps, cells));
  else
    out["atomics"] = py::none();
  return out;
}

static void xf_mismatch(py::list& out, const char* comparison, const char* op,
                        int cell, py::object expected, py::object got) {
  py::dict e;
  e["comparison"] = comparison;
  e["op"] = op;
  e["cell"] = cell;
  e["expected"] = expected;
  e["got"] = got;
  out.append(e);
}

static py::dict xf_run_atomics(int cus, const XfShape& s, uint64_t seed,
                               double& elapsed_ms) {
  const uint32_t grid = 2u * (uint32_t)cus;
  const uint32_t total = grid * kXfBlock;
  // throws when the f32 bound does not hold for this device's thread count
  const XfAtomExpected e = xf_atom_expected(seed, total, s.reps, s.cells);

  std::vector<XfCell> cells((size_t)s.cells);
  std::memset(cells.data(), 0, sizeof(XfCell) * cells.size());
  for (XfCell& c : cells) {
    c.min64 = ~0ull;
    c.a = ~0u;
  }
  DeviceBuf<XfCell> d_cells(cells.size());
  DeviceBuf<uint32_t> d_ticket(kXfTicketStride);  // a 128-byte line of its own
  DeviceBuf<uint32_t> d_seen(total), d_adders(kXfXccs);
  DeviceBuf<unsigned long long> d_ctl(kXfActlWords);
  d_cells.upload(cells.data(), cells.size());
  d_ticket.fill(0);
  d_seen.fill(0);
  d_adders.fill(0);
  d_ctl.fill(0);
  EventTimer timer;

  XfAtomics a;
  a.cells = d_cells.get();
  a.ticket = d_ticket.get();
  a.seen = d_seen.get();
  a.adders = d_adders.get();
  a.ctl = d_ctl.get();
  a.seed = seed;
  a.reps = (uint32_t)s.reps;
  a.ncells = (uint32_t)s.cells;
  a.total = total;
  const float ms = timer.time_ms([&] {
    hipLaunchKernelGGL(xcd_atomics_kernel, dim3(grid), dim3(kXfBlock), 0, 0, a);
    HIP_CHECK(hipGetLastError());
  });
  elapsed_ms += ms;

  std::vector<uint32_t> seen(total), adders(kXfXccs);
  uint32_t counter = 0;
  unsigned long long ctl[kXfActlWords];
  d_cells.download(cells.data(), cells.size());
  d_seen.download(seen.data(), seen.size());
  d_adders.download(adders.data(), adders.size());
  d_ticket.download(&counter, 1);
  d_ctl.download(ctl, kXfActlWords);

  // test hook: data only, bit 0 of the expected value
  const auto px = [&](unsigned bit) { return (s.poison_mask & bit) ? 1u : 0u; };
  py::list mism;
  XfAtomExpected g = e;  // same shape, filled with what the device holds
  std::vector<double> got_f((size_t)s.cells);
  std::vector<uint32_t> claims((size_t)s.cells), confirms((size_t)s.cells);
  for (int c = 0; c < s.cells; ++c) {
    const XfCell& k = cells[(size_t)c];
    g.add32[c] = k.add32;
    g.add64[c] = k.add64;
    g.max64[c] = k.max64;
    g.min64[c] = k.min64;
    g.x[c] = k.x;
    g.o[c] = k.o;
    g.a[c] = k.a;
    got_f[c] = (double)k.addf;
    claims[c] = k.claim;
    confirms[c] = k.confirm;
    const uint32_t w32 = e.add32[c] ^ px(kXfPoisonAdd32);
    if (k.add32 != w32)
      xf_mismatch(mism, "add_u32", "add_u32", c, py::int_(w32), py::int_(k.add32));
    const uint64_t w64 = e.add64[c] ^ (uint64_t)px(kXfPoisonAdd64);
    if (k.add64 != w64)
      xf_mismatch(mism, "add_u64", "add_u64", c, py::int_(w64), py::int_(k.add64));
    const uint32_t wf = f32_bits((float)e.addf[c]) ^ px(kXfPoisonAddF32);
    if (f32_bits(k.addf) != wf) {
      float want;
      std::memcpy(&want, &wf, sizeof(want));
      xf_mismatch(mism, "add_f32", "add_f32", c, py::float_((double)want),
                  py::float_((double)k.addf));
    }
    const uint64_t wmax = e.max64[c] ^ (uint64_t)px(kXfPoisonMinMax);
    const uint64_t wmin = e.min64[c] ^ (uint64_t)px(kXfPoisonMinMax);
    if (k.max64 != wmax)
      xf_mismatch(mism, "minmax", "max_u64", c, py::int_(wmax), py::int_(k.max64));
    if (k.min64 != wmin)
      xf_mismatch(mism, "minmax", "min_u64", c, py::int_(wmin), py::int_(k.min64));
    const uint32_t pb = px(kXfPoisonBitwise);
    if (k.x != (e.x[c] ^ pb))
      xf_mismatch(mism, "bitwise", "xor_u32", c, py::int_(e.x[c] ^ pb), py::int_(k.x));
    if (k.o != (e.o[c] ^ pb))
      xf_mismatch(mism, "bitwise", "or_u32", c, py::int_(e.o[c] ^ pb), py::int_(k.o));
    if (k.a != (e.a[c] ^ pb))
      xf_mismatch(mism, "bitwise", "and_u32", c, py::int_(e.a[c] ^ pb), py::int_(k.a));
    // the winner of slot c is some thread id with id % cells == c
    const bool contested = (uint32_t)c < total;
    const uint32_t want_confirm = k.claim ^ px(kXfPoisonCas);
    const bool claim_ok =
        contested ? (k.claim != 0 && k.claim <= total &&
                     (k.claim - 1) % (uint32_t)s.cells == (uint32_t)c)
                  : k.claim == 0;
    if (!claim_ok || k.confirm != want_confirm)
      xf_mismatch(mism, "cas", "cas", c, py::int_(want_confirm),
                  py::int_(k.confirm));
  }
  // every ticket drawn exactly once: counter == total and no hole in seen
  uint64_t missing = 0, seen_range = 0;
  for (uint32_t t = 0; t < total; ++t) {
    missing += seen[t] == 0;
    seen_range += seen[t] > total;
  }
  const uint32_t want_total = total ^ px(kXfPoisonTickets);
  if (counter != want_total)
    xf_mismatch(mism, "tickets", "tickets", -1, py::int_(want_total),
                py::int_(counter));

  py::dict got = xf_expected_dict(g);
  got["add_f32"] = got_f;
  py::dict out;
  out["workgroups"] = grid;
  out["threads"] = total;
  out["totals"] = got;
  out["expected"] = xf_expected_dict(e);
  out["mismatches"] = mism;
  out["ticket_counter"] = counter;
  out["tickets_expected"] = total;
  out["tickets_missing"] = missing;
  out["tickets_out_of_range"] = ctl[kXfActlTicketRange] + seen_range;
  out["claims"] = claims;
  out["confirms"] = confirms;
  out["adders_per_xcc"] = adders;
  out["ms"] = (double)ms;
  return out;
}

static py::dict xcd_fabric_check(int device, int reps, int group, int slab_lines,
                                 int cells, int blocks, int max_rounds,
                                 uint64_t seed, int max_records,
                                 unsigned poison_mask, int poison_pair) {
  const XfShape s = {reps, group, slab_lines, cells, blocks, max_rounds,
                     max_records, poison_mask, poison_pair};
  xf_validate("xcd_fabric_check", s);

  const int cus = select_device("xcd_fabric_check", device).multiProcessorCount;
  // G: the largest odd number with group x G <= 2 x CUs (at least one group)
  int G = blocks > 0 ? blocks / group : (2 * cus) / group;
  if (blocks == 0) {
    if (G < 1) G = 1;
    if ((G & 1) == 0) --G;
  }
  const uint32_t nblocks = (uint32_t)(group * G);
  const size_t lines = (size_t)reps * nblocks * (size_t)slab_lines;
  const size_t slab_words = lines * kXfLineWords;
  const size_t n_tickets = (size_t)reps * (size_t)G;
  const size_t writer_count = (size_t)reps * nblocks;
  constexpr size_t kPlane = (size_t)kXfXccs * kXfXccs;

  // the initial upload plays round -1
  std::vector<uint64_t> h_slab(slab_words);
  for (size_t i = 0; i < slab_words; ++i)
    h_slab[i] = (i % kXfLineWords) < (size_t)kXfHalfWords
                    ? xf_static_word(seed, i)
                    : xf_payload_word(seed, -1, i);

  DeviceBuf<uint64_t> d_slab(slab_words);
  DeviceBuf<uint32_t> d_tickets(n_tickets * kXfTicketStride);
  DeviceBuf<uint32_t> d_writer(writer_count);
  DeviceBuf<unsigned long long> d_pair(kXfPairPlanes * kPlane);
  RecordLog<XfRecord> log((size_t)max_records, kXfCtlWords, kXfCtlClaims);
  d_slab.upload(h_slab.data(), slab_words);
  d_writer.fill(0xFF);
  d_pair.fill(0);
  EventTimer timer;

  std::vector<uint32_t> h_tickets(d_tickets.size());
  std::vector<uint32_t> h_writer(writer_count);
  std::vector<unsigned long long> h_pair(d_pair.size());
  std::vector<uint64_t> writes_per_xcc(kXfXccs, 0);
  uint64_t ticket_counter_errors = 0, writer_host_range = 0;
  int rounds = 0, pairs_covered = 0, xcc_seen = 0;
  unsigned xcc_mask = 0;
  double elapsed_ms = 0.0;
  py::list round_ms;
  const RecordLogView<XfRecord> log_view = log.view((size_t)max_records);
  while (rounds < max_rounds) {
    XfHandoff a;
    a.slab = d_slab.get();
    a.tickets = d_tickets.get();
    a.writer_xcc = d_writer.get();
    a.ctl = log.ctl();
    a.pair = d_pair.get();
    a.records = log_view.records;
    a.seed = seed;
    a.round = (uint32_t)rounds;
    a.reps = (uint32_t)reps;
    a.group = (uint32_t)group;
    a.G = (uint32_t)G;
    a.slab_lines = (uint32_t)slab_lines;
    a.max_records = log_view.cap;
    a.poison_mask = poison_mask;
    a.poison_pair = poison_pair;
    const float ms = timer.time_ms([&] {
      // the ticket counters are zeroed on the launch stream ahead of every launch
      d_tickets.fill_async(0);
      hipLaunchKernelGGL(xcd_handoff_kernel, dim3(nblocks), dim3(kXfBlock), 0, 0, a);
      HIP_CHECK(hipGetLastError());
    });
    elapsed_ms += ms;
    round_ms.append((double)ms);
    ++rounds;

    d_tickets.download(h_tickets.data(), h_tickets.size());
    d_writer.download(h_writer.data(), h_writer.size());
    d_pair.download(h_pair.data(), h_pair.size());
    for (size_t t = 0; t < n_tickets; ++t)
      ticket_counter_errors += h_tickets[t * kXfTicketStride] != (uint32_t)group;
    for (uint32_t wx : h_writer) {
      if (wx < (uint32_t)kXfXccs) {
        ++writes_per_xcc[wx];
        xcc_mask |= 1u << wx;
      } else {
        ++writer_host_range;
      }
    }
    pairs_covered = 0;
    for (int w = 0; w < kXfXccs; ++w)
      for (int r = 0; r < kXfXccs; ++r)
        if (h_pair[kXfPairWords * kPlane + (size_t)w * kXfXccs + r] != 0 ||
            h_pair[kXfPairExtra * kPlane + (size_t)w * kXfXccs + r] != 0) {
          ++pairs_covered;
          xcc_mask |= (1u << w) | (1u << r);
        }
    xcc_seen = __builtin_popcount(xcc_mask);
    if (rounds >= 2 && pairs_covered >= xcc_seen * xcc_seen) break;
  }

  const auto taken = log.collect((size_t)max_records);
  const std::vector<unsigned long long>& ctl = taken.ctl;

  py::dict atomics = xf_run_atomics(cus, s, seed, elapsed_ms);

  py::list records;
  for (const XfRecord& r : taken.records) {
    py::dict e;
    const bool payload = r.kind == kXfKindPayload;
    const uint64_t idx =
        xf_line_index(nblocks, (uint32_t)slab_lines, r.rep,
                      r.group + r.member * (uint32_t)G, r.line) * kXfLineWords +
        r.word;
    e["round"] = r.round;
    e["rep"] = r.rep;
    e["group"] = r.group;
    e["member"] = r.member;
    e["block"] = r.group + r.member * (uint32_t)G;
    e["line"] = r.line;
    e["word"] = r.word;
    e["writer_xcc"] = payload ? py::object(py::int_(r.writer_xcc)) : py::none();
    e["reader_xcc"] = r.reader_xcc;
    e["kind"] = payload ? "payload" : "header";
    e["extra"] = r.extra != 0;
    e["expected"] = r.expected;
    e["got"] = r.got;
    // what a hand-off that never happened would have read
    e["stale"] = payload &&
                 r.got == xf_payload_word(seed, (int64_t)r.round - 1, idx);
    records.append(e);
  }
  py::list pairs;
  uint64_t words_verified = 0, extra_words = 0;
  for (int w = 0; w < kXfXccs; ++w)
    for (int r = 0; r < kXfXccs; ++r) {
      const size_t at = (size_t)w * kXfXccs + r;
      const uint64_t words = h_pair[kXfPairWords * kPlane + at];
      const uint64_t errs = h_pair[kXfPairErrors * kPlane + at];
      const uint64_t extra = h_pair[kXfPairExtra * kPlane + at];
      if (words == 0 && errs == 0 && extra == 0) continue;
      py::dict e;
      e["writer_xcc"] = w;
      e["reader_xcc"] = r;
      e["words"] = words;
      e["lines"] = words / kXfHalfWords;
      e["extra_lines"] = extra / kXfHalfWords;
      e["errors"] = errs;
      pairs.append(e);
      words_verified += words;
      extra_words += extra;
    }
  py::list xcc_ids;
  for (int x = 0; x < kXfXccs; ++x)
    if (xcc_mask & (1u << x)) xcc_ids.append(x);

  const uint64_t episodes_per_round = (uint64_t)reps * (uint64_t)G;
  const uint64_t group_lines = (uint64_t)group * (uint64_t)slab_lines;
  py::dict out;
  out["compute_units"] = cus;
  out["seed"] = seed;
  out["reps"] = reps;
  out["group"] = group;
  out["groups"] = G;
  out["blocks"] = nblocks;
  out["slab_lines"] = slab_lines;
  out["cells"] = cells;
  out["rounds"] = rounds;
  out["max_rounds"] = max_rounds;
  out["round_ms"] = round_ms;
  out["episodes_completed"] = ctl[kXfCtlEpisodes];
  out["episodes_expected"] = (uint64_t)rounds * episodes_per_round;
  out["lines_verified"] = words_verified / kXfHalfWords;
  out["lines_expected"] = (uint64_t)rounds * episodes_per_round * group_lines;
  out["extra_lines_verified"] = extra_words / kXfHalfWords;
  out["header_lines_verified"] = ctl[kXfCtlHeaderWords] / kXfHalfWords;
  out["header_lines_expected"] =
      (uint64_t)rounds * (uint64_t)reps * nblocks * group_lines;
  out["payload_errors"] = ctl[kXfCtlPayloadErrors];
  out["header_errors"] = ctl[kXfCtlHeaderErrors];
  out["error_count"] = ctl[kXfCtlPayloadErrors] + ctl[kXfCtlHeaderErrors];
  out["ticket_counter_errors"] = ticket_counter_errors;
  out["tickets_out_of_range"] = ctl[kXfCtlTicketRange];
  out["writer_xcc_out_of_range"] = ctl[kXfCtlWriterRange] + writer_host_range;
  out["pairs"] = pairs;
  out["pairs_covered"] = pairs_covered;
  out["xcc_seen"] = xcc_seen;
  out["xcc_ids"] = xcc_ids;
  out["writes_per_xcc"] = writes_per_xcc;
  out["records"] = records;
  out["records_dropped"] = taken.claims - (uint64_t)taken.records.size();
  out["atomics"] = atomics;
  out["elapsed_ms"] = elapsed_ms;
  return out;
}

// ---------------------------------------------------------------------------
// LDS data-integrity check.  One 256-thread workgroup claims all 160 KiB of a
// CU's Local Data Share as one static array, so exactly one workgroup fits on
// a CU, and runs `reps` repetitions of six phases over it (generators and the
// layouts in lds_problems.hpp):
//   bit 0 pattern    moving inversions over all 40960 words: `passes` hash
//                    patterns and one checker, each as fill p / verify p and
//                    write ~p / verify ~p, the three steps in three different
//                    widths out of b32, b64, b128, rotated per pattern
//   bit 1 subword    every word assembled over its inverse from four byte
//                    stores or two 16-bit stores issued by different waves,
//                    verified as b32 and read back as u8 / u16
//   bit 2 transpose  the whole array read with ds_read_b64_tr_b16 as 4 x 16
//                    blocks, under 64-byte and under 160-byte rows
//   bit 3 dma        the whole array filled by direct global->LDS loads, half
//                    16 bytes and half 4 bytes per lane, from permuted source
//                    addresses; verified with ordinary reads
//   bit 4 atomics    the LDS ALU: u32 / u64 / f32 add, u32 max / min, xor, or,
//                    and, one compare-and-swap claim per cell
//   bit 5 permute    ds_bpermute_b32 / ds_permute_b32 with lane permutations
//                    that change every step
//
// A step splits the array into 160 chunks of 1 KiB; chunk c of step s belongs
// to wave (c + s) % 4 and s advances with every step, so a word is always
// verified by another wave than the one that wrote it.  Workgroup barriers
// separate the steps.  The whole array is in use, so nothing is reduced
// through LDS: fail masks go through ballots, counts through lane shuffles,
// and both through global atomics once per wave at the end.
//
// Grid, placement key, bounded relaunch and the fixed amount of work per
// workgroup are those of cu_coverage_kernel; coverage is per CU, LDS belongs
// to the CU.  The poison hook is data only: it XORs into the *expected*
// values and never alters LDS, so a record's `got` is real LDS content.
// ---------------------------------------------------------------------------

constexpr int kLdsCtlErrors = 0, kLdsCtlXor = 1, kLdsCtlClaims = 2,
              kLdsCtlWords = 4;
constexpr int kLdsKeyPlanes = 4;  // workgroups | fail | hw_id | xcc_id

struct LdsRecord {
  uint32_t key, block, rep, phase, detail, word;
  uint64_t expected, got;
};

struct LdsLaunch {
  const uint32_t* src;           // kLdsWords words, the source of the dma phase
  uint32_t* keys;                // [kLdsKeyPlanes][kCovKeys]
  unsigned long long* ctl;
  unsigned long long* counters;  // [kLdsPhases] items compared
  LdsRecord* records;
  uint64_t seed;
  uint32_t reps, passes, max_records, poison_mask, poison_xor;
  int poison_key, poison_all, poison_word;
};

struct LdsLane {
  uint32_t key, block, rep, pm;
  int tid, lane, wave;
  uint32_t fail, bad;
  uint64_t bad_xor;
  uint32_t compared[kLdsPhases];
};

using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using s16x4 = __attribute__((ext_vector_type(4))) short;

#if defined(__gfx950__)
// the rare path: count the mismatch and, while slots are left, claim a record
// (by value and out of line: the lane's counters stay in registers)
__device__ __noinline__ void lds_record(unsigned long long* ctl, LdsRecord* records,
                                        uint32_t max_records, LdsRecord r) {
  const RecordLogView<LdsRecord> log = {&ctl[kLdsCtlClaims], records, max_records};
  if (__hip_atomic_load(log.claims, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <
      log.cap)  // a full log is left alone: no atomic per further mismatch
    record_log_claim(log, [&] { return r; });
}

__device__ __forceinline__ void lds_check(const LdsLaunch& a, LdsLane& st,
                                          int phase, uint32_t detail,
                                          uint32_t word, uint64_t expected,
                                          uint64_t got) {
  ++st.compared[phase];
  if (expected != got) {
    ++st.bad;
    st.bad_xor |= expected ^ got;
    st.fail |= 1u << phase;
    const LdsRecord r = {st.key, st.block, st.rep, (uint32_t)phase, detail, word,
                         expected, got};
    lds_record(a.ctl, a.records, a.max_records, r);
  }
}

// first word of the j-th chunk (j < 40) of this wave in step s
__device__ __forceinline__ uint32_t lds_chunk(const LdsLane& st, uint32_t s, int j) {
  return ((((uint32_t)st.wave - s) & 3u) + 4u * (uint32_t)j) * kLdsChunkWords;
}

// One step of a moving-inversions pattern in W-word accesses.  KIND 0 fills
// with p, 1 verifies p and writes ~p, 2 verifies ~p.
template <int W, int KIND>
__device__ __forceinline__ void lds_pattern_step(uint32_t* lds, const LdsLaunch& a,
                                                 LdsLane& st, int pat, uint32_t s) {
  const uint32_t inv = KIND == 2 ? ~0u : 0u, winv = KIND == 1 ? ~0u : 0u;
  const bool poisoned = (st.pm >> kLdsPhasePattern) & 1u;
#pragma unroll 1
  for (int j = 0; j < kLdsChunks / 4; ++j) {
    const uint32_t c0 = lds_chunk(st, s, j);
#pragma unroll
    for (int it = 0; it < 4 / W; ++it) {
      const uint32_t w0 = c0 + (uint32_t)(it * 64 + st.lane) * W;
      uint32_t g[W], p[W];
      for (int k = 0; k < W; ++k)
        p[k] = lds_pattern_word(a.seed, (int)a.passes, st.block, st.rep, pat, w0 + k);
      if (KIND != 0) {
        if constexpr (W == 1) {
          g[0] = lds[w0];
        } else if constexpr (W == 2) {
          const u32x2 v = *reinterpret_cast<const u32x2*>(lds + w0);
          g[0] = v[0];
          g[1] = v[1];
        } else {
          const u32x4 v = *reinterpret_cast<const u32x4*>(lds + w0);
          for (int k = 0; k < 4; ++k) g[k] = v[k];
        }
        for (int k = 0; k < W; ++k) {
          uint32_t want = p[k] ^ inv;
          // test hook: data only, moves the *expected* word
          if (poisoned && (a.poison_word < 0 || (uint32_t)a.poison_word == w0 + k))
            want ^= a.poison_xor;
          lds_check(a, st, kLdsPhasePattern, (uint32_t)(pat * 4 + KIND), w0 + k,
                    want, g[k]);
        }
      }
      if (KIND != 2) {
        if constexpr (W == 1) {
          lds[w0] = p[0] ^ winv;
        } else if constexpr (W == 2) {
          u32x2 v;
          v[0] = p[0] ^ winv;
          v[1] = p[1] ^ winv;
          *reinterpret_cast<u32x2*>(lds + w0) = v;
        } else {
          u32x4 v;
          for (int k = 0; k < 4; ++k) v[k] = p[k] ^ winv;
          *reinterpret_cast<u32x4*>(lds + w0) = v;
        }
      }
    }
  }
  __syncthreads();
}

template <int KIND>
__device__ __forceinline__ void lds_pattern_dispatch(uint32_t* lds,
                                                     const LdsLaunch& a,
                                                     LdsLane& st, int pat,
                                                     uint32_t s) {
  switch (lds_pattern_width(pat, KIND)) {  // uniform
    case 0: lds_pattern_step<1, KIND>(lds, a, st, pat, s); break;
    case 1: lds_pattern_step<2, KIND>(lds, a, st, pat, s); break;
    default: lds_pattern_step<4, KIND>(lds, a, st, pat, s); break;
  }
}

__device__ __forceinline__ void lds_phase_subword(uint32_t* lds, const LdsLaunch& a,
                                                  LdsLane& st, uint32_t& s) {
  const uint32_t px = (st.pm >> kLdsPhaseSubword) & 1u;
  // explicitly LDS pointers: a volatile access through a generic pointer
  // would be a flat instruction
  typedef volatile __attribute__((address_space(3))) uint8_t* lds_b8_t;
  typedef volatile __attribute__((address_space(3))) uint16_t* lds_b16_t;
  const lds_b8_t b8 = (lds_b8_t)lds;
  const lds_b16_t b16 = (lds_b16_t)lds;
  // the background: the inverse of every word
#pragma unroll 1
  for (int j = 0; j < kLdsChunks / 4; ++j)
    for (int it = 0; it < 4; ++it) {
      const uint32_t w = lds_chunk(st, s, j) + (uint32_t)(it * 64 + st.lane);
      lds[w] = ~lds_subword_word(a.seed, st.block, st.rep, w);
    }
  ++s;
  __syncthreads();
  // every wave stores into every chunk: byte k of the words of an even chunk,
  // half k & 1 of words 128 (k >> 1) .. + 127 of an odd one, k its role there
#pragma unroll 1
  for (uint32_t c = 0; c < (uint32_t)kLdsChunks; ++c) {
    const uint32_t k = ((uint32_t)st.wave + c + s) & 3u;
    if ((c & 1u) == 0) {
      for (int it = 0; it < 4; ++it) {
        const uint32_t w = c * kLdsChunkWords + (uint32_t)(it * 64 + st.lane);
        const uint32_t v = lds_subword_word(a.seed, st.block, st.rep, w);
        b8[4 * w + k] = (uint8_t)(v >> (8 * k));
      }
    } else {
      for (int it = 0; it < 2; ++it) {
        const uint32_t w = c * kLdsChunkWords + (k >> 1) * 128u +
                           (uint32_t)(it * 64 + st.lane);
        const uint32_t v = lds_subword_word(a.seed, st.block, st.rep, w);
        b16[2 * w + (k & 1u)] = (uint16_t)(v >> (16 * (k & 1u)));
      }
    }
  }
  ++s;
  __syncthreads();
  // whole words
#pragma unroll 1
  for (int j = 0; j < kLdsChunks / 4; ++j)
    for (int it = 0; it < 4; ++it) {
      const uint32_t w = lds_chunk(st, s, j) + (uint32_t)(it * 64 + st.lane);
      const uint32_t want = lds_subword_word(a.seed, st.block, st.rep, w) ^ px;
      lds_check(a, st, kLdsPhaseSubword, 0u, w, want, lds[w]);
    }
  // and bytes and halves, each read by another wave than the one that stored it
#pragma unroll 1
  for (uint32_t c = 0; c < (uint32_t)kLdsChunks; ++c) {
    const uint32_t k = ((uint32_t)st.wave + c + s + 1u) & 3u;
    if ((c & 1u) == 0) {
      for (int it = 0; it < 4; ++it) {
        const uint32_t w = c * kLdsChunkWords + (uint32_t)(it * 64 + st.lane);
        const uint32_t v = lds_subword_word(a.seed, st.block, st.rep, w) ^ px;
        lds_check(a, st, kLdsPhaseSubword, 1u + k, w, (v >> (8 * k)) & 0xFFu,
                  b8[4 * w + k]);
      }
    } else {
      for (int it = 0; it < 2; ++it) {
        const uint32_t w = c * kLdsChunkWords + (k >> 1) * 128u +
                           (uint32_t)(it * 64 + st.lane);
        const uint32_t v = lds_subword_word(a.seed, st.block, st.rep, w) ^ px;
        lds_check(a, st, kLdsPhaseSubword, 5u + (k & 1u), w,
                  (v >> (16 * (k & 1u))) & 0xFFFFu, b16[2 * w + (k & 1u)]);
      }
    }
  }
  ++s;
  __syncthreads();
}

__device__ __forceinline__ void lds_phase_transpose(uint32_t* lds,
                                                    const LdsLaunch& a, LdsLane& st,
                                                    uint32_t& s) {
  const uint32_t px = (st.pm >> kLdsPhaseTranspose) & 1u;
#pragma unroll 1
  for (int j = 0; j < kLdsChunks / 4; ++j) {
    const uint32_t w0 = lds_chunk(st, s, j) + (uint32_t)st.lane * 4u;
    u32x4 v;
    for (int k = 0; k < 4; ++k)
      v[k] = lds_tr_word(a.seed, st.block, st.rep, w0 + k);
    *reinterpret_cast<u32x4*>(lds + w0) = v;
  }
  ++s;
  __syncthreads();
  // One wave-instruction reads four blocks, one per 16-lane group.  The loops
  // are uniform and every lane holds an in-bounds 8-byte-aligned address, so
  // EXEC is all ones at the read; the compare comes afterwards.
  const uint32_t i = (uint32_t)st.lane & 15u, grp = (uint32_t)st.lane >> 4;
  for (int layout = 0; layout < 2; ++layout) {
    const int R = layout == 0 ? kLdsTrRowBlocks[0] : kLdsTrRowBlocks[1];
#pragma unroll 1
    for (int j = 0; j < kLdsTrBlocks / 16; ++j) {
      const uint32_t n = (((uint32_t)st.wave - s) & 3u) + 4u * (uint32_t)j;
      const uint32_t b = 4u * n + grp;
      const uint32_t off = lds_tr_lane_offset(R, b, i);
      const s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(
              reinterpret_cast<char*>(lds) + off));
      for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t e = lds_tr_expected_elem(R, b, i, q);
        lds_check(a, st, kLdsPhaseTranspose, (uint32_t)layout, e >> 1,
                  lds_tr_elem(a.seed, st.block, st.rep, e) ^ px,
                  (uint32_t)(uint16_t)r[q]);
      }
    }
    ++s;
  }
  __syncthreads();
}

__device__ __forceinline__ void lds_phase_dma(uint32_t* lds, const LdsLaunch& a,
                                              LdsLane& st, uint32_t& s) {
  const uint32_t px = (st.pm >> kLdsPhaseDma) & 1u;
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
#pragma unroll 1
  for (int j = 0; j < kLdsChunks / 4; ++j) {
    const uint32_t c0 = lds_chunk(st, s, j);  // wave-uniform: the LDS base
    if (lds_dma_wide(st.rep, c0 / kLdsChunkWords)) {
      // lane l lands at words 4l .. 4l+3 of the chunk
      const uint32_t src =
          lds_dma_src_index(st.block, st.rep, c0 + 4u * (uint32_t)st.lane);
      __builtin_amdgcn_global_load_lds((gptr_t)(a.src + src), (lptr_t)(lds + c0),
                                       16, 0, 0);
    } else {
      for (uint32_t q = 0; q < 4; ++q) {  // load q, lane l lands at word 64q + l
        const uint32_t src = lds_dma_src_index(
            st.block, st.rep, c0 + 64u * q + (uint32_t)st.lane);
        __builtin_amdgcn_global_load_lds((gptr_t)(a.src + src),
                                         (lptr_t)(lds + c0 + 64u * q), 4, 0, 0);
      }
    }
  }
  ++s;
  // a direct load is a pending LDS write on the vector-memory counter
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll 1
  for (int j = 0; j < kLdsChunks / 4; ++j) {
    const uint32_t w0 = lds_chunk(st, s, j) + (uint32_t)st.lane * 4u;
    const u32x4 g = *reinterpret_cast<const u32x4*>(lds + w0);
    for (int k = 0; k < 4; ++k) {
      // volatile: the source is re-read from global memory, never folded
      const uint32_t want = ((const volatile __attribute__((address_space(1)))
                                  uint32_t*)a.src)[lds_dma_src_index(
          st.block, st.rep, w0 + k)];
      lds_check(a, st, kLdsPhaseDma, 0u, w0 + k, want ^ px, g[k]);
    }
  }
  ++s;
  __syncthreads();
}

__device__ __forceinline__ void lds_phase_atomics(uint32_t* lds, const LdsLaunch& a,
                                                  LdsLane& st) {
  const uint32_t px = (st.pm >> kLdsPhaseAtomics) & 1u;
  const uint32_t tid = (uint32_t)st.tid;
  if (tid < (uint32_t)kLdsAtomCells) {
    const uint32_t base = lds_atom_cell_base(tid);
    for (int f = 0; f <= kLdsCellConfirm; ++f) lds[base + f] = 0u;
    lds[base + kLdsCellMin] = ~0u;
    lds[base + kLdsCellAnd] = ~0u;
  }
  __syncthreads();
  for (uint32_t step = 0; step < (uint32_t)kLdsAtomSteps; ++step) {
    uint32_t* c = lds + lds_atom_cell_base((tid + step) % kLdsAtomCells);
    const LdsAtomVals v = lds_atom_vals(a.seed, st.block, st.rep, tid, step);
    __hip_atomic_fetch_add(c + kLdsCellAdd32, v.add32, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(c + kLdsCellAdd64),
                           (unsigned long long)v.add64, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(reinterpret_cast<float*>(c + kLdsCellAddF),
                           (float)v.addf, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_max(c + kLdsCellMax, v.mm, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_min(c + kLdsCellMin, v.mm, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_xor(c + kLdsCellXor, v.x, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_or(c + kLdsCellOr, v.o, __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_and(c + kLdsCellAnd, v.a, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  {  // single-shot compare-and-swap: one attempt, the winner confirms
    uint32_t* c = lds + lds_atom_cell_base(tid % kLdsAtomCells);
    if (atomicCAS(c + kLdsCellClaim, 0u, tid + 1u) == 0u)
      c[kLdsCellConfirm] = tid + 1u;
  }
  __syncthreads();
  // every wave compares a part of every cell, lane l cell l
  const uint32_t cell = (uint32_t)st.lane;
  const uint32_t base = lds_atom_cell_base(cell);
  const LdsAtomCell e = lds_atom_expected_cell(a.seed, st.block, st.rep, cell);
  if (st.wave == 0) {
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellAdd32, base + kLdsCellAdd32,
              e.add32 ^ px, lds[base + kLdsCellAdd32]);
    const uint64_t got64 = (uint64_t)lds[base + kLdsCellAdd64] |
                           (uint64_t)lds[base + kLdsCellAdd64 + 1] << 32;
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellAdd64, base + kLdsCellAdd64,
              e.add64 ^ px, got64);
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellAddF, base + kLdsCellAddF,
              __float_as_uint((float)e.addf) ^ px, lds[base + kLdsCellAddF]);
  } else if (st.wave == 1) {
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellMax, base + kLdsCellMax,
              e.max32 ^ px, lds[base + kLdsCellMax]);
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellMin, base + kLdsCellMin,
              e.min32 ^ px, lds[base + kLdsCellMin]);
  } else if (st.wave == 2) {
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellXor, base + kLdsCellXor, e.x ^ px,
              lds[base + kLdsCellXor]);
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellOr, base + kLdsCellOr, e.o ^ px,
              lds[base + kLdsCellOr]);
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellAnd, base + kLdsCellAnd, e.a ^ px,
              lds[base + kLdsCellAnd]);
  } else {
    // the winner of cell c is some thread t with t % 64 == c; expected is the
    // cell number where the claim is none
    const uint32_t claim = lds[base + kLdsCellClaim];
    const bool valid = claim >= 1u && claim <= (uint32_t)kLdsBlock &&
                       (claim - 1u) % kLdsAtomCells == cell;
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellClaim, base + kLdsCellClaim,
              (valid ? claim : cell + 1u) ^ px, claim);
    lds_check(a, st, kLdsPhaseAtomics, kLdsCellConfirm, base + kLdsCellConfirm,
              claim ^ px, lds[base + kLdsCellConfirm]);
  }
  __syncthreads();
}

__device__ __forceinline__ void lds_phase_permute(const LdsLaunch& a, LdsLane& st) {
  const uint32_t px = (st.pm >> kLdsPhasePermute) & 1u;
  const uint32_t lane = (uint32_t)st.lane, w0 = (uint32_t)st.wave * 64u;
#pragma unroll 1
  for (uint32_t step = 0; step < (uint32_t)kLdsPermSteps; ++step) {
    const uint32_t map = lds_perm_map(a.seed, st.block, st.rep, step, (uint32_t)st.wave);
    const uint32_t val = lds_perm_value(a.seed, st.block, st.rep, step, w0 + lane);
    const uint32_t to = lds_perm_sigma(map, lane);
    // pull: this lane reads the value of lane sigma(l)
    const uint32_t pulled =
        (uint32_t)__builtin_amdgcn_ds_bpermute((int)(to * 4u), (int)val);
    // push: this lane's value goes to lane sigma(l), so it receives the value
    // of lane sigma^-1(l)
    const uint32_t pushed =
        (uint32_t)__builtin_amdgcn_ds_permute((int)(to * 4u), (int)val);
    lds_check(a, st, kLdsPhasePermute, step * 2u, (uint32_t)st.tid,
              lds_perm_value(a.seed, st.block, st.rep, step, w0 + to) ^ px, pulled);
    lds_check(a, st, kLdsPhasePermute, step * 2u + 1u, (uint32_t)st.tid,
              lds_perm_value(a.seed, st.block, st.rep, step,
                             w0 + lds_perm_sigma_inv(map, lane)) ^ px,
              pushed);
  }
}
#endif  // __gfx950__

// second bound = waves per SIMD: one workgroup per CU
__global__ void __launch_bounds__(kLdsBlock, 1) lds_integrity_kernel(LdsLaunch a) {
#if defined(__gfx950__)
  __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
  const uint32_t hw_id = __builtin_amdgcn_s_getreg(kCovHwRegHwId);
  const uint32_t xcc_id = __builtin_amdgcn_s_getreg(kCovHwRegXccId);
  LdsLane st = {};
  st.key = ((xcc_id & 0xFu) << 8) | ((hw_id >> 8) & 0xFFu);
  st.block = blockIdx.x;
  st.tid = (int)threadIdx.x;
  st.lane = st.tid & 63;
  st.wave = __builtin_amdgcn_readfirstlane(st.tid >> 6);
  // test hook: data only
  st.pm = (a.poison_all || (int)st.key == a.poison_key) ? a.poison_mask : 0u;

  uint32_t s = 0;  // chunk c of step s belongs to wave (c + s) % 4
#pragma unroll 1
  for (uint32_t rep = 0; rep < a.reps; ++rep) {
    st.rep = rep;
#pragma unroll 1
    for (int pat = 0; pat <= (int)a.passes; ++pat) {
      lds_pattern_dispatch<0>(lds, a, st, pat, s++);
      lds_pattern_dispatch<1>(lds, a, st, pat, s++);
      lds_pattern_dispatch<2>(lds, a, st, pat, s++);
    }
    lds_phase_subword(lds, a, st, s);
    lds_phase_transpose(lds, a, st, s);
    lds_phase_dma(lds, a, st, s);
    lds_phase_atomics(lds, a, st);
    lds_phase_permute(a, st);
  }

  // one flush per wave: ballots and shuffles, nothing goes through LDS
  unsigned wave_fail = 0;
  for (int b = 0; b < kLdsPhases; ++b)
    if (__ballot((st.fail >> b) & 1u) != 0) wave_fail |= 1u << b;
  if (st.bad != 0) {  // on a mismatch, and only then
    atomicAdd(&a.ctl[kLdsCtlErrors], (unsigned long long)st.bad);
    atomicOr(&a.ctl[kLdsCtlXor], (unsigned long long)st.bad_xor);
  }
  for (int p = 0; p < kLdsPhases; ++p) {
    uint32_t sum = st.compared[p];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (st.lane == 0) atomicAdd(&a.counters[p], (unsigned long long)sum);
  }
  if (st.lane == 0 && wave_fail)  // key < kCovKeys by the masks above
    atomicOr(&a.keys[kCovKeys + st.key], wave_fail);
  if (st.tid == 0) {
    atomicAdd(&a.keys[st.key], 1u);
    a.keys[2 * kCovKeys + st.key] = hw_id;    // raw registers, kept as evidence
    a.keys[3 * kCovKeys + st.key] = xcc_id;
  }
#endif
}

// Single-wave probe: copy a 16-bit image into LDS, issue one
// ds_read_b64_tr_b16 with the caller's 64 addresses, return what every lane
// received.  The host has validated alignment and bounds.
__global__ void __launch_bounds__(64, 1)
lds_tr_tile_kernel(const uint16_t* __restrict__ image, uint32_t elems,
                   const uint32_t* __restrict__ offsets,
                   uint16_t* __restrict__ out) {
#if defined(__gfx950__)
  __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
  const uint32_t lane = threadIdx.x;  // one wave of 64
  uint16_t* l16 = reinterpret_cast<uint16_t*>(lds);
  for (uint32_t e = lane; e < elems && e < 2u * kLdsWords; e += 64) l16[e] = image[e];
  __syncthreads();
  // the loop above has reconverged: EXEC is all ones here
  uint32_t off = offsets[lane] & ~7u;
  if (off > (uint32_t)kLdsBytes - 8u) off = (uint32_t)kLdsBytes - 8u;
  const s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(reinterpret_cast<char*>(lds) + off));
  for (int q = 0; q < 4; ++q) out[lane * 4 + q] = (uint16_t)r[q];
#endif
}

static std::vector<std::vector<int>> lds_tr_tile(
    int device, const std::vector<uint16_t>& image,
    const std::vector<int64_t>& lane_byte_offsets) {
  lds_tr_tile_validate(image.size(), lane_byte_offsets);  // before any HIP call
  std::vector<uint32_t> offs(lane_byte_offsets.begin(), lane_byte_offsets.end());
  HIP_CHECK(hipSetDevice(device));
  DeviceBuf<uint16_t> d_image(image.size()), d_out(64 * 4);
  DeviceBuf<uint32_t> d_offs(offs.size());
  d_image.upload(image.data(), image.size());
  d_offs.upload(offs.data(), offs.size());
  d_out.fill(0xFF);
  hipLaunchKernelGGL(lds_tr_tile_kernel, dim3(1), dim3(64), 0, 0, d_image.get(),
                     (uint32_t)image.size(), d_offs.get(), d_out.get());
  HIP_CHECK(hipGetLastError());
  std::vector<uint16_t> h(64 * 4);
  d_out.download(h.data(), h.size());
  std::vector<std::vector<int>> out(64, std::vector<int>(4));
  for (int l = 0; l < 64; ++l)
    for (int q = 0; q < 4; ++q) out[l][q] = h[l * 4 + q];
  return out;
}

struct LdsShape {
  int reps, passes, max_rounds, blocks, poison_key, poison_word;
  unsigned poison_mask;
  uint64_t poison_xor;
};

// every argument is validated here, before the first HIP call
static void lds_validate(const std::string& who, const LdsShape& s) {
  require_range(who, "reps", s.reps, 1, kLdsMaxReps);
  require_range(who, "passes", s.passes, 1, kLdsMaxPasses);
  require_range(who, "max_rounds", s.max_rounds, 1, 64);
  if (s.blocks < 0 || s.blocks > kLdsMaxBlocks)
    throw std::invalid_argument(
        who + ": blocks must be 0 (two per compute unit) or in [1, 65536]");
  require_poison_key(who, s.poison_key);
  if (s.poison_mask >= (1u << kLdsPhases))
    throw std::invalid_argument(who + ": poison_mask has 6 bits");
  if (s.poison_word < -1 || s.poison_word >= kLdsWords)
    throw std::invalid_argument(who + ": poison_word is -1 or a word below 40960");
  if (s.poison_xor == 0 || s.poison_xor > 0xFFFFFFFFull)
    throw std::invalid_argument(who + ": poison_xor is a non-zero 32-bit mask");
}

static py::dict lds_phase_dict(const uint64_t* v) {
  py::dict d;
  for (int p = 0; p < kLdsPhases; ++p) d[kLdsPhaseNames[p]] = v[p];
  return d;
}

static py::dict lds_integrity_check(int device, int reps, int passes,
                                    int max_rounds, uint64_t seed, int blocks,
                                    int poison_key, unsigned poison_mask,
                                    bool poison_all, int poison_word,
                                    uint64_t poison_xor) {
  const LdsShape s = {reps, passes, max_rounds, blocks, poison_key, poison_word,
                      poison_mask, poison_xor};
  lds_validate("lds_integrity_check", s);

  const int cus = select_device("lds_integrity_check", device).multiProcessorCount;
  const int grid = blocks > 0 ? blocks : kCovBlocksPerCu * cus;

  const std::vector<uint32_t> h_src = lds_dma_source(seed);
  DeviceBuf<uint32_t> d_src(h_src.size());
  DeviceBuf<uint32_t> d_keys((size_t)kLdsKeyPlanes * kCovKeys);
  DeviceBuf<unsigned long long> d_counters(kLdsPhases);
  RecordLog<LdsRecord> log(kLdsMaxRecords, kLdsCtlWords, kLdsCtlClaims);
  d_src.upload(h_src.data(), h_src.size());
  d_keys.fill(0);
  d_counters.fill(0);

  const RecordLogView<LdsRecord> log_view = log.view(kLdsMaxRecords);
  LdsLaunch a;
  a.src = d_src.get();
  a.keys = d_keys.get();
  a.ctl = log.ctl();
  a.counters = d_counters.get();
  a.records = log_view.records;
  a.seed = seed;
  a.reps = (uint32_t)reps;
  a.passes = (uint32_t)passes;
  a.max_records = log_view.cap;
  a.poison_mask = poison_mask;
  a.poison_xor = (uint32_t)poison_xor;
  a.poison_key = poison_key;
  a.poison_all = poison_all ? 1 : 0;
  a.poison_word = poison_word;

  // A device or partition that grants less than 160 KiB to a workgroup
  // rejects the launch: that raises in the sweep, it never tests less.  The
  // launch status decides, not the sharedMemPerBlock property.  One table
  // entry per CU: coverage is every CU.
  const SweepRun run = sweep_relaunch(cus, 1, max_rounds, d_keys, [&](int) {
    hipLaunchKernelGGL(lds_integrity_kernel, dim3(grid), dim3(kLdsBlock), 0, 0, a);
  });
  const int rounds = run.rounds;

  unsigned long long counters[kLdsPhases];
  const auto taken = log.collect(kLdsMaxRecords);
  const std::vector<unsigned long long>& ctl = taken.ctl;
  d_counters.download(counters, kLdsPhases);

  py::list records;
  for (const LdsRecord& r : taken.records) {
    py::dict e;
    e["key"] = r.key;
    e["block"] = r.block;
    e["rep"] = r.rep;
    e["phase"] = r.phase < (uint32_t)kLdsPhases ? kLdsPhaseNames[r.phase] : "?";
    e["detail"] = r.detail;
    e["word"] = r.word;
    e["expected"] = r.expected;
    e["got"] = r.got;
    records.append(e);
  }
  uint64_t verified[kLdsPhases], expected[kLdsPhases];
  for (int p = 0; p < kLdsPhases; ++p) {
    verified[p] = counters[p];
    expected[p] = (uint64_t)rounds * (uint64_t)grid * (uint64_t)reps *
                  lds_phase_items(p, passes);
  }
  py::dict out;
  out["compute_units"] = cus;
  out["cus_covered"] = run.tally.cus_covered;
  out["rounds"] = rounds;
  out["blocks"] = grid;
  out["reps"] = reps;
  out["passes"] = passes;
  out["seed"] = seed;
  out["lds_bytes"] = kLdsBytes;
  out["units"] = sweep_unit_list(run.tally, false);
  out["phase_words_verified"] = lds_phase_dict(verified);
  out["phase_words_expected"] = lds_phase_dict(expected);
  out["error_count"] = ctl[kLdsCtlErrors];
  out["xor_or"] = ctl[kLdsCtlXor];
  out["records"] = records;
  // a mismatch that found no record slot left, or found them all claimed
  out["records_dropped"] = ctl[kLdsCtlErrors] - (uint64_t)taken.records.size();
  out["elapsed_ms"] = run.elapsed_ms;
  return out;
}

// host only: no HIP call
static py::dict lds_integrity_reference(uint64_t seed, int block, int rep,
                                        int passes) {
  if (block < 0 || block >= kLdsMaxBlocks || rep < 0 || rep >= kLdsMaxReps)
    throw std::invalid_argument(
        "lds_integrity_reference: block is in [0, 65535], rep in [0, 4095]");
  require_range("lds_integrity_reference", "passes", passes, 1, kLdsMaxPasses);
  const uint32_t b = (uint32_t)block, r = (uint32_t)rep;
  static const char* const kWidthNames[3] = {"b32", "b64", "b128"};

  py::dict out;
  out["lds_words"] = kLdsWords;
  out["phases"] = std::vector<std::string>(kLdsPhaseNames, kLdsPhaseNames + kLdsPhases);
  py::list images, widths;
  for (int pat = 0; pat <= passes; ++pat) {
    images.append(lds_pattern_image(seed, passes, b, r, pat));
    py::list w;
    for (int step = 0; step < 3; ++step)
      w.append(kWidthNames[lds_pattern_width(pat, step)]);
    widths.append(w);
  }
  out["pattern_images"] = images;  // after the fill of each pattern, checker last
  out["pattern_widths"] = widths;
  out["subword_image"] = lds_subword_image(seed, b, r);
  out["dma_source"] = lds_dma_source(seed);
  out["dma_image"] = lds_dma_image(seed, b, r);
  out["transpose_image"] = lds_tr_image(seed, b, r);

  // the last wave-instruction of the 160-byte-row image: its fourth block
  // ends at byte 163839
  {
    const int R = kLdsTrRowBlocks[1];
    const uint32_t n = kLdsTrBlocks / 4 - 1;
    std::vector<uint32_t> offs(64);
    std::vector<std::vector<uint32_t>> lanes(64, std::vector<uint32_t>(4));
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t blk = 4 * n + (l >> 4), i = l & 15;
      offs[l] = lds_tr_lane_offset(R, blk, i);
      for (uint32_t q = 0; q < 4; ++q)
        lanes[l][q] = lds_tr_elem(seed, b, r, lds_tr_expected_elem(R, blk, i, q));
    }
    py::dict t;
    t["row_stride_bytes"] = 32 * R;
    t["first_block"] = 4 * n;
    t["lane_byte_offsets"] = offs;
    t["lanes"] = lanes;
    out["transpose"] = t;
  }
  {
    const LdsAtomExpected e = lds_atom_expected(seed, b, r);  // enforces the bound
    py::dict d;
    d["add_u32"] = e.add32;
    d["add_u64"] = e.add64;
    d["add_f32"] = e.addf;
    d["add_f32_abs_sum"] = e.addf_abs;
    d["max_u32"] = e.max32;
    d["min_u32"] = e.min32;
    d["xor_u32"] = e.x;
    d["or_u32"] = e.o;
    d["and_u32"] = e.a;
    d["f32_bound"] = kLdsF32Bound;
    d["cells"] = kLdsAtomCells;
    d["steps"] = kLdsAtomSteps;
    out["atomics"] = d;
  }
  py::list perm;
  for (uint32_t step = 0; step < (uint32_t)kLdsPermSteps; ++step) {
    std::vector<uint32_t> values(kLdsBlock), sigma(kLdsBlock), pulled(kLdsBlock),
        pushed(kLdsBlock);
    for (uint32_t t = 0; t < (uint32_t)kLdsBlock; ++t) {
      const uint32_t wave = t >> 6, lane = t & 63;
      const uint32_t map = lds_perm_map(seed, b, r, step, wave);
      values[t] = lds_perm_value(seed, b, r, step, t);
      sigma[t] = lds_perm_sigma(map, lane);
      pulled[t] = lds_perm_value(seed, b, r, step, wave * 64 + sigma[t]);
      pushed[t] = lds_perm_value(seed, b, r, step,
                                 wave * 64 + lds_perm_sigma_inv(map, lane));
    }
    py::dict e;
    e["values"] = values;
    e["sigma"] = sigma;
    e["bpermute"] = pulled;
    e["permute"] = pushed;
    perm.append(e);
  }
  out["permute"] = perm;
  return out;
}

// ---------------------------------------------------------------------------
// Host-link data-integrity check: bytes that cross the path between host
// memory and the device (pinning, IOMMU / GART mappings, the copy engines,
// userptr registration, PCIe AtomicOps) are compared exactly.  Per memory kind
// (pinned: hipHostMalloc, registered: hipHostRegister of ordinary pages,
// pageable: malloc) one host buffer H and one device buffer D go through
//   h2d        CPU fills H with p0, copy H->D, a kernel compares D and writes ~p0
//   d2h        copy D->H, the CPU compares H with ~p0
//   zc_read    CPU fills H with p2, a kernel reads H through its device pointer
//   zc_write   a kernel writes ~p2 into H (16-byte, byte and 16-bit stores),
//              the CPU compares
//   duplex     H.lo->D.lo and D.hi->H.hi enqueued on two streams at once
//   unaligned  464 short copies at odd offsets and lengths, whole destination
//              slots compared
//   atomics    system-scope fetch-add, swap and compare-and-swap on pinned
//              memory while the host thread adds to the same cells
// Patterns, the copy plan and the atomics operands are in
// hostlink_problems.hpp; the device-memory steps reuse hbm_pattern_kernel.
//
// Counting is as in the HBM check: lanes count what they compared, a workgroup
// adds its total to a sharded counter once, the host sums the shards per phase
// and reports them next to the expected count.  Every kernel does a fixed
// amount of work and exits; the host reads memory a kernel writes only after
// a synchronise.  The poison hook XORs into expected values, never into
// memory.  The check sets no environment variable and leaves to the runtime
// which engine performs a copy.
// ---------------------------------------------------------------------------

constexpr int kHlBlock = 256;
constexpr int kHlChunkShift = 7;                 // 128 words: 1 KiB chunks
constexpr uint64_t kHlSubwordBytes = 1ull << 20;  // sub-word chunks live here

// zc_write: store ~p for vector i (words 2i, 2i + 1).  Inside the first
// sub_words words (a whole number of chunks) chunk c % 4 == 1 is assembled from
// byte stores and c % 4 == 3 from 16-bit stores: the owner of vector v of the
// chunk stores the pieces v, v + 64, v + 128, ... of the chunk, so the eight
// bytes (four halves) of one word come from eight (four) different lanes and
// the 64 vector owners of a chunk together store each of its pieces once.
__device__ __forceinline__ void hostlink_store_vec(const HbmLaunch& a,
                                                   uint64_t sub_words, uint64_t i) {
  const uint64_t w0 = 2 * i;
  if (w0 < sub_words) {
    const uint64_t c = w0 >> kHlChunkShift, first = c << kHlChunkShift;
    const uint32_t v = (uint32_t)(i & 63);
    if ((c & 3) == 1) {
      uint8_t* bytes = reinterpret_cast<uint8_t*>(a.buf + first);
      for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t o = v + 64 * k;  // < 1024
        const uint64_t p = ~hbm_pattern_value(a.pattern, a.seed, first + (o >> 3));
        bytes[o] = (uint8_t)(p >> (8 * (o & 7)));
      }
      return;
    }
    if ((c & 3) == 3) {
      uint16_t* halves = reinterpret_cast<uint16_t*>(a.buf + first);
      for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t h = v + 64 * k;  // < 512
        const uint64_t p = ~hbm_pattern_value(a.pattern, a.seed, first + (h >> 2));
        halves[h] = (uint16_t)(p >> (16 * (h & 3)));
      }
      return;
    }
  }
  u64x2 p;
  p[0] = ~hbm_pattern_value(a.pattern, a.seed, w0);
  p[1] = ~hbm_pattern_value(a.pattern, a.seed, w0 + 1);
  __builtin_nontemporal_store(p, reinterpret_cast<u64x2*>(a.buf) + i);
}

// a.buf is host memory seen through its device pointer.  WRITE false: compare
// with p (zc_read); true: write ~p (zc_write).  Shape and counting as in
// hbm_pattern_kernel: 16-byte nontemporal accesses, 2x unrolled grid-stride
// body, remainder loop, one thread for an odd last word.  A lane's counter is
// 32-bit: 2^27 words at the most, over at least 256 threads.
template <bool WRITE>
__global__ void __launch_bounds__(kHlBlock)
hostlink_pattern_kernel(HbmLaunch a, uint64_t sub_words) {
  __shared__ uint32_t wave_compared[kHlBlock / 64];
  const u64x2* __restrict__ v = reinterpret_cast<const u64x2*>(a.buf);
  const uint64_t nvec = a.nwords >> 1;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t compared = 0, bad = 0;
  uint64_t bad_xor = 0;

  uint64_t i = tid;
  for (; i + stride < nvec; i += 2 * stride) {
    if (WRITE) {
      hostlink_store_vec(a, sub_words, i);
      hostlink_store_vec(a, sub_words, i + stride);
    } else {
      const uint64_t w0 = 2 * i, w1 = 2 * (i + stride);
      const u64x2 g0 = __builtin_nontemporal_load(&v[i]);
      const u64x2 g1 = __builtin_nontemporal_load(&v[i + stride]);
      const uint64_t x0 = hbm_diff(a, w0, g0[0], 0);
      const uint64_t x1 = hbm_diff(a, w0 + 1, g0[1], 0);
      const uint64_t x2 = hbm_diff(a, w1, g1[0], 0);
      const uint64_t x3 = hbm_diff(a, w1 + 1, g1[1], 0);
      compared += 4;
      if ((x0 | x1 | x2 | x3) != 0) {
        hbm_report(a, w0, g0[0], x0, bad, bad_xor);
        hbm_report(a, w0 + 1, g0[1], x1, bad, bad_xor);
        hbm_report(a, w1, g1[0], x2, bad, bad_xor);
        hbm_report(a, w1 + 1, g1[1], x3, bad, bad_xor);
      }
    }
  }
  for (; i < nvec; i += stride) {
    if (WRITE) {
      hostlink_store_vec(a, sub_words, i);
    } else {
      const uint64_t w0 = 2 * i;
      const u64x2 g0 = __builtin_nontemporal_load(&v[i]);
      const uint64_t x0 = hbm_diff(a, w0, g0[0], 0);
      const uint64_t x1 = hbm_diff(a, w0 + 1, g0[1], 0);
      compared += 2;
      if ((x0 | x1) != 0) {
        hbm_report(a, w0, g0[0], x0, bad, bad_xor);
        hbm_report(a, w0 + 1, g0[1], x1, bad, bad_xor);
      }
    }
  }
  if ((a.nwords & 1ull) && tid == 0) {  // scalar tail: the odd last word
    const uint64_t t = a.nwords - 1;
    if (WRITE) {
      a.buf[t] = ~hbm_pattern_value(a.pattern, a.seed, t);
    } else {
      const uint64_t got = a.buf[t];
      ++compared;
      hbm_report(a, t, got, hbm_diff(a, t, got, 0), bad, bad_xor);
    }
  }

  if (!WRITE) {
    if (bad != 0) {  // on a mismatch, and only then
      atomicAdd(&a.ctl[kHbmCtlErrors], (unsigned long long)bad);
      atomicOr(&a.ctl[kHbmCtlXor], (unsigned long long)bad_xor);
    }
    uint32_t sum = compared;
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) wave_compared[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long total = 0;
      for (int w = 0; w < kHlBlock / 64; ++w) total += wave_compared[w];
      atomicAdd(&a.shards[(blockIdx.x & (kHbmShards - 1)) * kHbmShardStride],
                total);
    }
  }
}

// The atomics tables, all in one pinned host buffer: 64 cells and four
// counters, each on a 128-byte line of its own, then seen[] and olds[].
struct alignas(128) HlCell {
  uint64_t add64, swap64, claim64, confirm64;
  uint32_t add32, claim32, confirm32;
};
struct alignas(128) HlLine {
  unsigned long long v;
};
constexpr int kHlLineTicket = 0, kHlLineWinners32 = 1, kHlLineWinners64 = 2,
              kHlLineTicketRange = 3, kHlLines = 4;

struct HlAtomics {
  HlCell* cells;
  HlLine* lines;
  uint32_t* seen;   // [threads]: id + 1 of the thread that drew ticket t
  uint64_t* olds;   // [threads]: what thread id got back from its exchange
  uint64_t seed;
  uint32_t reps, threads;
};

// Fetch-add, swap and compare-and-swap, 32 and 64 bit, all system scope and
// all on host memory.  Fixed work: nothing here waits for another thread or
// for the host, which adds to the same cells while this runs.
__global__ void __launch_bounds__(kHostlinkAtomBlock)
hostlink_atomics_kernel(HlAtomics a) {
  const uint32_t id = blockIdx.x * kHostlinkAtomBlock + threadIdx.x;
  for (uint32_t r = 0; r < a.reps; ++r) {
    const HostlinkAtomVals v = hostlink_atom_vals(a.seed, id, r);
    HlCell& c = a.cells[(id + r) % kHostlinkAtomCells];
    __hip_atomic_fetch_add(&c.add32, v.add32, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_fetch_add(&c.add64, v.add64, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // the ticket is range-checked before it is used as an index
  const unsigned long long ticket =
      __hip_atomic_fetch_add(&a.lines[kHlLineTicket].v, 1ull, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
  if (ticket < a.threads)
    a.seen[ticket] = id + 1;
  else
    __hip_atomic_fetch_add(&a.lines[kHlLineTicketRange].v, 1ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
  a.olds[id] = __hip_atomic_exchange(&a.cells[id % kHostlinkAtomCells].swap64,
                                     (uint64_t)id + 1, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_SYSTEM);
  HlCell& k = a.cells[id % kHostlinkClaimCells];
  uint32_t free32 = 0;
  if (__hip_atomic_compare_exchange_strong(&k.claim32, &free32, id + 1,
                                           __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM)) {
    k.confirm32 = id + 1;
    __hip_atomic_fetch_add(&a.lines[kHlLineWinners32].v, 1ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
  }
  uint64_t free64 = 0;
  if (__hip_atomic_compare_exchange_strong(&k.claim64, &free64, (uint64_t)id + 1,
                                           __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM)) {
    k.confirm64 = (uint64_t)id + 1;
    __hip_atomic_fetch_add(&a.lines[kHlLineWinners64].v, 1ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// One host buffer of a memory kind.  dev is null for pageable memory.
struct HlHostMem {
  HostBuf pinned;
  RegisteredBuf registered;
  void* pageable = nullptr;
  uint8_t* host = nullptr;
  uint8_t* dev = nullptr;
  HlHostMem(int kind, size_t bytes) {
    if (kind == kHostlinkPinned) {
      pinned = HostBuf(bytes);
      host = static_cast<uint8_t*>(pinned.get());
      dev = static_cast<uint8_t*>(pinned.device());
    } else if (kind == kHostlinkRegistered) {
      registered = RegisteredBuf(bytes);
      host = static_cast<uint8_t*>(registered.get());
      dev = static_cast<uint8_t*>(registered.device());
    } else {
      pageable = std::malloc(bytes);
      if (!pageable) throw std::bad_alloc();
      host = static_cast<uint8_t*>(pageable);
    }
  }
  HlHostMem(const HlHostMem&) = delete;
  HlHostMem& operator=(const HlHostMem&) = delete;
  ~HlHostMem() { std::free(pageable); }
};

struct HlPhase {
  bool ran = false;
  uint64_t compared = 0, expected = 0, errors = 0;
  double ms = 0.0;          // the whole phase, host fills and compares included
  double link_ms = 0.0;     // the step that crossed the link
  double link_bytes = 0.0;  // and what it moved
};

static double hl_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now() - t0).count();
}

// What a run accumulates over all kinds and phases.  The record cap is shared:
// a phase may keep what the phases before it left of max_records.
struct HlRun {
  int max_records = 0;
  uint64_t error_count = 0, xor_or = 0, dropped = 0;
  py::list records;
  size_t room() const { return (size_t)max_records - py::len(records); }
};

static py::dict hl_word_record(int kind, int phase, const char* side,
                               uint64_t word, uint64_t expected, uint64_t got) {
  py::dict e;
  e["kind"] = kHostlinkKindNames[kind];
  e["phase"] = kHostlinkPhaseNames[phase];
  e["side"] = side;
  e["word"] = word;
  e["byte_offset"] = 8 * word;
  e["expected"] = expected;
  e["got"] = got;
  py::list bits;
  for (int b = 0; b < 64; ++b)
    if (((expected ^ got) >> b) & 1ull) bits.append(b);
  e["flipped_bits"] = bits;
  return e;
}

// after a synchronise: move what the kernels of one phase counted and
// recorded into `ph` and `run`, and zero the tables for the next phase
static void hl_take_device(HbmTables& tables, int kind, int phase, HlPhase& ph,
                           HlRun& run) {
  const auto log = tables.log.collect(run.room(), true);
  ph.compared += tables.words_compared(true);
  ph.errors += log.ctl[kHbmCtlErrors];
  run.error_count += log.ctl[kHbmCtlErrors];
  run.xor_or |= log.ctl[kHbmCtlXor];
  for (const HbmRecord& r : log.records)
    run.records.append(
        hl_word_record(kind, phase, "device", r.word, r.expected, r.got));
  run.dropped += log.claims - log.records.size();
}

static void hl_take_host(int kind, int phase, const HostlinkTally& t, HlPhase& ph,
                         HlRun& run) {
  ph.compared += t.compared;
  ph.errors += t.errors;
  run.error_count += t.errors;
  run.xor_or |= t.xor_or;
  run.dropped += t.dropped;
  for (const HostlinkWordRecord& r : t.records)
    run.records.append(
        hl_word_record(kind, phase, "host", r.word, r.expected, r.got));
}

static void hl_atom_mismatch(HlRun& run, HlPhase& ph, const char* comparison,
                             const char* op, int cell, py::object expected,
                             py::object got) {
  ++ph.errors;
  ++run.error_count;
  if (run.room() == 0) {
    ++run.dropped;
    return;
  }
  py::dict e;
  e["kind"] = kHostlinkKindNames[kHostlinkPinned];
  e["phase"] = kHostlinkPhaseNames[kHostlinkAtomics];
  e["side"] = "host";
  e["comparison"] = comparison;
  e["op"] = op;
  e["cell"] = cell;
  e["expected"] = expected;
  e["got"] = got;
  run.records.append(e);
}

// The atomics phase on a pinned buffer of its own; returns its tables.
static py::dict hl_run_atomics(int blocks, int reps, uint64_t host_adds,
                               uint64_t seed, bool poisoned, uint64_t poison_xor,
                               HlPhase& ph, HlRun& run) {
  const uint32_t threads = (uint32_t)blocks * kHostlinkAtomBlock;
  const HostlinkAtomExpected e =
      hostlink_atom_expected(seed, threads, reps, host_adds);
  const size_t cells_b = sizeof(HlCell) * kHostlinkAtomCells;
  const size_t lines_b = sizeof(HlLine) * kHlLines;
  const size_t olds_b = sizeof(uint64_t) * threads;
  const size_t seen_b = sizeof(uint32_t) * threads;
  HostBuf mem(cells_b + lines_b + olds_b + seen_b);
  std::memset(mem.get(), 0, mem.size());
  uint8_t* h = static_cast<uint8_t*>(mem.get());
  uint8_t* d = static_cast<uint8_t*>(mem.device());
  HlCell* cells = reinterpret_cast<HlCell*>(h);
  HlLine* lines = reinterpret_cast<HlLine*>(h + cells_b);
  const uint64_t* olds = reinterpret_cast<const uint64_t*>(h + cells_b + lines_b);
  const uint32_t* seen =
      reinterpret_cast<const uint32_t*>(h + cells_b + lines_b + olds_b);

  HlAtomics a;
  a.cells = reinterpret_cast<HlCell*>(d);
  a.lines = reinterpret_cast<HlLine*>(d + cells_b);
  a.olds = reinterpret_cast<uint64_t*>(d + cells_b + lines_b);
  a.seen = reinterpret_cast<uint32_t*>(d + cells_b + lines_b + olds_b);
  a.seed = seed;
  a.reps = (uint32_t)reps;
  a.threads = threads;
  const auto t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(hostlink_atomics_kernel, dim3(blocks),
                     dim3(kHostlinkAtomBlock), 0, 0, a);
  HIP_CHECK(hipGetLastError());
  // the host's own adds to the same cells: fixed work, nobody waits
  for (uint64_t j = 0; j < host_adds; ++j) {
    const HostlinkAtomVals v = hostlink_atom_vals(seed, kHostlinkHostId + j, 0);
    HlCell& c = cells[j % kHostlinkAtomCells];
    __atomic_fetch_add(&c.add32, v.add32, __ATOMIC_RELAXED);
    __atomic_fetch_add(&c.add64, v.add64, __ATOMIC_RELAXED);
  }
  HIP_CHECK(hipDeviceSynchronize());
  ph.link_ms = hl_ms_since(t0);

  std::vector<uint32_t> add32(kHostlinkAtomCells);
  std::vector<uint64_t> add64(kHostlinkAtomCells);
  for (int c = 0; c < kHostlinkAtomCells; ++c) {
    add32[c] = cells[c].add32;
    add64[c] = cells[c].add64;
    // test hook: data only, the expected value of add32 cell 0
    const uint32_t w32 =
        e.add32[c] ^ (poisoned && c == 0 ? (uint32_t)poison_xor : 0u);
    if (add32[c] != w32)
      hl_atom_mismatch(run, ph, "add_u32", "add_u32", c, py::int_(w32),
                       py::int_(add32[c]));
    if (add64[c] != e.add64[c])
      hl_atom_mismatch(run, ph, "add_u64", "add_u64", c, py::int_(e.add64[c]),
                       py::int_(add64[c]));
  }
  ph.compared += 2 * kHostlinkAtomCells;

  // every ticket drawn exactly once: counter == threads and no hole in seen
  const uint64_t counter = lines[kHlLineTicket].v;
  const uint64_t out_of_range = lines[kHlLineTicketRange].v;
  if (counter != threads)
    hl_atom_mismatch(run, ph, "tickets", "fetch_add_u64", -1, py::int_(threads),
                     py::int_(counter));
  if (out_of_range != 0)
    hl_atom_mismatch(run, ph, "tickets", "ticket_range", -1, py::int_(0),
                     py::int_(out_of_range));
  uint64_t holes = 0;
  for (uint32_t t = 0; t < threads; ++t) holes += seen[t] == 0;
  if (holes != 0)
    hl_atom_mismatch(run, ph, "tickets", "seen_holes", -1, py::int_(0),
                     py::int_(holes));
  ph.compared += 2 + threads;

  // swap: what came back plus what stayed is {0 x 64} and {1 .. threads}
  std::vector<uint64_t> bag(olds, olds + threads);
  for (int c = 0; c < kHostlinkAtomCells; ++c) bag.push_back(cells[c].swap64);
  std::sort(bag.begin(), bag.end());
  uint64_t swap_bad = 0;
  for (size_t i = 0; i < bag.size(); ++i) {
    const uint64_t want =
        i < (size_t)kHostlinkAtomCells ? 0 : i - kHostlinkAtomCells + 1;
    if (bag[i] != want && swap_bad++ == 0)
      hl_atom_mismatch(run, ph, "swap", "swap_u64", -1, py::int_(want),
                       py::int_(bag[i]));
  }
  if (swap_bad > 1) {  // the first is recorded, the rest only counted
    ph.errors += swap_bad - 1;
    run.error_count += swap_bad - 1;
    run.dropped += swap_bad - 1;
  }
  ph.compared += bag.size();

  // compare-and-swap: one winner per cell and width, who confirmed it
  std::vector<uint64_t> claim32(kHostlinkClaimCells), confirm32(kHostlinkClaimCells),
      claim64(kHostlinkClaimCells), confirm64(kHostlinkClaimCells);
  for (int c = 0; c < kHostlinkClaimCells; ++c) {
    claim32[c] = cells[c].claim32;
    confirm32[c] = cells[c].confirm32;
    claim64[c] = cells[c].claim64;
    confirm64[c] = cells[c].confirm64;
    if (claim32[c] == 0 || claim32[c] != confirm32[c])
      hl_atom_mismatch(run, ph, "cas", "cas_u32", c, py::int_(claim32[c]),
                       py::int_(confirm32[c]));
    if (claim64[c] == 0 || claim64[c] != confirm64[c])
      hl_atom_mismatch(run, ph, "cas", "cas_u64", c, py::int_(claim64[c]),
                       py::int_(confirm64[c]));
  }
  const uint64_t winners32 = lines[kHlLineWinners32].v;
  const uint64_t winners64 = lines[kHlLineWinners64].v;
  const uint64_t want_winners = std::min<uint64_t>(threads, kHostlinkClaimCells);
  if (winners32 != want_winners)
    hl_atom_mismatch(run, ph, "cas", "winners_u32", -1, py::int_(want_winners),
                     py::int_(winners32));
  if (winners64 != want_winners)
    hl_atom_mismatch(run, ph, "cas", "winners_u64", -1, py::int_(want_winners),
                     py::int_(winners64));
  ph.compared += 2 * kHostlinkClaimCells + 2;
  ph.expected = hostlink_atom_items(threads);

  py::dict out;
  out["blocks"] = blocks;
  out["threads"] = threads;
  out["reps"] = reps;
  out["host_adds"] = host_adds;
  out["add32"] = add32;
  out["add64"] = add64;
  out["expected_add32"] = e.add32;
  out["expected_add64"] = e.add64;
  out["ticket_counter"] = counter;
  out["tickets_out_of_range"] = out_of_range;
  out["seen_holes"] = holes;
  out["swap_mismatches"] = swap_bad;
  out["claim32"] = claim32;
  out["confirm32"] = confirm32;
  out["claim64"] = claim64;
  out["confirm64"] = confirm64;
  out["winners32"] = winners32;
  out["winners64"] = winners64;
  return out;
}

static py::dict host_link_plan() {
  const HostlinkPlan plan = hostlink_plan();
  py::list cases;
  for (const HostlinkCase& c : plan.cases) {
    py::dict e;
    e["case"] = c.index;
    e["direction"] = kHostlinkDirectionNames[c.direction];
    e["len"] = c.len;
    e["src_off"] = c.src_off;
    e["dst_off"] = c.dst_off;
    e["src_pos"] = c.src_pos();
    e["dst_pos"] = c.dst_pos();
    cases.append(e);
  }
  py::dict out;
  out["slot_bytes"] = plan.slot_bytes;
  out["guard"] = plan.guard;
  out["cases"] = cases;
  return out;
}

static py::dict host_link_reference(uint64_t seed, uint64_t threads, int reps,
                                    int64_t host_adds) {
  // host only: no HIP call
  if (threads > (uint64_t)kHostlinkMaxAtomBlocks * kHostlinkAtomBlock)
    throw std::invalid_argument("host_link_reference: threads is at most 262144");
  require_range("host_link_reference", "reps", reps, 1, kHostlinkMaxReps);
  if (host_adds < 0 || host_adds > kHostlinkMaxHostAdds ||
      host_adds % kHostlinkAtomCells != 0)
    throw std::invalid_argument(
        "host_link_reference: host_adds must be a multiple of 64 in [0, 2^20]");
  const HostlinkAtomExpected e =
      hostlink_atom_expected(seed, threads, reps, (uint64_t)host_adds);
  py::dict out;
  out["add32"] = e.add32;
  out["add64"] = e.add64;
  out["device_add32"] = e.device32;
  out["device_add64"] = e.device64;
  out["host_add32"] = e.host32;
  out["host_add64"] = e.host64;
  out["items"] = hostlink_atom_items(threads);
  return out;
}

static py::dict host_link_check(int device, uint64_t nbytes, uint64_t seed,
                                const std::vector<std::string>& kinds, int blocks,
                                int atomics_blocks, int reps, int64_t host_adds,
                                int max_records, unsigned poison_mask,
                                int poison_kind, int64_t poison_word,
                                int64_t poison_case, uint64_t poison_xor) {
  // every argument is validated before the first HIP call
  HostlinkShape shape{nbytes,      hostlink_kind_list(kinds), blocks,
                      atomics_blocks, reps,                   host_adds,
                      max_records, poison_mask,               poison_kind,
                      poison_word, poison_case,               poison_xor};
  hostlink_validate(shape);

  HIP_CHECK(hipSetDevice(device));
  int cus = 0, native_atomics = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                  device));
  HIP_CHECK(hipDeviceGetAttribute(
      &native_atomics, hipDeviceAttributeHostNativeAtomicSupported, device));
  const int grid = blocks > 0 ? blocks : 4 * cus;
  const int atom_grid =
      atomics_blocks > 0 ? atomics_blocks : std::min(cus, kHostlinkMaxAtomBlocks);
  const uint64_t words = nbytes / 8, lo = words / 2;
  const uint64_t sub_words = (std::min(nbytes, kHlSubwordBytes) >> 10)
                             << kHlChunkShift;
  const HostlinkPlan plan = hostlink_plan();
  const auto run_t0 = std::chrono::steady_clock::now();

  HlRun run;
  run.max_records = max_records;
  HbmTables tables(max_records);
  Stream s1, s2;
  Event e1a, e1b, e2a, e2b;
  unsigned fail_mask = 0;
  py::dict kinds_out, atomics_out;
  bool atomics_ran = false;
  {
    // One 4 KiB copy each way on each stream between two scratch buffers, so
    // the rate of the first phase does not carry the runtime's first-use
    // set-up of a stream.  No checked buffer is touched.
    HostBuf warm_h(4096);
    DeviceBuf<uint8_t> warm_d(4096);
    std::memset(warm_h.get(), 0, 4096);
    for (hipStream_t s : {s1.s, s2.s}) {
      HIP_CHECK(hipMemcpyAsync(warm_d.get(), warm_h.get(), 4096,
                               hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(warm_h.get(), warm_d.get(), 4096,
                               hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  }

  for (const int kind : shape.kinds) {
    const unsigned runs = hostlink_kind_phases(kind);
    const bool poison_here = poison_kind < 0 || poison_kind == kind;
    const auto poisoned = [&](int phase) {
      return poison_here && ((poison_mask >> phase) & 1u);
    };
    const auto pword = [&](int phase) -> int64_t {
      return poisoned(phase) ? poison_word : -1;
    };
    const auto pseed = [&](int phase) {
      return hostlink_seed(seed, kind, hostlink_data_phase(phase));
    };
    HlPhase phases[kHostlinkPhases];
    bool overlap = false;

    // a failed allocation or registration raises: never silently test less
    HlHostMem hmem(kind, (size_t)nbytes);
    DeviceBuf<uint64_t> dbuf((size_t)words);
    uint64_t* H = reinterpret_cast<uint64_t*>(hmem.host);
    uint64_t* D = dbuf.get();

    // pinned and registered memory is copied on the check's own stream,
    // pageable memory with a plain hipMemcpy; both return when the copy is done
    const auto copy = [&](void* dst, const void* src, size_t n, hipMemcpyKind dir) {
      if (kind == kHostlinkPageable) {
        HIP_CHECK(hipMemcpy(dst, src, n, dir));
      } else {
        HIP_CHECK(hipMemcpyAsync(dst, src, n, dir, s1.s));
        HIP_CHECK(hipStreamSynchronize(s1.s));
      }
    };
    // a pattern kernel's arguments: this phase's hash pattern over n words at
    // buf, what the log has room for
    const auto pass_args = [&](uint64_t* buf, uint64_t n, uint64_t base, int phase,
                               int64_t poison_at) {
      HbmLaunch a;
      a.buf = buf;
      a.nwords = n;
      a.base = base;
      a.seed = pseed(phase);
      a.poison_xor = poison_xor;
      a.poison_stride = 0;
      a.poison_word = poison_at;
      tables.attach(a, run.room());
      a.verify_index = (uint32_t)phase;
      a.pattern = kHbmPatternHash;
      return a;
    };
    // hbm_pattern_kernel over device words [base, base + n) of D
    const auto device_pass = [&](int hbm_kind, uint64_t base, uint64_t n,
                                 int phase) {
      hbm_launch(hbm_kind, pass_args(D + base, n, base, phase, pword(phase)));
    };
    // hostlink_pattern_kernel over all of H through its device pointer
    const auto host_pass = [&](bool write, int phase) {
      const HbmLaunch a = pass_args(reinterpret_cast<uint64_t*>(hmem.dev), words, 0,
                                    phase, write ? -1 : pword(phase));
      if (write)
        hipLaunchKernelGGL(hostlink_pattern_kernel<true>, dim3(grid),
                           dim3(kHlBlock), 0, 0, a, sub_words);
      else
        hipLaunchKernelGGL(hostlink_pattern_kernel<false>, dim3(grid),
                           dim3(kHlBlock), 0, 0, a, sub_words);
      HIP_CHECK(hipGetLastError());
    };
    const auto host_verify = [&](int phase, uint64_t first, uint64_t n) {
      HostlinkTally t;
      hostlink_verify(H + first, first, n, pseed(phase),
                      hostlink_data_inverted(phase), pword(phase), poison_xor,
                      run.room(), t);
      hl_take_host(kind, phase, t, phases[phase], run);
    };
    const auto timed = [&](HlPhase& ph, double bytes, auto&& work) {
      const auto t0 = std::chrono::steady_clock::now();
      work();
      ph.link_ms += hl_ms_since(t0);
      ph.link_bytes += bytes;
    };

    {  // bit 0, h2d
      HlPhase& ph = phases[kHostlinkH2d];
      const auto t0 = std::chrono::steady_clock::now();
      ph.ran = true;
      ph.expected = words;
      hostlink_fill(H, 0, words, pseed(kHostlinkH2d), false);
      timed(ph, (double)nbytes, [&] { copy(D, H, nbytes, hipMemcpyHostToDevice); });
      device_pass(kHbmVerifyInvert, 0, words, kHostlinkH2d);
      HIP_CHECK(hipDeviceSynchronize());
      hl_take_device(tables, kind, kHostlinkH2d, ph, run);
      ph.ms = hl_ms_since(t0);
    }
    {  // bit 1, d2h: H still holds p0, D holds ~p0
      HlPhase& ph = phases[kHostlinkD2h];
      const auto t0 = std::chrono::steady_clock::now();
      ph.ran = true;
      ph.expected = words;
      timed(ph, (double)nbytes, [&] { copy(H, D, nbytes, hipMemcpyDeviceToHost); });
      host_verify(kHostlinkD2h, 0, words);
      ph.ms = hl_ms_since(t0);
    }
    if (runs & 1u << kHostlinkZcRead) {  // bit 2
      HlPhase& ph = phases[kHostlinkZcRead];
      const auto t0 = std::chrono::steady_clock::now();
      ph.ran = true;
      ph.expected = words;
      hostlink_fill(H, 0, words, pseed(kHostlinkZcRead), false);
      timed(ph, (double)nbytes, [&] {
        host_pass(false, kHostlinkZcRead);
        HIP_CHECK(hipDeviceSynchronize());
      });
      hl_take_device(tables, kind, kHostlinkZcRead, ph, run);
      ph.ms = hl_ms_since(t0);
    }
    if (runs & 1u << kHostlinkZcWrite) {  // bit 3: H holds p2 until the kernel ran
      HlPhase& ph = phases[kHostlinkZcWrite];
      const auto t0 = std::chrono::steady_clock::now();
      ph.ran = true;
      ph.expected = words;
      timed(ph, (double)nbytes, [&] {
        host_pass(true, kHostlinkZcWrite);
        HIP_CHECK(hipDeviceSynchronize());
      });
      host_verify(kHostlinkZcWrite, 0, words);
      ph.ms = hl_ms_since(t0);
    }
    if (runs & 1u << kHostlinkDuplex) {  // bit 4: H.hi holds ~p2, D.lo holds ~p0
      HlPhase& ph = phases[kHostlinkDuplex];
      const auto t0 = std::chrono::steady_clock::now();
      ph.ran = true;
      ph.expected = words;
      hostlink_fill(H, 0, lo, pseed(kHostlinkDuplex), false);
      // fill D.hi; hbm_pattern_kernel's 16-byte stores need an even first
      // word, so an odd one is filled by a launch of its own (its scalar tail)
      const uint64_t even = lo + (lo & 1ull);
      if (lo & 1ull) device_pass(kHbmFill, lo, 1, kHostlinkDuplex);
      if (even < words) device_pass(kHbmFill, even, words - even, kHostlinkDuplex);
      HIP_CHECK(hipDeviceSynchronize());
      timed(ph, (double)nbytes, [&] {
        HIP_CHECK(hipEventRecord(e1a.ev, s1.s));
        HIP_CHECK(hipMemcpyAsync(D, H, 8 * lo, hipMemcpyHostToDevice, s1.s));
        HIP_CHECK(hipEventRecord(e1b.ev, s1.s));
        HIP_CHECK(hipEventRecord(e2a.ev, s2.s));
        HIP_CHECK(hipMemcpyAsync(H + lo, D + lo, 8 * (words - lo),
                                 hipMemcpyDeviceToHost, s2.s));
        HIP_CHECK(hipEventRecord(e2b.ev, s2.s));
        HIP_CHECK(hipStreamSynchronize(s1.s));
        HIP_CHECK(hipStreamSynchronize(s2.s));
      });
      // reported, never judged: did the two copies run at the same time?
      float len1 = 0.f, start2 = 0.f, len2 = 0.f;
      HIP_CHECK(hipEventElapsedTime(&len1, e1a.ev, e1b.ev));
      HIP_CHECK(hipEventElapsedTime(&start2, e1a.ev, e2a.ev));
      HIP_CHECK(hipEventElapsedTime(&len2, e2a.ev, e2b.ev));
      overlap = start2 < len1 && start2 + len2 > 0.f;
      // the hook acts on the side that compares poison_word: the kernel sees
      // only words below lo, the host only the rest
      device_pass(kHbmVerifyInvert, 0, lo, kHostlinkDuplex);
      HIP_CHECK(hipDeviceSynchronize());
      hl_take_device(tables, kind, kHostlinkDuplex, ph, run);
      host_verify(kHostlinkDuplex, lo, words - lo);
      ph.ms = hl_ms_since(t0);
    }
    {  // bit 5, unaligned
      HlPhase& ph = phases[kHostlinkUnaligned];
      const auto t0 = std::chrono::steady_clock::now();
      ph.ran = true;
      ph.expected = (uint64_t)plan.cases.size() * plan.slot_bytes;
      const uint64_t src_seed = hostlink_seed(seed, kind, kHostlinkUnaligned);
      const uint64_t bg_seed = hostlink_seed(seed, kind, kHostlinkBackground);
      HlHostMem slots(kind, 2 * plan.slot_bytes);
      DeviceBuf<uint8_t> dslot(plan.slot_bytes);
      uint8_t* ha = slots.host;                    // the source image
      uint8_t* hb = slots.host + plan.slot_bytes;  // background / destination
      uint8_t* ds = dslot.get();
      HostlinkSlotTally t;
      for (const HostlinkCase& c : plan.cases) {
        hostlink_slot_fill(ha, src_seed, c.index);
        hostlink_slot_fill(hb, bg_seed, c.index);
        if (c.direction == 0) {
          // the destination slot is on the device: whole-slot aligned copies
          // set it and bring it back
          copy(ds, hb, plan.slot_bytes, hipMemcpyHostToDevice);
          timed(ph, (double)c.len, [&] {
            copy(ds + c.dst_pos(), ha + c.src_pos(), c.len, hipMemcpyHostToDevice);
          });
          copy(hb, ds, plan.slot_bytes, hipMemcpyDeviceToHost);
        } else {
          copy(ds, ha, plan.slot_bytes, hipMemcpyHostToDevice);
          timed(ph, (double)c.len, [&] {
            copy(hb + c.dst_pos(), ds + c.src_pos(), c.len, hipMemcpyDeviceToHost);
          });
        }
        const bool hit = poisoned(kHostlinkUnaligned) && c.index == poison_case;
        const size_t before = t.records.size();
        hostlink_slot_compare(hb, c, src_seed, bg_seed,
                              hit ? (uint8_t)poison_xor : (uint8_t)0,
                              before + run.room(), t);
        for (size_t r = before; r < t.records.size(); ++r) {
          const HostlinkByteRecord& b = t.records[r];
          py::dict e;
          e["kind"] = kHostlinkKindNames[kind];
          e["phase"] = kHostlinkPhaseNames[kHostlinkUnaligned];
          e["side"] = "host";
          e["case"] = c.index;
          e["direction"] = kHostlinkDirectionNames[c.direction];
          e["src_off"] = c.src_off;
          e["dst_off"] = c.dst_off;
          e["len"] = c.len;
          e["byte_offset"] = b.offset;
          e["expected"] = (int)b.expected;
          e["got"] = (int)b.got;
          py::list bits;
          for (int k = 0; k < 8; ++k)
            if (((b.expected ^ b.got) >> k) & 1) bits.append(k);
          e["flipped_bits"] = bits;
          run.records.append(e);
        }
      }
      ph.compared = t.compared;
      ph.errors = t.errors;
      run.error_count += t.errors;
      run.xor_or |= t.xor_or;
      run.dropped += t.dropped;
      ph.ms = hl_ms_since(t0);
    }
    if ((runs & 1u << kHostlinkAtomics) && native_atomics != 0) {  // bit 6
      HlPhase& ph = phases[kHostlinkAtomics];
      const auto t0 = std::chrono::steady_clock::now();
      ph.ran = true;
      atomics_out = hl_run_atomics(atom_grid, reps, (uint64_t)host_adds, seed,
                                   poisoned(kHostlinkAtomics), poison_xor, ph, run);
      atomics_ran = true;
      ph.ms = hl_ms_since(t0);
    }

    unsigned kind_mask = 0;
    py::dict phase_dict;
    for (int p = 0; p < kHostlinkPhases; ++p) {
      const HlPhase& ph = phases[p];
      if (!ph.ran) continue;
      if (ph.errors != 0) kind_mask |= 1u << p;
      py::dict e;
      e["compared"] = ph.compared;
      e["expected"] = ph.expected;
      e["errors"] = ph.errors;
      e["elapsed_ms"] = ph.ms;
      e["link_ms"] = ph.link_ms;
      e["gbps"] = ph.link_ms > 0.0 ? ph.link_bytes / 1e9 / (ph.link_ms / 1e3) : 0.0;
      phase_dict[kHostlinkPhaseNames[p]] = e;
    }
    fail_mask |= kind_mask;
    py::dict k;
    k["fail_mask"] = kind_mask;
    k["phases"] = phase_dict;
    if (phases[kHostlinkDuplex].ran) k["duplex_overlap"] = overlap;
    kinds_out[kHostlinkKindNames[kind]] = k;
  }

  py::dict out;
  out["bytes"] = nbytes;
  out["words"] = words;
  out["seed"] = seed;
  out["blocks"] = grid;
  out["plan_cases"] = plan.cases.size();
  out["slot_bytes"] = plan.slot_bytes;
  out["kinds"] = kinds_out;
  out["fail_mask"] = fail_mask;
  out["error_count"] = run.error_count;
  out["xor_or"] = run.xor_or;
  out["records"] = run.records;
  out["records_dropped"] = run.dropped;
  out["atomics_supported"] = native_atomics != 0;
  if (atomics_ran)
    out["atomics"] = atomics_out;
  else
    out["atomics"] = py::none();
  out["elapsed_ms"] = hl_ms_since(run_t0);
  return out;
}

// ---------------------------------------------------------------------------
// Vector-ALU check.  Every other sweep uses the VALU only to compare what
// another unit produced; this one runs the table of vector instructions of
// valu_problems.hpp (VALU_OPS) in every wave of a grid that fills the device.
// Groups 0..5 compare bit-exactly against the host reference; group 6 (raw
// transcendentals, stochastic rounding, v_prng_b32) has no host expectation
// and requires that every lane of every wave ends with the same digest.
//
// valu_eval<KIND, IMM> is the device side of the list of ValuKind: three
// 64-bit operands in, one 64-bit result out, the same convention as
// valu_ref_lane / valu_ref_wave.  The cross-lane kinds need EXEC all ones:
// they are only ever evaluated in wave-uniform control flow (the set loop of
// the sweep, the uniform op switch of the probe).
//
// Built on the frame of cu_coverage_kernel: same grid, launch bounds, 64 KiB
// LDS claim, placement key and slot scheme, fixed work per wave.  New here:
// every compare is counted (seven 64-bit counters, the host checks them
// against waves x reps x items), every wave leaves a digest record, and the
// first kValuMaxRecords mismatches are recorded.
// ---------------------------------------------------------------------------

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

__device__ __forceinline__ uint32_t valu_dlo(uint64_t v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t valu_dhi(uint64_t v) { return (uint32_t)(v >> 32); }
__device__ __forceinline__ uint64_t valu_dpack(uint32_t lo, uint32_t hi) {
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ f32x2 valu_df2(uint64_t v) {
  return f32x2{__uint_as_float(valu_dlo(v)), __uint_as_float(valu_dhi(v))};
}
__device__ __forceinline__ uint64_t valu_dbits(f32x2 v) {
  return valu_dpack(__float_as_uint(v.x), __float_as_uint(v.y));
}

template <int KIND, int IMM>
__device__ __forceinline__ uint64_t valu_eval(uint64_t a, uint64_t b, uint64_t c) {
#if defined(__gfx950__)
// the separate multiplies and adds must stay separate
#pragma clang fp contract(off)
  const uint32_t al = valu_dlo(a), ah = valu_dhi(a), bl = valu_dlo(b),
                 cl = valu_dlo(c), ch = valu_dhi(c);
  const float fa = __uint_as_float(al), fb = __uint_as_float(bl),
              fc = __uint_as_float(cl);
  // f32
  if constexpr (KIND == kVkFmaF32) return __float_as_uint(__builtin_fmaf(fa, fb, fc));
  else if constexpr (KIND == kVkAddF32) return __float_as_uint(fa + fb);
  else if constexpr (KIND == kVkMulF32) return __float_as_uint(fa * fb);
  else if constexpr (KIND == kVkPkFmaF32)
    return valu_dbits(__builtin_elementwise_fma(valu_df2(a), valu_df2(b), valu_df2(c)));
  else if constexpr (KIND == kVkPkAddF32) return valu_dbits(valu_df2(a) + valu_df2(b));
  else if constexpr (KIND == kVkPkMulF32) return valu_dbits(valu_df2(a) * valu_df2(b));
  else if constexpr (KIND == kVkMinF32) return __float_as_uint(__builtin_fminf(fa, fb));
  else if constexpr (KIND == kVkMaxF32) return __float_as_uint(__builtin_fmaxf(fa, fb));
  else if constexpr (KIND == kVkMed3F32)
    return __float_as_uint(__builtin_amdgcn_fmed3f(fa, fb, fc));
  else if constexpr (KIND == kVkLdexpF32)
    return __float_as_uint(__builtin_ldexpf(fa, (int)bl));
  else if constexpr (KIND == kVkFrexpMantF32)
    return __float_as_uint(__builtin_amdgcn_frexp_mantf(fa));
  else if constexpr (KIND == kVkRndneF32) return __float_as_uint(__builtin_rintf(fa));
  // f64
  else if constexpr (KIND == kVkFmaF64)
    return (uint64_t)__double_as_longlong(__builtin_fma(
        __longlong_as_double((long long)a), __longlong_as_double((long long)b),
        __longlong_as_double((long long)c)));
  else if constexpr (KIND == kVkAddF64)
    return (uint64_t)__double_as_longlong(__longlong_as_double((long long)a) +
                                          __longlong_as_double((long long)b));
  else if constexpr (KIND == kVkMulF64)
    return (uint64_t)__double_as_longlong(__longlong_as_double((long long)a) *
                                          __longlong_as_double((long long)b));
  else if constexpr (KIND == kVkLdexpF64)
    return (uint64_t)__double_as_longlong(
        __builtin_ldexp(__longlong_as_double((long long)a), (int)bl));
  // f16
  else if constexpr (KIND == kVkPkFmaF16)
    return __builtin_bit_cast(
        uint32_t, __builtin_elementwise_fma(__builtin_bit_cast(f16x2, al),
                                            __builtin_bit_cast(f16x2, bl),
                                            __builtin_bit_cast(f16x2, cl)));
  else if constexpr (KIND == kVkPkAddF16)
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, al) +
                                            __builtin_bit_cast(f16x2, bl));
  else if constexpr (KIND == kVkPkMulF16)
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, al) *
                                            __builtin_bit_cast(f16x2, bl));
  else if constexpr (KIND == kVkDot2F16)
    return __float_as_uint(__builtin_amdgcn_fdot2(
        __builtin_bit_cast(f16x2, al), __builtin_bit_cast(f16x2, bl), fc, false));
  else if constexpr (KIND == kVkDot2Bf16)
    return __float_as_uint(__builtin_amdgcn_fdot2_f32_bf16(
        __builtin_bit_cast(bf16x2, al), __builtin_bit_cast(bf16x2, bl), fc, false));
  // int
  else if constexpr (KIND == kVkMadU64U32) return (uint64_t)al * bl + c;
  else if constexpr (KIND == kVkMulHiU32) return __umulhi(al, bl);
  else if constexpr (KIND == kVkMulLoU32) return al * bl;
  else if constexpr (KIND == kVkMulI24) return (uint32_t)__mul24((int)al, (int)bl);
  // hipcc adds 64-bit integers with v_lshl_add_u64 and folds a bit select
  // into v_bitop3_b32; the carry chain and v_bfi_b32 are asked for by name
  else if constexpr (KIND == kVkAddU64) {
    uint32_t lo, hi;
    asm volatile("v_add_co_u32 %0, vcc, %2, %4\n\tv_addc_co_u32 %1, vcc, %3, %5, vcc"
                 : "=&v"(lo), "=v"(hi)
                 : "v"(al), "v"(ah), "v"(bl), "v"(valu_dhi(b))
                 : "vcc");
    return valu_dpack(lo, hi);
  } else if constexpr (KIND == kVkSubU64) {
    uint32_t lo, hi;
    asm volatile("v_sub_co_u32 %0, vcc, %2, %4\n\tv_subb_co_u32 %1, vcc, %3, %5, vcc"
                 : "=&v"(lo), "=v"(hi)
                 : "v"(al), "v"(ah), "v"(bl), "v"(valu_dhi(b))
                 : "vcc");
    return valu_dpack(lo, hi);
  }
  else if constexpr (KIND == kVkLshlB32) return al << (bl & 31u);
  else if constexpr (KIND == kVkLshrB32) return al >> (bl & 31u);
  else if constexpr (KIND == kVkAshrI32) return (uint32_t)((int32_t)al >> (bl & 31u));
  else if constexpr (KIND == kVkLshlB64) return a << (bl & 63u);
  else if constexpr (KIND == kVkLshrB64) return a >> (bl & 63u);
  else if constexpr (KIND == kVkAshrI64) return (uint64_t)((int64_t)a >> (bl & 63u));
  else if constexpr (KIND == kVkBfeU32) return __builtin_amdgcn_ubfe(al, bl & 31u, cl & 31u);
  else if constexpr (KIND == kVkBfiB32) {
    uint32_t r;
    asm volatile("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(al), "v"(bl), "v"(cl));
    return r;
  }
  else if constexpr (KIND == kVkPermB32) return __builtin_amdgcn_perm(al, bl, cl);
  else if constexpr (KIND == kVkAlignbitB32) return __builtin_amdgcn_alignbit(al, bl, cl);
  else if constexpr (KIND == kVkSadU8) return __builtin_amdgcn_sad_u8(al, bl, cl);
  else if constexpr (KIND == kVkBcntU32) return (uint32_t)__builtin_popcount(al) + bl;
  else if constexpr (KIND == kVkFfbhU32) return (uint32_t)__clz((int)al);
  else if constexpr (KIND == kVkBfrevB32) return __brev(al);
  else if constexpr (KIND == kVkBitop3B32) return (uint32_t)__builtin_amdgcn_bitop3_b32(al, bl, cl, IMM);
  else if constexpr (KIND == kVkDot4I8)
    return (uint32_t)__builtin_amdgcn_sdot4((int)al, (int)bl, (int)cl, false);
  else if constexpr (KIND == kVkDot4U8) return __builtin_amdgcn_udot4(al, bl, cl, false);
  else if constexpr (KIND == kVkCmpSelect) return (int32_t)al < (int32_t)bl ? cl : ch;
  // convert
  else if constexpr (KIND == kVkCvtF16F32)
    return __builtin_bit_cast(uint16_t, (_Float16)fa);
  else if constexpr (KIND == kVkCvtPkBf16F32)
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)fa) |
           (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)__uint_as_float(ah)) << 16;
  else if constexpr (KIND == kVkCvtI32F32) return (uint32_t)(int32_t)fa;
  else if constexpr (KIND == kVkCvtU32F32) return (uint32_t)fa;
  else if constexpr (KIND == kVkCvtF32I32) return __float_as_uint((float)(int32_t)al);
  else if constexpr (KIND == kVkCvtF32U32) return __float_as_uint((float)al);
  else if constexpr (KIND == kVkCvtPkFp8F32)
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(fa, __uint_as_float(ah), (int)cl, IMM != 0);
  else if constexpr (KIND == kVkCvtPkBf8F32)
    return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(fa, __uint_as_float(ah), (int)cl, IMM != 0);
  else if constexpr (KIND == kVkCvtF32Fp8)
    return __float_as_uint(__builtin_amdgcn_cvt_f32_fp8((int)al, IMM));
  else if constexpr (KIND == kVkCvtF32Bf8)
    return __float_as_uint(__builtin_amdgcn_cvt_f32_bf8((int)al, IMM));
  else if constexpr (KIND == kVkCvtScalePkF32Fp4)
    return valu_dbits(__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(al, fb, IMM));
  else if constexpr (KIND == kVkCvtScalePkFp4F32)
    return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(cl, fa, __uint_as_float(ah), fb, IMM);
  // crosslane: a is the source, b is `old` / the second register
  else if constexpr (KIND == kVkDpp)
    return (uint32_t)__builtin_amdgcn_update_dpp(
        (int)bl, (int)al, IMM & 0xFFF, kValuDppRowMask[IMM >> 12],
        kValuDppBankMask[IMM >> 12], (IMM >> 12) != 0);
  else if constexpr (KIND == kVkReadlane) {
    const uint32_t r0 = __builtin_amdgcn_readlane((int)al, kValuReadLanes[0]);
    const uint32_t r1 = __builtin_amdgcn_readlane((int)al, kValuReadLanes[1]);
    const uint32_t r2 = __builtin_amdgcn_readlane((int)al, kValuReadLanes[2]);
    const uint32_t r3 = __builtin_amdgcn_readlane((int)al, kValuReadLanes[3]);
    const int q = (int)(__lane_id() & 3u);
    return q == 0 ? r0 : q == 1 ? r1 : q == 2 ? r2 : r3;
  } else if constexpr (KIND == kVkReadfirstlane)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)al);
  else if constexpr (KIND == kVkPermlane16Swap) {
    const auto r = __builtin_amdgcn_permlane16_swap(al, bl, false, false);
    return valu_dpack(r[0], r[1]);
  } else if constexpr (KIND == kVkPermlane32Swap) {
    const auto r = __builtin_amdgcn_permlane32_swap(al, bl, false, false);
    return valu_dpack(r[0], r[1]);
  } else if constexpr (KIND == kVkMbcnt)
    return __builtin_amdgcn_mbcnt_hi(ah, __builtin_amdgcn_mbcnt_lo(al, bl));
  else if constexpr (KIND == kVkCmpMask) return (uint64_t)__ballot(al < bl);
  // consensus: the raw instructions, no refinement sequence
  else if constexpr (KIND == kVkExpF32) return __float_as_uint(__builtin_amdgcn_exp2f(fa));
  else if constexpr (KIND == kVkLogF32) return __float_as_uint(__builtin_amdgcn_logf(fa));
  else if constexpr (KIND == kVkRcpF32) return __float_as_uint(__builtin_amdgcn_rcpf(fa));
  else if constexpr (KIND == kVkRsqF32) return __float_as_uint(__builtin_amdgcn_rsqf(fa));
  else if constexpr (KIND == kVkSqrtF32) return __float_as_uint(__builtin_amdgcn_sqrtf(fa));
  else if constexpr (KIND == kVkSinF32) return __float_as_uint(__builtin_amdgcn_sinf(fa));
  else if constexpr (KIND == kVkCosF32) return __float_as_uint(__builtin_amdgcn_cosf(fa));
  else if constexpr (KIND == kVkRcpF64)
    return (uint64_t)__double_as_longlong(
        __builtin_amdgcn_rcp(__longlong_as_double((long long)a)));
  else if constexpr (KIND == kVkRsqF64)
    return (uint64_t)__double_as_longlong(
        __builtin_amdgcn_rsq(__longlong_as_double((long long)a)));
  else if constexpr (KIND == kVkCvtSrFp8F32)
    return (uint32_t)__builtin_amdgcn_cvt_sr_fp8_f32(fa, (int)bl, 0, 0);
  else if constexpr (KIND == kVkPrngB32) return __builtin_amdgcn_prng_b32(al);
  else static_assert(KIND < 0, "valu_eval: kind without a device implementation");
#else
  return 0;
#endif
}

struct ValuRecord {
  uint32_t key, simd, group, op, set, lane, rep, pad;
  uint64_t expected, got;
};

constexpr int kValuCtlErrors = kValuGroups, kValuCtlWords = kValuGroups + 1;
constexpr int kValuWaveRecWords = 1 + kValuConsOps;  // slot + 1 | digests

struct ValuLaunch {
  const uint32_t* tab;
  uint32_t* slots;      // waves | fail | hw_id | xcc_id, as cov_tally reads them
  uint64_t* ctl;        // compared[kValuGroups] | error count
  ValuRecord* records;  // the first kValuMaxRecords mismatches
  uint64_t* wave_recs;  // [round][block][wave][kValuWaveRecWords]
  int reps, poison_key, poison_all, round;
  unsigned poison_mask;
};

struct ValuWave {
  uint32_t key, simd, fail;
  uint32_t count[kValuGroups];
  uint64_t digest[kValuConsOps];
};

__device__ __noinline__ void valu_mismatch(uint64_t* ctl, ValuRecord* records,
                                           uint32_t key,
                                           uint32_t simd, int group, int op, int set,
                                           int lane, int rep, uint64_t expected,
                                           uint64_t got) {
  // the error counter is the claim counter: one atomic per mismatch
  const ValuRecord r = {key, simd, (uint32_t)group, (uint32_t)op, (uint32_t)set,
                        (uint32_t)lane, (uint32_t)rep, 0u, expected, got};
  record_log_claim(RecordLogView<ValuRecord>{(unsigned long long*)&ctl[kValuCtlErrors],
                                             records, kValuMaxRecords},
                   [&] { return r; });
}

template <int OP>
__device__ __forceinline__ void valu_step(const ValuLaunch& L, int lane, int rep,
                                          unsigned pm, ValuWave& w) {
#if defined(__gfx950__)
  constexpr int KIND = kValuOpKind[OP], IMM = kValuOpImm[OP], G = kValuOpGroup[OP];
  // volatile: operands and expected words are re-read from global memory
  // every repetition, so neither the op nor the compare can be hoisted; the
  // lane's base is opaque to the optimizer, or the address of every op's
  // records is hoisted out of the repetition loop and spills
  const uint32_t* lane_base = L.tab + (size_t)lane * kValuRecWords;
  asm volatile("" : "+v"(lane_base));
  if constexpr (G != kValuGroupConsensus) {
#pragma unroll 1
    for (int set = 0; set < kValuSets; ++set) {
      const uint32_t* rec =
          lane_base + (size_t)((OP * kValuSets + set) * 64) * kValuRecWords;
      const volatile u32x4* p = (const volatile u32x4*)rec;  // 32-byte records
      const u32x4 ab = p[0], ce = p[1];
      const uint64_t a = valu_dpack(ab[0], ab[1]), b = valu_dpack(ab[2], ab[3]),
                     c = valu_dpack(ce[0], ce[1]);
      // test hook: flips bit 0 of the *expected* value
      const uint64_t want = valu_dpack(ce[2], ce[3]) ^ (uint64_t)((pm >> G) & 1u);
      const uint64_t got = valu_eval<KIND, IMM>(a, b, c);
      ++w.count[G];
      if (got != want) {
        w.fail |= 1u << G;
        valu_mismatch(L.ctl, L.records, w.key, w.simd, G, OP, set, lane, rep, want, got);
      }
    }
  } else {
    // every lane runs all inputs, from a rotation of its own; the digest is
    // an order-independent sum, so all 64 lanes must end with the same value
    uint64_t digest = 0;
#pragma unroll 1
    for (int i = 0; i < kValuConsInputs; ++i) {
      const int idx = (i + 5 * lane) & (kValuConsInputs - 1);
      const uint32_t* rec =
          L.tab + (size_t)(OP * kValuSets * 64 + idx) * kValuRecWords;
      asm volatile("" : "+v"(rec));
      const u32x4 ab = *(const volatile u32x4*)rec;
      const uint64_t a = valu_dpack(ab[0], ab[1]), b = valu_dpack(ab[2], ab[3]);
      digest += valu_digest_term((uint32_t)OP, (uint32_t)idx,
                                 valu_eval<KIND, IMM>(a, b, 0));
      ++w.count[G];
    }
    const uint64_t first =
        valu_dpack((uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)digest),
                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(digest >> 32)));
    if (digest != first) {
      w.fail |= 1u << G;
      valu_mismatch(L.ctl, L.records, w.key, w.simd, G, OP, 0, lane, rep, first, digest);
    }
    w.digest[OP - kValuExactOps] = digest;
  }
#endif
}
static_assert((kValuConsInputs & (kValuConsInputs - 1)) == 0, "valu_step: rotation mask");

template <int... OPS>
__device__ __forceinline__ void valu_all_ops(std::integer_sequence<int, OPS...>,
                                             const ValuLaunch& L, int lane, int rep,
                                             unsigned pm, ValuWave& w) {
  (valu_step<OPS>(L, lane, rep, pm, w), ...);
}

__global__ void __launch_bounds__(kCovBlock, kCovBlocksPerCu)
valu_coverage_kernel(ValuLaunch L) {
#if defined(__gfx950__)
  __shared__ uint32_t lds[kCovLdsWords];  // the claim that keeps 2 per CU
  const uint32_t hw_id = __builtin_amdgcn_s_getreg(kCovHwRegHwId);
  const uint32_t xcc_id = __builtin_amdgcn_s_getreg(kCovHwRegXccId);
  ValuWave w = {};
  w.key = ((xcc_id & 0xFu) << 8) | ((hw_id >> 8) & 0xFFu);
  w.simd = (hw_id >> 4) & 3u;
  const unsigned pm =
      (L.poison_all || (int)w.key == L.poison_key) ? L.poison_mask : 0u;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
#pragma unroll 1
  for (int rep = 0; rep < L.reps; ++rep)
    valu_all_ops(std::make_integer_sequence<int, kValuOps>{}, L, lane, rep, pm, w);

  // the masks pass through LDS once (neighbouring lanes swap theirs), which
  // keeps the static claim alive; the wave-wide OR below makes it a no-op
  lds[tid * 64] = w.fail;  // tid < 256: index < kCovLdsWords
  __syncthreads();
  w.fail |= lds[(tid ^ 1) * 64];

  // counted, not trusted: the wave's compares per group, summed by lane
  // shuffles, added once to the global counters
#pragma unroll
  for (int g = 0; g < kValuGroups; ++g) {
    uint32_t n = w.count[g];
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (lane == 0) atomicAdd((unsigned long long*)&L.ctl[g], (unsigned long long)n);
  }

  unsigned wave_fail = 0;
  for (int b = 0; b < kValuGroups; ++b)
    if (__ballot((w.fail >> b) & 1u) != 0) wave_fail |= 1u << b;
  if (lane == 0) {
    const uint32_t slot = w.key * 4u + w.simd;  // < kCovSlots by the masks above
    atomicAdd(&L.slots[slot], 1u);
    if (wave_fail) atomicOr(&L.slots[kCovSlots + slot], wave_fail);
    L.slots[2 * kCovSlots + slot] = hw_id;
    L.slots[3 * kCovSlots + slot] = xcc_id;
    // [round][block][wave]: round < max_rounds, block < gridDim.x, wave < 4,
    // which is how the host sized the array
    uint64_t* wr = L.wave_recs +
                   ((size_t)(L.round * gridDim.x + blockIdx.x) * (kCovBlock / 64) +
                    (tid >> 6)) * kValuWaveRecWords;
    wr[0] = slot + 1u;
    // test hook: bit 6 flips bit 0 of the digests this unit *reports*
#pragma unroll
    for (int i = 0; i < kValuConsOps; ++i)
      wr[1 + i] = w.digest[i] ^ (uint64_t)((pm >> kValuGroupConsensus) & 1u);
  }
#endif
}

template <int OP>
__device__ __forceinline__ void valu_probe_one(int op, uint64_t a, uint64_t b,
                                               uint64_t c, uint64_t& r) {
  if (op == OP) r = valu_eval<kValuOpKind[OP], kValuOpImm[OP]>(a, b, c);  // uniform
}
template <int... OPS>
__device__ __forceinline__ void valu_probe_all(std::integer_sequence<int, OPS...>,
                                               int op, uint64_t a, uint64_t b,
                                               uint64_t c, uint64_t& r) {
  (valu_probe_one<OPS>(op, a, b, c, r), ...);
}

// one wave, one op: in[0..63] a, in[64..127] b, in[128..191] c
__global__ void __launch_bounds__(64, 1)
valu_probe_kernel(int op, const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
#if defined(__gfx950__)
  const int lane = threadIdx.x;  // < 64
  uint64_t r = 0;
  valu_probe_all(std::make_integer_sequence<int, kValuOps>{}, op, in[lane],
                 in[64 + lane], in[128 + lane], r);
  out[lane] = r;
#endif
}

static py::dict valu_reference() {
  // host only: no HIP call
  py::dict out;
  out["sets"] = kValuSets;
  out["lanes"] = 64;
  py::list groups, items, ops;
  for (int g = 0; g < kValuGroups; ++g) {
    groups.append(kValuGroupNames[g]);
    items.append(valu_items(g));
  }
  for (int op = 0; op < kValuOps; ++op) {
    const ValuProblem p = valu_problem(op);
    py::dict e;
    e["name"] = kValuOpTable[op].name;
    e["group"] = kValuGroupNames[kValuOpGroup[op]];
    e["a"] = p.a;
    e["b"] = p.b;
    e["c"] = p.c;
    if (p.expected.empty())
      e["expected"] = py::none();
    else
      e["expected"] = p.expected;
    ops.append(e);
  }
  out["groups"] = groups;
  out["items"] = items;
  out["ops"] = ops;
  out["consensus_inputs"] = kValuConsInputs;
  return out;
}

static std::vector<uint64_t> valu_probe(int device, const std::string& op_name,
                                        const std::vector<uint64_t>& a,
                                        const std::vector<uint64_t>& b,
                                        const std::vector<uint64_t>& c) {
  // everything is validated on the host before the first HIP call
  const int op = valu_op_index(op_name);
  if (a.size() != 64 || b.size() != 64 || c.size() != 64)
    throw std::invalid_argument("valu_probe: a, b and c take 64 lanes each");
  if (kValuOpGroup[op] == kValuGroupConsensus) {
    for (int l = 0; l < 64; ++l)
      valu_check_consensus_operand(kValuOpKind[op], a[l], b[l]);
  } else {
    std::vector<uint64_t> ref(64);
    try {
      valu_ref_wave(op, a.data(), b.data(), c.data(), ref.data());
    } catch (const std::domain_error& e) {
      throw std::invalid_argument(std::string("valu_probe: ") + e.what());
    }
  }
  std::vector<uint64_t> in(192), out(64);
  std::copy(a.begin(), a.end(), in.begin());
  std::copy(b.begin(), b.end(), in.begin() + 64);
  std::copy(c.begin(), c.end(), in.begin() + 128);
  HIP_CHECK(hipSetDevice(device));
  DeviceBuf<uint64_t> d_in(in.size()), d_out(out.size());
  d_in.upload(in.data(), in.size());
  d_out.fill(0);
  hipLaunchKernelGGL(valu_probe_kernel, dim3(1), dim3(64), 0, 0, op, d_in.get(),
                     d_out.get());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  d_out.download(out.data(), out.size());
  return out;
}

static py::dict valu_coverage_check(int device, int reps, int max_rounds,
                                    int poison_key, unsigned poison_mask,
                                    bool poison_all) {
  if (poison_all && ((poison_mask >> kValuGroupConsensus) & 1u))
    throw std::invalid_argument(
        "valu_coverage_check: poison_all with the consensus bit cannot be "
        "detected: a consensus poisoned everywhere is still a consensus");
  const std::string who = "valu_coverage_check";
  cov_validate(who, reps, max_rounds, poison_key, poison_mask, kValuGroups);
  const int cus = cov_select_device(who, device);
  const int blocks = kCovBlocksPerCu * cus;
  RecordLog<ValuRecord> log(kValuMaxRecords, kValuCtlWords, kValuCtlErrors);
  DeviceBuf<uint64_t> d_wave((size_t)max_rounds * blocks * (kCovBlock / 64) *
                             kValuWaveRecWords);
  d_wave.fill(0);
  const SweepRun run = cov_run_sweep(
      cus, max_rounds, valu_build_table(),
      [&](int round, uint32_t* tab, uint32_t* slots) {
        ValuLaunch L;
        L.tab = tab, L.slots = slots, L.ctl = (uint64_t*)log.ctl();
        L.records = log.view(kValuMaxRecords).records;
        L.wave_recs = d_wave.get();
        L.reps = reps, L.poison_key = poison_key, L.poison_all = poison_all ? 1 : 0;
        L.round = round;  // < max_rounds, which is how d_wave is sized
        L.poison_mask = poison_mask;
        hipLaunchKernelGGL(valu_coverage_kernel, dim3(blocks), dim3(kCovBlock), 0,
                           0, L);
      });

  const auto taken = log.collect(kValuMaxRecords);
  const std::vector<unsigned long long>& ctl = taken.ctl;
  std::vector<uint64_t> wave(d_wave.size());
  d_wave.download(wave.data(), wave.size());

  // per slot, the distinct digest tuples its waves reported
  const auto by_slot = valu_group_digests(
      wave.data(), (size_t)run.rounds * blocks * (kCovBlock / 64), kValuWaveRecWords);
  py::dict out = cov_sweep_dict(run);
  py::list units = out["units"];  // in the order of run.tally.units
  for (size_t i = 0; i < run.tally.units.size(); ++i) {
    const CovUnit& c = run.tally.units[i];
    units[i]["digests"] = by_slot[c.key * 4 + c.simd];
  }

  py::list compared, items, cons_ops, records;
  for (int g = 0; g < kValuGroups; ++g) {
    compared.append(ctl[g]);
    items.append(valu_items(g));
  }
  for (int op = kValuExactOps; op < kValuOps; ++op) cons_ops.append(kValuOpTable[op].name);
  const uint64_t errors = taken.claims, kept = taken.records.size();
  for (const ValuRecord& r : taken.records) {
    py::dict e;
    e["key"] = r.key;
    e["simd"] = r.simd;
    e["group"] = r.group < (uint32_t)kValuGroups ? kValuGroupNames[r.group] : "?";
    e["op"] = r.op < (uint32_t)kValuOps ? kValuOpTable[r.op].name : "?";
    e["set"] = r.set;
    e["lane"] = r.lane;
    e["rep"] = r.rep;
    e["expected"] = r.expected;
    e["got"] = r.got;
    records.append(e);
  }
  out["reps"] = reps;
  out["compared"] = compared;
  out["items"] = items;
  out["consensus_ops"] = cons_ops;
  out["records"] = records;
  out["records_dropped"] = errors - kept;
  out["error_count"] = errors;
  return out;
}


PYBIND11_MODULE(_gpu_validator, m) {
  m.doc() = "MI355X (gfx950) native GPU health validator";
  m.def("valu_coverage_check", &valu_coverage_check, py::arg("device") = 0,
        py::arg("reps") = 4, py::arg("max_rounds") = 8,
        py::arg("poison_key") = -1, py::arg("poison_mask") = 0u,
        py::arg("poison_all") = false,
        "Whole-device vector-ALU sweep: arithmetic, conversions and cross-lane "
        "ops bit-exact, transcendentals by consensus, compares counted, per "
        "(XCC, CU, SIMD)");
  m.def("valu_reference", &valu_reference,
        "Host-only: operands, expected words, items and op names of the "
        "vector-ALU sweep");
  m.def("valu_probe", &valu_probe, py::arg("device"), py::arg("op"), py::arg("a"),
        py::arg("b"), py::arg("c"),
        "Run one op of the vector-ALU table on one wave over the caller's "
        "64-lane operands; returns the 64 raw results");
  m.def("host_link_check", &host_link_check, py::arg("device") = 0,
        py::arg("nbytes") = 64ull << 20, py::arg("seed") = 1ull,
        py::arg("kinds") =
            std::vector<std::string>{"pinned", "registered", "pageable"},
        py::arg("blocks") = 0, py::arg("atomics_blocks") = 0, py::arg("reps") = 2,
        py::arg("host_adds") = (int64_t)4096, py::arg("max_records") = 64,
        py::arg("poison_mask") = 0u, py::arg("poison_kind") = -1,
        py::arg("poison_word") = (int64_t)-1, py::arg("poison_case") = (int64_t)-1,
        py::arg("poison_xor") = 1ull,
        "Host-link data-integrity check: DMA copies in both directions, "
        "zero-copy kernel access, duplex copies, unaligned copies and "
        "system-scope atomics on pinned, registered and pageable host memory, "
        "exact, coverage counted, failing words and cases recorded");
  m.def("host_link_plan", &host_link_plan,
        "Host-only: the unaligned copy plan of host_link_check");
  m.def("host_link_reference", &host_link_reference, py::arg("seed") = 1ull,
        py::arg("threads") = 0ull, py::arg("reps") = 2,
        py::arg("host_adds") = (int64_t)4096,
        "Host-only: the expected add cells of the host-link atomics phase");
  m.def("lds_integrity_check", &lds_integrity_check, py::arg("device") = 0,
        py::arg("reps") = 2, py::arg("passes") = 3, py::arg("max_rounds") = 8,
        py::arg("seed") = 1ull, py::arg("blocks") = 0, py::arg("poison_key") = -1,
        py::arg("poison_mask") = 0u, py::arg("poison_all") = false,
        py::arg("poison_word") = -1, py::arg("poison_xor") = 1ull,
        "LDS data-integrity check: all 160 KiB of every CU through moving "
        "inversions in three widths, sub-word stores, transposed reads, direct "
        "global->LDS loads, the LDS atomic ALU and the permute crossbar, exact, "
        "coverage counted, failures attributed per CU and word");
  m.def("lds_integrity_reference", &lds_integrity_reference, py::arg("seed") = 1ull,
        py::arg("block") = 0, py::arg("rep") = 0, py::arg("passes") = 3,
        "Host-only: the expected LDS images, one transposed read, the atomic "
        "totals and the permute results of one workgroup and repetition");
  m.def("lds_tr_tile", &lds_tr_tile, py::arg("device"), py::arg("image_u16"),
        py::arg("lane_byte_offsets"),
        "Run one ds_read_b64_tr_b16 over a caller-supplied 16-bit LDS image "
        "with 64 caller-supplied byte addresses; returns 64 x 4 raw elements");
  m.def("xcd_fabric_check", &xcd_fabric_check, py::arg("device") = 0,
        py::arg("reps") = 8, py::arg("group") = 16, py::arg("slab_lines") = 8,
        py::arg("cells") = 64, py::arg("blocks") = 0, py::arg("max_rounds") = 8,
        py::arg("seed") = 1ull, py::arg("max_records") = 64,
        py::arg("poison_mask") = 0u, py::arg("poison_pair") = -1,
        "Cross-XCD check: a wait-free last-arriver hand-off sweep (agent-scope "
        "release, ticket, acquire) and a device-scope atomics sweep, exact, "
        "coverage counted, failures attributed per (writer, reader) XCC pair");
  m.def("xcd_fabric_reference", &xcd_fabric_reference, py::arg("blocks"),
        py::arg("seed") = 1ull, py::arg("reps") = 8, py::arg("group") = 16,
        py::arg("slab_lines") = 8, py::arg("cells") = 64, py::arg("round") = 0,
        py::arg("rep") = 0, py::arg("block") = 0, py::arg("line") = 0,
        py::arg("threads") = 0ull,
        "Host-only: the header and payload words of one line of the hand-off "
        "slabs and, for a thread count, the expected atomic totals");
  m.def("hbm_pattern_check", &hbm_pattern_check, py::arg("device") = 0,
        py::arg("nbytes") = 1ull << 30, py::arg("chunk_bytes") = 1ull << 30,
        py::arg("passes") = 1, py::arg("seed") = 1ull, py::arg("checker") = true,
        py::arg("first_word") = 0ull, py::arg("max_records") = 64,
        py::arg("poison_word") = (int64_t)-1, py::arg("poison_stride") = 0ull,
        py::arg("poison_xor") = 0ull, py::arg("poison_phase") = -1,
        "Moving-inversions pattern test over nbytes of device memory (0 = all "
        "free memory minus a 2 GiB reserve), exact comparison, coverage "
        "counted, mismatches recorded per word");
  m.def("hbm_pattern_reference", &hbm_pattern_reference, py::arg("pattern"),
        py::arg("seed"), py::arg("first_word"), py::arg("count"),
        py::arg("inverted") = false,
        "Host-only: up to 65536 expected words of a pattern from first_word");
  m.def("cu_coverage_check", &cu_coverage_check, py::arg("device") = 0,
        py::arg("reps") = 32, py::arg("max_rounds") = 8,
        py::arg("poison_key") = -1, py::arg("poison_mask") = 0u,
        py::arg("poison_all") = false,
        "Whole-device sweep: f32/bf16/fp8 MFMA tiles + LDS round trip on every "
        "CU and SIMD, exact comparison, results per placement key");
  m.def("mx_coverage_check", &mx_coverage_check, py::arg("device") = 0,
        py::arg("reps") = 16, py::arg("max_rounds") = 8,
        py::arg("poison_key") = -1, py::arg("poison_mask") = 0u,
        py::arg("poison_all") = false,
        "Whole-device sweep of the MX block-scaled MFMA path (five formats, "
        "mixed pairs, both shapes) on every CU and SIMD, exact comparison, "
        "results per placement key");
  m.def("mx_reference", &mx_reference,
        "Host-only: the MX sweep's problems as raw operand and scale codes, "
        "packed lane words, expected tiles and achieved log2(S/q)");
  m.def("mx_mfma_tile", &mx_mfma_tile, py::arg("device") = 0,
        py::arg("fmt_a") = "e2m1", py::arg("fmt_b") = "e2m1",
        py::arg("shape") = "16x16x128", py::arg("set") = 0,
        "Run one scaled MFMA tile; returns the raw problem + GPU output for "
        "independent verification");
  m.def("mx_throughput_tflops", &mx_throughput_tflops, py::arg("device") = 0,
        py::arg("fmt") = "e2m1", py::arg("iters") = 20000,
        "Sustained MX (e2m1 or e4m3, 16x16x128) matrix-core throughput in "
        "TFLOP/s (burn-in check)");
  m.def("cu_coverage_reference", &cu_coverage_reference,
        "Host-only: the sweep's operand sets (decoded to f32) and expected "
        "tiles per dtype");
  m.def("device_probe", &device_probe, py::arg("device") = 0);
  m.def("mfma_f32_check", &mfma_f32_check, py::arg("device") = 0,
        "Max abs error of a v_mfma_f32_16x16x4_f32 tile vs exact CPU fmaf chain");
  m.def("mfma_bf16_check", &mfma_bf16_check, py::arg("device") = 0,
        "Max abs error of a v_mfma_f32_16x16x32_bf16 tile vs f32 CPU reference");
  m.def("hbm_bandwidth_gbps", &hbm_bandwidth_gbps, py::arg("device") = 0,
        py::arg("buf_mib") = 1024.0, py::arg("iters") = 10,
        "Streaming float4 copy bandwidth in GB/s (read+write)");
  m.def("lds_roundtrip_check", &lds_roundtrip_check, py::arg("device") = 0);
  m.def("mfma_bf16_tile", &mfma_bf16_tile, py::arg("device") = 0,
        "Run one bf16 MFMA tile; returns quantized inputs + GPU output for "
        "independent (e.g. torch fp32) verification");
  m.def("mfma_fp8_check", &mfma_fp8_check, py::arg("device") = 0,
        "Max abs error of a v_mfma_f32_16x16x32_fp8_fp8 (OCP e4m3) tile vs "
        "f32 CPU reference");
  m.def("mfma_throughput_tflops", &mfma_throughput_tflops, py::arg("device") = 0,
        py::arg("iters") = 200000,
        "Sustained bf16 matrix-core throughput in TFLOP/s (burn-in check)");
  m.def("xgmi_p2p_probe", &xgmi_p2p_probe, py::arg("device") = 0,
        py::arg("buf_mib") = 256.0, py::arg("iters") = 5,
        "Peer accessibility + p2p copy bandwidth (GB/s) to every other GPU");
}
