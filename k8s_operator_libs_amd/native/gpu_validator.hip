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
//
// Built standalone with hipcc (no torch linkage) via pybind11; the .so lives
// in-tree so it travels to GPU nodes with the package.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cmath>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace py = pybind11;

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error at " #expr ": ") +       \
                               hipGetErrorString(_e));                         \
    }                                                                          \
  } while (0)

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

static float decode_e4m3fn(uint8_t u) {
  int s = (u >> 7) & 1;
  int e = (u >> 3) & 0xF;
  int m = u & 7;
  float v;
  if (e == 0) {
    v = (float)m / 8.0f * (1.0f / 64.0f);  // subnormal: 2^-6 scale
  } else if (e == 15 && m == 7) {
    v = 0.0f;  // NaN code; never produced by our encoder
  } else {
    v = (1.0f + (float)m / 8.0f) * std::ldexp(1.0f, e - 7);
  }
  return s ? -v : v;
}

static uint8_t encode_e4m3fn_nearest(float f) {
  // exact nearest-representable search over the 256-code table (fine for a
  // smoke test; avoids re-deriving RNE tie rules)
  uint8_t best = 0;
  float best_err = 1e30f;
  for (int u = 0; u < 256; ++u) {
    if ((u & 0x7F) == 0x7F) continue;  // NaN codes
    float err = std::fabs(decode_e4m3fn((uint8_t)u) - f);
    if (err < best_err) {
      best_err = err;
      best = (uint8_t)u;
    }
  }
  return best;
}

static py::dict mfma_bf16_tile(int device) {
  // Run the bf16 MFMA tile and return decoded inputs + GPU output so Python
  // tests can verify against an independent fp32 reference (e.g. torch).
  HIP_CHECK(hipSetDevice(device));
  const int M = 16, N = 16, K = 32;
  std::vector<float> hAf(M * K), hBf(K * N), hD(M * N);
  std::vector<uint16_t> hA(M * K), hB(K * N);
  auto to_bf16 = [](float f) -> uint16_t {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    uint32_t rounded = u + 0x7FFF + ((u >> 16) & 1);
    return (uint16_t)(rounded >> 16);
  };
  auto from_bf16 = [](uint16_t v) -> float {
    uint32_t u = (uint32_t)v << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
  };
  for (int i = 0; i < M * K; ++i) hA[i] = to_bf16(0.07f * (float)((i * 13) % 41) - 1.2f);
  for (int i = 0; i < K * N; ++i) hB[i] = to_bf16(0.05f * (float)((i * 17) % 37) - 0.8f);
  for (int i = 0; i < M * K; ++i) hAf[i] = from_bf16(hA[i]);
  for (int i = 0; i < K * N; ++i) hBf[i] = from_bf16(hB[i]);
  uint16_t *dA, *dB;
  float* dD;
  HIP_CHECK(hipMalloc(&dA, sizeof(uint16_t) * M * K));
  HIP_CHECK(hipMalloc(&dB, sizeof(uint16_t) * K * N));
  HIP_CHECK(hipMalloc(&dD, sizeof(float) * M * N));
  HIP_CHECK(hipMemcpy(dA, hA.data(), sizeof(uint16_t) * M * K, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dB, hB.data(), sizeof(uint16_t) * K * N, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_bf16_16x16x32_kernel, dim3(1), dim3(64), 0, 0,
                     (const __bf16*)dA, (const __bf16*)dB, dD);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(hD.data(), dD, sizeof(float) * M * N, hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(dA));
  HIP_CHECK(hipFree(dB));
  HIP_CHECK(hipFree(dD));
  py::dict out;
  out["m"] = M;
  out["n"] = N;
  out["k"] = K;
  out["a"] = hAf;  // bf16-quantized values as f32, row-major MxK
  out["b"] = hBf;  // row-major KxN
  out["d"] = hD;   // GPU MFMA result, row-major MxN
  return out;
}

static double mfma_fp8_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const int M = 16, N = 16, K = 32;
  std::vector<uint8_t> hA(M * K), hB(K * N);
  std::vector<float> hD(M * N), ref(M * N);
  for (int i = 0; i < M * K; ++i)
    hA[i] = encode_e4m3fn_nearest(0.05f * (float)((i * 5) % 23) - 0.5f);
  for (int i = 0; i < K * N; ++i)
    hB[i] = encode_e4m3fn_nearest(0.03f * (float)((i * 7) % 19) - 0.25f);
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k)
        acc = fmaf(decode_e4m3fn(hA[m * K + k]), decode_e4m3fn(hB[k * N + n]), acc);
      ref[m * N + n] = acc;
    }
  uint8_t *dA, *dB;
  float* dD;
  HIP_CHECK(hipMalloc(&dA, M * K));
  HIP_CHECK(hipMalloc(&dB, K * N));
  HIP_CHECK(hipMalloc(&dD, sizeof(float) * M * N));
  HIP_CHECK(hipMemcpy(dA, hA.data(), M * K, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dB, hB.data(), K * N, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_fp8_16x16x32_kernel, dim3(1), dim3(64), 0, 0, dA, dB, dD);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(hD.data(), dD, sizeof(float) * M * N, hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(dA));
  HIP_CHECK(hipFree(dB));
  HIP_CHECK(hipFree(dD));
  double max_err = 0.0;
  for (int i = 0; i < M * N; ++i)
    max_err = std::max(max_err, (double)std::fabs(hD[i] - ref[i]));
  return max_err;
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
  // tiny bf16 operands around 1e-3 so accumulators stay finite
  std::vector<uint16_t> hseed(256);
  for (int i = 0; i < 256; ++i) {
    float f = 0.001f + 0.00001f * (float)(i % 17);
    uint32_t u;
    std::memcpy(&u, &f, 4);
    hseed[i] = (uint16_t)(u >> 16);
  }
  const int block = 256, grid = 1024;  // 4096 waves = 4 per SIMD
  uint16_t* dseed;
  float* dout;
  HIP_CHECK(hipMalloc(&dseed, sizeof(uint16_t) * 256));
  HIP_CHECK(hipMalloc(&dout, sizeof(float) * block * grid));
  HIP_CHECK(hipMemcpy(dseed, hseed.data(), sizeof(uint16_t) * 256,
                      hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_burn_kernel, dim3(grid), dim3(block), 0, 0,
                     (const __bf16*)dseed, dout, 1000);  // warmup
  HIP_CHECK(hipDeviceSynchronize());
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0));
  hipLaunchKernelGGL(mfma_burn_kernel, dim3(grid), dim3(block), 0, 0,
                     (const __bf16*)dseed, dout, iters);
  HIP_CHECK(hipEventRecord(t1));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipEventDestroy(t0));
  HIP_CHECK(hipEventDestroy(t1));
  HIP_CHECK(hipFree(dseed));
  HIP_CHECK(hipFree(dout));
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

static double mfma_f32_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const int M = 16, N = 16, K = 4;
  std::vector<float> hA(M * K), hB(K * N), hD(M * N), ref(M * N);
  // asymmetric operands so transposed writes can't pass (guide §3 note)
  for (int i = 0; i < M * K; ++i) hA[i] = 0.01f * (float)(i % 37) - 0.15f;
  for (int i = 0; i < K * N; ++i) hB[i] = 0.02f * (float)((i * 7) % 23) - 0.2f;
  // exact CPU reference: k-ordered fmaf chain (guide: bitwise equal)
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(hA[m * K + k], hB[k * N + n], acc);
      ref[m * N + n] = acc;
    }
  float *dA, *dB, *dD;
  HIP_CHECK(hipMalloc(&dA, sizeof(float) * M * K));
  HIP_CHECK(hipMalloc(&dB, sizeof(float) * K * N));
  HIP_CHECK(hipMalloc(&dD, sizeof(float) * M * N));
  HIP_CHECK(hipMemcpy(dA, hA.data(), sizeof(float) * M * K, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dB, hB.data(), sizeof(float) * K * N, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_f32_16x16x4_kernel, dim3(1), dim3(64), 0, 0, dA, dB, dD);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(hD.data(), dD, sizeof(float) * M * N, hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(dA));
  HIP_CHECK(hipFree(dB));
  HIP_CHECK(hipFree(dD));
  double max_err = 0.0;
  for (int i = 0; i < M * N; ++i)
    max_err = std::max(max_err, (double)std::fabs(hD[i] - ref[i]));
  return max_err;
}

static double mfma_bf16_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const int M = 16, N = 16, K = 32;
  std::vector<float> hAf(M * K), hBf(K * N), hD(M * N), ref(M * N);
  std::vector<uint16_t> hA(M * K), hB(K * N);
  auto to_bf16 = [](float f) -> uint16_t {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    // round-to-nearest-even truncation
    uint32_t rounded = u + 0x7FFF + ((u >> 16) & 1);
    return (uint16_t)(rounded >> 16);
  };
  auto from_bf16 = [](uint16_t v) -> float {
    uint32_t u = (uint32_t)v << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
  };
  for (int i = 0; i < M * K; ++i) hAf[i] = 0.03f * (float)((i * 3) % 29) - 0.4f;
  for (int i = 0; i < K * N; ++i) hBf[i] = 0.015f * (float)((i * 11) % 31) - 0.2f;
  for (int i = 0; i < M * K; ++i) hA[i] = to_bf16(hAf[i]);
  for (int i = 0; i < K * N; ++i) hB[i] = to_bf16(hBf[i]);
  // f32 CPU reference over the bf16-quantized operands
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k)
        acc = fmaf(from_bf16(hA[m * K + k]), from_bf16(hB[k * N + n]), acc);
      ref[m * N + n] = acc;
    }
  uint16_t *dA, *dB;
  float* dD;
  HIP_CHECK(hipMalloc(&dA, sizeof(uint16_t) * M * K));
  HIP_CHECK(hipMalloc(&dB, sizeof(uint16_t) * K * N));
  HIP_CHECK(hipMalloc(&dD, sizeof(float) * M * N));
  HIP_CHECK(hipMemcpy(dA, hA.data(), sizeof(uint16_t) * M * K, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dB, hB.data(), sizeof(uint16_t) * K * N, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_bf16_16x16x32_kernel, dim3(1), dim3(64), 0, 0,
                     (const __bf16*)dA, (const __bf16*)dB, dD);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(hD.data(), dD, sizeof(float) * M * N, hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(dA));
  HIP_CHECK(hipFree(dB));
  HIP_CHECK(hipFree(dD));
  double max_err = 0.0;
  for (int i = 0; i < M * N; ++i)
    max_err = std::max(max_err, (double)std::fabs(hD[i] - ref[i]));
  return max_err;
}

static double hbm_bandwidth_gbps(int device, double buf_mib, int iters) {
  HIP_CHECK(hipSetDevice(device));
  size_t bytes = (size_t)(buf_mib * 1024.0 * 1024.0);
  size_t n = bytes / sizeof(float4);
  bytes = n * sizeof(float4);
  float4 *src, *dst;
  HIP_CHECK(hipMalloc(&src, bytes));
  HIP_CHECK(hipMalloc(&dst, bytes));
  HIP_CHECK(hipMemset(src, 1, bytes));
  // sweep-tuned launch shape (see header comment): block 512, grid scaled to
  // ~2 float4 per thread, capped at the sweep's best 131072
  int block = 512;
  long want = (long)(n / (2 * (size_t)block)) + 1;
  int grid = (int)std::min<long>(131072, std::max<long>(1024, want));
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  // warmup
  hipLaunchKernelGGL(bw_copy_kernel, dim3(grid), dim3(block), 0, 0, src, dst, n);
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipEventRecord(t0));
  for (int i = 0; i < iters; ++i)
    hipLaunchKernelGGL(bw_copy_kernel, dim3(grid), dim3(block), 0, 0, src, dst, n);
  HIP_CHECK(hipEventRecord(t1));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipEventDestroy(t0));
  HIP_CHECK(hipEventDestroy(t1));
  HIP_CHECK(hipFree(src));
  HIP_CHECK(hipFree(dst));
  // read + write
  double gb = 2.0 * (double)bytes * iters / 1e9;
  return gb / ((double)ms / 1e3);
}

static bool lds_roundtrip_check(int device) {
  HIP_CHECK(hipSetDevice(device));
  const int blocks = 512, n = blocks * 1024;
  std::vector<float> hin(n), hout(n);
  for (int i = 0; i < n; ++i) hin[i] = (float)(i % 977) * 0.5f;
  float *din, *dout;
  HIP_CHECK(hipMalloc(&din, sizeof(float) * n));
  HIP_CHECK(hipMalloc(&dout, sizeof(float) * n));
  HIP_CHECK(hipMemcpy(din, hin.data(), sizeof(float) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lds_roundtrip_kernel, dim3(blocks), dim3(256), 0, 0, din, dout, n);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(hout.data(), dout, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(din));
  HIP_CHECK(hipFree(dout));
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
    void* src = nullptr;
    void* dst = nullptr;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipMalloc(&src, bytes));
    HIP_CHECK(hipMemset(src, 1, bytes));
    HIP_CHECK(hipSetDevice(peer));
    HIP_CHECK(hipMalloc(&dst, bytes));
    HIP_CHECK(hipSetDevice(device));
    hipEvent_t t0, t1;
    HIP_CHECK(hipEventCreate(&t0));
    HIP_CHECK(hipEventCreate(&t1));
    HIP_CHECK(hipMemcpyPeer(dst, peer, src, device, bytes));  // warmup
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipEventRecord(t0));
    for (int i = 0; i < iters; ++i)
      HIP_CHECK(hipMemcpyPeer(dst, peer, src, device, bytes));
    HIP_CHECK(hipEventRecord(t1));
    HIP_CHECK(hipEventSynchronize(t1));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
    entry["bandwidth_gbps"] = ((double)bytes * iters / 1e9) / ((double)ms / 1e3);
    HIP_CHECK(hipEventDestroy(t0));
    HIP_CHECK(hipEventDestroy(t1));
    HIP_CHECK(hipFree(src));
    HIP_CHECK(hipSetDevice(peer));
    HIP_CHECK(hipFree(dst));
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

constexpr int kCovSets = 4;                 // operand sets per repetition
constexpr int kCovLdsWords = 16384;         // 64 KiB static LDS per workgroup
constexpr int kCovKeys = 4096;              // 4 XCC bits + 8 HW_ID bits
constexpr int kCovSlots = kCovKeys * 4;     // x 4 SIMDs
constexpr int kCovBlock = 256;              // one wave per SIMD, normally
constexpr int kCovBlocksPerCu = 2;          // floor(160 KiB / 64 KiB)
constexpr unsigned kCovFailF32 = 1u, kCovFailBf16 = 2u, kCovFailFp8 = 4u,
                   kCovFailLds = 8u;

// s_getreg simm16 = id | offset << 6 | (size - 1) << 11; full 32 bits of each.
constexpr int kCovHwRegHwId = 4 | (31 << 11);
constexpr int kCovHwRegXccId = 20 | (31 << 11);

// Per-lane record of one operand set, already in MFMA fragment order (the
// layouts documented on the three smoke kernels above), packed by the host.
struct CovLaneRec {
  uint32_t f32_a, f32_b;        // A[l&15][l>>4], B[l>>4][l&15]
  uint32_t bf16_a[4], bf16_b[4];  // 8 bf16: A[l&15][(l>>4)*8+i], B[(l>>4)*8+i][l&15]
  uint32_t fp8_a[2], fp8_b[2];  // 8 e4m3, same geometry as bf16
  uint32_t exp[3][4];           // expected D[(l>>4)*4+r][l&15] bits per dtype
};
constexpr int kCovRecWords = sizeof(CovLaneRec) / sizeof(uint32_t);

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

// Integer operand generators: |v| <= 8, A and B unrelated (a transposed
// fragment cannot pass), every (set, dtype) pair a different pattern.
static int cov_a_val(int set, int dt, int m, int k) {
  return (m * 3 + k * 5 + set * 7 + dt * 2 + (m * k) % 5) % 17 - 8;
}
static int cov_b_val(int set, int dt, int k, int n) {
  return (k * 7 + n * 11 + set * 13 + dt * 4 + 3 + (k * n) % 7) % 17 - 8;
}

static uint16_t cov_to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return (uint16_t)((u + 0x7FFF + ((u >> 16) & 1)) >> 16);
}
static float cov_from_bf16(uint16_t v) {
  uint32_t u = (uint32_t)v << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static uint32_t cov_f32_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// One (set, dtype) problem: encoded operands, their decoded f32 values and
// the expected tile, which is computed in integers from the intended values
// (not from the decoded ones, so an encoding that fails to round-trip shows).
struct CovProblem {
  int k;
  std::vector<uint32_t> a_enc, b_enc;  // f32 bits / bf16 / e4m3 code per element
  std::vector<float> a_dec, b_dec, d;  // row-major 16xK, Kx16, 16x16
};

static const char* const kCovDtypeNames[3] = {"f32", "bf16", "fp8"};

static CovProblem cov_problem(int set, int dt) {
  CovProblem p;
  p.k = dt == 0 ? 4 : 32;
  const int K = p.k;
  std::vector<int> a(16 * K), b(K * 16);
  for (int m = 0; m < 16; ++m)
    for (int k = 0; k < K; ++k) a[m * K + k] = cov_a_val(set, dt, m, k);
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < 16; ++n) b[k * 16 + n] = cov_b_val(set, dt, k, n);
  auto encode = [dt](int v, uint32_t* enc, float* dec) {
    const float f = (float)v;
    if (dt == 0) {
      *enc = cov_f32_bits(f);
      *dec = f;
    } else if (dt == 1) {
      const uint16_t h = cov_to_bf16(f);
      *enc = h;
      *dec = cov_from_bf16(h);
    } else {
      const uint8_t q = encode_e4m3fn_nearest(f);
      *enc = q;
      *dec = decode_e4m3fn(q);
    }
  };
  p.a_enc.resize(16 * K);
  p.a_dec.resize(16 * K);
  p.b_enc.resize(K * 16);
  p.b_dec.resize(K * 16);
  for (int i = 0; i < 16 * K; ++i) encode(a[i], &p.a_enc[i], &p.a_dec[i]);
  for (int i = 0; i < K * 16; ++i) encode(b[i], &p.b_enc[i], &p.b_dec[i]);
  p.d.resize(256);
  for (int m = 0; m < 16; ++m)
    for (int n = 0; n < 16; ++n) {
      int acc = 0;
      for (int k = 0; k < K; ++k) acc += a[m * K + k] * b[k * 16 + n];
      p.d[m * 16 + n] = (float)acc;
    }
  return p;
}

// Pack every set into per-lane fragment records for the kernel.
static std::vector<uint32_t> cov_build_table() {
  std::vector<uint32_t> tab((size_t)kCovSets * 64 * kCovRecWords, 0u);
  for (int s = 0; s < kCovSets; ++s) {
    CovProblem pr[3] = {cov_problem(s, 0), cov_problem(s, 1), cov_problem(s, 2)};
    for (int l = 0; l < 64; ++l) {
      CovLaneRec rec;
      std::memset(&rec, 0, sizeof(rec));
      const int lo = l & 15, hi = l >> 4;
      rec.f32_a = pr[0].a_enc[lo * 4 + hi];
      rec.f32_b = pr[0].b_enc[hi * 16 + lo];
      for (int i = 0; i < 8; ++i) {
        const int k = hi * 8 + i;
        rec.bf16_a[i / 2] |= pr[1].a_enc[lo * 32 + k] << (16 * (i & 1));
        rec.bf16_b[i / 2] |= pr[1].b_enc[k * 16 + lo] << (16 * (i & 1));
        rec.fp8_a[i / 4] |= pr[2].a_enc[lo * 32 + k] << (8 * (i & 3));
        rec.fp8_b[i / 4] |= pr[2].b_enc[k * 16 + lo] << (8 * (i & 3));
      }
      for (int t = 0; t < 3; ++t)
        for (int r = 0; r < 4; ++r)
          rec.exp[t][r] = cov_f32_bits(pr[t].d[(hi * 4 + r) * 16 + lo]);
      std::memcpy(&tab[(size_t)(s * 64 + l) * kCovRecWords], &rec, sizeof(rec));
    }
  }
  return tab;
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

// RAII holders local to the sweep: nothing leaks when HIP_CHECK throws.
struct CovDeviceBuf {
  void* ptr = nullptr;
  CovDeviceBuf() = default;
  CovDeviceBuf(const CovDeviceBuf&) = delete;
  CovDeviceBuf& operator=(const CovDeviceBuf&) = delete;
  ~CovDeviceBuf() {
    if (ptr) (void)hipFree(ptr);
  }
  void alloc(size_t bytes) { HIP_CHECK(hipMalloc(&ptr, bytes)); }
  uint32_t* u32() const { return static_cast<uint32_t*>(ptr); }
};

struct CovEvent {
  hipEvent_t ev = nullptr;
  CovEvent() = default;
  CovEvent(const CovEvent&) = delete;
  CovEvent& operator=(const CovEvent&) = delete;
  ~CovEvent() {
    if (ev) (void)hipEventDestroy(ev);
  }
  void create() { HIP_CHECK(hipEventCreate(&ev)); }
};

// The host side of a whole-device sweep, shared by cu_coverage_check and
// mx_coverage_check: argument validation before the first HIP call, table
// upload, bounded relaunch until every CU and SIMD has been seen, and the
// per-slot result table.  `launch(cus, tab, slots)` enqueues one round of the
// sweep's kernel on a grid of kCovBlocksPerCu x CUs workgroups.
template <typename Launch>
static py::dict cov_run_sweep(const std::string& who, int device, int reps,
                              int max_rounds, int poison_key,
                              unsigned poison_mask, int mask_bits,
                              const std::vector<uint32_t>& tab, Launch launch) {
  if (reps < 1 || reps > 4096)
    throw std::invalid_argument(who + ": reps must be in [1, 4096]");
  if (max_rounds < 1 || max_rounds > 64)
    throw std::invalid_argument(who + ": max_rounds must be in [1, 64]");
  if (poison_key < -1 || poison_key >= kCovKeys)
    throw std::invalid_argument(who + ": poison_key out of range");
  if (poison_mask >= (1u << mask_bits))
    throw std::invalid_argument(who + ": poison_mask has " +
                                std::to_string(mask_bits) + " bits");

  hipDeviceProp_t prop;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  const int cus = prop.multiProcessorCount;
  if (cus < 1 || cus > kCovKeys)
    throw std::runtime_error(who + ": implausible compute unit count");
  if (prop.sharedMemPerBlock < sizeof(uint32_t) * kCovLdsWords)
    throw std::runtime_error(
        who + ": device grants less than 64 KiB of LDS per workgroup");

  const size_t slot_bytes = sizeof(uint32_t) * kCovSlots;
  CovDeviceBuf d_tab, d_slots;  // d_slots: waves | fail | hw_id | xcc_id
  d_tab.alloc(sizeof(uint32_t) * tab.size());
  d_slots.alloc(4 * slot_bytes);
  HIP_CHECK(hipMemcpy(d_tab.ptr, tab.data(), sizeof(uint32_t) * tab.size(),
                      hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(d_slots.ptr, 0, 4 * slot_bytes));
  CovEvent t0, t1;
  t0.create();
  t1.create();

  std::vector<uint32_t> h((size_t)4 * kCovSlots);
  const uint32_t* h_waves = h.data();
  const uint32_t* h_fail = h.data() + kCovSlots;
  const uint32_t* h_hw = h.data() + 2 * kCovSlots;
  const uint32_t* h_xcc = h.data() + 3 * kCovSlots;
  int rounds = 0, cus_covered = 0, slots_covered = 0;
  double elapsed_ms = 0.0;
  while (rounds < max_rounds) {
    HIP_CHECK(hipEventRecord(t0.ev));
    launch(cus, d_tab.u32(), d_slots.u32());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(t1.ev));
    HIP_CHECK(hipEventSynchronize(t1.ev));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, t0.ev, t1.ev));
    elapsed_ms += ms;
    ++rounds;
    HIP_CHECK(hipMemcpy(h.data(), d_slots.ptr, 4 * slot_bytes,
                        hipMemcpyDeviceToHost));
    cus_covered = slots_covered = 0;
    for (int key = 0; key < kCovKeys; ++key) {
      int simds = 0;
      for (int s = 0; s < 4; ++s) simds += h_waves[key * 4 + s] != 0;
      cus_covered += simds != 0;
      slots_covered += simds;
    }
    if (cus_covered >= cus && slots_covered >= 4 * cus) break;
  }

  py::list units;
  long waves_run = 0;
  int failed_slots = 0;
  for (int slot = 0; slot < kCovSlots; ++slot) {
    if (h_waves[slot] == 0) continue;
    const int key = slot >> 2;
    py::dict u;
    u["key"] = key;
    u["xcc"] = key >> 8;
    u["hw_bits"] = key & 0xFF;
    u["simd"] = slot & 3;
    u["waves"] = h_waves[slot];
    u["fail_mask"] = h_fail[slot];
    u["hw_id_raw"] = h_hw[slot];
    u["xcc_id_raw"] = h_xcc[slot];
    units.append(u);
    waves_run += h_waves[slot];
    failed_slots += h_fail[slot] != 0;
  }
  py::dict out;
  out["compute_units"] = cus;
  out["cus_covered"] = cus_covered;
  out["simd_slots_covered"] = slots_covered;
  out["waves_run"] = waves_run;
  out["rounds"] = rounds;
  out["failed_slots"] = failed_slots;
  out["units"] = units;
  out["elapsed_ms"] = elapsed_ms;
  return out;
}

static py::dict cu_coverage_check(int device, int reps, int max_rounds,
                                  int poison_key, unsigned poison_mask,
                                  bool poison_all) {
  return cov_run_sweep(
      "cu_coverage_check", device, reps, max_rounds, poison_key, poison_mask, 4,
      cov_build_table(), [&](int cus, uint32_t* tab, uint32_t* slots) {
        hipLaunchKernelGGL(cu_coverage_kernel, dim3(kCovBlocksPerCu * cus),
                           dim3(kCovBlock), 0, 0, tab, slots, slots + kCovSlots,
                           slots + 2 * kCovSlots, slots + 3 * kCovSlots, reps,
                           poison_key, poison_mask, poison_all ? 1 : 0);
      });
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

constexpr int kMxFormats = 5;
constexpr int kMxSets = 5;
constexpr int kMxSpanBoundLog2 = 20;

struct MxFormat {
  const char* name;
  int bits, ebits, mbits, bias;
  int unit;      // alphabet values are mags[i] * 2^unit
  int n_mags;
  int mags[16];  // both signs of each are used
  bool zero;     // plus zero
};

// Alphabets: both signs, every mantissa bit pattern, at least three exponent
// values, magnitudes small enough for the span bound.  e2m1: all 15 values.
static const MxFormat kMxFmt[kMxFormats] = {
    {"e4m3", 8, 4, 3, 7, -3, 13, {1, 2, 3, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16}, false},
    {"e5m2", 8, 5, 2, 15, -2, 11, {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14}, false},
    {"e2m3", 6, 2, 3, 1, -3, 16,
     {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, false},
    {"e3m2", 6, 3, 2, 3, -4, 12, {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16}, false},
    {"e2m1", 4, 2, 1, 1, -1, 7, {1, 2, 3, 4, 6, 8, 12}, true},
};

// A code as (-1)^sign * mant * 2^exp; NaN / Inf codes are not finite.
struct MxParts {
  bool finite;
  int sign, mant, exp;
};

static MxParts mx_decode_parts(int fmt, unsigned code) {
  const MxFormat& f = kMxFmt[fmt];
  const int e = (code >> f.mbits) & ((1 << f.ebits) - 1);
  const int m = code & ((1 << f.mbits) - 1);
  MxParts p{true, (int)((code >> (f.bits - 1)) & 1u), 0, 0};
  if (fmt == 0 && e == 15 && m == 7) p.finite = false;  // e4m3 NaN
  if (fmt == 1 && e == 31) p.finite = false;            // e5m2 Inf / NaN
  if (e == 0) {
    p.mant = m;  // subnormal
    p.exp = 1 - f.bias - f.mbits;
  } else {
    p.mant = (1 << f.mbits) + m;
    p.exp = e - f.bias - f.mbits;
  }
  return p;
}

static double mx_decode(int fmt, unsigned code) {
  const MxParts p = mx_decode_parts(fmt, code);
  const double v = std::ldexp((double)p.mant, p.exp);
  return p.sign ? -v : v;
}

// Exact encoder of n * 2^unit: throws when no finite code has that value.
static uint8_t mx_encode_exact(int fmt, int n, int unit) {
  if (n == 0) return 0;
  const int mag = n < 0 ? -n : n;
  for (unsigned code = 0; code < (1u << kMxFmt[fmt].bits); ++code) {
    const MxParts p = mx_decode_parts(fmt, code);
    if (!p.finite || p.mant == 0 || p.sign != (n < 0)) continue;
    const int d = p.exp - unit;
    if (d >= 0 ? (d < 24 && (p.mant << d) == mag)
               : (-d < 24 && (mag << -d) == p.mant))
      return (uint8_t)code;
  }
  throw std::domain_error(std::string("mx_encode_exact: ") + kMxFmt[fmt].name +
                          " cannot represent " + std::to_string(n) + " * 2^" +
                          std::to_string(unit));
}

// E8M0: 2^(code - 127); 0xFF is NaN and never produced.
static uint8_t mx_encode_e8m0(int exp) {
  if (exp < -127 || exp > 127)
    throw std::domain_error("mx_encode_e8m0: 2^" + std::to_string(exp) +
                            " has no E8M0 code");
  return (uint8_t)(exp + 127);
}
static double mx_decode_e8m0(uint8_t code) {
  return std::ldexp(1.0, (int)code - 127);
}

// op_sel byte of the scale VGPR, per set: A and B use different bytes
constexpr int mx_sel_a(int set) { return set & 3; }
constexpr int mx_sel_b(int set) { return set == 0 ? 0 : 1 + (set % 3); }
// scale exponents per set are base + one of three offsets: set 0 uniform, 1
// and 2 near one, 3 far apart, 4 a wider spread that takes S/q near the bound
static const int kMxScaleBaseA[kMxSets] = {0, -1, 2, 20, -2};
static const int kMxScaleBaseB[kMxSets] = {0, 0, -3, -21, -1};
static const int kMxScaleSpread[kMxSets][3] = {
    {0, 0, 0}, {0, 1, 2}, {0, 1, 2}, {0, 1, 2}, {0, 1, 3}};

struct MxProblem {
  int set, fa, fb, shape;  // shape 0: 16x16x128, 1: 32x32x64
  int m, n, k, kblocks, sel_a, sel_b;
  std::vector<uint8_t> a_codes, b_codes;    // row-major m x k, k x n
  std::vector<uint8_t> a_scales, b_scales;  // row-major m x kblocks, kblocks x n
  std::vector<float> d;                     // expected, row-major m x n
  double log2_span;                         // achieved log2(S / q)
  std::vector<uint32_t> a_words, b_words;   // 64 lanes x 8 operand words
  std::vector<uint32_t> a_scale_words, b_scale_words;  // 64 lanes
};

static const char* mx_shape_name(int shape) {
  return shape == 0 ? "16x16x128" : "32x32x64";
}

// K index of element j of a lane in lane group g (see the layout above)
static int mx_lane_k(int bits, int K, int g, int j) {
  return bits == 8 ? (K / 2) * (j >> 4) + 16 * g + (j & 15) : 32 * g + j;
}

// One lane's 32 elements of row / col `codes` (K elements, `stride` apart):
// element j at bits [w*j, w*j + w) of 8 words
static void mx_pack_lane(int bits, int K, int g, const uint8_t* codes,
                         size_t stride, uint32_t* words) {
  for (int i = 0; i < 8; ++i) words[i] = 0;
  for (int j = 0; j < 32; ++j) {
    const uint32_t c = codes[mx_lane_k(bits, K, g, j) * stride];
    const int pos = j * bits, w = pos >> 5, off = pos & 31;
    words[w] |= c << off;
    if (off + bits > 32) words[w + 1] |= c >> (32 - off);
  }
}

static int mx_ctz(int64_t v) {
  int z = 0;
  while ((v & 1) == 0) {
    v >>= 1;
    ++z;
  }
  return z;
}

static MxProblem mx_problem(int set, int fa, int fb, int shape) {
  if (set < 0 || set >= kMxSets)
    throw std::invalid_argument("mx_problem: set out of range");
  if (fa < 0 || fa >= kMxFormats || fb < 0 || fb >= kMxFormats)
    throw std::invalid_argument("mx_problem: unknown format");
  if (shape != 0 && shape != 1)
    throw std::invalid_argument("mx_problem: unknown shape");
  MxProblem p;
  p.set = set;
  p.fa = fa;
  p.fb = fb;
  p.shape = shape;
  p.m = p.n = shape == 0 ? 16 : 32;
  p.k = shape == 0 ? 128 : 64;
  p.kblocks = p.k / 32;
  p.sel_a = mx_sel_a(set);
  p.sel_b = mx_sel_b(set);
  const int M = p.m, N = p.n, K = p.k, KB = p.kblocks;

  auto alphabet = [](int fmt) {
    const MxFormat& f = kMxFmt[fmt];
    std::vector<int> v;
    for (int i = 0; i < f.n_mags; ++i) {
      v.push_back(f.mags[i]);
      v.push_back(-f.mags[i]);
    }
    if (f.zero) v.push_back(0);
    return v;
  };
  const std::vector<int> al_a = alphabet(fa), al_b = alphabet(fb);
  const int ua = kMxFmt[fa].unit, ub = kMxFmt[fb].unit;

  // intended values (integers in units of 2^ua, 2^ub) and scale exponents;
  // A and B are unrelated patterns and every (set, pair, shape) differs
  std::vector<int> a(M * K), b(K * N), sa(M * KB), sb(KB * N);
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < K; ++k)
      a[m * K + k] = al_a[(m * 3 + k * 5 + set * 7 + fa * 2 + fb * 3 +
                           shape * 11 + (m * k) % 5) % (int)al_a.size()];
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n)
      b[k * N + n] = al_b[(k * 7 + n * 11 + set * 13 + fb * 4 + fa * 5 +
                           shape * 3 + 3 + (k * n) % 7) % (int)al_b.size()];
  // neighbouring rows / cols and neighbouring kblocks get different scales
  // (set 0 is uniform: it checks the operand maps on their own)
  for (int m = 0; m < M; ++m)
    for (int kb = 0; kb < KB; ++kb)
      sa[m * KB + kb] =
          kMxScaleBaseA[set] + kMxScaleSpread[set][(m + 2 * kb + set) % 3];
  for (int kb = 0; kb < KB; ++kb)
    for (int n = 0; n < N; ++n)
      sb[kb * N + n] =
          kMxScaleBaseB[set] + kMxScaleSpread[set][(2 * n + kb + set + 1) % 3];

  // encode; an operand that does not round-trip throws
  p.a_codes.resize(M * K);
  p.b_codes.resize(K * N);
  p.a_scales.resize(M * KB);
  p.b_scales.resize(KB * N);
  for (int i = 0; i < M * K; ++i) {
    p.a_codes[i] = mx_encode_exact(fa, a[i], ua);
    if (mx_decode(fa, p.a_codes[i]) != std::ldexp((double)a[i], ua))
      throw std::domain_error("mx_problem: A operand does not round-trip");
  }
  for (int i = 0; i < K * N; ++i) {
    p.b_codes[i] = mx_encode_exact(fb, b[i], ub);
    if (mx_decode(fb, p.b_codes[i]) != std::ldexp((double)b[i], ub))
      throw std::domain_error("mx_problem: B operand does not round-trip");
  }
  for (int i = 0; i < M * KB; ++i) {
    p.a_scales[i] = mx_encode_e8m0(sa[i]);
    if (mx_decode_e8m0(p.a_scales[i]) != std::ldexp(1.0, sa[i]))
      throw std::domain_error("mx_problem: A scale does not round-trip");
  }
  for (int i = 0; i < KB * N; ++i) {
    p.b_scales[i] = mx_encode_e8m0(sb[i]);
    if (mx_decode_e8m0(p.b_scales[i]) != std::ldexp(1.0, sb[i]))
      throw std::domain_error("mx_problem: B scale does not round-trip");
  }

  // expected tile in 64-bit fixed point with unit 2^e_min, from the intended
  // integers and exponents (never from decoded floats)
  int e_min = INT32_MAX;
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n)
      for (int kb = 0; kb < KB; ++kb)
        e_min = std::min(e_min, ua + ub + sa[m * KB + kb] + sb[kb * N + n]);
  int q_exp = INT32_MAX;  // log2 of q
  int64_t s_max = 0;      // S in units of 2^e_min
  p.d.resize(M * N);
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) {
      int64_t acc = 0, abs_sum = 0;
      for (int k = 0; k < K; ++k) {
        const int64_t prod = (int64_t)a[m * K + k] * b[k * N + n];
        if (prod == 0) continue;
        const int e = ua + ub + sa[m * KB + k / 32] + sb[(k / 32) * N + n];
        if (e - e_min > 30) throw std::domain_error("mx_problem: scale spread");
        acc += prod * ((int64_t)1 << (e - e_min));
        abs_sum += (prod < 0 ? -prod : prod) * ((int64_t)1 << (e - e_min));
        q_exp = std::min(q_exp, e + mx_ctz(prod));
      }
      s_max = std::max(s_max, abs_sum);
      const double want = std::ldexp((double)acc, e_min);
      p.d[m * N + n] = (float)want;
      if ((double)p.d[m * N + n] != want)
        throw std::domain_error("mx_problem: expected value is not an f32");
    }
  if (s_max == 0) throw std::domain_error("mx_problem: empty tile");
  p.log2_span = std::log2((double)s_max) + (double)(e_min - q_exp);
  if (p.log2_span > (double)kMxSpanBoundLog2)
    throw std::domain_error(
        std::string("mx_problem: S/q = 2^") + std::to_string(p.log2_span) +
        " exceeds the exactness bound for " + kMxFmt[fa].name + " x " +
        kMxFmt[fb].name + " " + mx_shape_name(shape) + " set " +
        std::to_string(set));

  // per-lane fragments; the three scale bytes op_sel does not pick hold valid
  // scales that would give another answer
  p.a_words.resize(64 * 8);
  p.b_words.resize(64 * 8);
  p.a_scale_words.resize(64);
  p.b_scale_words.resize(64);
  for (int l = 0; l < 64; ++l) {
    const int rc = l % M, kb = l / M;
    mx_pack_lane(kMxFmt[fa].bits, K, kb, &p.a_codes[rc * K], 1,
                 &p.a_words[l * 8]);
    mx_pack_lane(kMxFmt[fb].bits, K, kb, &p.b_codes[rc], (size_t)N,
                 &p.b_words[l * 8]);
    const uint32_t ca = p.a_scales[rc * KB + kb], cb = p.b_scales[kb * N + rc];
    uint32_t wa = 0, wb = 0;
    for (int i = 0; i < 4; ++i) {
      wa |= (i == p.sel_a ? ca : ca + 3 + i) << (8 * i);
      wb |= (i == p.sel_b ? cb : cb + 3 + i) << (8 * i);
    }
    p.a_scale_words[l] = wa;
    p.b_scale_words[l] = wb;
  }
  return p;
}

// The sweep's problems per set: five same-format pairs and three mixed pairs
// (cbsz != blgp) on 16x16x128, then e2m1 and e4m3 on 32x32x64.
constexpr int kMxProbs = 10;
constexpr int kMxProbFa[kMxProbs] = {0, 1, 2, 3, 4, 0, 4, 3, 4, 0};
constexpr int kMxProbFb[kMxProbs] = {0, 1, 2, 3, 4, 4, 2, 1, 4, 0};
constexpr int kMxProbShape[kMxProbs] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1};
constexpr int kMxProbBit[kMxProbs] = {0, 1, 2, 3, 4, 5, 5, 5, 6, 6};
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
constexpr int kMxTileRecWords = 18;

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
  switch (set) {
    case 0:
      hipLaunchKernelGGL((mx_tile_kernel<SHAPE, 0>), dim3(1), dim3(64), 0, 0, rec, out, pair);
      break;
    case 1:
      hipLaunchKernelGGL((mx_tile_kernel<SHAPE, 1>), dim3(1), dim3(64), 0, 0, rec, out, pair);
      break;
    case 2:
      hipLaunchKernelGGL((mx_tile_kernel<SHAPE, 2>), dim3(1), dim3(64), 0, 0, rec, out, pair);
      break;
    case 3:
      hipLaunchKernelGGL((mx_tile_kernel<SHAPE, 3>), dim3(1), dim3(64), 0, 0, rec, out, pair);
      break;
    default:
      hipLaunchKernelGGL((mx_tile_kernel<SHAPE, 4>), dim3(1), dim3(64), 0, 0, rec, out, pair);
      break;
  }
}

static py::dict mx_mfma_tile(int device, const std::string& fmt_a,
                             const std::string& fmt_b, const std::string& shape,
                             int set) {
  // Run one scaled MFMA and return the raw problem + the GPU tile so Python
  // tests can verify against independent decoders.
  const int fa = mx_format_index(fmt_a), fb = mx_format_index(fmt_b);
  const int sh = mx_shape_index(shape);
  const MxProblem p = mx_problem(set, fa, fb, sh);  // validates set
  std::vector<uint32_t> rec((size_t)64 * kMxTileRecWords);
  for (int l = 0; l < 64; ++l) {
    uint32_t* r = &rec[(size_t)l * kMxTileRecWords];
    std::memcpy(r, &p.a_words[l * 8], 32);
    std::memcpy(r + 8, &p.b_words[l * 8], 32);
    r[16] = p.a_scale_words[l];
    r[17] = p.b_scale_words[l];
  }
  HIP_CHECK(hipSetDevice(device));
  CovDeviceBuf d_rec, d_out;
  d_rec.alloc(sizeof(uint32_t) * rec.size());
  d_out.alloc(sizeof(float) * 64 * 16);
  HIP_CHECK(hipMemcpy(d_rec.ptr, rec.data(), sizeof(uint32_t) * rec.size(),
                      hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(d_out.ptr, 0xFF, sizeof(float) * 64 * 16));
  if (sh == 0)
    mx_tile_launch<0>(set, d_rec.u32(), static_cast<float*>(d_out.ptr),
                      fa * kMxFormats + fb);
  else
    mx_tile_launch<1>(set, d_rec.u32(), static_cast<float*>(d_out.ptr),
                      fa * kMxFormats + fb);
  HIP_CHECK(hipGetLastError());
  std::vector<float> regs(64 * 16);
  HIP_CHECK(hipMemcpy(regs.data(), d_out.ptr, sizeof(float) * regs.size(),
                      hipMemcpyDeviceToHost));
  std::vector<float> d_gpu((size_t)p.m * p.n);
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < (sh == 0 ? 4 : 16); ++r) {
      const int row = sh == 0 ? (l >> 4) * 4 + r
                              : (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
      const int col = sh == 0 ? (l & 15) : (l & 31);
      d_gpu[row * p.n + col] = regs[l * 16 + r];
    }
  py::dict out = mx_problem_dict(p);
  out["d_gpu"] = d_gpu;  // GPU result, row-major m x n
  return out;
}

// Whole-device MX sweep, built like cu_coverage_kernel: same grid, launch
// bounds, 64 KiB LDS claim, placement key and slot scheme, fixed work per
// workgroup.  Per-lane record of one (set, problem): a[8] b[8] sa sb exp[16]
// (16x16 problems use exp[0..3]).
constexpr int kMxRecWords = 34;

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

static std::vector<uint32_t> mx_build_table() {
  std::vector<uint32_t> tab((size_t)kMxSets * kMxProbs * 64 * kMxRecWords, 0u);
  for (int s = 0; s < kMxSets; ++s)
    for (int i = 0; i < kMxProbs; ++i) {
      const MxProblem p =
          mx_problem(s, kMxProbFa[i], kMxProbFb[i], kMxProbShape[i]);
      for (int l = 0; l < 64; ++l) {
        uint32_t* r = &tab[(size_t)((s * kMxProbs + i) * 64 + l) * kMxRecWords];
        std::memcpy(r, &p.a_words[l * 8], 32);
        std::memcpy(r + 8, &p.b_words[l * 8], 32);
        r[16] = p.a_scale_words[l];
        r[17] = p.b_scale_words[l];
        for (int q = 0; q < (p.shape == 0 ? 4 : 16); ++q) {
          const int row = p.shape == 0 ? (l >> 4) * 4 + q
                                       : (q & 3) + 8 * (q >> 2) + 4 * (l >> 5);
          const int col = p.shape == 0 ? (l & 15) : (l & 31);
          r[18 + q] = cov_f32_bits(p.d[row * p.n + col]);
        }
      }
    }
  return tab;
}

static py::dict mx_coverage_check(int device, int reps, int max_rounds,
                                  int poison_key, unsigned poison_mask,
                                  bool poison_all) {
  return cov_run_sweep(
      "mx_coverage_check", device, reps, max_rounds, poison_key, poison_mask,
      kMxFailBits, mx_build_table(),
      [&](int cus, uint32_t* tab, uint32_t* slots) {
        hipLaunchKernelGGL(mx_coverage_kernel, dim3(kCovBlocksPerCu * cus),
                           dim3(kCovBlock), 0, 0, tab, slots, slots + kCovSlots,
                           slots + 2 * kCovSlots, slots + 3 * kCovSlots, reps,
                           poison_key, poison_mask, poison_all ? 1 : 0);
      });
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
  // 64 lanes x {a[8], b[8]} of non-zero alphabet codes, then the scale word
  const MxFormat& mf = kMxFmt[f];
  std::vector<uint32_t> hseed(64 * 16 + 1);
  for (int l = 0; l < 64; ++l)
    for (int h = 0; h < 2; ++h) {
      uint8_t codes[128];  // one row: only the lane's own 32 are read
      for (int j = 0; j < 128; ++j) {
        const int mag = mf.mags[(l * 7 + j * 3 + h * 5) % mf.n_mags];
        codes[j] = mx_encode_exact(f, (l + j + h) % 3 == 0 ? -mag : mag, mf.unit);
      }
      mx_pack_lane(mf.bits, 128, l >> 4, codes, 1, &hseed[l * 16 + h * 8]);
    }
  hseed[64 * 16] = 0x01010101u * mx_encode_e8m0(-20);
  const int block = 256, grid = 512;  // 2048 waves = 2 per SIMD, 4 chains each
  HIP_CHECK(hipSetDevice(device));
  CovDeviceBuf d_seed, d_out;
  d_seed.alloc(sizeof(uint32_t) * hseed.size());
  d_out.alloc(sizeof(float) * block * grid);
  HIP_CHECK(hipMemcpy(d_seed.ptr, hseed.data(), sizeof(uint32_t) * hseed.size(),
                      hipMemcpyHostToDevice));
  auto launch = [&](int n) {
    if (f == 4)
      hipLaunchKernelGGL(mx_burn_kernel<4>, dim3(grid), dim3(block), 0, 0,
                         d_seed.u32(), static_cast<float*>(d_out.ptr), n);
    else
      hipLaunchKernelGGL(mx_burn_kernel<0>, dim3(grid), dim3(block), 0, 0,
                         d_seed.u32(), static_cast<float*>(d_out.ptr), n);
  };
  launch(1000);  // warmup
  HIP_CHECK(hipDeviceSynchronize());
  CovEvent t0, t1;
  t0.create();
  t1.create();
  HIP_CHECK(hipEventRecord(t0.ev));
  launch(iters);
  HIP_CHECK(hipEventRecord(t1.ev));
  HIP_CHECK(hipEventSynchronize(t1.ev));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0.ev, t1.ev));
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

constexpr int kHbmPatternHash = 0, kHbmPatternChecker = 1;
constexpr int kHbmFill = 0, kHbmVerifyInvert = 1, kHbmVerify = 2;
constexpr int kHbmBlock = 512;            // bw_copy_kernel's sweep-tuned shape
constexpr int kHbmShards = 1024;          // compared-word counters, one line each
constexpr int kHbmShardStride = 16;       // in uint64: 128 bytes apart
constexpr int kHbmMaxRecords = 4096;
constexpr int kHbmMaxPasses = 16;
constexpr size_t kHbmReferenceMax = 65536;
constexpr uint64_t kHbmReserveBytes = 2ull << 30;
constexpr uint64_t kHbmBeyondCacheBytes = 512ull << 20;  // 2 x Infinity Cache

// The one definition shared by the kernels and the host reference.
__host__ __device__ inline uint64_t hbm_pattern_value(int pattern, uint64_t seed,
                                                      uint64_t i) {
  if (pattern == kHbmPatternChecker)
    return (i & 1ull) ? 0x5555555555555555ull : 0xAAAAAAAAAAAAAAAAull;
  uint64_t z = i + seed * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

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
  const unsigned long long slot = atomicAdd(&a.ctl[kHbmCtlClaims], 1ull);
  if (slot < a.max_records) {  // claims past the cap are dropped
    HbmRecord r = {i, a.verify_index, got ^ x, got};
    a.records[slot] = r;
  }
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

// RAII holders in the style of CovDeviceBuf / CovEvent.
struct HbmDeviceBuf {
  void* ptr = nullptr;
  HbmDeviceBuf() = default;
  HbmDeviceBuf(const HbmDeviceBuf&) = delete;
  HbmDeviceBuf& operator=(const HbmDeviceBuf&) = delete;
  HbmDeviceBuf(HbmDeviceBuf&& o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
  ~HbmDeviceBuf() {
    if (ptr) (void)hipFree(ptr);
  }
  void alloc(size_t bytes) { HIP_CHECK(hipMalloc(&ptr, bytes)); }
};

struct HbmChunk {
  HbmDeviceBuf buf;
  uint64_t first_word = 0;  // logical
  uint64_t words = 0;
};

static void hbm_launch(int kind, const HbmLaunch& a) {
  // bw_copy_kernel's launch shape: ~2 vectors per thread, grid in [1024, 131072]
  const uint64_t nvec = a.nwords >> 1;
  const long want = (long)(nvec / (2 * (uint64_t)kHbmBlock)) + 1;
  const int grid = (int)std::min<long>(131072, std::max<long>(1024, want));
  if (kind == kHbmFill)
    hipLaunchKernelGGL(hbm_pattern_kernel<kHbmFill>, dim3(grid), dim3(kHbmBlock),
                       0, 0, a);
  else if (kind == kHbmVerifyInvert)
    hipLaunchKernelGGL(hbm_pattern_kernel<kHbmVerifyInvert>, dim3(grid),
                       dim3(kHbmBlock), 0, 0, a);
  else
    hipLaunchKernelGGL(hbm_pattern_kernel<kHbmVerify>, dim3(grid),
                       dim3(kHbmBlock), 0, 0, a);
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
  if (passes < 1 || passes > kHbmMaxPasses)
    throw std::invalid_argument("hbm_pattern_check: passes must be in [1, 16]");
  if (max_records < 1 || max_records > kHbmMaxRecords)
    throw std::invalid_argument("hbm_pattern_check: max_records must be in [1, 4096]");
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
    c.buf.alloc((size_t)(c.words * 8));
  }

  HbmDeviceBuf d_ctl, d_shards, d_records;
  const size_t shard_bytes = sizeof(uint64_t) * kHbmShards * kHbmShardStride;
  d_ctl.alloc(sizeof(uint64_t) * kHbmCtlWords);
  d_shards.alloc(shard_bytes);
  d_records.alloc(sizeof(HbmRecord) * (size_t)max_records);
  HIP_CHECK(hipMemset(d_ctl.ptr, 0, sizeof(uint64_t) * kHbmCtlWords));
  HIP_CHECK(hipMemset(d_shards.ptr, 0, shard_bytes));
  HIP_CHECK(hipMemset(d_records.ptr, 0, sizeof(HbmRecord) * (size_t)max_records));
  CovEvent t0, t1;
  t0.create();
  t1.create();

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
      HIP_CHECK(hipEventRecord(t0.ev));
      for (const HbmChunk& c : chunks) {
        HbmLaunch a;
        a.buf = static_cast<uint64_t*>(c.buf.ptr);
        a.nwords = c.words;
        a.base = c.first_word;
        a.seed = pseed;
        a.poison_xor = poison_xor;
        a.poison_stride = poison_stride;
        a.poison_word = poisoned ? poison_word : -1;
        a.ctl = static_cast<unsigned long long*>(d_ctl.ptr);
        a.shards = static_cast<unsigned long long*>(d_shards.ptr);
        a.records = static_cast<HbmRecord*>(d_records.ptr);
        a.max_records = (uint32_t)max_records;
        a.verify_index = (uint32_t)verify_index;
        a.pattern = is_hash ? kHbmPatternHash : kHbmPatternChecker;
        hbm_launch(kind, a);
      }
      HIP_CHECK(hipEventRecord(t1.ev));
      HIP_CHECK(hipEventSynchronize(t1.ev));
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, t0.ev, t1.ev));
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

  uint64_t ctl[kHbmCtlWords];
  std::vector<uint64_t> shards((size_t)kHbmShards * kHbmShardStride);
  HIP_CHECK(hipMemcpy(ctl, d_ctl.ptr, sizeof(ctl), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(shards.data(), d_shards.ptr, shard_bytes,
                      hipMemcpyDeviceToHost));
  const uint64_t claims = ctl[kHbmCtlClaims];
  const size_t kept = (size_t)std::min<uint64_t>(claims, (uint64_t)max_records);
  std::vector<HbmRecord> recs(kept);
  if (kept)
    HIP_CHECK(hipMemcpy(recs.data(), d_records.ptr, sizeof(HbmRecord) * kept,
                        hipMemcpyDeviceToHost));
  uint64_t words_verified = 0;
  for (int s = 0; s < kHbmShards; ++s)
    words_verified += shards[(size_t)s * kHbmShardStride];

  py::list chunk_list;
  for (size_t c = 0; c < chunks.size(); ++c) {
    py::dict e;
    e["index"] = c;
    e["first_word"] = chunks[c].first_word;
    e["bytes"] = chunks[c].words * 8;
    chunk_list.append(e);
  }
  py::list records;
  for (const HbmRecord& r : recs) {
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
  out["error_count"] = ctl[kHbmCtlErrors];
  out["xor_or"] = ctl[kHbmCtlXor];
  out["records"] = records;
  out["records_dropped"] = claims - (uint64_t)kept;
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
constexpr uint64_t kXfStaticKey = 0x5354415449435F58ull;
constexpr uint64_t kXfAtomKey1 = 0x41544F4D31ull, kXfAtomKey2 = 0x41544F4D32ull,
                   kXfAtomKey3 = 0x41544F4D33ull;
constexpr int64_t kXfF32Bound = 1ll << 23;
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

__host__ __device__ inline uint64_t xf_static_word(uint64_t seed, uint64_t idx) {
  return hbm_pattern_value(kHbmPatternHash, seed ^ kXfStaticKey, idx);
}
// round -1 is the initial upload
__host__ __device__ inline uint64_t xf_payload_word(uint64_t seed, int64_t round,
                                                    uint64_t idx) {
  return hbm_pattern_value(kHbmPatternHash, seed + (uint64_t)round, idx);
}
__host__ __device__ inline uint64_t xf_line_index(uint32_t blocks,
                                                  uint32_t slab_lines,
                                                  uint32_t rep, uint32_t block,
                                                  uint32_t line) {
  return ((uint64_t)rep * blocks + block) * slab_lines + line;
}

// the rare path: claim a record slot, as hbm_report does
__device__ __forceinline__ void xf_report(const XfHandoff& a, uint32_t rep,
                                          uint32_t group, uint32_t member,
                                          uint32_t line, uint32_t word,
                                          uint32_t wx, uint32_t rx, uint32_t kind,
                                          uint32_t extra, uint64_t expected,
                                          uint64_t got) {
  const unsigned long long slot = atomicAdd(&a.ctl[kXfCtlClaims], 1ull);
  if (slot < a.max_records) {  // claims past the cap are dropped
    XfRecord r = {a.round, rep, group, member, line, word, wx, rx, kind, extra,
                  expected, got};
    a.records[slot] = r;
  }
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

struct XfAtomVals {
  uint64_t add64, mm;
  uint32_t add32, x, o, a;
  int addf;  // integer in [-8, 8], added as f32
};

// The one generator shared by the kernel and the host: what thread `id` adds
// in repetition `rep`.  or/and operands are mostly neutral so the cells do
// not saturate.
__host__ __device__ inline XfAtomVals xf_atom_vals(uint64_t seed, uint64_t id,
                                                   uint32_t rep) {
  const uint64_t n = id * 64 + rep;
  const uint64_t h1 = hbm_pattern_value(kHbmPatternHash, seed ^ kXfAtomKey1, n);
  const uint64_t h2 = hbm_pattern_value(kHbmPatternHash, seed ^ kXfAtomKey2, n);
  const uint64_t h3 = hbm_pattern_value(kHbmPatternHash, seed ^ kXfAtomKey3, n);
  XfAtomVals v;
  v.add32 = (uint32_t)h1;
  v.addf = (int)((h1 >> 32) % 17) - 8;
  v.add64 = h2;
  v.mm = h3;
  v.x = (uint32_t)(h1 >> 20);
  v.o = ((h2 >> 40) & 1023) == 0 ? 1u << ((h2 >> 8) & 31) : 0u;
  v.a = ((h2 >> 50) & 1023) == 0 ? ~(1u << ((h2 >> 16) & 31)) : ~0u;
  return v;
}

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

// Expected cell contents after `threads` threads ran `reps` repetitions.
struct XfAtomExpected {
  std::vector<uint32_t> add32, x, o, a;
  std::vector<uint64_t> add64, max64, min64;
  std::vector<int64_t> addf;
};

static XfAtomExpected xf_atom_expected(uint64_t seed, uint64_t threads, int reps,
                                       int cells) {
  XfAtomExpected e;
  e.add32.assign(cells, 0u);
  e.x.assign(cells, 0u);
  e.o.assign(cells, 0u);
  e.a.assign(cells, ~0u);
  e.add64.assign(cells, 0ull);
  e.max64.assign(cells, 0ull);
  e.min64.assign(cells, ~0ull);
  e.addf.assign(cells, 0);
  std::vector<int64_t> mag(cells, 0);
  for (uint64_t id = 0; id < threads; ++id)
    for (int rep = 0; rep < reps; ++rep) {
      const size_t c = (size_t)((id + (uint64_t)rep) % (uint64_t)cells);
      const XfAtomVals v = xf_atom_vals(seed, id, (uint32_t)rep);
      e.add32[c] += v.add32;
      e.add64[c] += v.add64;
      e.addf[c] += v.addf;
      mag[c] += v.addf < 0 ? -v.addf : v.addf;
      e.max64[c] = std::max(e.max64[c], v.mm);
      e.min64[c] = std::min(e.min64[c], v.mm);
      e.x[c] ^= v.x;
      e.o[c] |= v.o;
      e.a[c] &= v.a;
    }
  // enforced, not assumed: below 2^23 every partial sum is an exact f32
  for (int c = 0; c < cells; ++c)
    if (mag[c] > kXfF32Bound)
      throw std::invalid_argument(
          "xcd_fabric: the f32 operands of cell " + std::to_string(c) +
          " sum to a magnitude of " + std::to_string(mag[c]) +
          " > 2^23; use more cells or fewer reps");
  return e;
}

struct XfShape {
  int reps, group, slab_lines, cells, blocks, max_rounds, max_records;
  unsigned poison_mask;
  int poison_pair;
};

// every argument is validated here, before the first HIP call
static void xf_validate(const std::string& who, const XfShape& s) {
  if (s.reps < 1 || s.reps > 64)
    throw std::invalid_argument(who + ": reps must be in [1, 64]");
  if (s.group < 2 || s.group > 64)
    throw std::invalid_argument(who + ": group must be in [2, 64]");
  if (s.slab_lines < 1 || s.slab_lines > 32)
    throw std::invalid_argument(who + ": slab_lines must be in [1, 32]");
  if (s.cells < 1 || s.cells > 4096)
    throw std::invalid_argument(who + ": cells must be in [1, 4096]");
  if (s.blocks < 0 || s.blocks > kXfMaxBlocks ||
      (s.blocks > 0 && s.blocks % s.group != 0))
    throw std::invalid_argument(
        who + ": blocks must be 0 (derive from the device) or a positive "
              "multiple of group, at most 1024");
  if (s.max_rounds < 2 || s.max_rounds > 64)
    throw std::invalid_argument(who + ": max_rounds must be in [2, 64]");
  if (s.max_records < 1 || s.max_records > kXfMaxRecords)
    throw std::invalid_argument(who + ": max_records must be in [1, 4096]");
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
  if (round < -1 || round >= 64)
    throw std::invalid_argument("xcd_fabric_reference: round must be in [-1, 63]");
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

static uint32_t xf_f32_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof(u));
  return u;
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
  HbmDeviceBuf d_cells, d_ticket, d_seen, d_adders, d_ctl;
  d_cells.alloc(sizeof(XfCell) * cells.size());
  d_ticket.alloc(128);
  d_seen.alloc(sizeof(uint32_t) * total);
  d_adders.alloc(sizeof(uint32_t) * kXfXccs);
  d_ctl.alloc(sizeof(uint64_t) * kXfActlWords);
  HIP_CHECK(hipMemcpy(d_cells.ptr, cells.data(), sizeof(XfCell) * cells.size(),
                      hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(d_ticket.ptr, 0, 128));
  HIP_CHECK(hipMemset(d_seen.ptr, 0, sizeof(uint32_t) * total));
  HIP_CHECK(hipMemset(d_adders.ptr, 0, sizeof(uint32_t) * kXfXccs));
  HIP_CHECK(hipMemset(d_ctl.ptr, 0, sizeof(uint64_t) * kXfActlWords));
  CovEvent t0, t1;
  t0.create();
  t1.create();

  XfAtomics a;
  a.cells = static_cast<XfCell*>(d_cells.ptr);
  a.ticket = static_cast<uint32_t*>(d_ticket.ptr);
  a.seen = static_cast<uint32_t*>(d_seen.ptr);
  a.adders = static_cast<uint32_t*>(d_adders.ptr);
  a.ctl = static_cast<unsigned long long*>(d_ctl.ptr);
  a.seed = seed;
  a.reps = (uint32_t)s.reps;
  a.ncells = (uint32_t)s.cells;
  a.total = total;
  HIP_CHECK(hipEventRecord(t0.ev));
  hipLaunchKernelGGL(xcd_atomics_kernel, dim3(grid), dim3(kXfBlock), 0, 0, a);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1.ev));
  HIP_CHECK(hipEventSynchronize(t1.ev));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0.ev, t1.ev));
  elapsed_ms += ms;

  std::vector<uint32_t> seen(total), adders(kXfXccs);
  uint32_t counter = 0;
  uint64_t ctl[kXfActlWords];
  HIP_CHECK(hipMemcpy(cells.data(), d_cells.ptr, sizeof(XfCell) * cells.size(),
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(seen.data(), d_seen.ptr, sizeof(uint32_t) * total,
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(adders.data(), d_adders.ptr, sizeof(uint32_t) * kXfXccs,
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(&counter, d_ticket.ptr, sizeof(counter),
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(ctl, d_ctl.ptr, sizeof(ctl), hipMemcpyDeviceToHost));

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
    const uint32_t wf = xf_f32_bits((float)e.addf[c]) ^ px(kXfPoisonAddF32);
    if (xf_f32_bits(k.addf) != wf) {
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

  hipDeviceProp_t prop;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  const int cus = prop.multiProcessorCount;
  if (cus < 1 || cus > kCovKeys)
    throw std::runtime_error("xcd_fabric_check: implausible compute unit count");
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
  const size_t ticket_bytes = n_tickets * kXfTicketStride * sizeof(uint32_t);
  const size_t writer_count = (size_t)reps * nblocks;
  constexpr size_t kPlane = (size_t)kXfXccs * kXfXccs;
  const size_t pair_bytes = sizeof(uint64_t) * kXfPairPlanes * kPlane;

  // the initial upload plays round -1
  std::vector<uint64_t> h_slab(slab_words);
  for (size_t i = 0; i < slab_words; ++i)
    h_slab[i] = (i % kXfLineWords) < (size_t)kXfHalfWords
                    ? xf_static_word(seed, i)
                    : xf_payload_word(seed, -1, i);

  HbmDeviceBuf d_slab, d_tickets, d_writer, d_ctl, d_pair, d_records;
  d_slab.alloc(slab_words * sizeof(uint64_t));
  d_tickets.alloc(ticket_bytes);
  d_writer.alloc(writer_count * sizeof(uint32_t));
  d_ctl.alloc(sizeof(uint64_t) * kXfCtlWords);
  d_pair.alloc(pair_bytes);
  d_records.alloc(sizeof(XfRecord) * (size_t)max_records);
  HIP_CHECK(hipMemcpy(d_slab.ptr, h_slab.data(), slab_words * sizeof(uint64_t),
                      hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(d_writer.ptr, 0xFF, writer_count * sizeof(uint32_t)));
  HIP_CHECK(hipMemset(d_ctl.ptr, 0, sizeof(uint64_t) * kXfCtlWords));
  HIP_CHECK(hipMemset(d_pair.ptr, 0, pair_bytes));
  HIP_CHECK(hipMemset(d_records.ptr, 0, sizeof(XfRecord) * (size_t)max_records));
  CovEvent t0, t1;
  t0.create();
  t1.create();

  std::vector<uint32_t> h_tickets(n_tickets * kXfTicketStride);
  std::vector<uint32_t> h_writer(writer_count);
  std::vector<uint64_t> h_pair(kXfPairPlanes * kPlane);
  std::vector<uint64_t> writes_per_xcc(kXfXccs, 0);
  uint64_t ticket_counter_errors = 0, writer_host_range = 0;
  int rounds = 0, pairs_covered = 0, xcc_seen = 0;
  unsigned xcc_mask = 0;
  double elapsed_ms = 0.0;
  py::list round_ms;
  while (rounds < max_rounds) {
    XfHandoff a;
    a.slab = static_cast<uint64_t*>(d_slab.ptr);
    a.tickets = static_cast<uint32_t*>(d_tickets.ptr);
    a.writer_xcc = static_cast<uint32_t*>(d_writer.ptr);
    a.ctl = static_cast<unsigned long long*>(d_ctl.ptr);
    a.pair = static_cast<unsigned long long*>(d_pair.ptr);
    a.records = static_cast<XfRecord*>(d_records.ptr);
    a.seed = seed;
    a.round = (uint32_t)rounds;
    a.reps = (uint32_t)reps;
    a.group = (uint32_t)group;
    a.G = (uint32_t)G;
    a.slab_lines = (uint32_t)slab_lines;
    a.max_records = (uint32_t)max_records;
    a.poison_mask = poison_mask;
    a.poison_pair = poison_pair;
    HIP_CHECK(hipEventRecord(t0.ev));
    // the ticket counters are zeroed on the launch stream ahead of every launch
    HIP_CHECK(hipMemsetAsync(d_tickets.ptr, 0, ticket_bytes, 0));
    hipLaunchKernelGGL(xcd_handoff_kernel, dim3(nblocks), dim3(kXfBlock), 0, 0, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(t1.ev));
    HIP_CHECK(hipEventSynchronize(t1.ev));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, t0.ev, t1.ev));
    elapsed_ms += ms;
    round_ms.append((double)ms);
    ++rounds;

    HIP_CHECK(hipMemcpy(h_tickets.data(), d_tickets.ptr, ticket_bytes,
                        hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h_writer.data(), d_writer.ptr,
                        writer_count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(h_pair.data(), d_pair.ptr, pair_bytes,
                        hipMemcpyDeviceToHost));
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

  uint64_t ctl[kXfCtlWords];
  HIP_CHECK(hipMemcpy(ctl, d_ctl.ptr, sizeof(ctl), hipMemcpyDeviceToHost));
  const uint64_t claims = ctl[kXfCtlClaims];
  const size_t kept = (size_t)std::min<uint64_t>(claims, (uint64_t)max_records);
  std::vector<XfRecord> recs(kept);
  if (kept)
    HIP_CHECK(hipMemcpy(recs.data(), d_records.ptr, sizeof(XfRecord) * kept,
                        hipMemcpyDeviceToHost));

  py::dict atomics = xf_run_atomics(cus, s, seed, elapsed_ms);

  py::list records;
  for (const XfRecord& r : recs) {
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
  out["records_dropped"] = claims - (uint64_t)kept;
  out["atomics"] = atomics;
  out["elapsed_ms"] = elapsed_ms;
  return out;
}

PYBIND11_MODULE(_gpu_validator, m) {
  m.doc() = "MI355X (gfx950) native GPU health validator";
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
