// hbm_verify_sweep.hip — what limits the read-only verify phase of the
// validator's HBM pattern test on MI355X (gfx950): the pattern arithmetic or
// the launch shape?
//
// Reads a buffer far larger than the 256 MiB Infinity Cache with 16-byte
// nontemporal loads and compares every word with
//   hash     the splitmix64 finaliser the validator uses (two 64-bit
//            multiplies per word: 12 multiplier instructions per 16 bytes)
//   checker  0xAAAA.. / 0x5555.. by index parity (no multiplies)
//   none     no expected value at all: the read-only floor
// over block sizes, grid sizes and unroll depths.  If `hash` tracks `none`
// at a shape, the arithmetic hides behind HBM there.
//
// Build: hipcc --offload-arch=gfx950 -O3 experiments/hbm_verify_sweep.hip -o build/hbm_verify_sweep
// Run:   ./build/hbm_verify_sweep [buf_mib]

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define HIP_CHECK(x)                                                    \
  do {                                                                  \
    hipError_t e = (x);                                                 \
    if (e != hipSuccess) {                                              \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e),  \
              __FILE__, __LINE__);                                      \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

using u64x2 = __attribute__((ext_vector_type(2))) uint64_t;

enum { PAT_HASH = 0, PAT_CHECKER = 1, PAT_NONE = 2 };

template <int PAT>
__device__ __forceinline__ uint64_t want(uint64_t seed, uint64_t i) {
  if (PAT == PAT_NONE) return 0;
  if (PAT == PAT_CHECKER)
    return (i & 1ull) ? 0x5555555555555555ull : 0xAAAAAAAAAAAAAAAAull;
  uint64_t z = i + seed * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void fill_hash(u64x2* __restrict__ v, size_t nvec, uint64_t seed) {
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += stride) {
    u64x2 p;
    p[0] = want<PAT_HASH>(seed, 2 * i);
    p[1] = want<PAT_HASH>(seed, 2 * i + 1);
    __builtin_nontemporal_store(p, &v[i]);
  }
}

// The OR of got ^ want is the only result; it is stored under a condition the
// data never meets, which keeps every load and compare alive.
template <int PAT, int UNROLL>
__global__ void verify(const u64x2* __restrict__ v, size_t nvec, uint64_t seed,
                       uint64_t* __restrict__ sink) {
  size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t acc = 0;
  for (; i + (UNROLL - 1) * stride < nvec; i += UNROLL * stride) {
    u64x2 g[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      g[u] = __builtin_nontemporal_load(&v[i + u * stride]);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const uint64_t w = 2 * (i + u * stride);
      acc |= g[u][0] ^ want<PAT>(seed, w);
      acc |= g[u][1] ^ want<PAT>(seed, w + 1);
    }
  }
  for (; i < nvec; i += stride) {
    const u64x2 g = __builtin_nontemporal_load(&v[i]);
    acc |= g[0] ^ want<PAT>(seed, 2 * i);
    acc |= g[1] ^ want<PAT>(seed, 2 * i + 1);
  }
  if (acc == 0x0123456789ABCDEFull) sink[0] = acc;
}

using Kernel = void (*)(const u64x2*, size_t, uint64_t, uint64_t*);

static double run_case(Kernel k, const u64x2* v, size_t nvec, uint64_t* sink,
                       int grid, int block, int iters) {
  hipLaunchKernelGGL(k, dim3(grid), dim3(block), 0, 0, v, nvec, 1ull, sink);
  HIP_CHECK(hipDeviceSynchronize());
  hipEvent_t t0, t1;
  HIP_CHECK(hipEventCreate(&t0));
  HIP_CHECK(hipEventCreate(&t1));
  HIP_CHECK(hipEventRecord(t0));
  for (int i = 0; i < iters; ++i)
    hipLaunchKernelGGL(k, dim3(grid), dim3(block), 0, 0, v, nvec, 1ull, sink);
  HIP_CHECK(hipEventRecord(t1));
  HIP_CHECK(hipEventSynchronize(t1));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
  HIP_CHECK(hipEventDestroy(t0));
  HIP_CHECK(hipEventDestroy(t1));
  return (double)nvec * 16.0 * iters / 1e9 / (ms / 1e3);  // read only
}

int main(int argc, char** argv) {
  double buf_mib = argc > 1 ? atof(argv[1]) : 4096.0;
  size_t nvec = (size_t)(buf_mib * 1024 * 1024) / 16;
  u64x2* v;
  uint64_t* sink;
  HIP_CHECK(hipMalloc(&v, nvec * 16));
  HIP_CHECK(hipMalloc(&sink, 8));
  hipLaunchKernelGGL(fill_hash, dim3(65536), dim3(512), 0, 0, v, nvec, 1ull);
  HIP_CHECK(hipDeviceSynchronize());

  struct { const char* name; int unroll; Kernel k; } kernels[] = {
      {"none", 2, verify<PAT_NONE, 2>},       {"none", 4, verify<PAT_NONE, 4>},
      {"checker", 2, verify<PAT_CHECKER, 2>}, {"checker", 4, verify<PAT_CHECKER, 4>},
      {"hash", 2, verify<PAT_HASH, 2>},       {"hash", 4, verify<PAT_HASH, 4>},
  };
  int blocks[] = {256, 512};
  int grids[] = {2048, 8192, 32768, 131072};
  printf("buf=%.0f MiB, read-only GB/s\n", buf_mib);
  printf("%-8s %6s %6s %7s %10s\n", "pattern", "unroll", "block", "grid", "GB/s");
  for (auto& kk : kernels)
    for (int b : blocks)
      for (int g : grids)
        printf("%-8s %6d %6d %7d %10.0f\n", kk.name, kk.unroll, b, g,
               run_case(kk.k, v, nvec, sink, g, b, 3));
  HIP_CHECK(hipFree(v));
  HIP_CHECK(hipFree(sink));
  return 0;
}
