// hip_util.hpp — the HIP resource holders of gpu_validator.hip.
//
// HIP_CHECK throws, so everything a check allocates is owned by one of these:
// nothing leaks when a HIP call fails half-way through a check, which is what
// happens on the unhealthy node the validator exists for.  Nothing here pools,
// caches or outlives the call that made it.

#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <stdexcept>
#include <string>
#include <utility>

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error at " #expr ": ") +       \
                               hipGetErrorString(_e));                         \
    }                                                                          \
  } while (0)

// n elements of T in device memory.  Move-only; the destructor frees and
// ignores the return code.  The only place that turns a count into bytes.
template <typename T>
class DeviceBuf {
 public:
  DeviceBuf() = default;
  explicit DeviceBuf(size_t n) : n_(n) { HIP_CHECK(hipMalloc(&ptr_, sizeof(T) * n)); }
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  DeviceBuf(DeviceBuf&& o) noexcept { swap(o); }
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {  // o frees what this held
    swap(o);
    return *this;
  }
  ~DeviceBuf() { reset(); }

  // free now, on whichever device is current
  void reset() {
    if (ptr_) (void)hipFree(ptr_);
    ptr_ = nullptr;
    n_ = 0;
  }
  T* get() const { return static_cast<T*>(ptr_); }
  size_t size() const { return n_; }

  void upload(const T* src, size_t n) {
    check(n);
    HIP_CHECK(hipMemcpy(ptr_, src, sizeof(T) * n, hipMemcpyHostToDevice));
  }
  void download(T* dst, size_t n) const {
    check(n);
    HIP_CHECK(hipMemcpy(dst, ptr_, sizeof(T) * n, hipMemcpyDeviceToHost));
  }
  void fill(int byte) { HIP_CHECK(hipMemset(ptr_, byte, sizeof(T) * n_)); }
  // the same, enqueued on the null stream
  void fill_async(int byte) {
    HIP_CHECK(hipMemsetAsync(ptr_, byte, sizeof(T) * n_, 0));
  }

 private:
  void swap(DeviceBuf& o) noexcept {
    std::swap(ptr_, o.ptr_);
    std::swap(n_, o.n_);
  }
  void check(size_t n) const {
    if (n > n_) throw std::out_of_range("DeviceBuf: copy of more than was allocated");
  }
  void* ptr_ = nullptr;
  size_t n_ = 0;
};

struct Event {
  hipEvent_t ev = nullptr;
  Event() { HIP_CHECK(hipEventCreate(&ev)); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (ev) (void)hipEventDestroy(ev);
  }
};

// Two events on the null stream.  time_ms records, runs `work` (which enqueues
// and, where the caller wants it, checks hipGetLastError), records,
// synchronises and returns the time between the two records.
struct EventTimer {
  Event t0, t1;
  template <typename Work>
  float time_ms(Work&& work) {
    HIP_CHECK(hipEventRecord(t0.ev));
    work();
    HIP_CHECK(hipEventRecord(t1.ev));
    HIP_CHECK(hipEventSynchronize(t1.ev));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, t0.ev, t1.ev));
    return ms;
  }
};
