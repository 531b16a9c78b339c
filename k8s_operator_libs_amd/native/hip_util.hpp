// hip_util.hpp — the HIP resource holders of gpu_validator.hip.
//
// HIP_CHECK throws, so everything a check allocates is owned by one of these:
// nothing leaks when a HIP call fails half-way through a check, which is what
// happens on the unhealthy node the validator exists for.  Device memory
// (DeviceBuf), pinned and registered host memory (HostBuf, RegisteredBuf),
// streams and events.  Nothing here pools, caches or outlives the call that
// made it.

#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <new>
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

// `bytes` of pinned host memory from hipHostMalloc.  Move-only; device() is
// the address a kernel uses for it.
class HostBuf {
 public:
  HostBuf() = default;
  explicit HostBuf(size_t bytes) : bytes_(bytes) {
    HIP_CHECK(hipHostMalloc(&ptr_, bytes, hipHostMallocDefault));
  }
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept { swap(o); }
  HostBuf& operator=(HostBuf&& o) noexcept {
    swap(o);
    return *this;
  }
  ~HostBuf() {
    if (ptr_) (void)hipHostFree(ptr_);
  }
  void* get() const { return ptr_; }
  size_t size() const { return bytes_; }
  void* device() const {
    void* d = nullptr;
    HIP_CHECK(hipHostGetDevicePointer(&d, ptr_, 0));
    return d;
  }

 private:
  void swap(HostBuf& o) noexcept {
    std::swap(ptr_, o.ptr_);
    std::swap(bytes_, o.bytes_);
  }
  void* ptr_ = nullptr;
  size_t bytes_ = 0;
};

// `bytes` of page-aligned ordinary memory, registered with hipHostRegister
// (the userptr path).  Move-only; the destructor unregisters, then frees.
class RegisteredBuf {
 public:
  RegisteredBuf() = default;
  explicit RegisteredBuf(size_t bytes) : bytes_(bytes) {
    const size_t page = 4096;
    if (posix_memalign(&ptr_, page, (bytes + page - 1) / page * page) != 0) {
      ptr_ = nullptr;
      throw std::bad_alloc();
    }
    const hipError_t e = hipHostRegister(ptr_, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
      std::free(ptr_);
      ptr_ = nullptr;
      throw std::runtime_error(std::string("HIP error at hipHostRegister: ") +
                               hipGetErrorString(e));
    }
  }
  RegisteredBuf(const RegisteredBuf&) = delete;
  RegisteredBuf& operator=(const RegisteredBuf&) = delete;
  RegisteredBuf(RegisteredBuf&& o) noexcept { swap(o); }
  RegisteredBuf& operator=(RegisteredBuf&& o) noexcept {
    swap(o);
    return *this;
  }
  ~RegisteredBuf() {
    if (!ptr_) return;
    (void)hipHostUnregister(ptr_);
    std::free(ptr_);
  }
  void* get() const { return ptr_; }
  size_t size() const { return bytes_; }
  void* device() const {
    void* d = nullptr;
    HIP_CHECK(hipHostGetDevicePointer(&d, ptr_, 0));
    return d;
  }

 private:
  void swap(RegisteredBuf& o) noexcept {
    std::swap(ptr_, o.ptr_);
    std::swap(bytes_, o.bytes_);
  }
  void* ptr_ = nullptr;
  size_t bytes_ = 0;
};

// A non-blocking stream: it does not synchronise with the null stream.
struct Stream {
  hipStream_t s = nullptr;
  Stream() { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept { std::swap(s, o.s); }
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
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
