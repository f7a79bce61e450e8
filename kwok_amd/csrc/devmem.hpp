// Ownership of device memory, pinned host memory and events, shared by the HIP libraries and
// comm.cpp (each translation unit gets its own copy: the names are in an anonymous namespace; the
// includer includes <hip/hip_runtime.h> first).  Every buffer or event a handle owns is one of
// these members, so deleting the handle releases it; a pointer that aliases into another buffer
// stays raw.  The owners free with the device's blocking hipFree / hipHostFree: the handle's
// destructor sets the device and idles its streams before the members go.
#pragma once

#include <cstddef>
#include <type_traits>
#include <utility>

namespace {

// Move-only owner of n elements of T from hipMalloc (Host = false) or hipHostMalloc (Host = true);
// T = void counts bytes.
template <class T, bool Host>
class MemBuf {
  T* p_ = nullptr;
  size_t n_ = 0;
  static constexpr size_t elem() {
    if constexpr (std::is_void<T>::value) return 1; else return sizeof(T);
  }

 public:
  MemBuf() = default;
  MemBuf(const MemBuf&) = delete;
  MemBuf& operator=(const MemBuf&) = delete;
  MemBuf(MemBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  MemBuf& operator=(MemBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; n_ = o.n_;
      o.p_ = nullptr; o.n_ = 0;
    }
    return *this;
  }
  ~MemBuf() { reset(); }

  void reset() {
    if (p_) {
      if constexpr (Host) (void)hipHostFree(p_); else (void)hipFree(p_);
    }
    p_ = nullptr;
    n_ = 0;
  }
  // frees what it holds, then allocates n elements; empty after a failure
  hipError_t alloc(size_t n) {
    reset();
    void* q = nullptr;
    hipError_t r;
    if constexpr (Host) r = hipHostMalloc(&q, n * elem(), hipHostMallocDefault); else r = hipMalloc(&q, n * elem());
    if (r != hipSuccess) return r;
    p_ = static_cast<T*>(q);
    n_ = n;
    return hipSuccess;
  }
  // allocates only when n exceeds the held capacity (the contents are not carried over)
  hipError_t grow(size_t n) { return n > n_ ? alloc(n) : hipSuccess; }
  // hands the block to the caller, who frees it
  T* release() {
    T* q = p_;
    p_ = nullptr;
    n_ = 0;
    return q;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }  // elements (bytes for T = void)
  operator T*() const { return p_; }
};

template <class T> using DevBuf = MemBuf<T, false>;
template <class T> using HostBuf = MemBuf<T, true>;

// Move-only owner of a hipEvent_t.
class Event {
  hipEvent_t ev_ = nullptr;

 public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) {
      reset();
      ev_ = o.ev_;
      o.ev_ = nullptr;
    }
    return *this;
  }
  ~Event() { reset(); }

  void reset() {
    if (ev_) (void)hipEventDestroy(ev_);
    ev_ = nullptr;
  }
  // a no-op where the event exists already (lazy creation)
  hipError_t create(unsigned flags) { return ev_ ? hipSuccess : hipEventCreateWithFlags(&ev_, flags); }
  hipEvent_t get() const { return ev_; }
  operator hipEvent_t() const { return ev_; }
};

// Blocking copies on a stream: enqueued there and complete on return.
inline hipError_t copy_in(hipStream_t s, void* dst, const void* src, size_t bytes) {
  if (!bytes) return hipSuccess;
  hipError_t r = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
  return r != hipSuccess ? r : hipStreamSynchronize(s);
}
inline hipError_t copy_out(hipStream_t s, void* dst, const void* src, size_t bytes) {
  if (!bytes) return hipSuccess;
  hipError_t r = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
  return r != hipSuccess ? r : hipStreamSynchronize(s);
}

}  // namespace
