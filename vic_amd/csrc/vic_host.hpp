// vic_host.hpp — owners of the runtime objects of the host layer (vic_pipeline.hpp, vicgpu_api.hip, vic_group.hpp).  Host code only, no kernels.
// Move-only handles: each releases what it holds in its destructor, so an entry point that returns early and a context that
// is deleted half-built leave nothing behind.  Creation returns the runtime's error code; nothing throws.  The buffers
// convert to the raw pointer, so the kernel-argument structs and the runtime calls take them as they took the pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>

// n elements of device memory (DevBuf) or of pinned host memory (PinnedBuf)
template <typename T, bool PINNED>
struct Buf {
  Buf() = default;
  explicit Buf(T* adopt) : p(adopt) {}                   // takes over a block that release() gave away
  Buf(Buf&& o) noexcept { *this = std::move(o); }
  Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
  ~Buf() { reset(); }
  void reset() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; n = 0; }
  hipError_t alloc(size_t count) {                       // releases what it held, then allocates
    reset();
    const hipError_t e = PINNED ? hipHostMalloc(&p, sizeof(T) * count, hipHostMallocDefault) : hipMalloc(&p, sizeof(T) * count);
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
  }
  hipError_t reserve(size_t count) { return count > n ? alloc(count) : hipSuccess; }      // grows only; the content is not kept
  T* release() { T* r = p; p = nullptr; n = 0; return r; }
  T* get() const { return p; }
  operator T*() const { return p; }
  size_t size() const { return n; }
  T* p = nullptr;
  size_t n = 0;
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

struct Event {
  Event() = default;
  Event(Event&& o) noexcept { std::swap(e, o.e); }
  Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
  ~Event() { reset(); }
  void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
  hipError_t create() { reset(); return hipEventCreate(&e); }                             // with timing
  hipError_t create(unsigned flags) { reset(); return hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
  hipEvent_t e = nullptr;
};

// A non-blocking stream of its own, or a borrowed one (vicgpu_set_stream), which is never destroyed here
struct Stream {
  Stream() = default;
  Stream(Stream&& o) noexcept { *this = std::move(o); }
  Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); std::swap(owned, o.owned); return *this; }
  ~Stream() { reset(); }
  void reset() { if (owned && s) (void)hipStreamDestroy(s); s = nullptr; owned = false; }
  hipError_t create() {                                  // keeps what it had when the runtime refuses
    hipStream_t fresh = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking);
    if (e == hipSuccess) { reset(); s = fresh; owned = true; }
    return e;
  }
  void borrow(hipStream_t other) { reset(); s = other; }
  bool borrowed() const { return s && !owned; }
  operator hipStream_t() const { return s; }
  hipStream_t s = nullptr;
  bool owned = false;
};
