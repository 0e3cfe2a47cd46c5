// vic_host.hpp — owners of the runtime objects of the host layer (vic_pipeline.hpp, vicgpu_api.hip, vic_group.hpp).  Host code only, no kernels.
// Move-only handles: each releases what it holds in its destructor, so an entry point that returns early and a context that
// is deleted half-built leave nothing behind.  Creation returns the runtime's error code; nothing throws.  The buffers
// convert to the raw pointer, so the kernel-argument structs and the runtime calls take them as they took the pointers.
// A buffer knows its element count, and its transfers (upload, download, fill, download_cols) are counted in elements and
// checked against it: a table is sized once, where it is allocated, and a move past its end is refused, not made.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>

// Host <-> device copies of the set-up and read-back calls go through the context's own (non-blocking) stream and are waited
// for there: a copy on the null stream is not ordered against kernels on a non-blocking stream, and a pageable host-to-device
// copy may return before its last bytes have landed in device memory.
static inline hipError_t copy_on(hipStream_t st, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

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
  bool holds(size_t first, size_t count) const { return first <= n && count <= n - first; }
  // Elements [first, first + count), or the whole buffer, on a stream; hipErrorInvalidValue, and nothing moved, past size().
  // The copies wait for the stream (copy_on).  A fill involves no host memory and is only queued: the caller waits once.
  hipError_t upload(hipStream_t st, const T* src, size_t first, size_t count) {
    return holds(first, count) ? copy_on(st, p + first, src, sizeof(T) * count, hipMemcpyHostToDevice) : hipErrorInvalidValue;
  }
  hipError_t upload(hipStream_t st, const T* src) { return upload(st, src, 0, n); }
  hipError_t download(hipStream_t st, T* dst, size_t first, size_t count) const {
    return holds(first, count) ? copy_on(st, dst, p + first, sizeof(T) * count, hipMemcpyDeviceToHost) : hipErrorInvalidValue;
  }
  hipError_t download(hipStream_t st, T* dst) const { return download(st, dst, 0, n); }
  hipError_t fill(hipStream_t st, int byte, size_t first, size_t count) {
    return holds(first, count) ? hipMemsetAsync(p + first, byte, sizeof(T) * count, st) : hipErrorInvalidValue;
  }
  hipError_t fill(hipStream_t st, int byte) { return fill(st, byte, 0, n); }
  hipError_t alloc_fill(size_t count, int byte, hipStream_t st) {                         // empty when either step fails
    hipError_t e = alloc(count);
    if (e == hipSuccess && (e = fill(st, byte)) != hipSuccess) reset();
    return e;
  }
  // The table [nrow][ncell] at the start of the buffer -> the columns [0, ncell) of a host table whose rows are ld cells wide
  // (a group reads one shard's columns straight into the caller's global table); packed when ld == ncell.  Waits like a copy.
  hipError_t download_cols(hipStream_t st, T* dst, size_t ld, size_t nrow, size_t ncell) const {
    if (ld < ncell || !holds(0, nrow * ncell)) return hipErrorInvalidValue;
    if (ld == ncell) return download(st, dst, 0, nrow * ncell);
    hipError_t e = hipMemcpy2DAsync(dst, sizeof(T) * ld, p, sizeof(T) * ncell, sizeof(T) * ncell, nrow, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
  }
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

// The event pair of an entry that reports its time on a stream under VICGPU_STATS.  Off (create(false)), it holds no event and
// every call is a no-op that succeeds: an entry creates it before its first upload and calls it unconditionally.
struct StreamTimer {
  hipError_t create(bool enabled) {
    on = enabled;
    hipError_t e = on ? t0.create() : hipSuccess;
    if (on && e == hipSuccess) e = t1.create();
    return e;
  }
  hipError_t begin(hipStream_t st) { return on ? hipEventRecord(t0, st) : hipSuccess; }
  hipError_t end(hipStream_t st) { return on ? hipEventRecord(t1, st) : hipSuccess; }
  bool elapsed(float* ms) { return on && hipEventElapsedTime(ms, t0, t1) == hipSuccess; }      // once the stream has passed end()
  Event t0, t1;
  bool on = false;
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
