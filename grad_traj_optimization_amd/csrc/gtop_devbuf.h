// gtop_devbuf.h — the owner of the C-ABI layer's memory: a device buffer, or the pinned host staging a kernel can
// address.  Pointer and capacity live together and the destructor frees, so a buffer is declared in one place and
// nowhere else: no list of pointers to release, no capacity to name beside it.  Grow-only: a buffer that is large
// enough is left where it is (its address is what enqueued work and captured launches hold), so a caller that walks
// through problems of different sizes does not reallocate.  A buffer the library only BORROWS is a plain pointer kept
// beside the owner, never inside it.  Freed with the device current that the owner's context made current.
#ifndef GTOP_DEVBUF_H_
#define GTOP_DEVBUF_H_

#include <hip/hip_runtime.h>
#include <stddef.h>

// where a buffer's memory comes from: the device's own, or (GtopPinnedBuf) pinned host memory mapped into the device's
// address space, coherent (fine-grained) — a kernel's stores reach host memory as they retire, not at the end of the
// kernel, so the host can poll them; hipHostGetDevicePointer gives the address a kernel uses
struct GtopDeviceMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void *p) { return hipFree(p); }
};
struct GtopPinnedMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent); }
  static hipError_t free(void *p) { return hipHostFree(p); }
};

template <typename T, typename Mem = GtopDeviceMem>
class GtopDevBuf {
 public:
  GtopDevBuf() = default;
  GtopDevBuf(GtopDevBuf &&o) noexcept : p_(o.p_), capacity_(o.capacity_) { o.p_ = nullptr; o.capacity_ = 0; }
  GtopDevBuf &operator=(GtopDevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_; capacity_ = o.capacity_;
      o.p_ = nullptr; o.capacity_ = 0;
    }
    return *this;
  }
  GtopDevBuf(const GtopDevBuf &) = delete;
  GtopDevBuf &operator=(const GtopDevBuf &) = delete;
  ~GtopDevBuf() { release(); }

  // room for n elements: nothing happens when there is; otherwise the old buffer is freed, then the new one allocated
  // (contents are not carried over), and a failure leaves the buffer empty
  hipError_t reserve(size_t n) {
    if (n <= capacity_ && p_) return hipSuccess;
    release();
    const hipError_t e = Mem::alloc(reinterpret_cast<void **>(&p_), n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    else capacity_ = n;
    return e;
  }
  void release() {
    if (p_) (void)Mem::free(p_);
    p_ = nullptr;
    capacity_ = 0;
  }
  T *data() const { return p_; }
  size_t capacity() const { return capacity_; }   // elements

 private:
  T *p_ = nullptr;
  size_t capacity_ = 0;
};
template <typename T> using GtopPinnedBuf = GtopDevBuf<T, GtopPinnedMem>;

#endif  // GTOP_DEVBUF_H_
