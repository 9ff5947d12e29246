// devmem.h — move-only owners of HIP resources: device and pinned buffers, streams, events.
// A default-constructed owner holds nothing; each converts to the handle it owns and releases
// it when destroyed or reset. Creation reports hipError_t; nothing throws.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace smcrt {

template <class H, class Release>
struct Owned {
  H h{};
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : h(std::exchange(o.h, H{})) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) { reset(); h = std::exchange(o.h, H{}); }
    return *this;
  }
  ~Owned() { reset(); }
  void reset() {
    if (h) (void)Release()(h);
    h = H{};
  }
  H* out() { reset(); return &h; }  // for the hip*Create calls
  operator H() const { return h; }
};

struct FreeDevice { hipError_t operator()(void* p) const { return hipFree(p); } };
struct FreePinned { hipError_t operator()(void* p) const { return hipHostFree(p); } };
struct DestroyStream { hipError_t operator()(hipStream_t s) const { return hipStreamDestroy(s); } };
struct DestroyEvent { hipError_t operator()(hipEvent_t e) const { return hipEventDestroy(e); } };

template <class T>
struct DevBuf : Owned<T*, FreeDevice> {  // n elements of device memory (hipMalloc)
  hipError_t alloc(size_t n) {
    const hipError_t e = hipMalloc((void**)this->out(), n * sizeof(T));
    if (e != hipSuccess) this->h = nullptr;
    return e;
  }
};
template <class T>
struct PinnedBuf : Owned<T*, FreePinned> {  // n elements of pinned host memory (hipHostMalloc)
  hipError_t alloc(size_t n) {
    const hipError_t e = hipHostMalloc((void**)this->out(), n * sizeof(T));
    if (e != hipSuccess) this->h = nullptr;
    return e;
  }
};
using Stream = Owned<hipStream_t, DestroyStream>;
using Event = Owned<hipEvent_t, DestroyEvent>;

}  // namespace smcrt
