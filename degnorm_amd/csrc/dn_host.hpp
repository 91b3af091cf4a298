// dn_host.hpp -- move-only owners of the HIP resources of the host code: device buffers, pinned host buffers, streams and
// events.  An owner releases what it holds when it is reset, assigned to or destroyed.  A creation that fails leaves the
// owner empty and returns the hipError_t.  Buffers convert to their pointer, streams and events to their HIP handle.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace dn {

template <class H, hipError_t (*Release)(H)> class Owner {
  public:
    Owner() = default;
    Owner(Owner &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owner &operator=(Owner &&o) noexcept
    {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~Owner() { reset(); }

    void reset()
    {
        if (h_) (void) Release(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    operator H() const { return h_; }

    // what was held is released first; `make` writes the new handle through its first argument, e.g.
    // ev.create(hipEventCreateWithFlags, hipEventDisableTiming)
    template <class F, class... A> hipError_t create(F make, A... args)
    {
        reset();
        H h = nullptr;
        const hipError_t e = make(&h, args...);
        if (e == hipSuccess) h_ = h;
        return e;
    }

  private:
    H h_ = nullptr;
};

template <class T> hipError_t device_free(T *p) { return hipFree(p); }
template <class T> hipError_t pinned_free(T *p) { return hipHostFree(p); }

template <class T> struct DeviceBuffer : Owner<T *, device_free<T>> {
    hipError_t alloc(size_t bytes)
    {
        return this->create([](T **p, size_t b) { return hipMalloc((void **) p, b); }, bytes);
    }
};

template <class T> struct PinnedBuffer : Owner<T *, pinned_free<T>> {
    hipError_t alloc(size_t bytes)
    {
        return this->create([](T **p, size_t b) { return hipHostMalloc((void **) p, b, hipHostMallocDefault); }, bytes);
    }
};

using Stream = Owner<hipStream_t, hipStreamDestroy>;
using Event = Owner<hipEvent_t, hipEventDestroy>;

}  // namespace dn
