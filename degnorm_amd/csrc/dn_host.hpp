// dn_host.hpp -- move-only owners of the HIP resources of the host code: device buffers, pinned host buffers, streams and
// events.  An owner releases what it holds when it is reset, assigned to or destroyed.  A creation that fails leaves the
// owner empty and returns the hipError_t.  Buffers convert to their pointer, streams and events to their HIP handle.
//
// Also here, because every host unit needs them: the library's one error text (fail, DN_TRY), the exit rule of an entry
// point that queues work (synced), a device buffer that grows (GrowBuffer) and the scratch of hipcub calls (Scratch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/degnorm_amd.h"

namespace dn {

// The calling thread's error text: what dn_last_error() and the three per-family getters return.  fail stores msg and returns
// code; fail_hip stores "<what>: <the HIP error's text>" and returns DN_E_HIP.  (Defined in dn_api.hip.)
int fail(int code, const std::string &msg);
int fail_hip(const char *what, hipError_t e);
void clear_error();
const char *last_error();

// DN_TRY: leave the function through fail_hip when a HIP call fails, naming the expression; DN_TRY_AS names `what` instead
#define DN_TRY_AS(what, expr)                                                 \
    do {                                                                      \
        const hipError_t e_ = (expr);                                         \
        if (e_ != hipSuccess) return dn::fail_hip(what, e_);                  \
    } while (0)
#define DN_TRY(expr) DN_TRY_AS(#expr, expr)

// The exit rule of every entry point that queues work on a stream: run `body` (which returns the DN_* code on whichever
// path it leaves), then wait for `st`.  The device and pinned buffers that queued work touches, and the host variables
// that queued copies write, are declared in the frame that calls synced, not inside body: they outlive the wait, and
// nothing is still queued on caller memory when the code comes back.
template <class F> int synced(hipStream_t st, F body)
{
    const int rc = body();
    if (st) (void) hipStreamSynchronize(st);
    return rc;
}

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

// n elements and 16 bytes of slack
template <class T> hipError_t alloc_padded(DeviceBuffer<T> &b, size_t n) { return b.alloc(n * sizeof(T) + 16); }

// the capacity a store of `cap` elements grows to when it has to hold `need`
inline int64_t grown_capacity(int64_t cap, int64_t need)
{
    const int64_t nc = cap * 2 > need ? cap * 2 : need;
    return nc < 1024 ? 1024 : nc;
}

// A device array that grows: reserve(need, used, st) leaves room for `need` elements and keeps the first `used`.  The old
// buffer is released once the new one exists and the stream has finished with both.
template <class T> struct GrowBuffer {
    DeviceBuffer<T> buf;
    int64_t cap = 0;

    hipError_t reserve(int64_t need, int64_t used, hipStream_t st)
    {
        if (need <= cap) return hipSuccess;
        const int64_t new_cap = grown_capacity(cap, need);
        DeviceBuffer<T> nb;
        hipError_t e = alloc_padded(nb, (size_t) new_cap);
        if (e == hipSuccess && used > 0) e = hipMemcpyAsync(nb, buf, sizeof(T) * (size_t) used, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
        buf = std::move(nb);
        cap = new_cap;
        return hipSuccess;
    }
    T *get() const { return buf.get(); }
    operator T *() const { return buf.get(); }
};

// Temporary storage of hipcub calls on one stream.  run(call) asks `call` (void *tmp, size_t &bytes) -> hipError_t for its
// size with tmp == nullptr, adds a larger buffer when the latest is too small, and calls again with it.  Superseded
// buffers live as long as the holder: calls queued earlier may still be using them.
class Scratch {
  public:
    template <class F> hipError_t run(F call)
    {
        size_t need = 0;
        hipError_t e = call(nullptr, need);
        if (e == hipSuccess && need > bytes_) {
            DeviceBuffer<uint8_t> nb;
            e = alloc_padded(nb, need);
            if (e == hipSuccess) { bufs_.push_back(std::move(nb)); bytes_ = need; }
        }
        if (e == hipSuccess) e = call(bufs_.empty() ? nullptr : (void *) bufs_.back().get(), need);
        return e;
    }

  private:
    std::vector<DeviceBuffer<uint8_t>> bufs_;
    size_t bytes_ = 0;
};

}  // namespace dn
