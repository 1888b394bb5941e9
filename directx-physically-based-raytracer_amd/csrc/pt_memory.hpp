// pt_memory.hpp -- host-side owners of device memory, pinned memory and HIP handles. Every allocation of the library has exactly one of
// these as its owner; kernel-argument structs hold plain pointers that an owner fills in.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <type_traits>

namespace pt {

// A move-only array of T in device (hipMalloc) or pinned host (hipHostMalloc) memory. reserve() is grow-only and never synchronises: a
// caller that may still have work in flight on the old allocation waits for its stream first. Buffers that grow together keep one grow
// decision for the group, read from the buffer allocated last: a failed allocation leaves that one empty (capacity 0), so the next call
// grows the group again instead of using a null pointer.
template <typename T, bool Pinned>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    ~Buffer() { reset(); }

    T* data() const { return p_; }
    size_t capacity() const { return n_; }                 // in elements
    explicit operator bool() const { return p_ != nullptr; }

    void reset()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; n_ = 0;
    }
    // at least n elements: if they do not fit, the old allocation is freed and exactly n are allocated (contents are not kept). On failure
    // the buffer is empty.
    hipError_t reserve(size_t n)
    {
        if (n <= n_) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, sizeof(T) * n) : hipMalloc(&p, sizeof(T) * n);
        if (e != hipSuccess) return e;
        p_ = (T*)p; n_ = n;
        return hipSuccess;
    }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

// owning handles of the runtime's objects
template <typename H, hipError_t (*Destroy)(H)> struct HandleDeleter { void operator()(H h) const { (void)Destroy(h); } };
template <typename H, hipError_t (*Destroy)(H)> using Handle = std::unique_ptr<std::remove_pointer_t<H>, HandleDeleter<H, Destroy>>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

inline hipError_t create_event(Event& out, unsigned flags)
{
    hipEvent_t e = nullptr;
    const hipError_t r = hipEventCreateWithFlags(&e, flags);
    if (r == hipSuccess) out.reset(e);
    return r;
}
inline hipError_t create_stream(Stream& out, unsigned flags)
{
    hipStream_t s = nullptr;
    const hipError_t r = hipStreamCreateWithFlags(&s, flags);
    if (r == hipSuccess) out.reset(s);
    return r;
}

} // namespace pt
