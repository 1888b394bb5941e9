// pt_memory.hpp -- host-side owners of device memory, pinned memory and HIP handles. Every allocation of the library has exactly one of
// these as its owner; kernel-argument structs hold plain pointers that an owner fills in. A live device buffer of a context grows in one way
// only, grow() below: transactional (fresh buffers first, so a failure changes nothing) and with one wait for the stream.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstddef>
#include <memory>
#include <tuple>
#include <type_traits>

namespace pt {

// A move-only array of T in device (hipMalloc) or pinned host (hipHostMalloc) memory. reserve() allocates into an empty one, once; a buffer that
// holds an allocation is replaced by moving a fresh one in, which frees the old allocation: grow() does that for device buffers a stream may still read.
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
    // allocates exactly n elements into an empty buffer; a buffer that holds an allocation is refused (it grows through grow())
    hipError_t reserve(size_t n)
    {
        if (p_) return hipErrorInvalidValue;
        if (n == 0) return hipSuccess;
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

// ---- growth of device buffers that work in flight on `stream` may still read ---------------------------------------------------------
// A demand: each of the N buffers at `buffers` is to hold at least `count` elements. want() makes one from a buffer or an array of them.
template <typename T, size_t N> struct Demand { DeviceBuffer<T>* buffers; size_t count; };
template <typename T> Demand<T, 1> want(DeviceBuffer<T>& b, size_t count) { return { &b, count }; }
template <typename T, size_t N> Demand<T, N> want(DeviceBuffer<T> (&b)[N], size_t count) { return { b, count }; }

// Grows a group of buffers, of mixed T, as one transaction. If every buffer holds its demand already, nothing is allocated and nothing waits:
// a few compares. Otherwise a fresh buffer of exactly the demanded size is allocated for each one that is short, and only for those. If an
// allocation fails, the fresh ones are released, the error is returned (and taken off the runtime's last-error slot), and no buffer of the
// group has changed: pointer, capacity and contents are what they were. On success the stream is waited for once, the fresh buffers are moved
// in, which frees the old ones, and *grew is set: the caller then resets what depended on the old buffers. Contents are not carried over.
// While it grows, the old and the new allocations of the group exist side by side.
template <typename T, size_t N> bool demand_fits(const Demand<T, N>& d)
{
    for (size_t i = 0; i < N; ++i) if (d.buffers[i].capacity() < d.count) return false;
    return true;
}
template <typename T, size_t N> hipError_t demand_allocate(const Demand<T, N>& d, std::array<DeviceBuffer<T>, N>& fresh)
{
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < N && e == hipSuccess; ++i) if (d.buffers[i].capacity() < d.count) e = fresh[i].reserve(d.count);
    return e;
}
template <typename T, size_t N> void demand_commit(const Demand<T, N>& d, std::array<DeviceBuffer<T>, N>& fresh)
{
    for (size_t i = 0; i < N; ++i) if (fresh[i]) d.buffers[i] = std::move(fresh[i]);
}
template <typename... T, size_t... N>
hipError_t grow(hipStream_t stream, bool* grew, Demand<T, N>... demands)
{
    if (grew) *grew = false;
    if ((... && demand_fits(demands))) return hipSuccess;
    std::tuple<std::array<DeviceBuffer<T>, N>...> fresh;               // released on every return that has not moved them in
    hipError_t e = hipSuccess;
    std::apply([&](auto&... f) { (void)(... && ((e = demand_allocate(demands, f)) == hipSuccess)); }, fresh);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);             // work in flight may still read the old buffers
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    std::apply([&](auto&... f) { (demand_commit(demands, f), ...); }, fresh);
    if (grew) *grew = true;
    return hipSuccess;
}

// A table that never changes, uploaded by the first call that needs it: a fresh buffer, a synchronous copy, moved in when both succeeded.
template <typename T> hipError_t upload_once(DeviceBuffer<T>& table, const void* host, size_t bytes)
{
    if (table) return hipSuccess;
    DeviceBuffer<T> dev;
    hipError_t e = dev.reserve(bytes / sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(dev.data(), host, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) table = std::move(dev);
    return e;
}

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
