// pt_memory_check -- the contract of grow() and reserve() (pt_memory.hpp), checked by a program of its own: no kernels, no library.
// With a device it walks growth, the steady state, a refused growth and a partial growth; without one (hipMalloc answers
// hipErrorNoDevice) every call must fail and every buffer must stay empty. Prints one line per step and "mode: ..." first; exit status 0
// only if every step held.
#include "pt_memory.hpp"

#include <cstdio>
#include <vector>

using namespace pt;

static int g_failed = 0;
static void check(bool ok, const char* what)
{
    std::printf("%s: %s\n", ok ? "ok" : "FAILED", what);
    if (!ok) g_failed++;
}

static int without_device()
{
    std::printf("mode: no device\n");
    DeviceBuffer<float> f; DeviceBuffer<uint4> q[2];
    bool grew = true;
    check(grow(nullptr, &grew, want(f, 1024), want(q, 16)) != hipSuccess && !grew, "a growth fails and reports nothing grown");
    check(!f && !q[0] && !q[1] && f.capacity() == 0 && q[0].capacity() == 0 && q[1].capacity() == 0, "every buffer of the group stays empty");
    check(grow(nullptr, &grew, want(f, 0), want(q, 0)) == hipSuccess && !grew, "a demand that is held already allocates nothing");
    check(f.reserve(16) != hipSuccess && !f && f.capacity() == 0, "reserve fails and leaves the buffer empty");
    const float one = 1.0f;
    check(upload_once(f, &one, sizeof one) != hipSuccess && !f, "upload_once fails and leaves the table empty");
    (void)hipGetLastError();
    return g_failed ? 1 : 0;
}

int main()
{
    {
        DeviceBuffer<float> probe;
        const hipError_t e = probe.reserve(1);
        (void)hipGetLastError();
        if (e == hipErrorNoDevice) return without_device();
        if (e != hipSuccess) { std::printf("mode: device\nFAILED: hipMalloc of 4 bytes: %s\n", hipGetErrorString(e)); return 1; }
    }
    std::printf("mode: device\n");
    DeviceBuffer<float> f; DeviceBuffer<uint4> q;
    bool grew = false;

    // 1. growth
    hipError_t e = grow(nullptr, &grew, want(f, 1024), want(q, 16));
    check(e == hipSuccess && grew && f.capacity() == 1024 && q.capacity() == 16 && f && q, "1. both buffers grow");
    if (g_failed) return 1;                                          // nothing below makes sense without them
    std::vector<float> pattern(1024), back(1024, 0.0f);
    for (size_t i = 0; i < pattern.size(); ++i) pattern[i] = (float)(i * 3 + 1);
    check(hipMemcpy(f.data(), pattern.data(), sizeof(float) * 1024, hipMemcpyHostToDevice) == hipSuccess, "1. the pattern is written");

    // 2. the steady state
    float* const fp = f.data(); uint4* const qp = q.data();
    e = grow(nullptr, &grew, want(f, 1024), want(q, 16));
    check(e == hipSuccess && !grew && f.data() == fp && q.data() == qp, "2. the same demands grow nothing and move nothing");

    // 3. a growth that cannot be served: 2^46 uint4 are 2^50 bytes
    e = grow(nullptr, &grew, want(f, 2048), want(q, (size_t)1 << 46));
    check(e != hipSuccess && !grew, "3. an error is returned");
    check(f.data() == fp && q.data() == qp && f.capacity() == 1024 && q.capacity() == 16, "3. pointers and capacities are unchanged");
    check(hipMemcpy(back.data(), f.data(), sizeof(float) * 1024, hipMemcpyDeviceToHost) == hipSuccess && back == pattern, "3. the pattern reads back intact");
    check(hipGetLastError() == hipSuccess, "3. hipGetLastError() is clean");

    // 4. only the short buffer grows
    e = grow(nullptr, &grew, want(f, 2048), want(q, 16));
    check(e == hipSuccess && grew && f.capacity() >= 2048 && q.data() == qp && q.capacity() == 16, "4. the float buffer grows, the uint4 buffer stays");

    // 5. reserve is for empty buffers
    check(f.reserve(4096) == hipErrorInvalidValue && f.capacity() >= 2048 && f.capacity() < 4096, "5. reserve refuses a buffer that holds an allocation");
    (void)hipGetLastError();
    return g_failed ? 1 : 0;
}
