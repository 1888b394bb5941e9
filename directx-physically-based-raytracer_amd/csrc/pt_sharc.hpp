// pt_sharc.hpp -- the SHARC radiance cache's device rules ("Radiance cache"; restated in tests/sharcref.py): hash-grid
// key, hash and bucket, the voxel word, and the query-side lookup. Shared by the passes of pt_sharc.hip and by the SHARC instantiations of the
// shading bodies (pt_shade.hpp). The SDK headers (SharcCommon.h, HashGridCommon.h) are not part of the reference tree: this is the library's
// own specification, unpinned.
#pragma once
#include "pt_math.hpp"

namespace pt {

constexpr float kSharcPositionBias = 1e-4f, kSharcNormalBias = 1e-3f, kSharcRadianceScale = 1e3f;
constexpr uint32_t kSharcBucket = 32u;                                   // slots of a bucket; the capacity is a multiple of it
constexpr uint32_t kSharcSampleBits = 18u, kSharcFrameBits = 6u;         // voxel word w: samples | accumulated frames << 18 | stale frames << 24
constexpr uint32_t kSharcSampleMask = (1u << kSharcSampleBits) - 1u, kSharcFrameMask = (1u << kSharcFrameBits) - 1u;
constexpr uint32_t kSharcSampleCap = 1u << 17;                           // samples of history a voxel keeps
constexpr float kSharcDepositMax = 16383.0f;                             // per deposit and component, in units of 1e-3: 2^18 deposits cannot wrap a sum
constexpr uint32_t kSharcPropagationDepth = 4u;
constexpr uint32_t kSharcFireflyFactor = 8u;                             // anti-firefly: a frame's mean luminance per sample is held to this multiple of the history's

// what the query side reads: in device memory, rewritten in stream order by every pt_raytrace_render_sharc (the two voxel buffers alternate,
// a captured frame graph does not change)
struct SharcView {
    const unsigned long long* keys; const uint4* resolved;
    float cam[3]; float sceneScale;
    uint32_t capacity, _pad[3];
};

// Bob Jenkins' 32-bit integer hash
PT_DEV uint32_t sharc_jenkins(uint32_t a)
{
    a = (a + 0x7ED55D16u) + (a << 12);
    a = (a ^ 0xC761C23Cu) ^ (a >> 19);
    a = (a + 0x165667B1u) + (a << 5);
    a = (a + 0xD3A2646Cu) ^ (a << 9);
    a = (a + 0xFD7046C5u) + (a << 3);
    a = (a ^ 0xB55A4F09u) ^ (a >> 16);
    return a;
}
PT_DEV uint32_t sharc_bucket(unsigned long long key, uint32_t capacity)
{
    const uint32_t h = sharc_jenkins((uint32_t)key) ^ sharc_jenkins((uint32_t)(key >> 32));
    return (h % capacity) / kSharcBucket * kSharcBucket;
}

PT_DEV uint32_t sharc_level(v3 cam, v3 p)
{
    const v3 d = cam - p;
    const float d2 = d.x * d.x + d.y * d.y + d.z * d.z;                  // products and sums rounded one by one, left to right
    return (uint32_t)fminf(fmaxf(0.5f * log2f(d2), 1.0f), 1023.0f);
}
PT_DEV float sharc_voxel_size(uint32_t level, float sceneScale) { return ldexpf(1.0f, (int)level) / sceneScale; }

PT_DEV unsigned long long sharc_key(v3 cam, float sceneScale, v3 p, v3 n, uint32_t& level, float& voxelSize)
{
    level = sharc_level(cam, p);
    voxelSize = sharc_voxel_size(level, sceneScale);
    const int cx = (int)floorf((p.x + kSharcPositionBias) / voxelSize), cy = (int)floorf((p.y + kSharcPositionBias) / voxelSize),
              cz = (int)floorf((p.z + kSharcPositionBias) / voxelSize);
    const unsigned long long bits = (n.x + kSharcNormalBias < 0.0f ? 1ull : 0ull) | (n.y + kSharcNormalBias < 0.0f ? 2ull : 0ull) | (n.z + kSharcNormalBias < 0.0f ? 4ull : 0ull);
    return (unsigned long long)((uint32_t)cx & 0x1FFFFu) | ((unsigned long long)((uint32_t)cy & 0x1FFFFu) << 17) | ((unsigned long long)((uint32_t)cz & 0x1FFFFu) << 34)
         | ((unsigned long long)level << 51) | (bits << 61);
}

// slot of `key`, or ~0u: the 32 slots of its bucket, two keys per load; the scan goes on past empty slots (an eviction leaves a hole)
PT_DEV uint32_t sharc_find(const unsigned long long* __restrict__ keys, uint32_t capacity, unsigned long long key)
{
    const uint32_t base = sharc_bucket(key, capacity);
    const ulonglong2* b = (const ulonglong2*)(keys + base);
    for (uint32_t i = 0; i < kSharcBucket / 2u; i++) {
        const ulonglong2 k = b[i];
        if (k.x == key) return base + 2u * i;
        if (k.y == key) return base + 2u * i + 1u;
    }
    return ~0u;
}

PT_DEV v3 sharc_voxel_radiance(uint4 v)
{
    const float d = (float)(v.w & kSharcSampleMask) * kSharcRadianceScale;
    return V3((float)v.x / d, (float)v.y / d, (float)v.z / d);
}

// the query decision (Raytracing.hlsl:262-289) at a hit `distance` along the ray: true with the cached radiance when the hit is far and
// blurred enough for its voxel and the voxel of the resolved buffer holds samples
PT_DEV bool sharc_query(const SharcView& s, v3 p, v3 frontFlatNormal, float distance, float previousRoughness, v3& radiance)
{
    uint32_t level; float voxelSize;
    const unsigned long long key = sharc_key(V3(s.cam), s.sceneScale, p, frontFlatNormal, level, voxelSize);
    if (!(distance > voxelSize * 1.7320508f)) return false;
    const float r = fminf(previousRoughness, 0.99f), alpha = r * r, a2 = alpha * alpha;
    if (!(distance * sqrtf(0.5f * a2 / (1.0f - a2)) > voxelSize)) return false;
    const uint32_t slot = sharc_find(s.keys, s.capacity, key);
    if (slot == ~0u) return false;
    const uint4 v = s.resolved[slot];
    if (!(v.w & kSharcSampleMask)) return false;
    radiance = sharc_voxel_radiance(v);
    return true;
}

} // namespace pt
