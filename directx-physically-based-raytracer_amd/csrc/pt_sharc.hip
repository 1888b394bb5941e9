// pt_sharc.hip -- the SHARC radiance cache (gfx950): the Raytracing::Render overload with RTXGITechnique::SHARC
// (Source/Raytracing.ixx:114-148, Source/SHARC.ixx, the SHARC_UPDATE permutation of Shaders/Raytracing.hlsl).
//   k_sharc_update    one path per update pixel ((W / f) x (H / f) of them), walked in-kernel with the one-lane closest-hit walk of k_gbuffer;
//                     every vertex is inserted into the hash map and deposits into its voxel and into those of up to three vertices before it
//   k_sharc_resolve   one thread per slot: this frame's deposits + the history -> the resolved voxel, stale voxels evicted
//   the query pass is the plain frame with the SHARC instantiations of the shading bodies (pt_shade.hpp), launched by launch_raytrace
// The rules (key, hash, voxel word, update state machine, resolve, anti-firefly) are DESIGN.md section 1, "Radiance cache": the library's own, unpinned.
// All accumulation is integer atomics on u32: sums do not depend on arrival order. No float atomics.
#include "pt_internal.hpp"

#include <algorithm>
#include <cstring>

#include "pt_shade.hpp"

namespace pt {

static_assert(sizeof(PtSHARCSettings) == 28 && sizeof(PtSHARCEntry) == 32 && sizeof(PtSHARCPathVertex) == 64 && sizeof(PtSHARCPathScatter) == 128 && sizeof(PtSHARCQueryResult) == 16, "layout");
static_assert(sizeof(SharcView) == 48, "layout");

struct SharcUpdateArgs {
    unsigned long long* keys; uint4* current; const uint4* previous;     // HashEntries, VoxelData, PreviousVoxelData
    uint32_t capacity, downscale; float sceneScale, roughnessThreshold;
    PtSHARCPathVertex* log; PtSHARCPathScatter* logScatter; uint32_t logBounces;   // null: no log
};

__global__ void k_sharc_set_view(SharcView v, SharcView* dst) { if (threadIdx.x == 0) *dst = v; }
__global__ void k_sharc_set_constants(FrameConstants v, FrameConstants* dst)
{
    const uint32_t* s = (const uint32_t*)&v; uint32_t* d = (uint32_t*)dst;
    for (uint32_t i = threadIdx.x; i < sizeof(FrameConstants) / 4; i += blockDim.x) d[i] = s[i];
}

// slot of `key` after insertion, or ~0u when its bucket is full. A key that is in the bucket already is found first, whatever holes evictions
// left before it; a new key takes the first empty slot in order (compare-and-swap: every lane inserting the same key ends on the same slot,
// nothing empties a slot during the update pass).
PT_DEV uint32_t sharc_insert(unsigned long long* keys, uint32_t capacity, unsigned long long key)
{
    const uint32_t found = sharc_find(keys, capacity, key);
    if (found != ~0u) return found;
    const uint32_t base = sharc_bucket(key, capacity);
    for (uint32_t i = 0; i < kSharcBucket; i++) {
        const unsigned long long old = atomicCAS(&keys[base + i], 0ull, key);
        if (old == 0ull || old == key) return base + i;
    }
    return ~0u;
}

// uint(c * 1e3) per component, truncating, held to kSharcDepositMax; non-finite or negative gives 0. No-return atomics, zero components skipped.
PT_DEV uint32_t sharc_deposit_word(float c)
{
    if (!(isfinite(c) && c > 0.0f)) return 0u;
    return (uint32_t)fminf(c * kSharcRadianceScale, kSharcDepositMax);
}
PT_DEV void sharc_deposit(uint4* current, uint32_t slot, v3 c, uint32_t samples)
{
    uint32_t* w = (uint32_t*)&current[slot];
    const uint32_t x = sharc_deposit_word(c.x), y = sharc_deposit_word(c.y), z = sharc_deposit_word(c.z);
    if (x) atomicAdd(&w[0], x);
    if (y) atomicAdd(&w[1], y);
    if (z) atomicAdd(&w[2], z);
    if (samples) atomicAdd(&w[3], samples);
}

struct SharcState { uint32_t idx[kSharcPropagationDepth]; v3 weight[kSharcPropagationDepth]; uint32_t pathLength; };

// SharcUpdateHit. false: the path ends (resampled from the history, or the bucket was full)
PT_DEV bool sharc_update_hit(const SharcUpdateArgs& a, SharcState& s, unsigned long long key, v3 radiance, float random, bool& resampled)
{
    resampled = false;
    const uint32_t slot = sharc_insert(a.keys, a.capacity, key);
    if (slot == ~0u) return false;
    const uint32_t depth = (uint32_t)floorf((1.0f + 2.0f * random) + 0.5f);          // round(lerp(1, 3, random))
    v3 value = radiance;
    if (depth <= s.pathLength) {
        const uint4 h = a.previous[slot];
        if (h.w & kSharcSampleMask) { value = sharc_voxel_radiance(h); resampled = true; }
    }
    if (!resampled) sharc_deposit(a.current, slot, value, 1u);
    for (uint32_t i = 0; i < s.pathLength; i++) sharc_deposit(a.current, s.idx[i], value * s.weight[i], 0u);
    if (resampled) return false;
    for (uint32_t i = kSharcPropagationDepth - 1u; i > 0u; i--) { s.idx[i] = s.idx[i - 1u]; s.weight[i] = s.weight[i - 1u]; }
    s.idx[0] = slot; s.weight[0] = V3(1.0f, 1.0f, 1.0f);
    s.pathLength = min(s.pathLength + 1u, kSharcPropagationDepth - 1u);
    return true;
}

PT_DEV void sharc_log(const SharcUpdateArgs& a, uint32_t path, uint32_t bounce, v3 p, v3 n, v3 radiance, v3 thr, float random, unsigned long long key, uint32_t flags)
{
    PtSHARCPathVertex e;
    e.Position[0] = p.x; e.Position[1] = p.y; e.Position[2] = p.z; e.Flags = flags;
    e.Normal[0] = n.x; e.Normal[1] = n.y; e.Normal[2] = n.z; e.Random = random;
    e.Radiance[0] = radiance.x; e.Radiance[1] = radiance.y; e.Radiance[2] = radiance.z; e.KeyLo = (uint32_t)key;
    e.Throughput[0] = thr.x; e.Throughput[1] = thr.y; e.Throughput[2] = thr.z; e.KeyHi = (uint32_t)(key >> 32);
    a.log[(size_t)path * a.logBounces + bounce] = e;
}

// One update path (Raytracing.hlsl:103-369 under SHARC_UPDATE). Returns the rays it traced.
template <bool TEXTURED, bool LOG, typename STACK>
PT_DEV uint32_t sharc_update_path(const SceneView& sv, const FrameView& fv, const PtCamera& cam, const PtSceneData& sd, const PtGraphicsSettings& gs, const PtTextures& tx,
                                  const BlobView& bv, const SharcUpdateArgs& a, uint32_t ux, uint32_t uy, uint32_t uw, uint32_t uh, STACK& stack, TraceStats& st)
{
    const uint32_t path = uy * uw + ux;
    uint32_t rng = rng_init(ux, uy, gs.FrameIndex);                                  // :108, the update pixel
    const float jitter = rng_float(rng) - 0.5f;                                      // :112, one draw for both axes
    const float u = ((float)ux + 0.5f + jitter) / (float)uw, v = ((float)uy + 0.5f + jitter) / (float)uh;
    const uint32_t px = min((uint32_t)(u * (float)fv.width), fv.width - 1u), py = min((uint32_t)(v * (float)fv.height), fv.height - 1u);   // LOAD, :69
    const size_t pixel = (size_t)py * fv.width + px;
    v3 rayDir;
    {                                                                                // Camera::GeneratePinholeRay at this UV
        const float nx = u * 2.0f + -1.0f, ny = v * -2.0f + 1.0f;
        const v3 R = V3(cam.RightDirection), U = V3(cam.UpDirection), F = V3(cam.ForwardDirection);
        rayDir = normalize(V3(mad(ny, U.x, mad(nx, R.x, F.x)), mad(ny, U.y, mad(nx, R.y, F.y)), mad(ny, U.z, mad(nx, R.z, F.z))));
    }
    const float4 pos = ((const float4*)tx.Position)[pixel];
    const v3 zero = V3(0.0f, 0.0f, 0.0f), one = V3(1.0f, 1.0f, 1.0f);
    if (!isfinite(pos.w)) {                                                          // a primary miss updates nothing (no vertex before it), :241-252
        if (LOG) sharc_log(a, path, 0u, zero, zero, zero, zero, 0.0f, 0ull, PT_SHARC_VERTEX_MISS | PT_SHARC_VERTEX_ENDED);
        return 0u;
    }
    SurfaceHit h; BSDFSample bs; v3 emission;
    v3 baseColor; float metallic, ior, transmission;                                 // what BSDFSample::Initialize took (the log)
    {                                                                                // the primary surface from the G-buffer, :118-148
        const short4 nr = ((const short4*)tx.NormalRoughness)[pixel];
        const short2 fe = ((const short2*)tx.FlatNormal)[pixel], ge = ((const short2*)tx.GeometricNormal)[pixel];
        const uchar4 bcm = ((const uchar4*)tx.BaseColorMetalness)[pixel];
        const ushort4 rad = ((const ushort4*)tx.Radiance)[pixel];
        h.Position = V3(pos.x, pos.y, pos.z); h.PositionOffset = pos.w;
        h.FlatNormal = oct_decode(snorm16_to_f32(fe.x), snorm16_to_f32(fe.y));
        h.GeometricNormal = oct_decode(snorm16_to_f32(ge.x), snorm16_to_f32(ge.y));
        h.ShadingNormal = V3(snorm16_to_f32(nr.x), snorm16_to_f32(nr.y), snorm16_to_f32(nr.z));
        h.IsFrontFace = dot(h.GeometricNormal, rayDir) < 0.0f;
        emission = V3(f16_to_f32(rad.x), f16_to_f32(rad.y), f16_to_f32(rad.z));
        const float metal = unorm8_to_f32(bcm.w);
        const float tr = metal < 1.0f ? unorm8_to_f32(((const uint8_t*)tx.Transmission)[pixel]) : 0.0f;
        baseColor = V3(unorm8_to_f32(bcm.x), unorm8_to_f32(bcm.y), unorm8_to_f32(bcm.z)); metallic = metal; ior = f16_to_f32(((const uint16_t*)tx.IOR)[pixel]); transmission = tr;
        bs.Initialize(baseColor, metallic, snorm16_to_f32(nr.w), ior, transmission, h.IsFrontFace);
    }
    v3 DI = zero; bool isDIValid = false;
    if (gs.IsDIEnabled) {                                                            // :150-163
        v3 dd, ds; load_direct(tx, (uint32_t)pixel, dd, ds);
        DI = dd + ds; isDIValid = DI.x > 0.0f || DI.y > 0.0f || DI.z > 0.0f;
    }
    BlobReader<false> blob; blob.p = bv.base;
    const AlphaContext ac = alpha_context(sv);
    SharcState s; s.pathLength = 0u;
    for (uint32_t i = 0; i < kSharcPropagationDepth; i++) { s.idx[i] = 0u; s.weight[i] = zero; }
    v3 L = zero; uint32_t rays = 0u;
    for (uint32_t bounce = 0; bounce <= gs.Bounces; bounce++) {
        v3 thr = one;                                                                // :216
        if (bounce) {
            const v3 o = safe_world_ray_origin(h.Position, h.FlatNormal, h.PositionOffset, L);
            rayDir = L; rays++;
            const Hit hit = trace_single<false, false, false>(blob, bv, ac, o, L, 0.0f, INFINITY, stack, &st, nullptr);
            if (hit.inst == ~0u) {                                                   // SharcUpdateMiss, :241-258
                const v3 env = environment_light_color(sv, sd, rayDir);
                for (uint32_t i = 0; i < s.pathLength; i++) sharc_deposit(a.current, s.idx[i], env * s.weight[i], 0u);
                if (LOG) sharc_log(a, path, bounce, zero, zero, env, zero, 0.0f, 0ull, PT_SHARC_VERTEX_MISS | PT_SHARC_VERTEX_ENDED);
                break;
            }
            reconstruct_hit<TEXTURED>(sv, load_hit_geometry<false>(blob, bv, hit.inst, hit.slot), hit.inst, hit.u, hit.v, rayDir, h);
            const PtMaterial m = surface_material<TEXTURED>(sv, h);
            emission = isDIValid && bounce == 1u ? zero : material_emission(m);      // :302
            baseColor = V3(m.BaseColor); metallic = m.Metallic; ior = m.IOR; transmission = m.Transmission;
            bs.Initialize(baseColor, metallic, m.Roughness, ior, transmission, h.IsFrontFace);
        }
        bs.Roughness = fmaxf(bs.Roughness, a.roughnessThreshold);                    // :307
        const v3 n = dot(h.FlatNormal, rayDir) < 0.0f ? h.FlatNormal : -h.FlatNormal;
        uint32_t level; float voxelSize;
        const unsigned long long key = sharc_key(V3(cam.Position), a.sceneScale, h.Position, n, level, voxelSize);
        const v3 term = (isDIValid && bounce == 0u ? DI : zero) + emission;          // :311
        const float random = rng_float(rng);                                         // :312
        bool resampled;
        const bool on = sharc_update_hit(a, s, key, term, random, resampled);
        uint32_t flags = PT_SHARC_VERTEX_HIT | (resampled ? PT_SHARC_VERTEX_RESAMPLED : 0u);
        bool goes = on;
        if (goes) {                                                                  // :323-356, the plain path's BSDF step; no luminance cut-off
            int lobe = 0; float rnd[4];
            L = zero;
            goes = scatter_step(gs, bounce, rng, thr, h, bs, rayDir, L, lobe, LOG ? rnd : nullptr);
            if (LOG) {                                                               // what pt_bsdf_sample needs to repeat the step, and the ray that follows
                PtSHARCPathScatter e; memset(&e, 0, sizeof e);
                PtBsdfSampleQuery& q = e.Query;
                q.BaseColor[0] = baseColor.x; q.BaseColor[1] = baseColor.y; q.BaseColor[2] = baseColor.z; q.Metallic = metallic; q.Roughness = bs.Roughness;
                q.IOR = ior; q.Transmission = transmission; q.IsFrontFace = h.IsFrontFace ? 1.0f : 0.0f;
                q.GeometricNormal[0] = h.GeometricNormal.x; q.GeometricNormal[1] = h.GeometricNormal.y; q.GeometricNormal[2] = h.GeometricNormal.z;
                q.ShadingNormal[0] = h.ShadingNormal.x; q.ShadingNormal[1] = h.ShadingNormal.y; q.ShadingNormal[2] = h.ShadingNormal.z;
                q.V[0] = -rayDir.x; q.V[1] = -rayDir.y; q.V[2] = -rayDir.z;
                q.Random[0] = rnd[0]; q.Random[1] = rnd[1]; q.Random[2] = rnd[2]; q.Random[3] = rnd[3]; q.ExtFlags = gs.ExtFlags;
                const v3 o = safe_world_ray_origin(h.Position, h.FlatNormal, h.PositionOffset, L);
                e.Origin[0] = o.x; e.Origin[1] = o.y; e.Origin[2] = o.z; e.Sampled = 1u;
                e.L[0] = L.x; e.L[1] = L.y; e.L[2] = L.z; e.Goes = goes ? 1u : 0u;
                a.logScatter[(size_t)path * a.logBounces + bounce] = e;
            }
        }
        if (goes) for (uint32_t i = 0; i < s.pathLength; i++) s.weight[i] = s.weight[i] * thr;   // SharcSetThroughput, :359
        else flags |= PT_SHARC_VERTEX_ENDED;
        if (LOG) sharc_log(a, path, bounce, h.Position, n, term, thr, random, key, flags);
        if (!goes) break;
    }
    return rays;
}

template <bool TEXTURED, bool LOG>
__global__ __launch_bounds__(256) void k_sharc_update(SceneView sv, FrameView fv, const FrameConstants* __restrict__ fc, PtTextures tx, BlobView bv, SharcUpdateArgs a, DeviceCounters* counters)
{
    __shared__ uint2 ldsStack[kLdsStackDepth * 256];
    __shared__ uint32_t blockRays;
    uint2 spill[kStackSize - kLdsStackDepth];
    GroupStack<kLdsStackDepth> stack; stack.init((PT_LDS_AS void*)ldsStack, spill);
    if (threadIdx.x == 0) blockRays = 0u;
    __syncthreads();
    const uint32_t uw = fv.width / a.downscale, uh = fv.height / a.downscale;
    const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63u;                    // a wave covers an 8 x 8 square of update pixels, as in k_gbuffer
    const uint32_t x = blockIdx.x * 16u + (wv & 1u) * 8u + (ln & 7u), y = blockIdx.y * 16u + (wv >> 1) * 8u + (ln >> 3);
    TraceStats st; st.nodes = 0; st.tris = 0; st.overflow = 0;
    uint32_t rays = 0u;
    if (x < uw && y < uh) rays = sharc_update_path<TEXTURED, LOG>(sv, fv, fc->cam, fc->sd, fc->gs, tx, bv, a, x, y, uw, uh, stack, st);
    if (rays) atomicAdd(&blockRays, rays);
    __syncthreads();
    if (threadIdx.x == 0 && blockRays) atomicAdd(&counters->secondaryRays, (unsigned long long)blockRays);
    if (st.overflow + stack.overflow) atomicAdd(&counters->stackOverflows, st.overflow + stack.overflow);
}

// Resolve: one thread per slot. c: this frame's deposits (w counts its samples in all 32 bits), p: the history.
__global__ __launch_bounds__(256) void k_sharc_resolve(unsigned long long* __restrict__ keys, uint4* __restrict__ current, uint4* __restrict__ previous, uint32_t capacity,
                                                       uint32_t accumulationFrames, uint32_t staleLimit, uint32_t antiFirefly)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= capacity) return;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if (keys[i] == 0ull) { current[i] = zero; return; }
    uint4 c = current[i]; const uint4 p = previous[i];
    const unsigned long long cN = min(c.w, 1u << kSharcSampleBits), pN = p.w & kSharcSampleMask;   // a frame counts at most 2^18 samples of a voxel
    const uint32_t pF = (p.w >> kSharcSampleBits) & kSharcFrameMask, pS = p.w >> (kSharcSampleBits + kSharcFrameBits);
    if (antiFirefly && cN && pN) {                                                   // integer luminance weights 77 / 150 / 29 (of 256)
        const unsigned long long lc = 77ull * c.x + 150ull * c.y + 29ull * c.z, lh = 77ull * p.x + 150ull * p.y + 29ull * p.z;
        const unsigned long long lim = (unsigned long long)kSharcFireflyFactor * lh * cN, got = lc * pN;   // mean(c) > factor * mean(p), cross-multiplied
        if (lh && got > lim) {
            const float sc = (float)lim / (float)got;
            c.x = (uint32_t)((float)c.x * sc); c.y = (uint32_t)((float)c.y * sc); c.z = (uint32_t)((float)c.z * sc);
        }
    }
    unsigned long long R[3] = { (unsigned long long)c.x + p.x, (unsigned long long)c.y + p.y, (unsigned long long)c.z + p.z }, N = cN + pN;
    uint32_t F = pF + 1u;
    // A rescale truncates the sample count, and the sums follow the count it actually got (new / old, not the nominal factor): the voxel's mean
    // is kept. Scaling both by the nominal factor loses up to one sample of N per frame and nothing to speak of from the sums -- a mean that
    // creeps up every frame and, through the update pass's resampling, feeds on itself (DESIGN.md section 1 has the measurement).
    if (F > accumulationFrames) {
        const unsigned long long Nn = (unsigned long long)((float)N * ((float)accumulationFrames / (float)F));
        const float sc = N ? (float)Nn / (float)N : 0.0f;
        for (int k = 0; k < 3; k++) R[k] = (unsigned long long)((float)R[k] * sc);
        N = Nn; F = accumulationFrames;
    }
    if (N > kSharcSampleCap) {
        const unsigned long long Nn = (unsigned long long)((float)N * ((float)kSharcSampleCap / (float)N));
        const float sc = (float)Nn / (float)N;
        for (int k = 0; k < 3; k++) R[k] = (unsigned long long)((float)R[k] * sc);
        N = Nn;
    }
    const uint32_t S = cN ? 0u : pS + 1u;
    if (S >= staleLimit) { keys[i] = 0ull; current[i] = zero; previous[i] = zero; return; }
    current[i] = make_uint4((uint32_t)min(R[0], 0xFFFFFFFFull), (uint32_t)min(R[1], 0xFFFFFFFFull), (uint32_t)min(R[2], 0xFFFFFFFFull),
                            (uint32_t)N | (F << kSharcSampleBits) | (S << (kSharcSampleBits + kSharcFrameBits)));
}

__global__ void k_sharc_debug_keys(PtCamera cam, float sceneScale, const float* __restrict__ pos, const float* __restrict__ nrm, uint32_t n,
                                   unsigned long long* keys, uint32_t* levels, float* voxelSizes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t level; float voxelSize;
    keys[i] = sharc_key(V3(cam.Position), sceneScale, V3(pos + 3 * (size_t)i), V3(nrm + 3 * (size_t)i), level, voxelSize);
    levels[i] = level; voxelSizes[i] = voxelSize;
}

__global__ void k_sharc_debug_query(SharcView view, const float* __restrict__ pos, const float* __restrict__ nrm, const float* __restrict__ dist, const float* __restrict__ rough,
                                    uint32_t n, PtSHARCQueryResult* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    v3 r = V3(0.0f, 0.0f, 0.0f);
    const bool ok = sharc_query(view, V3(pos + 3 * (size_t)i), V3(nrm + 3 * (size_t)i), dist[i], rough[i], r);
    PtSHARCQueryResult q; q.Valid = ok ? 1u : 0u; q.Radiance[0] = r.x; q.Radiance[1] = r.y; q.Radiance[2] = r.z;
    out[i] = q;
}

static SharcView sharc_view(const Context& c, uint32_t resolvedParity)
{
    SharcView v; std::memset(&v, 0, sizeof v);
    v.keys = c.sharcKeys.data(); v.resolved = c.sharcVoxels[resolvedParity].data();
    v.cam[0] = c.camera.Position[0]; v.cam[1] = c.camera.Position[1]; v.cam[2] = c.camera.Position[2];
    v.sceneScale = c.sharcSettings.SceneScale; v.capacity = c.sharcCapacity;
    return v;
}

static hipError_t sharc_clear(Context& c)
{
    hipError_t e = hipMemsetAsync(c.sharcKeys.data(), 0, sizeof(unsigned long long) * (size_t)c.sharcCapacity, c.stream);
    for (auto& v : c.sharcVoxels) if (e == hipSuccess) e = hipMemsetAsync(v.data(), 0, sizeof(uint4) * (size_t)c.sharcCapacity, c.stream);
    return e;
}

} // namespace pt

using namespace pt;

extern "C" {

int pt_sharc_configure(PtContext* ctx, uint32_t capacity)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    if (capacity == 0u) capacity = 1u << 22;
    API_ARG(&c, capacity % kSharcBucket == 0u, "SHARC capacity must be a multiple of 32 (the bucket of the hash map)");
    API_HIP(&c, hipSetDevice(c.device));
    // (a refused growth leaves the previous configuration, and its cache, as they were)
    API_HIP(&c, grow(c.stream, nullptr, want(c.sharcKeys, capacity), want(c.sharcVoxels, capacity), want(c.sharcView, 1)));
    c.sharcCapacity = capacity; c.sharcParity = 0;
    API_HIP(&c, sharc_clear(c));
    return PT_OK;
}

int pt_sharc_set_constants(PtContext* ctx, const PtSHARCSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, s, "settings is NULL");
    API_ARG(&c, s->DownscaleFactor >= 1u && s->DownscaleFactor <= 4u, "SHARC DownscaleFactor must be 1..4");
    API_ARG(&c, s->AccumulationFrames >= 1u && s->AccumulationFrames <= kSharcFrameMask, "SHARC AccumulationFrames must be 1..63");
    API_ARG(&c, s->MaxStaleFrames >= 1u && s->MaxStaleFrames <= 255u, "SHARC MaxStaleFrames must be 1..255");
    API_ARG(&c, s->SceneScale >= 5.0f && s->SceneScale <= 100.0f, "SHARC SceneScale must be in [5, 100]");
    API_ARG(&c, s->RoughnessThreshold >= 0.0f && s->RoughnessThreshold <= 1.0f, "SHARC RoughnessThreshold must be in [0, 1]");
    API_ARG(&c, s->IsAntiFireflyEnabled <= 1u, "SHARC IsAntiFireflyEnabled must be 0 or 1");
    API_ARG(&c, s->IsHashGridVisualizationEnabled == 0u, "SHARC hash-grid visualisation is not served");
    c.sharcSettings = *s; c.haveSharcSettings = true;
    return PT_OK;
}

int pt_sharc_reset(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    if (!c.sharcCapacity) return fail(&c, PT_ERROR_NOT_READY, "no SHARC cache: call pt_sharc_configure first");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, sharc_clear(c));
    return PT_OK;
}

int pt_raytrace_render_sharc(PtContext* ctx, const PtTextures* tx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, tx, "textures is NULL");
    if (!c.sharcCapacity) return fail(&c, PT_ERROR_NOT_READY, "no SHARC cache: call pt_sharc_configure first");
    if (!c.haveSharcSettings) return fail(&c, PT_ERROR_NOT_READY, "call pt_sharc_set_constants first");
    if (!c.haveSettings) return fail(&c, PT_ERROR_NOT_READY, "call pt_raytrace_set_constants first");
    const PtGraphicsSettings& gs = c.settings;
    API_ARG(&c, c.sharding.RankCount == 1u, "the SHARC cache needs an unsharded context (RankCount 1): it is world-space and global, a band holds only its own G-buffer rows");
    API_ARG(&c, gs.Denoiser == PT_DENOISER_NONE || gs.Denoiser == PT_DENOISER_DLSS_RAY_RECONSTRUCTION, "the SHARC query serves Denoiser None and DLSS-RR, not the NRD packing");
    API_ARG(&c, !(c.debugFlags & (PT_DEBUG_BRUTE_FORCE | PT_DEBUG_TRAVERSAL_V1)), "the SHARC query needs the hit distance: not with PT_DEBUG_BRUTE_FORCE / PT_DEBUG_TRAVERSAL_V1");
    int st = check_raytrace_args(c, tx);
    if (st != PT_OK) return st;
    API_HIP(&c, hipSetDevice(c.device));
    SceneView sv; FrameView fv; memset(&sv, 0, sizeof sv); memset(&fv, 0, sizeof fv);
    st = make_views(c, gs.RenderSize[0], gs.RenderSize[1], sv, fv, true);
    if (st != PT_OK) return st;
    if (gs.Bounces == 0) return PT_OK;                       // the pass is not dispatched, Source/App.cpp:1277-1279
    const PtSHARCSettings& ss = c.sharcSettings;
    const uint32_t cur = c.sharcParity, prev = cur ^ 1u;
    const bool skip = (c.debugFlags & PT_DEBUG_SHARC_SKIP_UPDATE) != 0;
    const uint32_t uw = fv.width / ss.DownscaleFactor, uh = fv.height / ss.DownscaleFactor;
    uint32_t resolved = prev;                                // skipping: the query sees the cache as the last frame left it
    if (!skip) {
        API_HIP(&c, grow(c.stream, nullptr, want(c.frameConstants, 1)));
        API_HIP(&c, hipMemsetAsync(c.sharcVoxels[cur].data(), 0, sizeof(uint4) * (size_t)c.sharcCapacity, c.stream));
        if (uw && uh) {
            SharcUpdateArgs a; memset(&a, 0, sizeof a);
            a.keys = c.sharcKeys.data(); a.current = c.sharcVoxels[cur].data(); a.previous = c.sharcVoxels[prev].data();
            a.capacity = c.sharcCapacity; a.downscale = ss.DownscaleFactor; a.sceneScale = ss.SceneScale; a.roughnessThreshold = ss.RoughnessThreshold;
            const bool log = (c.debugFlags & PT_DEBUG_SHARC_LOG_PATHS) != 0;
            c.sharcLogPaths = 0; c.sharcLogBounces = 0;
            if (log) {
                const size_t n = (size_t)uw * uh * (gs.Bounces + 1u);
                API_HIP(&c, grow(c.stream, nullptr, want(c.sharcLogScatter, n), want(c.sharcLog, n)));
                API_HIP(&c, hipMemsetAsync(c.sharcLog.data(), 0, sizeof(PtSHARCPathVertex) * n, c.stream));
                API_HIP(&c, hipMemsetAsync(c.sharcLogScatter.data(), 0, sizeof(PtSHARCPathScatter) * n, c.stream));
                a.log = c.sharcLog.data(); a.logScatter = c.sharcLogScatter.data(); a.logBounces = gs.Bounces + 1u;
                c.sharcLogPaths = uw * uh; c.sharcLogBounces = gs.Bounces + 1u;
            }
            // the update pass reads the frame's constants where the query will: written here, and again (the same values) by the frame
            FrameConstants fc; fc.cam = c.camera; fc.sd = c.sceneData; fc.gs = c.settings;
            k_sharc_set_constants<<<1, 256, 0, c.stream>>>(fc, c.frameConstants.data());
            const dim3 grid((uw + 15u) / 16u, (uh + 15u) / 16u);
            with_flags([&](auto T, auto L) {
                k_sharc_update<T(), L()><<<grid, 256, 0, c.stream>>>(sv, fv, c.frameConstants.data(), *tx, c.scene.blob, a, c.counters.data());
            }, c.heapHasTextures, log);
            API_HIP(&c, hipGetLastError());
        }
        k_sharc_resolve<<<(c.sharcCapacity + 255u) / 256u, 256, 0, c.stream>>>(c.sharcKeys.data(), c.sharcVoxels[cur].data(), c.sharcVoxels[prev].data(), c.sharcCapacity,
                                                                                 ss.AccumulationFrames, std::min(std::max(ss.MaxStaleFrames, 8u), 255u), ss.IsAntiFireflyEnabled);
        API_HIP(&c, hipGetLastError());
        resolved = cur;
    }
    k_sharc_set_view<<<1, 64, 0, c.stream>>>(sharc_view(c, resolved), c.sharcView.data());
    API_HIP(&c, hipGetLastError());
    const hipError_t e = launch_raytrace(c, sv, fv, *tx, true);
    if (e != hipSuccess) return fail_hip(&c, e, "SHARC query frame");
    if (!skip) c.sharcParity = prev;                         // the buffers swap: this frame's resolved cache is the next frame's history
    return PT_OK;
}

int pt_sharc_download(PtContext* ctx, PtSHARCEntry* host_dst, uint32_t capacity, uint32_t* out_count)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_count && (host_dst || capacity == 0), "out_count / host_dst is NULL");
    if (!c.sharcCapacity) return fail(&c, PT_ERROR_NOT_READY, "no SHARC cache: call pt_sharc_configure first");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    std::vector<unsigned long long> keys(c.sharcCapacity); std::vector<uint4> vox(c.sharcCapacity);
    API_HIP(&c, hipMemcpy(keys.data(), c.sharcKeys.data(), sizeof(unsigned long long) * keys.size(), hipMemcpyDeviceToHost));
    API_HIP(&c, hipMemcpy(vox.data(), c.sharcVoxels[c.sharcParity ^ 1u].data(), sizeof(uint4) * vox.size(), hipMemcpyDeviceToHost));   // the resolved buffer: the last render's, now the history
    uint32_t n = 0;
    for (uint32_t i = 0; i < c.sharcCapacity; i++) {
        if (!keys[i]) continue;
        if (n < capacity) { PtSHARCEntry e; memset(&e, 0, sizeof e); e.Key = keys[i]; e.Voxel[0] = vox[i].x; e.Voxel[1] = vox[i].y; e.Voxel[2] = vox[i].z; e.Voxel[3] = vox[i].w; host_dst[n] = e; }
        n++;
    }
    *out_count = n;
    return PT_OK;
}

int pt_sharc_debug_keys(PtContext* ctx, const float* positions, const float* normals, uint32_t n, uint64_t* keys, uint32_t* levels, float* voxel_sizes)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, n == 0 || (positions && normals && keys && levels && voxel_sizes), "an array is NULL");
    if (!c.haveSharcSettings) return fail(&c, PT_ERROR_NOT_READY, "call pt_sharc_set_constants first");
    if (!c.haveCamera) return fail(&c, PT_ERROR_NOT_READY, "camera not set");
    if (!n) return PT_OK;
    API_HIP(&c, hipSetDevice(c.device));
    DeviceBuffer<float> in; DeviceBuffer<unsigned long long> dk; DeviceBuffer<uint32_t> dl; DeviceBuffer<float> dv;
    API_HIP(&c, in.reserve(6 * (size_t)n)); API_HIP(&c, dk.reserve(n)); API_HIP(&c, dl.reserve(n)); API_HIP(&c, dv.reserve(n));
    API_HIP(&c, hipMemcpyAsync(in.data(), positions, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c.stream));
    API_HIP(&c, hipMemcpyAsync(in.data() + 3 * (size_t)n, normals, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c.stream));
    k_sharc_debug_keys<<<(n + 255u) / 256u, 256, 0, c.stream>>>(c.camera, c.sharcSettings.SceneScale, in.data(), in.data() + 3 * (size_t)n, n, dk.data(), dl.data(), dv.data());
    API_HIP(&c, hipGetLastError());
    API_HIP(&c, hipMemcpyAsync(keys, dk.data(), sizeof(uint64_t) * n, hipMemcpyDeviceToHost, c.stream));
    API_HIP(&c, hipMemcpyAsync(levels, dl.data(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c.stream));
    API_HIP(&c, hipMemcpyAsync(voxel_sizes, dv.data(), sizeof(float) * n, hipMemcpyDeviceToHost, c.stream));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    return PT_OK;
}

int pt_sharc_debug_query(PtContext* ctx, const float* positions, const float* normals, const float* distances, const float* previous_roughness,
                         uint32_t n, PtSHARCQueryResult* results)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, n == 0 || (positions && normals && distances && previous_roughness && results), "an array is NULL");
    if (!c.sharcCapacity) return fail(&c, PT_ERROR_NOT_READY, "no SHARC cache: call pt_sharc_configure first");
    if (!c.haveSharcSettings) return fail(&c, PT_ERROR_NOT_READY, "call pt_sharc_set_constants first");
    if (!c.haveCamera) return fail(&c, PT_ERROR_NOT_READY, "camera not set");
    if (!n) return PT_OK;
    API_HIP(&c, hipSetDevice(c.device));
    DeviceBuffer<float> in; DeviceBuffer<PtSHARCQueryResult> out;
    API_HIP(&c, in.reserve(8 * (size_t)n)); API_HIP(&c, out.reserve(n));
    float* d = in.data();
    API_HIP(&c, hipMemcpyAsync(d, positions, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c.stream));
    API_HIP(&c, hipMemcpyAsync(d + 3 * (size_t)n, normals, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c.stream));
    API_HIP(&c, hipMemcpyAsync(d + 6 * (size_t)n, distances, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c.stream));
    API_HIP(&c, hipMemcpyAsync(d + 7 * (size_t)n, previous_roughness, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c.stream));
    k_sharc_debug_query<<<(n + 255u) / 256u, 256, 0, c.stream>>>(sharc_view(c, c.sharcParity ^ 1u), d, d + 3 * (size_t)n, d + 6 * (size_t)n, d + 7 * (size_t)n, n, out.data());
    API_HIP(&c, hipGetLastError());
    API_HIP(&c, hipMemcpyAsync(results, out.data(), sizeof(PtSHARCQueryResult) * (size_t)n, hipMemcpyDeviceToHost, c.stream));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    return PT_OK;
}

int pt_sharc_download_update_paths(PtContext* ctx, PtSHARCPathVertex* host_dst, uint32_t capacity, uint32_t* out_paths, uint32_t* out_bounces)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_paths && out_bounces && (host_dst || capacity == 0), "out_paths / out_bounces / host_dst is NULL");
    return download_counted(c, c.sharcLog.data(), c.sharcLogPaths, c.sharcLogBounces, host_dst, capacity, out_paths, out_bounces);
}

int pt_sharc_download_update_scatter(PtContext* ctx, PtSHARCPathScatter* host_dst, uint32_t capacity, uint32_t* out_paths, uint32_t* out_bounces)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_paths && out_bounces && (host_dst || capacity == 0), "out_paths / out_bounces / host_dst is NULL");
    return download_counted(c, c.sharcLogScatter.data(), c.sharcLogPaths, c.sharcLogBounces, host_dst, capacity, out_paths, out_bounces);
}

} // extern "C"
