// pt_filter.hpp -- what the three screen-space filters (pt_denoise.hip, pt_upscale.hip, pt_reconstruct.hip) have in common, once.
//
//   device: the small arithmetic of the specs ("Denoiser", "Upscaler", "Ray reconstruction"), every expression in
//           the operation order the specs give, one rounding each; FlTaps, the four bilinear taps of a reprojected position; fl_resolve,
//           steps 1-6 of the upscaler over a tap source (the upscaler's texels, the reconstruction's filtered signal x albedo)
//   host:   the refusals the entry points share (bound textures, jitter, sizes), the settings hand-over, the transactional growth of a
//           history, the read-back of a history's .w
#pragma once
#include "pt_internal.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace pt {

constexpr uint32_t kFlMaxSize = 16384u;
constexpr int kFlTile = 16;                                    // a workgroup is one 16 x 16 tile of pixels
constexpr uint32_t kFlStagedMaxStep = 4u;                      // a-trous: 16 + 4 * step pixels a side, 32 x 32 records at step 4
constexpr float kFlWeightFloor = 0.015625f;                    // 1 / 64: the least weight of the nearest sample
constexpr float kFlDenominatorFloor = 7.62939453125e-06f;      // 2^-17: the guard of the inverse tone map
constexpr float kFlMax16 = 65504.0f;

typedef uint16_t h4v __attribute__((ext_vector_type(4)));     // one fp16 RGBA texel
typedef int16_t  s4v __attribute__((ext_vector_type(4)));     // one snorm16 RGBA texel

PT_DEV float fl_max0(float x) { return x > 0.0f ? x : 0.0f; }
PT_DEV float fl_max3(float r, float g, float b) { const float m = r > g ? r : g; return m > b ? m : b; }
PT_DEV float fl_lum(float4 c) { return ml_luminance(V3(c.x, c.y, c.z)); }
// hist + (cur - hist) * (1 / n)
PT_DEV float fl_blend(float hist, float cur, float inv) { return hist + (cur - hist) * inv; }
PT_DEV v3 fl_rgb16(h4v q) { return V3(f16_to_f32(q.x), f16_to_f32(q.y), f16_to_f32(q.z)); }
// a colour as a filter takes it: rgb all 0 when one of them is not finite
PT_DEV v3 fl_guard(v3 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z) ? c : V3(0.0f, 0.0f, 0.0f); }
// wg, wn and the roughness weight of an a-trous tap (the variance stage asks whether the first two are > 0)
PT_DEV float fl_wg(v3 Np, v3 Pp, v3 Pq, float planeScale) { return fl_max0(1.0f - fabsf(dot(Np, Pq - Pp)) / planeScale); }
PT_DEV float fl_wn(v3 Np, v3 Nq, float normalCosine) { return fl_max0((dot(Np, Nq) - normalCosine) / (1.0f - normalCosine)); }
PT_DEV float fl_wr(float rp, float rq, float roughnessFraction) { return fl_max0(1.0f - fabsf(rq - rp) / (roughnessFraction * (rp > rq ? rp : rq) + 1e-6f)); }
// the 3 x 3 binomial kernel that blurs the variance, and the five taps a side of the a-trous kernel
PT_DEV float fl_blur3(int dx, int dy) { return (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f); }
PT_DEV float fl_h5(int d) { const float h[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f }; return h[d + 2]; }
// the cap of a specular history: shorter on smooth surfaces that moved (surface motion only: no virtual motion)
PT_DEV float fl_specular_cap(float maxFrames, float r, float mvx, float mvy)
{
    if (!(mvx * mvx + mvy * mvy > 0.0625f)) return maxFrames;
    float t = r / 0.5f;
    t = t < 1.0f ? t : 1.0f;
    return 1.0f + floorf((maxFrames - 1.0f) * fl_max0(t));
}
// floor((o + 0.5) s - jitter) clamped into the frame, as a float: the nearest render sample of an output coordinate
PT_DEV float fl_nearest(float oc, float s, float j, float last)
{
    const float c = floorf(oc * s - j);
    return c < 0.0f ? 0.0f : (c > last ? last : c);
}

// The four bilinear taps around the position (fx, fy) of a W x H frame, row-major: tap t is (x0 + (t & 1), y0 + (t >> 1)). Which of
// them a pass accepts (depth, plane, normal, roughness, length) is the pass's own business.
struct FlTaps {
    float x0, y0, wx[2], wy[2];
    uint32_t W, H;
    PT_DEV FlTaps(float fx, float fy, uint32_t W_, uint32_t H_) : x0(floorf(fx)), y0(floorf(fy)), W(W_), H(H_)
    {
        const float tx = fx - x0, ty = fy - y0;
        wx[0] = 1.0f - tx; wx[1] = tx; wy[0] = 1.0f - ty; wy[1] = ty;
    }
    PT_DEV bool inside(int t) const
    {
        const float xf = x0 + (float)(t & 1), yf = y0 + (float)(t >> 1);
        return xf >= 0.0f && xf <= (float)(W - 1u) && yf >= 0.0f && yf <= (float)(H - 1u);
    }
    PT_DEV uint32_t index(int t) const { return (uint32_t)(y0 + (float)(t >> 1)) * W + (uint32_t)(x0 + (float)(t & 1)); }   // of an inside tap
    PT_DEV float weight(int t) const { return wx[t & 1] * wy[t >> 1]; }
};

// What the resolve needs beside its tap source: the output history and the geometry of the two grids.
struct FlResolveArgs {
    void* color;
    float4* hist; float* histZ;                                // this frame's parity, written
    const float4* prevHist; const float* prevZ;                // the last frame's
    uint32_t Rw, Rh, Ow, Oh, reset;                            // reset: no history
    float sx, sy, jx, jy, maxFrames, r2, tau;                  // s = RenderSize / OutputSize, r2 = KernelRadius^2
};

// DESIGN.md section 1, "Upscaler", steps 1-6 for the output pixel (ox, oy). A Source names a render texel (qx, qy) inside the frame by
// j = at(qx, qy), its index where the source keeps it, and answers depth(j), motion(j) (the fp16 texel) and colour(j) (three guarded floats).
template <typename Source>
PT_DEV void fl_resolve(const FlResolveArgs& a, uint32_t ox, uint32_t oy, const Source& src)
{
    const int Rw = (int)a.Rw, Rh = (int)a.Rh;
    // 1: position
    const float oxc = (float)ox + 0.5f, oyc = (float)oy + 0.5f;
    const float ux = oxc * a.sx, uy = oyc * a.sy;
    const int cx = (int)fl_nearest(oxc, a.sx, a.jx, (float)(Rw - 1)), cy = (int)fl_nearest(oyc, a.sy, a.jy, (float)(Rh - 1));

    // 2 and 3: the dilation and the current colour over the same 3 x 3 taps, row-major
    float best = INFINITY;
    uint32_t bj = 0;
    bool found = false;
    float wsum = 0.0f, k = 0.0f;
    float acc[3] = { 0.0f, 0.0f, 0.0f }, lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        const int qx = cx + dx, qy = cy + dy;
        if (qx < 0 || qx >= Rw || qy < 0 || qy >= Rh) continue;
        const uint32_t j = src.at(qx, qy);
        const float zq = src.depth(j);
        if (isfinite(zq) && zq < best) { best = zq; bj = j; found = true; }
        const float ddx = (((float)qx + 0.5f) + a.jx) - ux, ddy = (((float)qy + 0.5f) + a.jy) - uy;
        const float d2 = ddx * ddx + ddy * ddy;
        float w = fl_max0(1.0f - d2 / a.r2);
        w = w * w;
        if (dx == 0 && dy == 0) { w = w < kFlWeightFloor ? kFlWeightFloor : w; k = w; }
        const v3 q = src.colour(j);
        const float c[3] = { q.x, q.y, q.z };
        const float den = 1.0f + fl_max0(fl_max3(c[0], c[1], c[2]));
        for (int ch = 0; ch < 3; ++ch) {
            const float t = c[ch] / den;
            lo[ch] = t < lo[ch] ? t : lo[ch]; hi[ch] = t > hi[ch] ? t : hi[ch];
            if (w > 0.0f) acc[ch] = acc[ch] + w * t;
        }
        if (w > 0.0f) wsum = wsum + w;
    }
    const float cur[3] = { acc[0] / wsum, acc[1] / wsum, acc[2] / wsum };
    const float z = best;
    float mvx = 0.0f, mvy = 0.0f, mvz = 0.0f;
    if (found) { const h4v m = src.motion(bj); mvx = f16_to_f32(m.x); mvy = f16_to_f32(m.y); mvz = f16_to_f32(m.z); }

    // 4: the previous output at (o + 0.5) + mv / s, four bilinear taps, row-major
    const FlTaps taps((oxc + mvx / a.sx) - 0.5f, (oyc + mvy / a.sy) - 0.5f, a.Ow, a.Oh);
    const float zp = z + mvz, tol = a.tau * fabsf(zp);
    float hsum = 0.0f, h[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int t = 0; t < 4; ++t) {
        if (a.reset || !taps.inside(t)) continue;
        const uint32_t j = taps.index(t);
        const float zh = a.prevZ[j];
        if (!(found ? fabsf(zh - zp) <= tol : !isfinite(zh))) continue;
        const float w = taps.weight(t);
        const float4 q = a.prevHist[j];
        hsum = hsum + w;
        h[0] = h[0] + w * q.x; h[1] = h[1] + w * q.y; h[2] = h[2] + w * q.z; h[3] = h[3] + w * q.w;
    }

    // 5: clamp and blend
    float out[3] = { cur[0], cur[1], cur[2] }, n = k;          // disoccluded
    if (hsum > 0.0f) {
        const float n1 = h[3] / hsum + k;
        n = n1 < a.maxFrames ? n1 : a.maxFrames;
        const float alpha = k / n;
        if (!(alpha >= 1.0f)) for (int ch = 0; ch < 3; ++ch) {
            float hc = h[ch] / hsum;
            hc = hc < lo[ch] ? lo[ch] : (hc > hi[ch] ? hi[ch] : hc);
            out[ch] = hc + (cur[ch] - hc) * alpha;
        }
    }

    // 6: store
    const uint32_t i = oy * a.Ow + ox;
    a.hist[i] = float4{ out[0], out[1], out[2], n };
    a.histZ[i] = z;
    float den = 1.0f - fl_max0(fl_max3(out[0], out[1], out[2]));
    den = den < kFlDenominatorFloor ? kFlDenominatorFloor : den;
    uint16_t c16[3];
    for (int ch = 0; ch < 3; ++ch) {
        const float c = out[ch] / den;
        c16[ch] = f32_to_f16(c > kFlMax16 ? kFlMax16 : (c < -kFlMax16 ? -kFlMax16 : c));
    }
    ((PT_GLOBAL_AS h4v*)a.color)[i] = h4v{ c16[0], c16[1], c16[2], (uint16_t)0x3C00u };
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------

// One texture an entry point was handed. The refusals, over the whole table in this order: a NULL pointer, then a pointer that is not
// aligned to its texel. PT_OK when there is none.
struct BoundTexture { const char* name; const void* p; uint32_t texel; };
template <size_t N>
int fl_check_bound(Context& c, const BoundTexture (&bound)[N])
{
    for (const auto& b : bound) if (!b.p) return fail(&c, PT_ERROR_INVALID_ARGUMENT, std::string(b.name) + " is NULL");
    for (const auto& b : bound) if ((uintptr_t)b.p & (b.texel - 1u))
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, std::string(b.name) + " is not aligned to its texel (" + std::to_string(b.texel) + " bytes)");
    return PT_OK;
}

inline int fl_check_jitter(Context& c, const float jitter[2])
{
    for (int k = 0; k < 2; ++k) if (!(std::isfinite(jitter[k]) && jitter[k] >= -0.5f && jitter[k] <= 0.5f))
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "jitter must be finite and in [-0.5, 0.5] on both axes");
    return PT_OK;
}

// nullptr when a render size, or a render and an output size, are in range, else the message of the refusal
inline const char* fl_check_sizes(const uint32_t render[2], const uint32_t output[2] = nullptr)
{
    for (int k = 0; k < 2; ++k) if (!(render[k] >= 1u && render[k] <= kFlMaxSize)) return "RenderSize must be 1..16384 on both axes";
    if (!output) return nullptr;
    for (int k = 0; k < 2; ++k) if (!(output[k] >= 1u && output[k] <= kFlMaxSize)) return "OutputSize must be 1..16384 on both axes";
    for (int k = 0; k < 2; ++k) if (!(render[k] <= output[k] && output[k] <= 4u * render[k])) return "OutputSize must be RenderSize..4 RenderSize on both axes";
    return nullptr;
}

// pt_*_set_constants behind the context check: `check` gives nullptr or the message of the refusal
template <typename S>
int fl_set_constants(Context& c, const S* s, const char* (*check)(const S*), S& settings, FilterState& state)
{
    API_ARG(&c, s, "settings is NULL");
    if (const char* refusal = check(s)) return fail(&c, PT_ERROR_INVALID_ARGUMENT, refusal);
    S next = *s;
    memset(next._pad, 0, sizeof next._pad);
    if (!state.have || memcmp(&next, &settings, sizeof next) != 0) state.frames = 0;   // a change of settings (a size among them) restarts the history
    settings = next;
    state.have = true;
    return PT_OK;
}

// Grows the grow-only histories of a pass to the float4 counts asked for (want(), pt_memory.hpp); a history that grew starts again.
template <typename... D>
int fl_grow_history(Context& c, FilterState& state, D... demands)
{
    bool grew = false;
    API_HIP(&c, grow(c.stream, &grew, demands...));
    if (grew) state.frames = 0;
    return PT_OK;
}

// The output history of a resolve, in float4 units of an output frame of `no` pixels: two parities of (colour, n), then two of z.
inline size_t fl_output_slots(size_t no) { return 2 * no + (2 * no + 3) / 4; }
// ... and the resolve's arguments for the call that writes the parity after state's (asked for once the history has grown)
inline FlResolveArgs fl_resolve_args(const FilterState& state, float4* base, void* color, const uint32_t render[2], const uint32_t output[2],
                                     const float jitter[2], uint32_t maxFrames, float kernelRadius, float depthThreshold)
{
    const size_t no = (size_t)output[0] * output[1];
    float* zBase = (float*)(base + 2 * no);
    const uint32_t cur = state.parity ^ 1u, prev = state.parity;
    FlResolveArgs a{};
    a.color = color;
    a.hist = base + no * cur; a.histZ = zBase + no * cur; a.prevHist = base + no * prev; a.prevZ = zBase + no * prev;
    a.Rw = render[0]; a.Rh = render[1]; a.Ow = output[0]; a.Oh = output[1]; a.reset = state.frames == 0 ? 1u : 0u;
    a.sx = (float)a.Rw / (float)a.Ow; a.sy = (float)a.Rh / (float)a.Oh; a.jx = jitter[0]; a.jy = jitter[1];
    a.maxFrames = (float)maxFrames; a.r2 = kernelRadius * kernelRadius; a.tau = depthThreshold;
    return a;
}

// the .w of `count` float4 texels of a history, to the host
inline int fl_download_w(Context& c, const float4* src, size_t count, float* host)
{
    std::vector<float4> texels(count);
    API_HIP(&c, hipMemcpy(texels.data(), src, count * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < count; ++k) host[k] = texels[k].w;
    return PT_OK;
}

} // namespace pt
