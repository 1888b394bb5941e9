// pt_upscale.hip -- the library's own temporal upscaler for the super-resolution slot of App::PostProcessGraphics (gfx950).
//
//   k_upscale<STAGED>      one lane per output pixel, 16 x 16 tiles: the nearest render sample, the 3 x 3 dilation of depth and motion, the
//                          kernel-weighted current colour and its clamp box, four validated bilinear taps of the previous output, the blend;
//                          writes Color and the new history parity. STAGED: the tile's render footprint and a one-texel halo (colour, depth,
//                          motion vector: 20 B a texel, at most 19 x 19 of them) go through LDS first, else every tap is a global load. Same
//                          taps, same order, same arithmetic: the same bits.
// Not a port of DLSS or XeSS (closed SDKs the reference tree does not carry): DESIGN.md section 1, "Upscaler", is the arithmetic spec and
// tests/upscaleref.py restates it. Plain fp32 operations, one rounding each (-ffp-contract=off), nothing fused; no library transcendental.
// The two host helpers (the render size of a mode, the Halton jitter of a frame) need no GPU.
#include "pt_internal.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace pt {

constexpr uint32_t kUpMaxSize = 16384u;
constexpr int kUpTile = 16;                                    // a workgroup is one 16 x 16 tile of output pixels
constexpr int kUpSide = 20;                                    // the staged footprint: floor(15 s) + 2 samples and the halo, s <= 1: 19 a side
constexpr float kUpWeightFloor = 0.015625f;                    // 1 / 64: the least weight of the nearest sample
constexpr float kUpDenominatorFloor = 7.62939453125e-06f;      // 2^-17: the guard of the inverse tone map
constexpr float kUpMax16 = 65504.0f;

typedef uint16_t u4v __attribute__((ext_vector_type(4)));     // one fp16 RGBA texel

struct UpArgs {
    const void* radiance; const float* depth; const void* motion; void* color;
    float4* hist; float* histZ;                                // this frame's parity, written
    const float4* prevHist; const float* prevZ;                // the last frame's
    uint32_t Rw, Rh, Ow, Oh, reset;                            // reset: no history
    float sx, sy, jx, jy, maxFrames, r2, tau;                  // s = RenderSize / OutputSize, r2 = KernelRadius^2
};

PT_DEV float up_max0(float x) { return x > 0.0f ? x : 0.0f; }
PT_DEV float up_max3(float r, float g, float b) { const float m = r > g ? r : g; return m > b ? m : b; }
// floor((o + 0.5) s - jitter) clamped into the frame, as a float: the nearest render sample of an output coordinate
PT_DEV float up_nearest(float oc, float s, float j, float last)
{
    const float c = floorf(oc * s - j);
    return c < 0.0f ? 0.0f : (c > last ? last : c);
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_upscale(UpArgs a)
{
    __shared__ u32x2 ldsColour[STAGED ? kUpSide * kUpSide : 1];
    __shared__ u32x2 ldsMotion[STAGED ? kUpSide * kUpSide : 1];
    __shared__ float ldsDepth[STAGED ? kUpSide * kUpSide : 1];
    const int Rw = (int)a.Rw, Rh = (int)a.Rh;
    const int bx = blockIdx.x * kUpTile, by = blockIdx.y * kUpTile;
    int x0s = 0, y0s = 0, sw = 1;
    bool staged = false;
    if (STAGED) {
        // the footprint of the tile: the nearest sample is monotone in the output coordinate, so the first and the last pixel of the tile
        // (inside the frame) bound every lane's; one more texel each way for the 3 x 3 taps, clipped to the frame
        const int lastX = min(bx + kUpTile - 1, (int)a.Ow - 1), lastY = min(by + kUpTile - 1, (int)a.Oh - 1);
        x0s = max((int)up_nearest((float)bx + 0.5f, a.sx, a.jx, (float)(Rw - 1)) - 1, 0);
        y0s = max((int)up_nearest((float)by + 0.5f, a.sy, a.jy, (float)(Rh - 1)) - 1, 0);
        const int x1s = min((int)up_nearest((float)lastX + 0.5f, a.sx, a.jx, (float)(Rw - 1)) + 1, Rw - 1);
        const int y1s = min((int)up_nearest((float)lastY + 0.5f, a.sy, a.jy, (float)(Rh - 1)) + 1, Rh - 1);
        sw = x1s - x0s + 1;
        const int sh = y1s - y0s + 1;
        staged = sw <= kUpSide && sh <= kUpSide;               // always, while RenderSize <= OutputSize; the same in every lane
        if (staged) {
            for (int k = threadIdx.y * kUpTile + threadIdx.x; k < sw * sh; k += kUpTile * kUpTile) {
                const uint32_t j = (uint32_t)(y0s + k / sw) * a.Rw + (uint32_t)(x0s + k % sw);
                ldsColour[k] = gptr<u32x2>(a.radiance)[j]; ldsMotion[k] = gptr<u32x2>(a.motion)[j]; ldsDepth[k] = a.depth[j];
            }
        }
        __syncthreads();
    }
    const uint32_t ox = bx + threadIdx.x, oy = by + threadIdx.y;
    if (ox >= a.Ow || oy >= a.Oh) return;
    // one render texel as a tap sees it, from global memory or from the staged footprint
    auto depthAt = [&](int qx, int qy) { return STAGED && staged ? ldsDepth[(qy - y0s) * sw + (qx - x0s)] : a.depth[(uint32_t)qy * a.Rw + (uint32_t)qx]; };
    auto texelAt = [&](bool motion, int qx, int qy) {
        u32x2 v;
        if (STAGED && staged) v = motion ? ldsMotion[(qy - y0s) * sw + (qx - x0s)] : ldsColour[(qy - y0s) * sw + (qx - x0s)];
        else v = gptr<u32x2>(motion ? a.motion : a.radiance)[(uint32_t)qy * a.Rw + (uint32_t)qx];
        return u4v{ (uint16_t)(v.x & 0xFFFFu), (uint16_t)(v.x >> 16), (uint16_t)(v.y & 0xFFFFu), (uint16_t)(v.y >> 16) };
    };

    // 1: position
    const float oxc = (float)ox + 0.5f, oyc = (float)oy + 0.5f;
    const float ux = oxc * a.sx, uy = oyc * a.sy;
    const int cx = (int)up_nearest(oxc, a.sx, a.jx, (float)(Rw - 1)), cy = (int)up_nearest(oyc, a.sy, a.jy, (float)(Rh - 1));

    // 2 and 3: the dilation and the current colour over the same 3 x 3 taps, row-major
    float best = INFINITY;
    int bqx = 0, bqy = 0;
    bool found = false;
    float wsum = 0.0f, k = 0.0f;
    float acc[3] = { 0.0f, 0.0f, 0.0f }, lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        const int qx = cx + dx, qy = cy + dy;
        if (qx < 0 || qx >= Rw || qy < 0 || qy >= Rh) continue;
        const float zq = depthAt(qx, qy);
        if (isfinite(zq) && zq < best) { best = zq; bqx = qx; bqy = qy; found = true; }
        const float ddx = (((float)qx + 0.5f) + a.jx) - ux, ddy = (((float)qy + 0.5f) + a.jy) - uy;
        const float d2 = ddx * ddx + ddy * ddy;
        float w = up_max0(1.0f - d2 / a.r2);
        w = w * w;
        if (dx == 0 && dy == 0) { w = w < kUpWeightFloor ? kUpWeightFloor : w; k = w; }
        const u4v q = texelAt(false, qx, qy);
        float c[3] = { f16_to_f32(q.x), f16_to_f32(q.y), f16_to_f32(q.z) };
        if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]))) c[0] = c[1] = c[2] = 0.0f;
        const float den = 1.0f + up_max0(up_max3(c[0], c[1], c[2]));
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
    if (found) { const u4v m = texelAt(true, bqx, bqy); mvx = f16_to_f32(m.x); mvy = f16_to_f32(m.y); mvz = f16_to_f32(m.z); }

    // 4: the previous output at (o + 0.5) + mv / s, four bilinear taps, row-major
    const float fx = (oxc + mvx / a.sx) - 0.5f, fy = (oyc + mvy / a.sy) - 0.5f;
    const float hx0 = floorf(fx), hy0 = floorf(fy);
    const float tx = fx - hx0, ty = fy - hy0;
    const float wx[2] = { 1.0f - tx, tx }, wy[2] = { 1.0f - ty, ty };
    const float zp = z + mvz, tol = a.tau * fabsf(zp);
    float hsum = 0.0f, h[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int t = 0; t < 4; ++t) {
        const float xf = hx0 + (float)(t & 1), yf = hy0 + (float)(t >> 1);
        if (a.reset || !(xf >= 0.0f && xf <= (float)(a.Ow - 1u) && yf >= 0.0f && yf <= (float)(a.Oh - 1u))) continue;
        const uint32_t j = (uint32_t)yf * a.Ow + (uint32_t)xf;
        const float zh = a.prevZ[j];
        if (!(found ? fabsf(zh - zp) <= tol : !isfinite(zh))) continue;
        const float w = wx[t & 1] * wy[t >> 1];
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
    float den = 1.0f - up_max0(up_max3(out[0], out[1], out[2]));
    den = den < kUpDenominatorFloor ? kUpDenominatorFloor : den;
    uint16_t c16[3];
    for (int ch = 0; ch < 3; ++ch) {
        const float c = out[ch] / den;
        c16[ch] = f32_to_f16(c > kUpMax16 ? kUpMax16 : (c < -kUpMax16 ? -kUpMax16 : c));
    }
    ((PT_GLOBAL_AS u4v*)a.color)[i] = u4v{ c16[0], c16[1], c16[2], (uint16_t)0x3C00u };
}

// the form pt_upscaler_process takes: the staged one -- 1.17x faster at 1920 x 1080 -> 3840 x 2160, level with the direct one at the two
// 1920 x 1080 outputs ("Upscaler") -- unless PT_UPSCALER_FORM_DIRECT pins the direct one
static bool up_staged(const Context& c) { return !(c.debugFlags & PT_UPSCALER_FORM_DIRECT); }

// the radical inverse of pt_upscaler_jitter: the digits of index in the base from the least significant one, each weighed by 1 / base^k,
// every operation one fp32 rounding
static float up_radical_inverse(uint32_t index, uint32_t base)
{
    const float inv = 1.0f / (float)base;
    float weight = inv, value = 0.0f;
    for (uint32_t i = index; i > 0u; i /= base) {
        const float digit = (float)(i % base) * weight;
        value = value + digit;
        weight = weight * inv;
    }
    return value;
}

} // namespace pt

using namespace pt;

// nullptr when the settings are in range, else the message of the refusal
static const char* up_check_settings(const PtUpscalerSettings* s)
{
    for (int k = 0; k < 2; ++k) if (!(s->RenderSize[k] >= 1u && s->RenderSize[k] <= kUpMaxSize)) return "RenderSize must be 1..16384 on both axes";
    for (int k = 0; k < 2; ++k) if (!(s->OutputSize[k] >= 1u && s->OutputSize[k] <= kUpMaxSize)) return "OutputSize must be 1..16384 on both axes";
    for (int k = 0; k < 2; ++k) if (!(s->RenderSize[k] <= s->OutputSize[k] && s->OutputSize[k] <= 4u * s->RenderSize[k]))
        return "OutputSize must be RenderSize..4 RenderSize on both axes";
    if (!(s->MaxAccumulatedFrames >= 1u && s->MaxAccumulatedFrames <= 255u)) return "MaxAccumulatedFrames must be 1..255";
    if (!(s->KernelRadius >= 0.75f && s->KernelRadius <= 2.0f)) return "KernelRadius must be in [0.75, 2]";
    if (!(s->DepthThreshold > 0.0f && s->DepthThreshold <= 1.0f)) return "DepthThreshold must be in (0, 1]";
    return nullptr;
}

extern "C" {

int pt_upscaler_set_constants(PtContext* ctx, const PtUpscalerSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, s, "settings is NULL");
    if (const char* refusal = up_check_settings(s)) return fail(&c, PT_ERROR_INVALID_ARGUMENT, refusal);
    PtUpscalerSettings next = *s;
    memset(next._pad, 0, sizeof next._pad);
    if (!c.haveUp || memcmp(&next, &c.up, sizeof next) != 0) c.upFrames = 0;      // a change of settings (a size among them) restarts the history
    c.up = next;
    c.haveUp = true;
    return PT_OK;
}

int pt_upscaler_reset_history(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.upFrames = 0;
    return PT_OK;
}

int pt_upscaler_process(PtContext* ctx, const struct PtUpscalerTextures* t, const float jitter[2])
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, t, "textures is NULL");
    API_ARG(&c, jitter, "jitter is NULL");
    if (!c.haveUp) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "call pt_upscaler_set_constants first");
    if (c.sharding.RankCount > 1u)
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "the upscaler needs the whole frame: the context is sharded (run it on the gathered textures of an unsharded context)");
    const struct { const char* name; const void* p; uint32_t texel; } bound[4] = {
        { "Radiance", t->Radiance, 8 }, { "LinearDepth", t->LinearDepth, 4 }, { "MotionVector", t->MotionVector, 8 }, { "Color", t->Color, 8 } };
    for (const auto& b : bound) if (!b.p) return fail(&c, PT_ERROR_INVALID_ARGUMENT, std::string(b.name) + " is NULL");
    for (const auto& b : bound) if ((uintptr_t)b.p & (b.texel - 1u))
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, std::string(b.name) + " is not aligned to its texel (" + std::to_string(b.texel) + " bytes)");
    for (int k = 0; k < 2; ++k) if (!(std::isfinite(jitter[k]) && jitter[k] >= -0.5f && jitter[k] <= 0.5f))
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "jitter must be finite and in [-0.5, 0.5] on both axes");
    const PtUpscalerSettings& s = c.up;
    const size_t n = (size_t)s.OutputSize[0] * s.OutputSize[1];
    const size_t slots = 2 * n + (2 * n + 3) / 4;              // float4 units: two parities of (colour, n), then two of z
    API_HIP(&c, hipSetDevice(c.device));
    if (c.upHistory.capacity() < slots) {                      // transactional: the old history stays until the new one exists
        DeviceBuffer<float4> fresh;
        API_HIP(&c, fresh.reserve(slots));
        API_HIP(&c, hipStreamSynchronize(c.stream));           // an earlier call may still use the old one
        c.upHistory = std::move(fresh);
        c.upFrames = 0;
    }
    float4* base = c.upHistory.data();
    float* zBase = (float*)(base + 2 * n);
    const uint32_t cur = c.upParity ^ 1u, prev = c.upParity;
    UpArgs a{};
    a.radiance = t->Radiance; a.depth = (const float*)t->LinearDepth; a.motion = t->MotionVector; a.color = t->Color;
    a.hist = base + n * cur; a.histZ = zBase + n * cur; a.prevHist = base + n * prev; a.prevZ = zBase + n * prev;
    a.Rw = s.RenderSize[0]; a.Rh = s.RenderSize[1]; a.Ow = s.OutputSize[0]; a.Oh = s.OutputSize[1]; a.reset = c.upFrames == 0 ? 1u : 0u;
    a.sx = (float)a.Rw / (float)a.Ow; a.sy = (float)a.Rh / (float)a.Oh; a.jx = jitter[0]; a.jy = jitter[1];
    a.maxFrames = (float)s.MaxAccumulatedFrames; a.r2 = s.KernelRadius * s.KernelRadius; a.tau = s.DepthThreshold;
    const dim3 grid((a.Ow + kUpTile - 1) / kUpTile, (a.Oh + kUpTile - 1) / kUpTile), block(kUpTile, kUpTile);
    if (up_staged(c)) k_upscale<true><<<grid, block, 0, c.stream>>>(a);
    else k_upscale<false><<<grid, block, 0, c.stream>>>(a);
    API_HIP(&c, hipGetLastError());
    c.upParity = cur;
    c.upFrames += 1;
    c.upSize[0] = a.Ow; c.upSize[1] = a.Oh;
    return PT_OK;
}

int pt_upscaler_download_history(PtContext* ctx, float* host_length, uint64_t capacity_pixels, uint32_t* out_w, uint32_t* out_h)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_w && out_h && (host_length || capacity_pixels == 0), "out_w / out_h / host_length is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    const bool have = c.upFrames != 0;                         // after a reset there is no history to show: 0 x 0
    *out_w = have ? c.upSize[0] : 0u; *out_h = have ? c.upSize[1] : 0u;
    const size_t n = (size_t)*out_w * *out_h;
    const size_t count = (size_t)std::min<uint64_t>(capacity_pixels, n);
    if (!count) return PT_OK;
    std::vector<float4> texels(count);
    API_HIP(&c, hipMemcpy(texels.data(), c.upHistory.data() + n * c.upParity, count * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < count; ++k) host_length[k] = texels[k].w;
    return PT_OK;
}

int pt_upscaler_render_size(uint32_t mode, const uint32_t output[2], uint32_t render_out[2])
{
    if (!output || !render_out) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "output / render_out is NULL");
    if (mode > PT_SUPER_RESOLUTION_ULTRA_PERFORMANCE) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "mode must be a PtSuperResolutionMode value");
    for (int k = 0; k < 2; ++k) if (!(output[k] >= 1u && output[k] <= kUpMaxSize)) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "output must be 1..16384 on both axes");
    if (mode == PT_SUPER_RESOLUTION_AUTO) {                    // by the pixel count of the output (App.cpp:1427-1440)
        const uint64_t pixels = (uint64_t)output[0] * output[1];
        mode = pixels <= 1280u * 800u ? PT_SUPER_RESOLUTION_NATIVE : pixels <= 1920u * 1200u ? PT_SUPER_RESOLUTION_QUALITY
             : pixels <= 2560u * 1600u ? PT_SUPER_RESOLUTION_BALANCED : pixels <= 3840u * 2400u ? PT_SUPER_RESOLUTION_PERFORMANCE
             : PT_SUPER_RESOLUTION_ULTRA_PERFORMANCE;
    }
    static const uint32_t ratio10[6] = { 0u, 10u, 15u, 17u, 20u, 30u };    // ten times the ratio per axis
    const uint32_t r10 = ratio10[mode];
    for (int k = 0; k < 2; ++k) render_out[k] = std::max(1u, (output[k] * 10u + r10 / 2u) / r10);
    return PT_OK;
}

int pt_upscaler_jitter(uint64_t frame_index, const uint32_t render[2], const uint32_t output[2], float jitter_out[2])
{
    if (!render || !output || !jitter_out) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "render / output / jitter_out is NULL");
    for (int k = 0; k < 2; ++k) if (!(render[k] >= 1u && render[k] <= kUpMaxSize && output[k] >= 1u && output[k] <= kUpMaxSize))
        return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "render and output must be 1..16384 on both axes");
    // the length of the sequence: ceil(8 (ow / rw) (oh / rh)) in fp32, as App.cpp:661
    const float rx = (float)output[0] / (float)render[0], ry = (float)output[1] / (float)render[1];
    const float scaled = 8.0f * rx;
    const uint32_t count = (uint32_t)ceilf(scaled * ry);
    const uint32_t index = (uint32_t)(frame_index % count) + 1u;
    jitter_out[0] = up_radical_inverse(index, 2u) - 0.5f;
    jitter_out[1] = up_radical_inverse(index, 3u) - 0.5f;
    return PT_OK;
}

} // extern "C"
