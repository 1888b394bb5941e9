// pt_reconstruct.hip -- the library's own denoising upscaler for the ray-reconstruction slot of App::PostProcessGraphics (gfx950).
//
//   k_rr_temporal          stage 1, render size: Radiance divided by the floored albedo sum (the signal), reprojection through MotionVector,
//                          four validated bilinear taps of the history (same surface by depth or by plane distance, so that the jitter
//                          does not cost a slanted surface its history), the luminance reset (a history the input contradicts is
//                          dropped), accumulation of the signal and its two luminance moments; writes the new history, the frame's
//                          guide record and the albedo the resolve multiplies back
//   k_rr_variance          stage 2: the variance of the luminance, from the moments (length >= 4) or from the 7 x 7 neighbourhood
//   k_rr_atrous<STAGED>    stage 3: one 5 x 5 edge-stopping a-trous iteration at step 1, 2, 4, ...; STAGED: the 16 x 16 tile and its halo go
//                          through LDS first, else every tap is a global load. Same taps, same order, same arithmetic: the same bits.
//   k_rr_resolve           stage 4, output size: the upscaler's steps 1-6 (fl_resolve, pt_filter.hpp; k_upscale runs the same function)
//                          over taps whose colour is the filtered signal x the tap's own albedo, on this pass's own output history;
//                          writes Color
// One signal (Radiance, direct + indirect) where pt_denoise.hip carries two; no pack and no compose pass. Stages 1-3 share their small
// arithmetic and the set-up of the history taps with the denoiser (pt_filter.hpp); the bodies stay this pass's own. Not a port of DLSS Ray
// Reconstruction (a closed SDK the reference tree does not carry): DESIGN.md section 1, "Ray reconstruction", is the arithmetic spec and
// tests/reconstructref.py restates it. Plain fp32 operations, one rounding each (-ffp-contract=off); the only fused operations are those
// of dot() / ml_luminance(); no library transcendental. SpecularHitDistance is not read: reprojection follows the surface motion only
// (no virtual motion), as in the denoiser.
//
// History, context-owned and grow-only. Per render pixel 160 B: two parities of (signal, length), of the two moments and of the two
// guide records (112 B), the albedo (16 B), the a-trous ping-pong of (signal, variance) (32 B), the later of which holds the filtered
// signal. Per output pixel 40 B: two parities of (tone-mapped colour, n) and of the depth.
#include "pt_filter.hpp"

namespace pt {

constexpr int kRrTile = kFlTile;
constexpr uint32_t kRrStagedBytes = 48u;                       // a staged record: three float4 (48 kB at step 4: within what a launch gets unasked)
constexpr float kRrAlbedoFloor = 0.015625f;                    // 1 / 64: the least albedo sum a signal is divided by
constexpr float kRrAlbedoCeiling = 131008.0f;                  // 2 x 65504: the sum of two finite fp16 values is below it
constexpr float kRrResetRatio = 16.0f;                         // the luminance reset of stage 1: four stops against the history
// per-render-pixel slots of Context::rrHistory, in float4 units of one frame each; behind them two float2 arrays (the moments' parities)
enum { RR_HIST = 0, RR_G0 = 2, RR_G1 = 4, RR_ALBEDO = 6, RR_WORK = 7, RR_SLOTS4 = 9, RR_SLOTS = 10 };

struct RrSettings { float maxFrames, depthThreshold, normalCosine, sigma, roughnessFraction; };

struct RrTemporalArgs {
    const void *radiance, *diffuseAlbedo, *specularAlbedo, *normalRoughness, *motion; const float4* position; const float* depth;
    float4 *hist, *g0, *g1, *albedo, *out; float2* moments;                         // this frame's, written (out: missed pixels only)
    const float4 *prevHist, *prevG0, *prevG1; const float2* prevMoments;           // the last frame's
    uint32_t W, H, reset;                                      // reset: no history
    RrSettings s;
};

struct RrVarianceArgs {
    const float4 *hist, *g0, *g1, *albedo; const float2* moments; float4* out;     // out: (signal, variance), the first a-trous input
    uint32_t W, H;
    RrSettings s;
};

struct RrAtrousArgs {
    const float4 *g0, *g1, *in; float4* out;
    uint32_t W, H, step;
    RrSettings s;
};

struct RrResolveArgs { const float4 *filtered, *albedo; const float* depth; const void* motion; FlResolveArgs r; };

PT_DEV v3 rr_rgb16(const void* tex, uint32_t i) { return fl_rgb16(gptr<h4v>(tex)[i]); }
// one channel of the albedo sum: floored (a NaN reads as the floor), then kept finite
PT_DEV float rr_albedo(float d, float s)
{
    float a = d + s;
    a = a > kRrAlbedoFloor ? a : kRrAlbedoFloor;
    return a < kRrAlbedoCeiling ? a : kRrAlbedoCeiling;
}
// the signal's luminance of a neighbour of stage 1's pixel, this frame's: the same operations as the pixel's own
PT_DEV float rr_signal_luminance(const RrTemporalArgs& a, uint32_t j)
{
    const v3 rad = fl_guard(rr_rgb16(a.radiance, j)), Ad = rr_rgb16(a.diffuseAlbedo, j), As = rr_rgb16(a.specularAlbedo, j);
    return fl_lum(float4{ rad.x / rr_albedo(Ad.x, As.x), rad.y / rr_albedo(Ad.y, As.y), rad.z / rr_albedo(Ad.z, As.z), 0.0f });
}

__global__ __launch_bounds__(256) void k_rr_temporal(RrTemporalArgs a)
{
    const uint32_t x = blockIdx.x * kRrTile + threadIdx.x, y = blockIdx.y * kRrTile + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const uint32_t i = y * a.W + x;
    const float z = a.depth[i];
    const v3 rad = fl_guard(rr_rgb16(a.radiance, i));
    const float4 zero4{ 0.0f, 0.0f, 0.0f, 0.0f };
    if (!isfinite(z)) {                                        // the G-buffer missed: the guarded Radiance goes to the resolve, length 0, never a tap
        a.g0[i] = float4{ 0.0f, 0.0f, 0.0f, z }; a.g1[i] = zero4;
        a.hist[i] = zero4; a.moments[i] = float2{ 0.0f, 0.0f };
        a.albedo[i] = float4{ 1.0f, 1.0f, 1.0f, 0.0f };
        a.out[i] = float4{ rad.x, rad.y, rad.z, 0.0f };
        return;
    }
    const s4v nr = gptr<s4v>(a.normalRoughness)[i];
    const v3 N = V3(snorm16_to_f32(nr.x), snorm16_to_f32(nr.y), snorm16_to_f32(nr.z));
    const float r = snorm16_to_f32(nr.w);
    const float4 P = a.position[i];
    const h4v mvh = gptr<h4v>(a.motion)[i];
    const float mvx = f16_to_f32(mvh.x), mvy = f16_to_f32(mvh.y), mvz = f16_to_f32(mvh.z);
    const v3 Ad = rr_rgb16(a.diffuseAlbedo, i), As = rr_rgb16(a.specularAlbedo, i);
    const v3 A = V3(rr_albedo(Ad.x, As.x), rr_albedo(Ad.y, As.y), rr_albedo(Ad.z, As.z));
    const float4 cur{ rad.x / A.x, rad.y / A.y, rad.z / A.z, 0.0f };
    const float L = fl_lum(cur);

    // the cap of the history: the specular one on specular-dominated surfaces
    const float cap = ml_luminance(As) > ml_luminance(Ad) ? fl_specular_cap(a.s.maxFrames, r, mvx, mvy) : a.s.maxFrames;

    // the previous position and the four taps around it, row-major
    const FlTaps taps((((float)x + 0.5f) + mvx) - 0.5f, (((float)y + 0.5f) + mvy) - 0.5f, a.W, a.H);
    const float zp = z + mvz, zTol = a.s.depthThreshold * fabsf(zp), planeScale = a.s.depthThreshold * fabsf(z);
    float wsum = 0.0f, h[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    for (int t = 0; t < 4; ++t) {
        if (a.reset || !taps.inside(t)) continue;
        const uint32_t j = taps.index(t);
        const float4 g0 = a.prevG0[j], g1 = a.prevG1[j];
        const float4 q = a.prevHist[j];
        const bool sameSurface = fabsf(g0.w - zp) <= zTol || fabsf(dot(N, V3(g0.x, g0.y, g0.z) - V3(P.x, P.y, P.z))) <= planeScale;
        const bool ok = sameSurface && dot(N, V3(g1.x, g1.y, g1.z)) >= a.s.normalCosine && q.w > 0.0f
                     && fabsf(r - g1.w) <= a.s.roughnessFraction * (r > g1.w ? r : g1.w);
        if (!ok) continue;
        const float2 m = a.prevMoments[j];
        const float w = taps.weight(t);
        wsum = wsum + w;
        h[0] = h[0] + w * q.x; h[1] = h[1] + w * q.y; h[2] = h[2] + w * q.z;
        h[3] = h[3] + w * m.x; h[4] = h[4] + w * m.y; h[5] = h[5] + w * q.w;
    }
    float4 out{ cur.x, cur.y, cur.z, 1.0f };                   // disoccluded: the input, length 1
    float2 mom{ L, L * L };
    float feature = 0.0f;
    if (wsum > 0.0f) {
        for (int k = 0; k < 6; ++k) h[k] = h[k] / wsum;
        // the luminance reset: sixteen times darker than the history less its deviation (a history of sparse outliers has sd >= mean and
        // never asks), or sixteen times brighter than the history plus its deviation with one of the eight neighbours of this frame at
        // least half as bright (a lone outlier keeps its history and is averaged in)
        const float sd = sqrtf(fl_max0(h[4] - h[3] * h[3]));
        if (L * kRrResetRatio < h[3] - sd) feature = 1.0f;
        else if (L > kRrResetRatio * (h[3] + sd)) {
            for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
                const int xq = (int)x + dx, yq = (int)y + dy;
                if ((dx == 0 && dy == 0) || xq < 0 || xq >= (int)a.W || yq < 0 || yq >= (int)a.H) continue;
                const uint32_t j = (uint32_t)yq * a.W + (uint32_t)xq;
                if (isfinite(a.depth[j]) && rr_signal_luminance(a, j) >= 0.5f * L) feature = 1.0f;
            }
        }
    }
    if (wsum > 0.0f && feature == 0.0f) {
        const float n1 = h[5] + 1.0f;
        const float n = n1 < cap ? n1 : cap;
        const float inv = 1.0f / n;
        out = float4{ fl_blend(h[0], cur.x, inv), fl_blend(h[1], cur.y, inv), fl_blend(h[2], cur.z, inv), n };
        mom = float2{ fl_blend(h[3], mom.x, inv), fl_blend(h[4], mom.y, inv) };
    }
    a.g0[i] = float4{ P.x, P.y, P.z, z }; a.g1[i] = float4{ N.x, N.y, N.z, r };
    a.hist[i] = out; a.moments[i] = mom;
    a.albedo[i] = float4{ A.x, A.y, A.z, feature };             // w: stage 2 gives a pixel the reset took a variance of 0
}

__global__ __launch_bounds__(256) void k_rr_variance(RrVarianceArgs a)
{
    const int x = blockIdx.x * kRrTile + threadIdx.x, y = blockIdx.y * kRrTile + threadIdx.y;
    if (x >= (int)a.W || y >= (int)a.H) return;
    const uint32_t i = (uint32_t)y * a.W + (uint32_t)x;
    const float4 g0 = a.g0[i];
    if (!isfinite(g0.w)) return;                               // stage 1 wrote the texel the resolve reads
    const float2 m = a.moments[i];
    const float4 c = a.hist[i];
    float v = fl_max0(m.y - m.x * m.x);
    if (a.albedo[i].w != 0.0f) v = 0.0f;                       // the luminance reset took its history: stage 3 does not spread it
    else if (c.w < 4.0f) {                                          // a short history: the moments of the 7 x 7 neighbourhood on the same surface
        const float4 g1 = a.g1[i];
        const v3 Pp = V3(g0.x, g0.y, g0.z), Np = V3(g1.x, g1.y, g1.z);
        const float planeScale = a.s.depthThreshold * fabsf(g0.w);
        float s1 = 0.0f, s2 = 0.0f, count = 0.0f;
        for (int dy = -3; dy <= 3; ++dy) for (int dx = -3; dx <= 3; ++dx) {
            const int xq = x + dx, yq = y + dy;
            if (xq < 0 || xq >= (int)a.W || yq < 0 || yq >= (int)a.H) continue;
            const uint32_t j = (uint32_t)yq * a.W + (uint32_t)xq;
            if (j != i) {
                const float4 q0 = a.g0[j];
                if (!isfinite(q0.w)) continue;
                const float4 q1 = a.g1[j];
                if (!(fl_wg(Np, Pp, V3(q0.x, q0.y, q0.z), planeScale) > 0.0f && fl_wn(Np, V3(q1.x, q1.y, q1.z), a.s.normalCosine) > 0.0f)) continue;
            }
            const float Lq = fl_lum(a.hist[j]);
            s1 = s1 + Lq; s2 = s2 + Lq * Lq; count = count + 1.0f;
        }
        const float m1 = s1 / count, m2 = s2 / count;
        v = fl_max0(m2 - m1 * m1);
    }
    a.out[i] = float4{ c.x, c.y, c.z, v };
}

// The record of one pixel as a tap sees it, from global memory or from the staged tile. c = (signal, variance).
struct RrTap { float4 g0, g1, c; };

template <bool STAGED>
__global__ __launch_bounds__(256) void k_rr_atrous(RrAtrousArgs a)
{
    extern __shared__ float4 rr_lds[];                         // STAGED: g0 | g1 | c of side x side pixels
    const int step = (int)a.step, W = (int)a.W, H = (int)a.H;
    const int bx = blockIdx.x * kRrTile, by = blockIdx.y * kRrTile;
    const int halo = 2 * step, side = kRrTile + 2 * halo, cells = side * side;
    if (STAGED) {
        for (int k = threadIdx.y * kRrTile + threadIdx.x; k < cells; k += kRrTile * kRrTile) {
            const int xq = bx - halo + k % side, yq = by - halo + k / side;
            if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;    // never read: every tap tests its coordinates first
            const uint32_t j = (uint32_t)yq * a.W + (uint32_t)xq;
            rr_lds[k] = a.g0[j]; rr_lds[cells + k] = a.g1[j]; rr_lds[2 * cells + k] = a.in[j];
        }
        __syncthreads();
    }
    const int x = bx + threadIdx.x, y = by + threadIdx.y;
    if (x >= W || y >= H) return;
    auto fetch = [&](int xq, int yq) {
        RrTap t;
        if (STAGED) {
            const int k = (yq - by + halo) * side + (xq - bx + halo);
            t.g0 = rr_lds[k]; t.g1 = rr_lds[cells + k]; t.c = rr_lds[2 * cells + k];
        } else {
            const uint32_t j = (uint32_t)yq * a.W + (uint32_t)xq;
            t.g0 = a.g0[j]; t.g1 = a.g1[j]; t.c = a.in[j];
        }
        return t;
    };
    const uint32_t i = (uint32_t)y * a.W + (uint32_t)x;
    const RrTap p = fetch(x, y);
    if (!isfinite(p.g0.w)) return;                             // missed: stage 1 wrote the texel the resolve reads
    // the 3 x 3 binomial blur of the variance over the hit pixels of the frame
    float b = 0.0f, bw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        const int xq = x + dx, yq = y + dy;
        if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
        const RrTap q = fetch(xq, yq);
        if (!isfinite(q.g0.w)) continue;
        const float k = fl_blur3(dx, dy);
        b = b + k * q.c.w; bw = bw + k;
    }
    const float sd = a.s.sigma * sqrtf(b / bw) + 1e-4f;
    const v3 Pp = V3(p.g0.x, p.g0.y, p.g0.z), Np = V3(p.g1.x, p.g1.y, p.g1.z);
    const float rp = p.g1.w, planeScale = a.s.depthThreshold * fabsf(p.g0.w);
    const float Lp = fl_lum(p.c);
    float s[3] = { 0.0f, 0.0f, 0.0f }, ws = 0.0f, v = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) for (int dx = -2; dx <= 2; ++dx) {
        const int xq = x + dx * step, yq = y + dy * step;
        float w;
        RrTap q;
        if (dx == 0 && dy == 0) { q = p; w = 0.140625f; }     // the centre always weighs h(0)^2
        else {
            if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
            q = fetch(xq, yq);
            if (!isfinite(q.g0.w)) continue;
            const float base = ((fl_h5(dy) * fl_h5(dx)) * fl_wg(Np, Pp, V3(q.g0.x, q.g0.y, q.g0.z), planeScale)) * fl_wn(Np, V3(q.g1.x, q.g1.y, q.g1.z), a.s.normalCosine);
            const float wr = fl_wr(rp, q.g1.w, a.s.roughnessFraction);
            w = (base * fl_max0(1.0f - fabsf(fl_lum(q.c) - Lp) / sd)) * wr;
        }
        if (w > 0.0f) {
            ws = ws + w; v = v + (w * w) * q.c.w;
            s[0] = s[0] + w * q.c.x; s[1] = s[1] + w * q.c.y; s[2] = s[2] + w * q.c.z;
        }
    }
    a.out[i] = float4{ s[0] / ws, s[1] / ws, s[2] / ws, v / (ws * ws) };
}

// A render texel as a tap of fl_resolve sees it: the filtered signal remodulated with the tap's own albedo (1 for a missed tap).
struct RrSource {
    const RrResolveArgs& a;
    PT_DEV uint32_t at(int qx, int qy) const { return (uint32_t)qy * a.r.Rw + (uint32_t)qx; }
    PT_DEV float depth(uint32_t j) const { return a.depth[j]; }
    PT_DEV h4v motion(uint32_t j) const { return gptr<h4v>(a.motion)[j]; }
    PT_DEV v3 colour(uint32_t j) const { const float4 f = a.filtered[j], A = a.albedo[j]; return V3(f.x * A.x, f.y * A.y, f.z * A.z); }
};

__global__ __launch_bounds__(256) void k_rr_resolve(RrResolveArgs a)
{
    const uint32_t ox = blockIdx.x * kRrTile + threadIdx.x, oy = blockIdx.y * kRrTile + threadIdx.y;
    if (ox >= a.r.Ow || oy >= a.r.Oh) return;
    fl_resolve(a.r, ox, oy, RrSource{ a });
}

// the form pt_reconstruction_process takes for an a-trous step: the staged one wherever the tile's halo fits (steps 1, 2 and 4; DESIGN.md
// section 4, "Ray reconstruction") unless PT_RECONSTRUCTION_FORM_DIRECT pins the direct one
static bool rr_staged(const Context& c, uint32_t step)
{
    return step <= kFlStagedMaxStep && !(c.debugFlags & PT_RECONSTRUCTION_FORM_DIRECT);
}

// which of the two work buffers holds the filtered signal after `iterations` a-trous launches: stage 2 writes the second one, iteration k
// reads the one iteration k - 1 wrote and writes the other
static uint32_t rr_final_work(uint32_t iterations) { return iterations == 0u ? 1u : ((iterations - 1u) & 1u); }

} // namespace pt

using namespace pt;

// nullptr when the settings are in range, else the message of the refusal
static const char* rr_check_settings(const PtReconstructionSettings* s)
{
    if (const char* refusal = fl_check_sizes(s->RenderSize, s->OutputSize)) return refusal;
    if (!(s->MaxAccumulatedFrames >= 1u && s->MaxAccumulatedFrames <= 255u)) return "MaxAccumulatedFrames must be 1..255";
    if (!(s->MaxOutputFrames >= 1u && s->MaxOutputFrames <= 255u)) return "MaxOutputFrames must be 1..255";
    if (s->AtrousIterations > 8u) return "AtrousIterations must be 0..8";
    if (!(s->DepthThreshold > 0.0f && s->DepthThreshold <= 1.0f)) return "DepthThreshold must be in (0, 1]";
    if (!(s->NormalCosine >= 0.0f && s->NormalCosine < 1.0f)) return "NormalCosine must be in [0, 1)";
    if (!(s->LuminanceSigma > 0.0f && std::isfinite(s->LuminanceSigma))) return "LuminanceSigma must be positive and finite";
    if (!(s->RoughnessFraction > 0.0f && std::isfinite(s->RoughnessFraction))) return "RoughnessFraction must be positive and finite";
    if (!(s->KernelRadius >= 0.75f && s->KernelRadius <= 2.0f)) return "KernelRadius must be in [0.75, 2]";
    return nullptr;
}

extern "C" {

int pt_reconstruction_set_constants(PtContext* ctx, const PtReconstructionSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    return fl_set_constants(ctx->c, s, rr_check_settings, ctx->c.rr, ctx->c.rrState);
}

int pt_reconstruction_reset_history(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.rrState.frames = 0;
    return PT_OK;
}

int pt_reconstruction_process(PtContext* ctx, const struct PtReconstructionTextures* t, const float jitter[2])
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, t, "textures is NULL");
    API_ARG(&c, jitter, "jitter is NULL");
    if (!c.rrState.have) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "call pt_reconstruction_set_constants first");
    if (c.sharding.RankCount > 1u)
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "the reconstruction needs the whole frame: the context is sharded (run it on the gathered textures of an unsharded context)");
    const PtReconstructionSettings& s = c.rr;
    const uint32_t W = s.RenderSize[0], H = s.RenderSize[1], Ow = s.OutputSize[0], Oh = s.OutputSize[1];
    const size_t n = (size_t)W * H, no = (size_t)Ow * Oh;
    const BoundTexture bound[8] = {
        { "Radiance", t->Radiance, 8 }, { "DiffuseAlbedo", t->DiffuseAlbedo, 8 }, { "SpecularAlbedo", t->SpecularAlbedo, 8 },
        { "NormalRoughness", t->NormalRoughness, 8 }, { "Position", t->Position, 16 }, { "LinearDepth", t->LinearDepth, 4 },
        { "MotionVector", t->MotionVector, 8 }, { "Color", t->Color, 8 } };
    if (int refusal = fl_check_bound(c, bound)) return refusal;
    for (int k = 0; k < 7; ++k) {                              // Color is written while the inputs are still read
        const uintptr_t in0 = (uintptr_t)bound[k].p, in1 = in0 + n * bound[k].texel, out0 = (uintptr_t)t->Color, out1 = out0 + no * 8u;
        if (in0 < out1 && out0 < in1) return fail(&c, PT_ERROR_INVALID_ARGUMENT, std::string("Color overlaps ") + bound[k].name);
    }
    if (int refusal = fl_check_jitter(c, jitter)) return refusal;
    API_HIP(&c, hipSetDevice(c.device));
    if (int e = fl_grow_history(c, c.rrState, want(c.rrHistory, n * RR_SLOTS), want(c.rrOutput, fl_output_slots(no)))) return e;
    float4* base = c.rrHistory.data();
    float2* halves = (float2*)(base + n * RR_SLOTS4);
    const uint32_t cur = c.rrState.parity ^ 1u, prev = c.rrState.parity;
    auto slot = [&](int first, uint32_t parity) { return base + n * (first + parity); };
    float4* filtered = slot(RR_WORK, rr_final_work(s.AtrousIterations));

    const RrSettings rs{ (float)s.MaxAccumulatedFrames, s.DepthThreshold, s.NormalCosine, s.LuminanceSigma, s.RoughnessFraction };
    const dim3 grid((W + kRrTile - 1) / kRrTile, (H + kRrTile - 1) / kRrTile), block(kRrTile, kRrTile);
    RrTemporalArgs ta{};
    ta.radiance = t->Radiance; ta.diffuseAlbedo = t->DiffuseAlbedo; ta.specularAlbedo = t->SpecularAlbedo; ta.normalRoughness = t->NormalRoughness;
    ta.motion = t->MotionVector; ta.position = (const float4*)t->Position; ta.depth = (const float*)t->LinearDepth;
    ta.hist = slot(RR_HIST, cur); ta.g0 = slot(RR_G0, cur); ta.g1 = slot(RR_G1, cur); ta.albedo = slot(RR_ALBEDO, 0); ta.out = filtered;
    ta.moments = halves + n * cur;
    ta.prevHist = slot(RR_HIST, prev); ta.prevG0 = slot(RR_G0, prev); ta.prevG1 = slot(RR_G1, prev); ta.prevMoments = halves + n * prev;
    ta.W = W; ta.H = H; ta.reset = c.rrState.frames == 0 ? 1u : 0u; ta.s = rs;
    k_rr_temporal<<<grid, block, 0, c.stream>>>(ta);
    const RrVarianceArgs va{ ta.hist, ta.g0, ta.g1, ta.albedo, ta.moments, slot(RR_WORK, 1), W, H, rs };
    k_rr_variance<<<grid, block, 0, c.stream>>>(va);
    RrAtrousArgs aa{};
    aa.g0 = ta.g0; aa.g1 = ta.g1; aa.in = va.out; aa.W = W; aa.H = H; aa.s = rs;
    for (uint32_t k = 0; k < s.AtrousIterations; ++k) {
        aa.step = 1u << k; aa.out = slot(RR_WORK, k & 1u);
        if (rr_staged(c, aa.step)) {
            const int side = kRrTile + 4 * (int)aa.step;
            k_rr_atrous<true><<<grid, block, (size_t)side * side * kRrStagedBytes, c.stream>>>(aa);   // 19.2, 27.6 and 49.2 kB at step 1, 2 and 4
        } else k_rr_atrous<false><<<grid, block, 0, c.stream>>>(aa);
        aa.in = aa.out;
    }
    RrResolveArgs ra{};
    ra.filtered = filtered; ra.albedo = ta.albedo; ra.depth = ta.depth; ra.motion = t->MotionVector;
    ra.r = fl_resolve_args(c.rrState, c.rrOutput.data(), t->Color, s.RenderSize, s.OutputSize, jitter, s.MaxOutputFrames, s.KernelRadius, s.DepthThreshold);
    const dim3 ogrid((Ow + kRrTile - 1) / kRrTile, (Oh + kRrTile - 1) / kRrTile);
    k_rr_resolve<<<ogrid, block, 0, c.stream>>>(ra);
    API_HIP(&c, hipGetLastError());
    c.rrState.advance(W, H, Ow, Oh);
    c.rrFinal = rr_final_work(s.AtrousIterations);
    return PT_OK;
}

int pt_reconstruction_download_history(PtContext* ctx, float* host_length, float* host_filtered, uint64_t capacity_render_pixels,
                                       float* host_n, uint64_t capacity_output_pixels, uint32_t render_out[2], uint32_t output_out[2])
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, render_out && output_out, "render_out / output_out is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    for (int k = 0; k < 2; ++k) { render_out[k] = c.rrState.shown(k); output_out[k] = c.rrState.shown(2 + k); }
    const size_t n = (size_t)render_out[0] * render_out[1], no = (size_t)output_out[0] * output_out[1];
    const size_t count = (size_t)std::min<uint64_t>(capacity_render_pixels, n), countOut = (size_t)std::min<uint64_t>(capacity_output_pixels, no);
    if (count && host_length)
        if (int e = fl_download_w(c, c.rrHistory.data() + n * (RR_HIST + c.rrState.parity), count, host_length)) return e;
    if (count && host_filtered)
        API_HIP(&c, hipMemcpy(host_filtered, c.rrHistory.data() + n * (RR_WORK + c.rrFinal), count * sizeof(float4), hipMemcpyDeviceToHost));
    if (countOut && host_n)
        if (int e = fl_download_w(c, c.rrOutput.data() + no * c.rrState.parity, countOut, host_n)) return e;
    return PT_OK;
}

} // extern "C"
