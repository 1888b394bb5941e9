// pt_denoise.hip -- the library's own denoiser for the ReLAX slot of the NRD composition pass (gfx950).
//
//   k_dn_temporal          stage 1: reprojection through MotionVector, four validated bilinear taps of the history, accumulation of colour,
//                          hit distance and the two luminance moments; writes the new history and the frame's guide record
//   k_dn_variance          stage 2: the variance of the luminance, from the moments (length >= 4) or from the 7 x 7 neighbourhood
//   k_dn_atrous<STAGED>    stage 3: one 5 x 5 edge-stopping a-trous iteration at step 1, 2, 4, ...; STAGED: the 16 x 16 tile and its halo go
//                          through LDS first, else every tap is a global load. Same taps, same order, same arithmetic: the same bits.
// Not a port of NRD's ReLAX (its source is not in the reference tree): DESIGN.md section 1, "Denoiser", is the arithmetic spec and
// tests/denoiseref.py restates it. Plain fp32 operations, one rounding each (-ffp-contract=off); the only fused operations are those
// of dot() / ml_luminance(); no library transcendental. The small arithmetic, the set-up of the history taps and the host plumbing are
// pt_filter.hpp's, shared with the upscaler and the reconstruction; the kernels' bodies (two channels, a float2 variance) are this pass's own.
#include "pt_filter.hpp"

namespace pt {

constexpr uint16_t kDnNaN16 = 0x7E00u;
constexpr int kDnTile = kFlTile;
constexpr uint32_t kDnStagedBytes = 72u;                       // a staged record: four float4 and the float2 variance
// per-pixel slots of Context::dnHistory, in float4 units of one frame each: the ping-pong pairs first
enum { DN_HIST_D = 0, DN_HIST_S = 2, DN_MOMENTS = 4, DN_G0 = 6, DN_G1 = 8, DN_WORK_D = 10, DN_WORK_S = 12, DN_PAIRS = 14, DN_SLOTS = 17 };
// behind them five float2 arrays (half a slot each): the lengths of both parities, the variance, the two work variances
enum { DN_LEN = 0, DN_VAR = 2, DN_WORK_VAR = 3 };

struct DnSettings { float maxFrames, depthThreshold, normalCosine, sigmaD, sigmaS, roughnessFraction; };

struct DnTemporalArgs {
    const float4* position; const float* depth; const void* normalRoughness; const void* motion;
    const void* noisyD; const void* noisyS; void* outD; void* outS;
    float4 *histD, *histS, *moments, *g0, *g1; float2 *len, *var;                             // this frame's, written
    const float4 *prevD, *prevS, *prevMoments, *prevG0, *prevG1; const float2* prevLen;       // the last frame's
    uint32_t W, H, reset, store;                               // reset: no history. store: AtrousIterations = 0, the stage writes Denoised*
    DnSettings s;
};

struct DnVarianceArgs {
    const float4 *histD, *histS, *moments, *g0, *g1; const float2* len; float2* var;
    uint32_t W, H;
    DnSettings s;
};

struct DnAtrousArgs {
    const float4 *g0, *g1, *inD, *inS; const float2* inVar;
    float4 *outD, *outS; float2* outVar;                       // the next iteration's input (not the last iteration)
    void *texD, *texS;                                         // the last iteration: Denoised*
    uint32_t W, H, step, last;
    DnSettings s;
};

PT_DEV uint16_t dn_h(float x) { return x != x ? kDnNaN16 : f32_to_f16(x); }
PT_DEV h4v dn_store(float4 c) { return h4v{ dn_h(c.x), dn_h(c.y), dn_h(c.z), dn_h(c.w) }; }
// the noisy texel as the filter takes it: the guarded rgb, a hit distance that is not finite 0 (the ReLAX pack leaves neither; a host
// that hands over something else cannot poison the history)
PT_DEV float4 dn_load(const void* tex, uint32_t i)
{
    const h4v q = gptr<h4v>(tex)[i];
    const v3 c = fl_guard(fl_rgb16(q));
    const float a = f16_to_f32(q.w);
    return float4{ c.x, c.y, c.z, isfinite(a) ? a : 0.0f };
}

// one channel of stage 1: the validated bilinear read of the history and the accumulation. q[t] = the four taps' colour, m[t] = their two
// moments, l[t] = their length; a tap with ok[t] false was not read.
struct DnChannel { float4 colour; float m1, m2, length; };
PT_DEV DnChannel dn_accumulate(const bool ok[4], const float w[4], const float4 q[4], const float2 m[4], const float l[4], float4 cur, float cap)
{
    const float L = fl_lum(cur);
    DnChannel out{ cur, L, L * L, 1.0f };                      // disoccluded: the input, length 1
    float wsum = 0.0f;
    for (int t = 0; t < 4; ++t) if (ok[t]) wsum = wsum + w[t];
    if (!(wsum > 0.0f)) return out;
    float h[7] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    for (int t = 0; t < 4; ++t) if (ok[t]) {
        h[0] = h[0] + w[t] * q[t].x; h[1] = h[1] + w[t] * q[t].y; h[2] = h[2] + w[t] * q[t].z; h[3] = h[3] + w[t] * q[t].w;
        h[4] = h[4] + w[t] * m[t].x; h[5] = h[5] + w[t] * m[t].y; h[6] = h[6] + w[t] * l[t];
    }
    for (int k = 0; k < 7; ++k) h[k] = h[k] / wsum;
    const float n1 = h[6] + 1.0f;
    const float n = n1 < cap ? n1 : cap;
    const float inv = 1.0f / n;
    out.colour = float4{ fl_blend(h[0], cur.x, inv), fl_blend(h[1], cur.y, inv), fl_blend(h[2], cur.z, inv), fl_blend(h[3], cur.w, inv) };
    out.m1 = fl_blend(h[4], out.m1, inv); out.m2 = fl_blend(h[5], out.m2, inv); out.length = n;
    return out;
}

__global__ __launch_bounds__(256) void k_dn_temporal(DnTemporalArgs a)
{
    const uint32_t x = blockIdx.x * kDnTile + threadIdx.x, y = blockIdx.y * kDnTile + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const uint32_t i = y * a.W + x;
    const float z = a.depth[i];
    const float4 zero4{ 0.0f, 0.0f, 0.0f, 0.0f };
    if (!isfinite(z)) {                                        // the G-buffer missed: Noisy -> Denoised bit for bit, length 0, never a tap
        a.g0[i] = float4{ 0.0f, 0.0f, 0.0f, z }; a.g1[i] = zero4;
        a.histD[i] = zero4; a.histS[i] = zero4; a.moments[i] = zero4; a.len[i] = float2{ 0.0f, 0.0f }; a.var[i] = float2{ 0.0f, 0.0f };
        const h4v d = gptr<h4v>(a.noisyD)[i], s = gptr<h4v>(a.noisyS)[i];
        ((PT_GLOBAL_AS h4v*)a.outD)[i] = d; ((PT_GLOBAL_AS h4v*)a.outS)[i] = s;
        return;
    }
    const s4v nr = gptr<s4v>(a.normalRoughness)[i];
    const v3 N = V3(snorm16_to_f32(nr.x), snorm16_to_f32(nr.y), snorm16_to_f32(nr.z));
    const float r = snorm16_to_f32(nr.w);
    const float4 P = a.position[i];
    const h4v mvh = gptr<h4v>(a.motion)[i];
    const float mvx = f16_to_f32(mvh.x), mvy = f16_to_f32(mvh.y), mvz = f16_to_f32(mvh.z);
    const float4 curD = dn_load(a.noisyD, i), curS = dn_load(a.noisyS, i);

    // the previous position and the four taps around it, row-major
    const FlTaps taps((((float)x + 0.5f) + mvx) - 0.5f, (((float)y + 0.5f) + mvy) - 0.5f, a.W, a.H);
    const float zp = z + mvz, zTol = a.s.depthThreshold * fabsf(zp);
    bool okD[4], okS[4]; float w[4], lD[4], lS[4]; float4 qD[4], qS[4]; float2 mD[4], mS[4];
    for (int t = 0; t < 4; ++t) {
        w[t] = taps.weight(t);
        okD[t] = okS[t] = false;
        if (a.reset || !taps.inside(t)) continue;
        const uint32_t j = taps.index(t);
        const float4 g0 = a.prevG0[j], g1 = a.prevG1[j];
        const bool geometry = fabsf(g0.w - zp) <= zTol && dot(N, V3(g1.x, g1.y, g1.z)) >= a.s.normalCosine;
        const float2 len = a.prevLen[j];
        okD[t] = geometry && len.x > 0.0f;
        okS[t] = geometry && len.y > 0.0f && fabsf(r - g1.w) <= a.s.roughnessFraction * (r > g1.w ? r : g1.w);
        if (!(okD[t] || okS[t])) continue;
        const float4 m = a.prevMoments[j];
        qD[t] = a.prevD[j]; qS[t] = a.prevS[j]; mD[t] = float2{ m.x, m.y }; mS[t] = float2{ m.z, m.w }; lD[t] = len.x; lS[t] = len.y;
    }
    const DnChannel D = dn_accumulate(okD, w, qD, mD, lD, curD, a.s.maxFrames);
    const DnChannel S = dn_accumulate(okS, w, qS, mS, lS, curS, fl_specular_cap(a.s.maxFrames, r, mvx, mvy));
    a.g0[i] = float4{ P.x, P.y, P.z, z }; a.g1[i] = float4{ N.x, N.y, N.z, r };
    a.histD[i] = D.colour; a.histS[i] = S.colour;
    a.moments[i] = float4{ D.m1, D.m2, S.m1, S.m2 }; a.len[i] = float2{ D.length, S.length };
    if (a.store) { ((PT_GLOBAL_AS h4v*)a.outD)[i] = dn_store(D.colour); ((PT_GLOBAL_AS h4v*)a.outS)[i] = dn_store(S.colour); }
}

__global__ __launch_bounds__(256) void k_dn_variance(DnVarianceArgs a)
{
    const int x = blockIdx.x * kDnTile + threadIdx.x, y = blockIdx.y * kDnTile + threadIdx.y;
    if (x >= (int)a.W || y >= (int)a.H) return;
    const uint32_t i = (uint32_t)y * a.W + (uint32_t)x;
    const float4 g0 = a.g0[i];
    if (!isfinite(g0.w)) return;                               // stage 1 wrote 0
    const float4 m = a.moments[i];
    const float2 n = a.len[i];
    float vD = fl_max0(m.y - m.x * m.x), vS = fl_max0(m.w - m.z * m.z);
    if (n.x < 4.0f || n.y < 4.0f) {                            // a short history: the moments of the 7 x 7 neighbourhood on the same surface
        const float4 g1 = a.g1[i];
        const v3 Pp = V3(g0.x, g0.y, g0.z), Np = V3(g1.x, g1.y, g1.z);
        const float planeScale = a.s.depthThreshold * fabsf(g0.w);
        float s1D = 0.0f, s2D = 0.0f, s1S = 0.0f, s2S = 0.0f, count = 0.0f;
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
            const float LD = fl_lum(a.histD[j]), LS = fl_lum(a.histS[j]);
            s1D = s1D + LD; s2D = s2D + LD * LD; s1S = s1S + LS; s2S = s2S + LS * LS; count = count + 1.0f;
        }
        const float m1D = s1D / count, m2D = s2D / count, m1S = s1S / count, m2S = s2S / count;
        if (n.x < 4.0f) vD = fl_max0(m2D - m1D * m1D);
        if (n.y < 4.0f) vS = fl_max0(m2S - m1S * m1S);
    }
    a.var[i] = float2{ vD, vS };
}

// The record of one pixel as a tap sees it, from global memory or from the staged tile.
struct DnTap { float4 g0, g1, cD, cS; float2 var; };

template <bool STAGED>
__global__ __launch_bounds__(256) void k_dn_atrous(DnAtrousArgs a)
{
    extern __shared__ float4 dn_lds[];                         // STAGED: g0 | g1 | cD | cS of side x side pixels, then their float2 variance
    const int step = (int)a.step, W = (int)a.W, H = (int)a.H;
    const int bx = blockIdx.x * kDnTile, by = blockIdx.y * kDnTile;
    const int halo = 2 * step, side = kDnTile + 2 * halo, cells = side * side;
    if (STAGED) {
        float2* ldsVar = (float2*)(dn_lds + 4 * cells);
        for (int k = threadIdx.y * kDnTile + threadIdx.x; k < cells; k += kDnTile * kDnTile) {
            const int xq = bx - halo + k % side, yq = by - halo + k / side;
            if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;    // never read: every tap tests its coordinates first
            const uint32_t j = (uint32_t)yq * a.W + (uint32_t)xq;
            dn_lds[k] = a.g0[j]; dn_lds[cells + k] = a.g1[j]; dn_lds[2 * cells + k] = a.inD[j]; dn_lds[3 * cells + k] = a.inS[j];
            ldsVar[k] = a.inVar[j];
        }
        __syncthreads();
    }
    const int x = bx + threadIdx.x, y = by + threadIdx.y;
    if (x >= W || y >= H) return;
    auto fetch = [&](int xq, int yq, bool colour) {
        DnTap t;
        if (STAGED) {
            const int k = (yq - by + halo) * side + (xq - bx + halo);
            t.g0 = dn_lds[k]; t.g1 = dn_lds[cells + k];
            if (colour) { t.cD = dn_lds[2 * cells + k]; t.cS = dn_lds[3 * cells + k]; }
            t.var = ((const float2*)(dn_lds + 4 * cells))[k];
        } else {
            const uint32_t j = (uint32_t)yq * a.W + (uint32_t)xq;
            t.g0 = a.g0[j]; t.g1 = a.g1[j];
            if (colour) { t.cD = a.inD[j]; t.cS = a.inS[j]; }
            t.var = a.inVar[j];
        }
        return t;
    };
    const uint32_t i = (uint32_t)y * a.W + (uint32_t)x;
    const DnTap p = fetch(x, y, true);
    if (!isfinite(p.g0.w)) return;                             // missed: stage 1 copied the texel
    // v3: the 3 x 3 binomial blur of the variance over the hit pixels of the frame
    float bD = 0.0f, bS = 0.0f, bw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        const int xq = x + dx, yq = y + dy;
        if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
        const DnTap q = fetch(xq, yq, false);
        if (!isfinite(q.g0.w)) continue;
        const float k = fl_blur3(dx, dy);
        bD = bD + k * q.var.x; bS = bS + k * q.var.y; bw = bw + k;
    }
    const float sdD = a.s.sigmaD * sqrtf(bD / bw) + 1e-4f, sdS = a.s.sigmaS * sqrtf(bS / bw) + 1e-4f;
    const v3 Pp = V3(p.g0.x, p.g0.y, p.g0.z), Np = V3(p.g1.x, p.g1.y, p.g1.z);
    const float rp = p.g1.w, planeScale = a.s.depthThreshold * fabsf(p.g0.w);
    const float LDp = fl_lum(p.cD), LSp = fl_lum(p.cS);
    float4 sD{ 0.0f, 0.0f, 0.0f, 0.0f }, sS{ 0.0f, 0.0f, 0.0f, 0.0f };
    float wsD = 0.0f, wsS = 0.0f, vD = 0.0f, vS = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) for (int dx = -2; dx <= 2; ++dx) {
        const int xq = x + dx * step, yq = y + dy * step;
        float wD, wS;
        DnTap q;
        if (dx == 0 && dy == 0) { q = p; wD = wS = 0.140625f; }          // the centre always weighs h(0)^2
        else {
            if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
            q = fetch(xq, yq, true);
            if (!isfinite(q.g0.w)) continue;
            const float base = ((fl_h5(dy) * fl_h5(dx)) * fl_wg(Np, Pp, V3(q.g0.x, q.g0.y, q.g0.z), planeScale)) * fl_wn(Np, V3(q.g1.x, q.g1.y, q.g1.z), a.s.normalCosine);
            const float wr = fl_wr(rp, q.g1.w, a.s.roughnessFraction);
            wD = base * fl_max0(1.0f - fabsf(fl_lum(q.cD) - LDp) / sdD);
            wS = (base * fl_max0(1.0f - fabsf(fl_lum(q.cS) - LSp) / sdS)) * wr;
        }
        if (wD > 0.0f) {
            wsD = wsD + wD; vD = vD + (wD * wD) * q.var.x;
            sD.x = sD.x + wD * q.cD.x; sD.y = sD.y + wD * q.cD.y; sD.z = sD.z + wD * q.cD.z; sD.w = sD.w + wD * q.cD.w;
        }
        if (wS > 0.0f) {
            wsS = wsS + wS; vS = vS + (wS * wS) * q.var.y;
            sS.x = sS.x + wS * q.cS.x; sS.y = sS.y + wS * q.cS.y; sS.z = sS.z + wS * q.cS.z; sS.w = sS.w + wS * q.cS.w;
        }
    }
    const float4 oD{ sD.x / wsD, sD.y / wsD, sD.z / wsD, sD.w / wsD }, oS{ sS.x / wsS, sS.y / wsS, sS.z / wsS, sS.w / wsS };
    if (a.last) { ((PT_GLOBAL_AS h4v*)a.texD)[i] = dn_store(oD); ((PT_GLOBAL_AS h4v*)a.texS)[i] = dn_store(oS); }
    else { a.outD[i] = oD; a.outS[i] = oS; a.outVar[i] = float2{ vD / (wsD * wsD), vS / (wsS * wsS) }; }
}

// the form pt_denoiser_process takes for a step: the staged one wherever the tile's halo fits -- it is the faster one at steps 1, 2 and 4,
// by 2.5x, 2.1x and 1.3x ("Denoiser") -- unless PT_DENOISER_FORM_DIRECT pins the direct one
static bool dn_staged(const Context& c, uint32_t step)
{
    return step <= kFlStagedMaxStep && !(c.debugFlags & PT_DENOISER_FORM_DIRECT);
}

} // namespace pt

using namespace pt;

// nullptr when the settings are in range, else the message of the refusal
static const char* dn_check_settings(const PtDenoiserSettings* s)
{
    if (const char* refusal = fl_check_sizes(s->RenderSize)) return refusal;
    if (!(s->MaxAccumulatedFrames >= 1u && s->MaxAccumulatedFrames <= 255u)) return "MaxAccumulatedFrames must be 1..255";
    if (s->AtrousIterations > 8u) return "AtrousIterations must be 0..8";
    if (!(s->DepthThreshold > 0.0f && s->DepthThreshold <= 1.0f)) return "DepthThreshold must be in (0, 1]";
    if (!(s->NormalCosine >= 0.0f && s->NormalCosine < 1.0f)) return "NormalCosine must be in [0, 1)";
    if (!(s->DiffuseLuminanceSigma > 0.0f && std::isfinite(s->DiffuseLuminanceSigma))) return "DiffuseLuminanceSigma must be positive and finite";
    if (!(s->SpecularLuminanceSigma > 0.0f && std::isfinite(s->SpecularLuminanceSigma))) return "SpecularLuminanceSigma must be positive and finite";
    if (!(s->RoughnessFraction > 0.0f && std::isfinite(s->RoughnessFraction))) return "RoughnessFraction must be positive and finite";
    return nullptr;
}

extern "C" {

int pt_denoiser_set_constants(PtContext* ctx, const PtDenoiserSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    return fl_set_constants(ctx->c, s, dn_check_settings, ctx->c.dn, ctx->c.dnState);
}

int pt_denoiser_reset_history(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.dnState.frames = 0;
    return PT_OK;
}

int pt_denoiser_process(PtContext* ctx, const struct PtDenoiserTextures* t)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, t, "textures is NULL");
    if (!c.dnState.have) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "call pt_denoiser_set_constants first");
    const BoundTexture bound[8] = {
        { "Position", t->Position, 16 }, { "LinearDepth", t->LinearDepth, 4 }, { "NormalRoughness", t->NormalRoughness, 8 },
        { "MotionVector", t->MotionVector, 8 }, { "NoisyDiffuse", t->NoisyDiffuse, 8 }, { "NoisySpecular", t->NoisySpecular, 8 },
        { "DenoisedDiffuse", t->DenoisedDiffuse, 8 }, { "DenoisedSpecular", t->DenoisedSpecular, 8 } };
    if (int refusal = fl_check_bound(c, bound)) return refusal;
    const PtDenoiserSettings& s = c.dn;
    const uint32_t W = s.RenderSize[0], H = s.RenderSize[1];
    const size_t n = (size_t)W * H;
    API_HIP(&c, hipSetDevice(c.device));
    if (int e = fl_grow_history(c, c.dnState, want(c.dnHistory, n * DN_SLOTS))) return e;
    if (s.AtrousIterations >= 3u && dn_staged(c, 4u))           // the staged tile of step 4 is beyond the 64 kB a launch gets unasked
        API_HIP(&c, hipFuncSetAttribute((const void*)k_dn_atrous<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 32 * 32 * (int)kDnStagedBytes));
    float4* base = c.dnHistory.data();
    float2* halves = (float2*)(base + n * DN_PAIRS);
    const uint32_t cur = c.dnState.parity ^ 1u, prev = c.dnState.parity;
    auto slot = [&](int first, uint32_t parity) { return base + n * (first + parity); };

    const DnSettings ds{ (float)s.MaxAccumulatedFrames, s.DepthThreshold, s.NormalCosine, s.DiffuseLuminanceSigma, s.SpecularLuminanceSigma, s.RoughnessFraction };
    const dim3 grid((W + kDnTile - 1) / kDnTile, (H + kDnTile - 1) / kDnTile), block(kDnTile, kDnTile);
    DnTemporalArgs ta{};
    ta.position = (const float4*)t->Position; ta.depth = (const float*)t->LinearDepth; ta.normalRoughness = t->NormalRoughness; ta.motion = t->MotionVector;
    ta.noisyD = t->NoisyDiffuse; ta.noisyS = t->NoisySpecular; ta.outD = t->DenoisedDiffuse; ta.outS = t->DenoisedSpecular;
    ta.histD = slot(DN_HIST_D, cur); ta.histS = slot(DN_HIST_S, cur); ta.moments = slot(DN_MOMENTS, cur); ta.g0 = slot(DN_G0, cur); ta.g1 = slot(DN_G1, cur);
    ta.len = halves + n * (DN_LEN + cur); ta.var = halves + n * DN_VAR;
    ta.prevD = slot(DN_HIST_D, prev); ta.prevS = slot(DN_HIST_S, prev); ta.prevMoments = slot(DN_MOMENTS, prev); ta.prevG0 = slot(DN_G0, prev);
    ta.prevG1 = slot(DN_G1, prev); ta.prevLen = halves + n * (DN_LEN + prev);
    ta.W = W; ta.H = H; ta.reset = c.dnState.frames == 0 ? 1u : 0u; ta.store = s.AtrousIterations == 0u ? 1u : 0u; ta.s = ds;
    k_dn_temporal<<<grid, block, 0, c.stream>>>(ta);
    if (s.AtrousIterations) {
        DnVarianceArgs va{ ta.histD, ta.histS, ta.moments, ta.g0, ta.g1, ta.len, ta.var, W, H, ds };
        k_dn_variance<<<grid, block, 0, c.stream>>>(va);
        DnAtrousArgs aa{};
        aa.g0 = ta.g0; aa.g1 = ta.g1; aa.inD = ta.histD; aa.inS = ta.histS; aa.inVar = ta.var;
        aa.texD = t->DenoisedDiffuse; aa.texS = t->DenoisedSpecular; aa.W = W; aa.H = H; aa.s = ds;
        for (uint32_t k = 0; k < s.AtrousIterations; ++k) {
            aa.step = 1u << k; aa.last = k + 1u == s.AtrousIterations ? 1u : 0u;
            aa.outD = slot(DN_WORK_D, k & 1u); aa.outS = slot(DN_WORK_S, k & 1u); aa.outVar = halves + n * (DN_WORK_VAR + (k & 1u));
            if (dn_staged(c, aa.step)) {
                const int side = kDnTile + 4 * (int)aa.step;
                k_dn_atrous<true><<<grid, block, (size_t)side * side * kDnStagedBytes, c.stream>>>(aa);   // 28.8, 41.5 and 73.7 kB at step 1, 2 and 4
            } else k_dn_atrous<false><<<grid, block, 0, c.stream>>>(aa);
            aa.inD = aa.outD; aa.inS = aa.outS; aa.inVar = aa.outVar;
        }
    }
    API_HIP(&c, hipGetLastError());
    c.dnState.advance(W, H);
    return PT_OK;
}

int pt_denoiser_download_history(PtContext* ctx, float* host_length, uint64_t capacity_pixels, uint32_t* out_w, uint32_t* out_h)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_w && out_h && (host_length || capacity_pixels == 0), "out_w / out_h / host_length is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    *out_w = c.dnState.shown(0); *out_h = c.dnState.shown(1);
    const size_t n = (size_t)*out_w * *out_h;
    const size_t count = (size_t)std::min<uint64_t>(capacity_pixels, n);
    if (!count) return PT_OK;
    std::vector<float2> both(count);
    const float2* len = (const float2*)(c.dnHistory.data() + n * DN_PAIRS) + n * (DN_LEN + c.dnState.parity);
    API_HIP(&c, hipMemcpy(both.data(), len, count * sizeof(float2), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < count; ++k) host_length[k] = both[k].x;   // the diffuse length (the specular one differs only where its own tests do)
    return PT_OK;
}

} // extern "C"
