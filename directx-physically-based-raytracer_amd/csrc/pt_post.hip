// pt_post.hip -- the post-processing chain after the frame (gfx950): bloom, merge, tone mapping and the display encodes.
//
//   k_post_down<KARIS>        <- Shaders/Bloom.hlsl Downsample: stages 0-4 of Bloom::Process (Source/Bloom.ixx:87-124), KARIS on 0 and 1
//   k_post_up                 <- Shaders/Bloom.hlsl Upsample: stages 5-8
//   k_post_resolve<B, OP, HDR> <- Shaders/Merge.hlsl (B: bloom on), DirectXTK ToneMapPostProcess (OP / HDR) and CopyTexture into the
//                                R10G10B10A2_UNORM back buffer, in one pass over the frame (App::PostProcessGraphics, App.cpp:1506-1571).
//                                The two fp16 round trips of the reference's Color texture are kept in registers.
// DESIGN.md section 1, "Post-processing", is the arithmetic spec. Every stage reads the image of the stage before it; stage s writes
// slot s of Context::postLevels, so the nine images stay downloadable (the reference ping-pongs them through two pyramids).
#include "pt_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pt {

constexpr int kPostStages = 9;
constexpr int kPostMips = 5;
constexpr uint32_t kPostMaxSize = 16384u;              // D3D12_REQ_TEXTURE2D_U_OR_V_DIMENSION: texel indices stay 32-bit
constexpr float kUpsampleRadius = 5e-3f;               // Bloom.ixx:110, in UV units on both axes
constexpr float kInvGamma = 0.454545454545f;           // 1 / 2.2 (DirectXTK LinearToSRGBEst)

// ST.2084 (DirectXTK LinearToST2084): constants of SMPTE ST 2084
constexpr float kPqM1 = 0.1593017578125f, kPqM2 = 78.84375f, kPqC1 = 0.8359375f, kPqC2 = 18.8515625f, kPqC3 = 18.6875f;

typedef uint16_t h4v __attribute__((ext_vector_type(4)));      // one fp16 RGBA texel: 8-byte loads and stores in the global address space
PT_DEV v3 h3(h4v q) { return V3(f16_to_f32(q.x), f16_to_f32(q.y), f16_to_f32(q.z)); }

// SampleLevel(linear, CLAMP): bilinear over an fp16 RGBA texture, weights from the fp32 coordinate as in pt_texture.hpp.
PT_DEV v3 post_bilinear(const ushort4* t, int W, int H, float u, float v)
{
    const float fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float wx = fx - x0f, wy = fy - y0f;
    const int xa = (int)x0f, ya = (int)y0f;
    const int x0 = min(max(xa, 0), W - 1), x1 = min(max(xa + 1, 0), W - 1);
    const int y0 = min(max(ya, 0), H - 1), y1 = min(max(ya + 1, 0), H - 1);
    const PT_GLOBAL_AS h4v* r0 = gptr<h4v>(t) + (uint32_t)y0 * (uint32_t)W;
    const PT_GLOBAL_AS h4v* r1 = gptr<h4v>(t) + (uint32_t)y1 * (uint32_t)W;
    const v3 c00 = h3(r0[x0]), c10 = h3(r0[x1]), c01 = h3(r1[x0]), c11 = h3(r1[x1]);
    const float ix = 1.0f - wx, iy = 1.0f - wy;
    v3 o;
    { const float top = mad(c10.x, wx, c00.x * ix), bot = mad(c11.x, wx, c01.x * ix); o.x = mad(bot, wy, top * iy); }
    { const float top = mad(c10.y, wx, c00.y * ix), bot = mad(c11.y, wx, c01.y * ix); o.y = mad(bot, wy, top * iy); }
    { const float top = mad(c10.z, wx, c00.z * ix), bot = mad(c11.z, wx, c01.z * ix); o.z = mad(bot, wy, top * iy); }
    return o;
}

// FLOAT -> fp16 of an fp32 value. The empty asm makes the value opaque: without it the compiler fuses the fma that produced it and the
// conversion into v_fma_mixlo_f16, which rounds the exact a * b + c to fp16 once -- one value in about 10^4 then differs by an fp16 ulp
// from the spec's fp32 rounding followed by the fp16 one.
PT_DEV uint16_t f16_of_f32(float x) { asm volatile("" : "+v"(x)); return f32_to_f16(x); }

PT_DEV void store_h3(ushort4* out, uint32_t i, v3 c)           // a float3 store to a 4-channel texture: 0 in the 4th channel
{
    ((PT_GLOBAL_AS h4v*)out)[i] = h4v{ f16_of_f32(c.x), f16_of_f32(c.y), f16_of_f32(c.z), 0 };
}

PT_DEV v3 add3(v3 a, v3 b) { return V3(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_DEV v3 sum4(v3 a, v3 b, v3 c, v3 d) { return add3(add3(add3(a, b), c), d); }
PT_DEV v3 mad3(v3 a, float s, v3 b) { return V3(mad(a.x, s, b.x), mad(a.y, s, b.y), mad(a.z, s, b.z)); }

// x^y for x >= 0 (0^y = 0, 1^y = 1) as exp2(y log2 x) on v_log_f32 / v_exp_f32: the powers of this file are not bit-pinned (DESIGN.md
// section 1), and within the bounds of tests/test_post_processing_gpu.py this costs a fraction of powf's VALU work.
PT_DEV float pow_pos(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }

// [unpinned] Color::ToSrgb (MathLib): saturate, then the piecewise sRGB OETF with exponent 0.41666
PT_DEV float to_srgb1(float x)
{
    x = saturate(x);
    return x < 0.0031308f ? 12.92f * x : mad(1.055f, pow_pos(x, 0.41666f), -0.055f);
}
PT_DEV v3 karis(v3 g)                                             // g * KarisAverage(g): 1 / (1 + Luminance(ToSrgb(g)) / 4)
{
    const float w = 1.0f / mad(ml_luminance(V3(to_srgb1(g.x), to_srgb1(g.y), to_srgb1(g.z))), 0.25f, 1.0f);
    return g * w;
}

// One thread per output texel; the block is 64 x 4 texels (a wave = 64 texels of one row).
struct PostStage { const ushort4* in; ushort4* out; int wi, hi, wo, ho; };

template <bool KARIS>
__global__ __launch_bounds__(256) void k_post_down(PostStage a)
{
    const int x = blockIdx.x * 64 + (int)(threadIdx.x & 63u), y = blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.wo || y >= a.ho) return;
    const float u = ((float)x + 0.5f) / (float)a.wo, v = ((float)y + 0.5f) / (float)a.ho;    // Math::CalculateUV
    const float sx = 1.0f / (float)a.wo, sy = 1.0f / (float)a.ho;                           // g_size: output texels
    auto S = [&](float dx, float dy) { return post_bilinear(a.in, a.wi, a.hi, mad(sx, dx, u), mad(sy, dy, v)); };
    const v3 A = S(-2, 2), B = S(0, 2), Cc = S(2, 2), D = S(-2, 0), E = S(0, 0), F = S(2, 0), G = S(-2, -2), Hh = S(0, -2), I = S(2, -2);
    const v3 J = S(-1, 1), K = S(1, 1), L = S(-1, -1), M = S(1, -1);
    v3 r;
    if (KARIS) {
        const v3 g0 = karis(sum4(A, B, D, E) * 0.03125f), g1 = karis(sum4(B, Cc, E, F) * 0.03125f);
        const v3 g2 = karis(sum4(D, E, G, Hh) * 0.03125f), g3 = karis(sum4(E, F, Hh, I) * 0.03125f);
        const v3 g4 = karis(sum4(J, K, L, M) * 0.125f);
        r = add3(add3(add3(add3(g0, g1), g2), g3), g4);
        r = V3(fmaxf(r.x, 1e-4f), fmaxf(r.y, 1e-4f), fmaxf(r.z, 1e-4f));
    } else {
        r = mad3(sum4(J, K, L, M), 0.125f, mad3(sum4(B, D, F, Hh), 0.0625f, mad3(sum4(A, Cc, G, I), 0.03125f, E * 0.125f)));
    }
    store_h3(a.out, (uint32_t)y * (uint32_t)a.wo + (uint32_t)x, r);
}

__global__ __launch_bounds__(256) void k_post_up(PostStage a)
{
    const int x = blockIdx.x * 64 + (int)(threadIdx.x & 63u), y = blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.wo || y >= a.ho) return;
    const float u = ((float)x + 0.5f) / (float)a.wo, v = ((float)y + 0.5f) / (float)a.ho;
    const float s = kUpsampleRadius;
    auto S = [&](float dx, float dy) { return post_bilinear(a.in, a.wi, a.hi, mad(s, dx, u), mad(s, dy, v)); };
    const v3 A = S(-1, 1), B = S(0, 1), Cc = S(1, 1), D = S(-1, 0), E = S(0, 0), F = S(1, 0), G = S(-1, -1), Hh = S(0, -1), I = S(1, -1);
    v3 r = mad3(sum4(B, D, F, Hh), 2.0f, E * 4.0f);
    r = add3(add3(add3(add3(r, A), Cc), G), I);
    store_h3(a.out, (uint32_t)y * (uint32_t)a.wo + (uint32_t)x, r * 0.0625f);   // / 16: a power of two, exact
}

struct PostResolve {
    const ushort4* radiance; const ushort4* blur;      // blur: stage 8's image (Blur1 mip 0)
    ushort4* color; uint32_t* back; uint32_t* disp8;
    int w, h, bw, bh;
    float w1, w2;                                       // Merge weights: 1 - Strength (Radiance), Strength (bloom)
    float scale;                                        // SDR: exp2(Exposure); HDR: PaperWhiteNits / 10000
    float M[9];                                         // HDR: the colour-primary rotation, rows for column vectors
};

PT_DEV uint32_t f32_to_unorm_n(float f, float maxCode)          // D3D11.3 FLOAT -> UNORM, as f32_to_unorm8
{
    if (!(f == f)) return 0u;
    f = saturate(f) * maxCode + 0.5f;
    return (uint32_t)f;
}
PT_DEV float tone_op(int op, float x)
{
    if (op == PT_TONE_MAP_SATURATE) return saturate(x);
    if (op == PT_TONE_MAP_REINHARD) return x / (1.0f + x);
    return saturate(x * mad(2.51f, x, 0.03f) / mad(x, mad(2.43f, x, 0.59f), 0.14f));   // ACES filmic (Narkowicz fit)
}
PT_DEV float pq(float n)
{
    const float p = pow_pos(fabsf(n), kPqM1);
    return pow_pos(mad(kPqC2, p, kPqC1) / mad(kPqC3, p, 1.0f), kPqM2);
}

template <bool BLOOM, int OP, bool HDR>
__global__ __launch_bounds__(256) void k_post_resolve(PostResolve a)
{
    const int x = blockIdx.x * 64 + (int)(threadIdx.x & 63u), y = blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.w || y >= a.h) return;
    const uint32_t i = (uint32_t)y * (uint32_t)a.w + (uint32_t)x;
    v3 m; uint16_t alpha;
    if (BLOOM) {                                        // Merge: both terms sampled at the output UV, stored as fp16 (Color)
        const float u = ((float)x + 0.5f) / (float)a.w, v = ((float)y + 0.5f) / (float)a.h;
        const v3 r = post_bilinear(a.radiance, a.w, a.h, u, v), b = post_bilinear(a.blur, a.bw, a.bh, u, v);
        m = V3(mad(b.x, a.w2, r.x * a.w1), mad(b.y, a.w2, r.y * a.w1), mad(b.z, a.w2, r.z * a.w1));
        m = V3(f16_to_f32(f16_of_f32(m.x)), f16_to_f32(f16_of_f32(m.y)), f16_to_f32(f16_of_f32(m.z)));
        alpha = 0;                                      // Merge's float3 store
    } else {                                            // ToneMap reads each texel exactly
        const h4v q = gptr<h4v>(a.radiance)[i];
        m = h3(q); alpha = q.w;
    }
    v3 c;
    if (HDR) {
        const v3 r = V3(sop3(a.M[0], m.x, a.M[1], m.y, a.M[2], m.z), sop3(a.M[3], m.x, a.M[4], m.y, a.M[5], m.z),
                        sop3(a.M[6], m.x, a.M[7], m.y, a.M[8], m.z));
        c = V3(pq(r.x * a.scale), pq(r.y * a.scale), pq(r.z * a.scale));
    } else {
        c = V3(pow_pos(fabsf(tone_op(OP, m.x * a.scale)), kInvGamma), pow_pos(fabsf(tone_op(OP, m.y * a.scale)), kInvGamma),
               pow_pos(fabsf(tone_op(OP, m.z * a.scale)), kInvGamma));
    }
    const h4v q = h4v{ f16_of_f32(c.x), f16_of_f32(c.y), f16_of_f32(c.z), alpha };
    if (a.color) ((PT_GLOBAL_AS h4v*)a.color)[i] = q;
    const float cr = f16_to_f32(q.x), cg = f16_to_f32(q.y), cb = f16_to_f32(q.z), ca = f16_to_f32(q.w);
    if (a.back)
        ((PT_GLOBAL_AS uint32_t*)a.back)[i] = f32_to_unorm_n(cr, 1023.0f) | f32_to_unorm_n(cg, 1023.0f) << 10 |
                                              f32_to_unorm_n(cb, 1023.0f) << 20 | f32_to_unorm_n(ca, 3.0f) << 30;
    if (a.disp8)
        ((PT_GLOBAL_AS uint32_t*)a.disp8)[i] = (uint32_t)f32_to_unorm8(cr) | (uint32_t)f32_to_unorm8(cg) << 8 |
                                               (uint32_t)f32_to_unorm8(cb) << 16 | (uint32_t)f32_to_unorm8(ca) << 24;
}

} // namespace pt

using namespace pt;

static dim3 post_grid(uint32_t w, uint32_t h) { return dim3((w + 63u) / 64u, (h + 3u) / 4u); }

// the resolve kernel's variants: bloom on or off; HDR (no operator), or one of the three tone-mapping operators
static void launch_resolve(const PostResolve& a, bool bloom, uint32_t op, bool hdr, hipStream_t stream)
{
    auto variants = [&](auto BLOOM) {
        auto launch = [&](auto OP, auto HDR) { k_post_resolve<BLOOM(), OP(), HDR()><<<post_grid((uint32_t)a.w, (uint32_t)a.h), 256, 0, stream>>>(a); };
        if (hdr) launch(std::integral_constant<int, 0>{}, std::true_type{});
        else if (op == PT_TONE_MAP_SATURATE) launch(std::integral_constant<int, PT_TONE_MAP_SATURATE>{}, std::false_type{});
        else if (op == PT_TONE_MAP_REINHARD) launch(std::integral_constant<int, PT_TONE_MAP_REINHARD>{}, std::false_type{});
        else launch(std::integral_constant<int, PT_TONE_MAP_ACES_FILMIC>{}, std::false_type{});
    };
    if (!bloom) variants(std::false_type{}); else variants(std::true_type{});
}

// DirectXTK's colour-primary rotations (ToneMapPostProcess.cpp), rows for column vectors
static const float kRotations[3][9] = {
    { 0.6274040f, 0.3292820f, 0.0433136f, 0.0690970f, 0.9195400f, 0.0113612f, 0.0163916f, 0.0880132f, 0.8955950f },          // 709 -> 2020
    { 0.753845f, 0.198593f, 0.047562f, 0.0457456f, 0.941777f, 0.0124772f, -0.00121055f, 0.0176041f, 0.983607f },              // P3-D65 -> 2020
    { 0.822461969f, 0.1775380f, 0.0f, 0.033194199f, 0.9668058f, 0.0f, 0.017082631f, 0.0723974f, 0.9105199f },                 // 709 -> P3-D65
};

extern "C" {

int pt_post_set_constants(PtContext* ctx, const PtPostProcessSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, s, "settings is NULL");
    API_ARG(&c, s->RenderSize[0] >= 1u && s->RenderSize[0] <= kPostMaxSize && s->RenderSize[1] >= 1u && s->RenderSize[1] <= kPostMaxSize,
             "RenderSize must be 1..16384 on both axes");
    API_ARG(&c, s->IsBloomEnabled <= 1u && s->IsHDREnabled <= 1u, "IsBloomEnabled / IsHDREnabled must be 0 or 1");
    API_ARG(&c, s->BloomStrength >= 0.0f && s->BloomStrength <= 1.0f, "BloomStrength must be in [0, 1]");
    API_ARG(&c, s->ToneMappingOperator >= PT_TONE_MAP_SATURATE && s->ToneMappingOperator <= PT_TONE_MAP_ACES_FILMIC, "unknown ToneMappingOperator");
    API_ARG(&c, s->Exposure >= -10.0f && s->Exposure <= 10.0f, "Exposure must be in [-10, 10]");
    API_ARG(&c, s->PaperWhiteNits >= 50.0f && s->PaperWhiteNits <= 10000.0f, "PaperWhiteNits must be in [50, 10000]");
    API_ARG(&c, s->ColorPrimaryRotation <= PT_COLOR_ROTATION_HDTV_TO_DCI_P3_D65, "unknown ColorPrimaryRotation");
    c.post = *s;
    memset(c.post._pad, 0, sizeof c.post._pad);
    c.havePost = true;
    return PT_OK;
}

int pt_post_render(PtContext* ctx, const PtPostTextures* t)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, t, "textures is NULL");
    if (!c.havePost) return fail(&c, PT_ERROR_NOT_READY, "call pt_post_set_constants first");
    const PtPostProcessSettings& s = c.post;
    const uint32_t W = s.RenderSize[0], H = s.RenderSize[1];
    const bool bloom = s.IsBloomEnabled != 0;
    API_ARG(&c, t->Radiance, "Radiance is NULL");
    API_ARG(&c, t->Color || t->BackBuffer || t->Display8, "no output bound (Color, BackBuffer, Display8)");
    API_ARG(&c, ((uintptr_t)t->Radiance & 7u) == 0 && ((uintptr_t)t->Color & 7u) == 0 && ((uintptr_t)t->BackBuffer & 3u) == 0 &&
             ((uintptr_t)t->Display8 & 3u) == 0, "textures must be aligned to their texel size");
    API_ARG(&c, !bloom || (W >= 2u && H >= 2u && std::max(W, H) >= 32u),
             "bloom needs RenderSize W, H >= 2 and max(W, H) >= 32 (five mips of the half-size pyramid)");
    API_HIP(&c, hipSetDevice(c.device));

    PostResolve r; memset(&r, 0, sizeof r);
    r.radiance = (const ushort4*)t->Radiance; r.color = (ushort4*)t->Color; r.back = (uint32_t*)t->BackBuffer; r.disp8 = (uint32_t*)t->Display8;
    r.w = (int)W; r.h = (int)H;
    if (s.IsHDREnabled) {
        r.scale = (float)((double)s.PaperWhiteNits / 10000.0);
        memcpy(r.M, kRotations[s.ColorPrimaryRotation], sizeof r.M);
    } else {
        r.scale = (float)std::exp2((double)s.Exposure);
    }
    if (!bloom) {
        launch_resolve(r, false, s.ToneMappingOperator, s.IsHDREnabled != 0, c.stream);
        API_HIP(&c, hipGetLastError());
        return PT_OK;
    }

    // level sizes: mip 0 = (W/2, H/2), mip k = max(1, mip0 >> k); slot s holds the image of stage s
    uint32_t dims[kPostStages][2]; size_t off[kPostStages]; size_t total = 0;
    for (int st = 0; st < kPostStages; ++st) {
        const int k = st < kPostMips ? st : 2 * (kPostMips - 1) - st;
        dims[st][0] = std::max(1u, (W / 2u) >> k); dims[st][1] = std::max(1u, (H / 2u) >> k);
        off[st] = total; total += (size_t)dims[st][0] * dims[st][1];
    }
    API_HIP(&c, grow(c.stream, nullptr, want(c.postLevels, total)));
    memset(c.postDims, 0, sizeof c.postDims);
    ushort4* base = c.postLevels.data();
    for (int st = 0; st < kPostStages; ++st) {
        PostStage a;
        a.in = st == 0 ? r.radiance : base + off[st - 1];
        a.wi = st == 0 ? (int)W : (int)dims[st - 1][0]; a.hi = st == 0 ? (int)H : (int)dims[st - 1][1];
        a.out = base + off[st]; a.wo = (int)dims[st][0]; a.ho = (int)dims[st][1];
        const dim3 g = post_grid(dims[st][0], dims[st][1]);
        if (st < 2) k_post_down<true><<<g, 256, 0, c.stream>>>(a);          // InputMipLevel 0 on both: the Karis branch
        else if (st < kPostMips) k_post_down<false><<<g, 256, 0, c.stream>>>(a);
        else k_post_up<<<g, 256, 0, c.stream>>>(a);
        API_HIP(&c, hipGetLastError());
    }
    r.blur = base + off[kPostStages - 1]; r.bw = (int)dims[kPostStages - 1][0]; r.bh = (int)dims[kPostStages - 1][1];
    r.w1 = 1.0f - s.BloomStrength; r.w2 = s.BloomStrength;
    launch_resolve(r, true, s.ToneMappingOperator, s.IsHDREnabled != 0, c.stream);
    API_HIP(&c, hipGetLastError());
    memcpy(c.postDims, dims, sizeof dims); memcpy(c.postOffset, off, sizeof off);
    return PT_OK;
}

int pt_post_download_bloom(PtContext* ctx, uint32_t stage, uint16_t* host, uint64_t capacity, uint32_t* out_width, uint32_t* out_height)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_width && out_height && (host || capacity == 0), "out_width / out_height / host_rgba16f is NULL");
    API_ARG(&c, stage < (uint32_t)kPostStages, "stage must be 0..8");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    *out_width = c.postDims[stage][0]; *out_height = c.postDims[stage][1];
    const uint64_t n = std::min<uint64_t>(capacity, (uint64_t)c.postDims[stage][0] * c.postDims[stage][1]);
    if (n) API_HIP(&c, hipMemcpy(host, c.postLevels.data() + c.postOffset[stage], n * sizeof(ushort4), hipMemcpyDeviceToHost));
    return PT_OK;
}

} // extern "C"
