// pt_nrd.hip -- the NRD composition pass around a host's denoiser (gfx950).
//
//   k_nrd<PACK, CLS, TWO>  <- Shaders/NRDComposition.hlsl:36-88 (NRDComposition::Process, Source/NRDComposition.ixx), which App::ProcessNRD
//                             (Source/App.cpp:1595-1688) runs with IsPack = true in front of the denoiser and IsPack = false behind it.
//                             CLS: the denoiser class (ReBLUR, ReLAX, neither: the shader falls through both branches), so the kernel has
//                             no per-pixel branch on the mode. TWO: two pixels per lane with 16-byte accesses instead of one with 8-byte ones.
// NRD.hlsli is not part of the reference tree: DESIGN.md section 1, "NRD composition", is the arithmetic spec (tests/nrdref.py restates it).
// The pass is element-wise, so the frame is one linear array of RenderSize[0] * RenderSize[1] pixels.
#include "pt_internal.hpp"

#include <cmath>

namespace pt {

constexpr uint32_t kNrdMaxSize = 16384u;                       // D3D12_REQ_TEXTURE2D_U_OR_V_DIMENSION: the pixel count stays below 2^32
constexpr float kNrdFp16Max = 65504.0f;
constexpr float kNrdMinHitDistance = 1e-7f;                    // 0 is NRD's "no data" mark: a hit distance that is not 0 stays above it
constexpr uint16_t kNrdNaN16 = 0x7E00u;

enum { NRD_CLS_REBLUR = 0, NRD_CLS_RELAX = 1, NRD_CLS_NONE = 2 };

typedef uint16_t n4v __attribute__((ext_vector_type(4)));     // one fp16 RGBA texel
typedef uint16_t n8v __attribute__((ext_vector_type(8)));     // two of them
typedef float    f2v __attribute__((ext_vector_type(2)));
typedef int16_t  s4v __attribute__((ext_vector_type(4)));
typedef int16_t  s8v __attribute__((ext_vector_type(8)));

struct NrdArgs {
    const float* depth; const void* diffuseAlbedo; const void* specularAlbedo; const void* normalRoughness;
    void* noisyDiffuse; void* noisySpecular; const void* denoisedDiffuse; const void* denoisedSpecular; void* radiance;
    uint32_t n;                                                // pixels
    float P[4];                                                // ReBLURHitDistance
};

// The selects of the spec: NaN and -0 go to +0, so that no result depends on how a min / max instruction orders them.
PT_DEV float nrd_clamp0(float x, float hi) { return x > 0.0f ? (x < hi ? x : hi) : 0.0f; }   // clamp(x, 0, hi), saturate(x) for hi = 1
PT_DEV float nrd_max0(float x) { return x > 0.0f ? x : 0.0f; }
PT_DEV float nrd_mark(float a) { return a != 0.0f && a < kNrdMinHitDistance ? kNrdMinHitDistance : a; }   // a >= 0
// the fp16 store: round to nearest even; a NaN is stored as the one quiet NaN 0x7E00 (the payload of an fp32 NaN is not part of the spec)
PT_DEV uint16_t nrd_h(float x) { return x != x ? kNrdNaN16 : f32_to_f16(x); }

PT_DEV void nrd_sanitize(v3& c)                                // all three go to 0 when one is NaN or +-inf, else clamp(c, 0, 65504)
{
    const bool ok = finite3(c);
    c = V3(ok ? nrd_clamp0(c.x, kNrdFp16Max) : 0.0f, ok ? nrd_clamp0(c.y, kNrdFp16Max) : 0.0f, ok ? nrd_clamp0(c.z, kNrdFp16Max) : 0.0f);
}

// REBLUR_FrontEnd_GetNormHitDist: every product and every sum is rounded (-ffp-contract=off); exp2f is not bit-pinned
PT_DEV float nrd_norm_hit_dist(float a, float z, const float P[4], float r)
{
    const float s = P[0] + fabsf(z) * P[1];
    const float t = nrd_clamp0(exp2f(P[3] * r * r), 1.0f);
    const float f = s * (1.0f + t * (P[2] - 1.0f));
    return nrd_clamp0(a / f, 1.0f);
}

template <int CLS>
PT_DEV n4v nrd_pack_texel(n4v q, n4v albedo, float z, const float P[4], float r)
{
    v3 c = V3(f16_to_f32(q.x) / f16_to_f32(albedo.x), f16_to_f32(q.y) / f16_to_f32(albedo.y), f16_to_f32(q.z) / f16_to_f32(albedo.z));
    if (CLS == NRD_CLS_NONE) return n4v{ nrd_h(c.x), nrd_h(c.y), nrd_h(c.z), q.w };          // demodulation only: the alpha keeps its bits
    float a = f16_to_f32(q.w);
    if (CLS == NRD_CLS_REBLUR) {
        a = nrd_norm_hit_dist(a, z, P, r);                      // in [0, 1], NaN -> 0: the sanitize's second saturate changes nothing
        nrd_sanitize(c);
        a = nrd_mark(a);
        const float Y = (c.x * 0.25f + c.y * 0.5f) + c.z * 0.25f;
        const float Co = c.x * 0.5f + c.z * -0.5f;
        const float Cg = (c.x * -0.25f + c.y * 0.5f) + c.z * -0.25f;
        return n4v{ nrd_h(Y), nrd_h(Co), nrd_h(Cg), nrd_h(a) };
    }
    nrd_sanitize(c);
    a = nrd_mark(isfinite(a) ? nrd_clamp0(a, kNrdFp16Max) : 0.0f);
    return n4v{ nrd_h(c.x), nrd_h(c.y), nrd_h(c.z), nrd_h(a) };
}

template <int CLS>
PT_DEV v3 nrd_unpack_texel(n4v q)
{
    const v3 c = V3(f16_to_f32(q.x), f16_to_f32(q.y), f16_to_f32(q.z));
    if (CLS != NRD_CLS_REBLUR) return c;                        // RELAX_BackEnd_UnpackRadiance: rgb as stored
    const float t = c.x - c.z;                                  // Y - Cg
    return V3(nrd_max0(t + c.y), nrd_max0(c.x + c.z), nrd_max0(t - c.y));
}

template <int CLS>
PT_DEV n4v nrd_compose_texel(n4v rad, n4v d, n4v s, n4v da, n4v sa)
{
    const v3 cd = nrd_unpack_texel<CLS>(d), cs = nrd_unpack_texel<CLS>(s);
    const float x = f16_to_f32(rad.x) + (cd.x * f16_to_f32(da.x) + cs.x * f16_to_f32(sa.x));
    const float y = f16_to_f32(rad.y) + (cd.y * f16_to_f32(da.y) + cs.y * f16_to_f32(sa.y));
    const float z = f16_to_f32(rad.z) + (cd.z * f16_to_f32(da.z) + cs.z * f16_to_f32(sa.z));
    return n4v{ nrd_h(x), nrd_h(y), nrd_h(z), rad.w };
}

template <typename T> PT_DEV PT_GLOBAL_AS T* nrd_out(void* p) { return (PT_GLOBAL_AS T*)p; }
PT_DEV n4v lo4(n8v v) { return n4v{ v.s0, v.s1, v.s2, v.s3 }; }
PT_DEV n4v hi4(n8v v) { return n4v{ v.s4, v.s5, v.s6, v.s7 }; }
PT_DEV n8v cat4(n4v a, n4v b) { return n8v{ a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w }; }

// one pixel, 8-byte accesses
template <bool PACK, int CLS>
PT_DEV void nrd_pixel(const NrdArgs& a, uint32_t i)
{
    const float z = gptr<float>(a.depth)[i];
    if (!isfinite(z)) return;
    const n4v da = gptr<n4v>(a.diffuseAlbedo)[i], sa = gptr<n4v>(a.specularAlbedo)[i];
    if (PACK) {
        float r = 0.0f;
        if (CLS == NRD_CLS_REBLUR) r = snorm16_to_f32(gptr<s4v>(a.normalRoughness)[i].w);
        const n4v d = nrd_out<n4v>(a.noisyDiffuse)[i], s = nrd_out<n4v>(a.noisySpecular)[i];
        nrd_out<n4v>(a.noisyDiffuse)[i] = nrd_pack_texel<CLS>(d, da, z, a.P, 1.0f);
        nrd_out<n4v>(a.noisySpecular)[i] = nrd_pack_texel<CLS>(s, sa, z, a.P, r);
    } else {
        const n4v d = gptr<n4v>(a.denoisedDiffuse)[i], s = gptr<n4v>(a.denoisedSpecular)[i];
        const n4v rad = nrd_out<n4v>(a.radiance)[i];
        nrd_out<n4v>(a.radiance)[i] = nrd_compose_texel<CLS>(rad, d, s, da, sa);
    }
}

// TWO = false: lane l owns pixel l. TWO = true: lane l owns pixels 2l and 2l + 1 and moves them with 16-byte accesses (the textures are
// 16-byte aligned: the host checked); an odd last pixel, and a pair of which only one pixel has a finite depth, take the one-pixel path.
template <bool PACK, int CLS, bool TWO>
__global__ __launch_bounds__(256) void k_nrd(NrdArgs a)
{
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (!TWO) {
        if (l < a.n) nrd_pixel<PACK, CLS>(a, l);
        return;
    }
    const uint32_t lanes = (a.n + 1u) >> 1;
    if (l >= lanes) return;
    const uint32_t i = 2u * l;
    if (i + 1u >= a.n) { nrd_pixel<PACK, CLS>(a, i); return; }
    const f2v z = gptr<f2v>(a.depth)[l];
    const bool f0 = isfinite(z.x), f1 = isfinite(z.y);
    if (!(f0 && f1)) {
        if (f0) nrd_pixel<PACK, CLS>(a, i);
        if (f1) nrd_pixel<PACK, CLS>(a, i + 1u);
        return;
    }
    const n8v da = gptr<n8v>(a.diffuseAlbedo)[l], sa = gptr<n8v>(a.specularAlbedo)[l];
    if (PACK) {
        float r0 = 0.0f, r1 = 0.0f;
        if (CLS == NRD_CLS_REBLUR) { const s8v nr = gptr<s8v>(a.normalRoughness)[l]; r0 = snorm16_to_f32(nr.s3); r1 = snorm16_to_f32(nr.s7); }
        const n8v d = nrd_out<n8v>(a.noisyDiffuse)[l], s = nrd_out<n8v>(a.noisySpecular)[l];
        nrd_out<n8v>(a.noisyDiffuse)[l] = cat4(nrd_pack_texel<CLS>(lo4(d), lo4(da), z.x, a.P, 1.0f), nrd_pack_texel<CLS>(hi4(d), hi4(da), z.y, a.P, 1.0f));
        nrd_out<n8v>(a.noisySpecular)[l] = cat4(nrd_pack_texel<CLS>(lo4(s), lo4(sa), z.x, a.P, r0), nrd_pack_texel<CLS>(hi4(s), hi4(sa), z.y, a.P, r1));
    } else {
        const n8v d = gptr<n8v>(a.denoisedDiffuse)[l], s = gptr<n8v>(a.denoisedSpecular)[l];
        const n8v rad = nrd_out<n8v>(a.radiance)[l];
        nrd_out<n8v>(a.radiance)[l] = cat4(nrd_compose_texel<CLS>(lo4(rad), lo4(d), lo4(s), lo4(da), lo4(sa)),
                                           nrd_compose_texel<CLS>(hi4(rad), hi4(d), hi4(s), hi4(da), hi4(sa)));
    }
}

} // namespace pt

using namespace pt;

static void launch_nrd(const NrdArgs& a, bool pack, int cls, bool two, hipStream_t stream)
{
    const uint32_t lanes = two ? (a.n + 1u) >> 1 : a.n;
    const dim3 grid((lanes + 255u) / 256u);
    auto forms = [&](auto PACK, auto CLS) {
        if (two) k_nrd<PACK(), CLS(), true><<<grid, 256, 0, stream>>>(a);
        else k_nrd<PACK(), CLS(), false><<<grid, 256, 0, stream>>>(a);
    };
    auto classes = [&](auto PACK) {
        if (cls == NRD_CLS_REBLUR) forms(PACK, std::integral_constant<int, NRD_CLS_REBLUR>{});
        else if (cls == NRD_CLS_RELAX) forms(PACK, std::integral_constant<int, NRD_CLS_RELAX>{});
        else forms(PACK, std::integral_constant<int, NRD_CLS_NONE>{});
    };
    if (pack) classes(std::true_type{}); else classes(std::false_type{});
}

extern "C" {

void pt_nrd_reblur_hit_distance_defaults(float out[4])
{
    if (!out) return;
    out[0] = 3.0f; out[1] = 0.1f; out[2] = 20.0f; out[3] = -25.0f;      // nrd::ReblurSettings().hitDistanceParameters: A, B, C, D
}

// The checks of a call, in the order their messages are reported: nullptr when it is accepted (*two: every texture it touches is aligned
// to two texels, so the two-pixel form runs), else the message of the refusal. Pointer values only: nothing is dereferenced.
static const char* nrd_check(const PtNRDCompositionConstants* k, const PtNRDCompositionTextures* t, bool* two)
{
    if (!k) return "constants is NULL";
    if (!t) return "textures is NULL";
    if (!(k->RenderSize[0] >= 1u && k->RenderSize[0] <= kNrdMaxSize && k->RenderSize[1] >= 1u && k->RenderSize[1] <= kNrdMaxSize))
        return "RenderSize must be 1..16384 on both axes";
    if (k->IsPack > 1u) return "IsPack must be 0 or 1";
    if (k->Denoiser > PT_DENOISER_NRD_RELAX) return "unknown Denoiser value";
    for (int i = 0; i < 4; ++i) if (!std::isfinite(k->ReBLURHitDistance[i])) return "ReBLURHitDistance must be finite";
    const bool pack = k->IsPack != 0, reblur = k->Denoiser == PT_DENOISER_NRD_REBLUR;
    if (!t->LinearDepth) return "LinearDepth is NULL";
    if (!t->DiffuseAlbedo) return "DiffuseAlbedo is NULL";
    if (!t->SpecularAlbedo) return "SpecularAlbedo is NULL";
    if (pack) {
        if (reblur && !t->NormalRoughness) return "NormalRoughness is NULL (the ReBLUR pack reads the roughness)";
        if (!t->NoisyDiffuse) return "NoisyDiffuse is NULL";
        if (!t->NoisySpecular) return "NoisySpecular is NULL";
    } else {
        if (!t->DenoisedDiffuse) return "DenoisedDiffuse is NULL";
        if (!t->DenoisedSpecular) return "DenoisedSpecular is NULL";
        if (!t->Radiance) return "Radiance is NULL";
    }
    // what this call touches, with the texel size of each
    const void* used[8]; uint32_t texel[8]; int nu = 0;
    auto use = [&](const void* p, uint32_t bytes) { used[nu] = p; texel[nu++] = bytes; };
    use(t->LinearDepth, 4); use(t->DiffuseAlbedo, 8); use(t->SpecularAlbedo, 8);
    if (pack) { if (reblur) use(t->NormalRoughness, 8); use(t->NoisyDiffuse, 8); use(t->NoisySpecular, 8); }
    else { use(t->DenoisedDiffuse, 8); use(t->DenoisedSpecular, 8); use(t->Radiance, 8); }
    bool aligned1 = true, aligned2 = true;
    for (int i = 0; i < nu; ++i) {
        aligned1 = aligned1 && ((uintptr_t)used[i] & (texel[i] - 1u)) == 0;
        aligned2 = aligned2 && ((uintptr_t)used[i] & (2u * texel[i] - 1u)) == 0;
    }
    if (!aligned1) return "textures must be aligned to their texel size (8 bytes; LinearDepth 4)";
    *two = aligned2;
    return nullptr;
}

int pt_nrd_composition_pixels_per_lane(const struct PtNRDCompositionConstants* k, const struct PtNRDCompositionTextures* t)
{
    bool two = false;
    return nrd_check(k, t, &two) ? 0 : two ? 2 : 1;
}

int pt_nrd_composition_process(PtContext* ctx, const struct PtNRDCompositionConstants* k, const struct PtNRDCompositionTextures* t)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    bool two = false;
    if (const char* refusal = nrd_check(k, t, &two)) return fail(&c, PT_ERROR_INVALID_ARGUMENT, refusal);
    const bool pack = k->IsPack != 0, reblur = k->Denoiser == PT_DENOISER_NRD_REBLUR;
    API_HIP(&c, hipSetDevice(c.device));

    NrdArgs a{};
    a.depth = (const float*)t->LinearDepth; a.diffuseAlbedo = t->DiffuseAlbedo; a.specularAlbedo = t->SpecularAlbedo;
    a.normalRoughness = t->NormalRoughness; a.noisyDiffuse = t->NoisyDiffuse; a.noisySpecular = t->NoisySpecular;
    a.denoisedDiffuse = t->DenoisedDiffuse; a.denoisedSpecular = t->DenoisedSpecular; a.radiance = t->Radiance;
    a.n = k->RenderSize[0] * k->RenderSize[1];
    for (int i = 0; i < 4; ++i) a.P[i] = k->ReBLURHitDistance[i];
    const int cls = reblur ? NRD_CLS_REBLUR : k->Denoiser == PT_DENOISER_NRD_RELAX ? NRD_CLS_RELAX : NRD_CLS_NONE;
    // the two-pixel form is the faster one where it differs ("NRD composition"); textures aligned to one texel only
    // (a view that starts at an odd pixel) take the one-pixel form
    launch_nrd(a, pack, cls, two, c.stream);
    API_HIP(&c, hipGetLastError());
    return PT_OK;
}

} // extern "C"
