// pt_upscale.hip -- the library's own temporal upscaler for the super-resolution slot of App::PostProcessGraphics (gfx950).
//
//   k_upscale<STAGED>      one lane per output pixel, 16 x 16 tiles: the nearest render sample, the 3 x 3 dilation of depth and motion, the
//                          kernel-weighted current colour and its clamp box, four validated bilinear taps of the previous output, the blend;
//                          writes Color and the new history parity. STAGED: the tile's render footprint and a one-texel halo (colour, depth,
//                          motion vector: 20 B a texel, at most 19 x 19 of them) go through LDS first, else every tap is a global load. Same
//                          taps, same order, same arithmetic: the same bits. The kernel is the staging and a tap source; the steps
//                          themselves are fl_resolve (pt_filter.hpp), which stage 4 of the reconstruction runs too.
// Not a port of DLSS or XeSS (closed SDKs the reference tree does not carry): DESIGN.md section 1, "Upscaler", is the arithmetic spec and
// tests/upscaleref.py restates it. Plain fp32 operations, one rounding each (-ffp-contract=off), nothing fused; no library transcendental.
// The two host helpers (the render size of a mode, the Halton jitter of a frame) need no GPU.
#include "pt_filter.hpp"

namespace pt {

constexpr int kUpTile = kFlTile;                               // a workgroup is one 16 x 16 tile of output pixels
constexpr int kUpSide = 20;                                    // the staged footprint: floor(15 s) + 2 samples and the halo, s <= 1: 19 a side

struct UpArgs { const void* radiance; const float* depth; const void* motion; FlResolveArgs r; };

PT_DEV h4v up_texel(u32x2 v) { return h4v{ (uint16_t)(v.x & 0xFFFFu), (uint16_t)(v.x >> 16), (uint16_t)(v.y & 0xFFFFu), (uint16_t)(v.y >> 16) }; }

// One render texel as a tap of fl_resolve sees it. The direct form: every tap is a global load; it has no LDS to name.
template <bool STAGED>
struct UpSource {
    const UpArgs& a;
    PT_DEV uint32_t at(int qx, int qy) const { return (uint32_t)qy * a.r.Rw + (uint32_t)qx; }
    PT_DEV float depth(uint32_t j) const { return a.depth[j]; }
    PT_DEV h4v motion(uint32_t j) const { return up_texel(gptr<u32x2>(a.motion)[j]); }
    PT_DEV v3 colour(uint32_t j) const { return fl_guard(fl_rgb16(up_texel(gptr<u32x2>(a.radiance)[j]))); }
};
// The staged form: from the footprint in LDS when the kernel did stage one (`staged`, the same in every lane), else from global memory.
template <>
struct UpSource<true> {
    const UpArgs& a;
    const u32x2 *ldsColour, *ldsMotion; const float* ldsDepth;
    int x0s, y0s, sw;
    bool staged;
    PT_DEV uint32_t at(int qx, int qy) const { return staged ? (uint32_t)((qy - y0s) * sw + (qx - x0s)) : (uint32_t)qy * a.r.Rw + (uint32_t)qx; }
    PT_DEV float depth(uint32_t j) const { return staged ? ldsDepth[j] : a.depth[j]; }
    PT_DEV h4v texel(bool motion, uint32_t j) const
    {
        u32x2 v;
        if (staged) v = motion ? ldsMotion[j] : ldsColour[j];
        else v = gptr<u32x2>(motion ? a.motion : a.radiance)[j];
        return up_texel(v);
    }
    PT_DEV h4v motion(uint32_t j) const { return texel(true, j); }
    PT_DEV v3 colour(uint32_t j) const { return fl_guard(fl_rgb16(texel(false, j))); }
};

template <bool STAGED>
__global__ __launch_bounds__(256) void k_upscale(UpArgs a)
{
    const FlResolveArgs& r = a.r;
    const int bx = blockIdx.x * kUpTile, by = blockIdx.y * kUpTile;
    const uint32_t ox = bx + threadIdx.x, oy = by + threadIdx.y;
    if constexpr (!STAGED) {
        if (ox < r.Ow && oy < r.Oh) fl_resolve(r, ox, oy, UpSource<false>{ a });
    } else {
        __shared__ u32x2 ldsColour[kUpSide * kUpSide];
        __shared__ u32x2 ldsMotion[kUpSide * kUpSide];
        __shared__ float ldsDepth[kUpSide * kUpSide];
        const int Rw = (int)r.Rw, Rh = (int)r.Rh;
        // the footprint of the tile: the nearest sample is monotone in the output coordinate, so the first and the last pixel of the tile
        // (inside the frame) bound every lane's; one more texel each way for the 3 x 3 taps, clipped to the frame
        const int lastX = min(bx + kUpTile - 1, (int)r.Ow - 1), lastY = min(by + kUpTile - 1, (int)r.Oh - 1);
        const int x0s = max((int)fl_nearest((float)bx + 0.5f, r.sx, r.jx, (float)(Rw - 1)) - 1, 0);
        const int y0s = max((int)fl_nearest((float)by + 0.5f, r.sy, r.jy, (float)(Rh - 1)) - 1, 0);
        const int x1s = min((int)fl_nearest((float)lastX + 0.5f, r.sx, r.jx, (float)(Rw - 1)) + 1, Rw - 1);
        const int y1s = min((int)fl_nearest((float)lastY + 0.5f, r.sy, r.jy, (float)(Rh - 1)) + 1, Rh - 1);
        const int sw = x1s - x0s + 1, sh = y1s - y0s + 1;
        const bool staged = sw <= kUpSide && sh <= kUpSide;               // always, while RenderSize <= OutputSize; the same in every lane
        if (staged) {
            for (int k = threadIdx.y * kUpTile + threadIdx.x; k < sw * sh; k += kUpTile * kUpTile) {
                const uint32_t j = (uint32_t)(y0s + k / sw) * r.Rw + (uint32_t)(x0s + k % sw);
                ldsColour[k] = gptr<u32x2>(a.radiance)[j]; ldsMotion[k] = gptr<u32x2>(a.motion)[j]; ldsDepth[k] = a.depth[j];
            }
        }
        __syncthreads();
        if (ox < r.Ow && oy < r.Oh) fl_resolve(r, ox, oy, UpSource<true>{ a, ldsColour, ldsMotion, ldsDepth, x0s, y0s, sw, staged });
    }
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
    if (const char* refusal = fl_check_sizes(s->RenderSize, s->OutputSize)) return refusal;
    if (!(s->MaxAccumulatedFrames >= 1u && s->MaxAccumulatedFrames <= 255u)) return "MaxAccumulatedFrames must be 1..255";
    if (!(s->KernelRadius >= 0.75f && s->KernelRadius <= 2.0f)) return "KernelRadius must be in [0.75, 2]";
    if (!(s->DepthThreshold > 0.0f && s->DepthThreshold <= 1.0f)) return "DepthThreshold must be in (0, 1]";
    return nullptr;
}

extern "C" {

int pt_upscaler_set_constants(PtContext* ctx, const PtUpscalerSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    return fl_set_constants(ctx->c, s, up_check_settings, ctx->c.up, ctx->c.upState);
}

int pt_upscaler_reset_history(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.upState.frames = 0;
    return PT_OK;
}

int pt_upscaler_process(PtContext* ctx, const struct PtUpscalerTextures* t, const float jitter[2])
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, t, "textures is NULL");
    API_ARG(&c, jitter, "jitter is NULL");
    if (!c.upState.have) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "call pt_upscaler_set_constants first");
    if (c.sharding.RankCount > 1u)
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "the upscaler needs the whole frame: the context is sharded (run it on the gathered textures of an unsharded context)");
    const BoundTexture bound[4] = { { "Radiance", t->Radiance, 8 }, { "LinearDepth", t->LinearDepth, 4 }, { "MotionVector", t->MotionVector, 8 }, { "Color", t->Color, 8 } };
    if (int refusal = fl_check_bound(c, bound)) return refusal;
    if (int refusal = fl_check_jitter(c, jitter)) return refusal;
    const PtUpscalerSettings& s = c.up;
    const size_t n = (size_t)s.OutputSize[0] * s.OutputSize[1];
    API_HIP(&c, hipSetDevice(c.device));
    if (int e = fl_grow_history(c, c.upState, want(c.upHistory, fl_output_slots(n)))) return e;
    UpArgs a{};
    a.radiance = t->Radiance; a.depth = (const float*)t->LinearDepth; a.motion = t->MotionVector;
    a.r = fl_resolve_args(c.upState, c.upHistory.data(), t->Color, s.RenderSize, s.OutputSize, jitter, s.MaxAccumulatedFrames, s.KernelRadius, s.DepthThreshold);
    const dim3 grid((a.r.Ow + kUpTile - 1) / kUpTile, (a.r.Oh + kUpTile - 1) / kUpTile), block(kUpTile, kUpTile);
    if (up_staged(c)) k_upscale<true><<<grid, block, 0, c.stream>>>(a);
    else k_upscale<false><<<grid, block, 0, c.stream>>>(a);
    API_HIP(&c, hipGetLastError());
    c.upState.advance(a.r.Ow, a.r.Oh);
    return PT_OK;
}

int pt_upscaler_download_history(PtContext* ctx, float* host_length, uint64_t capacity_pixels, uint32_t* out_w, uint32_t* out_h)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, out_w && out_h && (host_length || capacity_pixels == 0), "out_w / out_h / host_length is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    *out_w = c.upState.shown(0); *out_h = c.upState.shown(1);
    const size_t n = (size_t)*out_w * *out_h;
    const size_t count = (size_t)std::min<uint64_t>(capacity_pixels, n);
    return count ? fl_download_w(c, c.upHistory.data() + n * c.upState.parity, count, host_length) : PT_OK;
}

int pt_upscaler_render_size(uint32_t mode, const uint32_t output[2], uint32_t render_out[2])
{
    if (!output || !render_out) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "output / render_out is NULL");
    if (mode > PT_SUPER_RESOLUTION_ULTRA_PERFORMANCE) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "mode must be a PtSuperResolutionMode value");
    for (int k = 0; k < 2; ++k) if (!(output[k] >= 1u && output[k] <= kFlMaxSize)) return fail(nullptr, PT_ERROR_INVALID_ARGUMENT, "output must be 1..16384 on both axes");
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
    for (int k = 0; k < 2; ++k) if (!(render[k] >= 1u && render[k] <= kFlMaxSize && output[k] >= 1u && output[k] <= kFlMaxSize))
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
