// pt_framegen.hip -- the library's own frame interpolator for the frame-generation slot of App::PostProcessGraphics (gfx950).
//
//   k_fg_scatter           one lane per render pixel: the surface it sees is carried along its motion vector to where it stands at phase
//                          phi between the previous frame and this one, and its key (depth bits << 32 | pixel index) goes into the cell of
//                          the midpoint field it lands in by one 64-bit atomic minimum: the nearest surface wins, then the lower index.
//   k_fg_resolve           one lane per output pixel, 16 x 16 tiles: the field entry of its cell (else the farthest of the 3 x 3), the two
//                          positions the surface has in the current and in the previous Color, four bilinear taps of each, a depth test of
//                          each against the frame it comes from, the blend; writes Generated, Generated8 and the class byte.
//   k_fg_first             the call without a previous frame: Generated is Color.
// Not a port of DLSS-G or FSR 3 (SDKs the reference tree does not carry) and unpinned against both: DESIGN.md section 1, "Frame
// generation", is the arithmetic spec and tests/framegenref.py restates it. Plain fp32 operations, one rounding each (-ffp-contract=off),
// nothing fused; no library transcendental. No optical flow, no UI or reactive mask, no presentation pacing.
#include "pt_filter.hpp"

namespace pt {

static_assert(sizeof(PtFrameGenerationSettings) == 48, "PtFrameGenerationSettings is 48 B (layouts.FRAME_GENERATION_SETTINGS, host/ptamd.hpp)");
static_assert(sizeof(PtFrameGenerationTextures) == 40, "PtFrameGenerationTextures is five pointers");

constexpr int kFgTile = kFlTile;                               // a workgroup of the resolve is one 16 x 16 tile of output pixels
constexpr int kFgLanes = 256;                                  // ... of the scatter 256 render pixels in index order
constexpr unsigned long long kFgEmpty = ~0ull;                 // a cell no surface landed in
constexpr uint32_t kFgSkyBits = 0x7F800000u;                   // the depth key of a sky pixel: the bits of +inf, behind every surface

struct FgArgs {
    const void* color; const float* depth; const void* motion;       // this frame
    const void* prevColor; const float* prevDepth;                    // the frame before it, context-owned
    unsigned long long* field; uint8_t* cls;
    void* generated; uint32_t* generated8;
    uint32_t Rw, Rh, Ow, Oh;
    float sx, sy, jx, jy, pjx, pjy;                            // s = RenderSize / OutputSize; this frame's jitter, the previous frame's
    float phi, omp, tau;                                       // Phase, 1 - Phase (one subtraction on the host), DepthThreshold
};

PT_DEV h4v fg_texel(u32x2 v) { return h4v{ (uint16_t)(v.x & 0xFFFFu), (uint16_t)(v.x >> 16), (uint16_t)(v.y & 0xFFFFu), (uint16_t)(v.y >> 16) }; }
PT_DEV v3 fg_colour(const void* tex, uint32_t j) { return fl_guard(fl_rgb16(fg_texel(gptr<u32x2>(tex)[j]))); }
// a depth that names no surface: not finite, or not in front of the camera
PT_DEV bool fg_sky(float z) { return !(isfinite(z) && z > 0.0f); }

__global__ __launch_bounds__(kFgLanes) void k_fg_scatter(FgArgs a)
{
    const uint32_t q = blockIdx.x * kFgLanes + threadIdx.x;
    if (q >= a.Rw * a.Rh) return;
    const uint32_t qx = q % a.Rw, qy = q / a.Rw;
    const float z = a.depth[q];
    const bool sky = fg_sky(z);
    float mvx = 0.0f, mvy = 0.0f;
    if (!sky) { const h4v m = fg_texel(gptr<u32x2>(a.motion)[q]); mvx = f16_to_f32(m.x); mvy = f16_to_f32(m.y); }
    if (!(isfinite(mvx) && isfinite(mvy))) return;
    const float xm = (((float)qx + 0.5f) + a.jx) + a.omp * mvx, ym = (((float)qy + 0.5f) + a.jy) + a.omp * mvy;
    const float cx = floorf(xm), cy = floorf(ym);
    if (!(cx >= 0.0f && cx <= (float)(a.Rw - 1u) && cy >= 0.0f && cy <= (float)(a.Rh - 1u))) return;
    const unsigned long long key = (unsigned long long)(sky ? kFgSkyBits : __float_as_uint(z)) << 32 | q;
    atomicMin(&a.field[(uint32_t)cy * a.Rw + (uint32_t)cx], key);
}

// The colour of a frame at the position (px, py) in output pixels: the four bilinear taps around it in the upscaler's order and weights, the
// taps outside the frame dropped and the rest renormalised. false when no weight is left.
PT_DEV bool fg_sample(const void* tex, float px, float py, uint32_t Ow, uint32_t Oh, float out[3])
{
    const FlTaps taps(px - 0.5f, py - 0.5f, Ow, Oh);
    float wsum = 0.0f, acc[3] = { 0.0f, 0.0f, 0.0f };
    for (int t = 0; t < 4; ++t) {
        if (!taps.inside(t)) continue;
        const float w = taps.weight(t);
        const v3 q = fg_colour(tex, taps.index(t));
        wsum = wsum + w;
        acc[0] = acc[0] + w * q.x; acc[1] = acc[1] + w * q.y; acc[2] = acc[2] + w * q.z;
    }
    if (!(wsum > 0.0f)) return false;
    out[0] = acc[0] / wsum; out[1] = acc[1] / wsum; out[2] = acc[2] / wsum;
    return true;
}

// the depth of a frame at its render sample nearest to the output position (px, py), under the jitter (jx, jy) the frame was rendered with
PT_DEV float fg_depth_at(const float* depth, const FgArgs& a, float px, float py, float jx, float jy)
{
    const uint32_t x = (uint32_t)fl_nearest(px, a.sx, jx, (float)(a.Rw - 1u)), y = (uint32_t)fl_nearest(py, a.sy, jy, (float)(a.Rh - 1u));
    return depth[y * a.Rw + x];
}

PT_DEV void fg_store(const FgArgs& a, uint32_t i, const float c[3], uint8_t cls)
{
    uint16_t c16[3];
    for (int ch = 0; ch < 3; ++ch) c16[ch] = f32_to_f16(c[ch] > kFlMax16 ? kFlMax16 : (c[ch] < -kFlMax16 ? -kFlMax16 : c[ch]));
    ((PT_GLOBAL_AS h4v*)a.generated)[i] = h4v{ c16[0], c16[1], c16[2], (uint16_t)0x3C00u };
    // the rule of the post chain's Display8: the stored fp16 values through f32_to_unorm8
    if (a.generated8)
        ((PT_GLOBAL_AS uint32_t*)a.generated8)[i] = (uint32_t)f32_to_unorm8(f16_to_f32(c16[0])) | (uint32_t)f32_to_unorm8(f16_to_f32(c16[1])) << 8 |
                                                    (uint32_t)f32_to_unorm8(f16_to_f32(c16[2])) << 16 | 0xFF000000u;
    a.cls[i] = cls;
}

__global__ __launch_bounds__(kFgTile * kFgTile) void k_fg_resolve(FgArgs a)
{
    const uint32_t ox = blockIdx.x * kFgTile + threadIdx.x, oy = blockIdx.y * kFgTile + threadIdx.y;
    if (ox >= a.Ow || oy >= a.Oh) return;
    const uint32_t i = oy * a.Ow + ox;
    const int Rw = (int)a.Rw, Rh = (int)a.Rh;
    const float oxc = (float)ox + 0.5f, oyc = (float)oy + 0.5f;

    // source: the entry of the cell the pixel lies in, else the farthest entry of the cell's 3 x 3
    const int cx = (int)fl_nearest(oxc, a.sx, 0.0f, (float)(Rw - 1)), cy = (int)fl_nearest(oyc, a.sy, 0.0f, (float)(Rh - 1));
    unsigned long long key = a.field[(uint32_t)cy * a.Rw + (uint32_t)cx];
    if (key == kFgEmpty) {
        bool found = false;
        for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
            const int x = cx + dx, y = cy + dy;
            if (x < 0 || x >= Rw || y < 0 || y >= Rh) continue;
            const unsigned long long k = a.field[(uint32_t)y * a.Rw + (uint32_t)x];
            if (k != kFgEmpty && (!found || k > key)) { key = k; found = true; }
        }
    }

    uint8_t cls = PT_FRAME_GENERATION_FALLBACK;
    float out[3];
    if (key != kFgEmpty) {
        const uint32_t q = (uint32_t)(key & 0xFFFFFFFFull), zbits = (uint32_t)(key >> 32);
        const bool sky = zbits == kFgSkyBits;
        const float z = __uint_as_float(zbits);
        float mvx = 0.0f, mvy = 0.0f, mvz = 0.0f;
        if (!sky) { const h4v m = fg_texel(gptr<u32x2>(a.motion)[q]); mvx = f16_to_f32(m.x); mvy = f16_to_f32(m.y); mvz = f16_to_f32(m.z); }
        const float Dx = mvx / a.sx, Dy = mvy / a.sy;
        const float pcx = oxc - a.omp * Dx, pcy = oyc - a.omp * Dy;
        const float ppx = oxc + a.phi * Dx, ppy = oyc + a.phi * Dy;
        float cur[3], prev[3];
        bool okc = fg_sample(a.color, pcx, pcy, a.Ow, a.Oh, cur), okp = fg_sample(a.prevColor, ppx, ppy, a.Ow, a.Oh, prev);
        const float zc = fg_depth_at(a.depth, a, pcx, pcy, a.jx, a.jy), zh = fg_depth_at(a.prevDepth, a, ppx, ppy, a.pjx, a.pjy);
        const float zp = z + mvz;
        okc = okc && (sky ? fg_sky(zc) : fabsf(zc - z) <= a.tau * fabsf(z));
        okp = okp && (sky ? fg_sky(zh) : fabsf(zh - zp) <= a.tau * fabsf(zp));
        if (okc && okp) { cls = PT_FRAME_GENERATION_BOTH; for (int ch = 0; ch < 3; ++ch) out[ch] = prev[ch] + (cur[ch] - prev[ch]) * a.phi; }
        else if (okc) { cls = PT_FRAME_GENERATION_CURRENT_ONLY; for (int ch = 0; ch < 3; ++ch) out[ch] = cur[ch]; }
        else if (okp) { cls = PT_FRAME_GENERATION_PREVIOUS_ONLY; for (int ch = 0; ch < 3; ++ch) out[ch] = prev[ch]; }
    }
    if (cls == PT_FRAME_GENERATION_FALLBACK) {                 // no surface, or neither sample stands: the blend without motion
        const v3 c = fg_colour(a.color, i), p = fg_colour(a.prevColor, i);
        out[0] = p.x + (c.x - p.x) * a.phi; out[1] = p.y + (c.y - p.y) * a.phi; out[2] = p.z + (c.z - p.z) * a.phi;
    }
    fg_store(a, i, out, cls);
}

// no previous frame: Generated is Color bit for bit, Generated8 its four channels by the same rule
__global__ __launch_bounds__(kFgLanes) void k_fg_first(const void* color, void* generated, uint32_t* generated8, uint32_t n)
{
    const uint32_t i = blockIdx.x * kFgLanes + threadIdx.x;
    if (i >= n) return;
    const u32x2 v = gptr<u32x2>(color)[i];
    ((PT_GLOBAL_AS u32x2*)generated)[i] = v;
    const h4v q = fg_texel(v);
    if (generated8)
        ((PT_GLOBAL_AS uint32_t*)generated8)[i] = (uint32_t)f32_to_unorm8(f16_to_f32(q.x)) | (uint32_t)f32_to_unorm8(f16_to_f32(q.y)) << 8 |
                                                  (uint32_t)f32_to_unorm8(f16_to_f32(q.z)) << 16 | (uint32_t)f32_to_unorm8(f16_to_f32(q.w)) << 24;
}

} // namespace pt

using namespace pt;

// nullptr when the settings are in range, else the message of the refusal
static const char* fg_check_settings(const PtFrameGenerationSettings* s)
{
    if (const char* refusal = fl_check_sizes(s->RenderSize, s->OutputSize)) return refusal;
    if (!(s->Phase > 0.0f && s->Phase < 1.0f)) return "Phase must be in (0, 1)";
    if (!(s->DepthThreshold > 0.0f && s->DepthThreshold <= 1.0f)) return "DepthThreshold must be in (0, 1]";
    return nullptr;
}

extern "C" {

int pt_frame_generation_set_constants(PtContext* ctx, const PtFrameGenerationSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    return fl_set_constants(ctx->c, s, fg_check_settings, ctx->c.fg, ctx->c.fgState);
}

int pt_frame_generation_reset_history(PtContext* ctx)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    ctx->c.fgState.frames = 0;
    return PT_OK;
}

int pt_frame_generation_process(PtContext* ctx, const struct PtFrameGenerationTextures* t, const float jitter[2], uint32_t* out_generated)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, t, "textures is NULL");
    API_ARG(&c, jitter, "jitter is NULL");
    API_ARG(&c, out_generated, "out_generated is NULL");
    if (!c.fgState.have) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "call pt_frame_generation_set_constants first");
    if (c.sharding.RankCount > 1u)
        return fail(&c, PT_ERROR_INVALID_ARGUMENT, "frame generation needs the whole frame: the context is sharded (run it on the gathered textures of an unsharded context)");
    const PtFrameGenerationSettings& s = c.fg;
    const size_t nr = (size_t)s.RenderSize[0] * s.RenderSize[1], no = (size_t)s.OutputSize[0] * s.OutputSize[1];
    const BoundTexture bound[4] = { { "Color", t->Color, 8 }, { "LinearDepth", t->LinearDepth, 4 }, { "MotionVector", t->MotionVector, 8 }, { "Generated", t->Generated, 8 } };
    if (int refusal = fl_check_bound(c, bound)) return refusal;
    if ((uintptr_t)t->Generated8 & 3u) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "Generated8 is not aligned to its texel (4 bytes)");
    // the outputs are written while the inputs are still read: Generated against the three inputs, Generated8 against those and Generated
    const size_t pixels[4] = { no, nr, nr, no };
    const struct { const char* name; const void* p; size_t bytes; int against; } outs[2] = { { "Generated", t->Generated, no * 8u, 3 }, { "Generated8", t->Generated8, no * 4u, 4 } };
    for (const auto& o : outs) {
        if (!o.p) continue;
        const uintptr_t out0 = (uintptr_t)o.p, out1 = out0 + o.bytes;
        for (int k = 0; k < o.against; ++k) {
            const uintptr_t in0 = (uintptr_t)bound[k].p, in1 = in0 + pixels[k] * bound[k].texel;
            if (in0 < out1 && out0 < in1) return fail(&c, PT_ERROR_INVALID_ARGUMENT, std::string(o.name) + " overlaps " + bound[k].name);
        }
    }
    if (int refusal = fl_check_jitter(c, jitter)) return refusal;
    API_HIP(&c, hipSetDevice(c.device));
    if (int e = fl_grow_history(c, c.fgState, want(c.fgPrevColor, no), want(c.fgPrevDepth, nr), want(c.fgField, nr), want(c.fgClass, no))) return e;

    const bool generate = c.fgState.frames != 0;
    if (generate) {
        FgArgs a{};
        a.color = t->Color; a.depth = (const float*)t->LinearDepth; a.motion = t->MotionVector;
        a.prevColor = c.fgPrevColor.data(); a.prevDepth = c.fgPrevDepth.data();
        a.field = (unsigned long long*)c.fgField.data(); a.cls = c.fgClass.data();
        a.generated = t->Generated; a.generated8 = (uint32_t*)t->Generated8;
        a.Rw = s.RenderSize[0]; a.Rh = s.RenderSize[1]; a.Ow = s.OutputSize[0]; a.Oh = s.OutputSize[1];
        a.sx = (float)a.Rw / (float)a.Ow; a.sy = (float)a.Rh / (float)a.Oh;
        a.jx = jitter[0]; a.jy = jitter[1]; a.pjx = c.fgPrevJitter[0]; a.pjy = c.fgPrevJitter[1];
        a.phi = s.Phase; a.omp = 1.0f - s.Phase; a.tau = s.DepthThreshold;
        API_HIP(&c, hipMemsetAsync(c.fgField.data(), 0xFF, nr * sizeof(uint64_t), c.stream));
        k_fg_scatter<<<dim3((unsigned)((nr + kFgLanes - 1) / kFgLanes)), dim3(kFgLanes), 0, c.stream>>>(a);
        API_HIP(&c, hipGetLastError());
        k_fg_resolve<<<dim3((a.Ow + kFgTile - 1) / kFgTile, (a.Oh + kFgTile - 1) / kFgTile), dim3(kFgTile, kFgTile), 0, c.stream>>>(a);
        API_HIP(&c, hipGetLastError());
    } else {
        k_fg_first<<<dim3((unsigned)((no + kFgLanes - 1) / kFgLanes)), dim3(kFgLanes), 0, c.stream>>>(t->Color, t->Generated, (uint32_t*)t->Generated8, (uint32_t)no);
        API_HIP(&c, hipGetLastError());
    }
    // the history: this frame, for the next call (the caller may overwrite its textures): 8 B per output pixel and 4 B per render pixel
    // read, and as many written
    API_HIP(&c, hipMemcpyAsync(c.fgPrevColor.data(), t->Color, no * 8u, hipMemcpyDeviceToDevice, c.stream));
    API_HIP(&c, hipMemcpyAsync(c.fgPrevDepth.data(), t->LinearDepth, nr * 4u, hipMemcpyDeviceToDevice, c.stream));
    c.fgPrevJitter[0] = jitter[0]; c.fgPrevJitter[1] = jitter[1];
    c.fgFieldValid = generate;
    c.fgState.advance(s.RenderSize[0], s.RenderSize[1], s.OutputSize[0], s.OutputSize[1]);
    *out_generated = generate ? 1u : 0u;
    return PT_OK;
}

int pt_frame_generation_download_field(PtContext* ctx, uint64_t* host_field, uint64_t capacity_render_pixels, uint8_t* host_class,
                                       uint64_t capacity_output_pixels, uint32_t render_out[2], uint32_t output_out[2])
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, render_out && output_out, "render_out / output_out is NULL");
    API_HIP(&c, hipSetDevice(c.device));
    API_HIP(&c, hipStreamSynchronize(c.stream));
    const bool valid = c.fgFieldValid && c.fgState.frames != 0;
    for (int k = 0; k < 2; ++k) { render_out[k] = valid ? c.fgState.size[k] : 0u; output_out[k] = valid ? c.fgState.size[2 + k] : 0u; }
    const size_t nr = (size_t)render_out[0] * render_out[1], no = (size_t)output_out[0] * output_out[1];
    const size_t fields = host_field ? (size_t)std::min<uint64_t>(capacity_render_pixels, nr) : 0;
    const size_t classes = host_class ? (size_t)std::min<uint64_t>(capacity_output_pixels, no) : 0;
    if (fields) API_HIP(&c, hipMemcpy(host_field, c.fgField.data(), fields * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (classes) API_HIP(&c, hipMemcpy(host_class, c.fgClass.data(), classes, hipMemcpyDeviceToHost));
    return PT_OK;
}

} // extern "C"
