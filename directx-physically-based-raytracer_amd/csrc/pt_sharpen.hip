// pt_sharpen.hip -- the library's own edge-adaptive sharpening filter for the image-scaling slot of App::PostProcessGraphics (gfx950).
//
//   k_sharpen              one workgroup per 16 x 16 tile of pixels. The tile's 20 x 20 footprint (two texels of halo, the coordinates
//                          clamped into the frame while staging) goes through LDS once, one 16-byte record (r, g, b, Y) per texel: the
//                          8-byte load, the guard, the conversion and the luminance happen once per texel. Every lane then reads its 17
//                          taps (the 5 x 5's row, column and two diagonals) as 16-byte LDS reads, sharpens across the edge and not along
//                          it, limits the result to the 3 x 3 range of the input and stores one 8-byte texel.
// Not a port of NVIDIA Image Scaling (Streamline's NIS plugin, a binary the reference tree does not carry) and unpinned against it:
// DESIGN.md section 1, "Sharpening", is the arithmetic spec and tests/sharpenref.py restates it. Plain fp32 operations, one rounding each
// (-ffp-contract=off), nothing fused but the two operations of ml_luminance; no library transcendental. No scaler mode, no history.
#include "pt_filter.hpp"

namespace pt {

static_assert(sizeof(PtSharpenSettings) == 32, "PtSharpenSettings is 32 B (layouts.SHARPEN_SETTINGS, host/ptamd.hpp)");
static_assert(sizeof(PtSharpenTextures) == 16, "PtSharpenTextures is two pointers");

// How many pixels a lane sharpens. 1: a workgroup is one 16 x 16 tile, 20 x 20 records staged (1.56 per pixel). 2: a 32 x 16 tile, lane x
// takes the pixels x and x + 16 of its row one after the other, 36 x 20 records (1.41 per pixel). The same bytes either way; which one
// the library is built with is decided by DESIGN.md section 4, "Sharpening".
#ifndef PT_SHARPEN_PIXELS_PER_LANE
#define PT_SHARPEN_PIXELS_PER_LANE 1
#endif
constexpr int kShPixels = PT_SHARPEN_PIXELS_PER_LANE;
static_assert(kShPixels == 1 || kShPixels == 2, "one or two pixels a lane");
constexpr int kShTile = kFlTile;                               // 16 x 16 lanes
constexpr int kShTileW = kShTile * kShPixels;                  // pixels a workgroup covers along x
constexpr int kShHalo = 2;                                     // the taps reach two texels beyond the tile
constexpr int kShSide = kShTile + 2 * kShHalo, kShSideW = kShTileW + 2 * kShHalo;   // 20 rows of 20 (36) records staged
// The row stride of the LDS image, in 16-byte records. A wave is four rows of 16 lanes; ds_read_b128 serves it in four groups of 16 lanes,
// each group lanes 0-3 and 12-15 of one row and lanes 4-11 of the next (or the other way round), and a group is free of bank conflicts
// when its 16 records fall into 16 different 16-byte slots of the 256-byte bank row. With a stride that is a multiple of 16 records the
// second row's x = 4..11 land beside the first row's x = 0..3, 12..15: no conflict for any tap offset. The plain stride of 20 puts four
// lanes of every group on a slot another lane holds (2-way). 32 records: 20 rows x 512 B = 10 KB, no limit on occupancy (48 records
// and 15 KB with two pixels a lane, whose second pixel lies 16 records on: the same slots).
constexpr int kShStride = (kShSideW + 15) / 16 * 16;
constexpr float kShMinFloor = 0.0009765625f;                   // 2^-10

struct ShArgs {
    const void* color; void* sharpened;
    uint32_t W, H;
    float gain, floor;                                         // 2 Sharpness (exact, on the host), ContrastFloor
};

PT_DEV h4v sh_texel(u32x2 v) { return h4v{ (uint16_t)(v.x & 0xFFFFu), (uint16_t)(v.x >> 16), (uint16_t)(v.y & 0xFFFFu), (uint16_t)(v.y >> 16) }; }
typedef float f4v __attribute__((ext_vector_type(4)));       // one staged record: r, g, b, Y
// One tap: the whole 16-byte record in one ds_read_b128. The empty statement keeps all four words live, so the reads of the taps whose Y
// the arithmetic does not need are not narrowed to 12-byte ones, which the LDS serves in eight lane groups instead of four.
PT_DEV f4v sh_tap(const f4v* q) { f4v v = *q; asm("" : "+v"(v)); return v; }

// DESIGN.md section 1, "Sharpening", steps 1-7 for the pixel (ox, oy) inside the frame, whose staged record is *p
PT_DEV void sh_pixel(const ShArgs& a, const f4v* p, uint32_t ox, uint32_t oy)
{
    // the 17 taps: t[k][i + 2] = texel(p + i d_k), d0 = (1, 0), d1 = (0, 1), d2 = (1, 1), d3 = (1, -1)
    constexpr int dxs[4] = { 1, 0, 1, 1 }, dys[4] = { 0, 1, 1, -1 };
    const f4v c = sh_tap(p);
    f4v t[4][5];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = -2; i <= 2; ++i) t[k][i + 2] = i == 0 ? c : sh_tap(p + (i * dys[k]) * kShStride + i * dxs[k]);

    // 1: the range over the 3 x 3, row-major: (k, i) of the nine texels
    constexpr int rk[9] = { 2, 1, 3, 0, 0, 0, 3, 1, 2 }, ri[9] = { -1, -1, 1, -1, 0, 1, -1, 1, 1 };
    float lo[3], hi[3], Ylo, Yhi;
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        const f4v q = t[rk[n]][ri[n] + 2];
        if (n == 0) { for (int ch = 0; ch < 3; ++ch) lo[ch] = hi[ch] = q[ch]; Ylo = Yhi = q.w; continue; }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { const float v = q[ch]; lo[ch] = v < lo[ch] ? v : lo[ch]; hi[ch] = v > hi[ch] ? v : hi[ch]; }
        Ylo = q.w < Ylo ? q.w : Ylo; Yhi = q.w > Yhi ? q.w : Yhi;
    }
    // 2: contrast
    const float s = Yhi + Ylo;
    const float k = s > 0.0f ? (Yhi - Ylo) / s : 0.0f;
    float ramp = fl_max0(k - a.floor) / a.floor;
    ramp = ramp < 1.0f ? ramp : 1.0f;
    const float amount = a.gain * ramp;
    // 3: gradient energies
    float e[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const float g = t[kk][3].w - t[kk][1].w;
        e[kk] = g * g;
        if (kk >= 2) e[kk] = e[kk] * 0.5f;
    }
    const float E = ((e[0] + e[1]) + e[2]) + e[3];
    // 4 .. 7
    float o[3] = { c.x, c.y, c.z };
    if (amount > 0.0f && E > 0.0f) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float cc = c[ch];
            float N = 0.0f;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                float B = 0.0f;
#pragma unroll
                for (int i = -2; i <= 2; ++i) B = B + fl_h5(i) * t[kk][i + 2][ch];
                N = N + e[kk] * (cc - B);
            }
            float v = cc + amount * (N / E);
            v = v > lo[ch] ? v : lo[ch];
            v = v < hi[ch] ? v : hi[ch];
            o[ch] = v;
        }
    }
    ((PT_GLOBAL_AS h4v*)a.sharpened)[oy * a.W + ox] = h4v{ f32_to_f16(o[0]), f32_to_f16(o[1]), f32_to_f16(o[2]), (uint16_t)0x3C00u };
}

__global__ __launch_bounds__(kShTile * kShTile) void k_sharpen(ShArgs a)
{
    __shared__ f4v tile[kShSide * kShStride];
    const int lane = threadIdx.y * kShTile + threadIdx.x;
    const int x0 = (int)(blockIdx.x * kShTileW) - kShHalo, y0 = (int)(blockIdx.y * kShTile) - kShHalo;
    const int lastX = (int)a.W - 1, lastY = (int)a.H - 1;
    // staging: every lane, those outside the frame too; the clamp here is the replicate rule of every tap
    for (int t = lane; t < kShSideW * kShSide; t += kShTile * kShTile) {
        const int sx = t % kShSideW, sy = t / kShSideW;
        const int gx = min(max(x0 + sx, 0), lastX), gy = min(max(y0 + sy, 0), lastY);
        const v3 c = fl_guard(fl_rgb16(sh_texel(gptr<u32x2>(a.color)[(uint32_t)gy * a.W + (uint32_t)gx])));
        tile[sy * kShStride + sx] = f4v{ c.x, c.y, c.z, fl_max0(ml_luminance(c)) };
    }
    __syncthreads();
    const uint32_t oy = blockIdx.y * kShTile + threadIdx.y;
    if (oy >= a.H) return;
    for (int px = 0; px < kShPixels; ++px) {
        const int lx = (int)threadIdx.x + px * kShTile;
        const uint32_t ox = blockIdx.x * kShTileW + (uint32_t)lx;
        if (ox < a.W) sh_pixel(a, tile + ((int)threadIdx.y + kShHalo) * kShStride + (lx + kShHalo), ox, oy);
    }
}

} // namespace pt

using namespace pt;

// nullptr when the settings are in range, else the message of the refusal
static const char* sh_check_settings(const PtSharpenSettings* s)
{
    if (fl_check_sizes(s->Size)) return "Size must be 1..16384 on both axes";
    if (!(s->Sharpness >= 0.0f && s->Sharpness <= 1.0f)) return "Sharpness must be in [0, 1]";
    if (!(s->ContrastFloor >= kShMinFloor && s->ContrastFloor <= 0.5f)) return "ContrastFloor must be in [2^-10, 0.5]";
    return nullptr;
}

extern "C" {

int pt_sharpen_set_constants(PtContext* ctx, const PtSharpenSettings* s)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    return fl_set_constants(ctx->c, s, sh_check_settings, ctx->c.sh, ctx->c.shState);
}

int pt_sharpen_process(PtContext* ctx, const struct PtSharpenTextures* t)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    API_ARG(&c, t, "textures is NULL");
    if (!c.shState.have) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "call pt_sharpen_set_constants first");
    const PtSharpenSettings& s = c.sh;
    const BoundTexture bound[2] = { { "Color", t->Color, 8 }, { "Sharpened", t->Sharpened, 8 } };
    if (int refusal = fl_check_bound(c, bound)) return refusal;
    // every lane reads its neighbours' texels: an output that overlaps the input would be read after it was written
    const size_t bytes = (size_t)s.Size[0] * s.Size[1] * 8u;
    const uintptr_t in0 = (uintptr_t)t->Color, out0 = (uintptr_t)t->Sharpened;
    if (in0 < out0 + bytes && out0 < in0 + bytes) return fail(&c, PT_ERROR_INVALID_ARGUMENT, "Sharpened overlaps Color");
    API_HIP(&c, hipSetDevice(c.device));
    ShArgs a{};
    a.color = t->Color; a.sharpened = t->Sharpened;
    a.W = s.Size[0]; a.H = s.Size[1];
    a.gain = 2.0f * s.Sharpness; a.floor = s.ContrastFloor;
    k_sharpen<<<dim3((a.W + kShTileW - 1) / kShTileW, (a.H + kShTile - 1) / kShTile), dim3(kShTile, kShTile), 0, c.stream>>>(a);
    API_HIP(&c, hipGetLastError());
    return PT_OK;
}

} // extern "C"
