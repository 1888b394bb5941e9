// pt_mip.hip -- the mip chain of an R32_FLOAT texture (gfx950).
//
//   k_mip<VEC>  <- MipmapGeneration::SetTexture + Process (Source/MipmapGeneration.ixx), which App::PrepareReSTIRDI
//                  (Source/App.cpp:1095-1116) runs on the LocalLightPDF texture behind LightPreparation. One launch takes a source
//                  level s and writes up to five levels, s + 1 .. s + 5. VEC: a lane reads each row of its 2 x 2 source quad with
//                  one 8-byte load.
// The reference's shader is not restated: DESIGN.md section 1, "Local-light PDF texture", is the arithmetic spec (additions in a
// stated order and one multiplication by 0.25; tests/pdfmipref.py restates it).
//
// The block: 256 threads on a 32 x 32 tile of level s. Thread t sits at the Z-curve position of t inside the block's 16 x 16 texels
// of level s + 1 (x from the even bits of t, y from the odd ones), so lanes 4q .. 4q + 3 are a 2 x 2 quad in Z order, 16 lanes a
// 4 x 4 block and a wave an 8 x 8 block. Levels s + 2, s + 3 and s + 4 are three in-wave reductions (lane l reads lanes l + d, l + 2d,
// l + 3d; no LDS, no barrier); level s + 5 is the four wave results through LDS behind the one barrier.
// A texel outside its level reads as 0 and is never written: the levels of a 2:1 texture stay zero-padded to a square, and every
// access is checked against its level.
#include "pt_internal.hpp"

namespace pt {

constexpr uint32_t kMipMaxSize = 16384u;                       // D3D12_REQ_TEXTURE2D_U_OR_V_DIMENSION
constexpr uint32_t kMipMaxLevels = 16u;
constexpr uint32_t kMipLevelsPerLaunch = 5u;

typedef float mip2v __attribute__((ext_vector_type(2)));

struct MipArgs {
    const float* src; float* dst[kMipLevelsPerLaunch];
    uint32_t width, height;                                    // of the source level
    uint32_t levels;                                           // written by this launch: 1..5
};

PT_DEV uint32_t mip_even_bits(uint32_t v)                      // bits 0, 2, 4, 6 of v, packed
{
    v &= 0x55u; v = (v | (v >> 1)) & 0x33u; v = (v | (v >> 2)) & 0x0Fu;
    return v;
}
PT_DEV uint32_t mip_extent(uint32_t e, uint32_t k) { const uint32_t v = e >> k; return v ? v : 1u; }

// the quad sum of lanes l, l + d, l + 2d, l + 3d (Z order), valid in the lanes that are a multiple of 4d
PT_DEV float mip_reduce(float v, uint32_t d)
{
    const float s1 = __shfl_down(v, d), s2 = __shfl_down(v, 2u * d), s3 = __shfl_down(v, 3u * d);
    return (((v + s1) + s2) + s3) * 0.25f;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_mip(MipArgs a)
{
    const uint32_t t = threadIdx.x;
    const uint32_t x = blockIdx.x * 16u + mip_even_bits(t), y = blockIdx.y * 16u + mip_even_bits(t >> 1);   // the lane's texel of level s + 1
    const uint32_t sx = 2u * x, sy = 2u * y;
    // a(i, j) = source (sx + i, sy + j), 0 outside the level
    float a00 = 0.0f, a10 = 0.0f, a01 = 0.0f, a11 = 0.0f;
    if (sy < a.height && sx < a.width) {
        const float* r0 = a.src + (size_t)sy * a.width + sx;
        const bool right = sx + 1u < a.width, below = sy + 1u < a.height;
        if (VEC && right) {                                    // the width is even and the base 8-byte aligned: the host checked
            const mip2v u = *(const mip2v*)r0;
            a00 = u.x; a10 = u.y;
            if (below) { const mip2v w = *(const mip2v*)(r0 + a.width); a01 = w.x; a11 = w.y; }
        } else {
            a00 = r0[0];
            if (right) a10 = r0[1];
            if (below) { a01 = r0[a.width]; if (right) a11 = r0[a.width + 1u]; }
        }
    }
    // the first level of a launch (level index 1, 6, 11) sums its quad column by column; the in-wave levels behind it in Z order
    float v = (((a00 + a01) + a10) + a11) * 0.25f;
    uint32_t w = mip_extent(a.width, 1u), h = mip_extent(a.height, 1u);
    if (x < w && y < h) a.dst[0][(size_t)y * w + x] = v;
#pragma unroll
    for (uint32_t k = 1; k < 4u; k++) {                        // levels s + 2, s + 3, s + 4: lanes 4^k apart
        if (k >= a.levels) return;                             // uniform over the grid
        const uint32_t d = 1u << (2u * (k - 1u));
        v = mip_reduce(v, d);
        w = mip_extent(a.width, k + 1u); h = mip_extent(a.height, k + 1u);
        const uint32_t lx = x >> k, ly = y >> k;
        if ((t & (4u * d - 1u)) == 0u && lx < w && ly < h) a.dst[k][(size_t)ly * w + lx] = v;
    }
    if (a.levels < 5u) return;
    __shared__ float waves[4];                                 // the block's four texels of level s + 4, in Z order
    if ((t & 63u) == 0u) waves[t >> 6] = v;
    __syncthreads();
    if (t != 0u) return;
    w = mip_extent(a.width, 5u); h = mip_extent(a.height, 5u);
    if (blockIdx.x < w && blockIdx.y < h) a.dst[4][(size_t)blockIdx.y * w + blockIdx.x] = (((waves[0] + waves[1]) + waves[2]) + waves[3]) * 0.25f;
}

static bool mip_pow2(uint32_t v) { return v && !(v & (v - 1u)); }

// The checks of a call, in the order their messages are reported: nullptr when it is accepted.
static const char* mip_check(float* const* levels, uint32_t width, uint32_t height, uint32_t mips)
{
    if (!levels) return "levels is NULL";
    if (!(mip_pow2(width) && width <= kMipMaxSize)) return "width must be a power of two in 1..16384";
    if (!(mip_pow2(height) && height <= kMipMaxSize)) return "height must be a power of two in 1..16384";
    uint32_t full = 1;
    for (uint32_t e = std::max(width, height); e > 1u; e >>= 1) full++;
    if (!(mips >= 1u && mips <= kMipMaxLevels && mips <= full)) return "mip_levels must be 1..min(16, log2(max(width, height)) + 1)";
    for (uint32_t k = 0; k < mips; k++) {
        if (!levels[k]) return "a level is NULL";
        if ((uintptr_t)levels[k] & 3u) return "a level is not aligned to its texel (4 bytes)";
    }
    return nullptr;
}

// levels: a host array of device pointers. ceil((mips - 1) / 5) launches on the context's stream; mips = 1: none.
int mip_generate(Context& c, float* const* levels, uint32_t width, uint32_t height, uint32_t mips)
{
    if (const char* refusal = mip_check(levels, width, height, mips)) return fail(&c, PT_ERROR_INVALID_ARGUMENT, refusal);
    for (uint32_t s = 0; s + 1u < mips; s += kMipLevelsPerLaunch) {
        MipArgs a{};
        a.src = levels[s];
        a.width = std::max(1u, width >> s); a.height = std::max(1u, height >> s);
        a.levels = std::min(kMipLevelsPerLaunch, mips - 1u - s);
        for (uint32_t k = 0; k < a.levels; k++) a.dst[k] = levels[s + 1u + k];
        const dim3 grid((a.width + 31u) / 32u, (a.height + 31u) / 32u);
        if (a.width >= 2u && ((uintptr_t)a.src & 7u) == 0) k_mip<true><<<grid, 256, 0, c.stream>>>(a);
        else k_mip<false><<<grid, 256, 0, c.stream>>>(a);
    }
    API_HIP(&c, hipGetLastError());
    return PT_OK;
}

} // namespace pt

using namespace pt;

extern "C" {

int pt_mipmap_generate(PtContext* ctx, float* const* levels, uint32_t width, uint32_t height, uint32_t mip_levels)
{
    if (!ctx) return PT_ERROR_INVALID_ARGUMENT;
    Context& c = ctx->c;
    if (const char* refusal = mip_check(levels, width, height, mip_levels)) return fail(&c, PT_ERROR_INVALID_ARGUMENT, refusal);
    API_HIP(&c, hipSetDevice(c.device));
    return mip_generate(c, levels, width, height, mip_levels);
}

} // extern "C"
