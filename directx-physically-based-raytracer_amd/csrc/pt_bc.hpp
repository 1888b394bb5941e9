// pt_bc.hpp -- block-compressed texture arithmetic (BC1, BC3, BC4, BC5): DESIGN.md "Arithmetic spec", the BC bullet.
//
// Plain functions over words that are already loaded: which block a texel lies in, and the code / value of texel i of a
// block. Nothing of HIP is included and no address space is named, so that a host program can include this file and be
// compared with the harness's bc.py bit for bit (tests/host/bc_decode.cpp). pt_texture.hpp does the loads.
//
//   texel (x, y) of a block is i = 4 (y & 3) + (x & 3); blocks are row-major, ceil(W / 4) per row, tightly packed
//   colour half   (BC1; bytes 8..15 of BC3): c0 | c1 << 16 (R5G6B5), then sixteen 2-bit indices, texel i at bits 2i
//   alpha block   (bytes 0..7 of BC3; BC4; each half of BC5): a0, a1, then 48 bits of 3-bit indices, texel i at bits 3i
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_BC_FN __host__ __device__ inline
#else
#define PT_BC_FN inline
#endif

namespace pt {
namespace bc {

PT_BC_FN uint64_t block_index(uint32_t W, uint32_t H, uint32_t face, uint32_t x, uint32_t y)
{
    const uint32_t bw = (W + 3u) >> 2, bh = (H + 3u) >> 2;
    return ((uint64_t)face * bh + (y >> 2)) * bw + (x >> 2);
}
PT_BC_FN uint32_t texel_in_block(uint32_t x, uint32_t y) { return 4u * (y & 3u) + (x & 3u); }

// r | g << 8 | b << 16 | a << 24 of texel i. w0 = c0 | c1 << 16, w1 = the index word. bc1: the three-colour mode exists (c0 <= c1),
// whose index 3 is transparent black; BC3's colour half is always four-colour. Endpoints expand by bit replication; the thirds are
// the exact rationals rounded to nearest (thirds never tie).
PT_BC_FN uint32_t color_code(uint32_t w0, uint32_t w1, uint32_t i, bool bc1)
{
    const uint32_t c0 = w0 & 0xFFFFu, c1 = w0 >> 16, k = (w1 >> (2u * i)) & 3u;
    const uint32_t r0 = (c0 >> 11) & 31u, g0 = (c0 >> 5) & 63u, b0 = c0 & 31u;
    const uint32_t r1 = (c1 >> 11) & 31u, g1 = (c1 >> 5) & 63u, b1 = c1 & 31u;
    const uint32_t e0[3] = { (r0 << 3) | (r0 >> 2), (g0 << 2) | (g0 >> 4), (b0 << 3) | (b0 >> 2) };
    const uint32_t e1[3] = { (r1 << 3) | (r1 >> 2), (g1 << 2) | (g1 >> 4), (b1 << 3) | (b1 >> 2) };
    const bool four = !bc1 || c0 > c1;
    if (!four && k == 3u) return 0u;
    uint32_t out = 0xFF000000u;
    for (int c = 0; c < 3; c++) {
        uint32_t v;
        if (k == 0u) v = e0[c];
        else if (k == 1u) v = e1[c];
        else if (four) v = (k == 2u ? 2u * e0[c] + e1[c] + 1u : e0[c] + 2u * e1[c] + 1u) / 3u;
        else v = (e0[c] + e1[c] + 1u) >> 1;
        out |= v << (8 * c);
    }
    return out;
}

// the 3-bit index of texel i of an alpha-layout block (w0 = bytes 0..3, w1 = bytes 4..7)
PT_BC_FN uint32_t alpha_index(uint32_t w0, uint32_t w1, uint32_t i)
{
    const uint64_t bits = (((uint64_t)w1 << 32) | w0) >> 16;
    return (uint32_t)(bits >> (3u * i)) & 7u;
}

// The interpolant of index k between a0 and a1 as a numerator over `den` (7 in the eight-value mode a0 > a1, 5 in the six-value
// mode): a0 -> a0 den, a1 -> a1 den, codes 2.. -> (den + 1 - k) a0 + (k - 1) a1. The six-value mode's codes 6 and 7 are the
// constants 0 and 1: fixed = 0 or 1 then (num is not meaningful), -1 otherwise.
PT_BC_FN uint32_t alpha_numerator(uint32_t a0, uint32_t a1, uint32_t k, uint32_t& den, int& fixed)
{
    den = a0 > a1 ? 7u : 5u; fixed = -1;
    if (k == 0u) return a0 * den;
    if (k == 1u) return a1 * den;
    if (den == 5u && k >= 6u) { fixed = (int)(k - 6u); return 0u; }
    return (den + 1u - k) * a0 + (k - 1u) * a1;
}

// BC3 alpha: the 8-bit code of texel i, integer division to nearest (sevenths and fifths never tie)
PT_BC_FN uint32_t alpha_code(uint32_t w0, uint32_t w1, uint32_t i)
{
    uint32_t den; int fixed;
    const uint32_t num = alpha_numerator(w0 & 0xFFu, (w0 >> 8) & 0xFFu, alpha_index(w0, w1, i), den, fixed);
    if (fixed >= 0) return fixed ? 255u : 0u;
    return (num + (den >> 1)) / den;
}

// BC4 / a half of BC5: the value of texel i keeps the interpolant's precision: the correctly rounded fp32 of num / (255 den),
// evaluated as this project evaluates x / c for a constant c (pt_math.hpp PT_DIV_CONST): in double, times the rounded reciprocal.
PT_BC_FN float bc4_value(uint32_t w0, uint32_t w1, uint32_t i)
{
    uint32_t den; int fixed;
    const uint32_t num = alpha_numerator(w0 & 0xFFu, (w0 >> 8) & 0xFFu, alpha_index(w0, w1, i), den, fixed);
    if (fixed >= 0) return fixed ? 1.0f : 0.0f;
    return den == 7u ? (float)((double)num * (1.0 / 1785.0)) : (float)((double)num * (1.0 / 1275.0));
}

} // namespace bc
} // namespace pt
