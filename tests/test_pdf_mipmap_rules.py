"""CPU checks of the local-light PDF texture (pt_di_set_pdf_mipmap, pt_mipmap_generate): the library's size rule against the restatement
(tests/pdfmipref.py), the Z-curve, the per-level summation order, the chain's top against the float64 sum of the powers, the distribution
and the edge cases of the restatement's descent, and the exports against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pdfmipref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZES = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 1024, 1025, 1 << 20, (1 << 20) + 1, 1 << 24]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _chain(power):
    w, h, mips = M.texture_size(len(power))
    levels = M.build(M.level0(power, w, h))
    assert len(levels) == mips and levels[-1].shape == (1, 1)
    return levels


def test_size_rule_matches_the_library(ptamd):
    shapes = set()
    for n in SIZES:
        w, h, mips = M.texture_size(n)
        assert ptamd.pdf_texture_size(n) == (w, h, mips), n
        assert w & (w - 1) == 0 and h & (h - 1) == 0 and w * h >= max(n, 1) and w in (h, 2 * h), (n, w, h)
        assert mips == int(np.log2(max(w, h))) + 1
        if n > 1:
            assert (w // 2) * h < n or w == h and w * (h // 2) < n, "the texture is the smallest the rule allows"
        shapes.add(w == h)
    assert shapes == {True, False}                                       # square and 2:1 both occur
    assert M.texture_size(0) == M.texture_size(1) == (1, 1, 1)
    assert M.texture_size(5) == (4, 2, 3) and M.texture_size(17) == (8, 4, 4) and M.texture_size(1 << 20) == (1024, 1024, 11)
    with pytest.raises(ptamd.PtInvalidArgument):
        ptamd.pdf_texture_size((1 << 24) + 1)
    with pytest.raises(ValueError):
        M.texture_size((1 << 24) + 1)
    lib = ptamd.load_library()
    w = C.c_uint32(7)
    assert lib.pt_di_pdf_texture_size((1 << 24) + 1, C.byref(w), C.byref(w), C.byref(w)) != 0 and w.value == 7   # refused: nothing written
    assert lib.pt_di_pdf_texture_size(4, None, C.byref(w), C.byref(w)) != 0


def test_zcurve_round_trip_and_extent():
    li = np.arange((1 << 16) + 1)
    x, y = M.zcurve(li)
    assert np.array_equal(M.zindex(x, y), li)
    assert (int(x[0b1101]), int(y[0b1101])) == (0b11, 0b10)              # x: the even bits, y: the odd ones
    assert len(set(zip(x.tolist(), y.tolist()))) == len(li)
    for n in SIZES:
        if n == 0 or n > (1 << 16) + 1:
            continue
        w, h, _ = M.texture_size(n)
        assert x[:n].max() < w and y[:n].max() < h, n


def test_level_order_rule():
    """quad order a(0,0), a(0,1), a(1,0), a(1,1) at level 1 (and 6, 11), Z order a(0,0), a(1,0), a(0,1), a(1,1) elsewhere: with
    a(0,0) = 2^24, a(1,0) = 2, a(0,1) = 1 the first order gives 2^24 + 2 (the 1 is rounded away first), the second 2^24 + 4 (a tie to even)"""
    quad = np.array([[2.0 ** 24, 2.0], [1.0, 0.5]], f32)                 # [y, x]
    one = M.build(quad)
    assert float(one[1][0, 0]) == (2.0 ** 24 + 2.0) * 0.25
    assert float(M.build(quad, quad_levels=())[1][0, 0]) == (2.0 ** 24 + 4.0) * 0.25
    # the same quad one level up: each level-0 quad carries four times its level-1 value and three powers of two too small to count
    tex = np.zeros((4, 4), f32)
    tiny = iter(2.0 ** -np.arange(40, 52))
    for (qy, qx), v in np.ndenumerate(quad):
        tex[2 * qy, 2 * qx] = 4.0 * v
        for dy, dx in ((0, 1), (1, 0), (1, 1)):
            tex[2 * qy + dy, 2 * qx + dx] = next(tiny)
    assert len(set(tex.reshape(-1).tolist())) == 16 and np.all(np.log2(tex) == np.round(np.log2(tex)))   # distinct powers of two
    two = M.build(tex)
    assert np.array_equal(_bits(two[1]), _bits(quad))
    assert float(two[2][0, 0]) == (2.0 ** 24 + 4.0) * 0.25               # level 2: Z order
    assert float(M.build(tex, quad_levels=(1, 2))[2][0, 0]) == (2.0 ** 24 + 2.0) * 0.25
    assert M.QUAD_ORDER_LEVELS == (1, 6, 11)
    # level 6 switches back: a 64 x 64 texture whose level 5 is that quad
    big = np.zeros((64, 64), f32)
    for (qy, qx), v in np.ndenumerate(quad):
        big[32 * qy, 32 * qx] = v * 4.0 ** 5
    six = M.build(big)
    assert np.array_equal(_bits(six[5]), _bits(quad)) and float(six[6][0, 0]) == (2.0 ** 24 + 2.0) * 0.25


@pytest.mark.parametrize("n", [1000, 1500])
def test_top_times_m_squared_is_the_sum(n):
    """every level adds four values (three roundings, each within 2^-24 relative of a sum of positive terms) and scales by a power of
    two; the powers are positive, so a level's relative error is at most that of the level below plus 2 * 2^-24 to first order: the
    derived bound over the chain, (2 * mips + 2) * 2^-24"""
    rng = np.random.default_rng(20240 + n)
    power = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)).astype(f32)
    levels = _chain(power)
    h, w = levels[0].shape
    assert (w == h) == (n == 1000)                                       # 32 x 32 and 64 x 32
    m = max(w, h)
    top = float(levels[-1][0, 0]) * m * m
    exact = float(power.astype(np.float64).sum())
    assert abs(top - exact) <= (2 * len(levels) + 2) * 2.0 ** -24 * exact
    assert np.array_equal(_bits(M.source_pdf(power, levels)), _bits(power / f32(f32(levels[-1][0, 0] * f32(m)) * f32(m))))


def test_descent_distribution():
    rng = np.random.default_rng(7)
    power = np.exp(rng.uniform(0.0, np.log(1000.0), 64)).astype(f32)
    levels = _chain(power)
    li, inv = M.descend(levels, 64, 0)
    N = len(li)
    assert N == 131072 and li.min() >= 0 and np.all(inv > 0)             # no entry is empty
    p = power.astype(np.float64) / power.astype(np.float64).sum()
    counts = np.bincount(li, minlength=64)
    sigma = np.sqrt(N * p * (1 - p))
    z = np.abs(counts - N * p) / sigma
    assert z.max() < 5.0, z.max()
    # the stored inverse pdf is that of the light: the product of the branch probabilities is power / total to a few ulp per level
    assert np.allclose(1.0 / inv.astype(np.float64), p[li], rtol=len(levels) * 4 * 2.0 ** -24)


def test_descent_edges():
    entries = np.arange(4096, dtype=np.uint64)
    li, inv = M.descend(_chain(np.array([3.5], f32)), 1, 2, entries)     # n = 1: light 0, pdf 1
    assert np.all(li == 0) and np.all(inv == 1.0)
    li, inv = M.descend(_chain(np.zeros(37, f32)), 37, 2, entries)       # nothing to select: every entry empty
    assert np.all(li == -1) and np.all(inv == 0.0)
    one = np.zeros(37, f32); one[29] = 6.0
    li, inv = M.descend(_chain(one), 37, 2, entries)
    assert np.all(li == 29) and np.all(inv == 1.0)
    rng = np.random.default_rng(3)
    for bad in (np.nan, -4.0):
        power = rng.uniform(1.0, 2.0, 100).astype(f32)
        power[[5, 6]] = bad
        li, inv = M.descend(_chain(power), 100, 1, entries)
        assert not np.isin(li, [5, 6]).any() and (li >= 0).any()
        assert np.all((li >= 0) == (inv > 0)) and np.all(np.isfinite(inv))
    power = rng.uniform(1.0, 2.0, 100).astype(f32)
    power[17] = np.inf                                                   # the first sum of the descent is not finite: every entry empty
    li, inv = M.descend(_chain(power), 100, 1, entries)
    assert np.all(li == -1) and np.all(inv == 0.0)
    # a light index past the count is never handed out, whatever the texture holds there
    levels = _chain(np.ones(16, f32))
    li, _ = M.descend(levels, 10, 0, entries)
    assert li.max() < 10 and (li == -1).any()


def test_exports_and_header(ptamd):
    raw = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for decl in (r"int\s+pt_di_pdf_texture_size\(uint32_t light_count, uint32_t\* width, uint32_t\* height, uint32_t\* mip_levels\);",
                 r"int\s+pt_di_set_pdf_mipmap\(PtContext\* ctx, uint32_t enabled\);",
                 r"int\s+pt_di_download_pdf_texture\(PtContext\* ctx, uint32_t level, float\* host_dst, uint32_t capacity, uint32_t\* out_width, uint32_t\* out_height\);",
                 r"int\s+pt_mipmap_generate\(PtContext\* ctx, float\* const\* levels, uint32_t width, uint32_t height, uint32_t mip_levels\);"):
        assert re.search(decl, text), decl
    lib = ptamd.load_library()
    for sym in ("pt_di_pdf_texture_size", "pt_di_set_pdf_mipmap", "pt_di_download_pdf_texture", "pt_mipmap_generate"):
        assert sym in ptamd.EXPORTS and hasattr(lib, sym), sym
    # the feature added no struct to the C ABI: every typedef struct of the header is one the other layers already mirror
    import test_scene_specialisation as pinned                              # the struct list of the C ABI as the ABI tests pin it
    names = [n for n in re.findall(r"typedef struct (\w+)", raw) if n != "PtContext"]
    assert sorted(names) == sorted(pinned.STRUCT_SIZES) and not [n for n in names if re.search(r"mip|pdf", n, re.I)]
    assert lib.pt_abi_version() == 4
    for name in ("MipmapGeneration", "pdf_texture_size"):
        assert hasattr(ptamd, name)
    assert hasattr(ptamd.DirectLighting, "SetPdfMipmap") and hasattr(ptamd.DirectLighting, "download_pdf_texture")
