"""Restatement of the local-light PDF texture of the DI pass ("Local-light PDF texture"): the size rule, the Z-curve,
the mip chain of pt_mipmap_generate, the descent that fills the Power_RIS tiles and the source pdf of a light no tile produced. Float32
and integers throughout: every step the device takes is an IEEE add, subtract, multiply by 0.25, divide or compare, so the restatement
is meant to agree in bits. The RNG is the one presamplingref restates."""
import numpy as np

import presamplingref as P

f32 = np.float32
MAX_LIGHTS = 1 << 24
QUAD_ORDER_LEVELS = (1, 6, 11)                  # level indices summed a(0,0), a(0,1), a(1,0), a(1,1); every other one in Z order


# ---- size rule ---------------------------------------------------------------------------------------------------------------------
def _pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def _isqrt_ceil(n):
    r = int(np.floor(np.sqrt(float(n))))
    while r * r < n:
        r += 1
    while r > 0 and (r - 1) * (r - 1) >= n:
        r -= 1
    return r


def texture_size(n):
    """(width, height, mips) of the PDF texture of n lights; n = 0 counts as 1"""
    if not 0 <= n <= MAX_LIGHTS:
        raise ValueError("the light count must be 0..2^24")
    n = max(int(n), 1)
    width = _pow2_at_least(_isqrt_ceil(n))
    height = _pow2_at_least(-(-n // width))
    return width, height, max(width, height).bit_length()


def level_size(width, height, k):
    return max(1, width >> k), max(1, height >> k)


# ---- Z-curve -----------------------------------------------------------------------------------------------------------------------
def _compact(v):
    v = np.asarray(v, np.uint64) & np.uint64(0x55555555)
    for s, m in ((1, 0x33333333), (2, 0x0F0F0F0F), (4, 0x00FF00FF), (8, 0x0000FFFF)):
        v = (v | (v >> np.uint64(s))) & np.uint64(m)
    return v.astype(np.int64)


def _spread(v):
    v = np.asarray(v, np.uint64) & np.uint64(0x0000FFFF)
    for s, m in ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555)):
        v = (v | (v << np.uint64(s))) & np.uint64(m)
    return v


def zcurve(li):
    """light index -> (x, y): x takes the even bits, y the odd ones"""
    li = np.asarray(li, np.uint64)
    return _compact(li), _compact(li >> np.uint64(1))


def zindex(x, y):
    return (_spread(x) | (_spread(y) << np.uint64(1))).astype(np.int64)


def level0(power, width, height):
    """level 0 [height, width]: Power at zcurve(li), 0 elsewhere"""
    power = np.asarray(power, np.float32)
    out = np.zeros((height, width), np.float32)
    x, y = zcurve(np.arange(len(power)))
    out[y, x] = power
    return out


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def _padded(level):
    """the level with a zero row / column where its extent is 1, so that every 2 x 2 quad exists"""
    h, w = level.shape
    out = np.zeros((max(h, 2) if h % 2 else h, max(w, 2) if w % 2 else w), np.float32)
    out[:h, :w] = level
    return out


def next_level(level, index, quad_levels=QUAD_ORDER_LEVELS):
    """level `index` from level `index - 1` ([h, w] float32): a quarter of the quad's sum in the level's order"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = _padded(np.asarray(level, np.float32))
        a00, a10, a01, a11 = p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]        # a(i, j): x + i, y + j
        s = (a00, a01, a10, a11) if index in quad_levels else (a00, a10, a01, a11)
        v = (((s[0] + s[1]).astype(np.float32) + s[2]).astype(np.float32) + s[3]).astype(np.float32)
        return (v * f32(0.25)).astype(np.float32)


def build(level0_, mip_levels=None, quad_levels=QUAD_ORDER_LEVELS):
    """the levels of the chain, level 0 (the input, [height, width]) first; mip_levels None: the full chain"""
    level0_ = np.asarray(level0_, np.float32)
    h, w = level0_.shape
    full = max(w, h).bit_length()
    n = full if mip_levels is None else mip_levels
    levels = [level0_]
    for k in range(1, n):
        nxt = next_level(levels[-1], k, quad_levels)
        lw, lh = level_size(w, h, k)
        levels.append(np.ascontiguousarray(nxt[:lh, :lw]))
    return levels


# ---- the descent -------------------------------------------------------------------------------------------------------------------
def descend(levels, count, frame_index, entries=None):
    """k_di_presample_tiles_mip for entries g (None: all 128 * 1024): (LightIndex int64, -1 = empty; InvSourcePdf float32, 0 = empty)"""
    g = np.arange(P.TILE_COUNT * P.TILE_SIZE, dtype=np.uint64) if entries is None else np.asarray(entries, np.uint64)
    rng = P.rng_states(g & np.uint64(0xFFF), g >> np.uint64(12), frame_index, P.SALT_PRESAMPLE)
    n = len(g)
    px, py = np.zeros(n, np.int64), np.zeros(n, np.int64)
    pdf = np.ones(n, np.float32)
    live = np.ones(n, bool)                             # entries still descending; a dead one draws nothing more (its result is empty anyway)
    mips = len(levels)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for level in range(max(0, mips - 2), -1, -1):
            L = np.asarray(levels[level], np.float32)
            lh, lw = L.shape
            px, py = px * 2, py * 2

            def texel(x, y):
                inside = (x < lw) & (y < lh)
                t = np.where(inside, L[np.where(inside, y, 0), np.where(inside, x, 0)], f32(0)).astype(np.float32)
                return np.where(t > 0, t, f32(0)).astype(np.float32)              # max(0, NaN) = 0

            s0, s1, s2, s3 = texel(px, py), texel(px, py + 1), texel(px + 1, py), texel(px + 1, py + 1)
            total = (((s0 + s1).astype(np.float32) + s2).astype(np.float32) + s3).astype(np.float32)
            live &= (total > 0) & np.isfinite(total)
            p0, p1, p2, p3 = ((s / total).astype(np.float32) for s in (s0, s1, s2, s3))
            rng, r = P.rng_next(rng)
            t0 = r < p0
            r1 = (r - p0).astype(np.float32)
            t1 = ~t0 & (r1 < p1)
            r2 = (r1 - p1).astype(np.float32)
            t2 = ~t0 & ~t1 & (r2 < p2)
            t3 = ~t0 & ~t1 & ~t2
            px = px + (t2 | t3)
            py = py + (t1 | t3)
            taken = np.where(t0, p0, np.where(t1, p1, np.where(t2, p2, p3))).astype(np.float32)
            pdf = np.where(live, (pdf * taken).astype(np.float32), pdf).astype(np.float32)
        li = zindex(px, py)
        ok = live & (pdf > 0) & (li < count)
        inv = np.where(ok, (f32(1.0) / pdf).astype(np.float32), f32(0)).astype(np.float32)
    return np.where(ok, li, -1), inv


def source_pdf(power, levels):
    """RAB_EvaluateLocalLightSourcePdf: Power / ((top * M) * M), M = max(width, height), float32"""
    h, w = levels[0].shape
    M = f32(max(w, h))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        denominator = f32(f32(f32(levels[-1].reshape(-1)[0]) * M) * M)
        return (np.asarray(power, np.float32) / denominator).astype(np.float32)
