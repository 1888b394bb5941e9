"""numpy restatement of the adaptive sharpener ("Sharpening"): the arbiter of tests/test_sharpen_*.py.

The pass is this library's own edge-adaptive sharpening filter for the image-scaling slot the reference fills with NVIDIA Image Scaling in
its sharpen mode: not a port of NVIDIA Image Scaling, unpinned against it. Every operation below is one IEEE float32 operation on arrays in
the order of the spec; the only fused operations are the two of ml_luminance (dot()), evaluated exactly by fma32, as in denoiseref. So it
restates the device bit for bit. Textures: Color and Sharpened uint16 fp16 bits (H, W, 4). An fp16 store rounds to nearest even."""
import numpy as np

import denoiseref as D

F = np.float32
DEFAULTS = {"Sharpness": 0.5, "ContrastFloor": 0.015625}
H5 = tuple(F(v) for v in (0.0625, 0.25, 0.375, 0.25, 0.0625))            # fl_h5(-2..2)
DIRECTIONS = ((1, 0), (0, 1), (1, 1), (1, -1))                             # d0..d3 as (dx, dy)
NEIGHBOURS = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1))     # the 3 x 3, row-major
ONE16 = 0x3C00

f16_to_f32, f_to_f16, fma32 = D.f16_to_f32, D.f_to_f16, D.fma32


def f16(x):
    """float values as fp16 bits"""
    return f_to_f16(np.asarray(x, F))


def frame(rgb):
    """an (H, W, 3) or (H, W) array of values as a Color texture: fp16 bits (H, W, 4), alpha 1"""
    rgb = np.asarray(rgb, np.float64)
    if rgb.ndim == 2:
        rgb = np.repeat(rgb[..., None], 3, -1)
    out = np.empty(rgb.shape[:2] + (4,), np.uint16)
    out[..., :3] = f16(rgb)
    out[..., 3] = ONE16
    return out


def guarded_rgb(bits):
    """fl_guard(fl_rgb16(q)): the three colour channels as float32, all 0 where one of them is not finite"""
    rgb = f16_to_f32(bits)[..., :3]
    return np.where(np.isfinite(rgb).all(-1, keepdims=True), rgb, F(0)).astype(F)


def luminance(c):
    """max0(ml_luminance(c)): mad(c.z, 0.114f, mad(c.y, 0.587f, c.x * 0.299f)), negative values and -0 to 0"""
    y = fma32(c[..., 2], F(0.114), fma32(c[..., 1], F(0.587), c[..., 0] * F(0.299)))
    return np.where(y > 0, y, F(0)).astype(F)


def tap(a, dx, dy):
    """a(p + (dx, dy)) for every pixel p, the coordinates clamped into the frame"""
    h, w = a.shape[:2]
    ys = np.clip(np.arange(h) + dy, 0, h - 1)
    xs = np.clip(np.arange(w) + dx, 0, w - 1)
    return a[ys][:, xs]


def sharpen(color, **overrides):
    """Color (H, W, 4) fp16 bits -> Sharpened, the same."""
    s = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    sharpness, floor = F(s["Sharpness"]), F(s["ContrastFloor"])
    color = np.asarray(color, np.uint16)
    with np.errstate(all="ignore"):
        c = guarded_rgb(color)
        Y = luminance(c)
        # 1: the range over the 3 x 3, row-major
        lo, hi, Ylo, Yhi = c.copy(), c.copy(), Y.copy(), Y.copy()
        first = True
        for dx, dy in NEIGHBOURS:
            t, ty = tap(c, dx, dy), tap(Y, dx, dy)
            if first:
                lo, hi, Ylo, Yhi, first = t, t, ty, ty, False
                continue
            lo = np.where(t < lo, t, lo); hi = np.where(t > hi, t, hi)
            Ylo = np.where(ty < Ylo, ty, Ylo); Yhi = np.where(ty > Yhi, ty, Yhi)
        # 2: contrast
        ssum = (Yhi + Ylo).astype(F)
        k = np.where(ssum > 0, ((Yhi - Ylo).astype(F) / ssum).astype(F), F(0)).astype(F)
        d = (k - floor).astype(F)
        ramp = (np.where(d > 0, d, F(0)).astype(F) / floor).astype(F)
        ramp = np.where(ramp < 1, ramp, F(1)).astype(F)
        amount = ((F(2) * sharpness) * ramp).astype(F)
        # 3: gradient energies
        e = []
        for n, (dx, dy) in enumerate(DIRECTIONS):
            g = (tap(Y, dx, dy) - tap(Y, -dx, -dy)).astype(F)
            ek = (g * g).astype(F)
            e.append((ek * F(0.5)).astype(F) if n >= 2 else ek)
        E = (((e[0] + e[1]).astype(F) + e[2]).astype(F) + e[3]).astype(F)
        # 4
        active = (amount > 0) & (E > 0)
        # 5, 6
        N = np.zeros(c.shape, F)
        for n, (dx, dy) in enumerate(DIRECTIONS):
            B = np.zeros(c.shape, F)
            for i in range(-2, 3):
                B = (B + (H5[i + 2] * tap(c, i * dx, i * dy)).astype(F)).astype(F)
            Hk = (c - B).astype(F)
            N = (N + (e[n][..., None] * Hk).astype(F)).astype(F)
        Dv = (N / E[..., None]).astype(F)
        # 7
        o = (c + (amount[..., None] * Dv).astype(F)).astype(F)
        o = np.where(o > lo, o, lo)
        o = np.where(o < hi, o, hi)
        o = np.where(active[..., None], o, c).astype(F)
    out = np.empty(color.shape, np.uint16)
    out[..., :3] = f_to_f16(o)
    out[..., 3] = ONE16
    return out


def active_mask(color, **overrides):
    """which pixels step 4 calls active (what the rule tests reason about): the output differs from the guarded input only there"""
    a = sharpen(color, **overrides)[..., :3]
    return (a != f_to_f16(guarded_rgb(color))).any(-1)


def hostile_frame(w, h, seed):
    """what the tests call a hostile frame: normal x 100, negatives, zeros, fp16 subnormals, +-65504, a +inf texel, a texel with one NaN
    channel, and (where there is room) a lone 6000 on a flat 0.2 wall"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((h, w, 4)) * 100).astype(np.float16)
    flat = v.reshape(-1, 4)
    n = flat.shape[0]
    pick = lambda count: rng.integers(0, n, max(1, min(count, n)))
    flat[pick(n // 7)] = 0
    flat[pick(n // 9), rng.integers(0, 3)] = np.float16(6e-8) * np.float16(rng.integers(1, 900))
    flat[pick(n // 11), rng.integers(0, 3)] = -np.float16(6e-8)
    flat[pick(n // 13), rng.integers(0, 3)] = np.float16(65504)
    flat[pick(n // 13), rng.integers(0, 3)] = np.float16(-65504)
    if n > 1:
        flat[pick(1)] = np.float16(np.inf)
        flat[pick(1), rng.integers(0, 3)] = np.float16(np.nan)
    v = flat.reshape(h, w, 4)
    if w >= 9 and h >= 9:                                        # the wall and its firefly, in the lower right corner
        v[h - 8:, w - 8:, :] = np.float16(0.2)
        v[h - 4, w - 4, :3] = np.float16(6000)
    if w >= 16 and h >= 4:                                       # a smooth patch: gradients below and around the contrast floor
        xs = np.arange(8, dtype=np.float32)
        v[0:4, 4:12, :] = (np.float16(1.0) + np.float16(0.01) * xs.astype(np.float16))[None, :, None]
    return v.view(np.uint16).copy()


def pattern(w=96, h=64):
    """edges in two directions and a band-limited wave: what a blur takes away and the pass is to give back"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([0.5 + 0.45 * np.sign(np.sin(0.35 * x + 0.2 * y)), 0.5 + 0.4 * np.sin(0.6 * x) * np.cos(0.4 * y),
                     0.3 + 0.25 * np.sign(np.cos(0.15 * (x - y)))], -1)


def blur121(a):
    """[1, 2, 1] / 4 once per axis, wrap-around"""
    for axis in (0, 1):
        a = (np.roll(a, 1, axis) + 2 * a + np.roll(a, -1, axis)) / 4
    return a


def ulp16(x):
    """the spacing of fp16 at |x| (normal range)"""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(x)) - 10)
