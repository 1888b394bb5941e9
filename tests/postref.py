"""An independent numpy restatement of the post-processing spec ("Post-processing"): Bloom + Merge, DirectXTK's
ToneMapPostProcess, the back-buffer copy.

Reference: Shaders/Bloom.hlsl (Downsample :33-93, Upsample :95-115, main :117-143), Source/Bloom.ixx:87-124 (stage order, ping-pong,
UpsamplingFilterRadius 5e-3), Shaders/Merge.hlsl:24-34, Math::CalculateUV (Shaders/Math.hlsli:7-10), Source/App.cpp:1769-1812
(ProcessBloom, ToneMap, CopyTexture). Unpinned (not in the reference tree): Color::ToSrgb / Luminance (MathLib) and DirectXTK's
formulas and rotation matrices.

Arithmetic: float32 where the device's outcome is discrete or bit-exact (texel coordinates and bilinear weights, the filter sums, the
fma chains), emulating fmaf exactly (float64 product, round-to-odd float64 sum, one rounding to float32). Float64 where the device calls
powf (the Karis weight, the sRGB estimate, ST.2084): those results are compared within stated fp16-ulp bounds.

MUTATIONS each break one rule; tests/test_post_processing_gpu.py shows every one of them exceeds the bounds against the device.
"""
import numpy as np

F32 = np.float32
STAGES = 9
MIPS = 5
UPSAMPLE_RADIUS = F32(5e-3)
ROTATIONS = [  # DirectXTK ToneMapPostProcess, rows for column vectors
    [[0.6274040, 0.3292820, 0.0433136], [0.0690970, 0.9195400, 0.0113612], [0.0163916, 0.0880132, 0.8955950]],          # 709 -> 2020
    [[0.753845, 0.198593, 0.047562], [0.0457456, 0.941777, 0.0124772], [-0.00121055, 0.0176041, 0.983607]],              # P3-D65 -> 2020
    [[0.822461969, 0.1775380, 0.0], [0.033194199, 0.9668058, 0.0], [0.017082631, 0.0723974, 0.9105199]],                 # 709 -> P3-D65
]
PQ = dict(m1=0.1593017578125, m2=78.84375, c1=0.8359375, c2=18.8515625, c3=18.6875)
SATURATE, REINHARD, ACES_FILMIC = 1, 2, 3

MUTATIONS = [
    "karis_stage0_only",        # the learnopengl reading: Karis on the first downsample only (the reference's stage 1 has InputMipLevel 0 too)
    "offsets_input_texels",     # downsample g_size = 1 / dims_in instead of 1 / dims_out
    "radius_in_texels",         # upsample radius of one input texel instead of 5e-3 in UV units
    "additive_upsample",        # the up chain adds to the down chain's level instead of replacing it
    "no_floor",                 # Karis sum without max(., 1e-4)
    "unclamped_srgb",           # ToSrgb without its saturate
    "bt709_luminance",          # Rec.709 luminance weights instead of BT.601
    "fp32_levels",              # pyramid levels kept in fp32 (no fp16 store between stages)
    "wrap_addressing",          # WRAP instead of CLAMP
    "swapped_merge_weights",    # Strength on Radiance, 1 - Strength on the bloom
    "linear_exposure",          # x * (1 + Exposure) instead of x * exp2(Exposure)
    "exact_srgb",               # the piecewise sRGB OETF instead of pow(x, 1/2.2)
    "unsaturated_aces",         # ACES filmic without its saturate
    "hdr_no_rotation",          # HDR10 without the colour-primary rotation
    "unorm_no_half",            # FLOAT -> UNORM truncation without the + 0.5
]


# ---- float32 arithmetic ------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fmaf(a, b, c) exactly: the float64 product of two float32 values is exact; the float64 sum is made round-to-odd (TwoSum error
    term), so the final rounding to float32 is the single rounding of the exact a * b + c."""
    a, b, c = (np.asarray(x, F32) for x in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        odd = (s.view(np.int64) & 1) == 1
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def f16(x):
    """FLOAT -> fp16 bits, round-to-nearest-even, overflow to inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, F32).astype(np.float16).view(np.uint16)


def h2f(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(F32)


def unorm(x, n, mut=()):
    """D3D11.3 FLOAT -> UNORMn: NaN -> 0, clamp to [0, 1], x (2^n - 1) (rounded), + 0.5 (rounded), truncate."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        y = np.fmin(np.fmax(x, F32(0)), F32(1)) * F32((1 << n) - 1)
        if "unorm_no_half" not in mut:
            y = y + F32(0.5)
    y = np.where(np.isnan(x), F32(0), y)
    return np.floor(y).astype(np.uint32)


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
def stage_mip(s):
    return s if s < MIPS else 2 * (MIPS - 1) - s


def level_dims(width, height):
    """(w, h) of mip 0..4: mip 0 = (W/2, H/2) by integer division, mip k = max(1, mip0 >> k)."""
    return [(max(1, (width // 2) >> k), max(1, (height // 2) >> k)) for k in range(MIPS)]


def stage_table(width, height):
    """[(kind, karis, input dims, output dims)] of stages 0..8 (Bloom.ixx:87-124)."""
    mips = level_dims(width, height)
    out = []
    for s in range(STAGES):
        din = (width, height) if s == 0 else mips[stage_mip(s - 1)]
        kind = "down" if s < MIPS else "up"
        out.append((kind, s < 2, din, mips[stage_mip(s)]))
    return out


def bloom_size_ok(width, height):
    return width >= 2 and height >= 2 and max(width, height) >= 32


# ---- sampling --------------------------------------------------------------------------------------------------------------------
def bilinear(tex, u, v, mut=()):
    """SampleLevel(linear, CLAMP, 0) of tex (h, w, 3) float32 at float32 UVs: fx = u * W - 0.5 (two roundings), weights fx - floor(fx);
    lerp = fma(c1, w, c0 * (1 - w)), x first."""
    H, W = tex.shape[:2]
    fx = u * F32(W) - F32(0.5)
    fy = v * F32(H) - F32(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    wx, wy = (fx - x0f)[..., None], (fy - y0f)[..., None]
    xa, ya = x0f.astype(np.int64), y0f.astype(np.int64)
    if "wrap_addressing" in mut:
        x0, x1, y0, y1 = xa % W, (xa + 1) % W, ya % H, (ya + 1) % H
    else:
        x0, x1 = np.clip(xa, 0, W - 1), np.clip(xa + 1, 0, W - 1)
        y0, y1 = np.clip(ya, 0, H - 1), np.clip(ya + 1, 0, H - 1)
    c00, c10, c01, c11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    ix, iy = F32(1) - wx, F32(1) - wy
    with np.errstate(invalid="ignore", over="ignore"):
        top = fma(c10, wx, c00 * ix)
        bot = fma(c11, wx, c01 * ix)
        return fma(bot, wy, top * iy)


def output_uv(w, h):
    """Math::CalculateUV of every texel of a (w, h) output: ((p + 0.5) / dims) in float32."""
    x = np.arange(w, dtype=F32)[None, :]
    y = np.arange(h, dtype=F32)[:, None]
    u = np.broadcast_to((x + F32(0.5)) / F32(w), (h, w))
    v = np.broadcast_to((y + F32(0.5)) / F32(h), (h, w))
    return u, v


def _sum(*xs):
    out = xs[0]
    with np.errstate(invalid="ignore", over="ignore"):
        for x in xs[1:]:
            out = out + x
    return out


# ---- bloom -----------------------------------------------------------------------------------------------------------------------
def to_srgb(x, mut=()):
    """[unpinned] Color::ToSrgb: saturate, then x < 0.0031308 ? 12.92 x : 1.055 x^0.41666 - 0.055 (float64)."""
    x = np.asarray(x, np.float64)
    if "unclamped_srgb" not in mut:
        x = np.fmin(np.fmax(x, 0.0), 1.0)
    with np.errstate(invalid="ignore"):
        return np.where(x < np.float64(F32(0.0031308)), np.float64(F32(12.92)) * x,
                        np.float64(F32(1.055)) * np.power(np.abs(x), np.float64(F32(0.41666))) - np.float64(F32(0.055)))


def luminance(c, mut=()):
    w = (0.2126, 0.7152, 0.0722) if "bt709_luminance" in mut else (F32(0.299), F32(0.587), F32(0.114))
    return c[..., 0] * np.float64(w[0]) + c[..., 1] * np.float64(w[1]) + c[..., 2] * np.float64(w[2])


def downsample(src, dims_out, karis, mut=()):
    """Bloom.hlsl Downsample at every texel of a dims_out level, reading src (h, w, 3) float32. Returns float32 (non-Karis, bit-exact)
    or float64 (Karis: powf on the device)."""
    wo, ho = dims_out
    hi, wi = src.shape[:2]
    u, v = output_uv(wo, ho)
    sx, sy = (F32(1) / F32(wi), F32(1) / F32(hi)) if "offsets_input_texels" in mut else (F32(1) / F32(wo), F32(1) / F32(ho))

    def S(dx, dy):
        return bilinear(src, fma(sx, F32(dx), u), fma(sy, F32(dy), v), mut)
    a, b, c, d, e, f = S(-2, 2), S(0, 2), S(2, 2), S(-2, 0), S(0, 0), S(2, 0)
    g, h, i, j, k, l, m = S(-2, -2), S(0, -2), S(2, -2), S(-1, 1), S(1, 1), S(-1, -1), S(1, -1)
    if not karis:
        with np.errstate(invalid="ignore", over="ignore"):
            r = fma(_sum(a, c, g, i), F32(0.03125), e * F32(0.125))
            r = fma(_sum(b, d, f, h), F32(0.0625), r)
            return fma(_sum(j, k, l, m), F32(0.125), r)
    D = [x.astype(np.float64) for x in (a, b, c, d, e, f, g, h, i, j, k, l, m)]
    a, b, c, d, e, f, g, h, i, j, k, l, m = D
    with np.errstate(invalid="ignore", over="ignore"):
        groups = [(a + b + d + e) * 0.03125, (b + c + e + f) * 0.03125, (d + e + g + h) * 0.03125, (e + f + h + i) * 0.03125,
                  (j + k + l + m) * 0.125]
        out = 0.0
        for grp in groups:
            out = out + grp * (1.0 / (1.0 + luminance(to_srgb(grp, mut), mut) * 0.25))[..., None]
    return out if "no_floor" in mut else np.fmax(out, np.float64(F32(1e-4)))


def upsample(src, dims_out, mut=()):
    """Bloom.hlsl Upsample: 3 x 3 tent at a fixed UV radius of 5e-3, float32, bit-exact."""
    wo, ho = dims_out
    hi, wi = src.shape[:2]
    u, v = output_uv(wo, ho)
    rx, ry = (F32(1) / F32(wi), F32(1) / F32(hi)) if "radius_in_texels" in mut else (UPSAMPLE_RADIUS, UPSAMPLE_RADIUS)

    def S(dx, dy):
        return bilinear(src, fma(rx, F32(dx), u), fma(ry, F32(dy), v), mut)
    a, b, c, d, e, f = S(-1, 1), S(0, 1), S(1, 1), S(-1, 0), S(0, 0), S(1, 0)
    g, h, i = S(-1, -1), S(0, -1), S(1, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        r = fma(_sum(b, d, f, h), F32(2), e * F32(4))
        return _sum(r, a, c, g, i) * F32(0.0625)


def store_level(x, mut=()):
    """the fp16 store of a level (float3 store: 4th channel 0) as the next stage reads it: float32 values; fp32_levels keeps them."""
    if "fp32_levels" in mut:
        return np.asarray(x, F32)
    return h2f(f16(x))


def stage(s, src, dims_out, mut=(), down_level=None):
    """stage s of the table on src (h, w, 3) float32: the unrounded result (float32 or float64). down_level: the image the down chain
    left in the output slot (only for the additive_upsample mutation)."""
    if s < MIPS:
        karis = s < 2 and not (s == 1 and "karis_stage0_only" in mut)
        return downsample(src, dims_out, karis, mut)
    r = upsample(src, dims_out, mut)
    if "additive_upsample" in mut and down_level is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            r = r + down_level
    return r


def bloom(radiance, mut=()):
    """The nine stage images (fp16 bits, (h, w, 4) with alpha 0) for radiance (H, W, 4) fp16 bits."""
    H, W = radiance.shape[:2]
    table = stage_table(W, H)
    src = h2f(radiance[..., :3])
    images, levels = [], []
    for s, (_, _, _, dout) in enumerate(table):
        down = levels[2 * (MIPS - 1) - s] if s >= MIPS else None
        r = stage(s, src, dout, mut, down)
        src = store_level(r, mut)
        levels.append(src)
        images.append(np.concatenate([f16(r), np.zeros(r.shape[:2] + (1,), np.uint16)], axis=-1))
    return images


# ---- merge, tone map, encodes ----------------------------------------------------------------------------------------------------
def merge(radiance, blur, strength, mut=()):
    """Merge.hlsl: fma(Blur1_0(UV), S, Radiance(UV) (1 - S)), both bilinear at the output UV; float32 (not yet stored)."""
    H, W = radiance.shape[:2]
    u, v = output_uv(W, H)
    s = F32(strength)
    w1, w2 = F32(1) - s, s
    if "swapped_merge_weights" in mut:
        w1, w2 = w2, w1
    r = bilinear(h2f(radiance[..., :3]), u, v, mut)
    b = bilinear(h2f(blur[..., :3]), u, v, mut)
    with np.errstate(invalid="ignore", over="ignore"):
        return fma(b, w2, r * w1)


def tone_map(m, settings, mut=()):
    """ToneMapPostProcess on float32 colours m (..., 3): the value stored to Color, before its fp16 rounding (float64)."""
    s = np.asarray(settings).reshape(())
    m = np.asarray(m, F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if int(s["IsHDREnabled"]):
            M = np.array(ROTATIONS[int(s["ColorPrimaryRotation"])], np.float32).astype(np.float64)
            r = m.astype(np.float64) @ M.T if "hdr_no_rotation" not in mut else m.astype(np.float64)
            n = np.abs(r * np.float64(F32(float(s["PaperWhiteNits"]) / 10000.0)))
            p = np.power(n, PQ["m1"])
            return np.power((PQ["c1"] + PQ["c2"] * p) / (1.0 + PQ["c3"] * p), PQ["m2"])
        e = float(np.float32(s["Exposure"]))
        scale = F32(1.0 + e) if "linear_exposure" in mut else F32(2.0 ** e)
        x = (m * scale).astype(np.float64)          # the product is one float32 rounding on the device
        op = int(s["ToneMappingOperator"])
        if op == SATURATE:
            t = np.fmin(np.fmax(x, 0.0), 1.0)
        elif op == REINHARD:
            t = x / (1.0 + x)
        else:
            t = x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)
            if "unsaturated_aces" not in mut:
                t = np.fmin(np.fmax(t, 0.0), 1.0)
        if "exact_srgb" in mut:
            t = np.abs(t)
            return np.where(t <= 0.0031308, 12.92 * t, 1.055 * np.power(t, 1 / 2.4) - 0.055)
        return np.power(np.abs(t), np.float64(F32(0.454545454545)))


def resolve(radiance, blur, settings, mut=()):
    """Color, BackBuffer, Display8 of the one-pass resolve: radiance (H, W, 4) fp16 bits; blur: stage 8's image or None (bloom off)."""
    s = np.asarray(settings).reshape(())
    if int(s["IsBloomEnabled"]):
        m = h2f(f16(merge(radiance, blur, float(s["BloomStrength"]), mut)))          # Merge writes Color (fp16)
        alpha = np.zeros(radiance.shape[:2], np.uint16)
    else:
        m = h2f(radiance[..., :3])
        alpha = radiance[..., 3]
    color = np.concatenate([f16(tone_map(m, s, mut)), alpha[..., None]], axis=-1)
    return (color,) + encode(color, mut)


def encode(color, mut=()):
    """BackBuffer (R10G10B10A2_UNORM words) and Display8 (R8G8B8A8_UNORM bytes) of Color (fp16 bits)."""
    c = h2f(color)
    back = unorm(c[..., 0], 10, mut) | unorm(c[..., 1], 10, mut) << 10 | unorm(c[..., 2], 10, mut) << 20 | unorm(c[..., 3], 2, mut) << 30
    d8 = np.stack([unorm(c[..., k], 8, mut) for k in range(4)], axis=-1).astype(np.uint8)
    return back.astype(np.uint32), d8


def post_process(radiance, settings, mut=()):
    """The whole chain: (stage images or [], Color, BackBuffer, Display8)."""
    s = np.asarray(settings).reshape(())
    images = bloom(radiance, mut) if int(s["IsBloomEnabled"]) else []
    return (images,) + resolve(radiance, images[-1] if images else None, s, mut)


# ---- comparisons -----------------------------------------------------------------------------------------------------------------
def f16_ulps(a, b):
    """per-element distance in fp16 ulps between two arrays of fp16 bits (the ordered integer line; -0 == +0); NaN == NaN, NaN against
    a number is 65536."""
    a, b = np.asarray(a, np.uint16).astype(np.int64), np.asarray(b, np.uint16).astype(np.int64)

    def key(x):
        return np.where(x & 0x8000, -(x & 0x7FFF), x)
    nan_a = ((a & 0x7C00) == 0x7C00) & ((a & 0x03FF) != 0)
    nan_b = ((b & 0x7C00) == 0x7C00) & ((b & 0x03FF) != 0)
    d = np.abs(key(a) - key(b))
    return np.where(nan_a & nan_b, 0, np.where(nan_a | nan_b, 65536, d))


def make_frame(width, height, seed=0, specials=True):
    """A seeded HDR Radiance frame (fp16 bits, alpha 0 as the path tracer writes it): log-uniform colours over [1e-4, 64], a black block
    (the Karis floor), a bright block, and -- with specials -- texels at 0, 65504, +inf and NaN."""
    rng = np.random.default_rng(seed)
    c = np.exp(rng.uniform(np.log(1e-4), np.log(64.0), (height, width, 3))).astype(F32)
    c[rng.random((height, width)) < 0.05] = 0
    bh, bw = max(1, height // 6), max(1, width // 6)
    c[:bh, :bw] = 0
    c[height - bh:, width - bw:] = rng.uniform(100, 2000, (bh, bw, 3)).astype(F32)
    if specials:
        n = width * height
        for val in (0.0, 65504.0, np.inf, np.nan):
            idx = rng.choice(n, size=max(1, n // 2000), replace=False)
            c.reshape(-1, 3)[idx, rng.integers(0, 3, idx.size)] = val
    out = np.zeros((height, width, 4), np.uint16)
    out[..., :3] = f16(c)
    return out
