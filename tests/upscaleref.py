"""numpy restatement of the temporal upscaler ("Upscaler"): the arbiter of tests/test_upscaler_*.py.

The pass is this library's own temporal accumulating upscaler (TAAU) for the super-resolution slot the reference fills with DLSS or XeSS:
not a port of either, unpinned against both. Every operation below is one IEEE operation on arrays of `dtype` in the order of the spec:
float32 restates the device bit for bit (no operation is fused); float64 is the same pass in double, the yardstick of the float32 one.
Textures: Radiance and MotionVector uint16 fp16 bits (Rh, Rw, 4), LinearDepth float32 (Rh, Rw); Color uint16 fp16 bits (Oh, Ow, 4). An
fp16 store rounds to nearest even. The two host helpers (render size of a mode, the Halton jitter) are restated here too."""
import math

import numpy as np

DEFAULTS = {"MaxAccumulatedFrames": 16, "KernelRadius": 1.0, "DepthThreshold": 0.01}
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))           # (dx, dy) of the four bilinear taps, row-major
NEIGHBOURS = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1))     # the 3 x 3 render taps, row-major
ONE16 = 0x3C00
MODES = ("AUTO", "NATIVE", "QUALITY", "BALANCED", "PERFORMANCE", "ULTRA_PERFORMANCE")
RATIO10 = {"NATIVE": 10, "QUALITY": 15, "BALANCED": 17, "PERFORMANCE": 20, "ULTRA_PERFORMANCE": 30}


def settings(**overrides):
    """the settings as the device receives them: the floats rounded to float32"""
    s = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return {k: (int(v) if k == "MaxAccumulatedFrames" else np.float32(v)) for k, v in s.items()}


def f16_to_f32(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def f_to_f16(x):
    x = np.asarray(x)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return x.astype(np.float16).view(np.uint16)


# ---------------------------------------------------------------------------------------------- host helpers
def resolve_mode(mode, output):
    """Auto by the pixel count of the output (the reference's thresholds), any other mode is itself"""
    mode = MODES[mode] if isinstance(mode, (int, np.integer)) else mode
    if mode != "AUTO":
        return mode
    pixels = int(output[0]) * int(output[1])
    for limit, m in ((1280 * 800, "NATIVE"), (1920 * 1200, "QUALITY"), (2560 * 1600, "BALANCED"), (3840 * 2400, "PERFORMANCE")):
        if pixels <= limit:
            return m
    return "ULTRA_PERFORMANCE"


def render_size(mode, output):
    r10 = RATIO10[resolve_mode(mode, output)]
    return tuple(max(1, (int(o) * 10 + r10 // 2) // r10) for o in output)


def radical_inverse(index, base):
    """the fp32 loop of pt_upscaler_jitter: digits from the least significant one, each weighed by 1 / base^k"""
    f32 = np.float32
    inv = f32(1) / f32(base)
    weight, value, i = inv, f32(0), int(index)
    while i > 0:
        value = f32(value + f32(f32(i % base) * weight))
        weight = f32(weight * inv)
        i //= base
    return value


def jitter_count(render, output):
    f32 = np.float32
    x = f32(f32(f32(8) * f32(f32(output[0]) / f32(render[0]))) * f32(f32(output[1]) / f32(render[1])))
    return int(math.ceil(float(x)))


def jitter(frame_index, render, output):
    i = int(frame_index) % jitter_count(render, output) + 1
    return (np.float32(radical_inverse(i, 2) - np.float32(0.5)), np.float32(radical_inverse(i, 3) - np.float32(0.5)))


# ---------------------------------------------------------------------------------------------- the pass
class Upscaler:
    """The pass with its history. process(tex, jitter) -> Color as uint16 (Oh, Ow, 4); .length is n per output pixel after the call
    ((Oh, Ow) of dtype; None before the first call and after reset()); .hist the stored history (tone-mapped colour, n, z)."""

    def __init__(self, render, output, dtype=np.float32, **overrides):
        self.render, self.output = (int(render[0]), int(render[1])), (int(output[0]), int(output[1]))
        self.T = np.dtype(dtype).type
        assert self.T in (np.float32, np.float64)
        self.s = settings(**overrides)
        self.reset()

    def reset(self):
        self.hist = None
        self.length = None
        self.box = self.reused = self.centre = self.weights = None

    def process(self, tex, jitter):
        with np.errstate(all="ignore"):
            return self._process(tex, jitter)

    def _process(self, tex, jitter):
        """the texture decode: the taps' guarded colour, depth and motion, as `dtype`"""
        T = self.T
        Rw, Rh = self.render
        depth = np.asarray(tex["LinearDepth"], np.float32).reshape(Rh, Rw).astype(T)
        motion = f16_to_f32(np.asarray(tex["MotionVector"]).reshape(Rh, Rw, 4))[..., :3].astype(T)
        rgb = f16_to_f32(np.asarray(tex["Radiance"]).reshape(Rh, Rw, 4))[..., :3].astype(T)
        rgb = np.where(np.isfinite(rgb).all(-1, keepdims=True), rgb, T(0))
        return self._resolve(rgb, depth, motion, jitter)

    def resolve(self, rgb, depth, motion, jitter):
        """Steps 1-6 on taps given as arrays of `dtype`: rgb (Rh, Rw, 3) guarded colour, depth (Rh, Rw), motion (Rh, Rw, 3). Owns the
        output history: process() is the texture decode and this; the reconstruction's stage 4 is this on its remodulated taps."""
        with np.errstate(all="ignore"):
            return self._resolve(rgb, depth, motion, jitter)

    def _resolve(self, rgb, depth, motion, jitter):
        T = self.T
        (Rw, Rh), (Ow, Oh) = self.render, self.output
        one, zero, half = T(1), T(0), T(0.5)
        jx, jy = T(np.float32(jitter[0])), T(np.float32(jitter[1]))
        M, R, tau = T(self.s["MaxAccumulatedFrames"]), T(self.s["KernelRadius"]), T(self.s["DepthThreshold"])
        R2 = R * R
        floor_w = T(0.015625)
        m = np.maximum(np.maximum(rgb[..., 0], rgb[..., 1]), rgb[..., 2])
        toned = (rgb / (one + np.where(m > 0, m, zero))[..., None]).astype(T)        # t(c), the same value at every tap that reads the texel

        # ---- 1: position
        sx, sy = T(Rw) / T(Ow), T(Rh) / T(Oh)
        oy, ox = np.mgrid[0:Oh, 0:Ow]
        oxc, oyc = ox.astype(T) + half, oy.astype(T) + half
        ux, uy = oxc * sx, oyc * sy
        cxf, cyf = np.floor(ux - jx), np.floor(uy - jy)
        cxf = np.where(cxf < 0, zero, np.where(cxf > T(Rw - 1), T(Rw - 1), cxf))
        cyf = np.where(cyf < 0, zero, np.where(cyf > T(Rh - 1), T(Rh - 1), cyf))
        cx, cy = cxf.astype(np.int64), cyf.astype(np.int64)

        # ---- 2 and 3: dilation and the current colour over the same 3 x 3 taps
        best = np.full((Oh, Ow), np.inf, T)
        bx, by = np.zeros((Oh, Ow), np.int64), np.zeros((Oh, Ow), np.int64)
        found = np.zeros((Oh, Ow), bool)
        wsum = np.zeros((Oh, Ow), T)
        acc = np.zeros((Oh, Ow, 3), T)
        lo, hi = np.full((Oh, Ow, 3), np.inf, T), np.full((Oh, Ow, 3), -np.inf, T)
        k = None
        for dx, dy in NEIGHBOURS:
            qx, qy = cx + dx, cy + dy
            inside = (qx >= 0) & (qx < Rw) & (qy >= 0) & (qy < Rh)
            qxc, qyc = np.clip(qx, 0, Rw - 1), np.clip(qy, 0, Rh - 1)
            zq = depth[qyc, qxc]
            better = inside & np.isfinite(zq) & (zq < best)
            best = np.where(better, zq, best)
            bx, by = np.where(better, qxc, bx), np.where(better, qyc, by)
            found |= better
            ddx = ((qx.astype(T) + half) + jx) - ux
            ddy = ((qy.astype(T) + half) + jy) - uy
            d2 = ddx * ddx + ddy * ddy
            w = one - d2 / R2
            w = np.where(w > 0, w, zero)
            w = w * w
            if dx == 0 and dy == 0:
                w = np.where(w < floor_w, floor_w, w)
                k = w
            use = inside & (w > 0)
            tq = toned[qyc, qxc]
            wsum = wsum + np.where(use, w, zero)
            acc = acc + np.where(use[..., None], w[..., None] * tq, zero)
            lo = np.where(inside[..., None] & (tq < lo), tq, lo)
            hi = np.where(inside[..., None] & (tq > hi), tq, hi)
        cur = (acc / wsum[..., None]).astype(T)
        z = best
        mv = np.where(found[..., None], motion[by, bx], zero)
        background = ~found

        # ---- 4: history
        px, py = oxc + mv[..., 0] / sx, oyc + mv[..., 1] / sy
        fx, fy = px - half, py - half
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        wx, wy = (one - tx, tx), (one - ty, ty)
        zp = z + mv[..., 2]
        tol = tau * np.abs(zp)
        hsum = np.zeros((Oh, Ow), T)
        hacc = np.zeros((Oh, Ow, 4), T)
        if self.hist is not None:
            for dx, dy in TAPS:
                xf, yf = x0 + T(dx), y0 + T(dy)
                inside = (xf >= 0) & (xf <= T(Ow - 1)) & (yf >= 0) & (yf <= T(Oh - 1))
                xi, yi = np.where(inside, xf, 0).astype(np.int64), np.where(inside, yf, 0).astype(np.int64)
                zh = self.hist["z"][yi, xi]
                ok = inside & np.where(background, ~np.isfinite(zh), np.abs(zh - zp) <= tol)
                w = wx[dx] * wy[dy]
                hsum = hsum + np.where(ok, w, zero)
                hacc = hacc + np.where(ok[..., None], w[..., None] * self.hist["colour_n"][yi, xi], zero)
        have = hsum > 0
        h = hacc / hsum[..., None]

        # ---- 5: clamp and blend
        hc = h[..., :3]
        hc = np.where(hc < lo, lo, np.where(hc > hi, hi, hc))
        n1 = h[..., 3] + k
        n = np.where(n1 < M, n1, M)
        a = k / n
        blend = np.where((a >= one)[..., None], cur, hc + (cur - hc) * a[..., None])
        out = np.where(have[..., None], blend, cur).astype(T)
        n = np.where(have, n, k).astype(T)

        # ---- 6: store
        self.hist = {"colour_n": np.concatenate([out, n[..., None]], -1).astype(T), "z": z.astype(T)}
        self.length = n
        self.box, self.reused, self.centre, self.weights = (lo, hi), have, (cx, cy), wsum       # what the rule tests reason about
        mo = np.maximum(np.maximum(out[..., 0], out[..., 1]), out[..., 2])
        den = one - np.where(mo > 0, mo, zero)
        den = np.where(den < T(2.0 ** -17), T(2.0 ** -17), den)
        c = out / den[..., None]
        c = np.where(c > T(65504), T(65504), np.where(c < T(-65504), T(-65504), c))
        color = np.empty((Oh, Ow, 4), np.uint16)
        color[..., :3] = f_to_f16(c)
        color[..., 3] = ONE16
        return color


def bilinear_upsample(image, output):
    """the plain bilinear resize of one (Rh, Rw, C) float64 frame to the output grid (pixel centres aligned, edges clamped): the yardstick
    a temporal upscaler has to beat"""
    Rh, Rw = image.shape[:2]
    Ow, Oh = output
    oy, ox = np.mgrid[0:Oh, 0:Ow]
    fx, fy = (ox + 0.5) * (Rw / Ow) - 0.5, (oy + 0.5) * (Rh / Oh) - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[..., None], (fy - y0)[..., None]
    def at(dx, dy):
        return image[np.clip(y0 + dy, 0, Rh - 1).astype(int), np.clip(x0 + dx, 0, Rw - 1).astype(int)]
    return (at(0, 0) * (1 - tx) + at(1, 0) * tx) * (1 - ty) + (at(0, 1) * (1 - tx) + at(1, 1) * tx) * ty


# ---------------------------------------------------------------------------------------------- frames
def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def synthetic_frames(render, output, seed, frames=3):
    """The hostile sequence of the bit-for-bit tests: `frames` consecutive (textures, jitter) of a render-size frame. A slanted plane with
    a depth edge at x = 0.6 Rw, a tenth of the pixels missed (another tenth each frame), motion that is sub-pixel (left third) and three
    pixels (the rest) and, in strips, leaves the frame (x < 2: sixty pixels to the left) or fails the depth test (rows 3-4: the previous
    depth 1 further); a few motion vectors that are not finite or huge; colours of 0, negative values, NaN, +-inf and 65504 seeded in;
    the Halton jitter of each frame."""
    Rw, Rh = render
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:Rh, 0:Rw]
    edge = xs >= int(0.6 * Rw)
    out = []
    for f in range(frames):
        z = np.where(edge, 7.0, 5.0) + 0.01 * xs + 0.004 * ys
        z = (z * (1.0 + 0.002 * rng.uniform(-1, 1, (Rh, Rw)))).astype(np.float32)
        mv = np.zeros((Rh, Rw, 4), np.float32)
        mv[..., 0] = np.where(xs < Rw // 3, 0.37, 3.0)
        mv[..., 1] = np.where(xs < Rw // 3, -0.21, 0.0)
        mv[..., 2] = rng.uniform(-0.01, 0.01, (Rh, Rw))
        mv[:, :2, 0] = -60.0
        mv[3:5, :, 2] = 1.0
        bad = rng.random((Rh, Rw)) < 0.02
        mv[bad, 0] = np.array([np.nan, np.inf, -np.inf, 60000.0], np.float32)[rng.integers(0, 4, int(bad.sum()))]
        dead = rng.permutation(Rw * Rh)[: max(3, Rw * Rh // 10)]
        zf = z.reshape(-1)
        zf[dead] = np.array([np.inf, -np.inf, np.nan], np.float32)[np.arange(len(dead)) % 3]
        c = f16(np.exp2(rng.uniform(-6, 4, (Rh, Rw, 4))))
        for v in (0x0000, f16(-2.5), 0x7E00, 0xFC01, 0x7C00, 0xFC00, f16(65504.0), 0x0001):
            c[rng.random((Rh, Rw, 4)) < 0.01] = v
        c[..., 3] = 0
        out.append(({"Radiance": c, "LinearDepth": zf.reshape(Rh, Rw), "MotionVector": f16(mv)}, jitter(f, render, output)))
    return out


def plain_frame(render, colour, depth=5.0, motion=(0.0, 0.0, 0.0)):
    """a frame every pixel of which is hit at `depth` (a number or an (Rh, Rw) array) with the motion vector given; Radiance = colour (a
    number, an rgb triple or an (Rh, Rw, 3) array), alpha 0"""
    Rw, Rh = render
    c = np.zeros((Rh, Rw, 4), np.float32)
    c[..., :3] = colour
    mv = np.zeros((Rh, Rw, 4), np.float32)
    mv[..., :3] = motion
    return {"Radiance": f16(c), "LinearDepth": np.broadcast_to(np.asarray(depth, np.float32), (Rh, Rw)).copy(), "MotionVector": f16(mv)}


def ulp16(x):
    """the spacing of the fp16 grid at |x| (float64): 2^-24 in the subnormal range"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15) - 10)
