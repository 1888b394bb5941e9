"""numpy restatement of the frame interpolator ("Frame generation"): the arbiter of tests/test_frame_generation_*.py.

The pass is this library's own motion-compensated frame interpolator for the frame-generation slot the reference fills with DLSS-G: not a
port of DLSS-G or FSR 3, unpinned against both. Every operation below is one IEEE float32 operation on arrays in the order of the spec (no
operation is fused), so it restates the device bit for bit. Textures: Color and MotionVector uint16 fp16 bits ((Oh, Ow, 4) and (Rh, Rw,
4)), LinearDepth float32 (Rh, Rw); Generated uint16 fp16 bits (Oh, Ow, 4), Generated8 uint32 (Oh, Ow). An fp16 store rounds to nearest
even. Written from the spec, apart from the kernel: the scatter is one unordered minimum per cell (np.minimum.at)."""
import numpy as np

import upscaleref as U

F = np.float32
DEFAULTS = {"Phase": 0.5, "DepthThreshold": 0.01}
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))           # (dx, dy) of the four bilinear taps, row-major
NEIGHBOURS = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1))     # the 3 x 3 cells, row-major
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SKY_BITS = 0x7F800000
BOTH, CURRENT_ONLY, PREVIOUS_ONLY, FALLBACK = 0, 1, 2, 3
ONE16 = 0x3C00

f16_to_f32, f_to_f16, f16 = U.f16_to_f32, U.f_to_f16, U.f16


def is_sky(z):
    """a depth that names no surface: not finite, or not in front of the camera"""
    return ~(np.isfinite(z) & (z > 0))


def guarded_rgb(bits):
    """the three colour channels of an fp16 texture as float32, all 0 where one of them is not finite"""
    rgb = f16_to_f32(bits)[..., :3]
    return np.where(np.isfinite(rgb).all(-1, keepdims=True), rgb, F(0)).astype(F)


def unorm8(x):
    """D3D's FLOAT -> UNORM8 on float32: NaN is 0, saturate, scale, add a half, truncate"""
    x = np.asarray(x, F)
    v = (np.clip(np.where(np.isnan(x), F(0), x), F(0), F(1)) * F(255) + F(0.5)).astype(F)
    return v.astype(np.uint32)


def pack8(bits):
    """R8G8B8A8_UNORM words of an fp16 (.., 4) texture"""
    c = unorm8(f16_to_f32(bits))
    return (c[..., 0] | c[..., 1] << 8 | c[..., 2] << 16 | c[..., 3] << 24).astype(np.uint32)


class FrameGeneration:
    """The pass with the frame it keeps. process(tex, jitter) -> (Generated, Generated8, generated?); after a call that generated,
    .field is the midpoint field (Rh, Rw) uint64 and .classes the class byte per output pixel (Oh, Ow) uint8; .candidates counts, per
    cell, the render pixels that scattered into it (what the rule tests reason about)."""

    def __init__(self, render, output, **overrides):
        self.render, self.output = (int(render[0]), int(render[1])), (int(output[0]), int(output[1]))
        s = dict(DEFAULTS)
        for k, v in overrides.items():
            if k not in s:
                raise KeyError(k)
            s[k] = v
        self.phi, self.tau = F(s["Phase"]), F(s["DepthThreshold"])
        self.reset()

    def reset(self):
        self.prev = None
        self.field = self.classes = self.candidates = None

    def process(self, tex, jitter):
        with np.errstate(all="ignore"):
            return self._process(tex, jitter)

    # ---- the four bilinear taps of a frame at the output position (px, py); taps outside the frame dropped, the rest renormalised
    def _sample(self, rgb, px, py):
        Ow, Oh = self.output
        fx, fy = px - F(0.5), py - F(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        wx, wy = (F(1) - tx, tx), (F(1) - ty, ty)
        wsum = np.zeros(px.shape, F)
        acc = np.zeros(px.shape + (3,), F)
        for dx, dy in TAPS:
            xf, yf = x0 + F(dx), y0 + F(dy)
            inside = (xf >= 0) & (xf <= F(Ow - 1)) & (yf >= 0) & (yf <= F(Oh - 1))
            xi, yi = np.where(inside, xf, 0).astype(np.int64), np.where(inside, yf, 0).astype(np.int64)
            w = (wx[dx] * wy[dy]).astype(F)
            wsum = wsum + np.where(inside, w, F(0))
            acc = acc + np.where(inside[..., None], w[..., None] * rgb[yi, xi], F(0))
        return (acc / wsum[..., None]).astype(F), wsum > 0

    # ---- the depth of a frame at its render sample nearest to the output position, under the jitter it was rendered with
    def _depth_at(self, depth, px, py, jx, jy, sx, sy):
        Rw, Rh = self.render
        cx, cy = np.floor(px * sx - jx), np.floor(py * sy - jy)
        cx = np.where(cx < 0, F(0), np.where(cx > F(Rw - 1), F(Rw - 1), cx))
        cy = np.where(cy < 0, F(0), np.where(cy > F(Rh - 1), F(Rh - 1), cy))
        return depth[cy.astype(np.int64), cx.astype(np.int64)]

    def _process(self, tex, jitter):
        (Rw, Rh), (Ow, Oh) = self.render, self.output
        color_bits = np.asarray(tex["Color"]).reshape(Oh, Ow, 4).astype(np.uint16)
        depth = np.asarray(tex["LinearDepth"], F).reshape(Rh, Rw)
        motion = f16_to_f32(np.asarray(tex["MotionVector"]).reshape(Rh, Rw, 4))[..., :3].astype(F)
        jx, jy = F(jitter[0]), F(jitter[1])
        keep = {"color": guarded_rgb(color_bits), "depth": depth.copy(), "jitter": (jx, jy)}
        if self.prev is None:                                  # no previous frame: Generated is Color
            self.prev = keep
            self.field = self.classes = self.candidates = None
            return color_bits.copy(), pack8(color_bits), False
        phi, tau = self.phi, self.tau
        omp = F(F(1) - phi)
        sx, sy = F(F(Rw) / F(Ow)), F(F(Rh) / F(Oh))
        cur_rgb, prev_rgb, prev_depth = keep["color"], self.prev["color"], self.prev["depth"]
        pjx, pjy = self.prev["jitter"]

        # ---- 1 and 2: clear and scatter
        qy, qx = np.mgrid[0:Rh, 0:Rw]
        sky = is_sky(depth)
        mvx, mvy = np.where(sky, F(0), motion[..., 0]), np.where(sky, F(0), motion[..., 1])
        xm = ((qx.astype(F) + F(0.5)) + jx) + omp * mvx
        ym = ((qy.astype(F) + F(0.5)) + jy) + omp * mvy
        cx, cy = np.floor(xm), np.floor(ym)
        lands = np.isfinite(mvx) & np.isfinite(mvy) & (cx >= 0) & (cx <= F(Rw - 1)) & (cy >= 0) & (cy <= F(Rh - 1))
        bits = np.where(sky, np.uint32(SKY_BITS), depth.view(np.uint32)).astype(np.uint64)
        keys = (bits << np.uint64(32)) | (qy * Rw + qx).astype(np.uint64)
        cells = (np.where(lands, cy, 0).astype(np.int64) * Rw + np.where(lands, cx, 0).astype(np.int64))[lands]
        field = np.full(Rw * Rh, EMPTY, np.uint64)
        np.minimum.at(field, cells, keys[lands])
        self.candidates = np.bincount(cells, minlength=Rw * Rh).reshape(Rh, Rw)
        field = field.reshape(Rh, Rw)

        # ---- 3: resolve. Source
        oy, ox = np.mgrid[0:Oh, 0:Ow]
        oxc, oyc = ox.astype(F) + F(0.5), oy.astype(F) + F(0.5)
        ux, uy = oxc * sx, oyc * sy
        fxc, fyc = np.floor(ux), np.floor(uy)
        fxc = np.where(fxc < 0, F(0), np.where(fxc > F(Rw - 1), F(Rw - 1), fxc))
        fyc = np.where(fyc < 0, F(0), np.where(fyc > F(Rh - 1), F(Rh - 1), fyc))
        ccx, ccy = fxc.astype(np.int64), fyc.astype(np.int64)
        key = field[ccy, ccx]
        best = np.zeros((Oh, Ow), np.uint64)
        found = np.zeros((Oh, Ow), bool)
        for dx, dy in NEIGHBOURS:
            x, y = ccx + dx, ccy + dy
            inside = (x >= 0) & (x < Rw) & (y >= 0) & (y < Rh)
            k = field[np.clip(y, 0, Rh - 1), np.clip(x, 0, Rw - 1)]
            better = inside & (k != EMPTY) & (~found | (k > best))
            best = np.where(better, k, best)
            found |= better
        key = np.where(key == EMPTY, np.where(found, best, EMPTY), key)
        has = key != EMPTY

        # displacement and taps
        q = np.where(has, key & np.uint64(0xFFFFFFFF), np.uint64(0)).astype(np.int64)
        zbits = (key >> np.uint64(32)).astype(np.uint32)
        src_sky = zbits == np.uint32(SKY_BITS)
        z = zbits.view(F)
        mv = np.where((src_sky | ~has)[..., None], F(0), motion.reshape(-1, 3)[q])
        Dx, Dy = mv[..., 0] / sx, mv[..., 1] / sy
        pcx, pcy = oxc - omp * Dx, oyc - omp * Dy
        ppx, ppy = oxc + phi * Dx, oyc + phi * Dy
        cur, okc = self._sample(cur_rgb, pcx, pcy)
        prev, okp = self._sample(prev_rgb, ppx, ppy)

        # validity
        zc = self._depth_at(depth, pcx, pcy, jx, jy, sx, sy)
        zh = self._depth_at(prev_depth, ppx, ppy, pjx, pjy, sx, sy)
        zp = z + mv[..., 2]
        okc = has & okc & np.where(src_sky, is_sky(zc), np.abs(zc - z) <= tau * np.abs(z))
        okp = has & okp & np.where(src_sky, is_sky(zh), np.abs(zh - zp) <= tau * np.abs(zp))

        # output
        blend = prev + (cur - prev) * phi
        still = prev_rgb + (cur_rgb - prev_rgb) * phi
        out = np.where((okc & okp)[..., None], blend, np.where(okc[..., None], cur, np.where(okp[..., None], prev, still))).astype(F)
        classes = np.where(okc & okp, BOTH, np.where(okc, CURRENT_ONLY, np.where(okp, PREVIOUS_ONLY, FALLBACK))).astype(np.uint8)

        # stores
        c = np.where(out > F(65504), F(65504), np.where(out < F(-65504), F(-65504), out))
        generated = np.empty((Oh, Ow, 4), np.uint16)
        generated[..., :3] = f_to_f16(c)
        generated[..., 3] = ONE16
        self.field, self.classes = field, classes
        self.prev = keep                                       # 4: history
        return generated, pack8(generated), True


# ---------------------------------------------------------------------------------------------- frames
def synthetic_frames(render, output, seed, frames=3):
    """The hostile sequence of the bit-for-bit tests: `frames` consecutive (textures, jitter). LinearDepth, MotionVector and the jitter are
    upscaleref.synthetic_frames' (depth edges, a tenth of the pixels sky, sub-pixel and three-pixel motion, strips that leave the frame or
    fail the depth test, motion vectors that are not finite); a 4 x 3 block of render pixels is sent towards one cell (motion 2 (t - q):
    the same cell at Phase 0.5, two neighbouring ones at 0.25); Color is an output-size frame of the same hostile colours (0, negative
    values, NaN, +-inf, 65504, a subnormal) with alpha 1."""
    Rw, Rh = render
    Ow, Oh = output
    rng = np.random.default_rng(seed + 7)
    out = []
    bx, by = Rw // 2, Rh // 2                                   # the block's first pixel; its target is the cell one right of its middle
    for tex, jitter in U.synthetic_frames(render, output, seed, frames):
        mv = f16_to_f32(tex["MotionVector"]).copy()
        z = tex["LinearDepth"]
        for y in range(by, min(by + 3, Rh)):
            for x in range(bx, min(bx + 4, Rw)):
                mv[y, x, 0], mv[y, x, 1] = 2.0 * (bx + 2 - x), 2.0 * (by + 1 - y)
                if not np.isfinite(z[y, x]):
                    z[y, x] = 4.0 + 0.1 * (x - bx) + 0.01 * (y - by)
        c = f16(np.exp2(rng.uniform(-6, 2, (Oh, Ow, 4))))
        for v in (0x0000, f16(-2.5), 0x7E00, 0xFC01, 0x7C00, 0xFC00, f16(65504.0), 0x0001):
            c[rng.random((Oh, Ow, 4)) < 0.01] = v
        c[..., 3] = ONE16
        out.append(({"Color": c, "LinearDepth": z, "MotionVector": f16(mv)}, jitter))
    return out


def plain_frame(render, output, colour, depth=5.0, motion=(0.0, 0.0, 0.0)):
    """a frame every render pixel of which is hit at `depth` (a number or an (Rh, Rw) array) with the motion vector given (a triple or an
    (Rh, Rw, 3) array); Color = colour (a number, a triple or an (Oh, Ow, 3) array), alpha 1"""
    Rw, Rh = render
    Ow, Oh = output
    c = np.ones((Oh, Ow, 4), np.float32)
    c[..., :3] = colour
    mv = np.zeros((Rh, Rw, 4), np.float32)
    mv[..., :3] = motion
    return {"Color": f16(c), "LinearDepth": np.broadcast_to(np.asarray(depth, np.float32), (Rh, Rw)).copy(), "MotionVector": f16(mv)}


# ---------------------------------------------------------------------------------------------- the analytic sequence of the quality test
def texture(x, y):
    """a band-limited pattern over the plane (periods of 7 pixels and more), in [0.1, 0.9]"""
    return 0.5 + 0.2 * np.sin(2 * np.pi * x / 9.0) * np.cos(2 * np.pi * y / 11.0) + 0.2 * np.sin(2 * np.pi * (x + y) / 7.0)


def analytic_frame(size, t, plane_velocity=(0.6, 0.25), square_velocity=(3.0, 1.0), square=(8.0, 6.0, 9.0)):
    """The scene of the quality test at time t (in frames), rendered analytically at pixel centres of a size x size... (w, h) frame at
    native resolution, jitter 0: a textured plane at depth 10 sliding by plane_velocity pixels a frame and, nearer (depth 4), a square of
    side square[2] whose corner is at square[:2] + t square_velocity, with a texture of its own that moves with it. Returns (textures,
    rgb float64): MotionVector leads from this frame's pixel to where its surface was a frame ago."""
    w, h = size
    ys, xs = np.mgrid[0:h, 0:w]
    x, y = xs + 0.5, ys + 0.5
    pvx, pvy = plane_velocity
    svx, svy = square_velocity
    sx0, sy0, side = square[0] + t * svx, square[1] + t * svy, square[2]
    inside = (x >= sx0) & (x < sx0 + side) & (y >= sy0) & (y < sy0 + side)
    plane = texture(x - t * pvx, y - t * pvy)
    fg = 1.0 - 0.8 * texture(3.0 + (x - sx0) * 1.3, 5.0 + (y - sy0) * 1.3)
    grey = np.where(inside, fg, plane)
    rgb = np.stack([grey, 0.8 * grey + 0.1, np.where(inside, 0.9 - 0.5 * grey, 0.3 + 0.5 * grey)], -1)
    mv = np.zeros((h, w, 3))
    mv[..., 0], mv[..., 1] = np.where(inside, -svx, -pvx), np.where(inside, -svy, -pvy)
    tex = plain_frame(size, size, rgb, depth=np.where(inside, 4.0, 10.0), motion=mv)
    return tex, rgb
