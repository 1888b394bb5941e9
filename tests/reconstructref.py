"""numpy restatement of the ray-reconstruction pass ("Ray reconstruction"): the arbiter of
tests/test_reconstruction_*.py.

The pass is this library's own denoising upscaler for the slot the reference fills with DLSS Ray Reconstruction: not a port of it,
unpinned against it. Every operation below is one IEEE operation on arrays of `dtype` in the order of the spec: float32 restates the
device bit for bit (the only fused operations are those of dot() and luminance(), evaluated exactly by fma()); float64 is the same pass
in double. Textures at the render size: Radiance, DiffuseAlbedo, SpecularAlbedo and MotionVector uint16 fp16 bits (Rh, Rw, 4),
NormalRoughness int16 (Rh, Rw, 4), Position float32 (Rh, Rw, 4), LinearDepth float32 (Rh, Rw); Color uint16 fp16 bits (Oh, Ow, 4)."""
import numpy as np

import denoiseref as D
import upscaleref as U

DEFAULTS = {"MaxAccumulatedFrames": 30, "MaxOutputFrames": 16, "AtrousIterations": 5, "DepthThreshold": 0.01, "NormalCosine": 0.8,
            "LuminanceSigma": 2.0, "RoughnessFraction": 0.15, "KernelRadius": 1.0}
INTEGERS = ("MaxAccumulatedFrames", "MaxOutputFrames", "AtrousIterations")
ALBEDO_FLOOR, ALBEDO_CEILING = 0.015625, 131008.0
RESET_RATIO = 16.0
TAPS, ONE16 = U.TAPS, U.ONE16
f16_to_f32, f16, jitter, ulp16 = U.f16_to_f32, U.f16, U.jitter, U.ulp16
_shift = D._shift


def settings(**overrides):
    """the settings as the device receives them: the floats rounded to float32"""
    s = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return {k: (int(v) if k in INTEGERS else np.float32(v)) for k, v in s.items()}


class Reconstruction:
    """The pass with its two histories. process(tex, jitter) -> Color as uint16 (Oh, Ow, 4). After a call: .length the history length of
    the signal per render pixel, .filtered the (Rh, Rw, 4) record the resolve read (filtered signal and variance; the guarded Radiance
    and 0 where the G-buffer missed), .albedo the (Rh, Rw, 3) albedo it multiplied back, .n the accumulated weight per output pixel,
    .reused / .reused_out where a history was used at render / output size, .feature where the luminance reset dropped one. None before the first call and after reset()."""

    def __init__(self, render, output, dtype=np.float32, **overrides):
        self.render, self.output = (int(render[0]), int(render[1])), (int(output[0]), int(output[1]))
        self.A = D.Arith(dtype)
        self.s = settings(**overrides)
        # stage 4 is the upscaler's resolve with this pass's own output history
        self.up = U.Upscaler(render, output, dtype, MaxAccumulatedFrames=self.s["MaxOutputFrames"], KernelRadius=self.s["KernelRadius"],
                             DepthThreshold=self.s["DepthThreshold"])
        self.reset()

    def reset(self):
        self.hist = None
        self.up.reset()
        self.length = self.filtered = self.albedo = self.n = self.reused = self.reused_out = self.feature = None

    @property
    def out_hist(self):
        """the output history: stage 4's (tone-mapped colour, n, z), None when there is none"""
        return self.up.hist

    def process(self, tex, jitter):
        with np.errstate(all="ignore"):
            return self._process(tex, jitter)

    # ---- pieces shared by the stages
    def _wg(self, Np, Pp, Pq, plane):
        A = self.A
        return A.max0(A.T(1) - np.abs(A.dot(Np, Pq - Pp)) / plane)

    def _wn(self, Np, Nq):
        A = self.A
        nc = A.T(self.s["NormalCosine"])
        return A.max0((A.dot(Np, Nq) - nc) / (A.T(1) - nc))

    def _process(self, tex, jitter):
        A, T, s = self.A, self.A.T, self.s
        W, H = self.render
        zero, one = T(0), T(1)
        z = np.asarray(tex["LinearDepth"], np.float32).reshape(H, W).astype(T)
        hit = np.isfinite(z)
        nr = np.asarray(tex["NormalRoughness"], np.int16).reshape(H, W, 4)
        N, r = A.snorm16(nr[..., :3]), A.snorm16(nr[..., 3])
        P = np.asarray(tex["Position"], np.float32).reshape(H, W, 4)[..., :3].astype(T)
        mv = f16_to_f32(np.asarray(tex["MotionVector"]).reshape(H, W, 4)).astype(T)
        rad = f16_to_f32(np.asarray(tex["Radiance"]).reshape(H, W, 4))[..., :3].astype(T)
        rad = np.where(np.isfinite(rad).all(-1, keepdims=True), rad, zero).astype(T)
        Ad = f16_to_f32(np.asarray(tex["DiffuseAlbedo"]).reshape(H, W, 4))[..., :3].astype(T)
        As = f16_to_f32(np.asarray(tex["SpecularAlbedo"]).reshape(H, W, 4))[..., :3].astype(T)
        M = T(s["MaxAccumulatedFrames"])
        dthr, nc, rf = T(s["DepthThreshold"]), T(s["NormalCosine"]), T(s["RoughnessFraction"])

        # ---- stage 1: demodulate + temporal
        alb = Ad + As
        alb = np.where(alb > T(ALBEDO_FLOOR), alb, T(ALBEDO_FLOOR))
        alb = np.where(alb < T(ALBEDO_CEILING), alb, T(ALBEDO_CEILING)).astype(T)
        cur = (rad / alb).astype(T)
        L = A.luminance(cur)
        t = r / T(0.5)
        t = A.max0(np.where(t < 1, t, one))
        shorter = (A.luminance(As) > A.luminance(Ad)) & (mv[..., 0] * mv[..., 0] + mv[..., 1] * mv[..., 1] > T(0.0625))
        cap = np.where(shorter, one + np.floor((M - one) * t), M).astype(T)
        ys, xs = np.mgrid[0:H, 0:W]
        fx = ((xs.astype(T) + T(0.5)) + mv[..., 0]) - T(0.5)
        fy = ((ys.astype(T) + T(0.5)) + mv[..., 1]) - T(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        zp = z + mv[..., 2]
        ztol = dthr * np.abs(zp)
        plane = dthr * np.abs(z)
        wx, wy = (one - tx, tx), (one - ty, ty)
        cur_q = [cur[..., 0], cur[..., 1], cur[..., 2], L, L * L]
        wsum = np.zeros((H, W), T)
        h = [np.zeros((H, W), T) for _ in range(6)]
        if self.hist is not None:
            for dx, dy in TAPS:
                xf, yf = x0 + T(dx), y0 + T(dy)
                inside = (xf >= 0) & (xf <= T(W - 1)) & (yf >= 0) & (yf <= T(H - 1))
                xi, yi = np.where(inside, xf, 0).astype(np.int64), np.where(inside, yf, 0).astype(np.int64)
                g = {k: v[yi, xi] for k, v in self.hist.items()}
                same_surface = (np.abs(g["z"] - zp) <= ztol) | (np.abs(A.dot(N, g["P"] - P)) <= plane)
                ok = (inside & same_surface & (A.dot(N, g["N"]) >= nc) & (g["length"] > 0)
                      & (np.abs(r - g["r"]) <= rf * np.where(r > g["r"], r, g["r"])))
                w = wx[dx] * wy[dy]
                wsum = wsum + np.where(ok, w, zero)
                for k, v in enumerate((g["signal"][..., 0], g["signal"][..., 1], g["signal"][..., 2], g["moments"][..., 0],
                                       g["moments"][..., 1], g["length"])):
                    h[k] = h[k] + np.where(ok, w * v, zero)
        have = (wsum > 0) & hit
        h = [v / wsum for v in h]
        # the luminance reset: sixteen times darker than the history less its deviation, or sixteen times brighter than the history plus
        # its deviation with a neighbour of this frame at least half as bright
        sd = np.sqrt(A.max0(h[4] - h[3] * h[3]))
        corroborated = np.zeros((H, W), bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    Lq, inside = _shift(L, dx, dy)
                    hq, _ = _shift(hit, dx, dy)
                    corroborated |= inside & hq & (Lq >= T(0.5) * L)
        feature = have & ((L * T(RESET_RATIO) < h[3] - sd) | ((L > T(RESET_RATIO) * (h[3] + sd)) & corroborated))
        have = have & ~feature
        n1 = h[5] + one
        n = np.where(n1 < cap, n1, cap).astype(T)
        inv = one / n
        acc = [np.where(have, h[k] + (cur_q[k] - h[k]) * inv, cur_q[k]) for k in range(5)]
        signal = np.where(hit[..., None], np.stack(acc[:3], -1), zero).astype(T)
        moments = np.where(hit[..., None], np.stack(acc[3:], -1), zero).astype(T)
        length = np.where(hit, np.where(have, n, one), zero).astype(T)
        self.hist = {"signal": signal, "moments": moments, "length": length, "z": z, "N": N, "r": r, "P": P}
        self.length, self.reused, self.feature = length, have, feature
        albedo = np.where(hit[..., None], alb, one).astype(T)

        # ---- stage 2: variance
        var = A.max0(moments[..., 1] - moments[..., 0] * moments[..., 0])
        var = np.where(length < 4, self._spatial_variance(signal, P, N, hit, plane), var)
        var = np.where(feature, zero, var).astype(T)
        # ---- stage 3: a-trous
        for k in range(s["AtrousIterations"]):
            signal, var = self._atrous(signal, var, 1 << k, P, N, r, hit, plane, T(s["LuminanceSigma"]), rf)
        filtered = np.concatenate([np.where(hit[..., None], signal, rad), np.where(hit, var, zero)[..., None]], -1).astype(T)
        self.filtered, self.albedo = filtered, albedo

        # ---- stage 4: resolve
        color = self.up.resolve((filtered[..., :3] * albedo).astype(T), z, mv[..., :3], jitter)
        self.n, self.reused_out = self.up.length, self.up.reused
        return color

    def _spatial_variance(self, signal, P, N, hit, plane):
        A, T = self.A, self.A.T
        H, W = hit.shape
        L = A.luminance(signal)
        s1, s2, count = np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W), T)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                hq, inside = _shift(hit, dx, dy)
                if dx == 0 and dy == 0:
                    use = inside
                else:
                    Pq, _ = _shift(P, dx, dy)
                    Nq, _ = _shift(N, dx, dy)
                    use = inside & hq & (self._wg(N, P, Pq, plane) > 0) & (self._wn(N, Nq) > 0)
                Lq, _ = _shift(L, dx, dy)
                s1 = s1 + np.where(use, Lq, T(0))
                s2 = s2 + np.where(use, Lq * Lq, T(0))
                count = count + np.where(use, T(1), T(0))
        m1, m2 = s1 / count, s2 / count
        return A.max0(m2 - m1 * m1)

    def _atrous(self, signal, var, step, P, N, r, hit, plane, sigma, rf):
        A, T = self.A, self.A.T
        H, W = hit.shape
        b, bw = np.zeros((H, W), T), np.zeros((H, W), T)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                hq, inside = _shift(hit, dx, dy)
                use = inside & hq
                k = T(0.5 if dx == 0 else 0.25) * T(0.5 if dy == 0 else 0.25)
                vq, _ = _shift(var, dx, dy)
                b = b + np.where(use, k * vq, T(0))
                bw = bw + np.where(use, k, T(0))
        sd = sigma * np.sqrt(b / bw) + A.c(1e-4)
        Lp = A.luminance(signal)
        acc, ws, va = np.zeros((H, W, 3), T), np.zeros((H, W), T), np.zeros((H, W), T)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                hq, inside = _shift(hit, dx * step, dy * step)
                if dx == 0 and dy == 0:
                    wq = np.full((H, W), T(0.140625))
                else:
                    Pq, _ = _shift(P, dx * step, dy * step)
                    Nq, _ = _shift(N, dx * step, dy * step)
                    rq, _ = _shift(r, dx * step, dy * step)
                    Lq, _ = _shift(Lp, dx * step, dy * step)
                    base = ((T(D.H5[dy + 2]) * T(D.H5[dx + 2])) * self._wg(N, P, Pq, plane)) * self._wn(N, Nq)
                    wr = A.max0(T(1) - np.abs(rq - r) / (rf * np.where(r > rq, r, rq) + A.c(1e-6)))
                    wl = A.max0(T(1) - np.abs(Lq - Lp) / sd)
                    wq = np.where(inside & hq, (base * wl) * wr, T(0)).astype(T)
                cq, _ = _shift(signal, dx * step, dy * step)
                vq, _ = _shift(var, dx * step, dy * step)
                use = wq > 0
                ws = ws + np.where(use, wq, T(0))
                va = va + np.where(use, (wq * wq) * vq, T(0))
                acc = acc + np.where(use[..., None], wq[..., None] * cq, T(0))
        return (acc / ws[..., None]).astype(T), (va / (ws * ws)).astype(T)


# ---------------------------------------------------------------------------------------------- frames
def synthetic_frames(render, output, seed, frames=3):
    """The hostile sequence of the bit-for-bit tests: `frames` consecutive (textures, jitter) of a render-size frame. The denoiser's
    hostile guides (a slanted plane with a depth and a normal edge at x = 0.6 Rw, a roughness step at y = Rh / 2, a tenth of the pixels
    missed, another tenth each frame; motion that is sub-pixel on the left third and three pixels elsewhere and, in strips, leaves the
    frame or fails the depth test; a few motion vectors that are not finite) with one Radiance (0, negative values, NaN, +-inf and 65504
    seeded in) and the two albedos: the left half diffuse-dominated, the right half specular-dominated, with zeros, values whose sum
    stays under the floor of 1 / 64, NaN and inf seeded in; the Halton jitter of each frame."""
    Rw, Rh = render
    guides = D.synthetic_frames(Rw, Rh, seed, frames)
    rng = np.random.default_rng(seed + 7919)
    ys, xs = np.mgrid[0:Rh, 0:Rw]
    out = []
    for f, g in enumerate(guides):
        tex = {k: g[k] for k in ("Position", "LinearDepth", "NormalRoughness", "MotionVector")}
        rad = g["NoisyDiffuse"].copy()
        rad[..., 3] = 0
        tex["Radiance"] = rad
        specular = (xs >= Rw // 2)[..., None]
        ad = np.where(specular, rng.uniform(0.0, 0.2, (Rh, Rw, 4)), rng.uniform(0.2, 0.9, (Rh, Rw, 4)))
        sp = np.where(specular, rng.uniform(0.3, 1.0, (Rh, Rw, 4)), rng.uniform(0.0, 0.1, (Rh, Rw, 4)))
        ad, sp = f16(ad), f16(sp)
        n = Rw * Rh
        order = rng.permutation(n)                             # so many pixels of each kind, whatever the frame's size
        low, none, one = order[:max(3, n // 12)], order[max(3, n // 12):][:max(2, n // 30)], order[-max(4, n // 15):]
        ad.reshape(n, 4)[low] = f16(rng.uniform(0.0, 0.006, (len(low), 4)))      # both albedos tiny: the sum is under the floor
        sp.reshape(n, 4)[low] = f16(rng.uniform(0.0, 0.006, (len(low), 4)))
        ad.reshape(n, 4)[none] = 0                             # both zero
        sp.reshape(n, 4)[none] = 0
        ad.reshape(n, 4)[one[::2]] = 0                         # one of the two zero
        sp.reshape(n, 4)[one[1::2]] = 0
        for t in (ad, sp):
            for v in (0x7E00, 0x7C00, 0xFC00, f16(65504.0), f16(-0.5), 0x0001):
                t.reshape(-1)[rng.permutation(n * 4)[:max(2, n // 60)]] = v
        tex["DiffuseAlbedo"], tex["SpecularAlbedo"] = ad, sp
        out.append((tex, jitter(f, render, output)))
    return out


def upscaler_textures(tex):
    """what upscaleref reads of a frame"""
    return {k: tex[k] for k in ("Radiance", "LinearDepth", "MotionVector")}


def plain_frame(render, colour, albedo=(0.5, 0.25), depth=5.0, motion=(0.0, 0.0, 0.0), normal=(0.0, 0.0, -1.0), roughness=0.5):
    """a frame every pixel of which is hit at `depth` facing `normal`, with the motion vector given; Radiance = colour (a number, an rgb
    triple or an (Rh, Rw, 3) array); albedo = (diffuse, specular), each a number, a triple or an (Rh, Rw, 3) array"""
    Rw, Rh = render
    tex = U.plain_frame(render, colour, depth, motion)
    z = tex["LinearDepth"]
    ys, xs = np.mgrid[0:Rh, 0:Rw]
    P = np.zeros((Rh, Rw, 4), np.float32)
    P[..., 0] = (xs - Rw // 2) * 0.1; P[..., 1] = (ys - Rh // 2) * 0.1; P[..., 2] = z
    nr = np.zeros((Rh, Rw, 4), np.int16)
    nr[..., :3] = np.round(np.asarray(normal, np.float64) * 32767)
    nr[..., 3] = np.round(np.asarray(roughness, np.float64) * 32767)
    tex["Position"], tex["NormalRoughness"] = P, nr
    for name, v in zip(("DiffuseAlbedo", "SpecularAlbedo"), albedo):
        a = np.zeros((Rh, Rw, 4), np.float32)
        a[..., :3] = v
        tex[name] = f16(a)
    return tex


def noisy_sequence(render, output, frames, seed, sigma, contrast=0.25):
    """The sequence of the noise test, with its truth. Two planes facing the camera (a depth and a normal edge at the middle column of the
    output grid), piecewise-constant lighting E (one value a plane), a checker albedo at the output grid's pitch: truth = E x albedo at
    the output pixels, (Oh, Ow, 3) float64. Each frame samples lighting and albedo at its jittered sample positions (the albedo a
    sample sees is the checker cell under it) and multiplies the lighting by seeded noise 1 + sigma u, u uniform in [-1, 1): what a
    1 spp frame does to the lighting and not to the albedo. Returns ([(textures, jitter)], truth)."""
    Rw, Rh = render
    Ow, Oh = output
    rng = np.random.default_rng(seed)
    light = np.array([[1.6, 1.2, 0.8], [0.5, 0.7, 1.1]])
    bright = np.array([0.8, 0.7, 0.6])
    dark = bright * (1.0 - contrast)

    def plane(u):                  # u: x in output pixels
        return (u >= Ow / 2).astype(int)

    def checker(u, v):
        return np.where(((np.floor(u) + np.floor(v)) % 2 == 0)[..., None], bright, dark)

    oy, ox = np.mgrid[0:Oh, 0:Ow]
    truth = light[plane(ox + 0.5)] * checker(ox + 0.5, oy + 0.5)
    ys, xs = np.mgrid[0:Rh, 0:Rw]
    seq = []
    for f in range(frames):
        j = jitter(f, render, output)
        u, v = (xs + 0.5 + float(j[0])) * (Ow / Rw), (ys + 0.5 + float(j[1])) * (Oh / Rh)
        side = plane(u)
        alb = checker(u, v)
        noise = 1.0 + sigma * rng.uniform(-1, 1, (Rh, Rw, 1))
        # the right plane passes through (0, y, 7) with normal (0.6, 0, -0.8): z = 7 + 0.75 x, so its pixels lie in one another's plane
        tex = plain_frame(render, light[side] * noise * alb, albedo=(alb, 0.0), depth=np.where(side == 1, 7.0 + 0.075 * (xs - Rw // 2), 5.0))
        n = np.where((side == 1)[..., None], (0.6, 0.0, -0.8), (0.0, 0.0, -1.0))
        tex["NormalRoughness"][..., :3] = np.round(n * 32767)
        seq.append((tex, j))
    return seq, truth
