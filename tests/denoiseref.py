"""numpy restatement of the denoiser ("Denoiser"): the arbiter of tests/test_denoiser_*.py.

The filter is this library's own in ReLAX's shape, not a port of NRD's (its source is not in the reference tree): parity with the SDK is
unpinned. Every operation below is one IEEE operation on arrays of `dtype` in the order of the spec: float32 restates the device bit for
bit (the only fused operations are those of dot() and luminance(), evaluated exactly by fma()); float64 is the same filter in double,
the yardstick of the float32 one. Textures: Position float32 (H, W, 4), LinearDepth float32 (H, W), NormalRoughness int16 (H, W, 4),
MotionVector and the Noisy / Denoised pair uint16 fp16 bits (H, W, 4). An fp16 store rounds to nearest even and stores a NaN as 0x7E00."""
import numpy as np

NAN16 = 0x7E00
DEFAULTS = {"MaxAccumulatedFrames": 30, "AtrousIterations": 5, "DepthThreshold": 0.01, "NormalCosine": 0.8, "DiffuseLuminanceSigma": 2.0,
            "SpecularLuminanceSigma": 1.0, "RoughnessFraction": 0.15}
H5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)          # the a-trous kernel per axis
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))           # (dx, dy) of the four bilinear taps, row-major


def settings(**overrides):
    """the settings as the device receives them: the floats rounded to float32"""
    s = dict(DEFAULTS)
    for k, v in overrides.items():
        if k not in s:
            raise KeyError(k)
        s[k] = v
    return {k: (int(v) if k in ("MaxAccumulatedFrames", "AtrousIterations") else np.float32(v)) for k, v in s.items()}


def f16_to_f32(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def f_to_f16(x):
    x = np.asarray(x)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        h = x.astype(np.float16).view(np.uint16)
    return np.where(np.isnan(x), np.uint16(NAN16), h).astype(np.uint16)


def fma32(a, b, c):
    """fmaf(a, b, c) exactly: the float64 product of two float32 values is exact; the float64 sum is made round-to-odd (TwoSum error
    term), so the final rounding to float32 is the single rounding of the exact a * b + c."""
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = np.asarray(p + c64)
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        odd = (s.view(np.int64) & 1) == 1
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


class Arith:
    """the arithmetic of one evaluation: float32 (the device's) or float64"""

    def __init__(self, dtype):
        self.T = np.dtype(dtype).type
        assert self.T in (np.float32, np.float64)

    def c(self, literal):
        """an fp32 literal of the spec"""
        return self.T(np.float32(literal))

    def fma(self, a, b, c):
        if self.T is np.float32:
            return fma32(a, b, c)
        return np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)

    def dot(self, a, b):
        """sop3: mad(a.z, b.z, mad(a.y, b.y, a.x * b.x))"""
        return self.fma(a[..., 2], b[..., 2], self.fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))

    def luminance(self, c):
        """ml_luminance: dot(c, (0.299f, 0.587f, 0.114f))"""
        return self.fma(c[..., 2], self.c(0.114), self.fma(c[..., 1], self.c(0.587), c[..., 0] * self.c(0.299)))

    def max0(self, x):
        return np.where(x > 0, x, self.T(0))

    def snorm16(self, v):
        v = np.asarray(v, np.int16)
        return np.where(v == -32768, self.T(-1), v.astype(self.T) / self.T(32767)).astype(self.T)


def _shift(arr, dx, dy):
    """(arr at (x + dx, y + dy), inside): the index is clamped where the tap leaves the frame, and `inside` says so"""
    H, W = arr.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    xq, yq = xs + dx, ys + dy
    inside = (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
    return arr[np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)], inside


class Denoiser:
    """The filter with its history. process(tex) -> (DenoisedDiffuse, DenoisedSpecular) as uint16 (H, W, 4); .length is the diffuse
    history length per pixel after the call ((H, W) of dtype; None before the first call and after reset())."""

    def __init__(self, width, height, dtype=np.float32, **overrides):
        self.W, self.H = width, height
        self.A = Arith(dtype)
        self.s = settings(**overrides)
        self.reset()

    def reset(self):
        self.hist = None
        self.length = None

    # ---- pieces shared by the stages
    def _wg(self, Np, Pp, Pq, plane):
        A = self.A
        return A.max0(A.T(1) - np.abs(A.dot(Np, Pq - Pp)) / plane)

    def _wn(self, Np, Nq):
        A = self.A
        nc = A.T(self.s["NormalCosine"])
        return A.max0((A.dot(Np, Nq) - nc) / (A.T(1) - nc))

    def _load(self, bits):
        """the noisy texel as the filter takes it: rgb all 0 when one is not finite, a hit distance that is not finite 0"""
        q = f16_to_f32(bits).astype(self.A.T)
        ok = np.isfinite(q[..., :3]).all(-1, keepdims=True)
        out = np.where(ok, q, self.A.T(0))
        out[..., 3] = np.where(np.isfinite(q[..., 3]), q[..., 3], self.A.T(0))
        return out

    def _accumulate(self, ok, w, prev, which, cur, cap):
        """one channel of stage 1. ok, w: four (H, W) arrays; prev: per tap the gathered history; which: 0 diffuse, 1 specular"""
        A, T = self.A, self.A.T
        L = A.luminance(cur)
        cur_q = [cur[..., 0], cur[..., 1], cur[..., 2], cur[..., 3], L, L * L]
        wsum = np.zeros(cur.shape[:2], T)
        for t in range(4):
            wsum = wsum + np.where(ok[t], w[t], T(0))
        have = wsum > 0
        names = [("colour", 0), ("colour", 1), ("colour", 2), ("colour", 3), ("moments", 0), ("moments", 1), ("length", None)]
        h = []
        for name, k in names:
            acc = np.zeros(cur.shape[:2], T)
            for t in range(4):
                v = prev[t][name][which]
                acc = acc + np.where(ok[t], w[t] * (v if k is None else v[..., k]), T(0))
            h.append(acc / wsum)
        n1 = h[6] + T(1)
        n = np.where(n1 < cap, n1, cap).astype(T)
        inv = T(1) / n
        out = [np.where(have, h[k] + (cur_q[k] - h[k]) * inv, cur_q[k]) for k in range(6)]
        return np.stack(out[:4], -1).astype(T), np.stack(out[4:], -1).astype(T), np.where(have, n, T(1)).astype(T)

    def process(self, tex):
        with np.errstate(all="ignore"):
            return self._process(tex)

    def _process(self, tex):
        A, T, s, W, H = self.A, self.A.T, self.s, self.W, self.H
        z = np.asarray(tex["LinearDepth"], np.float32).reshape(H, W).astype(T)
        hit = np.isfinite(z)
        nr = np.asarray(tex["NormalRoughness"], np.int16).reshape(H, W, 4)
        N, r = A.snorm16(nr[..., :3]), A.snorm16(nr[..., 3])
        P = np.asarray(tex["Position"], np.float32).reshape(H, W, 4)[..., :3].astype(T)
        mv = f16_to_f32(np.asarray(tex["MotionVector"]).reshape(H, W, 4)).astype(T)
        noisy = [np.asarray(tex[n], np.uint16).reshape(H, W, 4) for n in ("NoisyDiffuse", "NoisySpecular")]
        cur = [self._load(b) for b in noisy]
        M = T(s["MaxAccumulatedFrames"])
        dthr, nc, rf = T(s["DepthThreshold"]), T(s["NormalCosine"]), T(s["RoughnessFraction"])

        # ---- stage 1: temporal
        ys, xs = np.mgrid[0:H, 0:W]
        fx = ((xs.astype(T) + T(0.5)) + mv[..., 0]) - T(0.5)
        fy = ((ys.astype(T) + T(0.5)) + mv[..., 1]) - T(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        zp = z + mv[..., 2]
        ztol = dthr * np.abs(zp)
        wx, wy = (T(1) - tx, tx), (T(1) - ty, ty)
        ok, w, prev = [[], []], [], []
        for dx, dy in TAPS:
            xf, yf = x0 + T(dx), y0 + T(dy)
            inside = (xf >= 0) & (xf <= T(W - 1)) & (yf >= 0) & (yf <= T(H - 1)) & (self.hist is not None)
            w.append(wx[dx] * wy[dy])
            if self.hist is None:
                ok[0].append(inside); ok[1].append(inside); prev.append(None)
                continue
            xi, yi = np.where(inside, xf, 0).astype(np.int64), np.where(inside, yf, 0).astype(np.int64)
            g = {k: (v[0][yi, xi], v[1][yi, xi]) if isinstance(v, tuple) else v[yi, xi] for k, v in self.hist.items()}
            geometry = inside & (np.abs(g["z"] - zp) <= ztol) & (A.dot(N, g["N"]) >= nc)
            ok[0].append(geometry & (g["length"][0] > 0))
            ok[1].append(geometry & (g["length"][1] > 0) & (np.abs(r - g["r"]) <= rf * np.where(r > g["r"], r, g["r"])))
            prev.append(g)
        t = r / T(0.5)
        t = A.max0(np.where(t < 1, t, T(1)))
        cap_s = np.where(mv[..., 0] * mv[..., 0] + mv[..., 1] * mv[..., 1] > T(0.0625), T(1) + np.floor((M - T(1)) * t), M).astype(T)
        if self.hist is None:
            acc = [(c, np.stack([A.luminance(c), A.luminance(c) * A.luminance(c)], -1), np.ones((H, W), T)) for c in cur]
        else:
            acc = [self._accumulate(ok[0], w, prev, 0, cur[0], M), self._accumulate(ok[1], w, prev, 1, cur[1], cap_s)]
        zero = T(0)
        colour = tuple(np.where(hit[..., None], a[0], zero).astype(T) for a in acc)
        moments = tuple(np.where(hit[..., None], a[1], zero).astype(T) for a in acc)
        length = tuple(np.where(hit, a[2], zero).astype(T) for a in acc)
        self.hist = {"colour": colour, "moments": moments, "length": length, "z": z, "N": N, "r": r}
        self.length = length[0]
        out = list(colour)

        iterations = s["AtrousIterations"]
        if iterations:
            plane = dthr * np.abs(z)
            # ---- stage 2: variance
            var = []
            spatial = self._spatial_moments(colour, P, N, hit, plane)
            for ch in range(2):
                m = moments[ch]
                v = A.max0(m[..., 1] - m[..., 0] * m[..., 0])
                var.append(np.where(length[ch] < 4, spatial[ch], v).astype(T))
            # ---- stage 3: a-trous
            sigma = (T(s["DiffuseLuminanceSigma"]), T(s["SpecularLuminanceSigma"]))
            for k in range(iterations):
                out, var = self._atrous(out, var, 1 << k, P, N, r, hit, plane, sigma, rf)
        den = []
        for ch in range(2):
            den.append(np.where(hit[..., None], f_to_f16(out[ch]), noisy[ch]).astype(np.uint16))
        return den[0], den[1]

    def _spatial_moments(self, colour, P, N, hit, plane):
        A, T = self.A, self.A.T
        H, W = hit.shape
        L = [A.luminance(c) for c in colour]
        s1 = [np.zeros((H, W), T), np.zeros((H, W), T)]
        s2 = [np.zeros((H, W), T), np.zeros((H, W), T)]
        count = np.zeros((H, W), T)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                hq, inside = _shift(hit, dx, dy)
                if dx == 0 and dy == 0:
                    use = inside
                else:
                    Pq, _ = _shift(P, dx, dy)
                    Nq, _ = _shift(N, dx, dy)
                    use = inside & hq & (self._wg(N, P, Pq, plane) > 0) & (self._wn(N, Nq) > 0)
                for ch in range(2):
                    Lq, _ = _shift(L[ch], dx, dy)
                    s1[ch] = s1[ch] + np.where(use, Lq, T(0))
                    s2[ch] = s2[ch] + np.where(use, Lq * Lq, T(0))
                count = count + np.where(use, T(1), T(0))
        out = []
        for ch in range(2):
            m1, m2 = s1[ch] / count, s2[ch] / count
            out.append(A.max0(m2 - m1 * m1))
        return out

    def _atrous(self, colour, var, step, P, N, r, hit, plane, sigma, rf):
        A, T = self.A, self.A.T
        H, W = hit.shape
        # v3: the 3 x 3 binomial blur of the variance over the hit pixels of the frame
        b = [np.zeros((H, W), T), np.zeros((H, W), T)]
        bw = np.zeros((H, W), T)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                hq, inside = _shift(hit, dx, dy)
                use = inside & hq
                k = T(0.5 if dx == 0 else 0.25) * T(0.5 if dy == 0 else 0.25)
                for ch in range(2):
                    vq, _ = _shift(var[ch], dx, dy)
                    b[ch] = b[ch] + np.where(use, k * vq, T(0))
                bw = bw + np.where(use, k, T(0))
        sd = [sigma[ch] * np.sqrt(b[ch] / bw) + A.c(1e-4) for ch in range(2)]
        Lp = [A.luminance(c) for c in colour]
        acc = [np.zeros((H, W, 4), T), np.zeros((H, W, 4), T)]
        ws = [np.zeros((H, W), T), np.zeros((H, W), T)]
        va = [np.zeros((H, W), T), np.zeros((H, W), T)]
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                centre = dx == 0 and dy == 0
                hq, inside = _shift(hit, dx * step, dy * step)
                wq = [None, None]
                if centre:
                    wq = [np.full((H, W), T(0.140625)), np.full((H, W), T(0.140625))]
                else:
                    Pq, _ = _shift(P, dx * step, dy * step)
                    Nq, _ = _shift(N, dx * step, dy * step)
                    rq, _ = _shift(r, dx * step, dy * step)
                    base = ((T(H5[dy + 2]) * T(H5[dx + 2])) * self._wg(N, P, Pq, plane)) * self._wn(N, Nq)
                    wr = A.max0(T(1) - np.abs(rq - r) / (rf * np.where(r > rq, r, rq) + A.c(1e-6)))
                    for ch in range(2):
                        Lq, _ = _shift(Lp[ch], dx * step, dy * step)
                        wl = A.max0(T(1) - np.abs(Lq - Lp[ch]) / sd[ch])
                        wq[ch] = np.where(inside & hq, base * wl if ch == 0 else (base * wl) * wr, T(0)).astype(T)
                for ch in range(2):
                    cq, _ = _shift(colour[ch], dx * step, dy * step)
                    vq, _ = _shift(var[ch], dx * step, dy * step)
                    use = wq[ch] > 0
                    ws[ch] = ws[ch] + np.where(use, wq[ch], T(0))
                    va[ch] = va[ch] + np.where(use, (wq[ch] * wq[ch]) * vq, T(0))
                    acc[ch] = acc[ch] + np.where(use[..., None], wq[ch][..., None] * cq, T(0))
        out = [(acc[ch] / ws[ch][..., None]).astype(T) for ch in range(2)]
        new_var = [(va[ch] / (ws[ch] * ws[ch])).astype(T) for ch in range(2)]
        return out, new_var


def synthetic_frames(W, H, seed, frames=3):
    """The hostile sequence of the bit-for-bit tests: `frames` consecutive texture sets of a W x H frame (dicts of numpy arrays).
    A slanted plane with a depth edge and a normal edge at x = 0.6 W, a roughness step at y = H / 2, a tenth of the pixels missed
    (another tenth each frame), motion that is sub-pixel (left), three pixels (middle) and, in strips, leaves the frame (x < 3: five
    pixels to the left) or fails the depth test (rows 4-5: the previous depth 1 further); a few motion vectors that are not finite;
    noisy texels of 0, negative values, NaN, +-inf and 65504 seeded in."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    edge = xs >= int(0.6 * W)
    out = []

    def f16(x):
        with np.errstate(over="ignore"):
            return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)

    for _ in range(frames):
        z = np.where(edge, 7.0, 5.0) + 0.01 * xs + 0.004 * ys
        z = (z * (1.0 + 0.002 * rng.uniform(-1, 1, (H, W)))).astype(np.float32)
        P = np.zeros((H, W, 4), np.float32)
        P[..., 0] = (xs - W / 2 + rng.uniform(-0.2, 0.2, (H, W))) * z * 0.02
        P[..., 1] = (ys - H / 2 + rng.uniform(-0.2, 0.2, (H, W))) * z * 0.02
        P[..., 2] = z
        P[..., 3] = 1e-4
        n = np.where(edge[..., None], (0.6, 0.0, -0.8), (-0.01, -0.004, -1.0)) + rng.uniform(-0.05, 0.05, (H, W, 3))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        nr = np.zeros((H, W, 4), np.int16)
        nr[..., :3] = np.round(n * 32767)
        nr[..., 3] = np.round((np.where(ys >= H // 2, 0.6, 0.2) + rng.uniform(-0.02, 0.02, (H, W))) * 32767)
        nr[rng.random((H, W)) < 0.03, 3] = 0
        mv = np.zeros((H, W, 4), np.float32)
        mv[..., 0] = np.where(xs < W // 3, 0.37, 3.0)
        mv[..., 1] = np.where(xs < W // 3, -0.21, 0.0)
        mv[..., 2] = rng.uniform(-0.01, 0.01, (H, W))
        mv[:, :3, 0] = -5.0
        mv[4:6, :, 2] = 1.0
        bad = rng.random((H, W)) < 0.02
        mv[bad, 0] = np.array([np.nan, np.inf, -np.inf, 60000.0], np.float32)[rng.integers(0, 4, int(bad.sum()))]
        dead = rng.permutation(W * H)[: max(3, W * H // 10)]
        zf = z.reshape(-1)
        zf[dead] = np.array([np.inf, -np.inf, np.nan], np.float32)[np.arange(len(dead)) % 3]
        tex = {"Position": P, "LinearDepth": zf.reshape(H, W), "NormalRoughness": nr, "MotionVector": f16(mv)}
        for name in ("NoisyDiffuse", "NoisySpecular"):
            t = f16(np.exp2(rng.uniform(-6, 4, (H, W, 4))))
            for v in (0x0000, f16(-2.5), 0x7E00, 0xFC01, 0x7C00, 0xFC00, f16(65504.0), 0x0001):
                t[rng.random((H, W, 4)) < 0.01] = v
            tex[name] = t
        out.append(tex)
    return out


def plain_frame(W, H, colour, rng=None, edge=False, motion=(0.0, 0.0, 0.0)):
    """a frame every pixel of which is hit: the plane z = 5 facing the camera, normal (0, 0, -1) (edge: the right half is the plane through
    (0, y, 7) with normal (0.8, 0, -0.6) instead, z = 7 + 4 x / 3: 2 or more behind the left one), roughness 0.5, the motion vector given,
    the noisy pair = colour (a number, or an (H, W, 4) array)"""
    ys, xs = np.mgrid[0:H, 0:W]
    right = (xs >= W // 2) & edge
    x = (xs - W // 2) * 0.1
    z = np.where(right, 7.0 + x * 4.0 / 3.0, 5.0).astype(np.float32)
    P = np.zeros((H, W, 4), np.float32)
    P[..., 0] = x; P[..., 1] = (ys - H // 2) * 0.1; P[..., 2] = z
    nr = np.zeros((H, W, 4), np.int16)
    nr[..., 0] = np.where(right, 26214, 0); nr[..., 2] = np.where(right, -19660, -32767); nr[..., 3] = 16384
    mv = np.zeros((H, W, 4), np.float16)
    mv[..., :3] = motion
    c = np.broadcast_to(np.asarray(colour, np.float32), (H, W, 4)).astype(np.float16)
    return {"Position": P, "LinearDepth": z, "NormalRoughness": nr, "MotionVector": mv.view(np.uint16),
            "NoisyDiffuse": c.view(np.uint16).copy(), "NoisySpecular": c.view(np.uint16).copy()}


def ulp16(x):
    """the spacing of the fp16 grid at |x| (float64): 2^-24 in the subnormal range"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15) - 10)
