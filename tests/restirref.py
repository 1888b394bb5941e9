"""Float64 restatement of the reservoir-reuse rules of the DI pass ("Reservoir reuse"): the RNG streams, the
neighbour-offset table, view reflection, surface position reconstruction, the neighbour and material tests, combine and the two
normalisations, and the boiling filter; the temporal and spatial passes over whole frames, which also carry the reservoirs' Visibility
word ("Reservoir visibility") and take the Raytraced normalisation's occluders (the ray itself, initial visibility and final shading:
tests/restirvisref.py). Each rule that the device computes in float32 with a discrete outcome (pixel positions, the offset table, the
boiling sum) is restated with the same float32 steps."""
import numpy as np

M32 = 0xFFFFFFFF
LUMA = np.array([0.2990, 0.5870, 0.1140])
SALT_INITIAL, SALT_TEMPORAL, SALT_SPATIAL = 0x44490001, 0x44490002, 0x44490003
OFFSET_COUNT = 8192


def lowbias32(x):
    x = x & M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32; x ^= x >> 15; x = (x * 0x846CA68B) & M32; x ^= x >> 16
    return x


class Rng:
    """seed = hash(rng_init(x, y, frame) ^ salt); each draw: LCG step, hash, 24 bits"""

    def __init__(self, px, py, frame, salt):
        seed = lowbias32(frame + 0x035F9F29)
        v = ((px << 16) | (py & 0xFFFF)) & M32
        st = seed ^ ((lowbias32(v) + 0x9E3779B9 + ((seed << 6) & M32) + (seed >> 2)) & M32)
        self.state = lowbias32(st ^ salt)

    def next(self):
        self.state = (self.state * 1664525 + 1013904223) & M32
        return np.float32(lowbias32(self.state) >> 8) * np.float32(1.0 / 16777216.0)


def offset_table():
    """8192 int8 (x, y) pairs: the R2 sequence from (0.5, 0.5), points outside the disc of radius 0.5 rejected, trunc((c - .5) * 254)"""
    phi = 1.0 / 1.3247179572447
    phi2 = phi * phi
    u = v = 0.5
    out = []
    while len(out) < OFFSET_COUNT:
        u += phi; v += phi2
        if u >= 1.0:
            u -= 1.0
        if v >= 1.0:
            v -= 1.0
        if (u - 0.5) ** 2 + (v - 0.5) ** 2 > 0.25:
            continue
        out.append((int((u - 0.5) * 254.0), int((v - 0.5) * 254.0)))
    return np.array(out, np.int8)


def spatial_offset(q, radius):
    """trunc((float)q / 127 * radius) in float32"""
    return int(np.float32(np.float32(q) / np.float32(127.0)) * np.float32(radius))


def note(stats, key, n=1):
    """bookkeeping of what a pass met (the edge witnesses of the per-pixel pins): counts, never part of a result"""
    if stats is not None:
        stats[key] = stats.get(key, 0) + n


def reflect(x, y, w, h, stats=None, what="reflect"):
    """RAB_ClampSamplePositionIntoView (one reflection). stats[what + "_left" / "_top" / "_right" / "_bottom"] count the reflections by
    edge, stats[what + "_outside"] the positions one reflection leaves outside the view."""
    if x < 0:
        x = -x
        note(stats, what + "_left")
    if y < 0:
        y = -y
        note(stats, what + "_top")
    if x >= w:
        x = 2 * w - x - 1
        note(stats, what + "_right")
    if y >= h:
        y = 2 * h - y - 1
        note(stats, what + "_bottom")
    if not (0 <= x < w and 0 <= y < h):
        note(stats, what + "_outside")
    return x, y


def hlsl_round(v):
    """HLSL round as the device computes it: rint, ties to even"""
    return int(np.rint(np.float32(v)))


def temporal_candidates(x, y, mv, w, h, rng, rounding=hlsl_round, stats=None):
    """the up-to-9 positions of the history search, reflected into view, with the draws they consume (attempts >= 1 draw x, then y).
    stats: reflect's counters under "temporal_*" (positions the search reached before it found its history pixel)"""
    px, py = rounding(np.float32(x) + np.float32(mv[0])), rounding(np.float32(y) + np.float32(mv[1]))
    for i in range(9):
        qx, qy = px, py
        if i:
            rx, ry = rng.next(), rng.next()
            qx += int(np.float32(rx - np.float32(0.5)) * np.float32(6.0)); qy += int(np.float32(ry - np.float32(0.5)) * np.float32(6.0))
        yield reflect(qx, qy, w, h, stats, "temporal")


def reconstruct_position(x, y, w, h, jitter, depth, projection_to_view, view_to_world):
    """Camera::ReconstructWorldPosition(CalculateNDC(CalculateUV(pixel, size, jitter)), depth): row-vector 4x4 matrices"""
    u, v = (x + 0.5 + jitter[0]) / w, (y + 0.5 + jitter[1]) / h
    q = np.array([u * 2 - 1, v * -2 + 1, 0.5, 1.0]) @ np.asarray(projection_to_view, np.float64).reshape(4, 4)
    p = np.array([q[0] / q[2] * depth, q[1] / q[2] * depth, depth, 1.0]) @ np.asarray(view_to_world, np.float64).reshape(4, 4)
    return p[:3]


def previous_surface_position(x, y, w, h, cam, depth):
    """a previous surface: the Previous* matrices and -- as the reference does (RTXDIAppBridge.hlsli:332) -- the current Jitter"""
    return reconstruct_position(x, y, w, h, cam["Jitter"], depth, cam["PreviousProjectionToView"], cam["PreviousViewToWorld"])


def materials_similar(a, b):
    """RAB_AreMaterialsSimilar: a / b = dicts of Roughness, F0 (rgb), Albedo (rgb)"""
    return (abs(a["Roughness"] - b["Roughness"]) <= 0.5 * max(a["Roughness"], b["Roughness"])
            and abs(LUMA @ a["F0"] - LUMA @ b["F0"]) <= 0.25 and abs(LUMA @ a["Albedo"] - LUMA @ b["Albedo"]) <= 0.25)


def neighbour_ok(a, b, depth_a, normal_threshold, depth_threshold, check_material=True):
    """shading normals, relative depth against depth_a (the expected depth for the temporal search), materials"""
    if not np.dot(a["Normal"], b["Normal"]) >= normal_threshold:
        return False
    if not abs(depth_a - b["Depth"]) <= depth_threshold * max(depth_a, b["Depth"]):
        return False
    return materials_similar(a, b) if check_material else True


class Reservoir:
    def __init__(self, light=None, W=0.0, M=0, p=0.0, age=0):
        self.light, self.W, self.M, self.p, self.age = light, W, M, p, age


class State:
    """the streaming combination: combine(s, r, x, p): w = p * r.W * r.M; sum += w; M += r.M; select r's sample when x * sum < w"""

    def __init__(self):
        self.wsum, self.M, self.light, self.p, self.src, self.age = 0.0, 0, None, 0.0, None, 0

    def combine(self, r, x, p, src):
        w = p * r.W * r.M
        self.wsum += w
        self.M += r.M
        if x * self.wsum < w:
            self.light, self.p, self.src, self.age = r.light, p, src, r.age
            return True
        return False


def temporal_resample(cur, hist, p_cur_hist, p_prev_of, rng, max_history, basic, cap=True, combine_first=False, n_search_draws=0):
    """cur: the fresh reservoir (p = p_cur of its sample); hist: the history reservoir found (or None); p_cur_hist: p_cur(y_H);
    p_prev_of(light): p at the previous surface. rng: the temporal stream after the search (n_search_draws already consumed unless
    combine_first). Returns (light, W, M, p, age)."""
    s = State()
    s.combine(cur, 0.5, cur.p, "cur")
    m_h = 0
    if hist is not None:
        m_h = min(hist.M, max_history * cur.M) if cap else hist.M
        h = Reservoir(hist.light, hist.W, m_h, p_cur_hist, hist.age + 1)
        if combine_first:                                          # mutation: the combine draw before the search draws
            x = rng[0]
        else:
            x = rng[n_search_draws]
        s.combine(h, x, p_cur_hist, "hist")
    if not s.p > 0:
        return None, 0.0, s.M, 0.0, 0
    if basic:
        p_prev = p_prev_of(s.light) if hist is not None else 0.0
        den = s.p * (cur.M * s.p + m_h * p_prev)
        W = s.wsum * (p_prev if s.src == "hist" else s.p) / den if den > 0 else 0.0
    else:
        W = s.wsum / (s.p * s.M)
    return s.light, W, s.M, s.p, s.age if s.src == "hist" else 0


def spatial_normalise(wsum, p, Ms_and_p, p_src, basic):
    """Basic: wsum * p_src / (p * sum M_c p_c(y)) over the centre and the contributing neighbours; Off: wsum / (p * sum M)"""
    if not p > 0:
        return 0.0
    if basic:
        den = p * sum(m * q for m, q in Ms_and_p)
        return wsum * p_src / den if den > 0 else 0.0
    return wsum / (p * sum(m for m, _ in Ms_and_p))


def butterfly_sum(values):
    """the wave's 64-lane sum as the device forms it: xor partners 1, 2, 4, ..., 32, in float32 (every lane ends with the same bits)"""
    v = np.asarray(values, np.float32).copy()
    lanes = np.arange(64)
    m = 1
    while m < 64:
        v = (v + v[lanes ^ m]).astype(np.float32)
        m <<= 1
    return v[0]


def note_boiling_tile(stats, pixels_in_frame, count):
    """a tile in which the boiling filter decided (count > 0 reservoirs averaged): stats["boiling_tiles"], and for a tile the frame's
    right or bottom edge cuts (fewer than 64 pixels in the frame) stats["boiling_cut_tiles"] and its count in ["boiling_cut_count"]"""
    note(stats, "boiling_tiles")
    if pixels_in_frame < 64:
        note(stats, "boiling_cut_tiles")
        note(stats, "boiling_cut_count", int(count))


def boiling_filter(W, valid, strength):
    """one 8 x 8 tile (64 lanes, row-major): True where the reservoir is emptied"""
    W = np.asarray(W, np.float32)
    nz = np.asarray(valid) & (W > 0)
    total = butterfly_sum(np.where(nz, W, np.float32(0)))
    count = butterfly_sum(nz.astype(np.float32))
    if not count > 0:
        return np.zeros(64, bool)
    mul = np.float32(np.float32(10.0) / np.float32(min(max(strength, 1e-6), 1.0))) - np.float32(9.0)
    return W > np.float32(total / count) * mul


# ---- the passes over whole frames, for the per-pixel pins ------------------------------------------------------------------------
def _snorm(q):
    return np.maximum(np.asarray(q, np.float64) / 32767.0, -1.0)


def _oct_decode(e):
    x, y = e[..., 0], e[..., 1]
    z = 1.0 - np.abs(x) - np.abs(y)
    t = np.maximum(-z, 0.0)
    x = x + np.where(x >= 0, -t, t); y = y + np.where(y >= 0, -t, t)
    v = np.stack([x, y, z], -1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class Surfaces:
    """RAB_GetGBufferSurface over a whole G-buffer (numpy dict of textures_to_numpy planes, names without Previous), float64.
    cam: PtCamera record; previous=True uses the Previous* matrices and PreviousPosition with the current Jitter."""

    def __init__(self, gb, cam, previous=False):
        pre = "Previous" if previous else ""
        g = lambda n: gb[pre + n]
        self.depth = g("LinearDepth")[..., 0].astype(np.float64)
        H, W = self.depth.shape
        nr = g("NormalRoughness")
        rough = _snorm(nr[..., 3])
        self.valid = np.isfinite(self.depth) & (rough >= 0.05)
        d = np.where(self.valid, self.depth, 0.0)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        u, v = (xs + 0.5 + cam["Jitter"][0]) / W, (ys + 0.5 + cam["Jitter"][1]) / H
        ndc = np.stack([u * 2 - 1, v * -2 + 1, np.full_like(u, 0.5), np.ones_like(u)], -1)
        q = ndc @ cam[pre + "ProjectionToView"].reshape(4, 4).astype(np.float64)
        vp = np.stack([q[..., 0] / q[..., 2] * d, q[..., 1] / q[..., 2] * d, d, np.ones_like(d)], -1)
        self.P = (vp @ cam[pre + "ViewToWorld"].reshape(4, 4).astype(np.float64))[..., :3]
        V = cam[pre + "Position"].astype(np.float64) - self.P
        self.V = V / np.maximum(np.linalg.norm(V, axis=-1, keepdims=True), 1e-300)
        self.gn = _oct_decode(_snorm(g("GeometricNormal")))
        self.front = (self.gn * self.V).sum(-1) > 0
        self.Ns = _snorm(nr[..., :3])
        bcm = g("BaseColorMetalness").astype(np.float64) / 255.0
        self.base, self.metal, self.rough = bcm[..., :3], bcm[..., 3], rough
        self.ior = g("IOR")[..., 0].view(np.float16).astype(np.float64)
        self.trans = np.where(self.metal < 1, g("Transmission")[..., 0].astype(np.float64) / 255.0, 0.0)
        r = np.maximum(2e-3, rough)
        iori, ioro = np.where(self.front, 1.0, self.ior), np.where(self.front, self.ior, 1.0)
        r2 = ((iori - ioro) / (iori + ioro)) ** 2
        self.F0 = r2[..., None] + (self.base - r2[..., None]) * self.metal[..., None]
        self.albedo = self.base * (1 - self.metal)[..., None]
        self.r = r
        self.W, self.H = W, H

    def material(self, y, x):
        return {"Normal": self.Ns[y, x], "Depth": self.depth[y, x], "Roughness": self.r[y, x], "F0": self.F0[y, x], "Albedo": self.albedo[y, x]}


def target_pdfs(S, pix, lights, li, U, V, bsdf, margins=None):
    """p-hat of samples (li, U, V) at surface pixels pix [(y, x)]: luminance of the all-lobe Shade (bsdfref evaluate_all), float64.
    margins: a list that receives, per sample, the smallest |cosine| of L against the geometric and shading normals (where the BSDF
    switches between reflection, transmission and zero) and against the light's normal (where p-hat is ill-conditioned)"""
    n = len(pix)
    out = np.zeros(n)
    if n == 0:
        return out
    ys, xs = np.array(pix, np.int64).reshape(-1, 2).T
    li = np.asarray(li, np.int64)
    ok = (li >= 0) & (li < len(lights))
    lt = lights[np.where(ok, li, 0)]
    base, e0, e1 = (lt[k].astype(np.float64) for k in ("Base", "Edge0", "Edge1"))
    s = np.sqrt(np.asarray(U, np.float64))[:, None]
    Vv = np.asarray(V, np.float64)[:, None]
    pos = base + e0 * (s * (1 - Vv)) + e1 * (s * Vv)
    d = pos - S.P[ys, xs]
    ln = np.linalg.norm(d, axis=-1)
    dn = d / np.maximum(ln, 1e-300)[:, None]
    cosL = np.abs((dn * -lt["Normal"].astype(np.float64)).sum(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = (1.0 / lt["Area"].astype(np.float64)) * ln * ln / cosL
    q = np.zeros((n, 20))
    q[:, 0:3], q[:, 3], q[:, 4], q[:, 5], q[:, 6] = S.base[ys, xs], S.metal[ys, xs], S.rough[ys, xs], S.ior[ys, xs], S.trans[ys, xs]
    q[:, 7] = S.front[ys, xs]
    q[:, 8:11], q[:, 11:14], q[:, 14:17], q[:, 17:20] = S.gn[ys, xs], S.Ns[ys, xs], S.V[ys, xs], dn
    dif, spc, _pdf = bsdf.evaluate_all(q)[:3]
    Le = lt["Radiance"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = ((dif + spc) * Le / pdf[:, None]) @ LUMA
    good = ok & (pdf > 0) & np.isfinite(pdf) & np.isfinite(p)
    out[good] = p[good]
    if margins is not None:
        m = np.minimum(np.abs((S.gn[ys, xs] * dn).sum(-1)), np.abs((S.Ns[ys, xs] * dn).sum(-1)))
        m = np.minimum(m, cosL)                                          # p-hat ~ cosL: its relative error grows as 1 / cosL
        margins.extend(np.where(ok, m, np.inf).tolist())
    return out


def _margin(a, b):
    """relative distance of a comparison a <op> b from its boundary"""
    return abs(a - b) / max(abs(a), abs(b), 1e-30)


def roughness_margin(ra, rb):
    """the margin of RAB_AreMaterialsSimilar's roughness test, |ra - rb| <= 0.5 max(ra, rb). One roughness exactly twice the other -- the
    pin scene's floor and bar: snorm16 codes 13107 and 26214 -- is a tie, not a decision at risk: doubling is exact in binary floating
    point, so the decoded values keep the ratio in float32 as in float64, |ra - rb| is the smaller one and 0.5 max the same bits without
    a rounding anywhere, and `<=` holds in every arithmetic."""
    lo, hi = min(ra, rb), max(ra, rb)
    if hi == 2.0 * lo and np.float32(hi) == np.float32(2.0) * np.float32(lo):
        return np.inf
    return _margin(abs(ra - rb), 0.5 * hi)


# ---- the Visibility word of a reservoir ("Reservoir visibility") ------------------------------------------------
def pack(rgb, dx=0, dy=0, age=0):
    """bits 0-14: uint(clamp(v, 0, 1) * 31) per channel (float32, as stored); 15-20 / 21-26: dx, dy as 6-bit two's complement clamped to
    +-31; 27-30: age saturating at 15; bit 31: 0"""
    c = [int(np.float32(min(max(np.float32(v), np.float32(0)), np.float32(1))) * np.float32(31)) for v in rgb]
    dx, dy = max(-31, min(31, int(dx))), max(-31, min(31, int(dy)))
    return c[0] | c[1] << 5 | c[2] << 10 | (dx & 63) << 15 | (dy & 63) << 21 | min(int(age), 15) << 27


def unpack(word):
    """-> (rgb in [0, 1], dx, dy, age)"""
    w = int(word)
    s6 = lambda v: v - 64 if v & 32 else v
    return (np.array([w & 31, (w >> 5) & 31, (w >> 10) & 31]) / 31.0, s6((w >> 15) & 63), s6((w >> 21) & 63), (w >> 27) & 15)


def carry(word, ddx, ddy, dage):
    """the word of a sample taken from the pixel at offset (ddx, ddy), dage frames later: the colour stays, d and age move and saturate"""
    _, dx, dy, age = unpack(word)
    w = int(word)
    dx, dy = max(-31, min(31, dx + ddx)), max(-31, min(31, dy + ddy))
    return (w & 0x7FFF) | (dx & 63) << 15 | (dy & 63) << 21 | min(age + dage, 15) << 27


def reusable(word, max_age, max_distance):
    """final shading may use the stored visibility: 1 <= age <= max_age and sqrt(dx^2 + dy^2) < max_distance (float32, as compared)"""
    _, dx, dy, age = unpack(word)
    return 1 <= age <= max_age and bool(np.sqrt(np.float32(dx * dx + dy * dy)) < np.float32(max_distance))


def reuse_margin(word, max_distance):
    """relative distance of the distance test from its boundary (the age test is on integers)"""
    _, dx, dy, _ = unpack(word)
    return _margin(float(np.sqrt(float(dx * dx + dy * dy))), float(max_distance))


def sample_points(lights, li, U, V):
    """Math::SampleTriangle(r1 = U, r2 = V) on light records li: base + e0 * sqrt(U) (1 - V) + e1 * sqrt(U) V"""
    lt = lights[np.asarray(li, np.int64)]
    s = np.sqrt(np.asarray(U, np.float64))[:, None]
    v = np.asarray(V, np.float64)[:, None]
    return lt["Base"].astype(np.float64) + lt["Edge0"].astype(np.float64) * (s * (1 - v)) + lt["Edge1"].astype(np.float64) * (s * v)


# ---- reservoir frames: dicts of [H, W] arrays, LightIndex -1 = empty ---------------------------------------------------------------
FIELDS = ("LightIndex", "U", "V", "W", "M", "TargetPdf", "Age", "Visibility")


def as_frame(res, H, W):
    """a downloaded DI_RESERVOIR array -> dict of [H, W] arrays (float64 / int64), LightIndex -1 = empty"""
    out = {k: res[k].reshape(H, W).astype(np.float64 if res.dtype[k].kind == "f" else np.int64) for k in res.dtype.names}
    out["LightIndex"] = np.where(res["LightIndex"].reshape(H, W) == 0xFFFFFFFF, -1, out["LightIndex"])
    return out


def empty(out, c, M):
    for k in FIELDS:
        out[k][c] = 0
    out["LightIndex"][c], out["M"][c] = -1, M


def temporal_pass(cur, prev, mv, fresh, history, lights, frame, bsdf, max_history, basic, boiling, strength, depth_thr=0.1, normal_thr=0.5,
                  in_margin=None, occ=None, raytraced=False, stats=None):
    """k_di_initial_temporal's reuse over a frame. fresh / history: frames (the initial reservoirs of this frame, after initial visibility
    if that is on, with their margin in_margin, and last frame's final ones, or None: no history). A selected history sample takes the
    history pixel's Visibility moved by (hx - x, hy - y) and one frame older. raytraced (with basic): p at the previous surface := 0 when
    the ray from the current surface to the selected sample is blocked by occ (restirvisref.Occluders), traced only when a history pixel
    was found and that p > 0; stats["zeroed"] counts the zeroed terms. Returns (frame, margin [H, W])."""
    H, W = cur.H, cur.W
    out = {k: np.zeros((H, W), np.float64 if k in ("U", "V", "W", "TargetPdf") else np.int64) for k in FIELDS}
    out["LightIndex"][:] = -1
    margin = np.full((H, W), np.inf) if in_margin is None else np.array(in_margin, np.float64)
    found = {}
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x]:
                margin[y, x] = np.inf
                continue
            for k in ("LightIndex", "U", "V", "W", "M", "TargetPdf"):
                out[k][y, x] = fresh[k][y, x]
            if history is None:
                continue
            rng = Rng(x, y, frame, SALT_TEMPORAL)
            mvx, mvy, mvz = (np.float32(v) for v in mv[y, x, :3])
            expected = np.float32(np.float32(cur.depth[y, x]) + mvz)
            for c in (np.float32(x) + mvx, np.float32(y) + mvy):
                margin[y, x] = min(margin[y, x], abs(abs(float(c) - np.floor(float(c))) - 0.5))
            a = cur.material(y, x)
            for qx, qy in temporal_candidates(x, y, (mvx, mvy), W, H, rng, stats=stats):
                if not (0 <= qx < W and 0 <= qy < H) or not prev.valid[qy, qx]:
                    continue
                b = prev.material(qy, qx)
                margin[y, x] = min(margin[y, x], _margin(np.dot(a["Normal"], b["Normal"]), normal_thr),
                                   _margin(abs(float(expected) - b["Depth"]), depth_thr * max(float(expected), b["Depth"])),
                                   roughness_margin(a["Roughness"], b["Roughness"]),
                                   _margin(abs(LUMA @ a["F0"] - LUMA @ b["F0"]), 0.25),
                                   _margin(abs(LUMA @ a["Albedo"] - LUMA @ b["Albedo"]), 0.25))
                if neighbour_ok(a, b, float(expected), normal_thr, depth_thr):
                    found[(y, x)] = (qy, qx, rng.next())
                    break
    keys = list(found)
    Hs = [{k: history[k][qy, qx] for k in FIELDS} for (qy, qx, _) in found.values()]
    mH = []
    pH = target_pdfs(cur, keys, lights, [h["LightIndex"] for h in Hs], [h["U"] for h in Hs], [h["V"] for h in Hs], bsdf, mH)
    for k, m in zip(keys, mH):
        margin[k] = min(margin[k], m)
    sel_from_h = {}
    for (y, x), h, ph in zip(keys, Hs, pH):
        mcur = int(out["M"][y, x])
        mh = min(int(h["M"]), max_history * mcur)
        w0 = out["TargetPdf"][y, x] * out["W"][y, x] * mcur
        wH = ph * float(h["W"]) * mh
        wsum = w0 + wH
        rc = float(found[(y, x)][2])
        margin[y, x] = min(margin[y, x], _margin(rc * wsum, wH) if wH > 0 else np.inf)
        fromH = rc * wsum < wH
        if fromH:
            qy, qx = found[(y, x)][:2]
            out["LightIndex"][y, x], out["U"][y, x], out["V"][y, x] = int(h["LightIndex"]), float(h["U"]), float(h["V"])
            out["TargetPdf"][y, x], out["Age"][y, x] = ph, int(h["Age"]) + 1
            out["Visibility"][y, x] = carry(int(h["Visibility"]), qx - x, qy - y, 1)
        out["M"][y, x] = mcur + mh
        sel_from_h[(y, x)] = (fromH, mh, wsum, mcur)
    need = [(y, x) for (y, x) in sel_from_h if out["TargetPdf"][y, x] > 0]
    mP = []
    pprev = target_pdfs(prev, [(found[k][0], found[k][1]) for k in need], lights, [out["LightIndex"][k] for k in need],
                          [out["U"][k] for k in need], [out["V"][k] for k in need], bsdf, mP) if basic else []
    for k, m in zip(need, mP):
        margin[k] = min(margin[k], m)
    pprev = dict(zip(need, pprev))
    if basic and raytraced:
        rays = [k for k in need if pprev[k] > 0]
        if rays:
            ys, xs = np.array(rays).T
            blocked, _, m = occ.trace(cur.P[ys, xs], sample_points(lights, out["LightIndex"][ys, xs], out["U"][ys, xs], out["V"][ys, xs]))
            for k, b, mm in zip(rays, blocked, m):
                margin[k] = min(margin[k], mm)
                if b:
                    pprev[k] = 0.0
                    if stats is not None:
                        stats["zeroed"] = stats.get("zeroed", 0) + 1
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x] or history is None:
                continue
            p = out["TargetPdf"][y, x]
            if not p > 0:
                empty(out, (y, x), out["M"][y, x])
                continue
            fromH, mh, wsum, mcur = sel_from_h.get((y, x), (False, 0, None, int(out["M"][y, x])))
            if wsum is None:
                wsum = p * out["W"][y, x] * mcur
            if basic:
                pp = pprev.get((y, x), 0.0)
                den = p * (mcur * p + mh * pp)
                out["W"][y, x] = wsum * (pp if fromH else p) / den if den > 0 else 0.0
            else:
                out["W"][y, x] = wsum / (p * out["M"][y, x])
    if boiling:
        for ty in range(0, H, 8):
            for tx in range(0, W, 8):
                Wt = np.zeros(64, np.float32); vt = np.zeros(64, bool); idx = []
                for ln in range(64):
                    y, x = ty + ln // 8, tx + ln % 8
                    if y < H and x < W:
                        Wt[ln], vt[ln] = out["W"][y, x], cur.valid[y, x]
                        idx.append((ln, y, x))
                nz = vt & (Wt > 0)
                total, count = butterfly_sum(np.where(nz, Wt, 0)), butterfly_sum(nz.astype(np.float32))
                if not count > 0:
                    continue
                note_boiling_tile(stats, len(idx), count)
                mul = np.float32(np.float32(10.0) / np.float32(min(max(strength, 1e-6), 1.0))) - np.float32(9.0)
                thr = float(np.float32(total / count) * mul)
                for ln, y, x in idx:
                    if nz[ln]:
                        margin[y, x] = min(margin[y, x], _margin(float(Wt[ln]), thr))
                        if Wt[ln] > thr:
                            empty(out, (y, x), 0)
                            note(stats, "boiling_emptied" if len(idx) == 64 else "boiling_cut_emptied")
                tmin = min((margin[y, x] for _, y, x in idx), default=np.inf)
                if tmin < 1e-5:
                    for _, y, x in idx:
                        margin[y, x] = min(margin[y, x], tmin)
    return out, margin


def spatial_pass(cur, inp, in_margin, lights, table, frame, bsdf, samples, boost, max_history, radius, basic, depth_thr=0.1, normal_thr=0.5,
                 occ=None, raytraced=False, stats=None):
    """k_di_spatial_shade's reuse over a frame: inp = the temporal output. A selected neighbour's sample takes its Visibility moved by
    (qx - x, qy - y). raytraced (with basic): in the normalisation a contributing neighbour's p := 0 when the ray from that neighbour's
    surface to the selected sample is blocked by occ (traced only when that p > 0; the centre's own term is not tested). Returns
    (frame, margin)."""
    H, W = cur.H, cur.W
    out = {k: np.array(inp[k]).copy() for k in FIELDS}
    margin = np.array(in_margin, np.float64).copy()
    plan = {}
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x]:
                continue
            rng = Rng(x, y, frame, SALT_SPATIAL)
            start = int(np.float32(rng.next()) * np.float32(8191.0))
            n = max(samples, boost) if inp["M"][y, x] < max_history else samples
            a = cur.material(y, x)
            nb = []
            for i in range(n):
                e = table[(start + i) & 8191]
                qx, qy = reflect(x + spatial_offset(int(e[0]), radius), y + spatial_offset(int(e[1]), radius), W, H, stats, "spatial")
                if not (0 <= qx < W and 0 <= qy < H) or not cur.valid[qy, qx]:
                    continue
                b = cur.material(qy, qx)
                margin[y, x] = min(margin[y, x], _margin(np.dot(a["Normal"], b["Normal"]), normal_thr),
                                   _margin(abs(a["Depth"] - b["Depth"]), depth_thr * max(a["Depth"], b["Depth"])),
                                   roughness_margin(a["Roughness"], b["Roughness"]),
                                   _margin(abs(LUMA @ a["F0"] - LUMA @ b["F0"]), 0.25),
                                   _margin(abs(LUMA @ a["Albedo"] - LUMA @ b["Albedo"]), 0.25))
                if neighbour_ok(a, b, a["Depth"], normal_thr, depth_thr):
                    nb.append((qy, qx, rng.next()))
                    margin[y, x] = min(margin[y, x], in_margin[qy, qx])
            plan[(y, x)] = nb
    pairs = [((y, x), (qy, qx)) for (y, x), nb in plan.items() for (qy, qx, _) in nb]
    mN = []
    pn = target_pdfs(cur, [c for c, _ in pairs], lights, [inp["LightIndex"][q] for _, q in pairs], [inp["U"][q] for _, q in pairs],
                       [inp["V"][q] for _, q in pairs], bsdf, mN)
    for (c, _), m in zip(pairs, mN):
        margin[c] = min(margin[c], m)
    pn = iter(pn)
    sel = {}
    for (y, x), nb in plan.items():
        c = (y, x)
        wsum = inp["TargetPdf"][c] * inp["W"][c] * inp["M"][c]
        M, s = int(inp["M"][c]), -1
        for i, (qy, qx, rc) in enumerate(nb):
            p = next(pn)
            w = p * inp["W"][qy, qx] * inp["M"][qy, qx]
            wsum += w; M += int(inp["M"][qy, qx])
            if w > 0:
                margin[c] = min(margin[c], _margin(float(rc) * wsum, w))
            if float(rc) * wsum < w:
                s = i
                for k in ("LightIndex", "U", "V", "Age"):
                    out[k][c] = inp[k][qy, qx]
                out["TargetPdf"][c] = p
                out["Visibility"][c] = carry(int(inp["Visibility"][qy, qx]), qx - x, qy - y, 0)
        out["M"][c] = M
        sel[c] = (s, wsum)
    pc = {}
    if basic:
        q = [((y, x), (qy, qx)) for (y, x), nb in plan.items() if out["TargetPdf"][y, x] > 0 for (qy, qx, _) in nb]
        mC = []
        vals = target_pdfs(cur, [n for _, n in q], lights, [out["LightIndex"][c] for c, _ in q], [out["U"][c] for c, _ in q],
                             [out["V"][c] for c, _ in q], bsdf, mC)
        for (c, _), m in zip(q, mC):
            margin[c] = min(margin[c], m)
        vals = list(vals)
        if raytraced:
            rays = [j for j, v in enumerate(vals) if v > 0]
            if rays:
                cs = np.array([q[j][0] for j in rays]); ns = np.array([q[j][1] for j in rays])
                blocked, _, m = occ.trace(cur.P[ns[:, 0], ns[:, 1]],
                                          sample_points(lights, out["LightIndex"][cs[:, 0], cs[:, 1]], out["U"][cs[:, 0], cs[:, 1]], out["V"][cs[:, 0], cs[:, 1]]))
                for j, b, mm in zip(rays, blocked, m):
                    margin[q[j][0]] = min(margin[q[j][0]], mm)
                    if b:
                        vals[j] = 0.0
                        if stats is not None:
                            stats["zeroed"] = stats.get("zeroed", 0) + 1
        vals = iter(vals)
        for (y, x), nb in plan.items():
            if out["TargetPdf"][y, x] > 0:
                pc[(y, x)] = [next(vals) for _ in nb]
    for (y, x), nb in plan.items():
        c = (y, x)
        p = out["TargetPdf"][c]
        s, wsum = sel[c]
        if not p > 0:
            empty(out, c, out["M"][c])
            continue
        if basic:
            den, psrc = inp["M"][c] * p, p
            for i, ((qy, qx, _), pq) in enumerate(zip(nb, pc[c])):
                den += inp["M"][qy, qx] * pq
                if i == s:
                    psrc = pq
            den *= p
            out["W"][c] = wsum * psrc / den if den > 0 else 0.0
        else:
            out["W"][c] = wsum / (p * out["M"][c])
    return out, margin


