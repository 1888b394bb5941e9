"""Restatement of initial sampling with BRDF candidates ("BRDF candidates").

Two halves. The candidates themselves are discrete all the way -- a sampled direction, a ray, a triangle -- and are pinned bit for bit
through pieces the device and the CPU oracle already agree on: surfaces_f32 rebuilds RAB_GetGBufferSurface from a G-buffer with the
device's float32 steps (every fused multiply-add where the device has one), and replay_candidates runs or_bsdf_sample_batch,
or_bsdf_evaluate and or_trace_closest on them. The weights are continuous and are restated in float64 on restirref's Rng and Surfaces and
bsdfref's all-lobe evaluate: the two streams and their draw order, RandomFromBarycentrics, the blended pdf, the streaming selection,
W and M, and a per-pixel margin -- the distance of every coin from its threshold, of a cutoff distance from its limit, and of the
cosines at which the BSDF or p-hat turns ill-conditioned from 0."""
import numpy as np

import restirref as R

SALT_BRDF = 0x44490008
FLT_MAX = np.float32(3.402823466e+38)
f32 = np.float32

CANDIDATE = np.dtype([("LightIndex", "<u4"), ("U", "<f4"), ("V", "<f4"), ("BrdfPdf", "<f4")])
CLOSEST = np.dtype([("T", "<f4"), ("U", "<f4"), ("V", "<f4"), ("Inst", "<u4"), ("Geom", "<u4"), ("Prim", "<u4"), ("Slot", "<u4"), ("_", "<u4")])


# ---- float32 steps -------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf on float32 arrays, exactly. The product of two float32 is exact in float64; the float64 sum is rounded to float32, and where
    that sum sits exactly halfway between two float32 its rounding error (TwoSum) says which of them the true sum is nearer to."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        other = np.where(d > 0, np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf))).astype(np.float64)
        tie = (d != 0) & (r.astype(np.float64) + 2.0 * d == other)
    return np.where(tie & (e * d > 0), other, r.astype(np.float64)).astype(np.float32)


def dot32(a, b):
    """sop3: mad(a.z, b.z, mad(a.y, b.y, a.x * b.x))"""
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(np.float32)))


def normalize32(v):
    inv = (f32(1.0) / np.sqrt(dot32(v, v))).astype(np.float32)
    return (v * inv[..., None]).astype(np.float32)


def xform4_32(M, p):
    """row-vector 4x4 with w = 1: out[j] = mad(p.z, M[8 + j], mad(p.y, M[4 + j], mad(p.x, M[j], M[12 + j])))"""
    M = np.asarray(M, np.float32).reshape(-1)
    return np.stack([fma32(p[..., 2], M[8 + j], fma32(p[..., 1], M[4 + j], fma32(p[..., 0], M[j], np.broadcast_to(M[12 + j], p[..., 0].shape))))
                     for j in range(4)], -1)


def div_const32(x, c):
    """PT_DIV_CONST: (float)((double)x * (1.0 / (double)c))"""
    return (np.asarray(x, np.float32).astype(np.float64) * (1.0 / float(c))).astype(np.float32)


def snorm16_32(v):
    v = np.asarray(v, np.int16)
    return np.where(v == -32768, f32(-1.0), div_const32(v.astype(np.float32), 32767.0)).astype(np.float32)


def oct_decode32(px, py):
    z = ((f32(1.0) - np.abs(px)).astype(np.float32) - np.abs(py)).astype(np.float32)
    t = np.minimum(np.maximum(-z, f32(0.0)), f32(1.0)).astype(np.float32)
    x = (px - (t * np.where(px >= 0, f32(1.0), f32(-1.0))).astype(np.float32)).astype(np.float32)
    y = (py - (t * np.where(py >= 0, f32(1.0), f32(-1.0))).astype(np.float32)).astype(np.float32)
    return normalize32(np.stack([x, y, z], -1))


def surfaces_f32(gb, cam):
    """RAB_GetGBufferSurface over a G-buffer (numpy planes as textures_to_numpy / the oracle write them) with the device's float32
    arithmetic (pt_di.hip di_surface): dict of [H, W] arrays. What or_bsdf_sample_batch needs of a surface, bit for bit."""
    depth = gb["LinearDepth"][..., 0].astype(np.float32)
    H, W = depth.shape
    nr = gb["NormalRoughness"].view(np.int16)
    rough = snorm16_32(nr[..., 3])
    valid = np.isfinite(depth) & (rough >= f32(0.05))
    d = np.where(valid, depth, f32(1.0)).astype(np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    jx, jy = f32(cam["Jitter"][0]), f32(cam["Jitter"][1])
    u = (((xs.astype(np.float32) + f32(0.5)).astype(np.float32) + jx).astype(np.float32) / f32(W)).astype(np.float32)
    v = (((ys.astype(np.float32) + f32(0.5)).astype(np.float32) + jy).astype(np.float32) / f32(H)).astype(np.float32)
    ndc = np.stack([((u * f32(2.0)).astype(np.float32) + f32(-1.0)).astype(np.float32),
                    ((v * f32(-2.0)).astype(np.float32) + f32(1.0)).astype(np.float32), np.full_like(u, f32(0.5))], -1)
    q = xform4_32(cam["ProjectionToView"], ndc)
    vp = np.stack([((q[..., 0] / q[..., 2]).astype(np.float32) * d).astype(np.float32),
                   ((q[..., 1] / q[..., 2]).astype(np.float32) * d).astype(np.float32), d], -1)
    P = xform4_32(cam["ViewToWorld"], vp)[..., :3]
    V = normalize32((np.asarray(cam["Position"], np.float32)[:3] - P).astype(np.float32))
    ge = gb["GeometricNormal"].view(np.int16)
    gn = oct_decode32(snorm16_32(ge[..., 0]), snorm16_32(ge[..., 1]))
    front = dot32(gn, V) > 0
    Ns = np.stack([snorm16_32(nr[..., k]) for k in range(3)], -1)
    bcm = gb["BaseColorMetalness"]
    base = np.stack([div_const32(bcm[..., k].astype(np.float32), 255.0) for k in range(3)], -1)
    metal = div_const32(bcm[..., 3].astype(np.float32), 255.0)
    trans = np.where(metal < f32(1.0), div_const32(gb["Transmission"][..., 0].astype(np.float32), 255.0), f32(0.0)).astype(np.float32)
    ior = gb["IOR"][..., 0].view(np.float16).astype(np.float32)
    return {"valid": valid, "P": P, "V": V, "gn": gn, "Ns": Ns, "front": front, "base": base, "metal": metal, "rough": rough, "ior": ior,
            "trans": trans, "H": H, "W": W}


def random_from_barycentrics(b1, b2):
    """Math::RandomFromBarycentrics in float32: hit barycentrics (b1, b2) of vertices 1 and 2 -> the (U, V) Math::SampleTriangle maps back
    to them: t = b1 + b2, U = t t, V = b2 / t; (0, 0) at t = 0"""
    b1, b2 = np.asarray(b1, np.float32), np.asarray(b2, np.float32)
    t = (b1 + b2).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        U, V = (t * t).astype(np.float32), (b2 / t).astype(np.float32)
    return np.where(t != 0, U, f32(0)).astype(np.float32), np.where(t != 0, V, f32(0)).astype(np.float32)


def sample_triangle(U, V):
    """Math::SampleTriangle's barycentrics of vertices 1 and 2 for (r1, r2) = (U, V), float64"""
    s = np.sqrt(np.asarray(U, np.float64))
    return s * (1 - np.asarray(V, np.float64)), s * np.asarray(V, np.float64)


def brdf_draws(x, y, frame, n_b):
    """the BRDF stream of a pixel: [n_b, 5] float32, r0..r3 (Sample) and r4 (the coin) per candidate"""
    rng = R.Rng(x, y, frame, SALT_BRDF)
    return np.array([[rng.next() for _ in range(5)] for _ in range(n_b)], np.float32).reshape(n_b, 5)


def brdf_range(cutoff, q):
    """how far a BRDF ray of pdf q reaches: sqrt((1 / cutoff - 1) q) in float32"""
    return np.sqrt((((f32(1.0) / f32(cutoff)).astype(np.float32) - f32(1.0)).astype(np.float32) * np.asarray(q, np.float32)).astype(np.float32))


def light_lookup(lights):
    return {(int(l["InstanceIndex"]), int(l["GeometryIndex"]), int(l["PrimitiveIndex"])): i for i, l in enumerate(lights)}


def replay_candidates(oracle, osc, sf, lights, frame, n_b, cutoff, ext=0):
    """The BRDF candidates of every valid pixel through the CPU oracle: or_bsdf_sample_batch on the float32 surfaces with the stream's
    r0..r3, the all-lobe pdf of the direction by or_bsdf_evaluate, or_trace_closest on (P, 1e-3, L, tmax), the hit mapped to a light.
    Returns (records [H, W, n_b] CANDIDATE, info): info["t"] the hit distance of a candidate on a light, info["stopped"] the instance a
    ray stopped on (-1: none), info["beyond"]: the ray ended inside its range with nothing hit, and unbounded it would have reached a light
    (cutoff > 0 only, else None)."""
    lib = oracle.lib()
    H, W = sf["H"], sf["W"]
    rec = np.zeros((H, W, n_b), CANDIDATE)
    rec["LightIndex"] = 0xFFFFFFFF
    t_hit = np.full((H, W, n_b), np.nan, np.float32)
    stopped = np.full((H, W, n_b), -1, np.int64)
    beyond = np.zeros((H, W, n_b), bool) if cutoff > 0 else None
    ys, xs = np.nonzero(sf["valid"])
    n = len(ys)
    if n == 0:
        return rec, {"t": t_hit, "stopped": stopped, "beyond": beyond}
    draws = np.stack([brdf_draws(int(x), int(y), frame, n_b) for y, x in zip(ys, xs)])
    lookup = light_lookup(lights)
    q = np.zeros((n, 24), np.float32)
    q[:, 0:3], q[:, 3], q[:, 4], q[:, 5], q[:, 6] = sf["base"][ys, xs], sf["metal"][ys, xs], sf["rough"][ys, xs], sf["ior"][ys, xs], sf["trans"][ys, xs]
    q[:, 7] = sf["front"][ys, xs]
    q[:, 8:11], q[:, 11:14], q[:, 14:17] = sf["gn"][ys, xs], sf["Ns"][ys, xs], sf["V"][ys, xs]
    q[:, 21] = np.array([ext], np.uint32).view(np.float32)[0]
    for j in range(n_b):
        q[:, 17:21] = draws[:, j, :4]
        qq = np.ascontiguousarray(q)
        r = np.zeros((n, 12), np.float32)
        lib.or_bsdf_sample_batch(qq.ctypes.data, n, r.ctypes.data)
        ok = r[:, 11].view(np.uint32) != 0
        e = np.ascontiguousarray(np.concatenate([q[:, :17], r[:, :3]], 1))
        ev = np.zeros((n, 8), np.float32)
        lib.or_bsdf_evaluate(e.ctypes.data, n, ev.ctypes.data)
        qb = ev[:, 6]
        go = ok & (qb > 0)
        tmax = brdf_range(cutoff, qb) if cutoff > 0 else np.full(n, FLT_MAX, np.float32)
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = sf["P"][ys, xs], f32(1e-3), r[:, :3], tmax
        idx = np.nonzero(go)[0]
        hits = np.zeros(len(idx), CLOSEST)
        if len(idx):
            rr = np.ascontiguousarray(rays[idx])
            lib.or_trace_closest(osc.handle, rr.ctypes.data, len(idx), hits.ctypes.data)
        far = None
        if cutoff > 0 and len(idx):
            rr = np.ascontiguousarray(rays[idx]); rr[:, 7] = FLT_MAX
            far = np.zeros(len(idx), CLOSEST)
            lib.or_trace_closest(osc.handle, rr.ctypes.data, len(idx), far.ctypes.data)
        for k, i in enumerate(idx):
            y, x = ys[i], xs[i]
            rec["BrdfPdf"][y, x, j] = qb[i]
            h = hits[k]
            if far is not None and far[k]["Inst"] != 0xFFFFFFFF and h["Inst"] == 0xFFFFFFFF:
                beyond[y, x, j] = (int(far[k]["Inst"]), int(far[k]["Geom"]), int(far[k]["Prim"])) in lookup
            if h["Inst"] == 0xFFFFFFFF:
                continue
            stopped[y, x, j] = int(h["Inst"])
            li = lookup.get((int(h["Inst"]), int(h["Geom"]), int(h["Prim"])))
            if li is None:
                continue
            U, V = random_from_barycentrics(h["U"], h["V"])
            rec["LightIndex"][y, x, j], rec["U"][y, x, j], rec["V"][y, x, j] = li, U, V
            t_hit[y, x, j] = h["T"]
    return rec, {"t": t_hit, "stopped": stopped, "beyond": beyond}


# ---- the local-light sources' discrete halves, in the device's float32 --------------------------------------------------------------------
def power_cdf(power):
    """the inclusive prefix sum of the powers as k_cdf_local / k_cdf_add form it for up to 1024 lights: four lights per thread summed in
    order, a Hillis-Steele scan of the 256 thread sums, the last entry the total"""
    power = np.asarray(power, np.float32)
    n = len(power)
    assert 0 < n <= 1024
    p = np.zeros(1024, np.float32); p[:n] = power
    v = np.cumsum(p.reshape(256, 4), axis=1, dtype=np.float32)
    part = v[:, 3].copy()
    off = 1
    while off < 256:
        part = (part + np.concatenate([np.zeros(off, np.float32), part[:-off]])).astype(np.float32)
        off <<= 1
    before = np.concatenate([np.zeros(1, np.float32), part[:-1]])
    cdf = (before[:, None] + v).astype(np.float32).reshape(-1)[:n].copy()
    total = f32(f32(0.0) + part[255])
    cdf[n - 1] = total
    return cdf, total


def select_light(cdf, x, total):
    """first light whose inclusive prefix exceeds x (x >= total: the first that reaches the total)"""
    t = x if x < total else total
    lo, hi = 0, len(cdf) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        c = cdf[mid]
        if (c > t) if x < total else (c >= t):
            hi = mid
        else:
            lo = mid + 1
    return lo


# ---- the weights, float64 ---------------------------------------------------------------------------------------------------------------
def sample_terms(S, ys, xs, lights, li, U, V, bsdf):
    """of light samples (li, U, V) at the surfaces S (restirref.Surfaces) of pixels (ys, xs): p-hat, the solid-angle pdf, the all-lobe BSDF
    pdf of the direction, the distance, and the smallest |cosine| the value hinges on (restirref.target_pdfs' margin)"""
    n = len(ys)
    li = np.asarray(li, np.int64)
    ok = (li >= 0) & (li < len(lights))
    lt = lights[np.where(ok, li, 0)]
    b0, b1 = sample_triangle(U, V)
    pos = lt["Base"].astype(np.float64) + lt["Edge0"].astype(np.float64) * b0[:, None] + lt["Edge1"].astype(np.float64) * b1[:, None]
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
    dif, spc, qb = bsdf.evaluate_all(q)[:3]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = ((dif + spc) * lt["Radiance"].astype(np.float64) / pdf[:, None]) @ R.LUMA
    good = ok & (pdf > 0) & np.isfinite(pdf) & np.isfinite(p)
    p = np.where(good, p, 0.0)
    qb = np.where(good, qb, 0.0)
    m = np.minimum(np.minimum(np.abs((S.gn[ys, xs] * dn).sum(-1)), np.abs((S.Ns[ys, xs] * dn).sum(-1))), cosL)
    return p, pdf, qb, ln, np.where(ok, m, np.inf), pos


def blended_pdf(n_l, n_b, q_l, q_b, pdf_sa, dist=None, cutoff=0.0):
    """(N_L q_L + N_B q_B / pdfSA) / N, q_B counting as 0 beyond the cutoff range; N_L q_L / N where pdfSA is not positive and finite.
    Plain arithmetic on whatever number type comes in (float64, or Fractions in the rules test)."""
    n = n_l + n_b
    if not (pdf_sa > 0 and pdf_sa < float("inf")):
        return n_l * q_l / n
    if cutoff > 0 and dist is not None and dist > float(np.sqrt((1.0 / cutoff - 1.0) * float(q_b))):
        q_b = 0 * q_b
    return (n_l * q_l + n_b * q_b / pdf_sa) / n


def stream(weights, coins, targets):
    """RTXDI_StreamSample over candidates in order: returns (selected index or -1, sum of weights, margin of the coins)"""
    wsum, sel, margin = 0 * weights[0] if len(weights) else 0.0, -1, np.inf
    for i, (w, r) in enumerate(zip(weights, coins)):
        wsum = wsum + w
        if w > 0:
            margin = min(margin, R._margin(float(r) * float(wsum), float(w)))
        if r * wsum < w:
            sel = i
    return sel, wsum, margin


def reservoir_weight(wsum, n, p_sel):
    """W = sum w / (N p-hat(y))"""
    return wsum / (n * p_sel)


def initial_sampling(S, lights, records, frame, n_l, n_b, cutoff, source, bsdf):
    """Initial sampling with BRDF candidates over a frame: S restirref.Surfaces (float64), records [H, W, n_b] CANDIDATE (the device's, or
    replay_candidates'), source "cdf" or "uniform". Returns (frame dict of [H, W] arrays: LightIndex (-1 empty), U, V, W, M, TargetPdf;
    margin [H, W])."""
    H, W = S.H, S.W
    N = n_l + n_b
    out = {k: np.zeros((H, W), np.float64 if k in ("U", "V", "W", "TargetPdf") else np.int64) for k in ("LightIndex", "U", "V", "W", "M", "TargetPdf")}
    out["LightIndex"][:] = -1
    margin = np.full((H, W), np.inf)
    ys, xs = np.nonzero(S.valid)
    n = len(ys)
    if n == 0:
        return out, margin
    power = lights["Power"].astype(np.float32)
    cdf, total = power_cdf(power)
    count = len(lights)
    if not (total > 0 and np.isfinite(total)):
        out["M"][ys, xs] = N
        return out, margin
    # candidates, in stream order: n_l light candidates, then n_b BRDF candidates
    li = np.zeros((n, N), np.int64); U = np.zeros((n, N), np.float32); V = np.zeros((n, N), np.float32); coin = np.zeros((n, N), np.float32)
    ql = np.zeros((n, N))
    for i, (y, x) in enumerate(zip(ys, xs)):
        rng = R.Rng(int(x), int(y), frame, R.SALT_INITIAL)
        for k in range(n_l):
            r0, r1, r2, r3 = rng.next(), rng.next(), rng.next(), rng.next()
            if source == "cdf":
                l = select_light(cdf, f32(r0 * total), total)
                ql[i, k] = float(power[l]) / float(total)
            else:
                l = min(int(f32(r0 * f32(count))), count - 1)
                ql[i, k] = 1.0 / count
            li[i, k], U[i, k], V[i, k], coin[i, k] = l, r1, r2, r3
        d = brdf_draws(int(x), int(y), frame, n_b)
        for j in range(n_b):
            c = records[y, x, j]
            l = int(c["LightIndex"])
            li[i, n_l + j] = l if l < count else -1
            U[i, n_l + j], V[i, n_l + j], coin[i, n_l + j] = c["U"], c["V"], d[j, 4]
            if l < count:
                ql[i, n_l + j] = float(power[l]) / float(total) if source == "cdf" else 1.0 / count
    p = np.zeros((n, N)); w = np.zeros((n, N))
    for k in range(N):
        pk, pdf, qb, dist, mk, _ = sample_terms(S, ys, xs, lights, li[:, k], U[:, k], V[:, k], bsdf)
        p[:, k] = pk
        for i in range(n):
            if li[i, k] < 0:
                continue
            margin[ys[i], xs[i]] = min(margin[ys[i], xs[i]], mk[i])
            if not pk[i] > 0:
                continue
            if cutoff > 0 and qb[i] > 0:
                margin[ys[i], xs[i]] = min(margin[ys[i], xs[i]], R._margin(dist[i], float(np.sqrt((1.0 / cutoff - 1.0) * qb[i]))))
            w[i, k] = pk[i] / blended_pdf(n_l, n_b, ql[i, k], qb[i], pdf[i], dist[i], cutoff)
    for i, (y, x) in enumerate(zip(ys, xs)):
        sel, wsum, m = stream(list(w[i]), list(coin[i]), None)
        margin[y, x] = min(margin[y, x], m)
        out["M"][y, x] = N
        if sel >= 0 and p[i, sel] > 0:
            out["LightIndex"][y, x], out["U"][y, x], out["V"][y, x] = li[i, sel], U[i, sel], V[i, sel]
            out["TargetPdf"][y, x] = p[i, sel]
            out["W"][y, x] = reservoir_weight(wsum, N, p[i, sel])
    return out, margin
