"""What "a ray hits a triangle" means, stated without the fp32 recipe of csrc/pt_trace.hpp tri_test / oracle/pt_oracle.c tri_test
(numpy + fractions only), and that recipe restated in numpy float32 beside it so that wrong variants of it can be held against the same
assertions. The geometry (edge values, det, margins, cond, u, v, t) shares nothing with the recipe; the error model that says how far the
recipe may be from it (rho, below) is by design taken along the recipe's own axes.

The kernels and the oracle are the same Woop/Benthin/Wald arithmetic written twice: a mistake in the rule itself (dominant axis, the fp64
edge fallback, the det == 0 reject, the dropped kx/ky swap) is shared by both. Here the rule is geometry:

  A = v0 - o, B = v1 - o, C = v2 - o                      (exact differences of the fp32 inputs)
  U = d . (B x C),  V = d . (C x A),  W = d . (A x B)     signed edge values: scalar triple products, six products of three factors each
  det = U + V + W
  hit    <=>  no two of U, V, W have strictly opposite signs, and det != 0     (a zero counts with either side: edges and vertices belong
                                                                               to every triangle that shares them; no face is culled)
  u = V / det,  v = W / det                               u weights v1, v weights v2
  t = (d . P) / (d . d),  P = (U A + V B + W C) / det     the hit point relative to o; a hit counts for t in (tmin, tmax), both exclusive

`edge_values` evaluates this vectorised in float64 and again in exact rationals wherever float64 cannot decide a sign: the float64 value
of a triple product is off by at most 16 * 2^-53 times the sum m of the absolute values of its six terms (one rounding of each
difference v - o, two multiplications per term, five additions: nine roundings on the longest path, 16 for headroom), so a value beyond
that is decided and anything else goes to fractions.Fraction. The inputs are fp32, so this is rare (aimed rays, mostly). det is
evaluated as d . ((v1 - v0) x (v2 - v0)), the same number without the cancellation of a far origin, and decided the same way.

Per edge value:   margin = |value| / m       m = sum of the absolute values of its six product terms (mU, mV, mW)
Per pair:         cond   = (mU + mV + mW) / |det|

Accuracy of the fp32 rule, derived from its operations (eps = 2^-24, first order; kx, ky, kz = the rule's axes, s = d[kx] / d[kz]):
  subtraction of o            A^ = A (1 + eps)                                       1 rounding per component
  S: one division, two mult.  Sz^ = (1 / d[kz]) (1 + eps), Sx^ = s (1 + 2 eps)       2 roundings on Sx, Sy
  the shear                   Bx^ = fl(B^[kx] - fl(Sx^ B^[kz])) = B[kx] (1 + 2 eps) - s B[kz] (1 + 5 eps)
                              (B[kx]: subtraction of o, final subtraction; s B[kz]: subtraction of o, two of S, product, final subtraction)
  two-product difference      U^ = fl(fl(Cx^ By^) - fl(Cy^ Bx^)). Expanded, Cx By - Cy Bx has eight terms: the six terms of the triple product
                              divided by d[kz] -- two without s (2 + 2 + 1 + 1 = 6 roundings each), four with one s (2 + 5 + 1 + 1 = 9) --
                              and the pair +- sx sy B[kz] C[kz] (5 + 5 + 1 + 1 = 12) that cancels exactly but whose ROUNDINGS do not. Hence
                                  |U^ d[kz] - U| <= eps (9 mU + 12 * 2 X),   X = |d[kx] d[ky] B[kz] C[kz] / d[kz]|
                                                 <= K_EDGE eps rho mU,       K_EDGE = 12,  rho = (mU + 2 X) / mU >= 1.
                              rho is the price of the shear: the six-term sum m alone does not bound the rule's error (o = 0, d = (1, 1, 1),
                              B = C = (0, 0, 1): m = 0, yet the rule subtracts 1 * 1 from 1 * 1). For a ray aimed at its triangle X is about
                              one of the six terms (rho ~ 4/3); `edge_values` returns it per edge. The fallback (taken when a U^, V^ or W^ is
                              exactly 0) forms the same products exactly and rounds the difference once from float64: fewer roundings, same bound.
  So the rule's sign of an edge value is the exact one wherever margin >= K_EDGE * rho * eps, and `classify` calls a pair undecided(k)
  when a margin is below k * rho * 2^-24. With every margin decided the three signs are exact, a sum of three values of one sign cannot
  cancel, and the hit decision is the exact one.
  sum and reciprocal          det^ = fl(fl(U^ + V^) + W^): the three edge errors plus two roundings of at most |U| + |V| + |W| <= M = mU + mV + mW:
                                  |det^ - det| / |det| <= (12 rho + 2) eps cond      (rho: the largest of the three)
                              rcp = fl(1 / det^), u^ = fl(V^ rcp): two more roundings.
                                  |u^ - u| <= 12 rho eps mV / |det| + |u| ((12 rho + 2) cond + 2) eps <= (K_UV_RHO rho + K_UV_ONE) eps cond
                                  for |u| <= 1 and cond >= 1:  K_UV_RHO = 24, K_UV_ONE = 4   (+ 2^-10 relative for the second order)
  t                           The rule's t is P[kz] / d[kz]: T^ = fl(fl(fl(U^ Az^) + fl(V^ Bz^)) + fl(W^ Cz^)) with Az^ = fl(Sz^ A^[kz]) (3 roundings).
                              Each product carries its edge error times |Az| plus 4 roundings, the two additions 2 more; with
                              r = max_j |v_j - o|_inf / (|d|_inf |t|) >= max |Az| / |t| (how much deeper than the hit the vertices lie):
                                  |t^ - t| / |t| <= ((12 rho + 6) r + 12 rho + 4) eps cond  = (K_T_R(rho) r + K_T_ONE(rho)) eps cond
  The constants of u, v and t (28 and 38 at rho = r = 1) are far above 16, and far above what is seen (about 1.1 and 2.5 eps cond on the
  oracle): they add the worst case of every one of some thirty roundings with the same sign, and charge all of M to each edge, where a
  real pair spreads them over three edges with errors that mostly cancel. They are bounds, not estimates; the wrong rules of
  `WRONG_RULES` still break them (tests/test_intersection_reference.py).
  The float64 reference's own error in u, v, t is 16 * 2^-53 cond: 2^-25 of these bounds.

`woop_fp32` is the kernel's rule in numpy float32 (numpy does not contract; the fallback in float64), without the paper's kx/ky swap as
in pt_trace.hpp; it must equal the oracle's or_ray_triangle bit for bit. `paper_swap` puts the swap back: the hit decision, t and every
non-zero u, v must not change in a bit, and a u or v that is exactly zero may change its sign only (which is what the comment in
pt_trace.hpp claims, and what the oracle -- which used to keep the swap -- showed: -0 against +0 on rays through an edge). Its `wrong` switch selects one of
WRONG_RULES; `woop_closest` runs it over instances of a triangle soup with the project's closest-hit rule and carries the two wrong rules
that live there (an inclusive tmin, ties to the last triangle).

`to_object_space` is the project's fp32 rule for taking a ray into an instance (pt_math.hpp sop3 / sop3t: a chain of fused multiply-adds),
each fma evaluated in float64 and rounded once to fp32 with the tie case repaired, which is exact.
"""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -24
K_EDGE = 12.0
K_UV_RHO, K_UV_ONE = 24.0, 4.0
SECOND_ORDER = 1.0 + 2.0 ** -10
F64_DECIDES = 16.0 * 2.0 ** -53
OUTSIDE, INSIDE, UNDECIDED = 0, 1, 2
WRONG_RULES = ("no_fallback", "fma_edges", "fixed_kz", "accept_det0", "swap_uv", "cull_back", "inclusive_tmin", "last_tie")

f32, f64 = np.float32, np.float64


def k_t(rho, r):
    """the derived constant of |t^ - t| / |t| in units of eps * cond"""
    return (12.0 * rho + 6.0) * r + 12.0 * rho + 4.0


# ----------------------------------------------------------------------------------------------
# exact geometry
# ----------------------------------------------------------------------------------------------
def _triple(d, P, Q):
    """d . (P x Q) and the sum of the absolute values of its six terms"""
    terms = (d[..., 0] * P[..., 1] * Q[..., 2], -d[..., 0] * P[..., 2] * Q[..., 1], d[..., 1] * P[..., 2] * Q[..., 0],
             -d[..., 1] * P[..., 0] * Q[..., 2], d[..., 2] * P[..., 0] * Q[..., 1], -d[..., 2] * P[..., 1] * Q[..., 0])
    val = ((terms[0] + terms[1]) + (terms[2] + terms[3])) + (terms[4] + terms[5])
    return val, sum(np.abs(x) for x in terms)


def _fraction_row(o, d, v):
    """exact U, V, W, det, u, v, t of one pair (fp32 inputs as Fractions)"""
    F = Fraction
    o = [F(float(x)) for x in o]; d = [F(float(x)) for x in d]
    P = [[F(float(x)) - o[k] for k, x in enumerate(p)] for p in v]

    def triple(p, q):
        return (d[0] * (p[1] * q[2] - p[2] * q[1]) + d[1] * (p[2] * q[0] - p[0] * q[2]) + d[2] * (p[0] * q[1] - p[1] * q[0]))
    U, V, W = triple(P[1], P[2]), triple(P[2], P[0]), triple(P[0], P[1])
    det = U + V + W
    if det == 0:
        return U, V, W, det, None, None, None
    hit = [(U * P[0][k] + V * P[1][k] + W * P[2][k]) / det for k in range(3)]
    dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    t = (d[0] * hit[0] + d[1] * hit[1] + d[2] * hit[2]) / dd
    return U, V, W, det, V / det, W / det, t


def edge_values(o, d, v0, v1, v2):
    """Arrays [..., 3] of fp32 values (broadcast against each other). Returns a dict of float64 arrays: U, V, W, det with exact signs,
    mU, mV, mW, rhoU, rhoV, rhoW, marginU, marginV, marginW, cond, u, v, t, r (the depth ratio of the t bound) and `exact` (rows that
    went through rationals)."""
    o, d, v0, v1, v2 = np.broadcast_arrays(*(np.asarray(x, f32) for x in (o, d, v0, v1, v2)))
    shape = o.shape[:-1]
    o, d, v0, v1, v2 = (x.reshape(-1, 3).astype(f64) for x in (o, d, v0, v1, v2))
    A, B, C = v0 - o, v1 - o, v2 - o
    U, mU = _triple(d, B, C); V, mV = _triple(d, C, A); W, mW = _triple(d, A, B)
    # det = U + V + W = d . ((v1 - v0) x (v2 - v0)): the same number, taken from the edges because the sum of three triple products about
    # a far origin cancels where this does not (a 1e-3 sliver seen from 1e4 away)
    det, mdet = _triple(d, v1 - v0, v2 - v0)
    M = mU + mV + mW
    doubt = (np.abs(U) <= F64_DECIDES * mU) | (np.abs(V) <= F64_DECIDES * mV) | (np.abs(W) <= F64_DECIDES * mW) | (np.abs(det) <= F64_DECIDES * mdet)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = V / det, W / det
        Pt = (U[:, None] * A + V[:, None] * B + W[:, None] * C) / det[:, None]
        t = (d * Pt).sum(-1) / (d * d).sum(-1)
    for i in np.nonzero(doubt)[0]:
        fU, fV, fW, fdet, fu, fv, ft = _fraction_row(o[i], d[i], (v0[i], v1[i], v2[i]))
        U[i], V[i], W[i], det[i] = float(fU), float(fV), float(fW), float(fdet)
        for arr, x in ((U, fU), (V, fV), (W, fW), (det, fdet)):                                  # a float() that underflowed keeps its sign
            if x != 0 and arr[i] == 0.0:
                arr[i] = np.copysign(5e-324, 1.0 if x > 0 else -1.0)
        u[i], v[i], t[i] = (float(fu), float(fv), float(ft)) if fdet != 0 else (np.nan, np.nan, np.nan)
    # rho is the error model of the RULE (module docstring), so it is taken along the rule's axes: the one place where the reference looks
    # at the recipe. U, V, W, det, the margins, cond, u, v, t above do not depend on it.
    kz = _dominant(d)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    pick = lambda a, k: np.take_along_axis(a, k[:, None], -1)[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        sxy = np.abs(pick(d, kx) * pick(d, ky) / pick(d, kz))
        out = {"U": U, "V": V, "W": W, "det": det, "mU": mU, "mV": mV, "mW": mW, "u": u, "v": v, "t": t, "exact": doubt}
        for name, m, (P, Q), val in (("U", mU, (B, C), U), ("V", mV, (C, A), V), ("W", mW, (A, B), W)):
            X = sxy * np.abs(pick(P, kz) * pick(Q, kz))
            out["rho" + name] = np.where(m > 0, (m + 2.0 * X) / m, np.inf)
            out["margin" + name] = np.where(m > 0, np.abs(val) / m, 0.0)
        out["cond"] = np.where(det != 0, M / np.abs(det), np.inf)
        depth = np.maximum(np.maximum(np.abs(A).max(-1), np.abs(B).max(-1)), np.abs(C).max(-1)) / np.abs(d).max(-1)
        out["r"] = np.where(t != 0, depth / np.abs(t), np.inf)
    return {k: a.reshape(shape) for k, a in out.items()}


def exact_hit(ev):
    """the hit decision of the definition above, on exact signs"""
    U, V, W = ev["U"], ev["V"], ev["W"]
    mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
    return ~mixed & (ev["det"] != 0)


def classify(ev, k=K_EDGE):
    """INSIDE / OUTSIDE by the exact signs; UNDECIDED where a margin is below k * rho * 2^-24. rho >= 1 is by design computed along the fp32
    rule's own axes (_dominant): it is that rule's error model, without which no multiple of 2^-24 of the six-term sum bounds its error (module
    docstring). The exact signs themselves share nothing with the rule."""
    und = np.zeros(ev["U"].shape, bool)
    for n in "UVW":
        und |= ~(ev["margin" + n] >= k * ev["rho" + n] * EPS)
    return np.where(und, UNDECIDED, np.where(exact_hit(ev), INSIDE, OUTSIDE))


def bounds(ev):
    """(bound on |u^ - u| and |v^ - v|, bound on |t^ - t| / |t|) of the fp32 rule for every pair, from the derived constants"""
    rho = np.maximum(np.maximum(ev["rhoU"], ev["rhoV"]), ev["rhoW"])
    with np.errstate(invalid="ignore", over="ignore"):
        uv = (K_UV_RHO * rho + K_UV_ONE) * EPS * ev["cond"] * SECOND_ORDER
        tt = k_t(rho, ev["r"]) * EPS * ev["cond"] * SECOND_ORDER
    return uv, tt


def check_pairs(ev, hit, t, u, v, what):
    """The assertions on a rule's answers for pairs: hit [n] bool, t, u, v [n] (read where hit). Classification equals the exact one wherever
    every margin is decided; u, v, t of decided hits are within the derived bounds. Returns the observed figures (worst margin at which the
    rule disagreed with the exact classification, in units of 2^-24; worst errors in units of 2^-24 * cond)."""
    cls = classify(ev)
    decided = cls != UNDECIDED
    want = cls == INSIDE
    bad = decided & (hit != want)
    assert not bad.any(), f"{what}: classification differs from the exact one on {int(bad.sum())} decided pairs, first {int(np.nonzero(bad)[0][0])}"
    low = np.minimum(np.minimum(ev["marginU"], ev["marginV"]), ev["marginW"])
    wrong = hit != exact_hit(ev)
    ok = decided & want & hit
    uvb, tb = bounds(ev)
    with np.errstate(invalid="ignore", divide="ignore"):
        eu = np.abs(u.astype(f64) - ev["u"]); evv = np.abs(v.astype(f64) - ev["v"])
        et = np.abs(t.astype(f64) - ev["t"]) / np.abs(ev["t"])
    for name, e, b in (("u", eu, uvb), ("v", evv, uvb), ("t", et, tb)):
        over = ok & ~(e <= b)
        assert not over.any(), (f"{what}: {name} outside the derived bound on {int(over.sum())} hits, first {int(np.nonzero(over)[0][0])}: "
                                f"error {e[over][0]:.3e} against {b[over][0]:.3e}")
    unit = EPS * ev["cond"]
    with np.errstate(invalid="ignore", divide="ignore"):
        fig = {"worst_disagreeing_margin": float((low[wrong] / EPS).max()) if wrong.any() else 0.0,
               "disagreements": int(wrong.sum()),
               "u": float((eu[ok] / unit[ok]).max()) if ok.any() else 0.0, "v": float((evv[ok] / unit[ok]).max()) if ok.any() else 0.0,
               "t": float((et[ok] / unit[ok]).max()) if ok.any() else 0.0,
               "undecided_share": float((~decided).mean()), "decided_hits": int(ok.sum())}
    return fig


# ----------------------------------------------------------------------------------------------
# the project's fp32 ray transform
# ----------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a * b + c) for fp32 arrays: the product is exact in float64; the sum is rounded to float64 with its error known (TwoSum), and
    where that sum sits exactly halfway between two fp32 values the error decides the direction, as one rounding would."""
    p = a.astype(f64) * b.astype(f64); c = c.astype(f64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(f32)
    back = s - r.astype(f64)
    with np.errstate(over="ignore", invalid="ignore"):
        other = np.nextafter(r, np.where(back > 0, f32(np.inf), f32(-np.inf))).astype(f64)
        tie = (back != 0) & (e != 0) & np.isfinite(other) & ((other - s) == back)
    s = np.where(tie, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def to_object_space(w2o, o, d):
    """transform_ray of pt_trace.hpp: rows of the 3x4 worldToObject (12 fp32, row-major) applied by sop3t (origin) and sop3 (direction)"""
    W = np.asarray(w2o, f32).reshape(3, 4)
    o = np.asarray(o, f32); d = np.asarray(d, f32)
    ro = np.stack([fma32(W[k, 2], o[..., 2], fma32(W[k, 1], o[..., 1], fma32(W[k, 0], o[..., 0], np.broadcast_to(W[k, 3], o[..., 0].shape)))) for k in range(3)], -1)
    rd = np.stack([fma32(W[k, 2], d[..., 2], fma32(W[k, 1], d[..., 1], (W[k, 0] * d[..., 0]).astype(f32))) for k in range(3)], -1)
    return ro, rd


# ----------------------------------------------------------------------------------------------
# the fp32 rule, and wrong variants of it
# ----------------------------------------------------------------------------------------------
def _dominant(d):
    """the rule's kz: x, unless |dy| > |dx|, then z if |dz| exceeds both (ties keep the earlier axis). Part of the fp32 recipe, not of
    the geometry: besides woop_fp32 only the error model (rho in edge_values) uses it."""
    a = np.abs(d)
    kz = np.where(a[..., 1] > a[..., 0], 1, 0)
    kz = np.where(a[..., 2] > np.take_along_axis(a, kz[..., None], -1)[..., 0], 2, kz)
    return kz


def woop_fp32(o, d, v0, v1, v2, wrong=None, paper_swap=False):
    """tri_test of pt_trace.hpp on fp32 arrays [n, 3]: (hit, t, u, v, fallback taken). wrong: one of WRONG_RULES (the two closest-hit ones
    change nothing here). paper_swap: exchange kx and ky where d[kz] < 0, as the paper does and the kernels do not."""
    o, d, v0, v1, v2 = np.broadcast_arrays(*(np.asarray(x, f32) for x in (o, d, v0, v1, v2)))
    o, d, v0, v1, v2 = (np.ascontiguousarray(x.reshape(-1, 3)) for x in (o, d, v0, v1, v2))
    kz = np.full(len(d), 2) if wrong == "fixed_kz" else _dominant(d)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    pick = lambda a, k: np.take_along_axis(a, k[:, None], -1)[:, 0]
    if paper_swap:
        flip = pick(d, kz) < 0
        kx, ky = np.where(flip, ky, kx), np.where(flip, kx, ky)
    with np.errstate(all="ignore"):
        Sz = (f32(1.0) / pick(d, kz)).astype(f32)
        Sx = pick(d, kx) * Sz; Sy = pick(d, ky) * Sz
        A, B, C = v0 - o, v1 - o, v2 - o
        Akz, Bkz, Ckz = pick(A, kz), pick(B, kz), pick(C, kz)
        Ax = pick(A, kx) - Sx * Akz; Ay = pick(A, ky) - Sy * Akz
        Bx = pick(B, kx) - Sx * Bkz; By = pick(B, ky) - Sy * Bkz
        Cx = pick(C, kx) - Sx * Ckz; Cy = pick(C, ky) - Sy * Ckz
        if wrong == "fma_edges":                              # what a contracting compiler makes of x * y - z * w
            neg = lambda x: (-x).astype(f32)
            U = fma32(Cx, By, neg(Cy * Bx)); V = fma32(Ax, Cy, neg(Ay * Cx)); W = fma32(Bx, Ay, neg(By * Ax))
        else:
            U = Cx * By - Cy * Bx; V = Ax * Cy - Ay * Cx; W = Bx * Ay - By * Ax
        fb = (U == 0) | (V == 0) | (W == 0)
        if wrong == "no_fallback":
            fb = np.zeros(len(U), bool)
        D = lambda x: x.astype(f64)
        U = np.where(fb, (D(Cx) * D(By) - D(Cy) * D(Bx)).astype(f32), U)
        V = np.where(fb, (D(Ax) * D(Cy) - D(Ay) * D(Cx)).astype(f32), V)
        W = np.where(fb, (D(Bx) * D(Ay) - D(By) * D(Ax)).astype(f32), W)
        neg_any, pos_any = (U < 0) | (V < 0) | (W < 0), (U > 0) | (V > 0) | (W > 0)
        hit = ~(neg_any & pos_any)
        det = (U + V) + W
        if wrong != "accept_det0":
            hit &= det != 0
        if wrong == "cull_back":                              # keeps one winding: the rule's det against the sign of d[kz]
            hit &= (det * pick(d, kz)) > 0
        Az, Bz, Cz = Sz * Akz, Sz * Bkz, Sz * Ckz
        T = (U * Az + V * Bz) + W * Cz
        rcp = (f32(1.0) / det).astype(f32)
        t, u, v = T * rcp, V * rcp, W * rcp
        if wrong == "swap_uv":
            u, v = v, u
    return hit, t.astype(f32), u.astype(f32), v.astype(f32), fb


def _miss_records(rays):
    rec = np.zeros(len(rays), RECORD)
    rec["T"] = rays[:, 7]; rec["Instance"] = 0xFFFFFFFF
    return rec


def _record_dtype():
    import __graft_entry__ as ge
    ge.load_package()
    from dxpbrt_amd.ptamd import CLOSEST_HIT
    return CLOSEST_HIT


RECORD = _record_dtype()                                        # PtClosestHit as the binding lays it out


def woop_closest(rays, instances, wrong=None, chunk=1 << 18):
    """trace_brute_force of pt_trace.hpp over `instances` = [(worldToObject [12] fp32, tris [n, 3, 3] fp32, geom [n], prim [n])] for rays
    [m, 8] (origin, tmin, direction, tmax): PtClosestHit records, t in (tmin, tmax), ties to the lowest (instance, geometry, primitive).
    Slot is the triangle's position in its instance's list."""
    rays = np.asarray(rays, f32).reshape(-1, 8)
    rec = _miss_records(rays)
    found = np.zeros(len(rays), bool)
    tmin, tmax = rays[:, 3], rays[:, 7]
    for x, (w2o, tris, geom, prim) in enumerate(instances):
        tris = np.asarray(tris, f32)
        if not len(tris):
            continue
        ro, rd = to_object_space(w2o, rays[:, 0:3], rays[:, 4:7])
        step = max(1, chunk // len(tris))
        for r0 in range(0, len(rays), step):
            sl = slice(r0, r0 + step)
            n = len(ro[sl])
            hit, t, u, v, _ = woop_fp32(ro[sl][:, None, :], rd[sl][:, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2], wrong)
            hit, t, u, v = (a.reshape(n, len(tris)) for a in (hit, t, u, v))
            with np.errstate(invalid="ignore"):
                ok = hit & ((t >= tmin[sl, None]) if wrong == "inclusive_tmin" else (t > tmin[sl, None])) & (t < tmax[sl, None])
            tt = np.where(ok, t, np.inf)
            best = tt.min(1)
            # ties: the lowest (geometry, primitive) among the triangles at the best t (the last one under the wrong rule)
            key = geom.astype(np.int64) * (1 << 32) + prim.astype(np.int64)
            at = ok & (tt == best[:, None])
            keyed = np.where(at, key[None, :], -1 if wrong == "last_tie" else np.iinfo(np.int64).max)
            j = keyed.argmax(1) if wrong == "last_tie" else keyed.argmin(1)
            has = ok.any(1)
            cur = rec["T"][sl]
            better = has & ((best <= cur) if wrong == "last_tie" else (best < cur))      # instances come in ascending order
            idx = np.nonzero(better)[0]
            g = r0 + idx
            rec["T"][g] = best[idx]; rec["U"][g] = u[idx, j[idx]]; rec["V"][g] = v[idx, j[idx]]
            rec["Instance"][g] = x; rec["Geometry"][g] = geom[j[idx]]; rec["Primitive"][g] = prim[j[idx]]; rec["Slot"][g] = j[idx]
            found[g] = True
    return rec


# ----------------------------------------------------------------------------------------------
# the exact closest hit of a soup
# ----------------------------------------------------------------------------------------------
def closest(rays, instances, chunk=1 << 16):
    """For rays [m, 8] over `instances` (as woop_closest): per ray the exact t of the nearest triangle that is INSIDE by margin and whose t
    lies in (tmin, tmax) by more than its t bound -- `t_sure` (inf: none), with that bound as an absolute value `e_sure` and its
    (instance, slot) -- and the counts of INSIDE / UNDECIDED pairs. The ray enters every instance by the project's fp32 rule
    (to_object_space); everything after that is exact."""
    rays = np.asarray(rays, f32).reshape(-1, 8)
    m = len(rays)
    out = {"t_sure": np.full(m, np.inf), "e_sure": np.zeros(m), "inst": np.full(m, -1), "slot": np.full(m, -1),
           "inside": np.zeros(m, np.int64), "undecided": np.zeros(m, np.int64)}
    tmin, tmax = rays[:, 3].astype(f64), rays[:, 7].astype(f64)
    for x, (w2o, tris, geom, prim) in enumerate(instances):
        tris = np.asarray(tris, f32)
        if not len(tris):
            continue
        ro, rd = to_object_space(w2o, rays[:, 0:3], rays[:, 4:7])
        step = max(1, chunk // len(tris))
        for r0 in range(0, m, step):
            sl = slice(r0, r0 + step)
            ev = edge_values(ro[sl][:, None, :], rd[sl][:, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
            cls = classify(ev)
            _, tb = bounds(ev)
            with np.errstate(invalid="ignore"):
                e = tb * np.abs(ev["t"])
                sure = (cls == INSIDE) & (ev["t"] - e > tmin[sl, None]) & (ev["t"] + e < tmax[sl, None])
            out["inside"][sl] += (cls == INSIDE).sum(1); out["undecided"][sl] += (cls == UNDECIDED).sum(1)
            tt = np.where(sure, ev["t"], np.inf)
            j = tt.argmin(1); best = tt[np.arange(len(j)), j]
            better = best < out["t_sure"][sl]
            g = r0 + np.nonzero(better)[0]
            out["t_sure"][g] = best[better]; out["e_sure"][g] = e[np.arange(len(j)), j][better]
            out["inst"][g] = x; out["slot"][g] = j[better]
    return out


def check_closest(rays, instances, rec, slot_of, what, all_pairs=True, candidates=None):
    """The closest-of-many assertions on PtClosestHit records `rec` of a rule: the chosen triangle is exactly inside or undecided and,
    where inside by margin, carries u, v, t within the bounds; no triangle that is inside by margin (with t inside the interval by more than
    its bound) has an exact t smaller than the chosen one's by more than the two t bounds -- and a miss has no such triangle at all.
    slot_of(instance, geometry, primitive) -> position of that triangle in instances[instance]'s list (arrays in, array out).
    all_pairs = False: "no such triangle" is asked of one triangle per ray only, slot candidates[ray] of instance 0 (sets too large for
    every ray against every triangle)."""
    rays = np.asarray(rays, f32).reshape(-1, 8)
    if all_pairs:
        ref = closest(rays, instances)
    else:
        w2o, tris, geom, prim = instances[0]
        tris = np.asarray(tris, f32)[np.asarray(candidates)]
        ro, rd = to_object_space(w2o, rays[:, 0:3], rays[:, 4:7])
        ev = edge_values(ro, rd, tris[:, 0], tris[:, 1], tris[:, 2])
        _, tb = bounds(ev)
        with np.errstate(invalid="ignore"):
            e = tb * np.abs(ev["t"])
            sure = (classify(ev) == INSIDE) & (ev["t"] - e > rays[:, 3]) & (ev["t"] + e < rays[:, 7])
        ref = {"t_sure": np.where(sure, ev["t"], np.inf), "e_sure": np.where(sure, e, 0.0)}
    hit = rec["Instance"] != 0xFFFFFFFF
    missed = ~hit & np.isfinite(ref["t_sure"])
    assert not missed.any(), f"{what}: {int(missed.sum())} rays miss a triangle that is inside by margin, first ray {int(np.nonzero(missed)[0][0])}"
    fig = {"rays": len(rays), "hits": int(hit.sum()), "u": 0.0, "v": 0.0, "t": 0.0}
    if all_pairs:                                               # of all (ray, triangle) pairs, and of the pairs that are inside or undecided
        und, ins = int(ref["undecided"].sum()), int(ref["inside"].sum())
        fig["undecided_pairs"] = und
        fig["undecided_share"] = und / max(1, len(rays) * sum(len(x[1]) for x in instances))
        fig["undecided_share_of_candidates"] = und / max(1, und + ins)
    e_chosen = np.zeros(len(rays)); t_chosen = np.full(len(rays), np.inf)
    for x in np.unique(rec["Instance"][hit]):
        sel = np.nonzero(hit & (rec["Instance"] == x))[0]
        w2o, tris, geom, prim = instances[int(x)]
        tris = np.asarray(tris, f32)
        s = slot_of(int(x), rec["Geometry"][sel], rec["Primitive"][sel])
        ro, rd = to_object_space(w2o, rays[sel, 0:3], rays[sel, 4:7])
        ev = edge_values(ro, rd, tris[s, 0], tris[s, 1], tris[s, 2])
        cls = classify(ev)
        out = cls == OUTSIDE
        assert not out.any(), f"{what}: {int(out.sum())} rays report a triangle that is exactly outside, first ray {int(sel[np.nonzero(out)[0][0]])}"
        f = check_pairs(ev, np.ones(len(sel), bool), rec["T"][sel], rec["U"][sel], rec["V"][sel], what)
        for k in "uvt":
            fig[k] = max(fig[k], f[k])
        _, tb = bounds(ev)
        with np.errstate(invalid="ignore"):
            e_chosen[sel] = np.where(cls == INSIDE, tb * np.abs(ev["t"]), np.inf)
        t_chosen[sel] = np.where(cls == INSIDE, ev["t"], -np.inf)
    with np.errstate(invalid="ignore"):
        late = hit & (ref["t_sure"] < t_chosen - (e_chosen + ref["e_sure"]))
    assert not late.any(), f"{what}: {int(late.sum())} rays report a hit behind a triangle that is inside by margin, first ray {int(np.nonzero(late)[0][0])}"
    return fig
