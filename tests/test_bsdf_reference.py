"""BSDF sampling and evaluation against the float64 reference tests/bsdfref.py (tolerance model at its top).

The oracle's or_bsdf_sample_batch / or_bsdf_evaluate and the device's pt_bsdf_sample / pt_bsdf_evaluate take the same query
arrays. The CPU tests pin the oracle to bsdfref (directions, lobes, f, pdf), check that every sampled throughput weight is
finite, that the sampled directions follow the pdf and that the weights integrate to the BRDF's albedo, and render a mirror
plane under a constant environment against its closed form. The GPU tests hold the device to the oracle bit for bit.
"""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location("bsdfref", os.path.join(os.path.dirname(__file__), "bsdfref.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

EDGE_ROUGHNESS = (0.0, 2e-3, 5e-3, 0.01, 0.015, 0.02, 1.0)
ONE_MINUS_ULP = float(np.nextafter(np.float32(1), np.float32(0)))


# ---------------------------------------------------------------------------------------------- queries
def unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def frame(n):
    """Two unit tangents perpendicular to each row of n (float64)."""
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([1.0, 0, 0]), np.array([0, 1.0, 0]))
    t = np.cross(n, a); t /= np.linalg.norm(t, axis=1, keepdims=True)
    return t, np.cross(n, t)


def assemble(mat, ng_front, ns, V, rnd, ext=0, front=None):
    """Rows of the 24-word sample query. ng_front is the FrontGeometricNormal; the stored Ng is flipped on back faces."""
    n = len(V)
    q = np.zeros((n, 24), np.float32)
    q[:, 0:7] = mat
    if front is None:
        front = np.ones(n, bool)
    q[:, 7] = front
    q[:, 8:11] = np.where(front[:, None], ng_front, -ng_front)
    q[:, 11:14] = ns; q[:, 14:17] = V; q[:, 17:21] = rnd
    q[:, 21] = np.full(n, ext, np.uint32).view(np.float32)
    return q


def random_materials(rng, n):
    m = np.zeros((n, 7))
    m[:, 0:3] = rng.random((n, 3))
    m[:, 3] = np.where(rng.random(n) < 0.75, rng.choice([0.0, 0.3, 1.0], n), rng.random(n))
    m[:, 4] = np.where(rng.random(n) < 0.3, rng.choice(EDGE_ROUGHNESS, n), rng.random(n))
    m[:, 5] = rng.choice([1.0, 1.5, 1.33, 2.4], n)
    m[:, 6] = np.where(rng.random(n) < 0.75, rng.choice([0.0, 0.6, 1.0], n), rng.random(n))
    return m


def normalized32(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def sample_queries(seed=1):
    """The sampling domain: random queries plus the edge classes of the issue, as one float32 [n, 24] array."""
    rng = np.random.default_rng(seed)
    parts = []
    # random materials, views and normal maps
    n = 20000
    ngf = unit(rng, n)
    ns = np.where(rng.random((n, 1)) < 0.4, ngf, ngf + 0.35 * unit(rng, n))
    V = unit(rng, n); V = np.where((np.sum(V * ngf, 1) < 0)[:, None], -V, V)
    parts.append(assemble(random_materials(rng, n), normalized32(ngf), normalized32(ns), normalized32(V), rng.random((n, 4)),
                          front=rng.random(n) < 0.6))
    # the edge grid: roughness x metallic x transmission x IOR x face, each with random views and numbers
    grid = [(r, mt, tr, ior, fr) for r in EDGE_ROUGHNESS for mt in (0.0, 0.3, 1.0) for tr in (0.0, 0.6, 1.0)
            for ior in (1.0, 1.5) for fr in (0, 1)]
    k = 48
    mat = np.repeat(np.array([(0.9, 0.6, 0.3, mt, r, ior, tr) for r, mt, tr, ior, _ in grid]), k, 0)
    front = np.repeat(np.array([fr for *_, fr in grid], bool), k)
    m = len(mat)
    ngf = unit(rng, m)
    ns = np.where(rng.random((m, 1)) < 0.5, ngf, ngf + 0.2 * unit(rng, m))
    V = unit(rng, m); V = np.where((np.sum(V * ngf, 1) < 0)[:, None], -V, V)
    parts.append(assemble(mat, normalized32(ngf), normalized32(ns), normalized32(V), rng.random((m, 4)), front=front))
    # special views on axis-aligned and tilted normals: NoV -> 0, V = +N, V = -N above a tilted Ng, V below Ns above Ng
    mats = np.array([(0.9, 0.6, 0.3, mt, r, ior, tr) for r in EDGE_ROUGHNESS for mt in (0.0, 1.0) for tr in (0.0, 1.0)
                     for ior in (1.0, 1.5)])
    views = []
    for N in (np.array([0, 0, 1.0]), np.array([0, 0, -1.0]), normalized32([[0.3, -0.5, 0.81]])[0].astype(np.float64)):
        t, _ = frame(N[None])
        t = t[0]
        for c in (1e-6, 1e-4, 1e-2):                             # grazing
            views.append((N, N, np.sqrt(1 - c * c) * t + c * N))
        views.append((N, N, N))                                  # V = N exactly
        tilt = N + 0.6 * t
        views.append((tilt, N, -N))                              # V = -Ns, above the geometric surface
        views.append((tilt, N, normalized32([0.8 * t - 0.15 * N])[0]))   # below Ns, above Ng: the normal-map case
    rnds = [(0.5, 0.3, 0.7, 0.5), (0.0, 0.0, 0.0, 0.0), (ONE_MINUS_ULP,) * 4, (0.99, ONE_MINUS_ULP, 0.0, 0.3),
            (0.2, 0.25, ONE_MINUS_ULP, 0.9), (0.7, 0.75, 0.5, 0.0)]
    rows = []
    for ng, nsv, v in views:
        for mm in mats:
            for rr in rnds:
                for fr in (0, 1):
                    rows.append((mm, ng, nsv, v, rr, fr))
    mat = np.array([r[0] for r in rows]); ng = normalized32([r[1] for r in rows]); nsv = normalized32([r[2] for r in rows])
    v = normalized32([r[3] for r in rows]); rr = np.array([r[4] for r in rows]); fr = np.array([r[5] for r in rows], bool)
    parts.append(assemble(mat, ng, nsv, v, rr, front=fr))
    # the TIR threshold: a smooth glass seen from inside, NoV on a fine grid around the critical cosine sqrt(1 - 1/eta^2)
    crit = math.sqrt(1 - 1 / 1.5 ** 2)
    cs = np.concatenate([crit + np.linspace(-2e-3, 2e-3, 81), crit + np.arange(-40, 41) * 2.0 ** -24])
    m = len(cs) * 4
    c = np.repeat(cs, 4)
    r = np.tile([0.0, 2e-3, 0.01, 0.1], len(cs))
    V = np.stack([np.sqrt(1 - c * c), np.zeros(m), c], 1)
    mat = np.stack([np.full(m, 1.0), np.full(m, 1.0), np.full(m, 1.0), np.zeros(m), r, np.full(m, 1.5), np.ones(m)], 1)
    N = np.tile([0, 0, 1.0], (m, 1))
    parts.append(assemble(mat, N, N, normalized32(V), np.column_stack([np.full(m, 0.5), rng.random((m, 2)), rng.random(m)]),
                          front=np.zeros(m, bool)))
    # Lambertian-only switch (config C1)
    q = parts[0][:2000].copy(); q[:, 21] = np.full(len(q), B.EXT_LAMBERTIAN_ONLY, np.uint32).view(np.float32)
    parts.append(q)
    return np.concatenate(parts)


def on_lobe_boundaries(q, weights):
    """Copies of q with rnd.x on each lobe boundary (as the implementation rounds it) and one ulp either side."""
    w = weights.astype(np.float32)
    outs = []
    for b in (w[:, 2], w[:, 2] + w[:, 1]):
        for d in (-1, 0, 1):
            x = b.astype(np.float32)
            x = x if d == 0 else np.nextafter(x, np.float32(d * np.inf))
            keep = (x > 0) & (x < 1)
            qq = q[keep].copy(); qq[:, 17] = x[keep]
            outs.append(qq)
    return np.concatenate(outs)


def oracle_sample(oracle, q):
    q = np.ascontiguousarray(q, np.float32)
    r = np.zeros((len(q), 12), np.float32)
    oracle.lib().or_bsdf_sample_batch(q.ctypes.data, len(q), r.ctypes.data)
    return r


def oracle_evaluate(oracle, q):
    q = np.ascontiguousarray(q, np.float32)
    r = np.zeros((len(q), 8), np.float32)
    oracle.lib().or_bsdf_evaluate(q.ctypes.data, len(q), r.ctypes.data)
    return r


@pytest.fixture(scope="module")
def domain(oracle):
    q = sample_queries()
    r = oracle_sample(oracle, q)
    q = np.concatenate([q, on_lobe_boundaries(q[:30000], r[:30000, 7:10])])
    return q


def evaluate_queries(seed=2):
    """All-lobe evaluate queries (20 words): the sampling domain's materials and views with random L, plus L on edge cases."""
    rng = np.random.default_rng(seed)
    qs = sample_queries(seed)
    n = len(qs)
    e = np.zeros((n, 20), np.float32)
    e[:, :17] = qs[:, :17]
    ngf = np.where(qs[:, 7:8] != 0, qs[:, 8:11], -qs[:, 8:11]).astype(np.float64)
    L = unit(rng, n)
    pick = rng.random(n)
    # a third above the geometric surface, a third mirror directions about Ns (the D peak), the rest anywhere
    L = np.where((pick < 0.33)[:, None] & (np.sum(L * ngf, 1) < 0)[:, None], -L, L)
    ns, V = qs[:, 11:14].astype(np.float64), qs[:, 14:17].astype(np.float64)
    mirror = 2 * np.sum(ns * V, 1, keepdims=True) * ns - V
    L = np.where((pick > 0.66)[:, None], mirror, L)
    e[:, 17:20] = normalized32(L)
    return e


# ---------------------------------------------------------------------------------------------- checks
def angle(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    c = np.cross(a, b)
    return np.arctan2(np.linalg.norm(c, axis=1), np.sum(a * b, 1))


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


def check_samples(ref, q, r):
    """Sample results r of queries q against the reference. Returns {failure kind: row indices} (empty when all agree)
    and the per-row data the other tests use."""
    fails = {}
    def fail(kind, mask):
        idx = np.flatnonzero(mask)
        if len(idx):
            fails[kind] = idx
    ext = B.ext_bits(q)
    s = ref.initialize(q)
    w = ref.weights(s, ext)
    w_impl = r[:, 7:10].astype(np.float64)
    fail("weights", np.abs(w_impl - w).max(1) > B.REL * np.maximum(np.abs(w), 1e-3).max(1))
    # lobe: the reference's choice, or either side within NEAR of a boundary
    x = q[:, 17].astype(np.float64)
    lobe_impl = r[:, 10].view(np.uint32).astype(np.int64)
    ok_impl = r[:, 11].view(np.uint32) != 0
    lobe_ref = ref.find_lobe(w, x)
    lobe_lo, lobe_hi = ref.find_lobe(w, x - B.NEAR), ref.find_lobe(w, x + B.NEAR)
    near_lobe = (lobe_lo != lobe_ref) | (lobe_hi != lobe_ref)
    fail("lobe", (lobe_impl != lobe_ref) & ~(near_lobe & ((lobe_impl == lobe_lo) | (lobe_impl == lobe_hi))))
    lobe = np.where(near_lobe, lobe_impl, lobe_ref)
    rnd = q[:, 17:21].astype(np.float64)
    L_ref, ok_ref, side = ref.sample_lobe(s, rnd, lobe)
    L_impl = r[:, 0:3].astype(np.float64)
    # Sample's return value, either way where the direction's tolerance reaches the geometric horizon
    tol_angle = B.ANGLE + side["cond"]
    with np.errstate(invalid="ignore"):
        horizon = ~(np.abs(np.sum(s["Ng"] * L_ref, 1)) > B.NEAR + np.sin(np.minimum(tol_angle, 1.6)))
        horizon_impl = np.abs(np.sum(s["Ng"] * L_impl, 1)) <= B.NEAR
    fail("ok", (ok_impl != ok_ref) & ~horizon)
    # the transmission branch: reflect or refract, either near the TIR threshold or the Fresnel coin
    tlobe = lobe == B.TRANSMISSION
    near_branch = tlobe & ((np.abs(side["tir_margin"]) <= B.NEAR) | (np.abs(side["coin_margin"]) <= B.NEAR))
    with np.errstate(invalid="ignore"):
        a = angle(L_impl, L_ref)
        a_other = np.where(side["reflect"], angle(L_impl, side["Lt"]), angle(L_impl, side["Lr"]))
    finite_ref = np.isfinite(L_ref).all(1)
    bad_dir = ok_impl & finite_ref & ~(a <= tol_angle) & ~(near_branch & (a_other <= tol_angle))
    fail("direction", bad_dir)
    fail("rejected_has_value", ~ok_impl & ((r[:, 3] != 0) | (r[:, 4:7] != 0).any(1)))
    # evaluation at the implementation's own L, for the lobe it took
    okm = ok_impl & ~horizon_impl
    with np.errstate(invalid="ignore", divide="ignore"):
        p_all, f_all, NoH, aux = ref.eval_lobes(s, w, np.where(okm[:, None], L_impl, s["Ns"]), ext)
    rows = np.arange(len(q))
    p_ref, f_ref = p_all[rows, lobe], f_all[rows, lobe]
    pdf, f = r[:, 3].astype(np.float64), r[:, 4:7].astype(np.float64)
    ill = (lobe == B.SPECULAR) & (ref.ggx_ulp_sensitivity(s["rough"], NoH) > B.ILL_D)
    cos_min = np.minimum(aux["NoL"], np.where(lobe == B.TRANSMISSION, 1.0, aux["NoV"]))
    # rw = 1 - tw cancels as the transmission weight nears 1: relative error u / rw in the reflection lobes' f and pdf
    rw = 1.0 - w[:, B.TRANSMISSION]
    rw_cond = np.where(lobe == B.TRANSMISSION, 0.0, 2.0 ** -23 / np.maximum(rw, 1e-300))
    tol_pdf = B.REL + B.COS_ULP / np.maximum(cos_min, 1e-30) + np.where(lobe == B.SPECULAR, aux["len2_cond"], 0.0) + rw_cond
    tol = tol_pdf + np.where(lobe == B.SPECULAR, aux["schlick_cond"], 0.0)
    # a finite, non-zero reference: the implementation must be finite there too
    with np.errstate(invalid="ignore"):
        well = okm & ~ill & np.isfinite(p_ref) & np.isfinite(f_ref).all(1)
        fail("pdf", well & ~(rel_err(pdf, p_ref) <= tol_pdf))
        fail("f", well & ~(np.abs(f - f_ref) <= tol[:, None] * np.abs(f_ref) + TINY).all(1))
        live = okm & ill & (f_ref > 0).any(1)
        fail("ill_not_finite_positive", live & ~(np.isfinite(pdf) & (pdf > 0) & np.isfinite(f).all(1) & (f.max(1) > 0)))
        ratio_ref = f_ref / p_ref[:, None]
        ratio = f / pdf[:, None]
        fail("f_over_pdf", live & ~(np.abs(ratio - ratio_ref) <= tol[:, None] * np.abs(ratio_ref)).all(1))
    info = {"ill": ill, "near_lobe": near_lobe, "near_branch": near_branch, "horizon": horizon, "lobe": lobe}
    return fails, info


def close(got, want, tol):
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        return ((got == want) | (np.abs(got - want) <= tol * np.abs(want) + TINY)).all(1)


def check_evaluate(ref, q, r):
    """All-lobe evaluate results r of 20-word queries q against the reference, same tolerance model. Where the specular
    lobe's D is ill-conditioned, its share is compared as f_spec / pdf_spec after taking off the other lobes' reference values."""
    fails = {}
    dif, spc, pdf_ref, s, w, NoH, aux = ref.evaluate_all(q)
    L = q[:, 17:20].astype(np.float64)
    p_l, f_l, _, _ = ref.eval_lobes(s, w, L, 0)
    with np.errstate(invalid="ignore"):
        horizon = np.abs(np.sum(s["Ng"] * L, 1)) <= B.NEAR
    cos_min = np.minimum(aux["NoL"], aux["NoV"])
    tol_pdf = B.REL + B.COS_ULP / np.maximum(cos_min, 1e-30) + aux["len2_cond"]
    tol = (tol_pdf + aux["schlick_cond"])[:, None]
    ill = (ref.ggx_ulp_sensitivity(s["rough"], NoH) > B.ILL_D) & aux["above"] & (w[:, B.TRANSMISSION] < 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        good = ~horizon & np.isfinite(pdf_ref)
        for name, ok in (("pdf", close(r[:, 6:7], pdf_ref[:, None], tol_pdf[:, None]) | ill), ("diffuse", close(r[:, 0:3], dif, tol)),
                         ("specular", close(r[:, 3:6], spc, tol) | ill)):
            if (good & ~ok).any():
                fails[name] = np.flatnonzero(good & ~ok)
        live = good & ill
        bad = live & ~(np.isfinite(r[:, :7]).all(1) & (r[:, :7] >= 0).all(1))
        # the specular lobe's own f / pdf, where it has weight
        ft = np.where((w[:, B.TRANSMISSION] > 0)[:, None], f_l[:, 2], 0.0)
        pt = np.where(w[:, B.TRANSMISSION] > 0, p_l[:, 2], 0.0)
        fs_impl = r[:, 3:6] - ft
        ps_impl = r[:, 6] - pt - p_l[:, 0]
        ratio, ratio_ref = fs_impl / ps_impl[:, None], f_l[:, 1] / p_l[:, 1][:, None]
        slack = (B.REL * (np.abs(ft) + np.abs(pt + p_l[:, 0])[:, None] * np.abs(ratio_ref)) / np.maximum(np.abs(ps_impl), 1e-300)[:, None])
        weighted = live & (w[:, B.SPECULAR] > 0) & (p_l[:, 1] > 0)
        bad |= weighted & ~(np.abs(ratio - ratio_ref) <= tol * np.abs(ratio_ref) + slack + TINY).all(1)
        if bad.any():
            fails["ill_specular_over_pdf"] = np.flatnonzero(bad)
    return fails


TINY = 1e-37                            # below FLT_MIN: an fp32 result may flush where float64 keeps a subnormal


def describe(fails, q, r):
    out = []
    for k, idx in fails.items():
        i = idx[0]
        out.append(f"{k}: {len(idx)} rows, first {i}: q={q[i].tolist()} r={r[i].tolist()}")
    return "\n".join(out)


# ---------------------------------------------------------------------------------------------- CPU tests
def test_oracle_sampling_matches_float64(oracle, domain):
    r = oracle_sample(oracle, domain)
    fails, info = check_samples(B.Reference(), domain, r)
    assert not fails, describe(fails, domain, r)
    # the edge classes were reached: mirror-like samples, both sides of lobe and branch decisions
    assert info["ill"].sum() > 1000 and info["near_lobe"].sum() > 100 and info["near_branch"].sum() > 10


def test_oracle_evaluate_matches_float64(oracle):
    q = evaluate_queries()
    r = oracle_evaluate(oracle, q)
    fails = check_evaluate(B.Reference(), q, r)
    assert not fails, describe(fails, q, r)


def test_sampled_throughput_weights_are_finite(oracle, domain):
    """Raytracing.hlsl:336-346: a sample the path goes on with (ok, pdf > 0, f != 0) must give a finite f * (1/pdf)."""
    r = oracle_sample(oracle, domain)
    ok = r[:, 11].view(np.uint32) != 0
    pdf, f = r[:, 3], r[:, 4:7]
    live = ok & (pdf > 0) & (f != 0).any(1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        thr = f * (np.float32(1) / pdf)[:, None]
    bad = live & ~np.isfinite(thr).all(1)
    assert not bad.any(), f"{bad.sum()} of {live.sum()} live samples have a non-finite weight, e.g. {domain[np.flatnonzero(bad)[0]].tolist()}"
    # and pdf / f themselves never come back NaN or inf from a sample that was taken
    assert np.isfinite(r[ok, 3:7]).all()


def test_throughput_reciprocal_within_two_ulp(oracle, domain):
    """DESIGN "one reciprocal" rule: f * (1/pdf) stays within 2 ulp of the correctly rounded f / pdf."""
    r = oracle_sample(oracle, domain)
    ok = r[:, 11].view(np.uint32) != 0
    live = ok & (r[:, 3] > 0) & (r[:, 4:7] != 0).any(1)
    pdf, f = r[live, 3], r[live, 4:7]
    with np.errstate(over="ignore"):
        fast = f * (np.float32(1) / pdf)[:, None]
        exact = (f.astype(np.float64) / pdf.astype(np.float64)[:, None]).astype(np.float32)
    fin = np.isfinite(exact) & (exact != 0)
    d = np.abs(fast.view(np.int32).astype(np.int64) - exact.view(np.int32).astype(np.int64))
    assert fin.sum() > 0.9 * fin.size
    assert d[fin].max() <= 2, d[fin].max()


# sampling distribution and unbiasedness, opaque materials (the transmission "pdf" NoL * w is not a density by design)
HIST_MATERIALS = [(0.8, 0.8, 0.8, 0.0, 0.5, 1.5, 0.0), (0.9, 0.6, 0.3, 1.0, 0.3, 1.5, 0.0), (0.9, 0.6, 0.3, 1.0, 0.7, 1.5, 0.0),
                  (0.5, 0.7, 0.9, 0.3, 0.4, 1.5, 0.0), (0.8, 0.8, 0.8, 0.0, 1.0, 1.5, 0.0), (0.2, 0.9, 0.4, 0.0, 0.35, 1.0, 0.0)]
HIST_VIEWS = (0.9, 0.35)                 # NoV
N_HIST = 200_000
NB_COS, NB_PHI, SUB = 16, 16, 16
CHI2_Z = 5.0                             # chi-square in Wilson-Hilferty normal form; a pass is z < 5 (p ~ 3e-7)


def hist_case(mat, nov, n, seed):
    rng = np.random.default_rng(seed)
    N = np.array([0.0, 0.0, 1.0])
    V = np.array([math.sqrt(1 - nov * nov), 0.0, nov])
    return assemble(np.array(mat), np.tile(N, (n, 1)), np.tile(N, (n, 1)), np.tile(V, (n, 1)),
                    rng.random((n, 4)).astype(np.float32))


def bin_quadrature(ref, q1, fn):
    """fn(L [m,3]) integrated over each (cos theta, phi) bin of the upper hemisphere about +Z, midpoint rule on SUBxSUB cells."""
    cu = (np.arange(NB_COS * SUB) + 0.5) / (NB_COS * SUB)
    ph = (np.arange(NB_PHI * SUB) + 0.5) / (NB_PHI * SUB) * 2 * np.pi
    C_, P_ = np.meshgrid(cu, ph, indexing="ij")
    S_ = np.sqrt(1 - C_ * C_)
    L = np.stack([S_ * np.cos(P_), S_ * np.sin(P_), C_], -1).reshape(-1, 3)
    val = fn(L).reshape(NB_COS * SUB, NB_PHI * SUB, -1)
    cell = (1.0 / (NB_COS * SUB)) * (2 * np.pi / (NB_PHI * SUB))
    return val.reshape(NB_COS, SUB, NB_PHI, SUB, -1).sum((1, 3)) * cell


def ref_fields(ref, q1, L):
    """All-lobe pdf, and f summed over the lobes Sample can pick (weight > 0): a lobe of weight 0 is never sampled, so its f
    (e.g. the Schlick term of an IOR-1 dielectric, whose lobe weights are {1, 0, 0}) is outside what the estimator sees."""
    qe = np.zeros((len(L), 20))
    qe[:, :17] = q1[:17]
    qe[:, 17:20] = L
    dif, spc, pdf, s, w, _, _ = ref.evaluate_all(qe)
    p, f, _, _ = ref.eval_lobes(s, w, L, 0)
    fs = (f * (w > 0)[:, :, None]).sum(1)
    return np.column_stack([pdf, fs])


@pytest.mark.parametrize("mat", HIST_MATERIALS, ids=lambda m: f"m{m[3]}_r{m[4]}_ior{m[5]}")
def test_sampled_directions_follow_the_pdf(mat, oracle):
    ref = B.Reference()
    for k, nov in enumerate(HIST_VIEWS):
        q = hist_case(mat, nov, N_HIST, seed=100 + k)
        r = oracle_sample(oracle, q)
        ok = r[:, 11].view(np.uint32) != 0
        L = r[ok, 0:3].astype(np.float64)
        ci = np.minimum((L[:, 2] * NB_COS).astype(int), NB_COS - 1)
        pi = np.minimum((np.mod(np.arctan2(L[:, 1], L[:, 0]), 2 * np.pi) / (2 * np.pi) * NB_PHI).astype(int), NB_PHI - 1)
        counts = np.bincount(ci * NB_PHI + pi, minlength=NB_COS * NB_PHI).astype(np.float64)
        quad = bin_quadrature(ref, q[0], lambda LL: ref_fields(ref, q[0].astype(np.float64), LL))
        expected = N_HIST * quad[..., 0].reshape(-1)
        # bins with few expected samples are pooled so that the chi-square approximation holds
        big = expected >= 20
        obs = np.append(counts[big], counts[~big].sum()); exp = np.append(expected[big], expected[~big].sum())
        # the whole upper hemisphere: accepted samples vs the integral of the pdf (the sampler's rejection below Ng)
        assert abs(ok.sum() - expected.sum()) < 5 * math.sqrt(expected.sum()) + 1e-3 * N_HIST, (ok.sum(), expected.sum())
        chi2 = float(((obs - exp) ** 2 / np.maximum(exp, 1e-9)).sum())
        dof = len(obs) - 1
        z = ((chi2 / dof) ** (1 / 3) - (1 - 2 / (9 * dof))) / math.sqrt(2 / (9 * dof))
        assert z < CHI2_Z, (nov, chi2, dof, z)


@pytest.mark.parametrize("mat", HIST_MATERIALS, ids=lambda m: f"m{m[3]}_r{m[4]}_ior{m[5]}")
def test_throughput_weights_are_unbiased(mat, oracle):
    """E[f/pdf], rejected samples counting 0, equals the float64 quadrature of the all-lobe integral of f, to 4 sigma."""
    ref = B.Reference()
    for k, nov in enumerate(HIST_VIEWS):
        q = hist_case(mat, nov, N_HIST, seed=200 + k)
        r = oracle_sample(oracle, q)
        ok = (r[:, 11].view(np.uint32) != 0) & (r[:, 3] > 0)
        wgt = np.where(ok[:, None], r[:, 4:7].astype(np.float64) / np.where(ok, r[:, 3], 1.0)[:, None], 0.0)
        mean, sigma = wgt.mean(0), wgt.std(0) / math.sqrt(N_HIST)
        quad = bin_quadrature(ref, q[0], lambda LL: ref_fields(ref, q[0].astype(np.float64), LL))
        want = quad[..., 1:4].sum((0, 1))
        assert (np.abs(mean - want) <= 4 * sigma + 1e-4 * want).all(), (nov, mean, want, sigma)


@pytest.mark.parametrize("mutation", B.MUTATIONS)
def test_mutated_reference_is_caught(mutation, oracle, domain):
    ref = B.Reference(**{mutation: True})
    r = oracle_sample(oracle, domain)
    fails, _ = check_samples(ref, domain, r)
    q = evaluate_queries()
    fails.update(check_evaluate(ref, q, oracle_evaluate(oracle, q)))
    assert fails, f"mutation {mutation} went unnoticed"


# ---------------------------------------------------------------------------------------------- mirror plane
MIRROR_W, MIRROR_H, MIRROR_SPP = 32, 18, 4
MIRROR_E = (0.8, 1.1, 1.4)
# roughness 0.01 (a = 1e-4) spreads the half vector by ~a about N, which moves Schlick(c, VoH) off Schlick(c, NoV) by a few 1e-4
MIRROR_TOL = {0.0: 1e-4, 2e-3: 1e-4, 0.01: 1e-3}
MIRROR_C = (0.95, 0.64, 0.54)


def mirror_scene(S, roughness):
    mat = S.material(MIRROR_C, metallic=1.0, roughness=roughness)
    quad = S.quad_mesh((-50, 0, -50), (-50, 0, 50), (50, 0, 50), (50, 0, -50), (0, 1, 0), mat)
    cam = S.make_camera((0.0, 1.0, 0.0), forward=(0.0, -0.6, 1.0), hfov_deg=70.0, aspect=MIRROR_W / MIRROR_H)
    sc = S.Scene([S.MeshNode([quad])], [S.RenderObject(0, S.trs())], cam, S.make_scene_data(MIRROR_E + (1.0,)), name="mirror")
    return sc.finalize()


def mirror_closed_form(scene, gb):
    """E * Schlick(c, NoV): a smooth metal reflects the constant environment with the Fresnel factor of its view angle."""
    P = gb["Position"][..., :3].astype(np.float64)
    V = np.asarray(scene.camera["Position"], np.float64) - P
    nov = np.abs(V[..., 1]) / np.linalg.norm(V, axis=-1)
    c = gb["BaseColorMetalness"][..., :3] / 255.0                 # the base colour as the G-buffer's UNORM8 holds it
    F = c + (1 - c) * (1 - nov[..., None]) ** 5
    return np.array(MIRROR_E) * F


@pytest.mark.parametrize("roughness", (0.0, 2e-3, 0.01))
def test_oracle_mirror_plane_closed_form(roughness, oracle, pkg):
    S, L = pkg.scenes, pkg.layouts
    scene = mirror_scene(S, roughness)
    gs = S.graphics_settings(MIRROR_W, MIRROR_H, spp=MIRROR_SPP, bounces=2, russian_roulette=False)
    gb, _, f32 = oracle.render(scene, gs, want_f32=True, layouts=L)
    assert np.isfinite(gb["Position"][..., 3]).all()             # the plane fills the frame
    want = mirror_closed_form(scene, gb)
    got = f32[..., :3].astype(np.float64)
    err = np.abs(got - want) / want
    assert (err <= MIRROR_TOL[roughness]).all(), f"{int((err > MIRROR_TOL[roughness]).any(-1).sum())} of {MIRROR_W * MIRROR_H} pixels off, max rel {err.max():.3g}"


# ---------------------------------------------------------------------------------------------- GPU
def gpu_run(gpu, fn, q, width):
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    dr = torch.zeros((len(q), width), dtype=torch.float32, device="cuda")
    gpu.check(fn(gpu.handle, C.c_void_p(dq.data_ptr()), len(q), C.c_void_p(dr.data_ptr())))
    gpu.sync()
    return dr.cpu().numpy()


def same_bits(a, b):
    """Bit equality, except that any NaN equals any NaN (a rejected sample may carry a NaN direction) and +0 equals -0: where
    V has exact zero components (axis-aligned edge queries), a transmission sample's exactly-zero L components come out with
    the opposite sign of zero on the two compilers; every non-zero word is compared bit for bit."""
    na, nb = np.isnan(a), np.isnan(b)
    a = np.where(na | (a == 0), 0, a).astype(np.float32)
    b = np.where(nb | (b == 0), 0, b).astype(np.float32)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_gpu_bsdf_sample_matches_oracle_and_float64(gpu, oracle, domain):
    got = gpu_run(gpu, gpu.lib.pt_bsdf_sample, domain, 12)
    ref = oracle_sample(oracle, domain)
    assert same_bits(got, ref), f"{int((got != ref).any(1).sum())} rows differ"
    fails, _ = check_samples(B.Reference(), domain, got)
    assert not fails, describe(fails, domain, got)


@pytest.mark.gpu
def test_gpu_bsdf_evaluate_edge_set_matches_oracle(gpu, oracle):
    q = evaluate_queries()
    got = gpu_run(gpu, gpu.lib.pt_bsdf_evaluate, q, 8)
    assert same_bits(got, oracle_evaluate(oracle, q))


@pytest.mark.gpu
def test_gpu_mirror_plane_matches_oracle_and_closed_form(gpu, ptamd, oracle, pkg):
    S, L = pkg.scenes, pkg.layouts
    for roughness in (0.0, 2e-3, 0.01):
        scene = mirror_scene(S, roughness)
        gs = S.graphics_settings(MIRROR_W, MIRROR_H, spp=MIRROR_SPP, bounces=2, russian_roulette=False)
        gpu.set_sharding(0, 1, 16)
        g = ptamd.Scene(gpu, scene)
        rr = ptamd.Renderer(gpu, g, MIRROR_W, MIRROR_H, with_f32=True)
        rr.render(gs)
        gpu.sync()
        out = ptamd.textures_to_numpy(rr.textures)
        gb, _, f32 = oracle.render(scene, gs, want_f32=True, layouts=L)
        assert np.array_equal(out["RadianceF32"].view(np.uint32), f32.view(np.uint32)), roughness
        assert np.array_equal(out["Radiance"], gb["Radiance"]), roughness
        want = mirror_closed_form(scene, gb)
        assert (np.abs(out["RadianceF32"][..., :3] - want) <= MIRROR_TOL[roughness] * want).all(), roughness
