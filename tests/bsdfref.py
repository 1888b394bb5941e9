"""Float64 reference of the BSDF: BSDFSample's Initialize, lobe weights, lobe choice, sampling and evaluation (numpy only).

Restated from Shaders/BxDF.hlsli and the published algorithms behind the MathLib functions it calls, independently of
csrc/pt_math.hpp and oracle/pt_oracle.c, so that a mistake the GPU code and the oracle share does not pass unseen:

  Initialize, EstimateDiffuseProbability   BxDF.hlsli:45-67, :21-34 (clamp to [0.05, 0.95] only strictly inside (0, 1))
  ComputeLobeWeights, FindLobe, Sample     BxDF.hlsli:184-226 (FindLobe walks transmission, specular, diffuse on rnd.x)
  ComputeHalfVector, Evaluate(PDF)         BxDF.hlsli:228-315, single-lobe and all-lobe forms
  Geometry::GetBasis                       Duff et al., "Building an Orthonormal Basis, Revisited", JCGT 6(1) 2017; MathLib
                                           returns the negated pair (T = (-1,0,0), B = (0,-1,0) at N = +Z)
  Cosine::GetRay / GetPDF                  Malley's method, pdf = NoL / pi
  VNDF::GetRay / GetPDF                    Dupuy & Benyoub, "Sampling Visible GGX Normals with Spherical Caps", 2023;
                                           pdf of L = D / (2 (Vz + sqrt(a^2 (Vx^2 + Vy^2) + Vz^2))), a = roughness^2
  DistributionTerm, GeometryTermMod        GGX (Walter et al. 2007); height-correlated Smith G2 / (4 NoL NoV) (Heitz 2014)
  FresnelTerm, FresnelTerm_Dielectric      Schlick 1994; exact unpolarised dielectric Fresnel, eta = n_i / n_t
  DiffuseTerm                              Burley 2012, fd90 = 0.5 + 2 roughness VoH^2
  EnvironmentTerm_Rtg                      Ray Tracing Gems ch. 32 rational fit (feeds the lobe weights only)
  reflect / refract                        HLSL intrinsics by their definitions (refract returns 0 under TIR)

Query layout (float32 rows, shared with the oracle's or_bsdf_sample_batch and the device's pt_bsdf_sample):
  sample queries, 24 words: base.rgb metallic roughness ior transmission frontFace Ng.xyz Ns.xyz V.xyz rnd.xyzw ext(bits) 0 0
  sample results, 12 words: L.xyz pdf f.rgb weights[3] lobe(bits) ok(bits)
  evaluate queries, 20 words: the first 17 words as above, then L.xyz; results: diffuse.rgb specular.rgb pdf 0

Tolerance model (the tests follow it):
  * Evaluation is checked at the fp32 inputs the implementation used -- for a sampled query, its own L. f and pdf agree
    to REL (1e-4) relative, widened by COS_ULP / cos for cosines near 0 (an fp32 dot product of unit vectors carries an
    absolute error of a few 2^-24).
  * Where D is ill-conditioned -- one fp32 ulp of NoH moves D by more than ILL_D relative, which is true of every mirror-like
    sample -- f and pdf are each only required to be finite and > 0, and the throughput weight f / pdf is compared to REL.
  * Sampled directions are compared by angle, to ANGLE plus the conditioning of the sampler at that query
    (``sample_lobe``: the square roots near 0, and the half vector's cancellation when V grazes or lies below Ns).
  * A query within NEAR of a discrete decision may take either branch, and the branch taken must then be consistent: the
    lobe boundaries w[2] and w[2] + w[1] on rnd.x, the Fresnel coin on rnd.w, the TIR threshold and the sign of dot(Ng, L).

A `Reference` carries switches that each break one rule (``MUTATIONS``); the tests use them to show that the tolerances
are tight enough to notice each such mistake.
"""
import numpy as np

MIN_ROUGHNESS = 2e-3                      # BxDF.hlsli:19
DIFFUSE, SPECULAR, TRANSMISSION = 0, 1, 2
EXT_LAMBERTIAN_ONLY = 0x1

REL = 1e-4                                # f, pdf, f/pdf and lobe weights
COS_ULP = 4.0 * 2.0 ** -24                # absolute error of an fp32 cosine, scaled by 1/cos into the relative tolerance
ILL_D = 1e-5                              # D's relative change per fp32 ulp of NoH above which f/pdf is compared instead
ANGLE = 2e-5                              # radians
NEAR = 4e-6                               # distance to a discrete decision within which either branch is accepted

MUTATIONS = ("alpha_is_roughness", "schlick_pow4", "no_ior_swap", "no_prob_clamp", "lobe_order", "vndf_pdf_no_2",
             "burley_nol_for_voh")

# column indices of the query rows
Q_BASE, Q_METAL, Q_ROUGH, Q_IOR, Q_TRANS, Q_FRONT = slice(0, 3), 3, 4, 5, 6, 7
Q_NG, Q_NS, Q_V, Q_RND, Q_EXT, Q_L = slice(8, 11), slice(11, 14), slice(14, 17), slice(17, 21), 21, slice(17, 20)


def dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def luminance(c):                         # Color::Luminance, BT.601
    return c @ np.array([0.299, 0.587, 0.114])


def env_term_rtg(F0, NoV, roughness):
    """EnvironmentTerm_Rtg: Fenv = saturate(F0 * scale + bias), rational fits in NoV and a = roughness^2 (RTG ch. 32)."""
    a = roughness ** 2
    X = np.stack([np.ones_like(NoV), NoV, NoV ** 2, NoV ** 3], -1)
    Y = np.stack([np.ones_like(a), a, a ** 2, a ** 3], -1)
    M1 = np.array([[0.99044, -1.28514], [1.29678, -0.755907]])
    M2 = np.array([[1.0, 2.92338, 59.4188], [20.3225, -27.0302, 222.592], [121.563, 626.13, 316.627]])
    M3 = np.array([[0.0365463, 3.32707], [9.0632, -9.04756]])
    M4 = np.array([[1.0, 3.59685, -1.36772], [9.04401, -16.3174, 9.22949], [5.56589, 19.7886, -20.2123]])
    def ratio(Mn, xn, Md, xd):
        num = dot(X[..., xn] @ Mn.T, Y[..., [0, 1]])
        den = dot(X[..., xd] @ Md.T, Y[..., [0, 1, 3]])
        return num / den
    bias = ratio(M1, [0, 1], M2, [0, 1, 3])
    scale = ratio(M3, [0, 1], M4, [0, 2, 3])
    return np.clip(F0 * scale[..., None] + bias[..., None], 0.0, 1.0)


def get_basis(N):
    """Rows T, B, N; MathLib's sign convention: the negation of Duff et al.'s (b1, b2)."""
    s = np.where(N[..., 2] >= 0, 1.0, -1.0)
    a = -1.0 / (s + N[..., 2])
    b = N[..., 0] * N[..., 1] * a
    b1 = np.stack([1.0 + s * N[..., 0] ** 2 * a, s * b, -s * N[..., 0]], -1)
    b2 = np.stack([b, s + N[..., 1] ** 2 * a, -N[..., 1]], -1)
    return -b1, -b2, N


def to_local(basis, v):                   # Geometry::RotateVector
    return np.stack([dot(basis[0], v), dot(basis[1], v), dot(basis[2], v)], -1)


def to_world(basis, v):                   # Geometry::RotateVectorInverse
    return v[..., 0:1] * basis[0] + v[..., 1:2] * basis[1] + v[..., 2:3] * basis[2]


def reflect(i, n):
    return i - 2.0 * dot(n, i)[..., None] * n


def refract(i, n, eta):
    d = dot(n, i)
    k = 1.0 - eta ** 2 * (1.0 - d * d)
    out = eta[..., None] * i - (eta * d + np.sqrt(np.maximum(k, 0.0)))[..., None] * n
    return np.where((k < 0)[..., None], 0.0, out)


class Reference:
    def __init__(self, **mutations):
        unknown = set(mutations) - set(MUTATIONS)
        assert not unknown, unknown
        self.m = {k: bool(mutations.get(k, False)) for k in MUTATIONS}

    # ------------------------------------------------------------------ BRDF terms
    def alpha(self, r):
        return r if self.m["alpha_is_roughness"] else r * r

    def ggx(self, r, NoH):
        a2 = self.alpha(r) ** 2
        NoH = np.minimum(NoH, 1.0)            # fp32 unit vectors are unit to a few ulps only
        t = NoH * NoH * (a2 - 1.0) + 1.0
        return a2 / (np.pi * t * t)

    def ggx_ulp_sensitivity(self, r, NoH):
        """|dD/D| for one fp32 ulp of NoH: 4 NoH (1 - a^2) / t * ulp(NoH)."""
        a2 = self.alpha(r) ** 2
        NoH = np.minimum(NoH, 1.0)
        t = NoH * NoH * (a2 - 1.0) + 1.0
        ulp = np.spacing(np.abs(NoH).astype(np.float32)).astype(np.float64)
        return 4.0 * np.abs(NoH) * (1.0 - a2) / t * ulp

    def smith_mod(self, r, NoL, NoV):
        a2 = self.alpha(r) ** 2
        return 0.5 / (NoL * np.sqrt(a2 + NoV * NoV * (1 - a2)) + NoV * np.sqrt(a2 + NoL * NoL * (1 - a2)))

    def schlick(self, F0, VoH):
        x = np.clip(1.0 - VoH, 0.0, 1.0)[..., None]
        return F0 + (1.0 - F0) * x ** (4 if self.m["schlick_pow4"] else 5)

    @staticmethod
    def fresnel_dielectric(eta, c):
        st2 = eta * eta * (1.0 - c * c)
        ct = np.sqrt(np.clip(1.0 - st2, 0.0, 1.0))
        Rs = (eta * c - ct) / (eta * c + ct)
        Rp = (eta * ct - c) / (eta * ct + c)
        return 0.5 * (Rs * Rs + Rp * Rp)

    def burley(self, r, NoL, NoV, VoH):
        if self.m["burley_nol_for_voh"]:
            VoH = NoL
        fd90m1 = 2.0 * VoH * VoH * r - 0.5
        c = lambda x: np.clip(1.0 - x, 0.0, 1.0) ** 5
        return (1.0 + fd90m1 * c(NoV)) * (1.0 + fd90m1 * c(NoL)) / np.pi

    def vndf_pdf(self, Vl, NoH, r):
        a = self.alpha(r)
        len2 = a * a * (Vl[..., 0] ** 2 + Vl[..., 1] ** 2)
        t = np.sqrt(len2 + Vl[..., 2] ** 2)
        two = 1.0 if self.m["vndf_pdf_no_2"] else 2.0
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(Vl[..., 2] >= 0, self.ggx(r, NoH) / (two * (Vl[..., 2] + t)),
                            self.ggx(r, NoH) * (t - Vl[..., 2]) / (two * len2))

    # ------------------------------------------------------------------ BSDFSample state
    def initialize(self, q):
        q = np.asarray(q, np.float64)
        s = {"base": q[:, Q_BASE], "metal": q[:, Q_METAL], "trans": q[:, Q_TRANS], "front": q[:, Q_FRONT] != 0}
        s["albedo"] = s["base"] * (1.0 - s["metal"])[:, None]
        s["rough"] = np.maximum(MIN_ROUGHNESS, q[:, Q_ROUGH])
        ior = q[:, Q_IOR]
        swap = ~s["front"] & (not self.m["no_ior_swap"])
        s["iori"] = np.where(swap, ior, 1.0)
        s["ioro"] = np.where(swap, 1.0, ior)
        r2 = ((s["iori"] - s["ioro"]) / (s["iori"] + s["ioro"])) ** 2
        s["F0"] = r2[:, None] + (s["base"] - r2[:, None]) * s["metal"][:, None]
        s["Ng"] = np.where(s["front"][:, None], q[:, Q_NG], -q[:, Q_NG])      # FrontGeometricNormal
        s["Ns"] = q[:, Q_NS]
        s["basis"] = get_basis(s["Ns"])
        s["V"] = q[:, Q_V]
        return s

    def diffuse_probability(self, s, NoV):
        Fenv = env_term_rtg(s["F0"], NoV, s["rough"])
        d = luminance(s["albedo"] * (1.0 - Fenv))
        sp = luminance(Fenv)
        tot = d + sp
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(tot > 0, d / tot, 1.0)
        if self.m["no_prob_clamp"]:
            return p
        return np.where((p > 0) & (p < 1), np.clip(p, 0.05, 0.95), p)

    def weights(self, s, ext):
        NoV = np.abs(dot(s["Ns"], s["V"]))
        tw = s["trans"] * (1.0 - s["metal"])
        dw = self.diffuse_probability(s, NoV)
        w = np.stack([dw * (1 - tw), (1 - dw) * (1 - tw), tw], -1)
        lam = (np.asarray(ext, np.int64) & EXT_LAMBERTIAN_ONLY) != 0
        return np.where(lam[:, None], np.array([1.0, 0.0, 0.0]), w)

    def lobe_boundaries(self, w):
        """FindLobe's two thresholds on rnd.x, in the order it tests them, and the lobe each one selects."""
        order = [DIFFUSE, SPECULAR, TRANSMISSION] if self.m["lobe_order"] else [TRANSMISSION, SPECULAR, DIFFUSE]
        b0 = w[:, order[0]]
        return order, (b0, b0 + w[:, order[1]])

    def find_lobe(self, w, x):
        order, (b0, b1) = self.lobe_boundaries(w)
        return np.where(x < b0, order[0], np.where(x < b1, order[1], order[2]))

    # ------------------------------------------------------------------ sampling
    def sample_lobe(self, s, rnd, lobe):
        """Sample for a given lobe: returns L, ok, and per-row side information for the branch checks."""
        n = len(lobe)
        basis, V = s["basis"], s["V"]
        phi = 2.0 * np.pi * rnd[:, 1]
        # diffuse: cosine-weighted
        cosT = np.sqrt(np.clip(rnd[:, 2], 0, 1))
        sinT = np.sqrt(np.clip(1.0 - cosT * cosT, 0, 1))
        Ld = to_world(basis, np.stack([sinT * np.cos(phi), sinT * np.sin(phi), cosT], -1))
        # VNDF, spherical caps
        a = self.alpha(s["rough"])
        Vl = to_local(basis, V)
        with np.errstate(divide="ignore", invalid="ignore"):
            Vh = normalize(np.stack([a * Vl[:, 0], a * Vl[:, 1], Vl[:, 2]], -1))
            z = (1.0 - rnd[:, 2]) * (1.0 + Vh[:, 2]) - Vh[:, 2]
            sz = np.sqrt(np.clip(1.0 - z * z, 0, 1))
            h = np.stack([sz * np.cos(phi) + Vh[:, 0], sz * np.sin(phi) + Vh[:, 1], z + Vh[:, 2]], -1)
            hm = np.stack([a * h[:, 0], a * h[:, 1], np.maximum(h[:, 2], 0.0)], -1)
            H = to_world(basis, normalize(hm))
        Lr = reflect(-V, H)
        # transmission: Fresnel coin between reflect and refract about H
        VoH = np.abs(dot(V, H))
        eta = s["iori"] / s["ioro"]
        tir_margin = eta * eta * (1.0 - VoH * VoH) - 1.0
        with np.errstate(invalid="ignore"):
            Fr = self.fresnel_dielectric(eta, VoH)
        Lt = refract(-V, H, eta)
        Lt = np.where(np.isfinite(Lt).all(-1, keepdims=True), Lt, -V)
        take_reflect = (tir_margin > 0) | (rnd[:, 3] < Fr)
        Lx = np.where(take_reflect[:, None], Lr, Lt)
        L = np.where((lobe == DIFFUSE)[:, None], Ld, np.where((lobe == SPECULAR)[:, None], Lr, Lx))
        with np.errstate(invalid="ignore"):
            ok = np.where(lobe == TRANSMISSION, True, dot(s["Ng"], L) > 0)
        k = 1.0 - eta ** 2 * (1.0 - VoH ** 2)
        # conditioning, in radians of L, of the fp32 evaluation: the square roots sqrt(1 - z^2) (cosine, VNDF) and sqrt(k)
        # (refraction) amplify one rounding of their argument by 1/root; the cap's h.z = z + Vh.z carries an absolute error of
        # a few u however small it is, so H's angle errs by that over |(a h.x, a h.y, h.z)| -- large when V grazes or lies
        # below the shading hemisphere at low roughness, where fp32 leaves the half vector undetermined (L doubles it)
        u = 2.0 ** -24
        with np.errstate(divide="ignore", invalid="ignore"):
            c_vndf = 2 * (a * (2 * u / sz + 2 * u) + 4 * u) / np.linalg.norm(hm, axis=-1)
            c_refr = 4 * u / np.sqrt(np.abs(k))
        cond = np.where(lobe == DIFFUSE, 4 * u / sinT, c_vndf + np.where((lobe == TRANSMISSION) & ~take_reflect, c_refr, 0.0))
        side = {"Lr": Lr, "Lt": Lt, "tir_margin": tir_margin, "coin_margin": rnd[:, 3] - Fr,
                "cond": np.nan_to_num(cond, nan=np.inf), "reflect": take_reflect, "H": H}
        return L, ok, side

    # ------------------------------------------------------------------ evaluation
    def half_vector(self, s, L, transmissive):
        with np.errstate(invalid="ignore", divide="ignore"):
            below = transmissive & (dot(s["Ng"], L) < 0)
            Ht = normalize(L * s["ioro"][:, None] + s["V"] * s["iori"][:, None])
            Ht = np.where((dot(s["Ng"], Ht) < 0)[:, None], -Ht, Ht)
            return np.where(below[:, None], Ht, normalize(L + s["V"]))

    def eval_lobes(self, s, w, L, ext):
        """Single-lobe (pdf, f) for all three lobes: arrays [n, 3] and [n, 3, 3], plus the NoH the specular lobe used."""
        tw = w[:, TRANSMISSION]
        H = self.half_vector(s, L, tw > 0)
        N, V = s["Ns"], s["V"]
        above = dot(s["Ng"], L) > 0
        NoL, NoV, VoH, NoH = np.abs(dot(N, L)), np.abs(dot(N, V)), np.abs(dot(V, H)), np.abs(dot(N, H))
        rw = 1.0 - tw
        lam = (np.asarray(ext, np.int64) & EXT_LAMBERTIAN_ONLY) != 0
        dterm = np.where(lam, 1.0 / np.pi, self.burley(s["rough"], NoL, NoV, VoH))
        f_d = np.where(above[:, None], s["albedo"] * (NoL * dterm * rw)[:, None], 0.0)
        p_d = np.where(above, NoL / np.pi * w[:, DIFFUSE], 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            D = self.ggx(s["rough"], NoH)
            f_s = np.where(above[:, None], self.schlick(s["F0"], VoH) * (NoL * D * self.smith_mod(s["rough"], NoL, NoV) * rw)[:, None], 0.0)
            p_s = np.where(above, self.vndf_pdf(to_local(s["basis"], V), NoH, s["rough"]) * w[:, SPECULAR], 0.0)
        f_t = s["base"] * (NoL * tw)[:, None]
        p_t = NoL * tw
        # VNDF pdf below the shading hemisphere divides by a^2 (Vx^2 + Vy^2), whose fp32 components carry an absolute error of
        # a few u: relative conditioning 4u / |Vxy| (large as V -> -N)
        Vl = to_local(s["basis"], V)
        with np.errstate(divide="ignore"):
            len2_cond = np.where(Vl[:, 2] < 0, 4 * 2.0 ** -24 / np.hypot(Vl[:, 0], Vl[:, 1]), 0.0)
        # Schlick's (1 - VoH)^5 carries VoH's absolute error as 5 u / (1 - VoH) relative, in the share of F it makes up
        x5 = np.clip(1.0 - VoH, 0.0, 1.0) ** 5
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.nan_to_num(((1.0 - s["F0"]) * x5[:, None] / (s["F0"] + (1.0 - s["F0"]) * x5[:, None])).max(1))
            schlick_cond = share * 10 * 2.0 ** -24 / np.maximum(1.0 - VoH, 1e-300)
        aux = {"NoL": NoL, "NoV": NoV, "above": above, "len2_cond": len2_cond, "schlick_cond": schlick_cond}
        return np.stack([p_d, p_s, p_t], -1), np.stack([f_d, f_s, f_t], 1), NoH, aux

    def evaluate_all(self, q):
        """All-lobe Evaluate / EvaluatePDF (BxDF.hlsli:247-285) of evaluate queries: diffuse [n,3], specular [n,3], pdf [n]."""
        s = self.initialize(q)
        L = np.asarray(q, np.float64)[:, Q_L]
        w = self.weights(s, np.zeros(len(q), np.int64))
        p, f, NoH, aux = self.eval_lobes(s, w, L, 0)
        tw = w[:, TRANSMISSION]
        refl = (tw < 1) & aux["above"]
        pdf = np.where(tw > 0, p[:, 2], 0.0) + np.where(refl, p[:, 0] + p[:, 1], 0.0)
        dif = np.where(refl[:, None], f[:, 0], 0.0)
        spc = np.where((tw > 0)[:, None], f[:, 2], 0.0) + np.where(refl[:, None], f[:, 1], 0.0)
        return dif, spc, pdf, s, w, NoH, aux


def ext_bits(q):
    return np.ascontiguousarray(q[:, Q_EXT]).view(np.uint32).astype(np.int64)
