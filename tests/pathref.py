"""Float64 replay of the path estimator: RayGeneration of Shaders/Raytracing.hlsl:103-415 (default permutation; untextured or textured
scenes -- RGBA8, RGBA8 sRGB and RGBA32F textures, not block-compressed ones; constant environment colour, the procedural sky, or a lat-long
or cube environment texture under EnvironmentLightTransform), numpy only, vectorised over pixels with a loop over samples and bounces.

Restated from the shader, not from csrc/pt_shade.hpp or oracle/pt_oracle.c. It starts where the shader starts: from the G-buffer textures it
is handed (Position, FlatNormal / GeometricNormal octahedral, NormalRoughness, BaseColorMetalness, IOR, Transmission, Radiance), decoded
in float64; tests/surfaceref.py pins those textures, so the two references meet at the texture boundary.

  RNG        exact in integers: Rng::Hash::Initialize = HashCombine(Hash(frame + 0x035F9F29), x << 16 | y) with the lowbias32 hash and
             the boost combine; every draw advances the LCG (1664525, 1013904223), hashes the state and scales its top 24 bits by 2^-24.
             ONE stream per pixel across all samples; four floats per bounce (GetFloat4: x, y, z, w); one more for the roulette, drawn
             only when IsRussianRouletteEnabled and bounce > 3.
  BSDF       bsdfref.Reference: Initialize, lobe weights, FindLobe, Sample, single-lobe EvaluatePDF / Evaluate.
  geometry   surfaceref: brute-force float64 closest hit and hit reconstruction. The next ray starts at the hit position displaced along
             the flat normal on the side of L by the hit's own PositionOffset (GetSafeWorldRayOrigin in float64; for the primary
             surface the offset the texture stores). The fp32 rounding of that offset (a few 1e-7) is not mimicked.
  estimator  in the shader's order: emission (primary: the Radiance texture), sample; break on !ok, pdf == 0, f == 0; throughput *= f / pdf;
             roulette on max(throughput) from bounce 4 on; break on luminance(throughput) <= ThroughputThreshold; bounceIndex <= Bounces;
             environment on a miss; isDiffuse / hitDistance from sample 0 at bounce 1; sum over samples; 0 if the fp32 sum is not finite,
             else / spp. IsDIEnabled (:150-163, :302, :382/:390, :405-412): DI = Diffuse.rgb + Specular.rgb, valid if any channel > 0;
             a valid DI suppresses the emission met at bounce 1 and is added after the division (None, DLSS-RR) or goes, term by term,
             into the NRD outputs.

`risky` pixels: a decision of some sample lies within its margin of flipping in fp32 -- the lobe boundaries on rnd.x and the Fresnel coin /
TIR threshold (bsdfref.NEAR); the sign of dot(Ng, L) (NEAR + the sine of the direction tolerance bsdfref gives that sample); the
front-face sign at a hit (|dot(N, d)| < FRONT = 1e-4); surfaceref's edge / depth classification of the closest hit, widened by the lateral
drift of the ray (its angle tolerance times t, plus 1e-6 (1 + |origin|)) -- which also covers a ray that passes that close to a silhouette
edge it misses; the roulette draw against max(throughput) and the luminance against the threshold, each within DECISION_REL = 4 REL
(bounce + 1) relative (the throughput's accumulated tolerance); an fp32 sum within the pixel's tolerance of FLT_MAX.

`budget` = sum over contributions (emission or environment met at vertex k) of (k + 1) |contribution|: every vertex before a contribution
adds one f / pdf at bsdfref.REL. A pixel agrees when |got - ref| <= REL * budget / spp + one fp32 ulp of the result per channel (`tolerance`);
the f16 outputs get one f16 ulp on top, the hit distance REL relative plus one f16 ulp.
Largest error / tolerance seen on kept pixels of the CPU oracle (tests/test_estimator_reference.py prints it per row): 0.039, on row
`ggx_s2_b6_no_roulette` (at most 0.013 on the other rows; p99 below 0.0025 and the median relative error below 1e-7 on every row). Loose
by design; the mutations show that it is tight enough.

Textured vertices (Raytracing.hlsl:289-301 EvaluateMaterial with hitInfo.ShadingNormal, GetFrontTangent() and the hit's TextureCoordinates;
RaytracingHelpers.hlsli:19-44 the alpha test of every CANDIDATE_NON_OPAQUE_TRIANGLE; ShadingHelpers.hlsli:11-30 the environment): at every
bounce hit surfaceref.Surface.material evaluates the textured material, on every miss Surface.environment the textured environment, and
bounce rays take surfaceref's alpha-aware closest hit. A candidate the alpha rule turns down draws no random number: the stream of a pixel
advances at BSDF samples and roulette only. An untextured scene takes none of these branches, and its figures are bit for bit what they
were. What a texture adds to the tolerance is `texture_slack`, absolute, next to REL * budget:
  a tap's value      differs in fp32 because its position does: (the largest difference between neighbouring texels around the footprint)
                     x (texture size x the triangle's UV extent x the barycentric uncertainty of the hit -- surfaceref's edge margin of
                     that (ray, triangle) pair: EDGE_B, the transform term, and the ray's drift over the triangle's world altitude), plus
                     texref's own position and value tolerance (test_texture_reference.py's), which covers the fp32 interpolation of the
                     f16 corners (surfaceref.Surface.tap_bound)
  emission, environment   enter linearly: |throughput| x the bound
  base colour, metallic, roughness, transmission, the perturbed normal   finite differences (textured_vertex): the vertex evaluated once
                     more per quantity moved by its bound -- lobe weights, sampled direction, single-lobe f / pdf; the relative change of
                     f / pdf accumulates along the path and scales every later contribution; the change of the lobe weights widens
                     near_lobe; the change of the sampled direction widens the next ray's drift
  decisions          `risky` within their bound: Metallic < 1 ahead of the Transmission tap, the rim of the normal map where
                     sqrt(saturate(1 - x^2 - y^2)) clamps, a candidate's alpha against AlphaCutoff (unless the tap is constant 0 or 1 over
                     the whole box its position can lie in: then fp32 samples it exactly, also AT the cutoff), the lat-long poles
                     (atan2 / acos, and the NaN-coordinate rule at |w.y| = 1) within surfaceref.POLE
Largest error / tolerance on kept pixels of the CPU oracle on the textured rows (tests/test_textured_estimator.py prints it per row): 0.045 on
`textured_s1_b1`, 0.041 on `plain_s2_b6` and `plain_masked_s2_b6`, at most 0.0085 on the other rows (textured_s2_b6 with and without
roulette, DLSS-RR, latlong_s2_b6 0.0079, cube_s2_b6 0.0076, plain_transmissive_s2_b6, large_s2_b6); p99 below 0.0024 on every row.

MUTATIONS: switches that each break one rule; the tests show that the comparison notices each.
"""
import numpy as np

import bsdfref as B
import surfaceref as R

REL = B.REL
FRONT = 1e-4
DECISION_REL = 4.0 * REL
FLT_MAX = float(np.finfo(np.float32).max)
DENOISER_NONE, DENOISER_DLSS_RR, DENOISER_NRD_REBLUR, DENOISER_NRD_RELAX = 0, 1, 2, 3
MUTATIONS = ("roulette_from_3", "roulette_no_divide", "threshold_before_roulette", "bounce_exclusive", "emission_after_throughput",
             "divide_before_finite", "rng_per_sample", "hit_distance_bounce0", "is_diffuse_last_sample",
             "di_suppress_bounce2", "di_before_divide", "di_swapped", "di_valid_all",
             "alpha_skip_bounce", "material_at_primary_uv", "rejected_draws_random")
DI_MUTATIONS = tuple(m for m in MUTATIONS if m.startswith("di_"))
TEXTURE_MUTATIONS = ("alpha_skip_bounce", "material_at_primary_uv", "rejected_draws_random")

f64 = np.float64
M32 = np.uint64(0xFFFFFFFF)


# ----------------------------------------------------------------------------------------------
# Rng::Hash, in integers
# ----------------------------------------------------------------------------------------------
def hash32(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def hash_combine(seed, v):
    seed = np.asarray(seed, np.uint64) & M32
    return seed ^ ((hash32(v) + np.uint64(0x9E3779B9) + ((seed << np.uint64(6)) & M32) + (seed >> np.uint64(2))) & M32)


def rng_init(px, py, frame):
    px, py = np.asarray(px, np.uint64), np.asarray(py, np.uint64)
    return hash_combine(hash32(np.uint64((int(frame) + 0x035F9F29) & 0xFFFFFFFF)), ((px << np.uint64(16)) | py) & M32)


def rng_float(state, rows):
    """advance the streams `rows` of `state` (in place) and return their next float in [0, 1)"""
    state[rows] = (state[rows] * np.uint64(1664525) + np.uint64(1013904223)) & M32
    return (hash32(state[rows]) >> np.uint64(8)).astype(f64) * 2.0 ** -24


def ulp32(x):
    return np.spacing(np.minimum(np.abs(x), 3.0e38).astype(np.float32)).astype(f64)


# ----------------------------------------------------------------------------------------------
# the replay
# ----------------------------------------------------------------------------------------------
def decode_primary(textures, n):
    t = {k: np.asarray(v).reshape(n, -1) for k, v in textures.items()}
    P = t["Position"].astype(f64)
    nr = np.maximum(t["NormalRoughness"].astype(f64) / 32767.0, -1.0)
    bcm = t["BaseColorMetalness"].astype(f64) / 255.0
    out = {"position": P[:, :3], "offset": P[:, 3], "hit": np.isfinite(P[:, 3]),
           "flat": R.oct_decode(np.maximum(t["FlatNormal"].astype(f64) / 32767.0, -1.0)),
           "geometric": R.oct_decode(np.maximum(t["GeometricNormal"].astype(f64) / 32767.0, -1.0)),
           "shading": nr[:, :3], "roughness": nr[:, 3], "base": bcm[:, :3], "metal": bcm[:, 3], "ior": R.f16(t["IOR"][:, 0]),
           "transmission": np.where(bcm[:, 3] < 1, t["Transmission"][:, 0].astype(f64) / 255.0, 0.0), "radiance": R.f16(t["Radiance"][:, :3])}
    if "Diffuse" in t and "Specular" in t:
        out["direct_diffuse"], out["direct_specular"] = R.f16(t["Diffuse"][:, :3]), R.f16(t["Specular"][:, :3])
    return out


def replay(scene, settings, textures, camera, scene_data, di=None, mutations=(), surface=None, rows=None):
    """The frame the shader computes from `textures` (name -> array in the stored format, the pixels of rows [y0, y1) or the whole frame,
    row-major) for a finalized scenes.Scene. di: consume textures["Diffuse"] / ["Specular"] as IsDIEnabled does (default:
    settings["IsDIEnabled"]). Returns per pixel (flattened): primary_hit, radiance [n, 3] (what Denoiser None / DLSS-RR store; the
    G-buffer's value where the shader writes nothing), diffuse / specular [n, 4] (the NRD outputs), specular_hit_distance and
    specular_hit_distance_written, is_diffuse, hit_distance, segments (rays traced), budget / tolerance [n, 3], risky."""
    unknown = set(mutations) - set(MUTATIONS)
    assert not unknown, unknown
    mut = {k: k in mutations for k in MUTATIONS}
    gs = np.asarray(settings).reshape(())
    cam = np.asarray(camera).reshape(())
    sd = np.asarray(scene_data).reshape(())
    W, H = (int(v) for v in gs["RenderSize"])
    spp, bounces, frame = int(gs["SamplesPerPixel"]), int(gs["Bounces"]), int(gs["FrameIndex"])
    roulette, threshold, ext = int(gs["IsRussianRouletteEnabled"]) != 0, float(gs["ThroughputThreshold"]), int(gs["ExtFlags"])
    denoiser = int(gs["Denoiser"])
    di = (int(gs["IsDIEnabled"]) != 0) if di is None else bool(di)
    surface = surface if surface is not None else R.Surface(scene)
    ref = B.Reference()
    uv, pix = R.pixel_uv(W, H, cam["Jitter"], rows)
    n = len(uv)
    o0, d0, _, _ = R.pinhole(cam, uv)
    prim = decode_primary(textures, n)
    hitp = prim["hit"]
    state = rng_init(pix[:, 0].astype(np.uint64), pix[:, 1].astype(np.uint64), frame)
    state0 = state.copy()

    direct_d = np.zeros((n, 3)); direct_s = np.zeros((n, 3))
    if di:
        direct_d = np.where(hitp[:, None], prim["direct_diffuse"], 0.0); direct_s = np.where(hitp[:, None], prim["direct_specular"], 0.0)
    DI = direct_d + direct_s
    di_valid = ((DI > 0).all(1) if mut["di_valid_all"] else (DI > 0).any(1)) & di & hitp

    radiance = np.zeros((n, 3)); budget = np.zeros((n, 3))
    risky = np.zeros(n, bool)
    segments = np.zeros(n, np.int64)
    rejected = np.zeros(n, np.int64)                                        # candidates of bounce rays the alpha rule turned down
    is_diffuse = np.ones(n, bool); hit_distance = np.full(n, np.inf)
    emissive_at_bounce_1 = np.zeros(n, bool)
    primary_front = R.dot(prim["geometric"], d0) < 0
    risky |= hitp & (np.abs(R.dot(prim["geometric"], d0)) < FRONT)
    alpha = surface.alpha_rule if len(surface.alpha_rule.tested) else None
    slack = np.zeros((n, 3))                                                # what the textures' fp32 tap positions may move the sum by
    primary_uv = None
    if mut["material_at_primary_uv"]:
        _, _, tmin0, tmax0 = R.pinhole(cam, uv)
        c0 = surface.tris.closest(o0, d0, tmin0, tmax0, alpha=alpha)
        primary_uv = surface.uv_of(c0["tri"], c0["u"], c0["v"])

    for sample in range(spp):
        if mut["rng_per_sample"]:
            state[:] = state0
        act = np.nonzero(hitp)[0]                                           # a primary miss returns at bounce 0
        k = len(act)
        # the state of the live paths, rows parallel to `act`
        cur = {"position": prim["position"][act], "offset": prim["offset"][act], "flat": prim["flat"][act], "geometric": prim["geometric"][act],
               "shading": prim["shading"][act], "front": primary_front[act], "base": prim["base"][act], "metal": prim["metal"][act],
               "roughness": prim["roughness"][act], "ior": prim["ior"][act], "transmission": prim["transmission"][act],
               "emission": prim["radiance"][act], "direction": d0[act], "distance": np.linalg.norm(prim["position"][act] - o0[act], axis=1)}
        throughput = np.ones((k, 3)); sample_radiance = np.zeros((k, 3)); sample_budget = np.zeros((k, 3))
        sample_slack = np.zeros((k, 3)); drifted = np.zeros((k, 3))           # drifted: the throughput's relative error from textured vertices
        L = np.zeros((k, 3)); lobe = np.zeros(k, np.int64); angle = np.zeros(k)
        last = bounces - 1 if mut["bounce_exclusive"] else bounces
        for bounce in range(last + 1):
            if not len(act):
                break
            if bounce:
                sgn = np.where(R.dot(L, cur["flat"]) >= 0, 1.0, -1.0)       # Math::Sign: never 0
                origin = cur["position"] + (cur["offset"] * sgn)[:, None] * cur["flat"]
                c = closest_with_drift(surface.tris, origin, L, angle, None if mut["alpha_skip_bounce"] else alpha)
                if mut["rejected_draws_random"] and c["rejected"].any():
                    rng_float(state, act[c["rejected"] > 0])
                segments[act] += 1
                rejected[act] += c["rejected"]
                risky[act] |= c["unsafe"]
                h = surface.reconstruct(c["tri"], c["u"], c["v"], L)
                hit = c["hit"]
                cur = {"direction": L, "distance": c["t"], "hit": hit}
            else:
                hit = np.ones(len(act), bool)
            if bounce == 1 and sample == (spp - 1 if mut["is_diffuse_last_sample"] else 0):
                is_diffuse[act] = lobe == B.DIFFUSE
            if sample == 0 and bounce == (0 if mut["hit_distance_bounce0"] else 1):
                hit_distance[act] = cur["distance"]
            if bounce:
                miss = ~hit
                env = surface.environment(sd, L)
                contrib = throughput * env
                sample_radiance[miss] += contrib[miss]; sample_budget[miss] += (bounce + 1) * np.abs(contrib[miss])
                env_bound, env_undecided = surface.environment_bound(sd, L, angle)
                if env_bound.any() or drifted.any():
                    sample_slack[miss] += (np.abs(throughput) * env_bound[:, None] + np.abs(contrib) * drifted)[miss]
                risky[act[miss]] |= env_undecided[miss]
                # the paths that go on: compact every per-path array
                keep = hit
                radiance[act[miss]] += sample_radiance[miss]; budget[act[miss]] += sample_budget[miss]; slack[act[miss]] += sample_slack[miss]
                act, throughput, sample_radiance, sample_budget, L = act[keep], throughput[keep], sample_radiance[keep], sample_budget[keep], L[keep]
                sample_slack, drifted = sample_slack[keep], drifted[keep]
                hk = {kk: v[keep] for kk, v in h.items()}
                if primary_uv is not None:
                    hk["uv"] = primary_uv[act]
                mat = surface.material(hk["object"], hk, c["bary"][keep])       # EvaluateMaterial at the hit: its UVs, shading normal, front tangent
                emission = mat["EmissiveStrength"][:, None] * mat["EmissiveColor"]
                bound = mat.get("bound")
                if bound is not None:
                    risky[act] |= mat["undecided"]
                if bounce == 1:
                    emissive_at_bounce_1[act] |= (emission > 0).any(1)
                suppressed = 2 if mut["di_suppress_bounce2"] else 1
                if bounce == suppressed:
                    emission = np.where(di_valid[act][:, None], 0.0, emission)
                risky[act] |= hk["perp"] < FRONT
                cur = {"position": hk["position"], "offset": hk["offset"], "flat": hk["flat"], "geometric": hk["geometric"],
                       "shading": mat.get("Normal", hk["shading"]),
                       "front": hk["front"], "base": np.asarray(mat["BaseColor"], f64)[:, :3], "metal": np.asarray(mat["Metallic"], f64),
                       "roughness": np.asarray(mat["Roughness"], f64), "ior": np.asarray(mat["IOR"], f64),
                       "transmission": np.asarray(mat["Transmission"], f64), "emission": emission, "direction": L, "distance": cur["distance"][keep]}
                if bound is not None:
                    cur.update({"d_" + kk: v for kk, v in bound.items()})
                if not len(act):
                    break
            m = len(act)
            if not mut["emission_after_throughput"]:
                contrib = throughput * cur["emission"]
                sample_radiance += contrib; sample_budget += (bounce + 1) * np.abs(contrib)
                if drifted.any():
                    sample_slack += np.abs(contrib) * drifted
                if "d_emission" in cur:
                    sample_slack += np.abs(throughput) * cur["d_emission"][:, None]
            # BSDFSample: weights, lobe, direction, pdf, f
            rnd = np.stack([rng_float(state, act) for _ in range(4)], -1)
            q = np.zeros((m, 24))
            q[:, B.Q_BASE] = cur["base"]; q[:, B.Q_METAL] = cur["metal"]; q[:, B.Q_ROUGH] = cur["roughness"]; q[:, B.Q_IOR] = cur["ior"]
            q[:, B.Q_TRANS] = cur["transmission"]; q[:, B.Q_FRONT] = cur["front"]
            q[:, B.Q_NG] = cur["geometric"]; q[:, B.Q_NS] = cur["shading"]; q[:, B.Q_V] = -cur["direction"]
            extv = np.full(m, ext, np.int64)
            s = ref.initialize(q)
            w = ref.weights(s, extv)
            lobe = ref.find_lobe(w, rnd[:, 0])
            with np.errstate(invalid="ignore", divide="ignore"):
                L, ok, side = ref.sample_lobe(s, rnd, lobe)
            moved = textured_vertex(ref, cur, q, s, w, rnd, lobe, L, extv) if "d_base" in cur else None
            margin = B.NEAR if moved is None else B.NEAR + moved["weights"]
            near_lobe = (ref.find_lobe(w, rnd[:, 0] - margin) != lobe) | (ref.find_lobe(w, rnd[:, 0] + margin) != lobe)
            with np.errstate(invalid="ignore", divide="ignore"):
                angle = np.minimum(B.ANGLE + side["cond"], 1.0) if moved is None else np.minimum(B.ANGLE + side["cond"] + moved["angle"], 1.0)
                horizon = (lobe != B.TRANSMISSION) & ~(np.abs(R.dot(s["Ng"], L)) > B.NEAR + np.sin(angle))
                branch = (lobe == B.TRANSMISSION) & ((np.abs(side["tir_margin"]) <= B.NEAR) | (np.abs(side["coin_margin"]) <= B.NEAR))
                p_all, f_all, _, _ = ref.eval_lobes(s, w, np.where(np.isfinite(L).all(1, keepdims=True), L, s["Ns"]), extv)
            risky[act] |= near_lobe | horizon | branch
            rowsm = np.arange(m)
            pdf, f = p_all[rowsm, lobe], f_all[rowsm, lobe]
            with np.errstate(invalid="ignore", divide="ignore"):
                go = ok & (pdf != 0) & ~(f == 0).all(1)
                new_tp = throughput * f / pdf[:, None]
            if mut["emission_after_throughput"]:
                contrib = np.where(go[:, None], new_tp, throughput) * cur["emission"]
                sample_radiance += contrib; sample_budget += (bounce + 1) * np.abs(contrib)
            throughput = np.where(go[:, None], new_tp, throughput)
            rel = DECISION_REL * (bounce + 1)
            if moved is not None:
                drifted = drifted + moved["ratio"]
            if drifted.any():
                rel = rel + drifted.max(1)

            def threshold_test(tp):
                lum = B.luminance(tp)
                risky[act] |= go & (np.abs(lum - threshold) <= rel * lum)
                return lum <= threshold
            if mut["threshold_before_roulette"]:
                go &= ~threshold_test(throughput)
            if roulette and bounce > (2 if mut["roulette_from_3"] else 3):
                p = throughput.max(1)
                draw = np.zeros(m)
                draw[go] = rng_float(state, act[go])
                survive = ~(draw >= p)
                risky[act] |= go & (np.abs(draw - p) <= rel * p)
                go &= survive
                if not mut["roulette_no_divide"]:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        throughput = np.where(go[:, None], throughput / p[:, None], throughput)
            if not mut["threshold_before_roulette"]:
                go &= ~threshold_test(throughput)
            ended = ~go
            radiance[act[ended]] += sample_radiance[ended]; budget[act[ended]] += sample_budget[ended]; slack[act[ended]] += sample_slack[ended]
            act, throughput, sample_radiance, sample_budget = act[go], throughput[go], sample_radiance[go], sample_budget[go]
            sample_slack, drifted = sample_slack[go], drifted[go]
            L, lobe, angle = L[go], lobe[go], angle[go]
            cur = {kk: v[go] for kk, v in cur.items()}
        radiance[act] += sample_radiance; budget[act] += sample_budget        # paths the bounce limit ended
        slack[act] += sample_slack

    tolerance = REL * budget / max(spp, 1) + slack / max(spp, 1)
    if mut["di_before_divide"]:
        radiance = radiance + DI
    if mut["divide_before_finite"]:
        radiance = radiance / spp
        finite = np.isfinite(radiance.astype(np.float32)).all(1)
        radiance = np.where(finite[:, None], radiance, 0.0)
    else:
        with np.errstate(over="ignore"):
            finite = np.isfinite(radiance.astype(np.float32)).all(1)           # the shader's sum is fp32
        with np.errstate(invalid="ignore"):                                       # an infinite sum (an emitter beyond f16 in view) is decided
            risky |= (np.isfinite(radiance) & (np.abs(np.abs(radiance) - FLT_MAX) <= tolerance * spp + ulp32(radiance))).any(1)
        radiance = np.where(finite[:, None], radiance / spp, 0.0)
    tolerance = np.where(finite[:, None], tolerance, 0.0)
    out = {"primary_hit": hitp, "is_diffuse": is_diffuse, "hit_distance": hit_distance, "segments": segments, "rejected": rejected, "budget": budget, "texture_slack": slack, "risky": risky & hitp,
           "di_valid": di_valid, "sampled": radiance.copy(), "emissive_at_bounce_1": emissive_at_bounce_1}
    final = radiance + (0.0 if mut["di_before_divide"] else DI)
    out["radiance"] = np.where(hitp[:, None], final, prim["radiance"])
    out["tolerance"] = tolerance + ulp32(out["radiance"])
    out["specular_hit_distance_written"] = hitp & ~is_diffuse & np.isfinite(hit_distance) & (denoiser == DENOISER_DLSS_RR)
    out["specular_hit_distance"] = np.where(out["specular_hit_distance_written"], hit_distance, 0.0)
    indirect = np.maximum(radiance - prim["radiance"], 0.0)
    dd, ds = (direct_s, direct_d) if mut["di_swapped"] else (direct_d, direct_s)
    zero = np.zeros(n)
    out["diffuse"] = np.concatenate([dd + np.where(is_diffuse[:, None], indirect, 0.0), np.where(is_diffuse, hit_distance, zero)[:, None]], -1)
    out["specular"] = np.concatenate([ds + np.where(is_diffuse[:, None], 0.0, indirect), np.where(is_diffuse, zero, hit_distance)[:, None]], -1)
    return out


def closest_with_drift(tris, origin, direction, angle, alpha=None):
    """surfaceref's closest hit of bounce rays whose fp32 twins may drift sideways by angle * t + 1e-6 (1 + |origin|): the edge margin of
    every (ray, triangle) pair is widened by that drift over the triangle's smallest world-space altitude. alpha: surfaceref's alpha
    rule, put to every candidate; the margin is also the barycentric uncertainty the rule and the material's taps are bounded with."""
    return tris.closest(origin, direction, 0.0, np.inf, drift=(angle, 1e-6 * (1.0 + np.linalg.norm(origin, axis=1))), alpha=alpha)


def textured_vertex(ref, cur, q, s, w, rnd, lobe, L, extv):
    """What the bounds of a textured vertex's material (cur["d_*"], surfaceref.Surface.material) are worth downstream, by finite
    differences: one more evaluation of the whole vertex -- state, lobe weights, sampled direction, single-lobe f / pdf -- per quantity,
    moved by its bound (base colour: all channels at once, it enters linearly; the normal: tilted along the basis tangent). Returns
    `ratio` [m, 3] the relative change of f / pdf, `weights` [m] the change of the lobe weights (widens the lobe decision on rnd.x),
    `angle` [m] the change of the sampled direction (radians; widens the next ray's drift)."""
    m = len(lobe)
    rows = np.arange(m)
    out = {"ratio": np.zeros((m, 3)), "weights": np.zeros(m), "angle": np.zeros(m)}

    def evaluate(qq, ss=None, ww=None, LL=None):
        with np.errstate(invalid="ignore", divide="ignore"):
            if ss is None:
                ss = ref.initialize(qq); ww = ref.weights(ss, extv)
                LL = ref.sample_lobe(ss, rnd, lobe)[0]
            p, f, _, _ = ref.eval_lobes(ss, ww, np.where(np.isfinite(LL).all(1, keepdims=True), LL, ss["Ns"]), extv)
            return ww, LL, f[rows, lobe] / p[rows, lobe][:, None]
    _, _, ratio0 = evaluate(q, s, w, L)
    for key, col in (("base", B.Q_BASE), ("metal", B.Q_METAL), ("rough", B.Q_ROUGH), ("trans", B.Q_TRANS), ("normal", B.Q_NS)):
        dv = cur["d_" + key]
        if not dv.any():
            continue
        q2 = q.copy()
        if key == "normal":
            q2[:, col] = R.normalize(q[:, col] + dv[:, None] * s["basis"][0])
        elif key == "base":
            q2[:, col] = q[:, col] + dv[:, None]
        else:
            q2[:, col] = np.where(q[:, col] + dv > 1.0, q[:, col] - dv, q[:, col] + dv)      # stay inside [0, 1]
        w2, L2, ratio2 = evaluate(q2)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(ratio2 - ratio0) / np.abs(ratio0)
        out["ratio"] += np.where(np.isfinite(rel), rel, 0.0)
        out["weights"] += np.abs(w2 - w).sum(1)
        with np.errstate(invalid="ignore"):
            out["angle"] += np.nan_to_num(np.linalg.norm(L2 - L, axis=1), nan=0.0, posinf=0.0)
    return out


# ----------------------------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------------------------
def compare(out, rep, settings, f32=None):
    """Textures `out` of a frame (Radiance, and for a denoiser Diffuse / Specular / SpecularHitDistance; f32: RadianceF32 if the frame has
    it) against a replay. Returns (failures: output -> number of kept pixels outside tolerance, figures)."""
    gs = np.asarray(settings).reshape(())
    denoiser = int(gs["Denoiser"])
    n = len(rep["risky"])
    keep = rep["primary_hit"] & ~rep["risky"]
    fails, fig = {}, {"risky_share": float(rep["risky"].sum() / max(1, rep["primary_hit"].sum())), "kept": int(keep.sum())}

    def fail(name, bad, where=keep):
        k = int((bad & where).sum())
        if k:
            fails[name] = k
    flat = {k: np.asarray(v).reshape(n, -1) for k, v in out.items()}
    tol = rep["tolerance"]
    nrd = denoiser in (DENOISER_NRD_REBLUR, DENOISER_NRD_RELAX)
    if not nrd:
        if f32 is not None:
            got = np.asarray(f32).reshape(n, -1)[:, :3].astype(f64)
            err = np.abs(got - rep["radiance"])
            fail("RadianceF32", ~(err <= tol).all(1))
            ratio = (err / tol)[keep]
            fig["worst"] = float(np.nanmax(ratio)) if keep.any() else 0.0
            fig["p99"] = float(np.nanpercentile(ratio, 99)) if keep.any() else 0.0
            fig["median_rel"] = float(np.nanmedian((err / np.maximum(np.abs(rep["radiance"]), 1e-30))[keep])) if keep.any() else 0.0
        fail("Radiance", ~R.f16_close(flat["Radiance"][:, :3], rep["radiance"], tol).all(1))
        fail("Radiance (primary miss)", ~R.f16_close(flat["Radiance"][:, :3], rep["radiance"]).all(1), ~rep["primary_hit"])
    if denoiser == DENOISER_DLSS_RR:
        wr = rep["specular_hit_distance_written"]
        fail("SpecularHitDistance", ~R.f16_close(flat["SpecularHitDistance"][:, 0], rep["specular_hit_distance"], REL * rep["specular_hit_distance"]), keep & wr)
        fail("SpecularHitDistance (not written)", flat["SpecularHitDistance"][:, 0] != 0, keep & ~wr)
    if nrd:
        for name, key in (("Diffuse", "diffuse"), ("Specular", "specular")):
            fail(name, ~R.f16_close(flat[name][:, :3], rep[key][:, :3], tol).all(1))
            with np.errstate(invalid="ignore"):
                fail(name + ".w", ~R.f16_close(flat[name][:, 3], rep[key][:, 3], REL * np.nan_to_num(np.abs(rep[key][:, 3]), posinf=0.0)))
    return fails, fig
