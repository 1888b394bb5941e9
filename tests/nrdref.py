"""numpy restatement of the NRD composition pass ("NRD composition"): the arbiter of
tests/test_nrd_composition_*.py. Shaders/NRDComposition.hlsl:36-88 gives the frame of the pass; what it calls from NRD.hlsli (an empty
submodule of the reference) is this library's own specification after the SDK, from memory: parity with the SDK is unpinned.

Every operation is one IEEE fp32 operation on float32 arrays, in the order of the spec; textures are uint16 arrays of fp16 bits
(..., 4), LinearDepth float32 (...), NormalRoughness int16 (..., 4). The three selects (clamp0, max0, the no-data mark) send NaN and -0
to +0, so that no result depends on how a min / max instruction orders them. An fp16 store rounds to nearest even and stores a NaN as
0x7E00. The only operation that is not bit-pinned is exp2 in the ReBLUR hit-distance normalisation: here it is the correctly rounded
fp32 value (float64 exp2, rounded once)."""
import numpy as np

F32 = np.float32
DENOISER_NONE, DENOISER_DLSS_RR, DENOISER_NRD_REBLUR, DENOISER_NRD_RELAX = 0, 1, 2, 3
REBLUR_HIT_DISTANCE_DEFAULTS = (3.0, 0.1, 20.0, -25.0)
FP16_MAX = F32(65504.0)
MIN_HIT_DISTANCE = F32(1e-7)
NAN16 = 0x7E00


def f16_to_f32(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def f32_to_f16(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16).view(np.uint16)
    return np.where(np.isnan(x), np.uint16(NAN16), h).astype(np.uint16)


def snorm16_to_f32(v):
    v = np.asarray(v, np.int16)
    return np.where(v == -32768, F32(-1.0), v.astype(np.float32) / F32(32767.0)).astype(np.float32)


def clamp0(x, hi):
    """clamp(x, 0, hi) with NaN and -0 -> +0; saturate for hi = 1"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.minimum(x, F32(hi)), F32(0.0)).astype(np.float32)


def max0(x):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, F32(0.0)).astype(np.float32)


def mark(a):
    """0 is NRD's "no data" mark: a hit distance (>= 0) that is not 0 becomes max(a, 1e-7f)"""
    a = np.asarray(a, np.float32)
    return np.where((a != 0) & (a < MIN_HIT_DISTANCE), MIN_HIT_DISTANCE, a).astype(np.float32)


def sanitize(rgb):
    """(..., 3): all three become 0 when one is NaN or +-inf, else clamp(rgb, 0, 65504)"""
    rgb = np.asarray(rgb, np.float32)
    ok = np.isfinite(rgb).all(-1, keepdims=True)
    return np.where(ok, clamp0(rgb, FP16_MAX), F32(0.0)).astype(np.float32)


def exp2_f32(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp2(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def norm_hit_dist(a, z, P, r):
    """REBLUR_FrontEnd_GetNormHitDist: n = saturate(a / f), f = (P.x + |z| P.y) (1 + t (P.z - 1)), t = saturate(exp2(P.w r r))"""
    P = np.asarray(P, np.float32)
    a, z, r = (np.asarray(v, np.float32) for v in (a, z, r))
    with np.errstate(all="ignore"):
        s = P[0] + np.abs(z) * P[1]
        t = clamp0(exp2_f32(P[3] * r * r), 1.0)
        f = s * (F32(1.0) + t * (P[2] - F32(1.0)))
        return clamp0(a / f, 1.0)


def ycocg(rgb):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    with np.errstate(all="ignore"):
        Y = (r * F32(0.25) + g * F32(0.5)) + b * F32(0.25)
        Co = r * F32(0.5) + b * F32(-0.5)
        Cg = (r * F32(-0.25) + g * F32(0.5)) + b * F32(-0.25)
    return np.stack([Y, Co, Cg], -1).astype(np.float32)


def ycocg_to_rgb(ycc):
    Y, Co, Cg = ycc[..., 0], ycc[..., 1], ycc[..., 2]
    with np.errstate(all="ignore"):
        t = Y - Cg
        return np.stack([max0(t + Co), max0(Y + Cg), max0(t - Co)], -1).astype(np.float32)


def pack_values(denoiser, rgb, a, z, P, r):
    """The pack after the demodulation, before the fp16 store: (rgb or YCoCg (..., 3), alpha (...)) as float32. ReLAX / ReBLUR only."""
    if denoiser == DENOISER_NRD_REBLUR:
        n = norm_hit_dist(a, z, P, r)
        return ycocg(sanitize(rgb)), mark(clamp0(n, 1.0))
    assert denoiser == DENOISER_NRD_RELAX
    a = np.asarray(a, np.float32)
    return sanitize(rgb), mark(np.where(np.isfinite(a), clamp0(a, FP16_MAX), F32(0.0)))


def pack_texture(denoiser, noisy, albedo, z, P, r):
    """One texture of the pack: uint16 (..., 4) -> uint16 (..., 4), every pixel (the depth mask is applied by pack())."""
    q, al = f16_to_f32(noisy), f16_to_f32(albedo)
    with np.errstate(all="ignore"):
        rgb = (q[..., :3] / al[..., :3]).astype(np.float32)
    out = np.empty(noisy.shape, np.uint16)
    if denoiser not in (DENOISER_NRD_REBLUR, DENOISER_NRD_RELAX):       # demodulation only; the alpha keeps its bits
        out[..., :3] = f32_to_f16(rgb)
        out[..., 3] = noisy[..., 3]
        return out
    c, a = pack_values(denoiser, rgb, q[..., 3], z, P, r)
    out[..., :3] = f32_to_f16(c)
    out[..., 3] = f32_to_f16(a)
    return out


def pack(denoiser, depth, diffuse_albedo, specular_albedo, normal_roughness, noisy_diffuse, noisy_specular, hit_distance=REBLUR_HIT_DISTANCE_DEFAULTS):
    """IsPack = 1: the new (NoisyDiffuse, NoisySpecular). A pixel whose depth is not finite keeps its bytes."""
    depth = np.asarray(depth, np.float32)
    live = np.isfinite(depth)[..., None]
    r = snorm16_to_f32(normal_roughness[..., 3]) if denoiser == DENOISER_NRD_REBLUR else np.zeros(depth.shape, np.float32)
    d = pack_texture(denoiser, noisy_diffuse, diffuse_albedo, depth, hit_distance, np.ones(depth.shape, np.float32))
    s = pack_texture(denoiser, noisy_specular, specular_albedo, depth, hit_distance, r)
    return np.where(live, d, noisy_diffuse).astype(np.uint16), np.where(live, s, noisy_specular).astype(np.uint16)


def unpack_texture(denoiser, denoised):
    c = f16_to_f32(denoised)[..., :3]
    return ycocg_to_rgb(c) if denoiser == DENOISER_NRD_REBLUR else c


def compose(denoiser, depth, diffuse_albedo, specular_albedo, denoised_diffuse, denoised_specular, radiance):
    """IsPack = 0: the new Radiance: rgb + (d * DiffuseAlbedo + s * SpecularAlbedo), the alpha keeps its bits."""
    live = np.isfinite(np.asarray(depth, np.float32))[..., None]
    d, s = unpack_texture(denoiser, denoised_diffuse), unpack_texture(denoiser, denoised_specular)
    da, sa = f16_to_f32(diffuse_albedo)[..., :3], f16_to_f32(specular_albedo)[..., :3]
    with np.errstate(all="ignore"):
        rgb = f16_to_f32(radiance)[..., :3] + (d * da + s * sa)
    out = np.array(radiance, np.uint16)
    out[..., :3] = f32_to_f16(rgb)
    return np.where(live, out, radiance).astype(np.uint16)


def ulp16(x):
    """the spacing of the fp16 grid at |x| (float64): 2^-24 in the subnormal range"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15) - 10)
