"""Float64 reference of texture sampling, material evaluation and environment lookup (numpy only).

Restated from the reference's HLSL and the D3D sampling rules, independently of csrc/pt_texture.hpp and
oracle/pt_oracle.c, so that a mistake the GPU code and the oracle share does not pass unseen:

  Sample<T> / SampleLevel(s0, uv, 0)       Shaders/ShadingHelpers.hlsli:53-59; the root signature's default static
                                           sampler (Shaders/Raytracing.hlsl:79): WRAP addressing, mip 0, bilinear
  GetEnvironmentLightColor                 Shaders/ShadingHelpers.hlsli:11-30
  Math::ToLatLongCoordinate                Shaders/Math.hlsli:29-33
  EvaluateBaseColor / EvaluateTransmission Shaders/ShadingHelpers.hlsli:61-87
  PerturbNormal, Math::CalculateTBN        Shaders/ShadingHelpers.hlsli:89-103, Shaders/Math.hlsli:17-21
  IsOpaque (both overloads)                Shaders/ShadingHelpers.hlsli:105-159
  EvaluateMaterial                         Shaders/ShadingHelpers.hlsli:161-235
  GeneratePinholeRay, CalculateUV / NDC    Shaders/Camera.hlsli:27-41, Shaders/Math.hlsli:7-15

A `Reference` carries switches that deliberately break one rule each (``MUTATIONS``); the tests use them to show
that their tolerances are tight enough to notice each such mistake.
"""
import math

import numpy as np

FMT_RGBA8, FMT_RGBA8_SRGB, FMT_RGBA32F = 0, 1, 2
SLOTS = ["BaseColor", "EmissiveColor", "Metallic", "Roughness", "MetallicRoughness", "Transmission", "Normal"]
MIN_ROUGHNESS = 2e-3                      # BxDF.hlsli:19, applied by BSDFSample before the G-buffer store

MUTATIONS = ("no_half_texel", "clamp_uv", "srgb_alpha", "swap_mr_channels", "ignore_uv_index", "swap_wh",
             "flip_cube_face_sc", "cutoff_gt", "cube_clamp")


def srgb_to_linear(c):
    """IEC 61966-2-1 piecewise sRGB decode, float64."""
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def f16_values(h):
    """Values of fp16 storage as float64."""
    return np.asarray(h, np.float16).astype(np.float64)


def snorm16_values(q):
    """R16_SNORM decode (D3D: -32768 and -32767 both map to -1)."""
    return np.maximum(np.asarray(q, np.float64) / 32767.0, -1.0)


class Reference:
    def __init__(self, **mutations):
        unknown = set(mutations) - set(MUTATIONS)
        assert not unknown, unknown
        self.m = {k: bool(mutations.get(k, False)) for k in MUTATIONS}

    # ------------------------------------------------------------------ texels
    def decode(self, data, fmt):
        """Texel decode of a [.., H, W, 4] array: UNORM8 c/255, *_SRGB on RGB only (alpha stays linear), RGBA32F as stored."""
        if fmt == FMT_RGBA32F:
            return np.asarray(data, np.float64)
        x = np.asarray(data, np.float64) / 255.0
        if fmt == FMT_RGBA8_SRGB:
            x = x.copy()
            n = 4 if self.m["srgb_alpha"] else 3
            x[..., :n] = srgb_to_linear(x[..., :n])
        return x

    # ------------------------------------------------------------------ Texture2D
    def sample2d(self, tex, u, v):
        """Texture2D.SampleLevel(s0, uv, 0): bilinear at uv * size - 0.5, exact weights, both taps wrapped modulo the size.

        tex: decoded [H, W, 4]; u, v: arrays. [repo choice, DESIGN "Arithmetic spec"] NaN or infinite coordinates sample at 0."""
        H, W = tex.shape[0], tex.shape[1]
        if self.m["swap_wh"]:
            W, H = H, W
        u = np.where(np.isfinite(u), np.asarray(u, np.float64), 0.0)
        v = np.where(np.isfinite(v), np.asarray(v, np.float64), 0.0)
        half = 0.0 if self.m["no_half_texel"] else 0.5
        if self.m["clamp_uv"]:
            u, v = np.clip(u, 0.0, 1.0), np.clip(v, 0.0, 1.0)
        fx, fy = u * W - half, v * H - half
        x0, y0 = np.floor(fx), np.floor(fy)
        wx, wy = (fx - x0)[..., None], (fy - y0)[..., None]
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        if self.m["clamp_uv"]:
            xs = [np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)]; ys = [np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)]
        else:
            xs = [np.mod(x0, W), np.mod(x0 + 1, W)]; ys = [np.mod(y0, H), np.mod(y0 + 1, H)]
        if self.m["swap_wh"]:                     # index the texel array as if rows were columns
            flat = tex.reshape(-1, 4)
            fetch = lambda y, x: flat[(y * W + x) % flat.shape[0]]
        else:
            fetch = lambda y, x: tex[y, x]
        c00, c10, c01, c11 = fetch(ys[0], xs[0]), fetch(ys[0], xs[1]), fetch(ys[1], xs[0]), fetch(ys[1], xs[1])
        return (c00 * (1 - wx) + c10 * wx) * (1 - wy) + (c01 * (1 - wx) + c11 * wx) * wy

    def footprint2d(self, tex, u, v):
        """Largest difference between two neighbouring texels of the 2x2 footprint (per sample, over channels)."""
        H, W = tex.shape[0], tex.shape[1]
        u = np.where(np.isfinite(u), np.asarray(u, np.float64), 0.0)
        v = np.where(np.isfinite(v), np.asarray(v, np.float64), 0.0)
        x0 = np.floor(u * W - 0.5).astype(np.int64); y0 = np.floor(v * H - 0.5).astype(np.int64)
        xs = [np.mod(x0 - 1 + k, W) for k in range(4)]; ys = [np.mod(y0 - 1 + k, H) for k in range(4)]
        # a 4x4 neighbourhood: the fp32 position may fall one texel beside the float64 one
        c = np.stack([np.stack([tex[ys[j], xs[i]] for i in range(4)], -2) for j in range(4)], -3)   # [..., 4, 4, ch]
        d = np.maximum(np.abs(np.diff(c, axis=-2)).max((-1, -2, -3)), np.abs(np.diff(c, axis=-3)).max((-1, -2, -3)))
        return d, np.abs(c).max((-1, -2, -3))

    # ------------------------------------------------------------------ TextureCube
    # D3D major-axis table, faces +X, -X, +Y, -Y, +Z, -Z: (major axis, sign, sc = s_sign * d[s_axis], tc = t_sign * d[t_axis])
    CUBE = [(0, +1, (2, -1), (1, -1)), (0, -1, (2, +1), (1, -1)), (1, +1, (0, +1), (2, +1)),
            (1, -1, (0, +1), (2, -1)), (2, +1, (0, +1), (1, -1)), (2, -1, (0, -1), (1, -1))]

    def cube_face(self, d):
        """Face and (sc, tc, ma) per direction. [repo choice] ties go to X, then Y (the tests avoid exact ties)."""
        d = np.asarray(d, np.float64)
        a = np.abs(d)
        axis = np.where((a[..., 0] >= a[..., 1]) & (a[..., 0] >= a[..., 2]), 0, np.where(a[..., 1] >= a[..., 2], 1, 2))
        comp = np.take_along_axis(d, axis[..., None], -1)[..., 0]
        face = 2 * axis + (comp < 0)
        sc = np.zeros(d.shape[:-1]); tc = np.zeros(d.shape[:-1])
        for f, (_, _, (sa, ss), (ta, ts)) in enumerate(self.CUBE):
            sel = face == f
            s_sign = -ss if (self.m["flip_cube_face_sc"] and f == 4) else ss
            sc = np.where(sel, s_sign * d[..., sa], sc); tc = np.where(sel, ts * d[..., ta], tc)
        return face, sc, tc, np.abs(comp)

    def _cube_texel(self, tex, face, S, T):
        """Texel whose centre is nearest to face-local point (1, S, T) on the cube [-1, 1]^3, folding a point that lies past
        an edge of the face onto the adjacent face (rotation about the shared edge) -- seamless cube addressing."""
        N = tex.shape[1]
        p = np.zeros(S.shape + (3,))
        major = np.ones(S.shape)
        outS, outT = np.abs(S) > 1, np.abs(T) > 1
        # fold: the distance past the edge becomes distance from the edge into the adjacent face
        major = np.where(outS, 1 - (np.abs(S) - 1), np.where(outT, 1 - (np.abs(T) - 1), major))
        S = np.where(outS, np.sign(S), S); T = np.where(outT, np.sign(T), T)
        for f, (ma, ms, (sa, ss), (ta, ts)) in enumerate(self.CUBE):
            sel = (face == f)[..., None]
            q = np.zeros(S.shape + (3,))
            q[..., ma] = ms * major; q[..., sa] = ss * S; q[..., ta] = ts * T
            p = np.where(sel, q, p)
        f2, sc, tc, m = Reference().cube_face(p)     # the point is strictly inside one face: no mutation applies here
        x = np.clip(np.floor((sc / m + 1) / 2 * N), 0, N - 1).astype(np.int64)
        y = np.clip(np.floor((tc / m + 1) / 2 * N), 0, N - 1).astype(np.int64)
        return tex[f2, y, x]

    def sample_cube(self, tex, d):
        """TextureCube.SampleLevel(s0, d, 0), bilinear on the selected face, seamless: a tap past a face edge comes from the
        adjacent face, and at a cube corner the missing tap is the mean of the three texels meeting there.
        tex: decoded [6, N, N, 4]."""
        N = tex.shape[1]
        face, sc, tc, ma = self.cube_face(d)
        u, v = (sc / ma + 1) / 2, (tc / ma + 1) / 2
        fx, fy = u * N - 0.5, v * N - 0.5
        x0, y0 = np.floor(fx), np.floor(fy)
        wx, wy = (fx - x0)[..., None], (fy - y0)[..., None]
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        taps = {}
        for dy in (0, 1):
            for dx in (0, 1):
                x, y = x0 + dx, y0 + dy
                if self.m["cube_clamp"]:
                    taps[dx, dy] = tex[face, np.clip(y, 0, N - 1), np.clip(x, 0, N - 1)]
                    continue
                S = (2 * x + 1) / N - 1.0; T = (2 * y + 1) / N - 1.0          # texel centre, face-local
                corner = (np.abs(S) > 1) & (np.abs(T) > 1)
                S1 = np.where(corner, np.clip(S, -1 + 1.0 / N, 1 - 1.0 / N), S)   # placeholder tap for corners, replaced below
                taps[dx, dy] = (self._cube_texel(tex, face, S1, T), corner)
        if not self.m["cube_clamp"]:
            vals = {k: t[0] for k, t in taps.items()}
            for k, (_, corner) in taps.items():
                others = [vals[j] for j in vals if j != k]
                vals[k] = np.where(corner[..., None], (others[0] + others[1] + others[2]) / 3.0, vals[k])
            taps = vals
        return (taps[0, 0] * (1 - wx) + taps[1, 0] * wx) * (1 - wy) + (taps[0, 1] * (1 - wx) + taps[1, 1] * wx) * wy

    def cube_footprint(self, tex, d):
        """Largest texel difference anywhere near the sample (its face plus neighbours): a bound for tolerance use."""
        return np.full(np.asarray(d).shape[:-1], np.ptp(tex)), np.full(np.asarray(d).shape[:-1], np.abs(tex).max())

    # ------------------------------------------------------------------ environment
    def environment(self, sd, env_tex, env_fmt, dirs):
        """GetEnvironmentLightColor. RotateVector comes from the absent MathLib; the repo documents it as mul(M, v)
        (SURVEY.md Appendix B), i.e. row i of the 3x4 EnvironmentLightTransform dotted with the direction."""
        dirs = np.asarray(dirs, np.float64)
        if int(sd["EnvironmentLightTextureDescriptor"]) != 0xFFFFFFFF:
            M = np.asarray(sd["EnvironmentLightTransform"], np.float64).reshape(3, 4)[:, :3]
            w = dirs @ M.T
            w /= np.linalg.norm(w, axis=-1, keepdims=True)
            tex = self.decode(env_tex, env_fmt)
            if int(sd["IsEnvironmentLightTextureCubeMap"]):
                return self.sample_cube(tex, w)[..., :3]
            u = (1 + np.arctan2(w[..., 0], w[..., 2]) / math.pi) / 2
            v = np.arccos(np.clip(w[..., 1], -1, 1)) / math.pi
            return self.sample2d(tex, u, v)[..., :3]
        c = np.asarray(sd["EnvironmentLightColor"], np.float64)
        if c[3] >= 0:
            return np.broadcast_to(c[:3], dirs.shape).copy()
        t = (dirs[..., 1:2] + 1) * 0.5                                  # lerp(1, (0.5, 0.7, 1), t), then Color::FromSrgb
        return srgb_to_linear(1 + t * (np.array([0.5, 0.7, 1.0]) - 1))

    # ------------------------------------------------------------------ materials
    def _tap(self, textures, slot, uv):
        data, fmt, index = textures[slot]
        if self.m["ignore_uv_index"]:
            index = 0
        return self.sample2d(self.decode(data, fmt), uv[index][0], uv[index][1])

    def evaluate_material(self, mat, textures, uv, N=None, T=None):
        """EvaluateMaterial for arrays of hit points. mat: a MATERIAL record; textures: slot -> (texel data, fmt, uv index);
        uv: [2][2] arrays; N, T: [..., 3] front shading normal and front tangent (or None). Returns a dict of float64 arrays."""
        shape = np.shape(uv[0][0])
        bc = np.broadcast_to(np.asarray(mat["BaseColor"], np.float64), shape + (4,)).copy()
        em = np.broadcast_to(np.asarray(mat["EmissiveColor"], np.float64), shape + (3,)).copy()
        metal = np.full(shape, float(mat["Metallic"])); rough = np.full(shape, float(mat["Roughness"]))
        trans = np.full(shape, float(mat["Transmission"]))
        if (np.asarray(mat["BaseColor"]) > 0).any() and "BaseColor" in textures:          # any(baseColor > 0)
            bc = bc * self._tap(textures, "BaseColor", uv)
        if (np.asarray(mat["EmissiveColor"], np.float64) * float(mat["EmissiveStrength"]) > 0).any() and "EmissiveColor" in textures:
            em = em * self._tap(textures, "EmissiveColor", uv)[..., :3]
        if "MetallicRoughness" in textures:
            if mat["Metallic"] > 0 or mat["Roughness"] > 0:
                t = self._tap(textures, "MetallicRoughness", uv)
                mb, rg = (1, 2) if self.m["swap_mr_channels"] else (2, 1)    # metallic .b, roughness .g
                metal = metal * t[..., mb]; rough = rough * t[..., rg]
        else:
            if mat["Metallic"] > 0 and "Metallic" in textures:
                metal = metal * self._tap(textures, "Metallic", uv)[..., 0]
            if mat["Roughness"] > 0 and "Roughness" in textures:
                rough = rough * self._tap(textures, "Roughness", uv)[..., 0]
        if mat["Transmission"] > 0 and "Transmission" in textures:                 # only where Metallic < 1
            trans = np.where(metal < 1, trans * self._tap(textures, "Transmission", uv)[..., 0], trans)
        out = {"BaseColor": bc, "Emission": em * float(mat["EmissiveStrength"]), "Metallic": metal, "Roughness": rough,
               "Transmission": trans, "IOR": np.full(shape, float(mat["IOR"]))}
        if N is not None:
            N = np.asarray(N, np.float64)
            if T is not None and "Normal" in textures and (np.abs(T) > 0).any():
                t = self._tap(textures, "Normal", uv)
                n = np.stack([t[..., 0] * 2 - 1, t[..., 1] * 2 - 1], -1)               # Geometry::UnpackLocalNormal (repo spec)
                nz = np.sqrt(np.clip(1 - (n * n).sum(-1), 0, 1))
                Tn = T - N * (N * T).sum(-1, keepdims=True)
                Tn /= np.linalg.norm(Tn, axis=-1, keepdims=True)
                B = np.cross(N, Tn)
                r = Tn * n[..., :1] + B * n[..., 1:] + N * nz[..., None]            # RotateVectorInverse(TBN, n) = transpose(TBN) n
                N = r / np.linalg.norm(r, axis=-1, keepdims=True)
            out["Normal"] = N
        return out

    def is_opaque(self, mat, textures, uv):
        """IsOpaque (closest-hit overload): BaseColor.a >= AlphaCutoff. Returns (opaque, alpha)."""
        a = self.evaluate_base_alpha(mat, textures, uv)
        cut = float(mat["AlphaCutoff"])
        return (a > cut if self.m["cutoff_gt"] else a >= cut), a

    def evaluate_base_alpha(self, mat, textures, uv):
        shape = np.shape(uv[0][0])
        a = np.full(shape, float(mat["BaseColor"][3]))
        if (np.asarray(mat["BaseColor"]) > 0).any() and "BaseColor" in textures:
            a = a * self._tap(textures, "BaseColor", uv)[..., 3]
        return a

    def is_opaque_visibility(self, mat, textures, uv, vis):
        """IsOpaque with coloured visibility (direct-lighting overload). Returns (blocks, visibility, alpha, metallic)."""
        shape = np.shape(uv[0][0])
        bc = np.broadcast_to(np.asarray(mat["BaseColor"], np.float64), shape + (4,)).copy()
        if (np.asarray(mat["BaseColor"]) > 0).any() and "BaseColor" in textures:
            bc = bc * self._tap(textures, "BaseColor", uv)
        vis = np.broadcast_to(np.asarray(vis, np.float64), shape + (3,)).copy()
        metal = np.full(shape, float(mat["Metallic"]))
        if int(mat["AlphaMode"]) != 0:
            cut = float(mat["AlphaCutoff"])
            ret = bc[..., 3] > cut if self.m["cutoff_gt"] else bc[..., 3] >= cut
            return ret, vis * (~ret)[..., None], bc[..., 3], metal
        if mat["Metallic"] > 0:
            if "MetallicRoughness" in textures:
                metal = metal * self._tap(textures, "MetallicRoughness", uv)[..., 1 if self.m["swap_mr_channels"] else 2]
            elif "Metallic" in textures:
                metal = metal * self._tap(textures, "Metallic", uv)[..., 0]
        full_metal = metal == 1
        trans = np.full(shape, float(mat["Transmission"]))
        if mat["Transmission"] > 0 and "Transmission" in textures:
            trans = trans * self._tap(textures, "Transmission", uv)[..., 0]
        vis = vis * ((1 - metal) * trans)[..., None] * bc[..., :3]
        vis = np.where(full_metal[..., None], 0.0, vis)
        return full_metal | (vis == 0).all(-1), vis, bc[..., 3], metal


# ---------------------------------------------------------------------- geometry of closed-form scenes
def pinhole_rays(cam, W, H):
    """GeneratePinholeRay for every pixel, float64 from the fp32 camera: origin [3], directions [H, W, 3]."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    j = np.asarray(cam["Jitter"], np.float64)
    u, v = (x + 0.5 + j[0]) / W, (y + 0.5 + j[1]) / H
    nx, ny = u * 2 - 1, v * -2 + 1
    R, U, F = (np.asarray(cam[k], np.float64) for k in ("RightDirection", "UpDirection", "ForwardDirection"))
    d = nx[..., None] * R + ny[..., None] * U + F
    return np.asarray(cam["Position"], np.float64), d / np.linalg.norm(d, axis=-1, keepdims=True)


def ray_triangle(o, d, p0, p1, p2):
    """Analytic ray/triangle hit: t and DXR barycentrics (b1 weights p1, b2 weights p2), float64 (NaN t where missed)."""
    e1, e2 = p1 - p0, p2 - p0
    n = np.cross(e1, e2)
    den = (d * n).sum(-1)
    t = ((p0 - o) @ n) / den
    q = o + d * t[..., None] - p0
    # solve q = b1 e1 + b2 e2 in the plane
    g = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
    rhs = np.stack([(q * e1).sum(-1), (q * e2).sum(-1)], -1)
    b = rhs @ np.linalg.inv(g).T
    return t, b[..., 0], b[..., 1]


def quad_hits(o, d, vertices, indices):
    """Closed-form hit of a ray bundle with a planar two-triangle mesh: per ray (hit, t, triangle index, b1, b2, edge
    distance in barycentric units -- how far the hit lies inside its triangle's boundary, the diagonal excluded)."""
    pos = np.asarray(vertices["Position"], np.float64)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    best = None
    for k, (i0, i1, i2) in enumerate(idx):
        t, b1, b2 = ray_triangle(o, d, pos[i0], pos[i1], pos[i2])
        b0 = 1 - b1 - b2
        inside = (t > 0) & (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
        if best is None:
            best = dict(hit=inside, t=np.where(inside, t, np.nan), tri=np.where(inside, k, -1), b1=b1, b2=b2,
                        bmin=np.minimum(np.minimum(b0, b1), b2))
        else:
            take = inside & ~best["hit"]
            best["hit"] |= inside
            best["t"] = np.where(take, t, best["t"]); best["tri"] = np.where(take, k, best["tri"])
            best["b1"] = np.where(take, b1, best["b1"]); best["b2"] = np.where(take, b2, best["b2"])
            best["bmin"] = np.where(take, np.minimum(np.minimum(b0, b1), b2), best["bmin"])
    return best


def interpolate_attribute(vals, idx, tri, b1, b2):
    """Vertex::Interpolate over the triangle each ray hit: a0 + b1 (a1 - a0) + b2 (a2 - a0), in float64."""
    tri = np.maximum(tri, 0)
    i = np.asarray(idx, np.int64).reshape(-1, 3)[tri]
    a0, a1, a2 = vals[i[..., 0]], vals[i[..., 1]], vals[i[..., 2]]
    return a0 + b1[..., None] * (a1 - a0) + b2[..., None] * (a2 - a0)


def hit_attributes(vertices, indices, hits, dirs):
    """UV sets from the fp16 values actually stored, geometric normal and tangent from their snorm16 encodings (identity
    instance transform), front-face flip (HitInfo.hlsli): returns uv [2][2], front shading normal, front tangent, is_front."""
    tri, b1, b2 = hits["tri"], hits["b1"], hits["b2"]
    uv = []
    for key in ("TexCoord0", "TexCoord1"):
        a = interpolate_attribute(f16_values(vertices[key]), indices, tri, b1, b2)
        uv.append([a[..., 0], a[..., 1]])
    n = interpolate_attribute(snorm16_values(vertices["Normal"]), indices, tri, b1, b2)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    t = interpolate_attribute(snorm16_values(vertices["Tangent"]), indices, tri, b1, b2)
    tl = np.linalg.norm(t, axis=-1, keepdims=True)
    t = np.where(tl > 0, t / np.where(tl > 0, tl, 1), 0.0)
    front = (n * dirs).sum(-1) < 0
    s = np.where(front, 1.0, -1.0)[..., None]
    return uv, n * s, t * s, front


# ---------------------------------------------------------------------- tolerances
def texel_position_error(size, uv_mag):
    """Bound on the fp32 pipeline's error of a sample position, in texels.

    A UV of magnitude |uv| reaches the sampler with a relative error of a few fp32 ulps (barycentric interpolation, the
    ray/triangle test, atan2/acos for lat-long), i.e. an absolute error of about (|uv| + 1) * 2^-22 in UV units -- the +1
    covers values near zero, whose error is set by the operands, not the result. Scaled by the texture size and with a
    4x margin: size * (|uv| + 1) * 2^-20 texels."""
    return np.asarray(size, np.float64) * (np.abs(uv_mag) + 1.0) * 2.0 ** -20


def value_tolerance(pos_err_texels, neighbour_diff, magnitude, ulps=8):
    """A bilinear sample moves by at most (position error) x (largest neighbour difference of its footprint texels);
    the two fp32 lerp levels, the weights and the texel decode add a few ulps of the value's magnitude."""
    return pos_err_texels * neighbour_diff + ulps * 2.0 ** -24 * np.maximum(magnitude, 2.0 ** -10)


def unorm8_codes(x):
    return np.floor(np.clip(x, 0, 1) * 255 + 0.5)


def snorm16_codes(x):
    v = np.clip(x, -1, 1) * 32767
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def codes_agree(got, ref_value, tol, kind):
    """Quantised outputs compare as codes: exact, except where the float64 value lies within `tol` of a rounding boundary,
    where one code either way is allowed. kind: 'unorm8', 'snorm16' or 'f16'. Returns a boolean array."""
    got = np.asarray(got); ref_value = np.asarray(ref_value, np.float64); tol = np.broadcast_to(tol, ref_value.shape)
    if kind == "f16":
        g = got.view(np.float16).astype(np.float64) if got.dtype == np.uint16 else got.astype(np.float64)
        lo = (ref_value - tol).astype(np.float16).astype(np.float64)
        hi = (ref_value + tol).astype(np.float16).astype(np.float64)
        return (g >= np.minimum(lo, hi)) & (g <= np.maximum(lo, hi))
    enc, scale = (unorm8_codes, 255.0) if kind == "unorm8" else (snorm16_codes, 32767.0)
    g = got.astype(np.float64)
    return (g >= enc(ref_value - tol)) & (g <= enc(ref_value + tol))
