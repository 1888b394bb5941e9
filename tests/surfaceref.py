"""Float64 reference of the primary surface: camera ray, closest hit, hit reconstruction, normals, depths, motion vector, material
words and every pack of the G-buffer pass (numpy only).

Restated from Shaders/Camera.hlsli, Math.hlsli (CalculateUV / CalculateNDC), HitInfo.hlsli, SelfIntersectionAvoidance.hlsli,
RaytracingHelpers.hlsli (CastRay), GBufferGeneration.hlsl and Packing.hlsli, and from the published definitions of the MathLib functions
they call (ProjectiveTransform / AffineTransform = the matrix times (p, 1); GetScreenUv = clip.xy / clip.w * (0.5, -0.5) + 0.5; the signed
octahedral EncodeUnitVector), independently of csrc/ and oracle/pt_oracle.c. Matrix conventions follow from the declarations alone: the
3x4 transforms are `row_major` (M (p, 1)); the camera's float4x4 are default (column-major) cbuffer members filled from row-major
memory, which makes mul(m, (p, 1)) the row-vector product (p, 1) A of the stored array A.

The closest hit is brute force over WORLD-space triangles (float64 Moller-Trumbore); the barycentrics of a hit are affine invariants, so
they are the object-space ones the shader receives. WorldToObject is the float64 inverse of the fp32 ObjectToWorld.

`unsafe` pixels -- where fp32 may legitimately decide otherwise than exact geometry:
  * edge: the closest hit, or a triangle that is not hit but could be taken instead (t up to the closest t), lies within
    EDGE_B + 8 * 2^-24 * S_o / h of an edge in barycentric units. EDGE_B = 1e-5 covers isectref's bound on u, v ((24 rho + 4) 2^-24 cond,
    rho ~ 4/3, cond up to 5); the second term is what isectref's classification sees and a world-space evaluation does not: the ray enters
    the instance through an fp32 transform whose origin carries 4 roundings of S_o = sum |W_ij o_j| + |W_i3| (object units), against
    the triangle's smallest altitude h.
  * depth: a second triangle is hit within DEPTH_GAP = 1e-4 relative of the closest t, or the closest t lies that close to TMin / TMax.
  * perpendicular: |dot(geometric normal, ray direction)| < PERP = 1e-4 (the front-face decision; an fp32 dot product of unit vectors
    carries a few 2^-24).

Tolerances, from the formats (never from an implementation):
  snorm16   one step 1 / 32767 (octahedral normals compared in encoded space)      unorm8   one step 1 / 255
  f16       one ulp of the stored value, plus what is stated per texture:
    MotionVector.xy   (su - u) W keeps the ABSOLUTE error of its O(1) operands: MV_ROUNDINGS * 2^-24 * (1 + A) * W, with
                      A = (sum |p_i M_i0| + |M_30| + |su'| (sum |p_i M_i3| + |M_33|)) / |clip.w| the cancellation of the projection's
                      dot products at that pixel and MV_ROUNDINGS = 8 (four terms of each dot product, the division, the final
                      multiply-add, u's own two), plus the fp32 position's own error (below) seen through the projection.
    MotionVector.z    the same with the view-space and projection rows: both operands are depths.
    albedos           B.REL of the value (the rational fit of EnvironmentTerm_Rtg, the project's own figure for lobe weights).
  LinearDepth / NormalizedDepth   four roundings of sum |terms| plus the position's error through the row; z / w by the quotient rule.
  Position.w        OFFSET_ROUNDINGS = 32 roundings relative: the offset is a sum of positive terms.
  Position.xyz      (1) its distance to the exact triangle plane is <= its own PositionOffset: the algorithm's claim, no number chosen.
                    (2) its in-plane error is <= K_POSITION * 2^-24 * (|origin| + t).
                    K_POSITION = 100 = 4 x the largest ratio measured on the CPU oracle against this reference: 25.3 on
                    `depth_infinite` (18.7 on `depth_far50`; both on the 40 x 200 floor, whose barycentric error is worth the most
                    length), 9.4 on `transformed` and `moved`, 0.8 / 1.9 on the two `scale` cameras. The factor leaves room for another
                    evaluation order on the device, not for another algorithm: at distance 7 the limit is 4e-5.

Textured hits (RaytracingHelpers.hlsli:19-44 and :113-130, ShadingHelpers.hlsli:32-51 and :105-235, HitInfo.hlsli:85-88, sampled through
tests/texref.py): Triangles carries both UV sets per corner, decoded from f16 (an absent set reads 0); reconstruct() interpolates them and
hands the tangent on negated on a back face; closest() puts EVERY candidate of a geometry without the OPAQUE flag to the closest-hit
IsOpaque (BaseColor.a x the texture's alpha >= AlphaCutoff) at the candidate's own UVs; Surface.material() is EvaluateMaterial with the
perturbed shading normal, Surface.environment() the lat-long or cube lookup under EnvironmentLightTransform. render() uses them all. The
bound of a tap (Surface.tap_bound) and what decisions count as undecided are stated in tests/pathref.py's docstring; in the G-buffer
comparison the bound of each stored quantity is added to its format's step (the albedos: by finite differences of the rational fit).

Every switch of `MUTATIONS` breaks one rule; tests/test_gbuffer_reference.py and, for TEXTURE_MUTATIONS, tests/test_textured_estimator.py
show that the comparison notices each. `transmission_gate_on_factor` stands for "the Transmission texture applied at Metallic == 1": taken
literally that mistake leaves no trace (GBufferGeneration.hlsl:191-195 stores Transmission only where Metallic < 1, and the transmission
lobe's weight is Transmission (1 - Metallic)), so the switch breaks the observable half of the same rule -- the gate reads the Metallic
FACTOR instead of the textured value (ShadingHelpers.hlsli:213-220 tests it after the Metallic tap).
"""
import numpy as np

import bsdfref as B
import texref

EPS = 2.0 ** -24
EDGE_B = 1e-5
DEPTH_GAP = 1e-4
PERP = 1e-4
MV_ROUNDINGS = 8.0
OFFSET_ROUNDINGS = 32.0
K_POSITION = 100.0
SNORM16, UNORM8 = 1.0 / 32767.0, 1.0 / 255.0
TEXTURE_MUTATIONS = ("uv_corner0", "alpha_ignores_opaque_flag", "alpha_geometry0", "tangent_no_back_flip", "normal_map_ignored",
                     "normal_map_without_tangents", "emissive_texture_ignored", "transmission_gate_on_factor", "env_no_transform", "env_transposed")
MUTATIONS = ("normal_by_matrix", "no_front_flip", "mv_current_camera", "mv_no_vertex_term", "v_not_flipped") + TEXTURE_MUTATIONS
POLE = 1e-4                                          # sin of the angle to the lat-long poles below which atan2 / the NaN rule decide

f64 = np.float64
_TRUE = texref.Reference()                           # tolerances come from the unmutated sampler


def dot(a, b):
    return np.einsum("...i,...i->...", a, b)


def normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def f16(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(f64)


def ulp16(x):
    """the spacing of binary16 at |x| (at the largest finite value beyond it)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.spacing(np.minimum(np.abs(np.nan_to_num(x, posinf=65504.0, neginf=65504.0)), 65504.0).astype(np.float16)).astype(f64)


def f16_close(bits, ref, extra=0.0):
    """a stored binary16 against a float64 value: one ulp plus `extra`; past the format's range only the infinity of that sign"""
    got = f16(bits)
    tol = ulp16(ref) + extra
    with np.errstate(invalid="ignore"):
        return (np.abs(got - ref) <= tol) | (np.isinf(got) & (np.sign(got) == np.sign(ref)) & (np.abs(ref) + tol >= 65520.0))


def unpack_snorm16(v):                               # Packing.hlsli Unpack_R16_SNORM
    return np.maximum(np.asarray(v, np.int16).astype(f64) / 32767.0, -1.0)


def oct_encode(n):
    """signed octahedral EncodeUnitVector: project to |x| + |y| + |z| = 1, fold the lower half over the diagonals"""
    n = n / np.abs(n).sum(-1, keepdims=True)
    sgn = np.where(n[..., :2] >= 0, 1.0, -1.0)
    wrap = (1.0 - np.abs(n[..., 1::-1])) * sgn
    return np.where(n[..., 2:3] >= 0, n[..., :2], wrap)


def oct_decode(e):
    z = 1.0 - np.abs(e[..., 0]) - np.abs(e[..., 1])
    t = np.clip(-z, 0.0, 1.0)[..., None]
    xy = e - t * np.where(e >= 0, 1.0, -1.0)
    return normalize(np.concatenate([xy, z[..., None]], -1))


def pixel_uv(W, H, jitter, rows=None):
    """Math::CalculateUV for the pixels of rows [y0, y1) (the whole frame by default): [n, 2] and the pixel coordinates"""
    y0, y1 = rows if rows is not None else (0, H)
    py, px = np.mgrid[y0:y1, 0:W]
    pix = np.stack([px.reshape(-1), py.reshape(-1)], -1).astype(f64)
    return (pix + 0.5 + np.asarray(jitter, f64)) / np.array([W, H], f64), pix


def pinhole(cam, uv):
    """Camera::GeneratePinholeRay of Math::CalculateNDC(uv): origin, unit direction, TMin, TMax"""
    ndc = uv * np.array([2.0, -2.0]) + np.array([-1.0, 1.0])
    R, U, F = (np.asarray(cam[k], f64) for k in ("RightDirection", "UpDirection", "ForwardDirection"))
    d = normalize(ndc[:, 0:1] * R + ndc[:, 1:2] * U + F)
    inv_cos = 1.0 / dot(normalize(F), d)
    o = np.broadcast_to(np.asarray(cam["Position"], f64), d.shape)
    with np.errstate(invalid="ignore"):
        return o, d, float(cam["NearDepth"]) * inv_cos, float(cam["FarDepth"]) * inv_cos


def row_vector(A, p):
    """(p, 1) A of a stored float4x4: ProjectiveTransform / AffineTransform with a camera matrix; also sum |terms| per column"""
    A = np.asarray(A, f64)
    return p @ A[:3] + A[3], np.abs(p) @ np.abs(A[:3]) + np.abs(A[3])


class Triangles:
    """The visible triangles of a finalized scenes.Scene, flattened: world- and object-space corners and the per-corner attributes."""

    def __init__(self, scene):
        self.scene = scene
        n_inst = len(scene.objects)
        self.o2w = np.asarray(scene.instance_data["ObjectToWorld"], f64).reshape(n_inst, 3, 4)
        self.prev_o2w = np.asarray(scene.instance_data["PreviousObjectToWorld"], f64).reshape(n_inst, 3, 4)
        self.w2o = np.zeros_like(self.o2w)
        for i in range(n_inst):
            inv = np.linalg.inv(self.o2w[i, :, :3])
            self.w2o[i, :, :3] = inv
            self.w2o[i, :, 3] = -inv @ self.o2w[i, :, 3]
        cols = {k: [] for k in ("obj", "nrm", "tan", "mot", "has_n", "has_t", "inst", "geom", "prim", "object", "uv0", "uv1", "has_uv0", "has_uv1",
                                "opaque", "object0")}
        for i in range(n_inst):
            if not int(scene.instance_masks[i]):
                continue                                                   # InstanceMask 0: no ray sees it
            first, count = scene.blas[int(scene.instance_blas[i])]
            for g in range(count):
                mesh = scene.geometry[first + g][0]
                idx = np.asarray(mesh.indices).astype(np.int64).reshape(-1, 3)
                n = len(idx)
                cols["obj"].append(np.asarray(mesh.vertices["Position"], f64)[idx])
                cols["nrm"].append(unpack_snorm16(mesh.vertices["Normal"])[idx])
                cols["tan"].append(unpack_snorm16(mesh.vertices["Tangent"])[idx])
                mv = f16(mesh.motion_vectors)[:, :3] if mesh.motion_vectors is not None else np.zeros((len(mesh.vertices), 3))
                cols["mot"].append(mv[idx])
                cols["has_n"].append(np.full(n, bool(mesh.has_normals)))
                cols["has_t"].append(np.full(n, bool(mesh.has_tangents)))
                cols["inst"].append(np.full(n, i)); cols["geom"].append(np.full(n, g)); cols["prim"].append(np.arange(n))
                cols["object"].append(np.full(n, int(scene.instance_data[i]["FirstGeometryIndex"]) + g))
                cols["object0"].append(np.full(n, int(scene.instance_data[i]["FirstGeometryIndex"])))
                for k, key in enumerate(("TexCoord0", "TexCoord1")):                 # f16 storage; an absent set reads as 0
                    has = bool(mesh.has_uv[k])
                    cols[f"uv{k}"].append(np.asarray(mesh.vertices[key]).astype(f64)[idx] if has else np.zeros((n, 3, 2)))
                    cols[f"has_uv{k}"].append(np.full(n, has))
                # the bottom level's geometry flag (Scene.ixx:320-324): OPAQUE iff the mesh has no material or AlphaMode::Opaque
                cols["opaque"].append(np.full(n, mesh.material is None or int(mesh.material["AlphaMode"]) == 0))
        for k, v in cols.items():
            setattr(self, k, np.concatenate(v))
        M = self.o2w[self.inst]
        self.world = np.einsum("tij,tkj->tki", M[:, :, :3], self.obj) + M[:, None, :, 3]
        e1, e2 = self.obj[:, 1] - self.obj[:, 0], self.obj[:, 2] - self.obj[:, 0]
        longest = np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(e2 - e1, axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            self.altitude = np.linalg.norm(np.cross(e1, e2), axis=1) / longest          # the smallest one, object units
        w1, w2 = self.world[:, 1] - self.world[:, 0], self.world[:, 2] - self.world[:, 0]
        longest = np.maximum(np.maximum(np.linalg.norm(w1, axis=1), np.linalg.norm(w2, axis=1)), np.linalg.norm(w2 - w1, axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            self.altitude_world = np.linalg.norm(np.cross(w1, w2), axis=1) / longest
        self.uv = np.stack([self.uv0, self.uv1], 1)                                         # [T, set, corner, 2]
        self.uv_extent = np.abs(self.uv[:, :, 1:] - self.uv[:, :, :1]).sum(2).max(-1)       # [T, set]: |uv1 - uv0| + |uv2 - uv0|, larger axis
        self.uv_magnitude = np.abs(self.uv).max((2, 3))                                     # [T, set]

    def interpolate_uv(self, tri, u, v):
        """Vertex::Interpolate of both sets at hits (tri, u, v): [n, set, 2]"""
        c = self.uv[tri]
        return c[:, :, 0] + u[:, None, None] * (c[:, :, 1] - c[:, :, 0]) + v[:, None, None] * (c[:, :, 2] - c[:, :, 0])

    def closest(self, o, d, tmin, tmax, chunk=1 << 19, drift=None, alpha=None):
        """The exact closest hit of rays (float64 [n, 3], TMin / TMax [n] or scalars, both exclusive): hit, tri, u, v, t and `unsafe`
        (edge / depth of the module docstring). drift = (angle [n], shift [n]): the fp32 ray may lie that far off this one (radians about
        its origin, world units sideways); the edge margin of a pair widens by (angle |t| + shift) over the triangle's world altitude.
        alpha: the closest-hit alpha rule of RaytracingHelpers.hlsli:19-44 (Surface.alpha_rule): an object with `tested` (the triangles
        whose candidates are CANDIDATE_NON_OPAQUE_TRIANGLE) and __call__(tri, u, v, barycentric uncertainty) -> (commit, near the cutoff).
        EVERY candidate inside its triangle and the ray's interval is put to it, not the closest one alone; a candidate the rule cannot
        decide in fp32 that lies no further than the committed hit makes the ray unsafe."""
        n, T = len(o), len(self.world)
        tmin = np.broadcast_to(np.asarray(tmin, f64), (n,)); tmax = np.broadcast_to(np.asarray(tmax, f64), (n,))
        out = {"hit": np.zeros(n, bool), "tri": np.zeros(n, np.int64), "u": np.zeros(n), "v": np.zeros(n), "t": np.full(n, np.inf),
               "unsafe": np.zeros(n, bool), "bary": np.zeros(n), "rejected": np.zeros(n, np.int64)}
        V0, E1, E2 = self.world[:, 0], self.world[:, 1] - self.world[:, 0], self.world[:, 2] - self.world[:, 0]
        step = max(1, chunk // max(T, 1))
        W = self.w2o
        for r0 in range(0, n, step):
            sl = slice(r0, r0 + step)
            oo, dd = o[sl], d[sl]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                pvec = np.cross(dd[:, None, :], E2[None])
                det = dot(E1[None], pvec)
                tvec = oo[:, None, :] - V0[None]
                u = dot(tvec, pvec) / det
                qvec = np.cross(tvec, E1[None])
                v = dot(dd[:, None, :], qvec) / det
                t = dot(E2[None], qvec) / det
                b = np.minimum(np.minimum(u, v), 1.0 - u - v)
                # S_o per (ray, instance): the magnitude of the terms of the fp32 transform of the origin into the instance
                S = (np.einsum("pj,kij->pki", np.abs(oo), np.abs(W[:, :, :3])) + np.abs(W[None, :, :, 3])).max(-1)
                thr = EDGE_B + 8.0 * EPS * S[:, self.inst] / self.altitude[None]
                if drift is not None:
                    thr = thr + (drift[0][sl, None] * np.abs(t) + drift[1][sl, None]) / self.altitude_world[None]
                lo, hi = tmin[sl, None], tmax[sl, None]
                inside = (b >= 0) & (t > lo) & (t < hi)
                undecided, geometric = None, inside
                if alpha is not None and len(alpha.tested):
                    ri, ci = np.nonzero(inside[:, alpha.tested])
                    tj = alpha.tested[ci]
                    commit, close = alpha(tj, u[ri, tj], v[ri, tj], thr[ri, tj])
                    inside = inside.copy(); inside[ri[~commit], tj[~commit]] = False
                    np.add.at(out["rejected"], r0 + ri[~commit], 1)
                    undecided = (ri[close], tj[close])
                gap = DEPTH_GAP * np.abs(t)
                near = (b > -thr) & (t > lo - gap) & (t < hi + gap) & ~geometric
                tt = np.where(inside, t, np.inf)
                j = tt.argmin(1)
                rows = np.arange(len(oo))
                t1 = tt[rows, j]
                hit = np.isfinite(t1)
                limit = np.where(hit, t1 * (1.0 + DEPTH_GAP), np.inf)[:, None]
                steal = (near & (t < limit)).any(1)
                others = inside.copy(); others[rows, j] = False
                tie = (others & (t < limit)).any(1)
                edge = hit & (b[rows, j] < thr[rows, j])
                rng = hit & ((t1 - tmin[sl] < DEPTH_GAP * t1) | (tmax[sl] - t1 < DEPTH_GAP * t1))
                if undecided is not None and len(undecided[0]):
                    ri, tj = undecided
                    ri = ri[t[ri, tj] < limit[ri, 0]]
                    edge[ri] = True
            out["hit"][sl] = hit; out["tri"][sl] = j; out["t"][sl] = t1
            out["u"][sl] = np.where(hit, u[rows, j], 0.0); out["v"][sl] = np.where(hit, v[rows, j], 0.0)
            out["unsafe"][sl] = steal | tie | edge | rng
            out["bary"][sl] = thr[rows, j]
        return out


def object_textures(scene):
    """Per ObjectData record: (Material, slot -> (texel array, format, TextureCoordinateIndex)), read the way the shaders read them: the
    TextureMapInfoArray's descriptors into the heap. Block-compressed textures are not this reference's business (test_bc_*)."""
    out = []
    for od in scene.object_data:
        slots = {}
        for k, slot in enumerate(texref.SLOTS):
            info = od["TextureMapInfoArray"][k]
            if int(info["Descriptor"]) != 0xFFFFFFFF:
                item = scene.heap[int(info["Descriptor"])]
                assert item.fmt in (texref.FMT_RGBA8, texref.FMT_RGBA8_SRGB, texref.FMT_RGBA32F), item.fmt
                slots[slot] = (item.array, item.fmt, int(info["TextureCoordinateIndex"]))
        out.append((od["Material"], slots))
    return out


class AlphaRule:
    """The closest-hit alpha rule as Triangles.closest consumes it (RaytracingHelpers.hlsli:19-44, ShadingHelpers.hlsli:105-116): a candidate
    of a geometry without the OPAQUE flag commits only if BaseColor.a (factor times the texture's alpha at the candidate's own UVs) >=
    AlphaCutoff."""

    def __init__(self, surface):
        self.s = surface
        T = surface.tris
        self.tested = np.arange(len(T.opaque)) if surface.m["alpha_ignores_opaque_flag"] else np.nonzero(~T.opaque)[0]

    def __call__(self, tri, u, v, uncertainty):
        S, T = self.s, self.s.tris
        uvs = S.uv_of(tri, u, v)
        objects = T.object0[tri] if S.m["alpha_geometry0"] else T.object[tri]
        commit, close = np.ones(len(tri), bool), np.zeros(len(tri), bool)
        shift = T.uv_extent[tri] * (uncertainty + EPS)[:, None]
        for ob in np.unique(objects):
            sel = objects == ob
            mat, slots = S.objects[ob]
            uv = [[uvs[sel, k, 0], uvs[sel, k, 1]] for k in range(2)]
            commit[sel], alpha = S.tex.is_opaque(mat, slots, uv)
            if "BaseColor" in slots and (np.asarray(mat["BaseColor"]) > 0).any():
                bound = S.tap_bound(slots["BaseColor"], uvs[sel], shift[sel]) * float(mat["BaseColor"][3])
                close[sel] = (np.abs(alpha - float(mat["AlphaCutoff"])) <= bound) & ~S.tap_is_constant(slots["BaseColor"], uvs[sel], shift[sel], 3)
        return commit, close


class Surface:
    """The reference of one scene; the keyword switches (MUTATIONS) each break one rule. tex: the texref.Reference that samples (one with
    a switch of texref.MUTATIONS set carries that mistake through the frame)."""

    def __init__(self, scene, tex=None, **mutations):
        unknown = set(mutations) - set(MUTATIONS)
        assert not unknown, unknown
        self.m = {k: bool(mutations.get(k, False)) for k in MUTATIONS}
        self.scene = scene
        self.tris = Triangles(scene)
        self.tex = tex if tex is not None else texref.Reference()
        self.objects = object_textures(scene)
        self.textured = any(slots for _, slots in self.objects)
        self.alpha_rule = AlphaRule(self)

    # ------------------------------------------------------------------ textures
    def uv_of(self, tri, u, v):
        """both UV sets of hits: [n, set, 2]"""
        if self.m["uv_corner0"]:
            return self.tris.uv[tri][:, :, 0].copy()
        return self.tris.interpolate_uv(tri, u, v)

    def tap_bound(self, entry, uvs, shift):
        """|fp32 sample - float64 sample| of one tap (per hit, over channels, before the material's factor). The tap position differs by
        shift[n, set] in UV units -- the triangle's UV extent times the barycentric uncertainty of the hit -- plus texref's own position
        error (the fp32 interpolation of the f16 corners and the sampler's address arithmetic), in texels of the larger side; the value
        moves by that times the largest difference between neighbouring texels around the footprint, plus the sampler's roundings."""
        data, fmt, index = entry
        dec = _TRUE.decode(data, fmt)
        size = max(dec.shape[0], dec.shape[1])
        diff, mag = _TRUE.footprint2d(dec, uvs[:, index, 0], uvs[:, index, 1])
        pos = size * shift[:, index] + texref.texel_position_error(size, np.abs(uvs[:, index]).max(-1))
        return texref.value_tolerance(pos, diff, mag)

    def tap_is_constant(self, entry, uvs, shift, channel):
        """The tap is decided exactly: the channel samples to the same 0 or 1 at the hit and at the four corners of the box its fp32
        position can lie in, so every texel any such footprint touches holds that value, and a bilinear blend of equal texels 0 or 1 is
        exact in fp32 (c (1 - w) + c w; test_texture_reference.py's alpha case rests on the same fact). This is what lets a mask's solid
        cells stand exactly AT AlphaCutoff = 1 and still be decided."""
        data, fmt, index = entry
        dec = _TRUE.decode(data, fmt)
        size = max(dec.shape[0], dec.shape[1])
        e = (size * shift[:, index] + texref.texel_position_error(size, np.abs(uvs[:, index]).max(-1))) / min(dec.shape[0], dec.shape[1])
        u, v = uvs[:, index, 0], uvs[:, index, 1]
        at = _TRUE.sample2d(dec, u, v)[..., channel]
        same = np.isin(at, (0.0, 1.0))
        for su in (-1.0, 1.0):
            for sv in (-1.0, 1.0):
                same &= _TRUE.sample2d(dec, u + su * e, v + sv * e)[..., channel] == at
        return same

    # ------------------------------------------------------------------ HitInfo::Initialize, SelfIntersectionAvoidance
    def reconstruct(self, tri, u, v, d):
        """The HitInfo of hits (tri, u, v) seen along unit directions d."""
        T = self.tris
        P = T.obj[tri]
        inst = T.inst[tri]
        O, Wm = T.o2w[inst], T.w2o[inst]
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        obj_pos = P[:, 0] + (u[:, None] * e1 + v[:, None] * e2)
        pos = np.einsum("nij,nj->ni", O[:, :, :3], obj_pos) + O[:, :, 3]
        obj_n = np.cross(e1, e2)
        to_world = O[:, :, :3] if self.m["normal_by_matrix"] else Wm[:, :, :3].transpose(0, 2, 1)
        wld_n = np.einsum("nij,nj->ni", to_world, obj_n)
        with np.errstate(invalid="ignore", divide="ignore"):
            wld_scale = 1.0 / np.linalg.norm(wld_n, axis=1)
        flat = wld_n * wld_scale[:, None]
        # the offset: the error bounds of the reconstruction, the object-to-world and the world-to-object transform, along the normal
        c0, c1, c2 = 5.9604644775390625e-8, 1.788139769587360206060111522674560546875e-7, 1.19209317972490680404007434844970703125e-7
        extent = (np.abs(e1) + np.abs(e2) + np.abs(np.abs(e1) - np.abs(e2))).max(1)
        obj_err = c0 * np.abs(P[:, 0]) + c1 * extent[:, None]
        wld_err = c1 * np.einsum("nij,nj->ni", np.abs(O[:, :, :3]), np.abs(obj_pos)) + c2 * np.abs(O[:, :, 3])
        obj_err = c2 * (np.einsum("nij,nj->ni", np.abs(Wm[:, :, :3]), np.abs(pos)) + np.abs(Wm[:, :, 3])) + obj_err
        offset = wld_scale * dot(obj_err, np.abs(obj_n)) + dot(wld_err, np.abs(flat))
        nrm = T.nrm[tri]
        interp = nrm[:, 0] + u[:, None] * (nrm[:, 1] - nrm[:, 0]) + v[:, None] * (nrm[:, 2] - nrm[:, 0])
        geo = np.where(T.has_n[tri][:, None], normalize(np.einsum("nij,nj->ni", to_world, interp)), flat)
        front = dot(geo, d) < 0
        shading = geo if self.m["no_front_flip"] else np.where(front[:, None], geo, -geo)
        tan = T.tan[tri]
        tangent = tan[:, 0] + u[:, None] * (tan[:, 1] - tan[:, 0]) + v[:, None] * (tan[:, 2] - tan[:, 0])
        tangent = np.where(T.has_t[tri][:, None], normalize(np.einsum("nij,nj->ni", O[:, :, :3], tangent)), 0.0)
        mot = T.mot[tri]
        motion = mot[:, 0] + u[:, None] * (mot[:, 1] - mot[:, 0]) + v[:, None] * (mot[:, 2] - mot[:, 0])
        return {"position": pos, "object_position": obj_pos, "offset": offset, "flat": flat, "geometric": geo, "front": front,
                "shading": shading, "tangent": tangent, "motion": motion, "instance": inst, "geometry": T.geom[tri],
                "primitive": T.prim[tri], "object": T.object[tri], "perp": np.abs(dot(geo, d)), "uv": self.uv_of(tri, u, v), "tri": tri,
                "front_tangent": tangent if self.m["tangent_no_back_flip"] else np.where(front[:, None], tangent, -tangent)}

    def environment(self, scene_data, d):
        """GetEnvironmentLightColor (ShadingHelpers.hlsli:11-30): the texture (lat-long or cube) looked up along the direction turned by
        EnvironmentLightTransform; else the constant colour, or the procedural sky when its alpha is negative"""
        descriptor = int(scene_data["EnvironmentLightTextureDescriptor"])
        if descriptor != 0xFFFFFFFF:
            sd = np.array(scene_data).reshape(()).copy()
            M = np.asarray(sd["EnvironmentLightTransform"], f64).reshape(3, 4).copy()
            if self.m["env_no_transform"]:
                M[:, :3] = np.eye(3)
            if self.m["env_transposed"]:
                M[:, :3] = M[:, :3].T.copy()
            sd["EnvironmentLightTransform"] = M.reshape(np.shape(sd["EnvironmentLightTransform"]))
            item = self.scene.heap[descriptor]
            return self.tex.environment(sd, item.array, item.fmt, d)
        c = np.asarray(scene_data["EnvironmentLightColor"], f64)
        if c[3] >= 0:
            return np.broadcast_to(c[:3], d.shape).copy()
        t = (d[:, 1:2] + 1.0) * 0.5
        return texref.srgb_to_linear(1.0 + t * (np.array([0.5, 0.7, 1.0]) - 1.0))

    def environment_bound(self, scene_data, d, angle):
        """(|fp32 environment - float64 environment| per direction, undecided). Zero without a texture. The direction may be off by `angle`
        radians. Lat-long: v = acos(w.y) / pi moves by angle / pi, u = atan2 / 2 pi by angle / (2 pi r), r = |w.xz|, and the fp32 acos /
        atan2 of arguments rounded at 2^-24 add 2^-24 / r each (test_texture_reference's pole term); within POLE of a pole nothing is
        decided (atan2 of two roundings; the NaN-coordinate rule at |w.y| = 1). Cube: (sc, tc) / ma has slope <= 2 on a face, so the
        position moves by 2 angle of the face's half-width; the contrast is the texture's whole range (texref.cube_footprint), which also
        covers a face chosen differently: seamless filtering is continuous across edges."""
        n = len(d)
        descriptor = int(scene_data["EnvironmentLightTextureDescriptor"])
        if descriptor == 0xFFFFFFFF:
            return np.zeros(n), np.zeros(n, bool)
        item = self.scene.heap[descriptor]
        dec = _TRUE.decode(item.array, item.fmt)
        M = np.asarray(scene_data["EnvironmentLightTransform"], f64).reshape(3, 4)[:, :3]
        w = normalize(d @ M.T)
        angle = np.broadcast_to(np.asarray(angle, f64), (n,))
        if int(scene_data["IsEnvironmentLightTextureCubeMap"]):
            size = dec.shape[1]
            diff, mag = _TRUE.cube_footprint(dec, w)
            return texref.value_tolerance(texref.texel_position_error(size, 1.0) + size * 2.0 * angle, diff, mag), np.zeros(n, bool)
        size = max(dec.shape[0], dec.shape[1])
        r = np.hypot(w[:, 0], w[:, 2])
        uu = (1.0 + np.arctan2(w[:, 0], w[:, 2]) / np.pi) / 2.0
        vv = np.arccos(np.clip(w[:, 1], -1.0, 1.0)) / np.pi
        diff, mag = _TRUE.footprint2d(dec, uu, vv)
        with np.errstate(divide="ignore"):
            pos = texref.texel_position_error(size, 1.0) + size * (angle / np.pi + (angle / (2.0 * np.pi) + 2.0 * EPS) / np.maximum(r, 1e-30))
        return texref.value_tolerance(pos, diff, mag), r < POLE

    MATERIAL_KEYS = ("BaseColor", "EmissiveStrength", "EmissiveColor", "Metallic", "Roughness", "IOR", "Transmission")

    def material(self, objects, hit=None, uncertainty=None):
        """The Material of hits. Without `hit`, or in a scene without material textures: the record as it stands (EvaluateMaterial of an
        untextured object returns it unchanged). With `hit` (reconstruct's dictionary): EvaluateMaterial (ShadingHelpers.hlsli:161-235) through
        texref at the hit's UV sets, with its shading normal and FRONT tangent (HitInfo.hlsli:85-88). Adds
          Normal      the shading normal, perturbed where the object has a Normal texture AND the mesh has tangents (any(T != 0))
          bound       per quantity (base, emission, metal, rough, trans, normal) what fp32 may differ by: tap_bound at `uncertainty`
                      (the barycentric uncertainty of each hit; EDGE_B by default) times the material's factor
          undecided   a decision inside the material lies within its bound: Metallic < 1 ahead of the Transmission tap, or the normal
                      map's x^2 + y^2 at the rim where sqrt(saturate(1 - x^2 - y^2)) clamps"""
        m = self.scene.object_data["Material"][objects]
        out = {k: np.asarray(m[k], f64) for k in self.MATERIAL_KEYS}
        if hit is None or not self.textured:
            return out
        n = len(objects)
        out = {k: v.copy() for k, v in out.items()}
        out["Normal"] = hit["shading"].copy()
        bound = {k: np.zeros(n) for k in ("base", "emission", "metal", "rough", "trans", "normal")}
        undecided = np.zeros(n, bool)
        unc = np.full(n, EDGE_B) if uncertainty is None else np.asarray(uncertainty, f64)
        shift_all = self.tris.uv_extent[hit["tri"]] * (unc + EPS)[:, None]
        for ob in np.unique(objects):
            mat, slots = self.objects[ob]
            if not slots:
                continue
            sel = np.nonzero(objects == ob)[0]
            slots = dict(slots)
            if self.m["normal_map_ignored"]:
                slots.pop("Normal", None)
            if self.m["emissive_texture_ignored"]:
                slots.pop("EmissiveColor", None)
            uvs, shift = hit["uv"][sel], shift_all[sel]
            uv = [[uvs[:, k, 0], uvs[:, k, 1]] for k in range(2)]
            Ns = hit["shading"][sel]
            T = hit["front_tangent"][sel] if self.tris.has_t[hit["tri"][sel]].all() else None
            if T is None and self.m["normal_map_without_tangents"]:
                T = B.get_basis(Ns)[0]
            e = self.tex.evaluate_material(mat, slots, uv, Ns, T)
            strength = float(mat["EmissiveStrength"])
            out["BaseColor"][sel] = e["BaseColor"]; out["Metallic"][sel] = e["Metallic"]; out["Roughness"][sel] = e["Roughness"]
            out["Transmission"][sel] = e["Transmission"]; out["Normal"][sel] = e["Normal"]
            if strength != 0:
                out["EmissiveColor"][sel] = e["Emission"] / strength
            if self.m["transmission_gate_on_factor"] and float(mat["Metallic"]) >= 1:
                out["Transmission"][sel] = float(mat["Transmission"])

            def tb(slot):
                return self.tap_bound(slots[slot], uvs, shift)
            if "BaseColor" in slots and (np.asarray(mat["BaseColor"]) > 0).any():
                bound["base"][sel] = tb("BaseColor") * float(np.max(mat["BaseColor"][:3]))
            if "EmissiveColor" in slots and (np.asarray(mat["EmissiveColor"], f64) * strength > 0).any():
                bound["emission"][sel] = tb("EmissiveColor") * strength * float(np.max(mat["EmissiveColor"]))
            if "MetallicRoughness" in slots:
                if mat["Metallic"] > 0 or mat["Roughness"] > 0:
                    t = tb("MetallicRoughness")
                    bound["metal"][sel] = t * float(mat["Metallic"]); bound["rough"][sel] = t * float(mat["Roughness"])
            else:
                if "Metallic" in slots and mat["Metallic"] > 0:
                    bound["metal"][sel] = tb("Metallic") * float(mat["Metallic"])
                if "Roughness" in slots and mat["Roughness"] > 0:
                    bound["rough"][sel] = tb("Roughness") * float(mat["Roughness"])
            if "Transmission" in slots and mat["Transmission"] > 0:
                bound["trans"][sel] = tb("Transmission") * float(mat["Transmission"])
                undecided[sel] |= (bound["metal"][sel] > 0) & (np.abs(e["Metallic"] - 1.0) <= bound["metal"][sel])
            if "Normal" in slots and T is not None:
                t = tb("Normal")
                xy = _TRUE._tap(slots, "Normal", uv)[..., :2] * 2.0 - 1.0
                r2 = (xy * xy).sum(-1)
                nz = np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))
                # n = (x, y, sqrt(1 - x^2 - y^2)), x = 2 tap - 1: |dn| <= 2 t (sqrt 2 + |xy| / nz) before the normalisation, which only shrinks it
                bound["normal"][sel] = 2.0 * t * (np.sqrt(2.0) + np.sqrt(r2) / np.maximum(nz, 1e-3))
                undecided[sel] |= (1.0 - r2) <= 8.0 * t
        out["bound"], out["undecided"] = bound, undecided
        return out

    # ------------------------------------------------------------------ GBufferGeneration.hlsl main
    def render(self, camera, W, H, scene_data=None, rows=None):
        """Per pixel of rows [y0, y1) (row-major, flattened) what the pass stores, in float64, and the error terms of the tolerances."""
        cam = np.asarray(camera).reshape(())
        sd = np.asarray(scene_data if scene_data is not None else self.scene.scene_data).reshape(())
        uv, pix = pixel_uv(W, H, cam["Jitter"], rows)
        o, d, tmin, tmax = pinhole(cam, uv)
        c = self.tris.closest(o, d, tmin, tmax, alpha=self.alpha_rule if len(self.alpha_rule.tested) else None)
        hit = c["hit"]
        h = self.reconstruct(c["tri"], c["u"], c["v"], d)
        r = {"uv": uv, "pixel": pix, "origin": o, "direction": d, "tmin": tmin, "tmax": tmax, "hit": hit, "t": c["t"], "u": c["u"], "v": c["v"],
             "tri": c["tri"]}
        r.update({k: h[k] for k in ("flat", "geometric", "shading", "front", "tangent", "offset", "instance", "geometry", "primitive", "object")})
        r["unsafe"] = c["unsafe"] | (hit & (h["perp"] < PERP))
        pos = np.where(hit[:, None], h["position"], o + d * 1e8)                        # CastRay's miss position
        r["position"] = np.where(hit[:, None], pos, np.inf)
        pos_err = np.where(hit, K_POSITION * EPS * (np.linalg.norm(o, axis=1) + np.where(hit, c["t"], 0.0)) + np.where(hit, h["offset"], 0.0),
                           4.0 * EPS * 1e8)
        r["position_error"] = pos_err
        # depths
        w2p = np.asarray(cam["WorldToProjection"], f64)
        clip, mag = row_vector(w2p, pos)
        col = np.linalg.norm(w2p[:3], axis=0)
        lin = clip[:, 3]
        e_w = 4.0 * EPS * mag[:, 3] + pos_err * col[3]
        e_z = 4.0 * EPS * mag[:, 2] + pos_err * col[2]
        with np.errstate(invalid="ignore", divide="ignore"):
            nd = clip[:, 2] / clip[:, 3]
            e_nd = (e_z + np.abs(nd) * e_w) / np.abs(lin) + EPS * np.abs(nd)
        reversed_ = int(cam["IsNormalizedDepthReversed"]) != 0
        r["linear_depth"] = np.where(hit, lin, np.inf); r["linear_depth_error"] = e_w
        r["normalized_depth"] = np.where(hit, nd, 0.0 if reversed_ else 1.0); r["normalized_depth_error"] = np.where(hit, e_nd, 0.0)
        # CalculateMotionVector
        static = int(sd["IsStatic"]) != 0
        prev = pos
        if not static:
            q = h["object_position"] + (0.0 if self.m["mv_no_vertex_term"] else h["motion"])
            Pm = self.tris.prev_o2w[h["instance"]]
            moved = np.einsum("nij,nj->ni", Pm[:, :, :3], q) + Pm[:, :, 3]
            prev = np.where(hit[:, None], moved, pos)
        cur = self.m["mv_current_camera"]
        pw2p = w2p if cur else np.asarray(cam["PreviousWorldToProjection"], f64)
        pw2v = np.asarray(cam["PreviousWorldToView"], f64)
        if cur:                                                                        # the current view matrix: the inverse of ViewToWorld
            pw2v = np.linalg.inv(np.asarray(cam["ViewToWorld"], f64))
        pclip, pmag = row_vector(pw2p, prev)
        pview, vmag = row_vector(pw2v, prev)
        with np.errstate(invalid="ignore", divide="ignore"):
            ndc = pclip[:, :2] / pclip[:, 3:4]
            suv = ndc * np.array([0.5, 0.5 if self.m["v_not_flipped"] else -0.5]) + 0.5
            A = (pmag[:, :2] + np.abs(ndc) * pmag[:, 3:4]) / np.abs(pclip[:, 3:4])
            pcol = np.linalg.norm(pw2p[:3], axis=0)
            through = pos_err[:, None] * (pcol[:2] + np.abs(ndc) * pcol[3]) / np.abs(pclip[:, 3:4])
        dims = np.array([W, H], f64)
        lin_all = clip[:, 3]                                                           # the miss branch projects its far point too
        r["motion"] = np.concatenate([(suv - uv) * dims, (pview[:, 2] - lin_all)[:, None]], -1)
        r["motion_error"] = np.concatenate([(MV_ROUNDINGS * EPS * (1.0 + A) + through) * dims,
                                            (4.0 * EPS * (vmag[:, 2] + mag[:, 3]) + pos_err * (np.linalg.norm(pw2v[:3, 2]) + col[3]))[:, None]], -1)
        # material words: EvaluateMaterial at the hit (an untextured object's material as it stands)
        mat = self.material(h["object"], h, c["bary"])
        base, metal = mat["BaseColor"][:, :3], mat["Metallic"]
        r["base_color_metalness"] = np.concatenate([base, metal[:, None]], -1)
        r["roughness"] = np.maximum(B.MIN_ROUGHNESS, mat["Roughness"])
        r["ior"], r["transmission"] = mat["IOR"], mat["Transmission"]
        emission = mat["EmissiveStrength"][:, None] * mat["EmissiveColor"]
        r["radiance"] = np.where(hit[:, None], emission, self.environment(sd, d))
        env_bound, env_undecided = self.environment_bound(sd, d, 8.0 * EPS)
        r["unsafe"] = r["unsafe"] | (~hit & env_undecided)
        r["radiance_error"] = np.where(hit, 0.0, env_bound)
        if "bound" in mat:                                                            # a textured scene: the perturbed normal and every tap's bound
            bd = mat["bound"]
            r["shading"] = mat["Normal"]
            r["unsafe"] = r["unsafe"] | (hit & mat["undecided"])
            r["radiance_error"] = np.where(hit, bd["emission"], env_bound)
            r["base_color_metalness_error"] = np.stack([bd["base"]] * 3 + [bd["metal"]], -1)
            r["roughness_error"], r["transmission_error"], r["shading_error"] = bd["rough"], bd["trans"], bd["normal"]
        # EstimateDemodulationFactors (NRD's material factors): Fenv from EnvironmentTerm_Rtg; (1 - Fenv) albedo 0.99 + 0.01, Fenv 0.99 + 0.01
        ior_i = np.where(h["front"], 1.0, mat["IOR"]); ior_o = np.where(h["front"], mat["IOR"], 1.0)
        r2 = ((ior_i - ior_o) / (ior_i + ior_o)) ** 2

        def albedos(base, metal, rough, nov):
            F0 = r2[:, None] + (base - r2[:, None]) * metal[:, None]
            Fenv = B.env_term_rtg(F0, nov, rough)
            return (1.0 - Fenv) * (base * (1.0 - metal[:, None])) * 0.99 + 0.01, Fenv * 0.99 + 0.01
        nov = np.abs(dot(r["shading"], -d))
        r["diffuse_albedo"], r["specular_albedo"] = albedos(base, metal, r["roughness"], nov)
        if "bound" in mat:                                                            # one more evaluation per textured quantity, moved by its bound
            bd = mat["bound"]
            moved = (albedos(base + bd["base"][:, None], metal, r["roughness"], nov), albedos(base, np.clip(metal + bd["metal"], 0, 1), r["roughness"], nov),
                     albedos(base, metal, r["roughness"] + bd["rough"], nov), albedos(base, metal, r["roughness"], np.clip(nov + bd["normal"], 0, 1)))
            with np.errstate(invalid="ignore"):
                r["diffuse_albedo_error"] = sum(np.abs(mv[0] - r["diffuse_albedo"]) for mv in moved)
                r["specular_albedo_error"] = sum(np.abs(mv[1] - r["specular_albedo"]) for mv in moved)
        return r


# ----------------------------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------------------------
def compare(gb, ref, surface, flags=0xFFFFFFFF):
    """G-buffer textures `gb` (name -> [rows, W, c] in the stored formats) against Surface.render's `ref`. Returns (failures, figures):
    failures maps a texture (or "hit mask", "plane") to the number of kept pixels outside its tolerance; figures carries the unsafe
    share of hit pixels and the largest in-plane position error in units of 2^-24 (|origin| + t)."""
    n = len(ref["hit"])
    flat = {k: np.asarray(v).reshape(n, -1) for k, v in gb.items()}
    keep = ~ref["unsafe"]
    hit = ref["hit"]
    fails, fig = {}, {}

    def fail(name, bad, where):
        k = int((bad & where).sum())
        if k:
            fails[name] = k
    got_hit = np.isfinite(flat["Position"][:, 3])
    fail("hit mask", got_hit != hit, keep)
    fig["unsafe_share"] = float((ref["unsafe"] & hit).sum() / max(1, hit.sum()))
    k_hit, k_miss = keep & hit & got_hit, keep & ~hit & ~got_hit
    P = flat["Position"].astype(f64)
    fail("Position (miss)", ~np.isposinf(P).all(1), k_miss)
    corner = surface.tris.world[ref["tri"], 0]
    with np.errstate(invalid="ignore"):
        err = P[:, :3] - ref["position"]
        along = dot(err, ref["flat"])
        in_plane = np.linalg.norm(err - along[:, None] * ref["flat"], axis=1)
        unit = EPS * (np.linalg.norm(ref["origin"], axis=1) + ref["t"])
        plane = np.abs(dot(P[:, :3] - corner, ref["flat"]))
        fail("plane", ~(plane <= P[:, 3]), k_hit)
        fail("Position (in plane)", ~(in_plane <= K_POSITION * unit), k_hit)
        fail("Position.w", ~(np.abs(P[:, 3] - ref["offset"]) <= OFFSET_ROUNDINGS * EPS * ref["offset"]), k_hit)
        fig["in_plane"] = float((in_plane[k_hit] / unit[k_hit]).max()) if k_hit.any() else 0.0
        fig["plane_over_offset"] = float((plane[k_hit] / P[k_hit, 3]).max()) if k_hit.any() else 0.0
    for name, key in (("FlatNormal", "flat"), ("GeometricNormal", "geometric")):
        e = flat[name].astype(f64) * SNORM16
        fail(name, ~(np.abs(e - oct_encode(ref[key])) <= SNORM16).all(1), k_hit)
    nr = flat["NormalRoughness"].astype(f64) * SNORM16
    zero = np.zeros(n)
    extra = lambda key, shape=None: ref.get(key, zero if shape is None else np.zeros((n, shape)))   # the texture bounds of a textured scene
    fail("NormalRoughness.xyz", ~(np.abs(nr[:, :3] - ref["shading"]) <= SNORM16 + extra("shading_error")[:, None]).all(1), k_hit)
    fail("NormalRoughness.w", ~(np.abs(nr[:, 3] - ref["roughness"]) <= SNORM16 + extra("roughness_error")), k_hit)
    ld, ndp = flat["LinearDepth"][:, 0].astype(f64), flat["NormalizedDepth"][:, 0].astype(f64)
    with np.errstate(invalid="ignore"):
        fail("LinearDepth", ~(np.abs(ld - ref["linear_depth"]) <= ref["linear_depth_error"]), k_hit)
        fail("LinearDepth (miss)", ~np.isposinf(ld), k_miss)
        fail("NormalizedDepth", ~(np.abs(ndp - ref["normalized_depth"]) <= ref["normalized_depth_error"]), k_hit | k_miss)
    mv = flat["MotionVector"]
    fail("MotionVector", ~f16_close(mv[:, :3], ref["motion"], ref["motion_error"]).all(1), k_hit | k_miss)
    fail("MotionVector.w", mv[:, 3] != 0, k_hit | k_miss)
    bcm = flat["BaseColorMetalness"].astype(f64) * UNORM8
    fail("BaseColorMetalness", ~(np.abs(bcm - np.clip(ref["base_color_metalness"], 0, 1)) <= UNORM8 + extra("base_color_metalness_error", 4)).all(1), k_hit)
    fail("IOR", ~f16_close(flat["IOR"][:, 0], ref["ior"]), k_hit)
    fail("Transmission", ~(np.abs(flat["Transmission"][:, 0].astype(f64) * UNORM8 - ref["transmission"]) <= UNORM8 + extra("transmission_error")),
         k_hit & (ref["base_color_metalness"][:, 3] < 1))
    fail("Radiance", ~f16_close(flat["Radiance"][:, :3], ref["radiance"], extra("radiance_error")[:, None]).all(1), k_hit | k_miss)
    fail("Radiance.w", flat["Radiance"][:, 3] != 0, k_hit | k_miss)
    if flags & 0xC0 == 0xC0:
        for name, key in (("DiffuseAlbedo", "diffuse_albedo"), ("SpecularAlbedo", "specular_albedo")):
            fail(name, ~f16_close(flat[name][:, :3], ref[key], B.REL * ref[key] + extra(key + "_error", 3)).all(1), k_hit)
    return fails, fig


# ----------------------------------------------------------------------------------------------
# scenes (each <= 2 000 triangles, rendered at 96 x 64)
# ----------------------------------------------------------------------------------------------
SIZE = (96, 64)


def _fan(S, mat, n=7, radius=1.0):
    """a planar fan of n triangles about the origin in the object's xy plane, without vertex normals"""
    a = np.linspace(0.0, 2.0 * np.pi, n + 1)
    pos = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(a) * radius, np.sin(a) * radius * 0.8, np.zeros_like(a)], -1)])
    idx = np.stack([np.zeros(n, np.int64), np.arange(1, n + 1), np.arange(2, n + 2)], -1)
    return S.Mesh(S.make_vertices(pos), S.make_indices(idx.reshape(-1)), False, mat)


def _uv_quad(S, mat):
    """a unit quad in xy with normals, tangents and TexCoord0"""
    return S.quad_mesh((-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0), (0, 0, -1), mat, uv_scale=2.0)


def transformed(S, emissive=False, aspect=SIZE[0] / SIZE[1], subdiv=2, mirrored_sphere=True):
    """Mirrored and strongly non-uniform instances of an icosphere, a box and a normal-less box; a mesh with 32-bit indices; a hidden
    instance in front of everything; a mesh with tangents and UVs. emissive: the uv quad emits (the estimator's scene; a number: its strength). subdiv,
    mirrored_sphere: a finer sphere without its mirrored twin, for a scene beyond LDS."""
    sphere = S.icosphere_mesh(subdiv, S.material((0.8, 0.6, 0.3), metallic=1.0, roughness=0.25))
    box = S.box_mesh(S.material((0.2, 0.5, 0.8), roughness=0.4))
    bare = S.box_mesh(S.material((0.7, 0.7, 0.7), roughness=0.7, ior=1.33), has_normals=False)
    wide = S.box_mesh(S.material((0.6, 0.3, 0.6), metallic=0.5, roughness=0.3))
    wide.indices = wide.indices.astype(np.uint32)                                  # 32-bit indices without 65 536 of them
    quad = _uv_quad(S, S.material((0.9, 0.9, 0.2), emissive=(1.0, 0.8, 0.6) if emissive else (0, 0, 0),
                                    strength=6.0 if emissive is True else float(emissive), roughness=0.6))
    floor = S.quad_mesh((-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1), (0, 1, 0), S.material((0.6, 0.6, 0.6)))
    nodes = [S.MeshNode([m]) for m in (sphere, box, bare, wide, quad, floor)]
    objects = [
        S.RenderObject(0, S.trs((-1.6, 0.3, 0.2), 25.0, (1.0, 0.3, 0.6), pitch_deg=15.0)),
        S.RenderObject(1, S.trs((-0.1, 0.1, 0.6), -35.0, (-0.8, 0.5, 0.5), pitch_deg=-20.0)),       # mirrored
        S.RenderObject(2, S.trs((1.7, 0.0, 1.4), 50.0, (3.0, 0.2, 1.5), pitch_deg=10.0)),
        S.RenderObject(0, S.trs((0.9, 0.9, 0.4), -10.0, (-1.0, 0.4, 2.0), pitch_deg=30.0)),        # mirrored sphere
        S.RenderObject(3, S.trs((-0.9, -0.5, 0.0), 20.0, (0.5, 0.4, 0.7), pitch_deg=-5.0)),
        S.RenderObject(1, S.trs((0.0, 0.0, -1.5), 0.0, (3.0, 3.0, 0.1)), visible=False),          # would hide everything
        S.RenderObject(4, S.trs((0.6, -0.55, -0.4), 155.0, (0.9, 0.7, 1.0), pitch_deg=20.0)),          # seen from behind
        S.RenderObject(5, S.trs((0.0, -1.0, 1.0), 0.0, (4.0, 1.0, 3.0))),
    ]
    if not mirrored_sphere:
        del objects[3]
    cam = S.make_camera((0.15, 0.35, -3.2), forward=(0.02, -0.08, 1.0), hfov_deg=70.0, aspect=aspect, jitter=(0.23, -0.31))
    return S.Scene(nodes, objects, cam, S.make_scene_data((0.3, 0.4, 0.5, 1.0)), name="transformed").finalize()


def moved(S, aspect=SIZE[0] / SIZE[1]):
    """`transformed` in motion: IsStatic 0, every PreviousObjectToWorld different, per-vertex motion on the sphere, the previous
    camera elsewhere and looking elsewhere."""
    sc = transformed(S, aspect=aspect)
    sc.name = "moved"
    sphere = sc.nodes[0].meshes[0]
    p = np.asarray(sphere.vertices["Position"], f64)
    mv = np.zeros((len(p), 4), np.float16)
    mv[:, :3] = 0.05 * np.stack([np.sin(3.0 * p[:, 1]), p[:, 0] * p[:, 2], np.cos(2.0 * p[:, 0]) - 0.5], -1)
    sphere.motion_vectors = mv.view(np.uint16)
    sc.scene_data = S.make_scene_data((0.3, 0.4, 0.5, 1.0), is_static=False)
    sc.finalize()
    for i, ro in enumerate(sc.objects):
        shift = S.trs((0.05 * (i + 1), -0.03 * i, 0.02 * (i % 3)), 3.0 + i, (1.0 + 0.02 * i, 1.0, 1.0 - 0.01 * i)).astype(f64)
        m = np.vstack([np.asarray(ro.transform, f64), [0, 0, 0, 1]])
        sc.instance_data[i]["PreviousObjectToWorld"] = (np.vstack([shift, [0, 0, 0, 1]]) @ m)[:3]
    prev = S.make_camera((0.05, 0.42, -3.05), forward=(-0.03, -0.05, 1.0), hfov_deg=70.0, aspect=aspect)
    cam = sc.camera
    cam["PreviousPosition"] = prev["Position"]
    for k in ("WorldToView", "ViewToProjection", "WorldToProjection", "ProjectionToView", "ViewToWorld"):
        cam["Previous" + k] = prev["Previous" + k]
    return sc


def depth(S, far, reversed_, aspect=SIZE[0] / SIZE[1]):
    """Boxes from 2 to 60 units away under a camera with a finite (far = 50 cuts the last ones off) or infinite far plane, a quarter
    of the frame and more looking past them."""
    box = S.box_mesh(S.material((0.5, 0.5, 0.5)))
    nodes = [S.MeshNode([box])]
    objects = [S.RenderObject(0, S.trs((-3.0 + 1.1 * i, -0.4 + 0.15 * i, z), 12.0 * i, (1.0, 1.6, 1.0), pitch_deg=7.0 * i))
               for i, z in enumerate((2.0, 3.5, 6.0, 11.0, 24.0, 60.0))]
    objects.append(S.RenderObject(0, S.trs((0.0, -2.0, 95.0), 0.0, (40.0, 0.2, 200.0))))
    cam = S.make_camera((0.0, 0.6, -1.0), forward=(0.05, 0.12, 1.0), hfov_deg=80.0, aspect=aspect, near=0.1, far=far, jitter=(-0.2, 0.4))
    cam["IsNormalizedDepthReversed"] = 1 if reversed_ else 0
    return S.Scene(nodes, objects, cam, S.make_scene_data((0.0, 0.0, 0.0, -1.0)), name=f"depth_far{far}_rev{int(reversed_)}").finalize()


def scale(S, aspect=SIZE[0] / SIZE[1]):
    """Two planar fans: one translated to 1e3 and scaled 1e-2, one scaled 1e-3 near the origin. For the PositionOffset invariant only."""
    nodes = [S.MeshNode([_fan(S, S.material((0.5, 0.5, 0.5)))])]
    far = S.trs((1000.0, 1000.0, 1000.0), 20.0, (1e-2, 1e-2, 1e-2), pitch_deg=15.0)
    near = S.trs((0.0012, -0.0004, 0.004), -30.0, (1e-3, 1e-3, 1e-3), pitch_deg=-10.0)
    cams = {"far": S.make_camera((1000.0, 1000.0, 999.96), hfov_deg=40.0, aspect=aspect, near=1e-4, jitter=(0.1, 0.2)),
            "near": S.make_camera((0.0012, -0.0004, 0.0), hfov_deg=40.0, aspect=aspect, near=1e-5, jitter=(0.1, 0.2))}
    sc = S.Scene(nodes, [S.RenderObject(0, far), S.RenderObject(0, near)], cams["far"], S.make_scene_data((0, 0, 0, 1)), name="scale").finalize()
    return sc, cams


SCENES = {
    "transformed": lambda S: transformed(S),
    "moved": lambda S: moved(S),
    "depth_far50": lambda S: depth(S, 50.0, False),
    "depth_far50_reversed": lambda S: depth(S, 50.0, True),
    "depth_infinite": lambda S: depth(S, float("inf"), False),
    "depth_infinite_reversed": lambda S: depth(S, float("inf"), True),
}
