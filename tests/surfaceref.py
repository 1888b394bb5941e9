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

Every switch of `MUTATIONS` breaks one rule; tests/test_gbuffer_reference.py shows that the comparison notices each.
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
MUTATIONS = ("normal_by_matrix", "no_front_flip", "mv_current_camera", "mv_no_vertex_term", "v_not_flipped")

f64 = np.float64


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
        cols = {k: [] for k in ("obj", "nrm", "tan", "mot", "has_n", "has_t", "inst", "geom", "prim", "object")}
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

    def closest(self, o, d, tmin, tmax, chunk=1 << 19, drift=None):
        """The exact closest hit of rays (float64 [n, 3], TMin / TMax [n] or scalars, both exclusive): hit, tri, u, v, t and `unsafe`
        (edge / depth of the module docstring). drift = (angle [n], shift [n]): the fp32 ray may lie that far off this one (radians about
        its origin, world units sideways); the edge margin of a pair widens by (angle |t| + shift) over the triangle's world altitude."""
        n, T = len(o), len(self.world)
        tmin = np.broadcast_to(np.asarray(tmin, f64), (n,)); tmax = np.broadcast_to(np.asarray(tmax, f64), (n,))
        out = {"hit": np.zeros(n, bool), "tri": np.zeros(n, np.int64), "u": np.zeros(n), "v": np.zeros(n), "t": np.full(n, np.inf),
               "unsafe": np.zeros(n, bool)}
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
                gap = DEPTH_GAP * np.abs(t)
                near = (b > -thr) & (t > lo - gap) & (t < hi + gap) & ~inside
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
            out["hit"][sl] = hit; out["tri"][sl] = j; out["t"][sl] = t1
            out["u"][sl] = np.where(hit, u[rows, j], 0.0); out["v"][sl] = np.where(hit, v[rows, j], 0.0)
            out["unsafe"][sl] = steal | tie | edge | rng
        return out


class Surface:
    """The reference of one scene; the keyword switches (MUTATIONS) each break one rule."""

    def __init__(self, scene, **mutations):
        unknown = set(mutations) - set(MUTATIONS)
        assert not unknown, unknown
        self.m = {k: bool(mutations.get(k, False)) for k in MUTATIONS}
        self.scene = scene
        self.tris = Triangles(scene)

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
                "primitive": T.prim[tri], "object": T.object[tri], "perp": np.abs(dot(geo, d))}

    def environment(self, scene_data, d):
        """GetEnvironmentLightColor without a texture: the constant colour, or the procedural sky when its alpha is negative"""
        c = np.asarray(scene_data["EnvironmentLightColor"], f64)
        if c[3] >= 0:
            return np.broadcast_to(c[:3], d.shape).copy()
        t = (d[:, 1:2] + 1.0) * 0.5
        return texref.srgb_to_linear(1.0 + t * (np.array([0.5, 0.7, 1.0]) - 1.0))

    def material(self, objects):
        m = self.scene.object_data["Material"][objects]
        return {k: np.asarray(m[k], f64) for k in ("BaseColor", "EmissiveStrength", "EmissiveColor", "Metallic", "Roughness", "IOR", "Transmission")}

    # ------------------------------------------------------------------ GBufferGeneration.hlsl main
    def render(self, camera, W, H, scene_data=None, rows=None):
        """Per pixel of rows [y0, y1) (row-major, flattened) what the pass stores, in float64, and the error terms of the tolerances."""
        cam = np.asarray(camera).reshape(())
        sd = np.asarray(scene_data if scene_data is not None else self.scene.scene_data).reshape(())
        uv, pix = pixel_uv(W, H, cam["Jitter"], rows)
        o, d, tmin, tmax = pinhole(cam, uv)
        c = self.tris.closest(o, d, tmin, tmax)
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
        # material words (untextured: EvaluateMaterial returns the material as it stands)
        mat = self.material(h["object"])
        base, metal = mat["BaseColor"][:, :3], mat["Metallic"]
        r["base_color_metalness"] = np.concatenate([base, metal[:, None]], -1)
        r["roughness"] = np.maximum(B.MIN_ROUGHNESS, mat["Roughness"])
        r["ior"], r["transmission"] = mat["IOR"], mat["Transmission"]
        emission = mat["EmissiveStrength"][:, None] * mat["EmissiveColor"]
        r["radiance"] = np.where(hit[:, None], emission, self.environment(sd, d))
        # EstimateDemodulationFactors (NRD's material factors): Fenv from EnvironmentTerm_Rtg; (1 - Fenv) albedo 0.99 + 0.01, Fenv 0.99 + 0.01
        ior_i = np.where(h["front"], 1.0, mat["IOR"]); ior_o = np.where(h["front"], mat["IOR"], 1.0)
        r2 = ((ior_i - ior_o) / (ior_i + ior_o)) ** 2
        F0 = r2[:, None] + (base - r2[:, None]) * metal[:, None]
        Fenv = B.env_term_rtg(F0, np.abs(dot(h["shading"], -d)), r["roughness"])
        r["diffuse_albedo"] = (1.0 - Fenv) * (base * (1.0 - metal[:, None])) * 0.99 + 0.01
        r["specular_albedo"] = Fenv * 0.99 + 0.01
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
    fail("NormalRoughness.xyz", ~(np.abs(nr[:, :3] - ref["shading"]) <= SNORM16).all(1), k_hit)
    fail("NormalRoughness.w", ~(np.abs(nr[:, 3] - ref["roughness"]) <= SNORM16), k_hit)
    ld, ndp = flat["LinearDepth"][:, 0].astype(f64), flat["NormalizedDepth"][:, 0].astype(f64)
    with np.errstate(invalid="ignore"):
        fail("LinearDepth", ~(np.abs(ld - ref["linear_depth"]) <= ref["linear_depth_error"]), k_hit)
        fail("LinearDepth (miss)", ~np.isposinf(ld), k_miss)
        fail("NormalizedDepth", ~(np.abs(ndp - ref["normalized_depth"]) <= ref["normalized_depth_error"]), k_hit | k_miss)
    mv = flat["MotionVector"]
    fail("MotionVector", ~f16_close(mv[:, :3], ref["motion"], ref["motion_error"]).all(1), k_hit | k_miss)
    fail("MotionVector.w", mv[:, 3] != 0, k_hit | k_miss)
    bcm = flat["BaseColorMetalness"].astype(f64) * UNORM8
    fail("BaseColorMetalness", ~(np.abs(bcm - np.clip(ref["base_color_metalness"], 0, 1)) <= UNORM8).all(1), k_hit)
    fail("IOR", ~f16_close(flat["IOR"][:, 0], ref["ior"]), k_hit)
    fail("Transmission", ~(np.abs(flat["Transmission"][:, 0].astype(f64) * UNORM8 - ref["transmission"]) <= UNORM8), k_hit & (ref["base_color_metalness"][:, 3] < 1))
    fail("Radiance", ~f16_close(flat["Radiance"][:, :3], ref["radiance"]).all(1), k_hit | k_miss)
    fail("Radiance.w", flat["Radiance"][:, 3] != 0, k_hit | k_miss)
    if flags & 0xC0 == 0xC0:
        for name, key in (("DiffuseAlbedo", "diffuse_albedo"), ("SpecularAlbedo", "specular_albedo")):
            fail(name, ~f16_close(flat[name][:, :3], ref[key], B.REL * ref[key]).all(1), k_hit)
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
