"""Float64 restatement of visibility in the DI reservoirs ("Reservoir visibility"): the visibility ray over the
scene's world-space triangles (what a hit is: tests/isectref.py), initial visibility and final shading's reuse and discarding. The
temporal and spatial passes, with visibility carrying and the Raytraced normalisation, are restirref's; so is the Visibility word, which
they carry, and it is re-exported here.

Reservoir frames are restirref's: dicts of [H, W] arrays, LightIndex -1 = empty, "Visibility" the packed word.

Every ray has a margin in the sense of restirref's: the smallest relative distance of its decision from a boundary -- an edge value of
a triangle whose sign decides a hit (isectref's margin), or a hit's t against tmin / tmax. A pixel whose margin is below the caller's
threshold is one where float32 may decide differently; the caller leaves it out."""
import numpy as np

import isectref as I
from restirref import FIELDS, carry, empty, pack, reusable, reuse_margin, sample_points, unpack  # noqa: F401 (the word: re-exported)

TMIN, TMAX_BACKOFF = 1e-3, 2e-3


# ---- the visibility ray ----------------------------------------------------------------------------------------------------------
class Occluders:
    """the scene's triangles in world space (float64 transform of the float32 vertices) with what IsOpaque's direct-lighting overload
    needs of their materials. Textured materials are not restated."""

    def __init__(self, scene):
        tris, mats = [], []
        for i, ro in enumerate(scene.objects):
            if scene.instance_masks is not None and int(scene.instance_masks[i]) == 0:
                continue
            M = np.asarray(scene.instance_data["ObjectToWorld"][i], np.float64).reshape(3, 4)
            for mesh in scene.nodes[ro.node].meshes:
                if mesh.textures:
                    raise NotImplementedError("textured occluders")
                p = mesh.vertices["Position"].astype(np.float64) @ M[:, :3].T + M[:, 3]
                idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)
                tris.append(p[idx])
                m = mesh.material
                mats += [(int(m["AlphaMode"]), float(m["BaseColor"][3]), float(m["AlphaCutoff"]), float(m["Metallic"]),
                          tuple(float(v) for v in m["BaseColor"][:3]), float(m["Transmission"]))] * len(idx)
        self.tris = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
        self.mats = mats

    def _candidate(self, k):
        """IsOpaque (ShadingHelpers.hlsli:117-159) without textures: (blocks, transmittance rgb)"""
        mode, alpha, cutoff, metallic, base, tr = self.mats[k]
        if mode != 0:
            return (True, np.zeros(3)) if alpha >= cutoff else (False, np.ones(3))
        if metallic == 1.0:
            return True, np.zeros(3)
        f = np.float32(np.float32(1.0) - np.float32(metallic))
        t = np.array([float(np.float32(np.float32(f * np.float32(b)) * np.float32(tr))) for b in base])
        return bool((t == 0).all()), t

    def trace(self, origins, targets):
        """rays from origins to targets [n, 3]: direction to the target, tmin 1e-3, tmax = max(0, dist - 2e-3). Returns (blocked [n] bool: an
        opaque candidate inside (tmin, tmax), or the product of the transmittances reached zero; vis [n, 3]: the coloured visibility,
        zero where blocked; margin [n])."""
        o = np.asarray(origins, np.float64).reshape(-1, 3)
        p = np.asarray(targets, np.float64).reshape(-1, 3)
        n = len(o)
        blocked, vis, margin = np.zeros(n, bool), np.ones((n, 3)), np.full(n, np.inf)
        if n == 0 or len(self.tris) == 0:
            return blocked, vis, margin
        d = p - o
        dist = np.linalg.norm(d, axis=-1)
        dirs = d / np.maximum(dist, 1e-300)[:, None]
        tmax = np.maximum(0.0, dist - TMAX_BACKOFF)
        ev = I.edge_values(o[:, None, :], dirs[:, None, :], self.tris[None, :, 0], self.tris[None, :, 1], self.tris[None, :, 2])
        hit = I.exact_hit(ev)
        t = ev["t"]
        with np.errstate(invalid="ignore"):
            inside = hit & (t > TMIN) & (t < tmax[:, None])
            # a triangle's plane crossed well outside (tmin, tmax) cannot become a candidate whatever its edges say
            near_t = ~np.isfinite(t) | ((t > 0.5 * TMIN) & (t < 1.001 * tmax[:, None] + 1e-6))
        U, V, W = ev["U"], ev["V"], ev["W"]
        for name, (a, b) in (("U", (V, W)), ("V", (W, U)), ("W", (U, V))):
            # the sign of this edge value decides the hit only when the other two do not already disagree
            decides = ~(((a < 0) | (b < 0)) & ((a > 0) | (b > 0)))
            m = np.where(decides & near_t, ev["margin" + name], np.inf)
            margin = np.minimum(margin, m.min(-1))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = lambda a, b: np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-30)
            mt = np.where(hit, np.minimum(rel(t, TMIN), rel(t, np.broadcast_to(tmax[:, None], t.shape))), np.inf)
        margin = np.minimum(margin, np.nan_to_num(mt, nan=0.0).min(-1))
        # a ray (nearly) in a triangle's plane: det ~ 0, t and the hit itself are noise in float32 (a sample on the surface's own triangle)
        nrm = np.cross(self.tris[:, 1] - self.tris[:, 0], self.tris[:, 2] - self.tris[:, 0])
        nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-300)
        margin = np.minimum(margin, np.abs(dirs @ nrm.T).min(-1))
        for i, k in zip(*np.nonzero(inside)):
            blocks, tr = self._candidate(k)
            vis[i] = vis[i] * tr
            if blocks or (vis[i] == 0).all():
                blocked[i] = True
        vis[blocked] = 0.0
        for i in np.nonzero(~blocked & (vis != 1.0).any(-1))[0]:             # a partial visibility: its 5-bit quantisation is a decision too
            q = vis[i] * 31.0
            margin[i] = min(margin[i], float(np.abs(q - np.rint(q)).min()) if (np.abs(q - np.rint(q)) > 0).any() else np.inf)
        return blocked, vis, margin


def initial_visibility(cur, fresh, lights, occ, samples):
    """DIInitialSampling.hlsl:49-54: the ray of every initial sample with p-hat > 0; blocked: di_empty(M = LocalLightSamples).
    Returns (frame, margin [H, W], emptied [H, W] bool)."""
    out = {k: np.array(fresh[k]).copy() for k in FIELDS}
    margin = np.full((cur.H, cur.W), np.inf)
    emptied = np.zeros((cur.H, cur.W), bool)
    pix = [(y, x) for y in range(cur.H) for x in range(cur.W) if cur.valid[y, x] and out["LightIndex"][y, x] >= 0 and out["TargetPdf"][y, x] > 0]
    if pix:
        ys, xs = np.array(pix).T
        blocked, _, m = occ.trace(cur.P[ys, xs], sample_points(lights, out["LightIndex"][ys, xs], out["U"][ys, xs], out["V"][ys, xs]))
        for c, b, mm in zip(pix, blocked, m):
            margin[c] = mm
            if b:
                empty(out, c, samples)
                emptied[c] = True
    return out, margin, emptied


def final_pass(cur, inp, in_margin, lights, occ, reuse=False, max_age=4, max_distance=16.0, discard=False):
    """DIFinalShading's visibility: a reservoir with a sample and W > 0 either uses its stored visibility (reuse, 1 <= age <= max_age,
    |d| < max_distance) and is stored unchanged, or traces the coloured ray and stores it with d = 0, age 0; discard: a traced visibility
    of zero stores di_empty(M). Returns (frame, margin, info) with info = dict of [H, W] arrays: vis [H, W, 3] (what shading multiplies
    by), reused, traced, discarded (bool)."""
    H, W = cur.H, cur.W
    out = {k: np.array(inp[k]).copy() for k in FIELDS}
    margin = np.array(in_margin, np.float64).copy()
    info = {"vis": np.zeros((H, W, 3)), "reused": np.zeros((H, W), bool), "traced": np.zeros((H, W), bool), "discarded": np.zeros((H, W), bool)}
    rays = []
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x] or out["LightIndex"][y, x] < 0 or not out["W"][y, x] > 0:
                continue
            w = int(out["Visibility"][y, x])
            if reuse:
                margin[y, x] = min(margin[y, x], reuse_margin(w, max_distance))
            if reuse and reusable(w, max_age, max_distance):
                info["reused"][y, x] = True
                info["vis"][y, x] = unpack(w)[0]
            else:
                rays.append((y, x))
    if rays:
        ys, xs = np.array(rays).T
        _, vis, m = occ.trace(cur.P[ys, xs], sample_points(lights, out["LightIndex"][ys, xs], out["U"][ys, xs], out["V"][ys, xs]))
        for c, v, mm in zip(rays, vis, m):
            margin[c] = min(margin[c], mm)
            info["traced"][c] = True
            info["vis"][c] = v
            out["Visibility"][c] = pack(v)
            if discard and (v == 0).all():
                empty(out, c, out["M"][c])
                info["discarded"][c] = True
    return out, margin, info
