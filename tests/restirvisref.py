"""Float64 restatement of visibility in the DI reservoirs ("Reservoir visibility"): the Visibility word, the
visibility ray over the scene's world-space triangles (what a hit is: tests/isectref.py), and the temporal, spatial and final passes with
initial visibility, Raytraced normalisation, visibility carrying, final-visibility reuse and discarding. The reuse arithmetic itself is
restirref's (its primitives are imported, nothing there is edited); with every flag off the passes here are restirref's passes, which
tests/test_direct_lighting_visibility_rules.py checks.

Reservoir frames are dicts of [H, W] arrays as restirref uses them (LightIndex -1 = empty) plus "Visibility" (the packed word).

Every ray has a margin in the sense of restirref's: the smallest relative distance of its decision from a boundary -- an edge value of
a triangle whose sign decides a hit (isectref's margin), or a hit's t against tmin / tmax. A pixel whose margin is below the caller's
threshold is one where float32 may decide differently; the caller leaves it out."""
import numpy as np

import isectref as I
import restirref as R

TMIN, TMAX_BACKOFF = 1e-3, 2e-3
FIELDS = ("LightIndex", "U", "V", "W", "M", "TargetPdf", "Age", "Visibility")


# ---- the Visibility word ---------------------------------------------------------------------------------------------------------
def pack(rgb, dx=0, dy=0, age=0):
    """bits 0-14: uint(clamp(v, 0, 1) * 31) per channel (float32, as stored); 15-20 / 21-26: dx, dy as 6-bit two's complement clamped to
    +-31; 27-30: age saturating at 15; bit 31: 0"""
    c = [int(np.float32(min(max(np.float32(v), np.float32(0)), np.float32(1))) * np.float32(31)) for v in rgb]
    dx, dy = max(-31, min(31, int(dx))), max(-31, min(31, int(dy)))
    return c[0] | c[1] << 5 | c[2] << 10 | (dx & 63) << 15 | (dy & 63) << 21 | min(int(age), 15) << 27


def unpack(word):
    """-> (rgb in [0, 1], dx, dy, age)"""
    w = int(word)
    s6 = lambda v: v - 64 if v & 32 else v
    return (np.array([w & 31, (w >> 5) & 31, (w >> 10) & 31]) / 31.0, s6((w >> 15) & 63), s6((w >> 21) & 63), (w >> 27) & 15)


def carry(word, ddx, ddy, dage):
    """the word of a sample taken from the pixel at offset (ddx, ddy), dage frames later: the colour stays, d and age move and saturate"""
    _, dx, dy, age = unpack(word)
    w = int(word)
    dx, dy = max(-31, min(31, dx + ddx)), max(-31, min(31, dy + ddy))
    return (w & 0x7FFF) | (dx & 63) << 15 | (dy & 63) << 21 | min(age + dage, 15) << 27


def reusable(word, max_age, max_distance):
    """final shading may use the stored visibility: 1 <= age <= max_age and sqrt(dx^2 + dy^2) < max_distance (float32, as compared)"""
    _, dx, dy, age = unpack(word)
    return 1 <= age <= max_age and bool(np.sqrt(np.float32(dx * dx + dy * dy)) < np.float32(max_distance))


def reuse_margin(word, max_distance):
    """relative distance of the distance test from its boundary (the age test is on integers)"""
    _, dx, dy, _ = unpack(word)
    return R._margin(float(np.sqrt(float(dx * dx + dy * dy))), float(max_distance))


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


def sample_points(lights, li, U, V):
    """Math::SampleTriangle(r1 = U, r2 = V) on light records li: base + e0 * sqrt(U) (1 - V) + e1 * sqrt(U) V"""
    lt = lights[np.asarray(li, np.int64)]
    s = np.sqrt(np.asarray(U, np.float64))[:, None]
    v = np.asarray(V, np.float64)[:, None]
    return lt["Base"].astype(np.float64) + lt["Edge0"].astype(np.float64) * (s * (1 - v)) + lt["Edge1"].astype(np.float64) * (s * v)


# ---- reservoir frames ------------------------------------------------------------------------------------------------------------
def as_frame(res, H, W):
    """a downloaded DI_RESERVOIR array -> dict of [H, W] arrays (float64 / int64), LightIndex -1 = empty"""
    out = {k: res[k].reshape(H, W).astype(np.float64 if res.dtype[k].kind == "f" else np.int64) for k in res.dtype.names}
    out["LightIndex"] = np.where(res["LightIndex"].reshape(H, W) == 0xFFFFFFFF, -1, out["LightIndex"])
    out.setdefault("Visibility", np.zeros((H, W), np.int64))
    return out


def _empty(out, c, M):
    for k in FIELDS:
        out[k][c] = 0
    out["LightIndex"][c], out["M"][c] = -1, M


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
                _empty(out, c, samples)
                emptied[c] = True
    return out, margin, emptied


def temporal_pass(cur, prev, mv, fresh, in_margin, history, lights, frame, bsdf, max_history, basic, boiling, strength, occ=None,
                  raytraced=False, depth_thr=0.1, normal_thr=0.5, stats=None):
    """restirref.temporal_pass on frames, plus: a selected history sample takes the history pixel's Visibility moved by (hx - x, hy - y) and
    one frame older; raytraced (with basic): p at the previous surface := 0 when the ray from the current surface to the selected
    sample is blocked, traced only when a history pixel was found and that p > 0. history None: no history. stats["zeroed"] counts the
    zeroed terms. Returns (frame, margin)."""
    H, W = cur.H, cur.W
    out = {k: np.zeros((H, W), np.float64 if k in ("U", "V", "W", "TargetPdf") else np.int64) for k in FIELDS}
    out["LightIndex"][:] = -1
    margin = np.array(in_margin, np.float64).copy()
    found = {}
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x]:
                margin[y, x] = np.inf
                continue
            for k in ("LightIndex", "U", "V", "W", "M", "TargetPdf"):
                out[k][y, x] = fresh[k][y, x]
            if history is None:
                continue
            rng = R.Rng(x, y, frame, R.SALT_TEMPORAL)
            mvx, mvy, mvz = (np.float32(v) for v in mv[y, x, :3])
            expected = np.float32(np.float32(cur.depth[y, x]) + mvz)
            for c in (np.float32(x) + mvx, np.float32(y) + mvy):
                margin[y, x] = min(margin[y, x], abs(abs(float(c) - np.floor(float(c))) - 0.5))
            a = cur.material(y, x)
            for qx, qy in R.temporal_candidates(x, y, (mvx, mvy), W, H, rng):
                if not (0 <= qx < W and 0 <= qy < H) or not prev.valid[qy, qx]:
                    continue
                b = prev.material(qy, qx)
                margin[y, x] = min(margin[y, x], R._margin(np.dot(a["Normal"], b["Normal"]), normal_thr),
                                   R._margin(abs(float(expected) - b["Depth"]), depth_thr * max(float(expected), b["Depth"])),
                                   R._margin(abs(a["Roughness"] - b["Roughness"]), 0.5 * max(a["Roughness"], b["Roughness"])),
                                   R._margin(abs(R.LUMA @ a["F0"] - R.LUMA @ b["F0"]), 0.25),
                                   R._margin(abs(R.LUMA @ a["Albedo"] - R.LUMA @ b["Albedo"]), 0.25))
                if R.neighbour_ok(a, b, float(expected), normal_thr, depth_thr):
                    found[(y, x)] = (qy, qx, rng.next())
                    break
    keys = list(found)
    Hs = [{k: history[k][qy, qx] for k in FIELDS} for (qy, qx, _) in found.values()]
    mH = []
    pH = R.target_pdfs(cur, keys, lights, [h["LightIndex"] for h in Hs], [h["U"] for h in Hs], [h["V"] for h in Hs], bsdf, mH)
    for k, m in zip(keys, mH):
        margin[k] = min(margin[k], m)
    sel_from_h = {}
    for (y, x), h, ph in zip(keys, Hs, pH):
        mcur = int(out["M"][y, x])
        mh = min(int(h["M"]), max_history * mcur)
        w0 = out["TargetPdf"][y, x] * out["W"][y, x] * mcur
        wH = ph * float(h["W"]) * mh
        wsum = w0 + wH
        rc = float(found[(y, x)][2])
        margin[y, x] = min(margin[y, x], R._margin(rc * wsum, wH) if wH > 0 else np.inf)
        fromH = rc * wsum < wH
        if fromH:
            qy, qx = found[(y, x)][:2]
            out["LightIndex"][y, x], out["U"][y, x], out["V"][y, x] = int(h["LightIndex"]), float(h["U"]), float(h["V"])
            out["TargetPdf"][y, x], out["Age"][y, x] = ph, int(h["Age"]) + 1
            out["Visibility"][y, x] = carry(int(h["Visibility"]), qx - x, qy - y, 1)
        out["M"][y, x] = mcur + mh
        sel_from_h[(y, x)] = (fromH, mh, wsum, mcur)
    need = [(y, x) for (y, x) in sel_from_h if out["TargetPdf"][y, x] > 0]
    mP = []
    pprev = R.target_pdfs(prev, [(found[k][0], found[k][1]) for k in need], lights, [out["LightIndex"][k] for k in need],
                          [out["U"][k] for k in need], [out["V"][k] for k in need], bsdf, mP) if basic else []
    for k, m in zip(need, mP):
        margin[k] = min(margin[k], m)
    pprev = dict(zip(need, pprev))
    if basic and raytraced:
        rays = [k for k in need if pprev[k] > 0]
        if rays:
            ys, xs = np.array(rays).T
            blocked, _, m = occ.trace(cur.P[ys, xs], sample_points(lights, out["LightIndex"][ys, xs], out["U"][ys, xs], out["V"][ys, xs]))
            for k, b, mm in zip(rays, blocked, m):
                margin[k] = min(margin[k], mm)
                if b:
                    pprev[k] = 0.0
                    if stats is not None:
                        stats["zeroed"] = stats.get("zeroed", 0) + 1
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x] or history is None:
                continue
            p = out["TargetPdf"][y, x]
            if not p > 0:
                _empty(out, (y, x), out["M"][y, x])
                continue
            fromH, mh, wsum, mcur = sel_from_h.get((y, x), (False, 0, None, int(out["M"][y, x])))
            if wsum is None:
                wsum = p * out["W"][y, x] * mcur
            if basic:
                pp = pprev.get((y, x), 0.0)
                den = p * (mcur * p + mh * pp)
                out["W"][y, x] = wsum * (pp if fromH else p) / den if den > 0 else 0.0
            else:
                out["W"][y, x] = wsum / (p * out["M"][y, x])
    if boiling:
        for ty in range(0, H, 8):
            for tx in range(0, W, 8):
                Wt = np.zeros(64, np.float32); vt = np.zeros(64, bool); idx = []
                for ln in range(64):
                    y, x = ty + ln // 8, tx + ln % 8
                    if y < H and x < W:
                        Wt[ln], vt[ln] = out["W"][y, x], cur.valid[y, x]
                        idx.append((ln, y, x))
                nz = vt & (Wt > 0)
                total, count = R.butterfly_sum(np.where(nz, Wt, 0)), R.butterfly_sum(nz.astype(np.float32))
                if not count > 0:
                    continue
                mul = np.float32(np.float32(10.0) / np.float32(min(max(strength, 1e-6), 1.0))) - np.float32(9.0)
                thr = float(np.float32(total / count) * mul)
                for ln, y, x in idx:
                    if nz[ln]:
                        margin[y, x] = min(margin[y, x], R._margin(float(Wt[ln]), thr))
                        if Wt[ln] > thr:
                            _empty(out, (y, x), 0)
                tmin = min((margin[y, x] for _, y, x in idx), default=np.inf)
                if tmin < 1e-5:
                    for _, y, x in idx:
                        margin[y, x] = min(margin[y, x], tmin)
    return out, margin


def spatial_pass(cur, inp, in_margin, lights, table, frame, bsdf, samples, boost, max_history, radius, basic, occ=None, raytraced=False,
                 depth_thr=0.1, normal_thr=0.5, stats=None):
    """restirref.spatial_pass on frames, plus: a selected neighbour's sample takes its Visibility moved by (qx - x, qy - y); raytraced (with
    basic): in the normalisation a contributing neighbour's p := 0 when the ray from that neighbour's surface to the selected sample is
    blocked (traced only when that p > 0; the centre's own term is not tested). Returns (frame, margin)."""
    H, W = cur.H, cur.W
    out = {k: np.array(inp[k]).copy() for k in FIELDS}
    margin = np.array(in_margin, np.float64).copy()
    plan = {}
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x]:
                continue
            rng = R.Rng(x, y, frame, R.SALT_SPATIAL)
            start = int(np.float32(rng.next()) * np.float32(8191.0))
            n = max(samples, boost) if inp["M"][y, x] < max_history else samples
            a = cur.material(y, x)
            nb = []
            for i in range(n):
                e = table[(start + i) & 8191]
                qx, qy = R.reflect(x + R.spatial_offset(int(e[0]), radius), y + R.spatial_offset(int(e[1]), radius), W, H)
                if not (0 <= qx < W and 0 <= qy < H) or not cur.valid[qy, qx]:
                    continue
                b = cur.material(qy, qx)
                margin[y, x] = min(margin[y, x], R._margin(np.dot(a["Normal"], b["Normal"]), normal_thr),
                                   R._margin(abs(a["Depth"] - b["Depth"]), depth_thr * max(a["Depth"], b["Depth"])),
                                   R._margin(abs(a["Roughness"] - b["Roughness"]), 0.5 * max(a["Roughness"], b["Roughness"])),
                                   R._margin(abs(R.LUMA @ a["F0"] - R.LUMA @ b["F0"]), 0.25),
                                   R._margin(abs(R.LUMA @ a["Albedo"] - R.LUMA @ b["Albedo"]), 0.25))
                if R.neighbour_ok(a, b, a["Depth"], normal_thr, depth_thr):
                    nb.append((qy, qx, rng.next()))
                    margin[y, x] = min(margin[y, x], in_margin[qy, qx])
            plan[(y, x)] = nb
    pairs = [((y, x), (qy, qx)) for (y, x), nb in plan.items() for (qy, qx, _) in nb]
    mN = []
    pn = R.target_pdfs(cur, [c for c, _ in pairs], lights, [inp["LightIndex"][q] for _, q in pairs], [inp["U"][q] for _, q in pairs],
                       [inp["V"][q] for _, q in pairs], bsdf, mN)
    for (c, _), m in zip(pairs, mN):
        margin[c] = min(margin[c], m)
    pn = iter(pn)
    sel = {}
    for (y, x), nb in plan.items():
        c = (y, x)
        wsum = inp["TargetPdf"][c] * inp["W"][c] * inp["M"][c]
        M, s = int(inp["M"][c]), -1
        for i, (qy, qx, rc) in enumerate(nb):
            p = next(pn)
            w = p * inp["W"][qy, qx] * inp["M"][qy, qx]
            wsum += w; M += int(inp["M"][qy, qx])
            if w > 0:
                margin[c] = min(margin[c], R._margin(float(rc) * wsum, w))
            if float(rc) * wsum < w:
                s = i
                for k in ("LightIndex", "U", "V", "Age"):
                    out[k][c] = inp[k][qy, qx]
                out["TargetPdf"][c] = p
                out["Visibility"][c] = carry(int(inp["Visibility"][qy, qx]), qx - x, qy - y, 0)
        out["M"][c] = M
        sel[c] = (s, wsum)
    pc = {}
    if basic:
        q = [((y, x), (qy, qx)) for (y, x), nb in plan.items() if out["TargetPdf"][y, x] > 0 for (qy, qx, _) in nb]
        mC = []
        vals = R.target_pdfs(cur, [n for _, n in q], lights, [out["LightIndex"][c] for c, _ in q], [out["U"][c] for c, _ in q],
                             [out["V"][c] for c, _ in q], bsdf, mC)
        for (c, _), m in zip(q, mC):
            margin[c] = min(margin[c], m)
        vals = list(vals)
        if raytraced:
            rays = [j for j, v in enumerate(vals) if v > 0]
            if rays:
                cs = np.array([q[j][0] for j in rays]); ns = np.array([q[j][1] for j in rays])
                blocked, _, m = occ.trace(cur.P[ns[:, 0], ns[:, 1]],
                                          sample_points(lights, out["LightIndex"][cs[:, 0], cs[:, 1]], out["U"][cs[:, 0], cs[:, 1]], out["V"][cs[:, 0], cs[:, 1]]))
                for j, b, mm in zip(rays, blocked, m):
                    margin[q[j][0]] = min(margin[q[j][0]], mm)
                    if b:
                        vals[j] = 0.0
                        if stats is not None:
                            stats["zeroed"] = stats.get("zeroed", 0) + 1
        vals = iter(vals)
        for (y, x), nb in plan.items():
            if out["TargetPdf"][y, x] > 0:
                pc[(y, x)] = [next(vals) for _ in nb]
    for (y, x), nb in plan.items():
        c = (y, x)
        p = out["TargetPdf"][c]
        s, wsum = sel[c]
        if not p > 0:
            _empty(out, c, out["M"][c])
            continue
        if basic:
            den, psrc = inp["M"][c] * p, p
            for i, ((qy, qx, _), pq) in enumerate(zip(nb, pc[c])):
                den += inp["M"][qy, qx] * pq
                if i == s:
                    psrc = pq
            den *= p
            out["W"][c] = wsum * psrc / den if den > 0 else 0.0
        else:
            out["W"][c] = wsum / (p * out["M"][c])
    return out, margin


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
                _empty(out, c, out["M"][c])
                info["discarded"][c] = True
    return out, margin, info
