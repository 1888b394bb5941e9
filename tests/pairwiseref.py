"""Float64 restatement of Pairwise bias correction in the DI reuse passes ("Pairwise bias correction"): the
pairwise MIS weights, the temporal step (the fresh reservoir is the canonical domain, the history the one neighbour) and the spatial
step (neighbours streamed in slot order, the centre merged last), and the two passes over whole frames for the per-pixel pins. The
search, the neighbour tests, the streams, the boiling filter, the Visibility word and the reservoir frames are restirref's.

The scalar rules take any exact or floating arithmetic (the enumerations of test_direct_lighting_pairwise_rules.py feed Fractions)."""
import numpy as np

import restirref as R
from restirref import FIELDS, LUMA, Rng, SALT_SPATIAL, SALT_TEMPORAL, _margin, carry, empty, target_pdfs


# ---- the weights -----------------------------------------------------------------------------------------------------------------
def neighbour_share(n, Mi, pi, Mc, pc):
    """a / D with a = n M_i p_i(y), b = M_c p_c(y), D = a + b; D = 0 counts as 0. m_i(y) is this over (n + 1)."""
    a, b = n * Mi * pi, Mc * pc
    D = a + b
    return a / D if D > 0 else D * 0                                      # (a zero of the arithmetic in use)


def canonical_share(n, Mi, pi, Mc, pc):
    """b / D of the same pair: what neighbour i leaves the canonical sample"""
    a, b = n * Mi * pi, Mc * pc
    D = a + b
    return b / D if D > 0 else D * 0


def mis_weights(n, Mc, pc, contributing):
    """the weights of one sample y over n attempted slots: pc = p_c(y), contributing = [(M_i, p_i(y))] of the k <= n slots that
    contribute. Returns (m_c, [m_i]): slots that do not contribute give their share to the canonical sample."""
    k = len(contributing)
    m_c = (1 + (n - k) + sum(canonical_share(n, Mi, pi, Mc, pc) for Mi, pi in contributing)) / (n + 1)
    return m_c, [neighbour_share(n, Mi, pi, Mc, pc) / (n + 1) for Mi, pi in contributing]


# ---- the two steps on scalar reservoirs ------------------------------------------------------------------------------------------
# a reservoir here is (y, W, M); y = None: empty (W = 0)
def temporal_weights(fresh, hist, pc_c, pc_H, pp_c, pp_H):
    """(w_c, w_H) of the temporal step, n = 1: fresh = (y_c, W_c, M_c), hist = (y_H, W_H, M_H) with M_H already capped;
    pc_* = p at the current surface, pp_* = p at the previous surface, of y_c and y_H"""
    (_, Wc, Mc), (_, WH, MH) = fresh, hist
    mH = neighbour_share(1, MH, pp_H, Mc, pc_H) / 2
    mc = (1 + canonical_share(1, MH, pp_c, Mc, pc_c)) / 2
    return mc * pc_c * Wc, mH * pc_H * WH


def temporal_resample(fresh, hist, pc_c, pc_H, pp_c, pp_H, rc):
    """-> (y, W, M, p, from_history). hist None: no history pixel, the fresh reservoir with its W untouched."""
    yc, Wc, Mc = fresh
    if hist is None:
        return yc, Wc, Mc, pc_c, False
    wc, wH = temporal_weights(fresh, hist, pc_c, pc_H, pp_c, pp_H)
    wsum = wc + wH
    from_h = rc * wsum < wH
    y, p = (hist[0], pc_H) if from_h else (yc, pc_c)
    M = Mc + hist[2]
    if not p > 0:
        return None, 0, M, 0, False
    return y, wsum / p, M, p, from_h


def spatial_weights(n, canon, pc_c, neighbours):
    """the resampling weights of the spatial step: canon = (y_c, W_c, M_c), pc_c = p_c(y_c); neighbours = the k contributing slots in
    slot order, each ((y_i, W_i, M_i), p_i(y_i), p_c(y_i), p_i(y_c)). Returns ([w_i], w_c)."""
    _, Wc, Mc = canon
    k = len(neighbours)
    ws, own = [], 0
    for (_, Wi, Mi), pi_i, pc_i, pi_c in neighbours:
        ws.append(neighbour_share(n, Mi, pi_i, Mc, pc_i) / (n + 1) * pc_i * Wi)
        own = own + canonical_share(n, Mi, pi_c, Mc, pc_c)
    return ws, (1 + (n - k) + own) / (n + 1) * pc_c * Wc


def spatial_resample(n, canon, pc_c, neighbours, draws):
    """neighbours first, each with its draw, the canonical sample last with one more: selected iff r * wsum < w_c. k = 0: the canonical
    reservoir unchanged. -> (y, W, M, p, src) with src = the selected slot's position among the contributing ones, or -1: the centre"""
    yc, Wc, Mc = canon
    if not neighbours:
        return yc, Wc, Mc, pc_c, -1
    ws, wc = spatial_weights(n, canon, pc_c, neighbours)
    wsum, M, y, p, src = 0, Mc, None, 0, -1
    for j, (w, ((yi, _, Mi), _, pc_i, _)) in enumerate(zip(ws, neighbours)):
        wsum = wsum + w
        M += Mi
        if draws[j] * wsum < w:
            y, p, src = yi, pc_i, j
    wsum = wsum + wc
    if draws[len(neighbours)] * wsum < wc:
        y, p, src = yc, pc_c, -1
    if not p > 0:
        return None, 0, M, 0, -1
    return y, wsum / p, M, p, src


# ---- the passes over whole frames (restirref's frames and margins) ---------------------------------------------------------------
def _search_margins(a, b, depth_a, normal_thr, depth_thr):
    return min(_margin(np.dot(a["Normal"], b["Normal"]), normal_thr),
               _margin(abs(depth_a - b["Depth"]), depth_thr * max(depth_a, b["Depth"])),
               R.roughness_margin(a["Roughness"], b["Roughness"]),
               _margin(abs(LUMA @ a["F0"] - LUMA @ b["F0"]), 0.25), _margin(abs(LUMA @ a["Albedo"] - LUMA @ b["Albedo"]), 0.25))


def temporal_pass(cur, prev, mv, fresh, history, lights, frame, bsdf, max_history, boiling, strength, depth_thr=0.1, normal_thr=0.5,
                  in_margin=None, stats=None):
    """k_di_initial_temporal's Pairwise reuse over a frame; arguments and results as restirref.temporal_pass. stats["from_history"]
    counts the pixels that took the history's sample."""
    H, W = cur.H, cur.W
    out = {k: np.zeros((H, W), np.float64 if k in ("U", "V", "W", "TargetPdf") else np.int64) for k in FIELDS}
    out["LightIndex"][:] = -1
    margin = np.full((H, W), np.inf) if in_margin is None else np.array(in_margin, np.float64)
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
            rng = Rng(x, y, frame, SALT_TEMPORAL)
            mvx, mvy, mvz = (np.float32(v) for v in mv[y, x, :3])
            expected = float(np.float32(np.float32(cur.depth[y, x]) + mvz))
            for c in (np.float32(x) + mvx, np.float32(y) + mvy):
                margin[y, x] = min(margin[y, x], abs(abs(float(c) - np.floor(float(c))) - 0.5))
            a = cur.material(y, x)
            for qx, qy in R.temporal_candidates(x, y, (mvx, mvy), W, H, rng, stats=stats):
                if not (0 <= qx < W and 0 <= qy < H) or not prev.valid[qy, qx]:
                    continue
                b = prev.material(qy, qx)
                margin[y, x] = min(margin[y, x], _search_margins(a, b, expected, normal_thr, depth_thr))
                if R.neighbour_ok(a, b, expected, normal_thr, depth_thr):
                    found[(y, x)] = (qy, qx, float(rng.next()))
                    break
    keys = list(found)
    at_prev = [(qy, qx) for qy, qx, _ in found.values()]
    Hs = [{k: history[k][q] for k in FIELDS} for q in at_prev]
    hist_sample = ([h["LightIndex"] for h in Hs], [h["U"] for h in Hs], [h["V"] for h in Hs])
    own_sample = ([out["LightIndex"][k] for k in keys], [out["U"][k] for k in keys], [out["V"][k] for k in keys])
    ms = [[], [], []]
    pc_H = target_pdfs(cur, keys, lights, *hist_sample, bsdf, ms[0])
    pp_H = target_pdfs(prev, at_prev, lights, *hist_sample, bsdf, ms[1])
    pp_c = target_pdfs(prev, at_prev, lights, *own_sample, bsdf, ms[2])
    for m in ms:
        for k, v in zip(keys, m):
            margin[k] = min(margin[k], v)
    for k, (qy, qx, rc), h, pcH, ppH, ppc in zip(keys, found.values(), Hs, pc_H, pp_H, pp_c):
        y, x = k
        mcur = int(out["M"][k])
        mh = min(int(h["M"]), max_history * mcur)
        fresh_r = (int(out["LightIndex"][k]), float(out["W"][k]), mcur)
        pcc = float(out["TargetPdf"][k])
        wc, wH = temporal_weights(fresh_r, (int(h["LightIndex"]), float(h["W"]), mh), pcc, pcH, ppc, ppH)
        if wH > 0:
            margin[k] = min(margin[k], _margin(rc * (wc + wH), wH))
        _, Wn, M, p, from_h = temporal_resample(fresh_r, (int(h["LightIndex"]), float(h["W"]), mh), pcc, pcH, ppc, ppH, rc)
        if from_h:
            out["LightIndex"][k], out["U"][k], out["V"][k] = int(h["LightIndex"]), float(h["U"]), float(h["V"])
            out["Age"][k] = int(h["Age"]) + 1
            out["Visibility"][k] = carry(int(h["Visibility"]), qx - x, qy - y, 1)
            if stats is not None:
                stats["from_history"] = stats.get("from_history", 0) + 1
        if p > 0:
            out["TargetPdf"][k], out["W"][k], out["M"][k] = p, Wn, M
        else:
            empty(out, k, M)
    if boiling:
        _boil(cur, out, margin, strength, stats)
    return out, margin


def _boil(cur, out, margin, strength, stats=None):
    """the boiling filter over the frame's 8 x 8 tiles, as restirref.temporal_pass applies it (and counts it: restirref.note_boiling_tile)"""
    H, W = cur.H, cur.W
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
            R.note_boiling_tile(stats, len(idx), count)
            mul = np.float32(np.float32(10.0) / np.float32(min(max(strength, 1e-6), 1.0))) - np.float32(9.0)
            thr = float(np.float32(total / count) * mul)
            for ln, y, x in idx:
                if nz[ln]:
                    margin[y, x] = min(margin[y, x], _margin(float(Wt[ln]), thr))
                    if Wt[ln] > thr:
                        empty(out, (y, x), 0)
                        R.note(stats, "boiling_emptied" if len(idx) == 64 else "boiling_cut_emptied")
            tmin = min((margin[y, x] for _, y, x in idx), default=np.inf)
            if tmin < 1e-5:
                for _, y, x in idx:
                    margin[y, x] = min(margin[y, x], tmin)


def spatial_pass(cur, inp, in_margin, lights, table, frame, bsdf, samples, boost, max_history, radius, depth_thr=0.1, normal_thr=0.5,
                 stats=None):
    """k_di_spatial_shade's Pairwise reuse over a frame; arguments and results as restirref.spatial_pass. stats["from_centre"] /
    ["from_neighbour"] count what the merged pixels selected, stats["slots_left"] the attempted slots that did not contribute."""
    H, W = cur.H, cur.W
    out = {k: np.array(inp[k]).copy() for k in FIELDS}
    margin = np.array(in_margin, np.float64).copy()
    plan = {}
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x]:
                continue
            rng = Rng(x, y, frame, SALT_SPATIAL)
            start = int(np.float32(rng.next()) * np.float32(8191.0))
            n = max(samples, boost) if inp["M"][y, x] < max_history else samples
            a = cur.material(y, x)
            nb = []
            for i in range(n):
                e = table[(start + i) & 8191]
                qx, qy = R.reflect(x + R.spatial_offset(int(e[0]), radius), y + R.spatial_offset(int(e[1]), radius), W, H, stats, "spatial")
                if not (0 <= qx < W and 0 <= qy < H) or not cur.valid[qy, qx]:
                    continue
                b = cur.material(qy, qx)
                margin[y, x] = min(margin[y, x], _search_margins(a, b, a["Depth"], normal_thr, depth_thr))
                if R.neighbour_ok(a, b, a["Depth"], normal_thr, depth_thr):
                    nb.append((qy, qx, float(rng.next())))
                    margin[y, x] = min(margin[y, x], in_margin[qy, qx])
            plan[(y, x)] = (n, nb, float(rng.next()))                       # the centre's draw comes after every neighbour's
    pairs = [(c, (qy, qx)) for c, (_, nb, _) in plan.items() for (qy, qx, _) in nb]
    ms = [[], []]
    pc_i = target_pdfs(cur, [c for c, _ in pairs], lights, [inp["LightIndex"][q] for _, q in pairs], [inp["U"][q] for _, q in pairs],
                       [inp["V"][q] for _, q in pairs], bsdf, ms[0])       # the neighbour's sample at the centre
    pi_c = target_pdfs(cur, [q for _, q in pairs], lights, [inp["LightIndex"][c] for c, _ in pairs], [inp["U"][c] for c, _ in pairs],
                       [inp["V"][c] for c, _ in pairs], bsdf, ms[1])       # the centre's sample at the neighbour
    for m in ms:
        for (c, _), v in zip(pairs, m):
            margin[c] = min(margin[c], v)
    at = 0
    for c, (n, nb, rlast) in plan.items():
        y, x = c
        if not nb:
            continue                                                      # no contributing slot: the centre as it is
        canon = (int(inp["LightIndex"][c]), float(inp["W"][c]), int(inp["M"][c]))
        pcc = float(inp["TargetPdf"][c])
        ns = []
        for j, (qy, qx, _) in enumerate(nb):
            q = (qy, qx)
            ns.append(((int(inp["LightIndex"][q]), float(inp["W"][q]), int(inp["M"][q])), float(inp["TargetPdf"][q]), pc_i[at + j], pi_c[at + j]))
        at += len(nb)
        draws = [rc for _, _, rc in nb] + [rlast]
        ws, wc = spatial_weights(n, canon, pcc, ns)
        run = 0.0
        for w, d in zip(ws + [wc], draws):
            run += w
            if w > 0:
                margin[c] = min(margin[c], _margin(d * run, w))
        _, Wn, M, p, src = spatial_resample(n, canon, pcc, ns, draws)
        if stats is not None:
            stats["slots_left"] = stats.get("slots_left", 0) + n - len(nb)
            key = "from_centre" if src < 0 else "from_neighbour"
            stats[key] = stats.get(key, 0) + (1 if p > 0 else 0)
        if not p > 0:
            empty(out, c, M)
            continue
        if src >= 0:
            qy, qx, _ = nb[src]
            for k in ("LightIndex", "U", "V", "Age"):
                out[k][c] = inp[k][qy, qx]
            out["Visibility"][c] = carry(int(inp["Visibility"][qy, qx]), qx - x, qy - y, 0)
        out["TargetPdf"][c], out["W"][c], out["M"][c] = p, Wn, M
    return out, margin
