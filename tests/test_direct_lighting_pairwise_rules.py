"""CPU checks of Pairwise bias correction in the DI reuse passes: the settings struct and the export against the header, the pairwise MIS
weights as a partition of unity, and exact enumerations of a small discrete world in which the temporal and the spatial step reproduce
the integral and the uncorrected (Off) normalisation does not (tests/pairwiseref.py)."""
import itertools
import os
import re
from fractions import Fraction as F

import numpy as np

import pairwiseref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptamd.h")).read(), flags=re.S)


def test_pairwise_struct_and_export_match_header(pkg, ptamd):
    L = pkg.layouts
    text = _header()
    body = re.search(r"typedef struct PtDIPairwiseSettings \{(.*?)\} PtDIPairwiseSettings;", text, re.S).group(1)
    fields, off = {}, 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        typ, rest = decl.split(None, 1)
        assert typ == "uint32_t"
        for item in rest.split(","):
            name, count = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", item.strip()).groups()
            fields[name] = (off, int(count or 1))
            off += 4 * int(count or 1)
    assert off == 16 == L.PT_DI_PAIRWISE_SETTINGS.itemsize
    assert list(fields) == list(L.PT_DI_PAIRWISE_SETTINGS.names) == ["TemporalPairwise", "SpatialPairwise", "Reserved"]
    for n, (o, count) in fields.items():
        assert L.PT_DI_PAIRWISE_SETTINGS.fields[n][1] == o and L.PT_DI_PAIRWISE_SETTINGS.fields[n][0].itemsize == 4 * count, n
    assert re.search(r"int\s+pt_di_set_pairwise\(PtContext\* ctx, const PtDIPairwiseSettings\* settings\);", text)
    assert "pt_di_set_pairwise" in ptamd.EXPORTS and hasattr(ptamd.load_library(), "pt_di_set_pairwise")
    s = L.di_pairwise_settings()                                           # all off by default
    assert s.tobytes() == bytes(16)
    s = L.di_pairwise_settings(temporal=True, spatial=True)
    assert (int(s["TemporalPairwise"]), int(s["SpatialPairwise"]), s["Reserved"].tolist()) == (1, 1, [0, 0])
    assert L.di_pairwise_settings(spatial=True).tobytes() == bytes([0, 0, 0, 0, 1, 0, 0, 0]) + bytes(8)


def test_weights_are_a_partition_of_unity():
    """random (M, p-hat) sets with zeros, M = 0 neighbours, n in 1..32, k in 0..n: m_c + sum m_i = 1 to 1e-12 wherever p_c(y) > 0 (and M_c > 0:
    a canonical domain without confidence has no say in D, and an empty canonical reservoir carries no sample to weigh)"""
    rng = np.random.default_rng(11)
    seen_zero_p, seen_zero_M, seen_k0, seen_full = 0, 0, 0, 0
    for trial in range(4000):
        n = int(rng.integers(1, 33))
        k = int(rng.integers(0, n + 1))
        Mc = int(rng.integers(1, 200))
        pc = float(rng.random() * 10 ** rng.uniform(-6, 3))
        contributing = []
        for _ in range(k):
            Mi = 0 if rng.random() < 0.15 else int(rng.integers(1, 200))
            pi = 0.0 if rng.random() < 0.2 else float(rng.random() * 10 ** rng.uniform(-6, 3))
            seen_zero_M += Mi == 0; seen_zero_p += pi == 0.0
            contributing.append((Mi, pi))
        m_c, m_i = P.mis_weights(n, Mc, pc, contributing)
        assert abs(m_c + sum(m_i) - 1.0) <= 1e-12, (n, k, Mc, pc, contributing)
        assert m_c >= 1.0 / (n + 1) - 1e-15                                  # the defensive share
        assert all(m == 0 for m, (Mi, pi) in zip(m_i, contributing) if Mi == 0 or pi == 0)
        seen_k0 += k == 0; seen_full += k == n
    assert min(seen_zero_p, seen_zero_M, seen_k0, seen_full) > 20
    # exactly, in rationals
    m_c, m_i = P.mis_weights(3, 2, F(5, 7), [(4, F(1, 3)), (0, F(9)), (6, 0)])
    assert m_c + sum(m_i) == 1 and m_i[1] == 0 and m_i[2] == 0
    assert P.mis_weights(5, 3, F(2), []) == (1, [])                        # k = 0: the whole weight is the canonical sample's
    # a sample the canonical domain cannot produce (p_c = 0) gets nothing from it; the neighbours' shares are what is left
    m_c, m_i = P.mis_weights(2, 3, 0, [(4, F(1, 2)), (5, F(1, 3))])
    assert m_i == [F(1, 3), F(1, 3)]


def test_no_contributing_slot_returns_the_canonical_reservoir():
    assert P.spatial_resample(8, ("y", 0.3712, 24), 1.75, [], [0.9]) == ("y", 0.3712, 24, 1.75, -1)     # W bit for bit, not p W / p
    assert P.spatial_resample(1, (None, 0.0, 8), 0.0, [], [0.1]) == (None, 0.0, 8, 0.0, -1)            # an empty centre stays empty
    assert P.temporal_resample(("y", 0.3712, 8), None, 1.75, 0, 0, 0, 0.0) == ("y", 0.3712, 8, 1.75, False)


def test_selection_follows_the_draws():
    """the history is taken iff rc (w_c + w_H) < w_H; the centre, merged last, iff r wsum < w_c"""
    fresh, hist = ("c", F(2), 1), ("h", F(3), 4)
    wc, wH = P.temporal_weights(fresh, hist, F(1), F(2), F(1, 2), F(3, 2))
    edge = wH / (wc + wH)
    assert P.temporal_resample(fresh, hist, F(1), F(2), F(1, 2), F(3, 2), edge)[0] == "c"
    assert P.temporal_resample(fresh, hist, F(1), F(2), F(1, 2), F(3, 2), edge - F(1, 10 ** 9))[0] == "h"
    y, W, M, p, from_h = P.temporal_resample(fresh, hist, F(1), F(2), F(1, 2), F(3, 2), 0)
    assert (y, M, p, from_h) == ("h", 5, 2, True) and W == (wc + wH) / 2     # no division by M
    canon = ("c", F(2), 2)
    ns = [(("a", F(1), 3), F(2), F(1), F(1, 2)), (("b", F(5), 0), F(2), F(4), F(1)), (("d", F(1, 2), 5), F(1), F(3), F(2))]
    ws, wc = P.spatial_weights(4, canon, F(3, 2), ns)
    assert ws[1] == 0                                                      # an M = 0 neighbour weighs nothing, whatever its W
    total = sum(ws) + wc
    assert P.spatial_resample(4, canon, F(3, 2), ns, [0, 0, 0, 0])[4] == -1                  # the last draw decides for the centre
    assert P.spatial_resample(4, canon, F(3, 2), ns, [0, 0, 0, wc / total])[4] == 2          # at the edge: not the centre
    assert P.spatial_resample(4, canon, F(3, 2), ns, [0, 0, 1, 1])[4] == 0
    y, W, M, p, src = P.spatial_resample(4, canon, F(3, 2), ns, [0, 0, 0, 1])
    assert (y, M, p, src) == ("d", 2 + 3 + 0 + 5, 3, 2) and W == total / 3


# ---- a small discrete world, enumerated -------------------------------------------------------------------------------------------
# Lights 0..3; a domain's initial reservoir is one uniform candidate: (l, W = 1 / q = 4, M) when its p-hat(l) > 0, else empty. The
# confidences M differ from domain to domain (a history that has accumulated, a disoccluded neighbour).
LIGHTS = 4
PHAT = {  # p-hat of each light at each domain's surface; zeros: a light behind the surface
    "c": [F(3, 2), F(2), F(1, 4), F(0)],
    "a": [F(1), F(0), F(5, 2), F(3)],
    "b": [F(0), F(7, 3), F(1, 2), F(1)],
    "prev": [F(2), F(1, 3), F(0), F(4)],
}
TRUTH = sum(PHAT["c"])                                                     # sum_y f(y) with f = p-hat_c


def _initial(domain, light, M):
    return (light, F(LIGHTS), M) if PHAT[domain][light] > 0 else (None, F(0), M)


def _p(domain, y):
    return PHAT[domain][y] if y is not None else F(0)


def _spatial_expectation(n, others, Ms, pairwise):
    """E[p-hat_c(y) W] at the centre over every candidate of every domain and, through its exact probability, every outcome of the
    selection coins (streaming selection takes sample j with probability w_j / sum w)"""
    n = F(n)
    total = F(0)
    for lc, *ls in itertools.product(range(LIGHTS), repeat=1 + len(others)):
        canon = _initial("c", lc, Ms["c"])
        res = [_initial(d, l, Ms[d]) for d, l in zip(others, ls)]
        if pairwise:
            ns = [(r, _p(d, r[0]), _p("c", r[0]), _p(d, canon[0])) for d, r in zip(others, res)]
            if ns:
                ws, wc = P.spatial_weights(n, canon, _p("c", canon[0]), ns)
            else:
                ws, wc = [], _p("c", canon[0]) * canon[1]                  # unchanged: W stays
            outcomes = [(r[0], w) for r, w in zip(res, ws)] + [(canon[0], wc)]
            wsum = sum(w for _, w in outcomes)
            W_of = lambda y: wsum / _p("c", y)
        else:                                                              # Off: w = p_c(y) W M, W = wsum / (p_c(y) sum M)
            outcomes = [(r[0], _p("c", r[0]) * r[1] * r[2]) for r in [canon] + res]
            wsum = sum(w for _, w in outcomes)
            Msum = sum(r[2] for r in [canon] + res)
            W_of = lambda y: wsum / (_p("c", y) * Msum)
        if wsum == 0:
            continue
        for y, w in outcomes:
            if w > 0:
                total += F(1, LIGHTS ** (1 + len(others))) * (w / wsum) * _p("c", y) * W_of(y)
    return total


def test_spatial_pairwise_is_exact_and_off_is_not():
    Ms = {"c": 2, "a": 5, "b": 1}
    for n, others in ((1, ["a"]), (2, ["a", "b"]), (3, ["b", "a"]), (8, ["a", "b"]), (2, [])):     # n > k: slots that did not contribute
        assert _spatial_expectation(n, others, Ms, True) == TRUTH, (n, others)
    assert _spatial_expectation(2, ["a", "b"], {"c": 1, "a": 0, "b": 7}, True) == TRUTH          # an M = 0 neighbour
    off = _spatial_expectation(2, ["a", "b"], Ms, False)
    assert off != TRUTH                                                    # 1 / M counts every domain as a source of every sample
    assert _spatial_expectation(2, [], Ms, False) == TRUTH                 # (nothing reused: nothing to correct)


def _temporal_expectation(Mc, MH, pairwise):
    total = F(0)
    for lc, lh in itertools.product(range(LIGHTS), repeat=2):
        fresh, hist = _initial("c", lc, Mc), _initial("prev", lh, MH)
        if pairwise:
            wc, wH = P.temporal_weights(fresh, hist, _p("c", fresh[0]), _p("c", hist[0]), _p("prev", fresh[0]), _p("prev", hist[0]))
            W_of = lambda y: (wc + wH) / _p("c", y)
        else:
            wc, wH = _p("c", fresh[0]) * fresh[1] * Mc, _p("c", hist[0]) * hist[1] * MH
            W_of = lambda y: (wc + wH) / (_p("c", y) * (Mc + MH))
        if wc + wH == 0:
            continue
        for y, w in ((fresh[0], wc), (hist[0], wH)):
            if w > 0:
                total += F(1, LIGHTS ** 2) * (w / (wc + wH)) * _p("c", y) * W_of(y)
    return total


def test_temporal_pairwise_is_exact_and_off_is_not():
    for Mc, MH in ((1, 1), (8, 20), (8, 160), (3, 0)):
        assert _temporal_expectation(Mc, MH, True) == TRUTH, (Mc, MH)
    assert _temporal_expectation(8, 20, False) != TRUTH
    # and the step itself, through its draw: both outcomes of one pair of candidates carry the weights enumerated above
    fresh, hist = _initial("c", 0, 8), _initial("prev", 1, 20)
    wc, wH = P.temporal_weights(fresh, hist, _p("c", 0), _p("c", 1), _p("prev", 0), _p("prev", 1))
    y0, W0, M0, p0, h0 = P.temporal_resample(fresh, hist, _p("c", 0), _p("c", 1), _p("prev", 0), _p("prev", 1), F(0))
    y1, W1, M1, p1, h1 = P.temporal_resample(fresh, hist, _p("c", 0), _p("c", 1), _p("prev", 0), _p("prev", 1), F(999, 1000))
    assert (y0, h0, y1, h1, M0, M1) == (1, True, 0, False, 28, 28)
    assert W0 == (wc + wH) / _p("c", 1) and W1 == (wc + wH) / _p("c", 0)


def test_empty_canonical_takes_the_neighbours_sample():
    """w_c = 0 for an empty canonical reservoir; what it could have produced is still credited to it (m_i < 1 / (n + 1) ... 1)"""
    canon = (None, F(0), 4)
    ns = [((2, F(4), 6), _p("a", 2), _p("c", 2), F(0))]
    ws, wc = P.spatial_weights(1, canon, F(0), ns)
    assert wc == 0 and ws[0] > 0
    y, W, M, p, src = P.spatial_resample(1, canon, 0, ns, [F(1, 2), F(1, 2)])
    assert (y, M, p, src) == (2, 10, _p("c", 2), 0) and W == ws[0] / _p("c", 2)
    # a neighbour whose sample the centre cannot use leaves an empty reservoir with the summed M
    ns = [((3, F(4), 6), _p("a", 3), _p("c", 3), 0)]
    assert P.spatial_resample(1, canon, 0, ns, [0, 0]) == (None, 0, 10, 0, -1)


# ---- the passes on a synthetic frame ---------------------------------------------------------------------------------------------
def test_frame_passes_keep_what_pairwise_does_not_touch(pkg, oracle):
    """the oracle's G-buffer of the pin scene at 48 x 32 (static camera), a synthetic fresh frame and history: the Pairwise passes find the
    history pixels and neighbours restirref's passes find (the same M everywhere), select only samples their inputs hold, leave a pixel
    without history or without a contributing slot as it was, and leave out no more pixels than the per-pixel GPU pins may."""
    import bsdfref
    import restirref as R
    import visscene
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = visscene.pin_scene(S, W / H)
    gb, _, _ = oracle.render(scene, S.graphics_settings(W, H, spp=1, bounces=0), layouts=L)
    for n in L.DI_PREVIOUS_TEXTURES:
        gb[n] = gb[n[len("Previous"):]]
    bsdf = bsdfref.Reference()
    cur, prev = R.Surfaces(gb, scene.camera), R.Surfaces(gb, scene.camera, previous=True)
    lights = visscene.host_lights(scene, L)
    fresh = visscene.synthetic_frame(cur, lights, bsdf, 1)
    history = visscene.synthetic_frame(cur, lights, bsdf, 2, with_visibility=True)
    history["M"] = np.where(cur.valid, 60, 0)
    mv = np.zeros((H, W, 4), np.float32)
    table = R.offset_table()
    st = {}
    basic, _ = R.temporal_pass(cur, prev, mv, fresh, history, lights, 7, bsdf, 20, True, False, 0.2)
    t, m1 = P.temporal_pass(cur, prev, mv, fresh, history, lights, 7, bsdf, 20, False, 0.2, stats=st)
    assert np.array_equal(t["M"], basic["M"]) and (t["M"] > 8).any()
    took = t["Age"] > 0
    assert st["from_history"] == took.sum() > 0 and (~took & cur.valid & (t["LightIndex"] >= 0)).any()
    for k in ("LightIndex", "U", "V"):
        assert np.array_equal(t[k][took], history[k][took]), k                # static view: the history pixel is the pixel itself
        keep = cur.valid & ~took & (t["LightIndex"] >= 0)
        assert np.array_equal(t[k][keep], fresh[k][keep]), k
    assert (t["W"][cur.valid & (t["LightIndex"] >= 0)] > 0).all() and np.isfinite(t["W"]).all()
    none, _ = P.temporal_pass(cur, None, mv, fresh, None, lights, 7, bsdf, 20, False, 0.2)
    for k in ("LightIndex", "U", "V", "W", "M", "TargetPdf"):
        assert np.array_equal(none[k][cur.valid], fresh[k][cur.valid]), k          # no history: W untouched
    st = {}
    bs, _ = R.spatial_pass(cur, t, m1, lights, table, 7, bsdf, 2, 8, 20, 32.0, True)
    s, m2 = P.spatial_pass(cur, t, m1, lights, table, 7, bsdf, 2, 8, 20, 32.0, stats=st)
    assert np.array_equal(s["M"], bs["M"])
    assert st["from_centre"] > 0 and st["from_neighbour"] > 0 and st["slots_left"] > 0
    alone = cur.valid & (s["M"] == t["M"])                                 # no contributing slot
    for k in R.FIELDS:
        assert np.array_equal(s[k][alone], t[k][alone]), k
    lit = cur.valid & (s["LightIndex"] >= 0)
    assert (s["W"][lit] > 0).all() and np.isfinite(s["W"]).all()
    excluded, compared = int((cur.valid & (m2 < 1e-5)).sum()), int((cur.valid & (m2 >= 1e-5)).sum())
    print(f"{compared} compared, {excluded} within 1e-5 of a decision ({excluded / cur.valid.sum():.2%} of valid), exercised {st}")
    assert excluded < 0.25 * (compared + excluded) and compared > 0.3 * W * H
