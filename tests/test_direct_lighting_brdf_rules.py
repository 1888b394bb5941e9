"""BRDF candidates of the DI pass's initial sampling, the rules ("BRDF candidates"), no GPU: RandomFromBarycentrics
against Math::SampleTriangle, the degenerate mixes of the blended pdf in exact rationals, and the inputs of the GPU pins -- the scene, the
oracle replay and the float64 restatement (tests/brdfcandref.py) -- checked for being fit to pin anything."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import brdfcandref as B
import brdfscene
import bsdfref
import restirref as R
import visscene

EPS = 2.0 ** -24


def test_random_from_barycentrics_inverts_sample_triangle():
    """On a grid of (U, V): SampleTriangle's barycentrics of vertices 1 and 2, in the device's float32 steps (sqrt(U) (1 - V), sqrt(U) V),
    go back to (U, V) through t = b1 + b2, U' = t t, V' = b2 / t. Each of the five float32 operations on the way rounds once, so both come
    back within 8 * 2^-24 relative; t = 0 (U = 0) gives (0, 0), which is the same point, the base vertex."""
    g = np.linspace(0.0, 1.0, 33, endpoint=False, dtype=np.float32)
    U, V = (a.reshape(-1) for a in np.meshgrid(np.concatenate([g, np.float32([1e-12, 1e-6, 1 - 2.0 ** -24])]), np.concatenate([g, np.float32([1e-7, 1 - 2.0 ** -24])])))
    sq = np.sqrt(U)
    b1, b2 = (sq * (np.float32(1) - V)).astype(np.float32), (sq * V).astype(np.float32)
    U2, V2 = B.random_from_barycentrics(b1, b2)
    zero = (b1 + b2) == 0
    assert zero.any() and (U2[zero] == 0).all() and (V2[zero] == 0).all() and (U[zero] == 0).all()
    nz = ~zero
    assert (np.abs(U2[nz].astype(np.float64) - U[nz]) <= 8 * EPS * U[nz]).all()
    assert (np.abs(V2[nz].astype(np.float64) - V[nz]) <= 8 * EPS * V[nz]).all()
    assert U2.dtype == np.float32 and V2.dtype == np.float32


@pytest.mark.parametrize("tri", [((0, 0, 0), (1, 0, 0), (0, 1, 0)), ((-1.2, 1.2, -0.6), (1.2, 1.2, -0.6), (1.2, 1.2, 1.4)),
                                 ((100.5, -3.25, 7.0), (100.75, -3.0, 7.5), (99.0, -2.0, 6.0)), ((1e-3, 2e-3, 0), (3e-3, 2e-3, 1e-3), (1e-3, 5e-3, 2e-3))])
def test_rederived_point_is_the_hit_point(tri):
    """A hit (b1, b2) on a hand-made triangle, turned into (U, V) and back into a point the way di_target does it (float32: sqrt, two
    products, base + e0 b0 + e1 b1), lands on the hit point. Bound: every coordinate is a sum of three terms no larger than the
    triangle's extent E = max |base| + max |e0| + max |e1|, formed in about ten float32 roundings: 16 * 2^-24 * E."""
    p = np.array(tri, np.float32)
    base, e0, e1 = p[0], (p[1] - p[0]).astype(np.float32), (p[2] - p[0]).astype(np.float32)
    E = float(np.abs(base).max() + np.abs(e0).max() + np.abs(e1).max())
    rng = np.random.default_rng(5)
    b1 = rng.random(2000).astype(np.float32); b2 = (rng.random(2000) * (1 - b1)).astype(np.float32)
    b1[:4], b2[:4] = (0, 1, 0, 0.5), (0, 0, 1, 0.5)
    hit = base.astype(np.float64) + e0.astype(np.float64) * b1[:, None].astype(np.float64) + e1.astype(np.float64) * b2[:, None].astype(np.float64)
    U, V = B.random_from_barycentrics(b1, b2)
    sq = np.sqrt(U)
    c0, c1 = (sq * (np.float32(1) - V)).astype(np.float32), (sq * V).astype(np.float32)
    pos = ((base + (e0 * c0[:, None]).astype(np.float32)).astype(np.float32) + (e1 * c1[:, None]).astype(np.float32)).astype(np.float32)
    err = np.abs(pos.astype(np.float64) - hit).max()
    print(f"extent {E:.4g}: max |re-derived - hit| = {err:.3e} (bound {16 * EPS * E:.3e})")
    assert err <= 16 * EPS * E


def test_all_brdf_candidates_missing_exact():
    """N_L = 2, N_B = 1 and the BRDF ray misses: only the two light candidates carry weight. In exact rationals, W of the mix is the
    light-only W times N_L / N times the change of the per-candidate weights, sum w' / sum w; and where the BRDF pdf is 0 at both samples
    every w' is N / N_L times w, so W is the light-only W itself."""
    p, ql = [Fr(3, 7), Fr(5, 11)], [Fr(1, 4), Fr(3, 4)]
    qb, sa = [Fr(2, 3), Fr(9, 5)], [Fr(7, 2), Fr(1, 6)]
    coins = [Fr(1, 2), Fr(1, 3)]
    w = [pi / qi for pi, qi in zip(p, ql)]
    sel0, ws0, _ = B.stream(w, coins, None)
    W0 = B.reservoir_weight(ws0, 2, p[sel0])
    for qbs in (qb, [Fr(0), Fr(0)]):
        w2 = [pi / B.blended_pdf(2, 1, qi, b, s) for pi, qi, b, s in zip(p, ql, qbs, sa)] + [Fr(0)]     # the third candidate: the missing BRDF ray
        sel, ws, _ = B.stream(w2, coins + [Fr(9, 10)], None)
        if sel != sel0:
            continue                                                      # another selection: another p in W (not this identity)
        W = B.reservoir_weight(ws, 3, p[sel])
        assert W == W0 * Fr(2, 3) * (sum(w2) / sum(w))
        if qbs[0] == 0:
            assert all(a == Fr(3, 2) * b for a, b in zip(w2, w)) and W == W0
    # the blended weights themselves, written out
    assert w2[0] == p[0] / (Fr(2) * ql[0] / 3)
    assert B.blended_pdf(2, 1, ql[0], qb[0], sa[0]) == (2 * ql[0] + qb[0] / sa[0]) / 3
    assert B.blended_pdf(2, 1, ql[0], qb[0], Fr(0)) == 2 * ql[0] / 3           # pdfSA not positive: the light term alone
    assert B.blended_pdf(2, 1, ql[0], qb[0], float("inf")) == 2 * ql[0] / 3


def test_blended_pdf_is_the_balance_heuristic():
    """One light, known pdfs. A candidate's share of the estimate, w / N, is the balance heuristic's: p / (N_L q_L + N_B q_B') with q_B' the
    BRDF pdf in the light's measure, i.e. the technique's MIS weight times its own single-technique term. With q_B / pdfSA = q_L both
    techniques draw the sample with the same density and every weight is p / q_L whatever N_L : N_B."""
    p, ql, qb, sa = Fr(4, 9), Fr(1, 1), Fr(6, 5), Fr(3, 10)
    for nl, nb in ((8, 1), (1, 1), (2, 4), (1, 8)):
        w = p / B.blended_pdf(nl, nb, ql, qb, sa)
        qbl = qb / sa
        assert w / (nl + nb) == p / (nl * ql + nb * qbl)
        assert w / (nl + nb) == (nl * ql / (nl * ql + nb * qbl)) * (p / (nl * ql))           # light technique: MIS weight x p / (N_L q_L)
        assert w / (nl + nb) == (nb * qbl / (nl * ql + nb * qbl)) * (p / (nb * qbl))         # BRDF technique, same sample
        assert p / B.blended_pdf(nl, nb, ql, ql * sa, sa) == p / ql
    # the cutoff: beyond sqrt((1 / c - 1) q_B) the BRDF pdf counts as 0
    c = 0.25
    rng = float(np.sqrt(3.0 * 1.2))
    assert B.blended_pdf(2, 1, 1.0, 1.2, 0.3, dist=rng * 1.01, cutoff=c) == 2 * 1.0 / 3
    assert B.blended_pdf(2, 1, 1.0, 1.2, 0.3, dist=rng * 0.99, cutoff=c) == (2 * 1.0 + 1.2 / 0.3) / 3
    assert float(B.brdf_range(c, 1.2)) == pytest.approx(rng, rel=1e-6)


def test_streams_and_tables():
    """the BRDF stream is its own (salt 0x44490008): five draws per candidate, none of them the light stream's; the prefix sum's last
    entry is the total and a draw at or past the total selects a light of positive power"""
    a = B.brdf_draws(5, 7, 3, 2)
    rng = R.Rng(5, 7, 3, R.SALT_INITIAL)
    b = np.array([rng.next() for _ in range(10)], np.float32)
    assert a.shape == (2, 5) and ((a >= 0) & (a < 1)).all() and not np.array_equal(a.reshape(-1), b)
    rng = R.Rng(5, 7, 3, B.SALT_BRDF)
    assert np.array_equal(a.reshape(-1), np.array([rng.next() for _ in range(10)], np.float32))
    power = np.float32([0.5, 0.0, 2.25, 1e-3, 7.0, 0.0])
    cdf, total = B.power_cdf(power)
    assert cdf[-1] == total and abs(float(total) - float(power.astype(np.float64).sum())) < 1e-5
    assert B.select_light(cdf, np.float32(0.0), total) == 0 and B.select_light(cdf, total, total) == 4
    assert B.select_light(cdf, np.float32(0.5), total) == 2                 # the light of zero power never qualifies


def test_layouts_mirror_the_header(pkg, ptamd):
    """the numpy records of the setter's arguments and of a downloaded candidate (four 32-bit words, the header's order), the reference's default of one
    BRDF candidate with unbounded rays, and the two entry points among the exports the build checks"""
    L = pkg.layouts
    assert L.DI_BRDF_SETTINGS.itemsize == 16 and L.DI_BRDF_CANDIDATE.itemsize == 16 and B.CANDIDATE.itemsize == 16
    assert [L.DI_BRDF_SETTINGS.fields[k][1] for k in ("BrdfSamples", "BrdfCutoff")] == [0, 4]
    assert [L.DI_BRDF_CANDIDATE.fields[k][1] for k in ("LightIndex", "U", "V", "BrdfPdf")] == [0, 4, 8, 12]
    s = L.di_brdf_settings()
    assert int(s["BrdfSamples"]) == 1 and float(s["BrdfCutoff"]) == 0.0 and s.tobytes()[8:] == bytes(8)
    assert {"pt_di_set_brdf_sampling", "pt_di_download_brdf_candidates"} <= set(ptamd.EXPORTS)


@pytest.fixture(scope="module")
def pin_inputs(pkg, oracle):
    """the GPU pins' inputs from the CPU alone: the glossy scene's G-buffer by the oracle, its float32 and float64 surfaces, its lights"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = brdfscene.glossy_scene(S, W / H)
    gb, osc = brdfscene.oracle_gbuffer(oracle, L, scene, W, H)
    lights = visscene.host_lights(scene, L)
    yield scene, gb, osc, lights, B.surfaces_f32(gb, scene.camera), R.Surfaces(gb, scene.camera)
    osc.close()


def test_inputs_fit_for_the_gpu_pin(pin_inputs, oracle):
    """Conditions on the inputs, not measurements: (a) at least 10 % of the valid pixels have a BRDF candidate that lands on a light;
    (b) pixels within 1e-5 of a decision stay under 5 % of the valid pixels, for each case of the reservoir pin; (c) with the positive
    cutoff some rays reach a light inside their range and some would have reached one beyond it."""
    scene, gb, osc, lights, sf, S64 = pin_inputs
    bsdf = bsdfref.Reference()
    frame = 40
    valid = sf["valid"]
    assert np.array_equal(valid, S64.valid) and valid.sum() > 0.5 * valid.size
    assert np.abs(sf["P"].astype(np.float64) - S64.P)[valid].max() < 1e-5 and np.abs(sf["V"].astype(np.float64) - S64.V)[valid].max() < 1e-5
    assert len(lights) == 3
    rec, info = B.replay_candidates(oracle, osc, sf, lights, frame, 1, 0.0)
    on_light = (rec["LightIndex"] != 0xFFFFFFFF).any(-1)
    frac = on_light[valid].mean()
    print(f"(a) {frac:.1%} of {valid.sum()} valid pixels have a BRDF candidate on a light; on other geometry "
          f"{((info['stopped'] >= 0).any(-1) & ~on_light)[valid].mean():.1%}")
    assert frac >= 0.10
    assert not on_light[~valid].any() and (rec["BrdfPdf"][~valid] == 0).all()
    assert ((info["stopped"] >= 0).any(-1) & ~on_light)[valid].any()        # and some stop on the floor or the bar
    lit = rec["LightIndex"] != 0xFFFFFFFF
    assert ((rec["U"][lit] > 0) & (rec["U"][lit] <= 1.0 + 1e-6) & (rec["V"][lit] >= 0) & (rec["V"][lit] <= 1)).all()
    # the re-derived point of a record is the oracle's hit point: P + t L, to the float32 rounding of both
    ys, xs, js = np.nonzero(lit)
    pos = R.sample_points(lights, rec["LightIndex"][lit], rec["U"][lit], rec["V"][lit])
    dist = np.linalg.norm(pos - S64.P[ys, xs], axis=-1)
    assert np.abs(dist - info["t"][lit]).max() < 1e-4
    for n_l, n_b, source, cutoff in ((8, 1, "cdf", 0.0), (1, 1, "uniform", 0.0), (2, 4, "cdf", brdfscene.CUTOFF)):
        r, _ = B.replay_candidates(oracle, osc, sf, lights, frame, n_b, cutoff)
        out, margin = B.initial_sampling(S64, lights, r, frame, n_l, n_b, cutoff, source, bsdf)
        near = (margin < 1e-5) & valid
        print(f"(b) ({n_l}, {n_b}) {source} cutoff {cutoff}: {near.sum()} of {valid.sum()} pixels within 1e-5 of a decision; "
              f"{(out['LightIndex'][valid] >= 0).mean():.1%} reservoirs hold a sample")
        assert near.sum() < 0.05 * valid.sum()
        assert (out["M"][valid] == n_l + n_b).all() and (out["M"][~valid] == 0).all()
        assert (out["LightIndex"][valid] >= 0).mean() > 0.5 and np.isfinite(out["W"]).all() and (out["W"] >= 0).all()
    rc, ic = B.replay_candidates(oracle, osc, sf, lights, frame, 1, brdfscene.CUTOFF)
    inside, outside = int((rc["LightIndex"] != 0xFFFFFFFF).sum()), int(ic["beyond"].sum())
    print(f"(c) cutoff {brdfscene.CUTOFF}: {inside} rays reach a light inside their range, {outside} would have reached one beyond it")
    assert inside > 20 and outside > 20
    # inside the range the candidate is the unbounded ray's
    same = rc["LightIndex"] != 0xFFFFFFFF
    assert np.array_equal(rc[same], rec[same])
    assert (B.brdf_range(brdfscene.CUTOFF, rc["BrdfPdf"][same]) > ic["t"][same]).all()


def test_pane_scene_has_both_outcomes(pkg, oracle):
    """the alpha-masked pane between the floor and the emitter: rays go through its holes to the light and stop on its texels"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = brdfscene.glossy_scene(S, W / H, pane=True, bar=False)
    gb, osc = brdfscene.oracle_gbuffer(oracle, L, scene, W, H)
    lights = visscene.host_lights(scene, L)
    sf = B.surfaces_f32(gb, scene.camera)
    rec, info = B.replay_candidates(oracle, osc, sf, lights, 40, 1, 0.0)
    osc.close()
    pane = len(scene.objects) - 1
    floor_px = sf["valid"] & (np.abs(sf["P"][..., 1]) < 1e-3)
    through = (rec["LightIndex"][..., 0] < 2) & floor_px
    stopped = (info["stopped"][..., 0] == pane) & floor_px
    print(f"pane: {through.sum()} floor rays reach the quad light, {stopped.sum()} stop on the pane")
    assert through.sum() > 20 and stopped.sum() > 20
