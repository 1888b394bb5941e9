"""CPU checks of reservoir reuse: the new C structs against their numpy layouts, the neighbour-offset table, and the float64
restatement of the rules (tests/restirref.py), including mutations of the spec that it must tell apart."""
import os
import re

import numpy as np

import restirref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields, off = {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = decl.split(None, 1)
        size = {"float": 4, "uint32_t": 4, "void*": 8}[typ]
        for item in rest.split(","):
            m = re.match(r"\*?\s*(\w+)(?:\[(\d+)\])?", item.strip())
            n = int(m.group(2) or 1)
            fields[m.group(1)] = (off, n)
            off += size * n
    return fields, off


def test_reuse_struct_layouts_match_header(pkg):
    L = pkg.layouts
    for dt, cname in ((L.DI_RESAMPLING_SETTINGS, "PtDIResamplingSettings"), (L.DI_RESERVOIR, "PtDIReservoir")):
        fields, size = _header_struct(cname)
        assert dt.itemsize == size, cname
        for name, (off, n) in fields.items():
            if name.startswith("_"):
                continue
            assert dt.fields[name][1] == off, (cname, name)
    fields, size = _header_struct("PtDIPreviousTextures")
    assert size == 48 and list(fields) == L.DI_PREVIOUS_TEXTURES


def test_resampling_defaults(pkg):
    s = pkg.layouts.di_resampling_settings()
    assert (int(s["TemporalResampling"]), int(s["TemporalBiasCorrection"]), int(s["SpatialBiasCorrection"])) == (1, 1, 1)
    assert int(s["BoilingFilter"]) == 1 and np.isclose(s["BoilingFilterStrength"], 0.2) and int(s["SpatialSamples"]) == 1
    assert int(s["MaxHistoryLength"]) == 20 and int(s["DisocclusionBoostSamples"]) == 8 and float(s["SpatialSamplingRadius"]) == 32.0
    assert np.isclose(s["TemporalDepthThreshold"], 0.1) and np.isclose(s["TemporalNormalThreshold"], 0.5)


def test_offset_table():
    t = R.offset_table()
    assert t.shape == (8192, 2)
    assert np.array_equal(t, R.offset_table())                          # deterministic
    r2 = (t.astype(np.float64) / 127.0) ** 2
    assert (r2.sum(1) <= 1.0 + 1e-12).all()                             # inside the unit disc
    assert len(np.unique(t, axis=0)) > 4000                              # spread, not a short cycle
    assert abs(t[:, 0].astype(np.float64).mean()) < 2 and abs(t[:, 1].astype(np.float64).mean()) < 2
    assert R.spatial_offset(127, 32.0) == 32 and R.spatial_offset(-127, 32.0) == -32 and R.spatial_offset(3, 32.0) == 0


def test_rng_streams_differ_and_are_stable():
    a, b, c = (R.Rng(7, 9, 3, s) for s in (R.SALT_INITIAL, R.SALT_TEMPORAL, R.SALT_SPATIAL))
    da, db, dc = [a.next() for _ in range(4)], [b.next() for _ in range(4)], [c.next() for _ in range(4)]
    assert len({tuple(da), tuple(db), tuple(dc)}) == 3
    assert all(0 <= x < 1 for x in da + db + dc)
    again = R.Rng(7, 9, 3, R.SALT_TEMPORAL)
    assert [again.next() for _ in range(4)] == db


def test_reflect_into_view():
    assert R.reflect(-3, 5, 10, 8) == (3, 5)
    assert R.reflect(10, 8, 10, 8) == (9, 7)
    assert R.reflect(12, -1, 10, 8) == (7, 1)
    assert R.reflect(4, 4, 10, 8) == (4, 4)


# ---- mutations the restatement must tell apart ----------------------------------------------------------------------------------
def test_mutation_prev_rounding():
    """prev = round-half-even(p + mv): flipping to round-half-up (or truncation) moves ties and negative fractions"""
    rng = R.Rng(0, 0, 0, R.SALT_TEMPORAL)
    first = next(R.temporal_candidates(10, 10, (0.5, -1.5), 64, 64, rng))
    assert first == (10, 8)
    up = next(R.temporal_candidates(10, 10, (0.5, -1.5), 64, 64, rng, rounding=lambda v: int(np.floor(np.float32(v) + 0.5))))
    assert up != first


def test_mutation_previous_jitter():
    """a previous surface uses the current Jitter with the Previous* matrices"""
    cam = {"Jitter": np.array([0.3, -0.2]), "PreviousJitter": np.array([-0.1, 0.4]),
           "PreviousProjectionToView": np.diag([1.0, 0.7, 1.0, 1.0]).reshape(-1), "PreviousViewToWorld": np.eye(4).reshape(-1)}
    got = R.previous_surface_position(5, 6, 32, 24, cam, 2.0)
    wrong = R.reconstruct_position(5, 6, 32, 24, cam["PreviousJitter"], 2.0, cam["PreviousProjectionToView"], cam["PreviousViewToWorld"])
    assert not np.allclose(got, wrong)
    assert np.isclose(got[2], 2.0)


def _temporal_case():
    cur = R.Reservoir(light=1, W=0.5, M=8, p=2.0)
    hist = R.Reservoir(light=2, W=0.4, M=400, p=3.0, age=4)
    draws = [0.99, 0.2, 0.05]                                           # two search draws, then the combine draw
    return cur, hist, draws


def test_mutation_history_cap():
    cur, hist, draws = _temporal_case()
    capped = R.temporal_resample(cur, hist, 3.0, lambda l: 2.5, draws, 20, True, n_search_draws=2)
    uncapped = R.temporal_resample(cur, hist, 3.0, lambda l: 2.5, draws, 20, True, cap=False, n_search_draws=2)
    assert capped[2] == 8 + 160 and uncapped[2] == 408
    assert capped[0] == 2 and capped[4] == 5                            # the history sample, one frame older


def test_mutation_off_normaliser_under_basic():
    cur, hist, draws = _temporal_case()
    basic = R.temporal_resample(cur, hist, 3.0, lambda l: 1.0, draws, 20, True, n_search_draws=2)
    off = R.temporal_resample(cur, hist, 3.0, lambda l: 1.0, draws, 20, False, n_search_draws=2)
    assert not np.isclose(basic[1], off[1])
    # Basic: wsum * p_prev / (p * (M_cur p_cur + M_H p_prev)); Off: wsum / (p * sum M)
    wsum = 2.0 * 0.5 * 8 + 3.0 * 0.4 * 160
    assert np.isclose(basic[1], wsum * 1.0 / (3.0 * (8 * 3.0 + 160 * 1.0)))
    assert np.isclose(off[1], wsum / (3.0 * 168))
    # no history found: both reduce to the initial weight
    assert np.isclose(R.temporal_resample(cur, None, 0, None, [], 20, True)[1], 0.5)
    assert np.isclose(R.temporal_resample(cur, None, 0, None, [], 20, False)[1], 0.5)


def test_mutation_material_similarity():
    a = {"Normal": np.array([0, 1.0, 0]), "Depth": 2.0, "Roughness": 0.5, "F0": np.full(3, 0.04), "Albedo": np.full(3, 0.8)}
    b = dict(a, Albedo=np.full(3, 0.3))
    assert R.neighbour_ok(a, dict(a, Depth=2.1), 2.0, 0.5, 0.1)
    assert not R.neighbour_ok(a, b, 2.0, 0.5, 0.1)
    assert R.neighbour_ok(a, b, 2.0, 0.5, 0.1, check_material=False)   # the mutation would accept it
    assert not R.neighbour_ok(a, dict(a, Depth=2.5), 2.0, 0.5, 0.1)
    assert not R.neighbour_ok(a, dict(a, Normal=np.array([1.0, 0, 0])), 2.0, 0.5, 0.1)
    assert not R.neighbour_ok(a, dict(a, Roughness=0.2), 2.0, 0.5, 0.1)


def test_mutation_combine_before_search():
    cur, hist, draws = _temporal_case()
    right = R.temporal_resample(cur, hist, 3.0, lambda l: 2.5, draws, 20, True, n_search_draws=2)
    wrong = R.temporal_resample(cur, hist, 3.0, lambda l: 2.5, draws, 20, True, combine_first=True)
    assert right[0] != wrong[0]                                          # 0.05 keeps the history sample, 0.99 keeps the fresh one


def test_spatial_normalisation():
    assert np.isclose(R.spatial_normalise(6.0, 2.0, [(8, 2.0), (8, 0.0)], 2.0, True), 6.0 * 2.0 / (2.0 * 16.0))
    assert np.isclose(R.spatial_normalise(6.0, 2.0, [(8, 2.0), (8, 0.0)], 2.0, False), 6.0 / (2.0 * 16))
    assert R.spatial_normalise(6.0, 0.0, [(8, 2.0)], 2.0, True) == 0.0


def test_boiling_filter():
    W = np.full(64, 1.0, np.float32)
    valid = np.ones(64, bool)
    W[5] = 200.0
    cut = R.boiling_filter(W, valid, 0.2)                                # mean ~4.1, multiplier 41
    assert cut[5] and cut.sum() == 1
    assert R.boiling_filter(W, valid, 1.0).sum() == 1
    assert not R.boiling_filter(np.zeros(64, np.float32), valid, 0.2).any()
    v = np.random.default_rng(1).random(64).astype(np.float32)
    assert R.butterfly_sum(v) == R.butterfly_sum(v[np.arange(64) ^ 1])  # order-independent across lanes


# ---- what counts as "near a decision" ---------------------------------------------------------------------------------------------
def test_exact_roughness_tie_is_not_a_decision_at_risk():
    """The pin scene's floor (roughness 0.4, snorm16 code 13107) and bar (0.8, code 26214) meet the similarity test |ra - rb| <= 0.5 max
    exactly on its boundary. For codes q and 2 q the decoded values are in the ratio 2 in float32 as in float64, and both sides of the
    test are then the same bits: no arithmetic can take it the other way. roughness_margin says so; everywhere else it is the relative
    margin the pins always used."""
    q = np.arange(66, 16384)                                             # decoded >= the 2e-3 floor, 2 q still a code
    lo32, hi32 = q.astype(np.float32) / np.float32(32767.0), (2 * q).astype(np.float32) / np.float32(32767.0)
    assert np.array_equal(hi32, np.float32(2.0) * lo32)
    assert np.array_equal(np.abs(lo32 - hi32), np.float32(0.5) * np.maximum(lo32, hi32))
    lo, hi = 13107 / 32767.0, 26214 / 32767.0
    assert R._margin(abs(lo - hi), 0.5 * max(lo, hi)) == 0.0             # what the pins saw: a decision with no margin at all
    assert R.roughness_margin(lo, hi) == np.inf and R.roughness_margin(hi, lo) == np.inf
    a = {"Normal": np.array([0, 1.0, 0]), "Depth": 2.0, "Roughness": lo, "F0": np.full(3, 0.04), "Albedo": np.full(3, 0.8)}
    assert R.neighbour_ok(a, dict(a, Roughness=hi), 2.0, 0.5, 0.1)       # the tie is on the accepting side
    for ra, rb in ((lo, 26215 / 32767.0), (lo, 26213 / 32767.0), (0.4, 0.8000001), (0.5, 0.5), (0.2, 0.9), (2e-3, 4e-3 + 1e-12)):
        assert R.roughness_margin(ra, rb) == R._margin(abs(ra - rb), 0.5 * max(ra, rb)), (ra, rb)
    assert R.roughness_margin(lo, 26215 / 32767.0) < 1e-4                # one code off the tie is near, and is still left out


def test_tie_rule_changes_what_is_left_out_and_nothing_else(pkg, oracle, monkeypatch):
    """The spatial pass over the oracle's G-buffer of the pin scene at 37 x 23 and a synthetic fresh frame: with the tie taken for a
    decision at risk (the margin as it was) every floor pixel that drew a bar pixel among its eight neighbours is left out -- over a
    quarter of the valid pixels, the per-pixel pins' cap -- and with the tie rule a few per cent are; the reservoirs are the same."""
    import bsdfref
    import visscene
    S, L = pkg.scenes, pkg.layouts
    W, H = 37, 23
    scene = visscene.pin_scene(S, W / H)
    gb, _, _ = oracle.render(scene, S.graphics_settings(W, H, spp=1, bounces=0), layouts=L)
    cur = R.Surfaces(gb, scene.camera)
    lights, bsdf, table = visscene.host_lights(scene, L), bsdfref.Reference(), R.offset_table()
    fresh = visscene.synthetic_frame(cur, lights, bsdf, 1)

    def left_out():
        out, margin = R.spatial_pass(cur, fresh, np.full((H, W), np.inf), lights, table, 40, bsdf, 1, 8, 20, 32.0, True)
        return out, float((cur.valid & (margin < 1e-5)).sum()) / cur.valid.sum()
    new, share = left_out()
    monkeypatch.setattr(R, "roughness_margin", lambda ra, rb: R._margin(abs(ra - rb), 0.5 * max(ra, rb)))
    old, old_share = left_out()
    print(f"left out at {W} x {H}: {old_share:.1%} with the tie at risk, {share:.1%} with the tie rule")
    assert old_share > 0.25 and share < 0.05
    for k in R.FIELDS:
        assert np.array_equal(new[k], old[k]), k
