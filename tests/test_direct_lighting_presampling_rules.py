"""Local-light sampling rules on the CPU ("Local-light sampling"): the new structs against include/ptamd.h, the
reference's defaults, CalculateWeightForVolume in float32 against a float64 form of Light.hlsli, cell indexing, the RNG streams, the
entry-index rules, and mutations the restatement (tests/presamplingref.py) must catch."""
import os
import re

import numpy as np

import __graft_entry__ as ge
import presamplingref as P
import restirref as R

ge.load_package()
import dxpbrt_amd.layouts as L  # noqa: E402


def _header():
    return open(os.path.join(ge.ROOT, "include", "ptamd.h")).read()


def test_structs_match_the_header():
    h = _header()
    body = re.search(r"typedef struct PtDILightSamplingSettings \{(.*?)\} PtDILightSamplingSettings;", h, re.S).group(1)
    names = re.findall(r"(?:uint32_t|float)\s+(\w+);", body)
    assert names == ["Mode", "ReGIRCellSize", "ReGIRBuildSamples", "_pad"]
    assert L.DI_LIGHT_SAMPLING_SETTINGS.itemsize == 16 and list(L.DI_LIGHT_SAMPLING_SETTINGS.names) == names[:3]
    assert [L.DI_LIGHT_SAMPLING_SETTINGS.fields[n][1] for n in names[:3]] == [0, 4, 8]
    body = re.search(r"typedef struct PtDIPresampledLight \{(.*?)\} PtDIPresampledLight;", h, re.S).group(1)
    assert re.findall(r"(?:uint32_t|float)\s+(\w+);", body) == ["LightIndex", "InvSourcePdf"]
    assert L.DI_PRESAMPLED_LIGHT.itemsize == 8 and L.DI_PRESAMPLED_LIGHT.fields["InvSourcePdf"][1] == 4
    for name, v in (("POWER_CDF", 0), ("UNIFORM", 1), ("POWER_RIS", 2), ("REGIR_RIS", 3)):
        assert re.search(rf"PT_DI_LOCAL_LIGHT_{name}\s*=\s*{v}\b", h)
    assert (L.DI_LOCAL_LIGHT_POWER_CDF, L.DI_LOCAL_LIGHT_UNIFORM, L.DI_LOCAL_LIGHT_POWER_RIS, L.DI_LOCAL_LIGHT_REGIR_RIS) == (0, 1, 2, 3)
    assert "pt_di_set_light_sampling" in h and "pt_di_download_presampled" in h


def test_defaults_are_the_references():
    """MyAppData.h: LocalLight.Mode = ReGIR_RIS, ReGIR.Cell.Size = 1, ReGIR.BuildSamples = 8"""
    s = L.di_light_sampling_settings()
    assert int(s["Mode"]) == L.DI_LOCAL_LIGHT_REGIR_RIS and float(s["ReGIRCellSize"]) == 1.0 and int(s["ReGIRBuildSamples"]) == 8
    assert int(L.di_light_sampling_settings("power_ris")["Mode"]) == 2 and int(L.di_light_sampling_settings("cdf")["Mode"]) == 0


def test_volume_weight_float32_matches_float64():
    rng = np.random.default_rng(3)
    n = 400
    lights = np.zeros(n, L.TRIANGLE_LIGHT)
    base = rng.normal(size=(n, 3)) * 3
    e0, e1 = rng.normal(size=(n, 3)) * 0.3, rng.normal(size=(n, 3)) * 0.3
    rad = rng.random((n, 3)) * 5
    nrm = np.cross(e0, e1)
    ln = np.linalg.norm(nrm, axis=1)
    lights["Base"], lights["Edge0"], lights["Edge1"], lights["Radiance"] = base, e0, e1, rad
    lights["Normal"], lights["Area"] = nrm / ln[:, None], ln / 2
    centre = rng.normal(size=(n, 3)) * 3
    radius = rng.random(n) * 1.5 + 0.05
    got = P.volume_weight32(lights, np.arange(n), centre, radius[:, None][:, 0])
    ref = np.array([P.volume_weight64(base[i], e0[i], e1[i], rad[i], centre[i], radius[i]) for i in range(n)])
    nz = ref > 0
    assert nz.sum() > n // 3 and (got[~nz] == 0).all()
    assert np.max(np.abs(got[nz] - ref[nz]) / ref[nz]) < 1e-5
    # near the light: the solid angle saturates at 2 pi
    assert np.isclose(P.volume_weight64((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1), (0.3, -0.01, 0.3), 1e-3), 2 * np.pi, rtol=1e-12)


def test_cell_indexing_and_fallback():
    centre, cs = np.float32([1.0, 2.0, -3.0]), 0.5
    mid = np.float32([0.5, 0.5, 0.5])                                      # jitter draws of 0.5: no jitter
    assert P.regir_cell(centre, mid, centre, cs) == (8 * 16 + 8) * 16 + 8
    assert P.regir_cell(centre + np.float32([-0.01, 0, 0]), mid, centre, cs) == (8 * 16 + 8) * 16 + 7
    assert P.regir_cell(centre + np.float32([3.99, -4.0, 0]), mid, centre, cs) == (8 * 16 + 0) * 16 + 15
    assert P.regir_cell(centre + np.float32([4.0, 0, 0]), mid, centre, cs) == -1     # outside: Power_RIS
    assert P.regir_cell(centre + np.float32([0, -4.01, 0]), mid, centre, cs) == -1
    # jitter draws in [0, 1) move the point by up to one cell size either way
    assert P.regir_cell(centre, np.float32([0.0, 0.5, 0.5]), centre, cs) == (8 * 16 + 8) * 16 + 7
    assert P.regir_cell(centre + np.float32([0.25, 0, 0]), np.float32([0.99, 0.5, 0.5]), centre, cs) == (8 * 16 + 8) * 16 + 9
    c = P.cell_centre([(8 * 16 + 8) * 16 + 8, 0], centre, cs)
    assert np.allclose(c[0], centre + 0.25) and np.allclose(c[1], centre - 7.5 * cs)
    assert np.isclose(P.cell_radius(cs), np.sqrt(3) / 2 * cs)


def test_rng_streams_distinct_and_stable():
    draws = {}
    for salt in (R.SALT_INITIAL, R.SALT_TEMPORAL, R.SALT_SPATIAL, P.SALT_PRESAMPLE, P.SALT_REGIR, P.SALT_REGIR_COHERENT, P.SALT_SCREEN_TILE):
        st = P.rng_states(np.uint64(5), np.uint64(7), 3, salt)
        _, u = P.rng_next(st)
        ref = R.Rng(5, 7, 3, salt).next()
        assert np.float32(u) == ref                                         # the vectorised generator is restirref's
        draws[salt] = float(u)
    assert len(set(draws.values())) == len(draws)
    # stable: pinned values of the new streams at entry / pixel (5, 7), frame 3
    g = np.arange(8, dtype=np.uint64)
    _, u = P.rng_next(P.rng_states(g & np.uint64(0xFFF), g >> np.uint64(12), 0, P.SALT_PRESAMPLE))
    _, u2 = P.rng_next(P.rng_states(g & np.uint64(0xFFF), g >> np.uint64(12), 0, P.SALT_PRESAMPLE))
    assert np.array_equal(u, u2) and len(set(u.tolist())) == 8
    # the screen-tile stream depends only on (x / 16, y / 16): a 16-row band sees the tiles of the whole frame
    t = P.screen_tile(np.arange(64)[:, None], np.arange(48)[None, :], 9)
    assert (t[:16, :16] == t[0, 0]).all() and (t[16:32, 16:32] == t[16, 16]).all() and len(np.unique(t)) > 1
    # the coherent tile choice of the ReGIR build is shared by 256 consecutive slots
    g = np.arange(1024, dtype=np.uint64)
    _, ct = P.rng_next(P.rng_states(g >> np.uint64(8), np.zeros_like(g), 2, P.SALT_REGIR_COHERENT))
    tiles = P.index_of(ct, P.TILE_COUNT)
    assert all(len(np.unique(tiles[i:i + 256])) == 1 for i in range(0, 1024, 256)) and len(np.unique(tiles)) > 1


def test_entry_index_rules():
    top = np.float32(16777215.0 / 16777216.0)
    assert P.index_of(top, 1024) == 1023 and P.index_of(np.float32(0), 1024) == 0 and P.index_of(top, 131072) == 131071
    assert P.index_of(np.float32(0.5), 512) == 256
    # select_light: a zero-power light is never chosen; u * total >= total takes the first light that reaches the total
    cdf, total = P.power_cdf([0.0, 1.0, 0.0, 2.0, 0.0])
    assert cdf[-1] == total == 3.0
    assert P.select_light(cdf, np.float32([0.0, 0.999, 1.0, 2.9999, 3.0, 3.5]), total).tolist() == [1, 1, 3, 3, 3, 3]


def _field_lights(n=3000, seed=1):
    rng = np.random.default_rng(seed)
    lights = np.zeros(n, L.TRIANGLE_LIGHT)
    side = 0.1 * 10 ** (rng.random(n) - 1)
    base = np.stack([rng.random(n) * 8 - 4, 3.5 + rng.random(n) * 0.25, rng.random(n) * 8 - 4], 1)
    lights["Base"], lights["Edge0"], lights["Edge1"] = base, np.stack([side, 0 * side, 0 * side], 1), np.stack([side, 0 * side, side], 1)
    lights["Normal"] = (0, -1, 0)
    lights["Area"] = side * side / 2
    lights["Radiance"] = (1.0, 0.9, 0.8)
    lights["Power"] = (lights["Area"] * np.pi * (np.float32([1.0, 0.9, 0.8]) @ P.LUMA32)).astype(np.float32)
    return lights


def test_mutations_are_caught():
    lights = _field_lights()
    power = lights["Power"].astype(np.float32)
    li, inv = P.presample_tiles(power, 4)
    assert (li >= 0).all() and (power[li] > 0).all()
    np.testing.assert_allclose(np.bincount(li, minlength=len(power)) / len(li), power / power.sum(), atol=2e-3)
    # CDF presampling with u * total but without the >= total rule: some u draw rounds u * total up to the total and returns n
    cdf, total = P.power_cdf(power)
    u_top = np.float32(16777215.0 / 16777216.0)
    x = np.float32(u_top * total)
    assert x >= total or P.select_light(cdf, x, total) == P.select_light(cdf, x, total, ge_rule=False)
    tot = np.float32(7.0)
    cdf2 = np.float32([1.0, 3.0, 7.0, 7.0])
    assert P.select_light(cdf2, np.float32(7.0), tot) == 2 and P.select_light(cdf2, np.float32(7.0), tot, ge_rule=False) == 4
    # the ReGIR build: a cell above the emitters culls them one-sided; a two-sided cull keeps more of them empty
    centre = np.float32([0, 2, -3.5])
    cells = np.array([(12 * 16 + 8) * 16 + 8, (9 * 16 + 8) * 16 + 8, (8 * 16 + 10) * 16 + 8, (8 * 16 + 13) * 16 + 8])
    ref_li, ref_w = P.regir_build(lights, li, inv, cells, centre, 1.0, 8, 4)
    two_li, _ = P.regir_build(lights, li, inv, cells, centre, 1.0, 8, 4, two_sided=True)
    assert (ref_li[:3] >= 0).all() and not np.array_equal(ref_li, two_li)
    assert (ref_li[3] < 0).all()                                         # cell y = 13 (centre 7.5 m): above every emitter, culled
    # a missing BuildSamples in the stored weight
    _, w1 = P.regir_build(lights, li, inv, cells[:1], centre, 1.0, 8, 4, store_build_samples=False)
    assert np.allclose(w1, ref_w[:1] * 8, rtol=1e-6) and not np.allclose(w1, ref_w[:1])
    # jitter not doubled: some points land in another cell
    rng = np.random.default_rng(5)
    Pts = rng.random((2000, 3)).astype(np.float32) * 6 - 3
    j = rng.random((2000, 3)).astype(np.float32)
    assert (P.regir_cell(Pts, j, centre, 1.0) != P.regir_cell(Pts, j, centre, 1.0, jitter_scale=1.0)).mean() > 0.2
    # a screen tile of 8 px: pixels of one 16 px tile see different light tiles
    t16 = P.screen_tile(np.arange(16)[:, None], np.arange(16)[None, :], 3)
    t8 = P.screen_tile(np.arange(16)[:, None], np.arange(16)[None, :], 3, tile_px=8)
    assert len(np.unique(t16)) == 1 and len(np.unique(t8)) > 1

