"""CPU tests of the post-processing spec ("Post-processing") through its numpy restatement (tests/postref.py) and of
the settings helper of layouts.py: sizes and the stage table, invariants of the filters, known operator values, the UNORM encodes, and
the ranges pt_post_set_constants accepts."""
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as ge
import postref as R

ge.load_package()
from dxpbrt_amd import layouts as L  # noqa: E402

# (overrides of post_processing_settings, accepted?) -- the GPU suite runs the same table through pt_post_set_constants
SETTINGS_CASES = [
    ({}, True), ({"strength": 0.0}, True), ({"strength": 1.0}, True), ({"strength": -0.01}, False), ({"strength": 1.01}, False),
    ({"strength": float("nan")}, False), ({"exposure": -10.0}, True), ({"exposure": 10.0}, True), ({"exposure": 10.5}, False),
    ({"exposure": float("inf")}, False), ({"paper_white_nits": 50.0}, True), ({"paper_white_nits": 10000.0}, True),
    ({"paper_white_nits": 49.9}, False), ({"paper_white_nits": 10001.0}, False), ({"operator": 0}, False), ({"operator": 4}, False),
    ({"operator": "saturate"}, True), ({"operator": "reinhard"}, True), ({"rotation": 3}, False), ({"rotation": "hdtv_to_dci_p3_d65"}, True),
    ({"hdr": True}, True), ({"bloom": False}, True), ({"width": 0}, False), ({"height": 16385}, False), ({"width": 16384, "height": 1}, True),
]
RAW_CASES = [("IsBloomEnabled", 2), ("IsHDREnabled", 2)]


def settings_args(over):
    kw = dict(over)
    w, h = kw.pop("width", 64), kw.pop("height", 33)
    return w, h, kw


def test_mip_sizes_and_stage_table():
    t = R.stage_table(1920, 1080)
    assert [d for _, _, _, d in t] == [(960, 540), (480, 270), (240, 135), (120, 67), (60, 33), (120, 67), (240, 135), (480, 270), (960, 540)]
    assert [k for k, _, _, _ in t] == ["down"] * 5 + ["up"] * 4
    assert [karis for _, karis, _, _ in t] == [True, True] + [False] * 7            # stage 1 reads mip 0 too: the Karis branch
    assert t[0][2] == (1920, 1080) and all(t[s][2] == t[s - 1][3] for s in range(1, 9))   # each stage reads the image of the one before
    assert [d for _, _, _, d in R.stage_table(1917, 1083)][:5] == [(958, 541), (479, 270), (239, 135), (119, 67), (59, 33)]
    assert [d for _, _, _, d in R.stage_table(64, 33)][:5] == [(32, 16), (16, 8), (8, 4), (4, 2), (2, 1)]
    assert [d for _, _, _, d in R.stage_table(32, 2)][:5] == [(16, 1), (8, 1), (4, 1), (2, 1), (1, 1)]
    assert [d for _, _, _, d in R.stage_table(2, 32)][:5] == [(1, 16), (1, 8), (1, 4), (1, 2), (1, 1)]
    for w, h, ok in ((32, 2, True), (2, 32, True), (31, 31, False), (33, 1, False), (1, 40, False), (1920, 1080, True)):
        assert R.bloom_size_ok(w, h) == ok


def test_constant_image_passes_stages_2_to_8_unchanged():
    """every tap of a constant fp16 image is the constant (the bilinear lerp of equal texels is exact), and the weights of both filters
    sum to exactly 1 in powers of two"""
    for c in (0.0, 1.0, 0.3333, 6.1e-5, 1234.5, 65504.0):
        val = R.h2f(R.f16(np.float32(c)))
        for s in range(2, 9):
            table = R.stage_table(97, 61)
            _, _, din, dout = table[s]
            src = np.full((din[1], din[0], 3), val, np.float32)
            out = R.stage(s, src, dout)
            assert np.array_equal(R.f16(out), R.f16(np.full(out.shape, val, np.float32))), (c, s)


def test_strength_zero_is_the_radiance_sample():
    rad = R.make_frame(64, 33, seed=3, specials=False)
    a = R.merge(rad, R.make_frame(32, 16, seed=4, specials=False), 0.0)
    b = R.merge(rad, np.zeros((16, 32, 4), np.uint16), 0.0)
    assert np.array_equal(a, b)                                                     # a finite bloom term is multiplied by 0
    assert np.array_equal(R.f16(a), rad[..., :3])                                   # and the Radiance tap lands on its texel here
    full = R.merge(rad, R.make_frame(32, 16, seed=4, specials=False), 1.0)
    assert not np.array_equal(R.f16(full), rad[..., :3])


def test_known_operator_values():
    def tm(values, **kw):
        s = R_settings(**kw)
        return R.tone_map(np.array(values, np.float32).reshape(-1, 1).repeat(3, 1), s)[:, 0]
    assert tm([0.0], operator="aces_filmic")[0] == 0.0
    assert tm([1.0], operator="reinhard")[0] == pytest.approx(0.5 ** (1 / 2.2), rel=1e-6)
    assert tm([0.25, 2.0], operator="saturate").tolist() == pytest.approx([0.25 ** (1 / 2.2), 1.0], rel=1e-6)
    assert tm([1e9], operator="aces_filmic")[0] == 1.0                              # saturated: 2.51 / 2.43 > 1
    p = R.PQ
    pq1 = ((p["c1"] + p["c2"]) / (1 + p["c3"])) ** p["m2"]
    assert pq1 == 1.0                                                                # ST.2084 maps 10000 nits to 1
    white = np.float32(10000.0 / 200.0)
    assert R.tone_map(np.full((1, 3), white, np.float32), R_settings(hdr=True))[0] == pytest.approx(1.0, abs=2e-6)
    assert np.allclose(np.array(R.ROTATIONS).sum(-1), 1.0, atol=1e-4)              # each rotation row sums to ~1


def R_settings(**kw):
    return L.post_processing_settings(64, 33, **kw)


def test_unorm_edge_codes():
    x = np.array([0.0, -1.0, np.nan, 1.0, np.inf, 0.5, 1 / 1023, 0.5 / 1023, 0.49 / 1023, 1 / 255, 0.5 / 255], np.float32)
    assert R.unorm(x, 10).tolist() == [0, 0, 0, 1023, 1023, 512, 1, 1, 0, 4, 2]
    assert R.unorm(x, 8).tolist() == [0, 0, 0, 255, 255, 128, 0, 0, 0, 1, 1]
    assert R.unorm(np.array([1 / 3, 2 / 3, 1.0], np.float32), 2).tolist() == [1, 2, 3]
    color = np.zeros((1, 1, 4), np.uint16)
    color[0, 0] = R.f16(np.array([1.0, 0.0, 0.5, 1.0], np.float32))
    back, d8 = R.encode(color)
    assert int(back[0, 0]) == 1023 | 0 << 10 | 512 << 20 | 3 << 30                 # bits 0-9 R, 10-19 G, 20-29 B, 30-31 A
    assert d8[0, 0].tolist() == [255, 0, 128, 255]


def test_fma_emulation_is_single_rounding():
    a, b, c = np.float32(1 + 2 ** -12), np.float32(1 + 2 ** -12), np.float32(-1.0)
    assert R.fma(a, b, c) == np.float32(2 ** -11 + 2 ** -24)                        # a * b + c exactly representable: no rounding
    assert (a * b + c) != R.fma(a, b, c)                                            # the float32 product alone loses the 2^-24 term
    rng = np.random.default_rng(1)
    x, y, z = (rng.standard_normal(10000).astype(np.float32) for _ in range(3))
    exact = [float(np.float32(float(Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r))))) for p, q, r in zip(x[:300], y[:300], z[:300])]
    assert np.array_equal(R.fma(x[:300], y[:300], z[:300]), np.array(exact, np.float32))


def test_settings_helper_refuses_what_the_library_refuses():
    s = L.post_processing_settings(1920, 1080)
    assert L.POST_PROCESS_SETTINGS.itemsize == 48
    assert (int(s["IsBloomEnabled"]), float(s["BloomStrength"]), int(s["IsHDREnabled"]), int(s["ToneMappingOperator"]),
            float(s["Exposure"]), float(s["PaperWhiteNits"]), int(s["ColorPrimaryRotation"])) == \
        (1, pytest.approx(0.05), 0, L.TONE_MAP_ACES_FILMIC, 0.0, 200.0, L.COLOR_ROTATION_HDTV_TO_UHDTV)
    for over, ok in SETTINGS_CASES:
        w, h, kw = settings_args(over)
        if ok:
            L.post_processing_settings(w, h, **kw)
        else:
            with pytest.raises(ValueError):
                L.post_processing_settings(w, h, **kw)
    for field, value in RAW_CASES:
        s = L.post_processing_settings(64, 33)
        s[field] = value
        with pytest.raises(ValueError):
            L.check_post_processing_settings(s)


def test_every_mutation_changes_the_restatement():
    """each mutation of tests/postref.py is live on the test frame under the settings its GPU check uses"""
    rad = R.make_frame(67, 37, seed=5)
    for mut in R.MUTATIONS:
        kw = MUTATION_SETTINGS.get(mut, {})
        s = R_settings_sized(67, 37, **kw)
        base = R.post_process(rad, s)
        got = R.post_process(rad, s, mut=(mut,))
        differs = any(not np.array_equal(x, y) for x, y in zip(base[0], got[0])) or any(not np.array_equal(x, y) for x, y in zip(base[1:], got[1:]))
        assert differs, mut


MUTATION_SETTINGS = {"linear_exposure": {"exposure": 3.5}, "hdr_no_rotation": {"hdr": True}, "swapped_merge_weights": {"strength": 0.05},
                     "unsaturated_aces": {"exposure": 3.5}}


def R_settings_sized(w, h, **kw):
    return L.post_processing_settings(w, h, **kw)
