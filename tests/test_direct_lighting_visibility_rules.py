"""CPU checks of visibility in the DI reservoirs: the settings struct and the Visibility word against the header, the float64 restatement
(tests/restirref.py's passes, tests/restirvisref.py) with every flag off, Raytraced against Basic, an enumerated two-pixel case that tells the two
apart, the final-visibility reuse boundaries, and the share of pixels the per-pixel GPU pins may have to leave out."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import bsdfref
import restirref as R
import restirvisref as V
import visscene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 1e-5


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
        for item in rest.split(","):
            fields[item.strip()] = off
            off += 4
    return fields, off


def test_visibility_struct_matches_header(pkg, ptamd):
    L = pkg.layouts
    fields, size = _header_struct("PtDIVisibilitySettings")
    assert size == 32 == L.PT_DI_VISIBILITY_SETTINGS.itemsize
    assert [n for n in fields if not n.startswith("_")] == list(L.PT_DI_VISIBILITY_SETTINGS.names)
    for n, off in fields.items():
        if not n.startswith("_"):
            assert L.PT_DI_VISIBILITY_SETTINGS.fields[n][1] == off, n
    fields, size = _header_struct("PtDIReservoir")
    assert size == 32 and fields["Visibility"] == 28 and L.DI_RESERVOIR.fields["Visibility"][1] == 28 and "_pad" not in fields
    assert "pt_di_set_visibility" in ptamd.EXPORTS and hasattr(ptamd.load_library(), "pt_di_set_visibility")
    s = L.di_visibility_settings()                                        # the SDK's defaults (unpinned)
    assert (int(s["InitialVisibility"]), int(s["FinalVisibilityReuse"]), int(s["FinalVisibilityMaxAge"]), float(s["FinalVisibilityMaxDistance"]),
            int(s["DiscardInvisibleSamples"]), int(s["TemporalRaytraced"]), int(s["SpatialRaytraced"])) == (1, 1, 4, 16.0, 0, 0, 0)


def test_pack_round_trip_and_clamping(pkg):
    L = pkg.layouts
    rng = np.random.default_rng(5)
    for _ in range(200):
        c = rng.integers(0, 32, 3)
        dx, dy, age = int(rng.integers(-31, 32)), int(rng.integers(-31, 32)), int(rng.integers(0, 16))
        w = V.pack(c / 31.0 + 1e-4, dx, dy, age)                        # + a little: c / 31 * 31 may round below c in float32
        rgb, gx, gy, ga = V.unpack(w)
        assert (np.rint(rgb * 31) == c).all() and (gx, gy, ga) == (dx, dy, age) and w < 2 ** 31
        lr, lx, ly, la = L.di_unpack_visibility(np.uint32(w))           # the package's helpers agree
        assert np.array_equal(lr, rgb) and (int(lx), int(ly), int(la)) == (dx, dy, age)
        assert L.di_pack_visibility(c / 31.0 + 1e-4, dx, dy, age) == w
    assert V.pack((0, 0, 0)) == 0                                        # a fresh sample's word
    assert V.unpack(V.pack((1.0, 0.5, 0.0)))[0].tolist() == [1.0, 15 / 31, 0.0]          # uint(v * 31): truncation
    assert V.unpack(V.pack((7.0, -3.0, np.float32(0.999))))[0].tolist() == [1.0, 0.0, 30 / 31]
    assert V.unpack(V.pack((1, 1, 1), 40, -77, 99))[1:] == (31, -31, 15)
    # carrying: the colour stays, d accumulates and clamps, the age saturates
    w = V.pack((1, 0.5, 0.25), 3, -4, 2)
    assert V.unpack(V.carry(w, 2, 1, 1))[1:] == (5, -3, 3) and (V.carry(w, 2, 1, 1) & 0x7FFF) == (w & 0x7FFF)
    assert V.unpack(V.carry(w, 100, -100, 0))[1:] == (31, -31, 2)
    assert V.unpack(V.carry(V.pack((1, 1, 1), -31, 31, 15), -1, 1, 1))[1:] == (-31, 31, 15)
    assert V.unpack(V.carry(V.pack((1, 1, 1), 31, 0, 14), -2, 0, 1))[1:] == (29, 0, 15)     # a clamped d walks back: the clamp loses the excess


def test_reuse_eligibility_boundaries():
    one = (1, 1, 1)
    assert not V.reusable(V.pack(one, 0, 0, 0), 4, 16.0)                 # age 0: traced this frame, nothing to reuse yet
    assert V.reusable(V.pack(one, 0, 0, 1), 4, 16.0)
    assert V.reusable(V.pack(one, 0, 0, 4), 4, 16.0)                     # age = MaxAge
    assert not V.reusable(V.pack(one, 0, 0, 5), 4, 16.0)                 # MaxAge + 1
    assert not V.reusable(V.pack(one, 0, 0, 15), 14, 31.0)               # the saturated age is beyond the largest MaxAge
    assert V.reusable(V.pack(one, 9, 12, 1), 4, 15.5) and not V.reusable(V.pack(one, 9, 12, 1), 4, 15.0)    # |d| = 15: strictly inside only
    assert V.reusable(V.pack(one, -3, 4, 1), 4, 5.0001) and not V.reusable(V.pack(one, -3, 4, 1), 4, 5.0)
    assert not V.reusable(V.pack(one, 31, 0, 1), 14, 31.0) and not V.reusable(V.pack(one, 0, -45, 1), 14, 31.0)   # a saturated d never qualifies
    assert V.reusable(V.pack(one, 30, 0, 1), 14, 31.0)


# ---- the ray ---------------------------------------------------------------------------------------------------------------------
def test_visibility_ray(pkg):
    S = pkg.scenes
    scene = visscene.pin_scene(S, 1.5)
    occ = V.Occluders(scene)
    assert len(occ.tris) == 2 + 3 + 2 + 2
    o = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    p = np.array([[0.0, 1.45, 0.0],        # straight up through the bar (y = 0.7, z in [-0.1, 0.15])
                  [0.0, 1.45, 1.0],        # beside the bar
                  [0.0, 0.699, 0.0],       # ends below the bar
                  [0.0, 0.7015, 0.0],      # the bar inside the 2e-3 back-off before the target: not a candidate
                  [0.0, 1.45, 0.15 * 1.45 / 0.7]])   # through the bar's edge: undecided
    blocked, vis, margin = occ.trace(o, p)
    assert blocked.tolist()[:4] == [True, False, False, False]
    assert vis[0].tolist() == [0, 0, 0] and vis[1].tolist() == [1, 1, 1]
    assert margin[0] > 1e-2 and margin[1] > 1e-2 and margin[4] < 1e-6
    assert 0 < margin[3] < 1e-3                                           # t = 0.7 against tmax = 0.6995: near, and said so
    # a transmissive sheet colours the visibility and does not block; a masked one decides by alpha
    glass = S.quad_mesh((-1, 0.5, -1), (1, 0.5, -1), (1, 0.5, 1), (-1, 0.5, 1), (0, -1, 0), S.material((0.5, 1.0, 0.25), transmission=1.0))
    sc = S.Scene([S.MeshNode([glass])], [S.RenderObject(0, S.trs())], scene.camera, S.make_scene_data((0, 0, 0, 1))).finalize()
    o, p = np.array([[0.3, 0.0, 0.0]]), np.array([[0.3, 1.45, 0.0]])      # off the quad's diagonal: one triangle
    b, v, _ = V.Occluders(sc).trace(o[:1], p[:1])
    assert not b[0] and v[0].tolist() == [0.5, 1.0, 0.25]
    glass.material["AlphaMode"], glass.material["AlphaCutoff"] = 1, 0.5
    b, v, _ = V.Occluders(sc).trace(o[:1], p[:1])
    assert b[0] and v[0].tolist() == [0, 0, 0]
    glass.material["AlphaCutoff"] = 1.5
    b, v, _ = V.Occluders(sc).trace(o[:1], p[:1])
    assert not b[0] and v[0].tolist() == [1, 1, 1]


# ---- the passes on a synthetic frame ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame(pkg, oracle):
    """the oracle's G-buffer of the pin scene at 48 x 32 (a static camera: the previous frame is this frame), the scene's light records
    made on the host, a synthetic initial frame and a synthetic history"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = visscene.pin_scene(S, W / H)
    gb, _, _ = oracle.render(scene, S.graphics_settings(W, H, spp=1, bounces=0), layouts=L)
    for n in L.DI_PREVIOUS_TEXTURES:
        gb[n] = gb[n[len("Previous"):]]
    cam = scene.camera
    bsdf = bsdfref.Reference()
    cur, prev = R.Surfaces(gb, cam), R.Surfaces(gb, cam, previous=True)
    lights = visscene.host_lights(scene, L)
    assert len(lights) == 5
    fresh = visscene.synthetic_frame(cur, lights, bsdf, 1)
    history = visscene.synthetic_frame(cur, lights, bsdf, 2, with_visibility=True)
    history["M"] = np.where(cur.valid, 60, 0)
    mv = np.zeros((H, W, 4), np.float32)
    return dict(scene=scene, cur=cur, prev=prev, lights=lights, fresh=fresh, history=history, mv=mv, bsdf=bsdf, occ=V.Occluders(scene),
                table=R.offset_table(), W=W, H=H)


def test_flags_off_is_restirref(frame, pkg):
    """the passes without the visibility arguments are the passes given occluders and a margin with Raytraced off, field for field and
    margin for margin. The history's words are zero, so no output carries a colour: after the temporal pass a word is 0 on a fresh
    sample and the carried offset and age of a zero word on a sample from the history (the device without visibility stores 0 there;
    the word is not read)."""
    f = frame
    inf = np.full((f["H"], f["W"]), np.inf)
    assert not f["history"]["Visibility"].any() and not f["fresh"]["Visibility"].any()
    for basic, boiling in ((True, True), (False, False)):
        want, wm = R.temporal_pass(f["cur"], f["prev"], f["mv"], f["fresh"], f["history"], f["lights"], 7, f["bsdf"], 20, basic, boiling, 0.2)
        got, gm = R.temporal_pass(f["cur"], f["prev"], f["mv"], f["fresh"], f["history"], f["lights"], 7, f["bsdf"], 20, basic, boiling, 0.2,
                                  in_margin=inf, occ=f["occ"], raytraced=False, stats={})
        assert set(want) == set(got) == set(R.FIELDS)
        for k in want:
            assert np.array_equal(want[k], got[k]), ("temporal", basic, k)
        assert np.array_equal(wm, gm)
        assert (got["M"] > 8).any() and ((got["Age"] > 0).any())
        want2, wm2 = R.spatial_pass(f["cur"], want, wm, f["lights"], f["table"], 7, f["bsdf"], 2, 8, 20, 32.0, basic)
        got2, gm2 = R.spatial_pass(f["cur"], got, gm, f["lights"], f["table"], 7, f["bsdf"], 2, 8, 20, 32.0, basic, occ=f["occ"], raytraced=False,
                                   stats={})
        for k in want2:
            assert np.array_equal(want2[k], got2[k]), ("spatial", basic, k)
        assert np.array_equal(wm2, gm2)
        assert not (want["Visibility"] & 0x7FFF).any() and not (want2["Visibility"] & 0x7FFF).any(), basic
        assert not want["Visibility"][want["Age"] == 0].any(), basic


def test_raytraced_equals_basic_when_nothing_is_blocked(frame, pkg):
    S = pkg.scenes
    f = frame
    inf = np.full((f["H"], f["W"]), np.inf)
    scene = visscene.pin_scene(S, f["W"] / f["H"])
    scene.instance_masks[2] = 0                                           # no bar: nothing between the floor and the lights
    occ = V.Occluders(scene)
    st = {}
    b, _ = R.temporal_pass(f["cur"], f["prev"], f["mv"], f["fresh"], f["history"], f["lights"], 7, f["bsdf"], 20, True, False, 0.2)
    r, _ = R.temporal_pass(f["cur"], f["prev"], f["mv"], f["fresh"], f["history"], f["lights"], 7, f["bsdf"], 20, True, False, 0.2,
                           occ=occ, raytraced=True, stats=st)
    floor = f["cur"].valid & (np.abs(f["cur"].P[..., 1]) < 1e-3)
    assert floor.sum() > 0.3 * f["W"] * f["H"]
    for k in b:
        assert np.array_equal(b[k][floor], r[k][floor]), k
    b2, _ = R.spatial_pass(f["cur"], b, inf, f["lights"], f["table"], 7, f["bsdf"], 2, 8, 20, 32.0, True)
    r2, _ = R.spatial_pass(f["cur"], b, inf, f["lights"], f["table"], 7, f["bsdf"], 2, 8, 20, 32.0, True, occ=occ, raytraced=True, stats=st)
    on_floor = floor.copy()                                               # pixels all of whose neighbours lie on the floor too
    for k in b2:
        same = b2[k] == r2[k]
        assert same[on_floor].mean() > 0.98, k                            # (a neighbour on an emitter or the bar's top may be blocked by its own mesh)
    # and with the bar back, Raytraced zeroes terms
    st = {}
    R.temporal_pass(f["cur"], f["prev"], f["mv"], f["fresh"], f["history"], f["lights"], 7, f["bsdf"], 20, True, False, 0.2,
                    occ=f["occ"], raytraced=True, stats=st)
    assert st.get("zeroed", 0) > 0


def test_pins_leave_enough_pixels(frame):
    """what the per-pixel GPU pins will compare, from the restatement alone on the oracle's G-buffer of frame 0 (no history yet): initial
    visibility, the spatial pass Raytraced with 2 samples (8 on this first frame: the disocclusion boost), final shading. Pixels within
    1e-5 of a decision stay below 25 % of the valid ones and the compared ones above 30 % of all. Then the same with a synthetic
    history, for the rules only: initial visibility empties pixels, both passes zero terms, final shading reuses and traces."""
    f = frame
    st = {}
    iv, m0, emptied = V.initial_visibility(f["cur"], f["fresh"], f["lights"], f["occ"], 8)
    # (no boiling filter here: its cut depends on the tile's real weights, which the synthetic frame does not have)
    t, m1 = R.temporal_pass(f["cur"], None, f["mv"], iv, None, f["lights"], 7, f["bsdf"], 20, True, False, 0.2, in_margin=m0, occ=f["occ"], raytraced=True)
    s, m2 = R.spatial_pass(f["cur"], t, m1, f["lights"], f["table"], 7, f["bsdf"], 2, 8, 20, 32.0, True, occ=f["occ"], raytraced=True, stats=st)
    out, m3, info = V.final_pass(f["cur"], s, m2, f["lights"], f["occ"], reuse=True, max_age=2, max_distance=16.0)
    valid = f["cur"].valid
    excluded, compared = int((valid & (m3 < NEAR)).sum()), int((valid & (m3 >= NEAR)).sum())
    print(f"frame 0: {compared} compared, {excluded} within {NEAR} of a decision ({excluded / valid.sum():.2%} of valid), {int(emptied.sum())} "
          f"emptied by initial visibility, {st.get('zeroed', 0)} spatial terms zeroed")
    assert excluded < 0.25 * valid.sum() and compared > 0.3 * f["W"] * f["H"]
    assert emptied.sum() > 0 and st.get("zeroed", 0) > 0
    assert info["traced"].any() and not info["reused"].any()             # nothing is old enough on the first frame
    assert (info["vis"][info["traced"]] == 0).all(-1).any() and (info["vis"][info["traced"]] == 1).all(-1).any()   # the bar's shadow is there
    assert ((out["Visibility"][info["traced"]] >> 15) == 0).all()         # traced: d = 0, age 0
    st = {}
    t, m1 = R.temporal_pass(f["cur"], f["prev"], f["mv"], iv, f["history"], f["lights"], 7, f["bsdf"], 20, True, False, 0.2, in_margin=m0,
                            occ=f["occ"], raytraced=True, stats=st)
    assert st.get("zeroed", 0) > 0
    assert ((t["Visibility"] >> 27) >= 1)[t["Age"] > 0].all()             # a history sample's visibility is one frame older
    s, m2 = R.spatial_pass(f["cur"], t, m1, f["lights"], f["table"], 7, f["bsdf"], 2, 8, 20, 32.0, True, occ=f["occ"], raytraced=True)
    out, m3, info = V.final_pass(f["cur"], s, m2, f["lights"], f["occ"], reuse=True, max_age=2, max_distance=16.0)
    assert info["reused"].any() and info["traced"].any()
    assert np.array_equal(out["Visibility"][info["reused"]], s["Visibility"][info["reused"]])      # reused: stored unchanged


def test_discard_empties_only_traced_zero_visibility(frame):
    f = frame
    inf = np.full((f["H"], f["W"]), np.inf)
    keep, _, ik = V.final_pass(f["cur"], f["fresh"], inf, f["lights"], f["occ"])
    drop, _, idr = V.final_pass(f["cur"], f["fresh"], inf, f["lights"], f["occ"], discard=True)
    dark = ik["traced"] & (ik["vis"] == 0).all(-1)
    assert dark.any() and np.array_equal(idr["discarded"], dark)
    assert (drop["LightIndex"][dark] == -1).all() and (drop["W"][dark] == 0).all() and np.array_equal(drop["M"][dark], keep["M"][dark])
    for k in keep:
        assert np.array_equal(keep[k][~dark], drop[k][~dark]), k


# ---- two pixels, two lights, enumerated ------------------------------------------------------------------------------------------
def _expected_estimate(centre, other, phat, vis, raytraced):
    """E[p-hat_c(y) W V_c(y)] at pixel `centre` after initial sampling (one uniform candidate of two lights, initial visibility) at both
    pixels and spatial reuse of `other`'s reservoir with the Basic normalisation (raytraced: the neighbour's term counts visibility),
    over both candidates and the selection coin, in exact rationals"""
    total = Fraction(0)
    for lc in (0, 1):
        for ln in (0, 1):
            res = {}
            for px, l in ((centre, lc), (other, ln)):                    # W = (p / q) / (M p) = 1 / q = 2; blocked: emptied
                res[px] = (l, Fraction(2), 1) if vis[px][l] else (None, Fraction(0), 1)
            yc, Wc, Mc = res[centre]
            yn, Wn, Mn = res[other]
            wc = phat[centre][yc] * Wc * Mc if yc is not None else Fraction(0)
            wn = phat[centre][yn] * Wn * Mn if yn is not None else Fraction(0)
            wsum = wc + wn
            if wsum == 0:
                continue
            for y, from_n, prob in ((yc, False, wc / wsum), (yn, True, wn / wsum)):
                if prob == 0:
                    continue
                p = phat[centre][y]
                pn = phat[other][y] * (vis[other][y] if raytraced else 1)
                Wy = R.spatial_normalise(wsum, p, [(Mc, p), (Mn, pn)], pn if from_n else p, True)
                total += Fraction(1, 4) * prob * p * Wy * vis[centre][y]
    return total


def test_two_pixels_two_lights_raytraced_is_exact_basic_is_dark():
    """pixel B cannot see light 1. Reusing across the shadow edge, Raytraced reproduces the shadowed integrand sum_l p-hat(l) V(l) at both
    pixels exactly; Basic counts B as a source of light 1 in A's denominator although initial visibility never lets B deliver it, and is
    strictly darker at A (the lit side of the edge: penumbra darkening)."""
    F = Fraction
    phat = {"A": [F(3, 2), F(2)], "B": [F(1), F(5, 2)]}
    vis = {"A": [1, 1], "B": [1, 0]}
    truth = {px: sum(p * v for p, v in zip(phat[px], vis[px])) for px in phat}
    for centre, other in (("A", "B"), ("B", "A")):
        assert _expected_estimate(centre, other, phat, vis, True) == truth[centre]
    assert _expected_estimate("A", "B", phat, vis, False) < truth["A"]
    assert _expected_estimate("B", "A", phat, vis, False) == truth["B"]    # the shadowed side loses nothing: its own blocked samples shade to 0
    nothing_blocked = {"A": [1, 1], "B": [1, 1]}
    assert _expected_estimate("A", "B", phat, nothing_blocked, False) == sum(phat["A"]) == _expected_estimate("A", "B", phat, nothing_blocked, True)
