"""CPU tests of the denoiser's rules ("Denoiser"): tests/denoiseref.py in float32 against its own float64
evaluation, the Python mirrors of the two structs against include/ptamd.h, and the motion-vector convention of stage 1 against the
G-buffer restatement of tests/surfaceref.py. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import denoiseref as R

EPS32 = 2.0 ** -24                     # half an fp32 ulp, relative: what one rounded fp32 operation adds
SIZES = [(40, 24), (37, 19)]


def f64_of(bits):
    with np.errstate(invalid="ignore"):                # signalling NaN patterns among the hostile texels
        return R.f16_to_f32(bits).astype(np.float64)


def hostile_pair(W, H, **settings):
    out = []
    for dtype in (np.float32, np.float64):
        d = R.Denoiser(W, H, dtype, **settings)
        frames = []
        for tex in R.synthetic_frames(W, H, seed=W * 131 + H):
            dd, ds = d.process(tex)
            frames.append((dd, ds, d.length.copy(), tex))
        out.append(frames)
    return out


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_temporal_stage_float32_against_float64_on_the_hostile_sequence(size):
    """AtrousIterations = 0 on the synthetic sequence of the GPU test. Every value stage 1 stores is a convex combination of noisy values
    (bilinear weights >= 0 renormalised to 1, then hist + (cur - hist) / n with 1 / n in (0, 1]), so nothing exceeds A, the largest finite
    magnitude among the noisy texels, and a rounding adds at most EPS32 A. Per frame and value: four products and three sums of the
    bilinear read, its division, the three operations of the blend and the two of 1 / n and n: 13 roundings, taken as 16; the history a
    frame reads carries the error of the frames before it with weights that sum to 1, so after F frames 16 F EPS32 A. The fp16 store
    adds half an fp16 ulp on each side. The lengths (at most MaxAccumulatedFrames = 8) are bounded the same way with A = 8. The validity
    tests of the taps are discrete: the bound holds where both evaluations took the same decisions, which the lengths show (a tap that
    flipped would move a length by a weight, not by roundings)."""
    W, H = size
    f32, f64 = hostile_pair(W, H, AtrousIterations=0, MaxAccumulatedFrames=8)
    finite = [np.abs(f64_of(t[3][n])) for t in f32 for n in ("NoisyDiffuse", "NoisySpecular")]
    A = max(float(v[np.isfinite(v)].max()) for v in finite)
    assert A == 65504.0
    for f, (a, b) in enumerate(zip(f32, f64)):
        assert np.abs(a[2].astype(np.float64) - b[2]).max() <= 16 * (f + 1) * EPS32 * 8.0, ("length", f)
        hit = np.isfinite(a[3]["LinearDepth"])
        for ch in (0, 1):
            x, y = f64_of(a[ch])[hit], f64_of(b[ch])[hit]
            bound = 16 * (f + 1) * EPS32 * A + R.ulp16(y)
            err = np.abs(x - y)
            print(f"{W}x{H} frame {f} channel {ch}: largest |float32 - float64| / bound = {float((err / bound).max()):.3e}, "
                  f"texels that differ: {int((a[ch] != b[ch]).sum())}")
            assert (err <= bound).all()
            assert np.array_equal(a[ch][~hit], b[ch][~hit])          # missed pixels: the noisy bits, in both


def test_whole_filter_float32_against_float64_stays_inside_the_accumulated_range():
    """The whole filter (defaults: five a-trous iterations) on eight static frames of two noisy half-planes. The a-trous weights are
    ratios of differences, so an operation count bounds their error only through the smallest luminance scale sigma sqrt(v3) + 1e-4 of
    the run, which shrinks with every iteration: such a bound is valid and useless. What the operations do bound: every a-trous output is
    a normalised mean with weights >= 0 of the temporally accumulated colours of its own side of the edge (no tap crosses it: the
    plane distance is 2 against a scale of 0.05 on one side, the normals' cosine 0.6 against 0.8 on both), whatever the weights came out
    as. So both evaluations lie in the range [lo, hi] those colours span on that side, and differ by at most hi - lo, plus the rounding
    of up to 25 products and sums and one division per iteration on values <= hi: 5 * 51 * EPS32 * hi; the fp16 store adds half an ulp
    on each side. The temporally accumulated colours are the AtrousIterations = 0 outputs of the float64 evaluation."""
    W, H = 40, 24
    rng = np.random.default_rng(11)
    xs = np.mgrid[0:H, 0:W][1]
    sides = [xs < W // 2, xs >= W // 2]
    frames = [R.plain_frame(W, H, np.where(sides[1][..., None], 4.0, 1.0) + rng.uniform(-0.5, 0.5, (H, W, 4)), edge=True) for _ in range(8)]
    runs = {}
    for key, dtype, it in (("f32", np.float32, 5), ("f64", np.float64, 5), ("accumulated", np.float64, 0)):
        d = R.Denoiser(W, H, dtype, AtrousIterations=it)
        for tex in frames:
            out = d.process(tex)
        runs[key] = [R.f16_to_f32(o).astype(np.float64) for o in out]
        assert (d.length == 8).all()
    for ch in (0, 1):
        for k, side in enumerate(sides):
            acc = runs["accumulated"][ch][side]
            lo, hi = acc.min(), acc.max()
            x, y = runs["f32"][ch][side], runs["f64"][ch][side]
            bound = (hi - lo) + 5 * 51 * EPS32 * hi + R.ulp16(hi)
            err = float(np.abs(x - y).max())
            print(f"channel {ch} side {k}: accumulated range [{lo:.4f}, {hi:.4f}], largest |float32 - float64| = {err:.3e} (bound {bound:.3e})")
            assert err <= bound
            for v in (x, y):
                assert v.min() >= lo - 5 * 51 * EPS32 * hi - R.ulp16(lo) and v.max() <= hi + 5 * 51 * EPS32 * hi + R.ulp16(hi)
            assert y.var() < acc.var()                               # and the filter did filter


def test_fma32_is_the_single_rounding_of_the_exact_sum():
    """the emulation against exact rational arithmetic on cases picked to sit on fp32 half-way points, and on random ones"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(2000).astype(np.float32); b = rng.standard_normal(2000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * np.float32(1 + 2.0 ** -12)   # heavy cancellation
    a = np.concatenate([a, np.float32([1 + 2.0 ** -12, 3.0, 1.0])]); b = np.concatenate([b, np.float32([1 + 2.0 ** -12, 2.0 ** -25, 2.0 ** -24])])
    c = np.concatenate([c, np.float32([2.0 ** -30, 1.0, 1.0])])
    got = R.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(Fraction(float(g)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), (x, y, z, g)


def test_python_mirrors_match_the_header(pkg):
    """48 B of settings with the header's fields in the header's order, eight pointers, the defaults the header states"""
    L = pkg.layouts
    ge.load_package()
    import dxpbrt_amd.ptamd as P
    text = open(os.path.join(ge.ROOT, "include", "ptamd.h")).read()
    body = re.search(r"struct PtDenoiserSettings \{[^\n]*\n(.*?)\};\s*/\* 48 B \*/", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?;(?:\s*/\*\s*default ([0-9.]+))?", body, re.M)
    assert [f[1] for f in fields] == list(L.DENOISER_SETTINGS.names)
    offset = 0
    for ctype, name, count, default in fields:
        assert L.DENOISER_SETTINGS.fields[name][1] == offset, name
        base = L.DENOISER_SETTINGS[name].base
        assert base == np.dtype("<u4" if ctype == "uint32_t" else "<f4"), name
        offset += 4 * int(count or 1)
        if default:
            assert float(default) == L.DENOISER_DEFAULTS[name] == R.DEFAULTS[name], name
    assert offset == L.DENOISER_SETTINGS.itemsize == 48
    tex = re.search(r"struct PtDenoiserTextures \{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", tex, flags=re.S))
    assert names == L.DENOISER_TEXTURES and len(names) == 8
    assert C.sizeof(P.DenoiserTextures) == 8 * C.sizeof(C.c_void_p) and [f[0] for f in P.DenoiserTextures._fields_] == names
    for s in ("pt_denoiser_set_constants", "pt_denoiser_process", "pt_denoiser_reset_history", "pt_denoiser_download_history"):
        assert s in P.EXPORTS and re.search(r"\bint\s+%s\(" % s, text), s
    assert re.search(r"#define\s+PTAMD_ABI_VERSION\s+4\b", text)     # symbols only grow


def test_settings_helper_refuses_what_the_library_refuses(pkg):
    L = pkg.layouts
    s = L.denoiser_settings(1920, 1080)
    assert int(s["MaxAccumulatedFrames"]) == 30 and int(s["AtrousIterations"]) == 5 and tuple(s["RenderSize"]) == (1920, 1080)
    assert L.denoiser_settings(1, 16384, MaxAccumulatedFrames=1, AtrousIterations=0, DepthThreshold=1.0, NormalCosine=0.0) is not None
    for word, kw in (("MaxAccumulatedFrames", {"MaxAccumulatedFrames": 0}), ("MaxAccumulatedFrames", {"MaxAccumulatedFrames": 256}),
                     ("AtrousIterations", {"AtrousIterations": 9}), ("DepthThreshold", {"DepthThreshold": 0.0}), ("DepthThreshold", {"DepthThreshold": 1.01}),
                     ("NormalCosine", {"NormalCosine": 1.0}), ("NormalCosine", {"NormalCosine": -0.5}), ("DiffuseLuminanceSigma", {"DiffuseLuminanceSigma": 0.0}),
                     ("SpecularLuminanceSigma", {"SpecularLuminanceSigma": float("nan")}), ("RoughnessFraction", {"RoughnessFraction": -1.0}),
                     ("no field", {"Sigma": 1.0}), ("32-bit", {"AtrousIterations": -1})):
        with pytest.raises(ValueError, match=word):
            L.denoiser_settings(64, 64, **kw)
    for w, h in ((0, 8), (8, 0), (16385, 8)):
        with pytest.raises(ValueError, match="RenderSize"):
            L.denoiser_settings(w, h)


def test_motion_vector_convention_against_the_gbuffer_restatement(pkg):
    """Stage 1 takes MotionVector as GBufferGeneration.hlsl:87-90 writes it: xy = (previous screen UV - UV) * size in pixels, z =
    previous view depth - LinearDepth. tests/surfaceref.py restates the G-buffer in float64: on the Cornell box with the previous camera
    translated (the same orientation, no jitter), the point a pixel shows sat, one frame ago, at (x + 0.5 + mv.x, y + 0.5 + mv.y) with
    view depth LinearDepth + mv.z. Here that previous place is worked out from the previous camera's position and axes alone (no
    matrix of the restatement): the way stage 1 reads the vector."""
    import surfaceref as SR
    S = pkg.scenes
    W, H = 24, 16
    sc = S.cornell_box(aspect=W / H, variant="ggx")
    cam = np.array(sc.camera).copy().reshape(())
    assert tuple(cam["Jitter"]) == (0.0, 0.0)
    R3, U3, F3 = (np.asarray(cam[k], np.float64) for k in ("RightDirection", "UpDirection", "ForwardDirection"))
    r, u, f = (v / np.linalg.norm(v) for v in (R3, U3, F3))
    previous = np.asarray(cam["Position"], np.float64) - np.array([0.11, -0.04, 0.07])
    w2v = np.array(cam["PreviousWorldToView"], np.float64)
    w2v[3, :3] = [-previous @ r, -previous @ u, -previous @ f]        # XMMatrixLookToLH at the previous position, row-vector convention
    cam["PreviousWorldToView"] = w2v
    cam["PreviousWorldToProjection"] = w2v @ np.asarray(cam["PreviousViewToProjection"], np.float64)
    cam["PreviousPosition"] = previous
    got = SR.Surface(sc).render(cam, W, H)
    hit = got["hit"]
    assert hit.sum() > W * H // 2
    pos, mv, lin, pix = got["position"][hit], got["motion"][hit], got["linear_depth"][hit], got["pixel"][hit]
    rel = pos - previous
    vx, vy, vz = rel @ r, rel @ u, rel @ f
    px = (vx / (vz * np.linalg.norm(R3) / np.linalg.norm(F3)) * 0.5 + 0.5) * W
    py = (vy / (vz * np.linalg.norm(U3) / np.linalg.norm(F3)) * -0.5 + 0.5) * H
    # float32 camera matrices against float64 geometry: a few 2^-24 of O(1) operands, times the frame size
    assert np.abs((pix[:, 0] + 0.5 + mv[:, 0]) - px).max() < 1e-4 and np.abs((pix[:, 1] + 0.5 + mv[:, 1]) - py).max() < 1e-4
    assert np.abs((lin + mv[:, 2]) - vz).max() < 1e-5
    assert np.abs(mv[:, 0]).max() > 0.5 and np.abs(mv[:, 2]).max() > 0.05      # the camera did move: pixels and depth
