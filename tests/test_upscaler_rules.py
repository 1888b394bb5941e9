"""CPU tests of the upscaler's rules ("Upscaler"): tests/upscaleref.py in float32 against its own float64 evaluation,
the two host helpers against values written out by hand, the Python mirrors of the structs against include/ptamd.h, the settings helper's
refusals, the motion-vector and jitter convention against the G-buffer restatement of tests/surfaceref.py, and what the pass is for: a
pattern above the render grid's Nyquist limit comes out closer to the truth than a bilinear upsample of one frame. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import upscaleref as R

EPS32 = 2.0 ** -24                     # half an fp32 ulp, relative: what one rounded fp32 operation adds
SIZES = [((20, 12), (40, 24)), ((25, 13), (37, 19)), ((13, 7), (39, 21)), ((37, 19), (37, 19))]
IDS = [f"{r[0]}x{r[1]}-{o[0]}x{o[1]}" for r, o in SIZES]


def f64_of(bits):
    with np.errstate(invalid="ignore"):                # signalling NaN patterns among the hostile texels
        return R.f16_to_f32(bits).astype(np.float64)


@pytest.mark.parametrize("render,output", SIZES, ids=IDS)
def test_float32_against_float64_on_the_hostile_sequence(render, output):
    """The synthetic sequence of the GPU test, MaxAccumulatedFrames = 8, in both precisions. What the operations bound, in the tone-mapped
    space the history is kept in (the inverse map multiplies an error by (1 + m)^2, m up to 65504: nothing useful survives it):

    Every stored colour lies in the clamp box of its pixel, [lo, hi] over the in-frame 3 x 3 taps, up to rounding: the current colour is
    a mean with weights >= 0 of taps in the box, the history is clamped into it, the blend hist + (cur - hist) a has a in (0, 1]. The
    mean's 9 products, 9 sums and division and the blend's 3 operations round values <= A = max(|lo|, |hi|): 22 roundings, taken as 32.
    The two evaluations see the same box when they chose the same nearest sample (the box's own values carry one rounding, the division
    of t(c)): so they differ by at most (hi - lo) + 34 EPS32 A, whatever the history did. That holds in every frame.

    The first frame has no history, out = cur = sum(w t) / sum(w), and the weights bound it more tightly: a coordinate is at most 64 =
    2^6, so d = (q + 0.5 + J) - u carries 3 roundings of 2^6 EPS32 each, |d| <= 2, d2 = dx dx + dy dy then at most 2 (2 * 2 * 192) + 3
    * 8 = 1560 EPS32, the division by R^2 = 1 and the subtraction from 1 leave it under 1600 EPS32, and w = max0(.)^2 with the base <=
    1 under dw = 3300 EPS32 (the floor of the nearest tap only lowers an error). A mean whose nine weights are each off by dw moves by
    at most 2 * 9 dw A / sum(w), with sum(w) >= 1 / 64 as the float64 evaluation has it, plus the 32 roundings above.

    n: where neither evaluation found history it is k, the weight of the nearest tap: they differ by at most dw. Everywhere 1 / 64 <=
    n <= MaxAccumulatedFrames."""
    dw = 3300 * EPS32
    runs = []
    for dtype in (np.float32, np.float64):
        u = R.Upscaler(render, output, dtype, MaxAccumulatedFrames=8)
        frames = []
        for tex, jitter in R.synthetic_frames(render, output, seed=render[0] * 131 + output[0]):
            color = u.process(tex, jitter)
            frames.append({"color": color, "n": u.length.astype(np.float64), "hist": u.hist["colour_n"][..., :3].astype(np.float64),
                           "box": tuple(b.astype(np.float64) for b in u.box), "reused": u.reused.copy(), "centre": u.centre,
                           "weights": u.weights.astype(np.float64)})
        runs.append(frames)
    sequence = R.synthetic_frames(render, output, seed=render[0] * 131 + output[0])
    oy, ox = np.mgrid[0:output[1], 0:output[0]]
    for f, (a, b) in enumerate(zip(*runs)):
        # the nearest sample is a floor: the evaluations may differ where (o + 0.5) s - J is an integer up to its three roundings of
        # 2^6 EPS32 (at 3x with the base-3 jitter -1 / 6 it is one exactly, every third pixel) and nowhere else; such a pixel has another box
        j = [float(v) for v in sequence[f][1]]
        v = [(o + 0.5) * (render[k] / output[k]) - j[k] for k, o in enumerate((ox, oy))]
        tie = (np.abs(v[0] - np.round(v[0])) <= 256 * EPS32) | (np.abs(v[1] - np.round(v[1])) <= 256 * EPS32)
        same = (a["centre"][0] == b["centre"][0]) & (a["centre"][1] == b["centre"][1])
        assert (same | tie).all()
        lo, hi = b["box"]
        A = np.maximum(np.abs(lo), np.abs(hi))
        err = np.where(same[..., None], np.abs(a["hist"] - b["hist"]), 0)
        bound = (hi - lo) + 34 * EPS32 * A
        if f == 0:
            assert not a["reused"].any() and not b["reused"].any()
            bound = np.minimum(bound, (18 * dw / b["weights"])[..., None] * A + 32 * EPS32 * A)
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
        print(f"{render}->{output} frame {f}: largest |float32 - float64| / bound = {worst:.3e}, colour texels that differ: "
              f"{int((a['color'] != b['color']).sum())}, reused {int(b['reused'].sum())} of {b['reused'].size}, another nearest sample at {int((~same).sum())}")
        assert (err <= bound).all()
        for run in (a, b):
            assert (run["n"] >= 1 / 64).all() and (run["n"] <= 8).all()
            assert np.isfinite(f64_of(run["color"])).all() and (np.abs(f64_of(run["color"])) <= 65504).all()
            assert (run["color"][..., 3] == R.ONE16).all()
        fresh = ~a["reused"] & ~b["reused"] & same
        assert (np.abs(a["n"] - b["n"])[fresh] <= dw).all()
    assert any(fr["reused"].any() for fr in runs[0][1:]) and any((~fr["reused"]).any() for fr in runs[0][1:])


def test_render_size_against_values_written_out_by_hand(pkg, ptamd):
    """max(1, (output * 10 + r10 / 2) / r10) in integers: 1920 x 1080 at 1.5 is (19200 + 7) / 15 = 1280 and (10800 + 7) / 15 = 720; at
    1.7 (19200 + 8) / 17 = 1129 and (10800 + 8) / 17 = 635; at 2 960 x 540; at 3 (19200 + 15) / 30 = 640 and 360. Auto by the pixel
    count: 1280 x 720 = 921 600 <= 1280 * 800, native; 1920 x 1080 <= 1920 * 1200, quality; 2560 x 1440 <= 2560 * 1600, balanced, (25600
    + 8) / 17 = 1506 and (14400 + 8) / 17 = 847; 3840 x 2160 <= 3840 * 2400, performance; 7680 x 4320 beyond, ultra performance."""
    L = pkg.layouts
    hand = [(L.SUPER_RESOLUTION_NATIVE, (1920, 1080), (1920, 1080)), (L.SUPER_RESOLUTION_QUALITY, (1920, 1080), (1280, 720)),
            (L.SUPER_RESOLUTION_BALANCED, (1920, 1080), (1129, 635)), (L.SUPER_RESOLUTION_PERFORMANCE, (1920, 1080), (960, 540)),
            (L.SUPER_RESOLUTION_ULTRA_PERFORMANCE, (1920, 1080), (640, 360)), (L.SUPER_RESOLUTION_AUTO, (1280, 720), (1280, 720)),
            (L.SUPER_RESOLUTION_AUTO, (1920, 1080), (1280, 720)), (L.SUPER_RESOLUTION_AUTO, (2560, 1440), (1506, 847)),
            (L.SUPER_RESOLUTION_AUTO, (3840, 2160), (1920, 1080)), (L.SUPER_RESOLUTION_AUTO, (7680, 4320), (2560, 1440)),
            (L.SUPER_RESOLUTION_ULTRA_PERFORMANCE, (1, 1), (1, 1)), (L.SUPER_RESOLUTION_PERFORMANCE, (37, 19), (19, 10)),
            (L.SUPER_RESOLUTION_AUTO, (1280, 800), (1280, 800)), (L.SUPER_RESOLUTION_AUTO, (1281, 800), (854, 533))]
    for mode, output, render in hand:
        assert L.upscaler_render_size(mode, output) == render, (mode, output)
        assert ptamd.upscaler_render_size(mode, output) == render, (mode, output)
        assert R.render_size(mode, output) == render
    assert [L.SUPER_RESOLUTION_AUTO, L.SUPER_RESOLUTION_NATIVE, L.SUPER_RESOLUTION_QUALITY, L.SUPER_RESOLUTION_BALANCED,
            L.SUPER_RESOLUTION_PERFORMANCE, L.SUPER_RESOLUTION_ULTRA_PERFORMANCE] == list(range(6)) == [R.MODES.index(m) for m in R.MODES]
    for bad in ((6, (64, 64)), (1, (0, 64)), (1, (64, 16385))):
        with pytest.raises(ValueError):
            L.upscaler_render_size(*bad)
        with pytest.raises(ptamd.PtInvalidArgument):
            ptamd.upscaler_render_size(*bad)


def test_jitter_against_values_written_out_by_hand(pkg, ptamd):
    """20 x 12 -> 40 x 24: ceil(8 * 2 * 2) = 32 points. Index 1 is 0.1 in base 2 and in base 3: (1 / 2, 1 / 3); index 2 is 0.01 and
    0.2: (1 / 4, 2 / 3); index 3 is 0.11 and 0.01: (3 / 4, 1 / 9); index 6 is 0.011 and 0.02: (3 / 8, 2 / 9): each minus a half, in the
    fp32 operations of the loop. 1280 x 720 -> 1920 x 1080 has ceil(8 * 1.5 * 1.5) = 18 points, a native size 8, 13 x 7 -> 39 x 21 72."""
    L = pkg.layouts
    f = np.float32
    third = f(1) / f(3)
    half, quarter = f(0.5), f(0.25)
    hand = {0: (f(0.0), third - half), 1: (f(-0.25), f(2) * third - half), 2: (f(0.25), f(third * third) - half),
            5: (f(f(quarter + f(0.125)) - half), f(f(2) * f(third * third)) - half)}
    render, output = (20, 12), (40, 24)
    for frame, want in hand.items():
        for got in (L.upscaler_jitter(frame, render, output), ptamd.upscaler_jitter(frame, render, output), R.jitter(frame, render, output)):
            assert (f(got[0]).tobytes(), f(got[1]).tobytes()) == (f(want[0]).tobytes(), f(want[1]).tobytes()), (frame, got, want)
    for (render, output), count in ((((20, 12), (40, 24)), 32), (((1280, 720), (1920, 1080)), 18), (((37, 19), (37, 19)), 8), (((13, 7), (39, 21)), 72),
                                    (((25, 13), (37, 19)), R.jitter_count((25, 13), (37, 19)))):
        assert R.jitter_count(render, output) == count
        seq = [ptamd.upscaler_jitter(k, render, output) for k in range(2 * count + 1)]
        assert all(-0.5 <= v < 0.5 for j in seq for v in j)
        assert seq[:count] == seq[count:2 * count] and seq[2 * count] == seq[0]         # the stated period
        assert len(set(seq[:count])) == count                                            # and no shorter one
        assert seq == [L.upscaler_jitter(k, render, output) for k in range(2 * count + 1)]   # the Python restatement, bit for bit
    assert 17 <= R.jitter_count((25, 13), (37, 19)) <= 18
    assert ptamd.upscaler_jitter(2 ** 40 + 5, (20, 12), (40, 24)) == ptamd.upscaler_jitter((2 ** 40 + 5) % 32, (20, 12), (40, 24))
    with pytest.raises(ValueError):
        L.upscaler_jitter(0, (0, 12), (40, 24))
    with pytest.raises(ptamd.PtInvalidArgument):
        ptamd.upscaler_jitter(0, (0, 12), (40, 24))


def test_python_mirrors_match_the_header(pkg):
    """48 B of settings with the header's fields in the header's order, four pointers, the defaults the header states, the enum's values"""
    L = pkg.layouts
    ge.load_package()
    import dxpbrt_amd.ptamd as P
    text = open(os.path.join(ge.ROOT, "include", "ptamd.h")).read()
    body = re.search(r"struct PtUpscalerSettings \{[^\n]*\n(.*?)\};\s*/\* 48 B \*/", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?;(?:\s*/\*\s*default ([0-9.]+))?", body, re.M)
    assert [f[1] for f in fields] == list(L.UPSCALER_SETTINGS.names)
    offset = 0
    for ctype, name, count, default in fields:
        assert L.UPSCALER_SETTINGS.fields[name][1] == offset, name
        assert L.UPSCALER_SETTINGS[name].base == np.dtype("<u4" if ctype == "uint32_t" else "<f4"), name
        offset += 4 * int(count or 1)
        if default:
            assert float(default) == L.UPSCALER_DEFAULTS[name] == R.DEFAULTS[name], name
    assert offset == L.UPSCALER_SETTINGS.itemsize == 48
    assert set(L.UPSCALER_DEFAULTS) == set(R.DEFAULTS) == {"MaxAccumulatedFrames", "KernelRadius", "DepthThreshold"}
    tex = re.search(r"struct PtUpscalerTextures \{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", tex, flags=re.S))
    assert names == L.UPSCALER_TEXTURES and len(names) == 4
    assert C.sizeof(P.UpscalerTextures) == 4 * C.sizeof(C.c_void_p) and [f[0] for f in P.UpscalerTextures._fields_] == names
    enum = re.search(r"enum PtSuperResolutionMode \{(.*?)\};", text, re.S).group(1)
    values = dict((k, int(v)) for k, v in re.findall(r"PT_SUPER_RESOLUTION_(\w+) = (\d+)", enum))
    assert values == {m: i for i, m in enumerate(R.MODES)} == {m: getattr(L, "SUPER_RESOLUTION_" + m) for m in R.MODES}
    for s in ("pt_upscaler_set_constants", "pt_upscaler_process", "pt_upscaler_reset_history", "pt_upscaler_download_history",
              "pt_upscaler_render_size", "pt_upscaler_jitter"):
        assert s in P.EXPORTS and re.search(r"\bint\s+%s\(" % s, text), s
    bits = {n: int(v, 16) for n, v in re.findall(r"#define (PT_(?:DEBUG|DENOISER_FORM|UPSCALER_FORM)_\w+)\s+(0x[0-9a-fA-F]+)u", text)}
    assert bits["PT_UPSCALER_FORM_DIRECT"] == 0x2000 and bits["PT_UPSCALER_FORM_STAGED"] == 0x4000
    assert len(set(bits.values())) == len(bits) and all(v & (v - 1) == 0 for v in bits.values())       # one bit each, none shared
    assert re.search(r"#define\s+PTAMD_ABI_VERSION\s+4\b", text)     # symbols only grow


def test_settings_helper_refuses_what_the_library_refuses(pkg):
    L = pkg.layouts
    s = L.upscaler_settings((960, 540), (1920, 1080))
    assert int(s["MaxAccumulatedFrames"]) == 16 and float(s["KernelRadius"]) == 1.0 and tuple(s["OutputSize"]) == (1920, 1080)
    assert L.upscaler_settings((1, 4096), (4, 16384), MaxAccumulatedFrames=1, KernelRadius=0.75, DepthThreshold=1.0) is not None
    assert L.upscaler_settings((37, 19), (37, 19), MaxAccumulatedFrames=255, KernelRadius=2.0) is not None
    for word, kw in (("MaxAccumulatedFrames", {"MaxAccumulatedFrames": 0}), ("MaxAccumulatedFrames", {"MaxAccumulatedFrames": 256}),
                     ("KernelRadius", {"KernelRadius": 0.7}), ("KernelRadius", {"KernelRadius": 2.5}), ("KernelRadius", {"KernelRadius": float("nan")}),
                     ("DepthThreshold", {"DepthThreshold": 0.0}), ("DepthThreshold", {"DepthThreshold": 1.01}),
                     ("no field", {"NormalCosine": 0.5}), ("32-bit", {"MaxAccumulatedFrames": -1})):
        with pytest.raises(ValueError, match=word):
            L.upscaler_settings((32, 32), (64, 64), **kw)
    for word, render, output in (("RenderSize", (0, 8), (8, 8)), ("RenderSize", (16385, 8), (16385, 8)), ("OutputSize", (8, 8), (8, 0)),
                                 ("OutputSize", (8192, 8), (16385, 8)), ("4 RenderSize", (8, 8), (7, 8)), ("4 RenderSize", (8, 8), (8, 33)),
                                 ("32-bit", (-1, 8), (8, 8))):
        with pytest.raises(ValueError, match=word):
            L.upscaler_settings(render, output)


def test_motion_vector_and_jitter_convention_against_the_gbuffer_restatement(pkg):
    """The pass takes render pixel q as a sample of the scene at q + 0.5 + Jitter (Math::CalculateUV, GBufferGeneration.hlsl:128) and
    MotionVector.xy as measured from there to the unjittered previous screen position (:87-90). tests/surfaceref.py restates the G-buffer
    in float64: on the Cornell box with a static camera, under any jitter, the point a pixel shows projects (through the unjittered
    WorldToProjection) onto q + 0.5 + Jitter, and its motion vector is 0: the history read at (o + 0.5) + mv / s lands on the output
    pixel's own centre, whatever s."""
    import surfaceref as SR
    S = pkg.scenes
    W, H = 24, 16
    sc = S.cornell_box(aspect=W / H, variant="ggx")
    for jitter in ((0.0, 0.0), (0.23, -0.31), (-0.5, 0.4375), R.jitter(5, (W, H), (2 * W, 2 * H))):
        cam = np.array(sc.camera).copy().reshape(())
        cam["Jitter"] = jitter
        got = SR.Surface(sc).render(cam, W, H)
        hit = got["hit"]
        assert hit.sum() > W * H // 2
        pos, mv, pix = got["position"][hit], got["motion"][hit], got["pixel"][hit]
        clip = np.concatenate([pos, np.ones((len(pos), 1))], -1) @ np.asarray(cam["WorldToProjection"], np.float64)
        sx = (clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * W
        sy = (clip[:, 1] / clip[:, 3] * -0.5 + 0.5) * H
        j = np.asarray(cam["Jitter"], np.float64)
        # float32 camera matrices against float64 geometry: a few 2^-24 of O(1) operands, times the frame size
        assert np.abs(sx - (pix[:, 0] + 0.5 + j[0])).max() < 1e-4 and np.abs(sy - (pix[:, 1] + 0.5 + j[1])).max() < 1e-4
        assert np.abs(mv).max() < 1e-4
        for s in (1.0, 2.0 / 3.0, 0.5, 1.0 / 3.0):                # the reprojected position of output pixel o is o + 0.5 to the same accuracy
            assert np.abs(mv[:, :2] / s).max() < 3e-4


def resolution_figures(render=(20, 12), output=(40, 24), frequency=(0.35, 0.3)):
    """A noise-free pattern of `frequency` cycles per output pixel on each axis -- between the render grid's Nyquist limit (0.25 at 2x)
    and the output grid's (0.5) -- sampled at the jittered render positions for one jitter period, through the float32 restatement, and
    the bilinear upsample of the last frame: their RMS errors against the pattern at the output centres."""
    (Rw, Rh), (Ow, Oh) = render, output

    def pattern(X, Y):
        return 0.5 + 0.4 * np.cos(2 * np.pi * (frequency[0] * X + 0.1)) * np.cos(2 * np.pi * frequency[1] * Y)
    oy, ox = np.mgrid[0:Oh, 0:Ow]
    truth = pattern(ox + 0.5, oy + 0.5)
    u = R.Upscaler(render, output, np.float32)
    qy, qx = np.mgrid[0:Rh, 0:Rw]
    for frame in range(R.jitter_count(render, output)):
        j = R.jitter(frame, render, output)
        v = pattern((qx + 0.5 + float(j[0])) * Ow / Rw, (qy + 0.5 + float(j[1])) * Oh / Rh)
        tex = R.plain_frame(render, np.repeat(v[..., None], 3, -1))
        color = u.process(tex, j)
    got = f64_of(color)[..., 0]
    bilinear = R.bilinear_upsample(f64_of(tex["Radiance"])[..., :3], output)[..., 0]
    return float(np.sqrt(np.mean((got - truth) ** 2))), float(np.sqrt(np.mean((bilinear - truth) ** 2)))


def test_a_pattern_above_the_render_grids_nyquist_limit_is_resolved_better_than_bilinear():
    """The inequality only; the figures are recorded in DESIGN.md section 1, "Upscaler": 0.183 against 0.227, a ratio of 0.81 (with the
    clamp box taken over the contributing taps only, as first specified, 0.222: a ratio of 0.98 -- the box then is so tight that the
    history never survives it; hence the box over all in-frame 3 x 3 taps)."""
    upscaled, bilinear = resolution_figures()
    print(f"RMS error against the pattern: upscaled {upscaled:.4f}, bilinear upsample of one frame {bilinear:.4f}, ratio {upscaled / bilinear:.3f}")
    assert upscaled < bilinear
