"""CPU tests of the frame interpolator's rules ("Frame generation"): the Python mirrors of the structs against
include/ptamd.h and host/ptamd.hpp, the settings helper's refusals, tests/framegenref.py against cases whose answer is known in closed
form, and what the pass is for: on an analytic sequence the generated frame is closer to the true middle frame than the previous frame
repeated and than the blend without motion. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import framegenref as R

F = np.float32
ENTRY_POINTS = ("pt_frame_generation_set_constants", "pt_frame_generation_process", "pt_frame_generation_reset_history",
                "pt_frame_generation_download_field")


def f32_of(bits):
    return R.f16_to_f32(bits)


def blend16(prev_bits, cur_bits, phi):
    """prev + (cur - prev) phi in float32 on the fp16 values, stored as fp16, alpha 1"""
    p, c = f32_of(prev_bits)[..., :3], f32_of(cur_bits)[..., :3]
    out = np.empty(prev_bits.shape, np.uint16)
    out[..., :3] = R.f_to_f16((p + (c - p) * F(phi)).astype(F))
    out[..., 3] = R.ONE16
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# structs and settings
def test_python_mirrors_match_the_header(pkg):
    """48 B of settings with the header's fields in the header's order and the defaults it states, five pointers, the class enum, the
    entry points; the size is asserted in the header's three mirrors (the kernel file, layouts.py, host/ptamd.hpp)"""
    L = pkg.layouts
    ge.load_package()
    import dxpbrt_amd.ptamd as P
    text = open(os.path.join(ge.ROOT, "include", "ptamd.h")).read()
    body = re.search(r"struct PtFrameGenerationSettings \{[^\n]*\n(.*?)\};\s*/\* 48 B \*/", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?;(?:\s*/\*\s*default ([0-9.]+))?", body, re.M)
    assert [f[1] for f in fields] == list(L.FRAME_GENERATION_SETTINGS.names)
    offset = 0
    for ctype, name, count, default in fields:
        assert L.FRAME_GENERATION_SETTINGS.fields[name][1] == offset, name
        assert L.FRAME_GENERATION_SETTINGS[name].base == np.dtype("<u4" if ctype == "uint32_t" else "<f4"), name
        offset += 4 * int(count or 1)
        if default:
            assert float(default) == L.FRAME_GENERATION_DEFAULTS[name] == R.DEFAULTS[name], name
    assert offset == L.FRAME_GENERATION_SETTINGS.itemsize == 48
    assert set(L.FRAME_GENERATION_DEFAULTS) == set(R.DEFAULTS) == {"Phase", "DepthThreshold"}
    tex = re.search(r"struct PtFrameGenerationTextures \{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"\*\s*(\w+)", re.sub(r"/\*.*?\*/", "", tex, flags=re.S))
    assert names == L.FRAME_GENERATION_TEXTURES and len(names) == 5
    assert C.sizeof(P.FrameGenerationTextures) == 5 * C.sizeof(C.c_void_p) and [f[0] for f in P.FrameGenerationTextures._fields_] == names
    enum = re.search(r"enum PtFrameGenerationClass \{(.*?)\};", text, re.S).group(1)
    values = dict((k, int(v)) for k, v in re.findall(r"PT_FRAME_GENERATION_(\w+) = (\d+)", enum))
    assert values == {"BOTH": R.BOTH, "CURRENT_ONLY": R.CURRENT_ONLY, "PREVIOUS_ONLY": R.PREVIOUS_ONLY, "FALLBACK": R.FALLBACK}
    assert values == {k: getattr(L, "FRAME_GENERATION_" + k) for k in values}
    assert int(R.EMPTY) == L.FRAME_GENERATION_EMPTY
    for s in ENTRY_POINTS:
        assert s in P.EXPORTS and re.search(r"\bint\s+%s\(" % s, text) and hasattr(P.load_library(), s), s
    assert sorted(s for s in P.EXPORTS if s.startswith("pt_frame_generation_")) == sorted(ENTRY_POINTS)
    assert re.search(r"#define\s+PTAMD_ABI_VERSION\s+4\b", text)     # symbols only grow
    kernel = open(os.path.join(ge.PKG_DIR, "csrc", "pt_framegen.hip")).read()
    hpp = open(os.path.join(ge.PKG_DIR, "host", "ptamd.hpp")).read()
    for source in (kernel, hpp):
        assert re.search(r"static_assert\(sizeof\(PtFrameGenerationSettings\) == 48", source)
    for source in (text, kernel, hpp, P.FrameGeneration.__doc__):    # what the pass is not, wherever it is described
        assert re.search(r"(?i:not) a\s+port of DLSS-G or\s+FSR 3", re.sub(r"\s*\n\s*(?:\*|//)?\s*", " ", source)), source[:60]


def test_settings_helper_refuses_what_the_library_refuses(pkg):
    L = pkg.layouts
    s = L.frame_generation_settings((960, 540), (1920, 1080))
    assert float(s["Phase"]) == 0.5 and float(s["DepthThreshold"]) == np.float32(0.01) and tuple(s["OutputSize"]) == (1920, 1080)
    assert not np.asarray(s["_pad"]).any() and s.dtype.itemsize == 48
    assert L.frame_generation_settings((1, 4096), (4, 16384), Phase=0.25, DepthThreshold=1.0) is not None
    assert L.frame_generation_settings((37, 19), (37, 19), Phase=0.999) is not None
    for word, kw in (("Phase", {"Phase": 0.0}), ("Phase", {"Phase": 1.0}), ("Phase", {"Phase": -0.5}), ("Phase", {"Phase": float("nan")}),
                     ("DepthThreshold", {"DepthThreshold": 0.0}), ("DepthThreshold", {"DepthThreshold": 1.01}),
                     ("DepthThreshold", {"DepthThreshold": float("nan")}), ("no field", {"KernelRadius": 1.0})):
        with pytest.raises(ValueError, match=word):
            L.frame_generation_settings((32, 32), (64, 64), **kw)
    for word, render, output in (("RenderSize", (0, 8), (8, 8)), ("RenderSize", (16385, 8), (16385, 8)), ("OutputSize", (8, 8), (8, 0)),
                                 ("OutputSize", (8192, 8), (16385, 8)), ("4 RenderSize", (8, 8), (7, 8)), ("4 RenderSize", (8, 8), (8, 33)),
                                 ("32-bit", (-1, 8), (8, 8))):
        with pytest.raises(ValueError, match=word):
            L.frame_generation_settings(render, output)
    raw = np.zeros((), L.FRAME_GENERATION_SETTINGS)
    raw["RenderSize"], raw["OutputSize"], raw["Phase"], raw["DepthThreshold"] = (8, 8), (8, 8), 1.5, 0.01
    with pytest.raises(ValueError, match="Phase"):
        L.check_frame_generation_settings(raw)


def test_a_renderer_refuses_generate_without_post(pkg):
    """the Python layer's own check, ahead of any device call"""
    ge.load_package()
    import dxpbrt_amd.ptamd as P
    r = object.__new__(P.Renderer)
    r.scene = type("S", (), {"GetTopLevelAccelerationStructure": lambda self: None})()
    r.ctx = None
    with pytest.raises(P.PtInvalidArgument, match="generate needs post"):
        P.Renderer.render(r, None, generate=object.__new__(P.FrameGeneration))


# ------------------------------------------------------------------------------------------------------------------------------------
# closed-form cases
@pytest.mark.parametrize("phi", [0.5, 0.25])
@pytest.mark.parametrize("render,output", [((20, 12), (40, 24)), ((25, 13), (37, 19)), ((37, 19), (37, 19))])
def test_a_static_scene_is_the_blend_bit_for_bit(render, output, phi):
    """Motion 0 everywhere, one depth: every cell of the field is taken by its own pixel (q + 0.5 + J floors to q for J in [-0.5, 0.5)),
    both taps sit on the pixel's centre with the weights 1, 0, 0, 0, both depth tests compare equal depths: class "both" and
    prev + (cur - prev) phi in every pixel, at every ratio and jitter."""
    rng = np.random.default_rng(5)
    ref = R.FrameGeneration(render, output, Phase=phi)
    frames = [R.plain_frame(render, output, np.exp2(rng.uniform(-6, 2, (output[1], output[0], 3)))) for _ in range(3)]
    g, g8, did = ref.process(frames[0], R.U.jitter(0, render, output))
    assert not did and g.tobytes() == frames[0]["Color"].tobytes() and ref.field is None
    for f in (1, 2):
        g, g8, did = ref.process(frames[f], R.U.jitter(f, render, output))
        assert did and (ref.classes == R.BOTH).all()
        assert (ref.field & np.uint64(0xFFFFFFFF) == np.arange(render[0] * render[1], dtype=np.uint64).reshape(render[1], render[0])).all()
        want = blend16(frames[f - 1]["Color"], frames[f]["Color"], phi)
        assert g.tobytes() == want.tobytes()
        assert g8.tobytes() == R.pack8(want).tobytes() and (g8 >> 24 == 255).all()


def test_a_plane_translating_by_an_even_number_of_pixels_comes_out_shifted_by_half():
    """Native size, jitter 0, Phase 0.5. The plane's texture T moves by (4, 2) pixels a frame: prev = T(x, y), cur = T(x - 4, y - 2),
    MotionVector = (-4, -2). The surface pixel q shows lands in cell q - (2, 1); the output pixel o then reads cur at o + (2, 1) and prev
    at o - (2, 1), both on pixel centres: T(o - (2, 1)) twice, and prev + (cur - prev) / 2 of equal values is that value. Away from the
    borders (4 pixels: where a tap or a source would lie outside) Generated is T shifted by (2, 1), to the bit."""
    w, h, dx, dy = 32, 24, 4, 2
    rng = np.random.default_rng(8)
    T = np.exp2(rng.uniform(-4, 1, (h + 2 * dy, w + 2 * dx, 3))).astype(np.float16).astype(np.float32)     # the texture, with a margin
    def shown(shift_x, shift_y):                                # T(x - shift) over the frame
        return T[dy * 2 - shift_y: dy * 2 - shift_y + h, dx * 2 - shift_x: dx * 2 - shift_x + w]
    ref = R.FrameGeneration((w, h), (w, h))
    ref.process(R.plain_frame((w, h), (w, h), shown(0, 0), motion=(-dx, -dy, 0.0)), (0.0, 0.0))
    g, _, did = ref.process(R.plain_frame((w, h), (w, h), shown(dx, dy), motion=(-dx, -dy, 0.0)), (0.0, 0.0))
    assert did
    want = R.f16(shown(dx // 2, dy // 2))
    m = 4
    assert (g[m:-m, m:-m, :3] == want[m:-m, m:-m]).all()
    assert (ref.classes[m:-m, m:-m] == R.BOTH).all()


def test_a_square_moving_over_a_static_background_leaves_the_disocclusion_classes():
    """Native size, jitter 0, Phase 0.5. A square at depth 4 covers x in [8, 16) in the previous frame and [10, 18) in this one (rows 6 to
    13), over a static background at depth 10; at the middle it covers [9, 17). Behind it, at x = 8, the background is seen by this frame
    only (the previous one shows the square there: its depth fails the test): "current only", the side the square uncovers. Ahead of it,
    at x = 17, no pixel of this frame lands (the square's pixel 17 goes to 16): the cell is a hole, the farthest neighbour is the
    background of cell 18, whose current tap is the square (rejected) and whose previous tap is the background: "previous only", the side
    the square is about to cover. (The issue words the two sides the other way round; a background pixel that the square uncovers is
    visible in the current frame alone, whichever pass looks at it.)"""
    w, h = 28, 20
    rng = np.random.default_rng(3)
    B = np.exp2(rng.uniform(-3, 0, (h, w, 3)))
    S = np.full(3, 1.5)
    ys, xs = np.mgrid[0:h, 0:w]
    rows = (ys >= 6) & (ys < 14)
    def frame(x0):
        sq = rows & (xs >= x0) & (xs < x0 + 8)
        mv = np.zeros((h, w, 3))
        mv[sq, 0] = -2.0
        return R.plain_frame((w, h), (w, h), np.where(sq[..., None], S, B), depth=np.where(sq, 4.0, 10.0), motion=mv), sq
    ref = R.FrameGeneration((w, h), (w, h))
    prev, _ = frame(8)
    cur, _ = frame(10)
    ref.process(prev, (0.0, 0.0))
    g, _, did = ref.process(cur, (0.0, 0.0))
    c = ref.classes
    inner = slice(7, 13)                                       # rows whose 3 x 3 lies inside the square's rows
    assert (c[inner, 8] == R.CURRENT_ONLY).all() and (c[inner, 17] == R.PREVIOUS_ONLY).all()
    assert (c[inner, 9:17] == R.BOTH).all() and (c[inner, :8] == R.BOTH).all() and (c[inner, 18:] == R.BOTH).all()
    assert ref.field[8, 17] == R.EMPTY and ref.candidates[8, 9] == 2     # the square's pixel 10 and the background's pixel 9
    middle = np.where((rows & (xs >= 9) & (xs < 17))[..., None], S, B)
    assert (g[inner, :, :3] == R.f16(middle)[inner]).all()      # the true middle frame, in those rows


def test_every_pixel_scattering_into_one_cell_keeps_the_nearest_then_the_lower_index():
    w, h, tx, ty = 6, 4, 2, 1
    ys, xs = np.mgrid[0:h, 0:w]
    mv = np.zeros((h, w, 3))
    mv[..., 0], mv[..., 1] = 2.0 * (tx - xs), 2.0 * (ty - ys)
    z = 3.25 + ((xs * 7 + ys * 5) % 11) * 0.25
    z[0, 0] = z[2, 3] = 3.0                                    # the nearest, twice: the lower index wins
    z[3, 5] = np.inf                                           # sky has no motion: it stays in its own cell, keyed as +inf
    assert z.min() == 3.0 and (z == 3.0).sum() == 2 and z[0, 0] == 3.0
    ref = R.FrameGeneration((w, h), (w, h))
    a = R.plain_frame((w, h), (w, h), 0.5, depth=z, motion=mv)
    ref.process(a, (0.0, 0.0))
    ref.process(a, (0.0, 0.0))
    assert ref.candidates[ty, tx] == w * h - 1 and ref.candidates[3, 5] == 1 and ref.candidates.sum() == w * h
    want = np.full((h, w), R.EMPTY, np.uint64)
    want[ty, tx] = np.uint64(np.float32(3.0).view(np.uint32)) << np.uint64(32) | np.uint64(0)
    want[3, 5] = np.uint64(R.SKY_BITS) << np.uint64(32) | np.uint64(3 * w + 5)
    assert (ref.field == want).all()
    # sky alone in a cell keys as +inf; with a surface it loses
    z2 = np.full((h, w), np.nan)
    z2[1, 1] = 2.0
    b = R.plain_frame((w, h), (w, h), 0.5, depth=z2, motion=mv)
    ref.process(b, (0.0, 0.0))
    assert ref.field[ty, tx] == np.uint64(np.float32(2.0).view(np.uint32)) << np.uint64(32) | np.uint64(1 * w + 1)
    z2[1, 1] = -1.0                                            # a depth that is not in front of the camera is sky too
    for _ in range(2):                                         # twice: the second call's previous frame is all sky too
        ref.process(R.plain_frame((w, h), (w, h), 0.5, depth=z2, motion=np.zeros(3)), (0.0, 0.0))
    assert (ref.field >> np.uint64(32) == np.uint64(R.SKY_BITS)).all() and (ref.classes == R.BOTH).all()


def test_the_hostile_sequence_meets_every_case_it_is_there_for():
    """what the GPU test's sequence contains, counted on the restatement: all four classes, holes filled from the 3 x 3, cells with more
    than one candidate, sky sources, finite output"""
    seen = set()
    for render, output in (((20, 12), (40, 24)), ((25, 13), (37, 19)), ((13, 7), (39, 21)), ((37, 19), (37, 19))):
        for phi in (0.5, 0.25):
            ref = R.FrameGeneration(render, output, Phase=phi)
            for f, (tex, jitter) in enumerate(R.synthetic_frames(render, output, seed=render[0] * 131 + output[0])):
                g, g8, did = ref.process(tex, jitter)
                assert did == (f > 0)
                if did:
                    seen |= set(np.unique(ref.classes).tolist())
                    assert ref.candidates.max() >= 3 and (ref.field == R.EMPTY).any()
                    assert (ref.field >> np.uint64(32) == np.uint64(R.SKY_BITS)).any()
                    assert np.isfinite(f32_of(g)).all() and (g[..., 3] == R.ONE16).all()
    assert seen == {R.BOTH, R.CURRENT_ONLY, R.PREVIOUS_ONLY, R.FALLBACK}


# ------------------------------------------------------------------------------------------------------------------------------------
# quality
def test_the_generated_frame_beats_the_repeated_frame_and_the_blend():
    """40 x 30, native: a band-limited textured plane sliding by (0.6, 0.25) pixels a frame (sub-pixel) and a nearer textured square moving
    by (3, 1) (multi-pixel). The frames at t = 0 and 1 go through the restatement; the truth is the scene rendered analytically at
    t = 0.5. The inequalities only; the ratios are in DESIGN.md section 1, "Frame generation"."""
    size = (40, 30)
    ref = R.FrameGeneration(size, size)
    prev, prev_rgb = R.analytic_frame(size, 0.0)
    cur, cur_rgb = R.analytic_frame(size, 1.0)
    _, truth = R.analytic_frame(size, 0.5)
    ref.process(prev, (0.0, 0.0))
    g, _, did = ref.process(cur, (0.0, 0.0))
    assert did
    got = f32_of(g)[..., :3].astype(np.float64)
    rms = lambda a: float(np.sqrt(((a - truth) ** 2).mean()))
    e = {"generated": rms(got), "repeated": rms(prev_rgb), "blend": rms(0.5 * (prev_rgb + cur_rgb))}
    counts = np.bincount(ref.classes.ravel(), minlength=4).tolist()
    print(f"analytic sequence {size}: rms against the middle frame: generated {e['generated']:.5f}, previous frame repeated {e['repeated']:.5f} "
          f"(ratio {e['generated'] / e['repeated']:.3f}), blend without motion {e['blend']:.5f} (ratio {e['generated'] / e['blend']:.3f}); "
          f"classes both / current / previous / fallback {counts}")
    assert e["generated"] < e["repeated"] and e["generated"] < e["blend"]
