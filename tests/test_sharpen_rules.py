"""CPU tests of the sharpener's rules ("Sharpening"): the Python mirrors of the struct against include/ptamd.h and
host/ptamd.hpp, the settings helper's refusals, tests/sharpenref.py against cases whose answer is known in closed form, and what the pass
is for: a blurred pattern comes closer to the unblurred one. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import sharpenref as R

F = np.float32
ENTRY_POINTS = ("pt_sharpen_set_constants", "pt_sharpen_process")


def rgb_of(bits):
    return R.f16_to_f32(bits)[..., :3]


# ------------------------------------------------------------------------------------------------------------------------------------
# structs and settings
def test_python_mirrors_match_the_header(pkg):
    """32 B of settings with the header's fields in the header's order and the defaults it states, two pointers, the entry points; the
    size is asserted in the header's mirrors (the kernel file, layouts.py, host/ptamd.hpp); what the pass is not is said wherever it is
    described"""
    L = pkg.layouts
    ge.load_package()
    import dxpbrt_amd.ptamd as P
    text = open(os.path.join(ge.ROOT, "include", "ptamd.h")).read()
    body = re.search(r"struct PtSharpenSettings \{[^\n]*\n(.*?)\};\s*/\* 32 B \*/", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?;(?:\s*/\*\s*default ([0-9.]+))?", body, re.M)
    assert [f[1] for f in fields] == list(L.SHARPEN_SETTINGS.names) == ["Size", "Sharpness", "ContrastFloor", "_pad"]
    offset = 0
    for ctype, name, count, default in fields:
        assert L.SHARPEN_SETTINGS.fields[name][1] == offset, name
        assert L.SHARPEN_SETTINGS[name].base == np.dtype("<u4" if ctype == "uint32_t" else "<f4"), name
        offset += 4 * int(count or 1)
        if default:
            assert float(default) == L.SHARPEN_DEFAULTS[name] == R.DEFAULTS[name], name
    assert offset == L.SHARPEN_SETTINGS.itemsize == 32
    assert L.SHARPEN_DEFAULTS == R.DEFAULTS == {"Sharpness": 0.5, "ContrastFloor": 0.015625}
    tex = re.search(r"struct PtSharpenTextures \{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"\*\s*(\w+)", re.sub(r"/\*.*?\*/", "", tex, flags=re.S))
    assert names == L.SHARPEN_TEXTURES == ["Color", "Sharpened"]
    assert C.sizeof(P.SharpenTextures) == 2 * C.sizeof(C.c_void_p) and [f[0] for f in P.SharpenTextures._fields_] == names
    for s in ENTRY_POINTS:
        assert s in P.EXPORTS and re.search(r"\bint\s+%s\(" % s, text) and hasattr(P.load_library(), s), s
    assert sorted(s for s in P.EXPORTS if s.startswith("pt_sharpen_")) == sorted(ENTRY_POINTS)
    assert re.search(r"#define\s+PTAMD_ABI_VERSION\s+4\b", text)     # symbols only grow
    kernel = open(os.path.join(ge.PKG_DIR, "csrc", "pt_sharpen.hip")).read()
    hpp = open(os.path.join(ge.PKG_DIR, "host", "ptamd.hpp")).read()
    for source in (kernel, hpp):
        assert re.search(r"static_assert\(sizeof\(PtSharpenSettings\) == 32", source)
    # the C++ host's defaults are the header's
    m = re.search(r"struct Sharpening \{.*?float Sharpness = ([0-9.]+)f, ContrastFloor = ([0-9.]+)f;", hpp, re.S)
    assert (float(m.group(1)), float(m.group(2))) == (0.5, 0.015625)
    for source in (text, kernel, hpp, P.Sharpening.__doc__):         # what the pass is not, wherever it is described
        assert re.search(r"(?i:not) a\s+port of NVIDIA Image Scaling", re.sub(r"\s*\n\s*(?:\*|//)?\s*", " ", source)), source[:60]


def test_settings_helper_refuses_what_the_library_refuses(pkg):
    L = pkg.layouts
    s = L.sharpen_settings((1920, 1080))
    assert float(s["Sharpness"]) == 0.5 and float(s["ContrastFloor"]) == 0.015625 and tuple(s["Size"]) == (1920, 1080)
    assert not np.asarray(s["_pad"]).any() and s.dtype.itemsize == 32
    assert L.sharpen_settings((1, 16384), Sharpness=0.0, ContrastFloor=2.0 ** -10) is not None
    assert L.sharpen_settings((16384, 1), Sharpness=1.0, ContrastFloor=0.5) is not None
    for word, kw in (("Sharpness", {"Sharpness": -0.01}), ("Sharpness", {"Sharpness": 1.01}), ("Sharpness", {"Sharpness": float("nan")}),
                     ("Sharpness", {"Sharpness": float("inf")}), ("ContrastFloor", {"ContrastFloor": 0.0}),
                     ("ContrastFloor", {"ContrastFloor": 2.0 ** -11}), ("ContrastFloor", {"ContrastFloor": 0.51}),
                     ("ContrastFloor", {"ContrastFloor": float("nan")}), ("no field", {"KernelRadius": 1.0})):
        with pytest.raises(ValueError, match=word):
            L.sharpen_settings((32, 32), **kw)
    for word, size in (("Size", (0, 8)), ("Size", (8, 0)), ("Size", (16385, 8)), ("Size", (8, 16385)), ("32-bit", (-1, 8)), ("pair", (8, 8, 8))):
        with pytest.raises(ValueError, match=word):
            L.sharpen_settings(size)
    raw = np.zeros((), L.SHARPEN_SETTINGS)
    raw["Size"], raw["Sharpness"], raw["ContrastFloor"] = (8, 8), 1.5, 0.015625
    with pytest.raises(ValueError, match="Sharpness"):
        L.check_sharpen_settings(raw)


def test_a_renderer_refuses_a_sharpening_that_is_not_one(pkg):
    """the Python layer's own check, ahead of any device call"""
    ge.load_package()
    import dxpbrt_amd.ptamd as P
    r = object.__new__(P.Renderer)
    r.scene = type("S", (), {"GetTopLevelAccelerationStructure": lambda self: None})()
    r.ctx = None
    with pytest.raises(P.PtInvalidArgument, match="sharpen must be a Sharpening"):
        P.Renderer.render(r, None, sharpen=object())
    with pytest.raises(P.PtInvalidArgument, match="sharpen must be a Sharpening"):
        P.Renderer.render(r, None, sharpen=P.Sharpening(None))     # constants never set


# ------------------------------------------------------------------------------------------------------------------------------------
# closed forms, all bit for bit
def random_frame(w, h, seed, lo=-6, hi=2):
    rng = np.random.default_rng(seed)
    return R.frame(np.exp2(rng.uniform(lo, hi, (h, w, 3))))


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (33, 17)])
def test_a_constant_image_and_sharpness_zero_come_back_unchanged(size):
    w, h = size
    flat = R.frame(np.full((h, w, 3), (0.7, 0.25, 3.0)))
    for sharpness in (0.0, 0.5, 1.0):
        assert R.sharpen(flat, Sharpness=sharpness).tobytes() == flat.tobytes()
    img = random_frame(w, h, 3)
    out = R.sharpen(img, Sharpness=0.0)
    assert out[..., :3].tobytes() == img[..., :3].tobytes() and (out[..., 3] == R.ONE16).all()
    if w * h > 9:
        assert R.sharpen(img, Sharpness=0.5).tobytes() != img.tobytes()      # the same image is sharpened when asked


def line_by_hand(values, vertical, sharpness, floor=0.015625):
    """The spec on a frame that is one texel wide or high, written out for one line of n texels in float32 scalars: every tap off the
    line clamps back onto it. values: (n, 3) float32, finite. horizontal (n x 1): d1 sees the pixel itself five times, d2 and d3 both
    walk the line like d0. vertical (1 x n): d0 sees the pixel itself, d2 walks like d1, d3 walks the line backwards."""
    n = len(values)
    c = [[F(v) for v in px] for px in values]
    at = lambda i: c[min(max(i, 0), n - 1)]
    def lum(px):
        y = R.fma32(px[2], F(0.114), R.fma32(px[1], F(0.587), F(px[0] * F(0.299))))
        return F(y) if y > 0 else F(0)
    Y = [lum(px) for px in c]
    Yat = lambda i: Y[min(max(i, 0), n - 1)]
    h5 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
    steps = (0, 1, 1, -1) if vertical else (1, 0, 1, 1)          # how far along the line one step of d0..d3 moves
    out = []
    for p in range(n):
        lo = [min(at(p + d)[ch] for d in (-1, 0, 1)) for ch in range(3)]
        hi = [max(at(p + d)[ch] for d in (-1, 0, 1)) for ch in range(3)]
        Ylo, Yhi = min(Yat(p + d) for d in (-1, 0, 1)), max(Yat(p + d) for d in (-1, 0, 1))
        s = F(Yhi + Ylo)
        k = F(F(Yhi - Ylo) / s) if s > 0 else F(0)
        d = F(k - F(floor))
        ramp = F((d if d > 0 else F(0)) / F(floor))
        ramp = ramp if ramp < 1 else F(1)
        amount = F(F(F(2) * F(sharpness)) * ramp)
        e = []
        for kk, st in enumerate(steps):
            g = F(Yat(p + st) - Yat(p - st))
            ek = F(g * g)
            e.append(F(ek * F(0.5)) if kk >= 2 else ek)
        E = F(F(F(e[0] + e[1]) + e[2]) + e[3])
        if not (amount > 0 and E > 0):
            out.append(c[p])
            continue
        px = []
        for ch in range(3):
            N = F(0)
            for kk, st in enumerate(steps):
                B = F(0)
                for i in range(-2, 3):
                    B = F(B + F(h5[i + 2] * at(p + i * st)[ch]))
                N = F(N + F(e[kk] * F(c[p][ch] - B)))
            o = F(c[p][ch] + F(amount * F(N / E)))
            o = o if o > lo[ch] else lo[ch]
            o = o if o < hi[ch] else hi[ch]
            px.append(o)
        out.append(px)
    return np.array(out, F)


def test_frames_one_texel_wide_or_high_equal_the_one_dimensional_form():
    one = random_frame(1, 1, 1)
    assert R.sharpen(one, Sharpness=1.0).tobytes() == one.tobytes()          # every tap is the same texel
    changed = 0
    for seed in range(6):
        for sharpness in (0.5, 1.0):
            row = random_frame(7, 1, seed)                                  # 7 x 1: W = 7, H = 1
            want = R.f16(line_by_hand(rgb_of(row)[0], False, sharpness))
            got = R.sharpen(row, Sharpness=sharpness)
            assert got[0, :, :3].tobytes() == want.tobytes() and (got[..., 3] == R.ONE16).all()
            col = random_frame(1, 7, 100 + seed)                            # 1 x 7
            want = R.f16(line_by_hand(rgb_of(col)[:, 0], True, sharpness))
            got = R.sharpen(col, Sharpness=sharpness)
            assert got[:, 0, :3].tobytes() == want.tobytes()
            changed += int((got != col).any())
    assert changed == 12                                                    # the cases are not all gated away


@pytest.mark.parametrize("size,seed", [((16, 16), 1), ((17, 15), 2), ((33, 47), 3), ((48, 32), 4), ((7, 1), 5), ((1, 7), 6)])
@pytest.mark.parametrize("sharpness", [0.5, 1.0])
def test_no_channel_leaves_the_range_of_its_3x3(size, seed, sharpness):
    """every output channel of every pixel lies within the min / max of the guarded input over the pixel's 3 x 3; so non-negative input
    gives non-negative output and a firefly neither spreads nor digs a ring"""
    w, h = size
    img = R.hostile_frame(w, h, seed)
    for floor in (2.0 ** -10, 0.015625):
        out = R.sharpen(img, Sharpness=sharpness, ContrastFloor=floor)
        c = R.guarded_rgb(img)
        lo = np.min([R.tap(c, dx, dy) for dx, dy in R.NEIGHBOURS], 0)
        hi = np.max([R.tap(c, dx, dy) for dx, dy in R.NEIGHBOURS], 0)
        o = rgb_of(out)
        assert np.isfinite(o).all() and (o >= lo).all() and (o <= hi).all() and (out[..., 3] == R.ONE16).all()
    if w >= 9 and h >= 9:                                        # the lone 6000 on the 0.2 wall: it stays, and the wall around it stays flat
        wall = rgb_of(out)[h - 7:, w - 7:]                      # the texels whose 3 x 3 lies on the wall (its first row and column touch the noise)
        assert wall[3, 3, 0] == 6000 and np.count_nonzero(wall != F(np.float16(0.2))) == 3


def test_the_pass_commutes_with_exposure_bit_for_bit():
    """input in [2^-6, 2^6]: nothing leaves fp16's normal range under a scale of 4 or 1/4, every operation of the spec is homogeneous
    and a power of two scales every intermediate exactly"""
    img = random_frame(40, 28, 11, lo=-6, hi=6)
    base = rgb_of(R.sharpen(img, Sharpness=1.0))
    assert (R.sharpen(img, Sharpness=1.0) != img).any()
    for scale in (4.0, 0.25):
        scaled = R.frame(rgb_of(img).astype(np.float64) * scale)
        assert (rgb_of(scaled) == rgb_of(img) * F(scale)).all()
        assert (rgb_of(R.sharpen(scaled, Sharpness=1.0)) == base * F(scale)).all()


def test_a_blurred_step_gets_its_shoulders_moved_by_the_closed_form_amount():
    """A vertical step blurred to 0.1 | 0.3 0.5 0.7 | 0.9, Sharpness 1. A frame that is constant along y is, row by row, the 7 x 1 form:
    d1 sees the pixel itself, d2 and d3 see the row. Flats: the high-pass pushes them outwards, the 3 x 3 range holds them. Centre: the
    high-pass is 0 in exact arithmetic, -5e-5 on the fp16 values, less than half an fp16 step. Shoulders: contrast 2/3 (the ramp is 1,
    amount 2), every direction has the same H = s - B, so D = H and o = s + 2 (s - B) with B = 0.3125 a + 0.375 s + 0.25 * 0.5 +
    0.0625 t: 0.275 and 0.725 in exact arithmetic on exact inputs. The assertion is on the float32 value of the spec, computed by
    line_by_hand; that this value is 0.275 / 0.725 is checked to the error the fp16 inputs and the fp16 store leave. Half an fp16 step is
    2^-15 at 0.1, 2^-13 at 0.3, 2^-12 at 0.7 and 0.9. Lower shoulder: o = 2.25 s - 0.625 a - 0.125 - 0.125 t is off by 2.25 * 2^-13 +
    0.625 * 2^-15 + 0.125 * 2^-12 = 3.3e-4 at most, the store adds 2^-13: under two steps of 2^-12. Upper shoulder: o = 2.25 t - 0.625 b -
    0.125 - 0.125 s is off by 2.875 * 2^-12 + 0.125 * 2^-13 = 7.2e-4 at most, the store adds 2^-12: under two steps of 2^-11."""
    profile = [0.1] * 4 + [0.3, 0.5, 0.7] + [0.9] * 4
    img = R.frame(np.tile(np.array(profile)[None, :, None], (6, 1, 3)))
    out = R.sharpen(img, Sharpness=1.0)
    assert (out == out[0]).all()                                 # every row the same, the border rows too
    want = R.f16(line_by_hand(rgb_of(img)[0], False, 1.0))
    assert out[0, :, :3].tobytes() == want.tobytes()
    for x in (0, 1, 2, 3, 5, 7, 8, 9, 10):                       # the flats and the centre: exact
        assert (out[:, x, :3] == img[:, x, :3]).all(), x
    got = rgb_of(out)[0, :, 0].astype(np.float64)
    print(f"step shoulders: {got[4]:.6f} and {got[6]:.6f} (0.275 and 0.725 in exact arithmetic)")
    assert abs(got[4] - 0.275) <= 2 * 2.0 ** -12 and abs(got[6] - 0.725) <= 2 * 2.0 ** -11
    assert got[4] < rgb_of(img)[0, 4, 0] and got[6] > rgb_of(img)[0, 6, 0]


def test_a_linear_ramp_changes_by_at_most_one_fp16_step():
    """A linear signal has no high-pass. (a) Ramps whose texels are exact in fp16 (1.5 + (x - 16) / 64 + (y - 12) / 128 and its mirror images, inside
    one binade): every product and partial sum of B is exact in float32, B = c, H = 0: unchanged bit for bit where the 17 taps lie
    inside the frame, at Sharpness 1 with the gate at its lowest (contrast 0.0234 / v, far above 2^-10: amount is 2 everywhere). (b) A ramp rounded to fp16 (1 + 0.02 x + 0.01 y): each texel is off by
    half a step at most, H = 0.625 c - 0.25 (c-1 + c+1) - 0.0625 (c-2 + c+2) by 0.625 steps at most, amount is at most 1 at Sharpness
    0.5: the change rounds to one step at most. Within two texels of the border the replicated taps see a kink, not a ramp; there the
    range limit is what holds (test_no_channel_leaves_the_range_of_its_3x3)."""
    ys, xs = np.mgrid[0:24, 0:32].astype(np.float64)
    inner = (slice(2, -2), slice(2, -2))
    for sx, sy in ((1, 1), (-1, 1), (1, -1)):
        v = 1.5 + sx * (xs - 16) / 64 + sy * (ys - 12) / 128
        img = R.frame(v)
        assert (rgb_of(img)[..., 0] == v).all() and v.min() >= 1 and v.max() < 2
        assert R.active_mask(img, Sharpness=1.0, ContrastFloor=2.0 ** -10).any()     # not gated away: the borders do move
        out = R.sharpen(img, Sharpness=1.0, ContrastFloor=2.0 ** -10)
        assert (out[inner] == img[inner]).all()
    v = 1 + 0.02 * xs + 0.01 * ys
    assert v.max() < 2
    img = R.frame(v)
    out = R.sharpen(img, Sharpness=0.5)
    steps = np.abs(rgb_of(out)[inner].astype(np.float64) - rgb_of(img)[inner]) / 2.0 ** -10
    print(f"quantised ramp: largest change {steps.max():.0f} fp16 steps, {np.count_nonzero(steps)} of {steps.size} channels changed")
    assert steps.max() <= 1


# ------------------------------------------------------------------------------------------------------------------------------------
# what the pass is for
def test_a_blurred_pattern_comes_closer_to_the_unblurred_one():
    """the 96 x 64 pattern of edges and a band-limited wave, blurred once per axis by [1, 2, 1] / 4 (wrap-around), stored as fp16: the RMS
    error against the unblurred pattern on the interior (4 texels from every border: the wrap-around, nothing else) is smaller after
    the pass than before it, and the smaller the higher Sharpness. The ratios are in DESIGN.md section 1, "Sharpening"."""
    truth = R.pattern()
    img = R.frame(R.blur121(truth))
    inner = (slice(4, -4), slice(4, -4))
    rms = lambda bits: float(np.sqrt(((rgb_of(bits).astype(np.float64) - truth)[inner] ** 2).mean()))
    before = rms(img)
    after = [rms(R.sharpen(img, Sharpness=s)) for s in (0.25, 0.5, 1.0)]
    print("blurred pattern: rms before %.5f; after / before at Sharpness 0.25, 0.5, 1: %s" % (before, ", ".join("%.3f" % (a / before) for a in after)))
    for scale in (8.0, 100.0):
        scaled = R.frame(R.blur121(truth) * scale)
        r = float(np.sqrt(((rgb_of(R.sharpen(scaled, Sharpness=0.5)).astype(np.float64) - truth * scale)[inner] ** 2).mean()))
        r0 = float(np.sqrt(((rgb_of(scaled).astype(np.float64) - truth * scale)[inner] ** 2).mean()))
        print("  input scaled by %g: after / before at Sharpness 0.5: %.3f" % (scale, r / r0))
    assert after[0] < before and after[1] < before and after[2] < before
    assert after[0] > after[1] > after[2]


def test_noise_below_the_contrast_floor_comes_back_bit_identical():
    """a flat 0.5 frame with Gaussian noise of sigma 0.002: the contrast of a 3 x 3 is its range over its sum, about 6 sigma / 1 = 0.012 at
    the most likely extreme, under the floor of 1 / 64"""
    rng = np.random.default_rng(7)
    img = R.frame(0.5 + rng.normal(0.0, 0.002, (32, 48, 3)))
    assert len(np.unique(img[..., :3])) > 8
    assert R.sharpen(img, Sharpness=1.0).tobytes() == img.tobytes()
