"""GPU tests of the sharpener (pt_sharpen_*; DESIGN.md section 1, "Sharpening"): the device against tests/sharpenref.py byte for byte on
hostile frames at sizes below the halo, of whole tiles and of tiles that do not fill; the refusals; the pass inside Renderer.render between
the upscaler (or the reconstruction, or the frame) and the post chain; the C++ host."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import sharpenref as R
import upscaleref as U

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
# frames smaller than the halo; one tile exactly; a tile that does not fill; several tiles that do not fill; tiles that fill
SIZES = [(1, 1), (1, 7), (7, 1), (16, 16), (17, 15), (33, 47), (48, 32)]
IDS = [f"{w}x{h}" for w, h in SIZES]
FLOORS = [2.0 ** -10, 0.015625, 0.5]
GUARD = 0x1234                                                  # what the texels behind the output hold before and after
GUARD_ROWS = 3


def _torch():
    import torch
    return torch


def device_of(gpu):
    return _torch().device("cuda", gpu.device_ordinal)


def to_device(gpu, bits):
    return _torch().from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).to(device_of(gpu))


def bits_of(t):
    return t.cpu().numpy().view(np.uint16)


def assert_same(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, label
    assert got.tobytes() == want.tobytes(), (label, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


@pytest.fixture
def sharpening(gpu, ptamd):
    gpu.set_sharding(0, 1, 16)
    return ptamd.Sharpening(gpu)


def run(gpu, op, L, bits, **overrides):
    """one call on the device: Sharpened; the input must come back untouched and the guard band behind the output too"""
    torch = _torch()
    h, w = bits.shape[:2]
    color = to_device(gpu, bits)
    target = torch.full((h + GUARD_ROWS, w, 4), GUARD, dtype=torch.int16, device=device_of(gpu))
    op.SetConstants(L.sharpen_settings((w, h), **overrides))
    op.Process({"Color": color, "Sharpened": target})
    gpu.sync()
    assert_same(bits_of(color), bits, "the call wrote Color")
    got = bits_of(target)
    assert (got[h:] == GUARD).all(), "the call wrote behind the W x H output texels"
    return got[:h].copy()


@functools.lru_cache(maxsize=None)
def hostile(w, h):
    return R.hostile_frame(w, h, seed=w * 131 + h)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_hostile_frames_bit_for_bit(gpu, pkg, sharpening, size):
    """normal x 100, negatives, zeros, fp16 subnormals, +-65504, a +inf texel, a texel with one NaN channel, a lone 6000 on a flat 0.2
    wall: every pixel, every byte, Sharpness 0, 0.5 and 1 at the default ContrastFloor and at both ends of its range"""
    w, h = size
    img = hostile(w, h)
    changed = 0
    for sharpness in (0.0, 0.5, 1.0):
        for floor in FLOORS:
            want = R.sharpen(img, Sharpness=sharpness, ContrastFloor=floor)
            got = run(gpu, sharpening, pkg.layouts, img, Sharpness=sharpness, ContrastFloor=floor)
            assert_same(got, want, (size, sharpness, floor))
            changed += int((want[..., :3] != R.f16(R.guarded_rgb(img))).any())
    assert changed >= (4 if w * h > 1 else 0)                   # the cases are not all the identity


def test_smooth_frames_bit_for_bit(gpu, pkg, sharpening):
    """positive frames around the gate, where the contrast ramp and the division by a small E decide: a blurred pattern, a quantised
    ramp, noise at the contrast floor"""
    rng = np.random.default_rng(21)
    ys, xs = np.mgrid[0:47, 0:33].astype(np.float64)
    frames = {"pattern": R.frame(R.blur121(R.pattern(96, 64))[:47, :33]), "ramp": R.frame(1 + 0.02 * xs + 0.01 * ys),
              "noise": R.frame(0.5 + rng.normal(0.0, 0.008, (47, 33, 3))), "dim": R.frame(np.exp2(rng.uniform(-24, -14, (47, 33, 3))))}
    for name, img in frames.items():
        for sharpness in (0.5, 1.0):
            want = R.sharpen(img, Sharpness=sharpness)
            assert_same(run(gpu, sharpening, pkg.layouts, img, Sharpness=sharpness), want, (name, sharpness))
    assert (R.sharpen(frames["pattern"]) != frames["pattern"]).any() and (R.sharpen(frames["noise"]) != frames["noise"]).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
def raw_settings(L, size, **fields):
    s = np.zeros((), L.SHARPEN_SETTINGS)
    s["Size"] = size
    for k, v in dict(L.SHARPEN_DEFAULTS, **fields).items():
        s[k] = v
    return s


def test_refusals_name_the_field_and_keep_the_previous_settings(gpu, ptamd, pkg, sharpening):
    L = pkg.layouts
    torch = _torch()
    w, h = 17, 15
    img = hostile(w, h)
    first = run(gpu, sharpening, L, img, Sharpness=1.0)
    assert (first != run(gpu, sharpening, L, img, Sharpness=0.25)).any()
    sharpening.SetConstants(L.sharpen_settings((w, h), Sharpness=1.0))
    lib, handle = gpu.lib, gpu.handle
    for word, fields, size in (("Sharpness", {"Sharpness": -0.01}, (w, h)), ("Sharpness", {"Sharpness": 1.5}, (w, h)),
                               ("Sharpness", {"Sharpness": float("nan")}, (w, h)), ("Sharpness", {"Sharpness": float("inf")}, (w, h)),
                               ("ContrastFloor", {"ContrastFloor": 0.0}, (w, h)), ("ContrastFloor", {"ContrastFloor": 2.0 ** -11}, (w, h)),
                               ("ContrastFloor", {"ContrastFloor": 0.75}, (w, h)), ("ContrastFloor", {"ContrastFloor": float("nan")}, (w, h)),
                               ("Size", {"Sharpness": 0.25}, (0, h)), ("Size", {"Sharpness": 0.25}, (w, 16385))):
        s = raw_settings(L, size, **fields)
        with pytest.raises(ptamd.PtInvalidArgument, match=word):
            gpu.check(lib.pt_sharpen_set_constants(handle, C.c_void_p(s.ctypes.data)))
    with pytest.raises(ptamd.PtInvalidArgument, match="settings is NULL"):
        gpu.check(lib.pt_sharpen_set_constants(handle, None))
    color = to_device(gpu, img)
    target = torch.full((h, w, 4), GUARD, dtype=torch.int16, device=device_of(gpu))
    # a refused set_constants left the previous settings active: the next process gives the previous result
    sharpening.Process({"Color": color, "Sharpened": target})
    gpu.sync()
    assert_same(bits_of(target), first, "after refused settings")
    target.fill_(GUARD)
    with pytest.raises(ptamd.PtInvalidArgument, match="textures is NULL"):
        gpu.check(lib.pt_sharpen_process(handle, None))
    for name in L.SHARPEN_TEXTURES:
        bind = {"Color": color, "Sharpened": target}
        del bind[name]
        with pytest.raises(ptamd.PtInvalidArgument, match=name + " is NULL"):
            sharpening.Process(bind)
        t = ptamd.SharpenTextures(color.data_ptr(), target.data_ptr())
        setattr(t, name, getattr(t, name) + 4)
        with pytest.raises(ptamd.PtInvalidArgument, match=name + " is not aligned"):
            gpu.check(lib.pt_sharpen_process(handle, C.addressof(t)))
    # the output may not overlap the input anywhere: the same texture, and one that begins in the input's last texel
    both = torch.zeros((2 * h, w, 4), dtype=torch.int16, device=device_of(gpu))
    base, n = both.data_ptr(), w * h * 8
    for color_at, sharpened_at in ((base, base), (base, base + n - 8), (base + n, base + 8)):
        t = ptamd.SharpenTextures(color_at, sharpened_at)
        with pytest.raises(ptamd.PtInvalidArgument, match="Sharpened overlaps Color"):
            gpu.check(lib.pt_sharpen_process(handle, C.addressof(t)))
    t = ptamd.SharpenTextures(base, base + n)                    # back to back is no overlap
    gpu.check(lib.pt_sharpen_process(handle, C.addressof(t)))
    gpu.sync()
    assert (bits_of(target) == GUARD).all()                      # no refused call wrote


def test_process_before_set_constants_is_refused(ptamd, pkg):
    torch = _torch()
    ctx = ptamd.DeviceContext(0)
    try:
        dev = torch.device("cuda", ctx.device_ordinal)
        a, b = (torch.zeros((4, 4, 4), dtype=torch.int16, device=dev) for _ in range(2))
        with pytest.raises(ptamd.PtInvalidArgument, match="pt_sharpen_set_constants"):
            ptamd.Sharpening(ctx).Process({"Color": a, "Sharpened": b})
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# inside the frame: Cornell "ggx", 24 x 16 -> 48 x 32 (Performance), 1 spp, 3 bounces, static camera, Halton jitter
RENDER5, OUTPUT5, BOUNCES5, FRAMES5 = (24, 16), (48, 32), 3, 4


def _settings5(S, L, size, frame, denoiser=None):
    gs = S.graphics_settings(size[0], size[1], spp=1, bounces=BOUNCES5, frame_index=frame)
    gs["Denoiser"] = L.DENOISER_NONE if denoiser is None else denoiser
    return gs


def post_by_hand(gpu, ptamd, L, size, radiance):
    """pt_post_render on `radiance` (device tensor) with textures of its own: (Color, BackBuffer)"""
    post = ptamd.PostProcessing(gpu)
    tex = dict(ptamd.alloc_post_textures(size[0], size[1], device_of(gpu)), Radiance=radiance)
    post.SetConstants(L.post_processing_settings(*size))
    post.Render(tex)
    gpu.sync()
    return tex["Color"].cpu().numpy().view(np.uint16).copy(), tex["BackBuffer"].cpu().numpy().view(np.uint32).copy()


def check_chain(gpu, ptamd, L, r, source, size):
    """Sharpened is the restatement applied to `source`; Color and BackBuffer are the post chain run by hand on Sharpened"""
    gpu.sync()
    t = r.textures
    src, sharpened = bits_of(t[source]).copy(), bits_of(t["Sharpened"]).copy()
    assert sharpened.shape == (size[1], size[0], 4)
    assert_same(sharpened, R.sharpen(src, Sharpness=0.5), "Sharpened of " + source)
    assert (sharpened != src).any()
    color, back = t["Color"].cpu().numpy().view(np.uint16).copy(), t["BackBuffer"].cpu().numpy().view(np.uint32).copy()
    want_color, want_back = post_by_hand(gpu, ptamd, L, size, t["Sharpened"])
    assert_same(color, want_color, "Color after " + source)
    assert_same(back, want_back, "BackBuffer after " + source)
    return sharpened, back


@pytest.fixture(scope="module")
def cornell(gpu, ptamd, pkg):
    """the last frame of the sequence through Renderer.render(settings, upscale=, sharpen=, post=), checked on the way. Rendered once."""
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    gpu.set_debug_flags(0)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=OUTPUT5[0] / OUTPUT5[1], variant="ggx"))
    r = ptamd.Renderer(gpu, g, *RENDER5)
    up = r.upscaler(*OUTPUT5)
    up.ResetHistory()
    sh = r.sharpening(*OUTPUT5)
    post = L.post_processing_settings(*OUTPUT5)
    for f in range(FRAMES5):
        g.desc.camera["Jitter"] = ptamd.upscaler_jitter(f, RENDER5, OUTPUT5)
        r.render(_settings5(S, L, RENDER5, f), upscale=up, sharpen=sh, post=post)
    sharpened, back = check_chain(gpu, ptamd, L, r, "Upscaled", OUTPUT5)
    g.desc.camera["Jitter"] = (0.0, 0.0)
    yield {"scene": g, "sharpened": sharpened, "backbuffer": back}
    g.close()


def test_render_sharpens_what_the_upscaler_wrote_and_post_reads_it(cornell):
    assert cornell["sharpened"].shape == (OUTPUT5[1], OUTPUT5[0], 4) and (cornell["sharpened"][..., 3] == R.ONE16).all()


def test_render_sharpens_the_reconstruction_and_the_plain_frame(gpu, ptamd, pkg, cornell):
    S, L = pkg.scenes, pkg.layouts
    g = cornell["scene"]
    r = ptamd.Renderer(gpu, g, *RENDER5, with_denoiser_outputs=True)
    rr = r.reconstruction(*OUTPUT5)
    rr.ResetHistory()
    sh = r.sharpening(*OUTPUT5)
    for f in range(2):
        g.desc.camera["Jitter"] = ptamd.upscaler_jitter(f, RENDER5, OUTPUT5)
        r.render(_settings5(S, L, RENDER5, f, L.DENOISER_DLSS_RR), reconstruct=rr, sharpen=sh, post=L.post_processing_settings(*OUTPUT5))
    check_chain(gpu, ptamd, L, r, "Reconstructed", OUTPUT5)
    g.desc.camera["Jitter"] = (0.0, 0.0)
    # neither: the frame's own Radiance, at the renderer's size; and without post the pass still writes Sharpened
    r = ptamd.Renderer(gpu, g, *OUTPUT5)
    sh = r.sharpening(*OUTPUT5)
    r.render(_settings5(S, L, OUTPUT5, 0), sharpen=sh, post=L.post_processing_settings(*OUTPUT5))
    check_chain(gpu, ptamd, L, r, "Radiance", OUTPUT5)
    r.render(_settings5(S, L, OUTPUT5, 1), sharpen=sh)
    gpu.sync()
    assert_same(bits_of(r.textures["Sharpened"]), R.sharpen(bits_of(r.textures["Radiance"]), Sharpness=0.5), "Sharpened without post")
    with pytest.raises(ptamd.PtInvalidArgument, match="Size differs"):
        r.render(_settings5(S, L, OUTPUT5, 0), sharpen=ptamd.Renderer(gpu, g, *RENDER5).sharpening(*RENDER5))


def test_cpp_host_writes_the_same_bytes(tmp_path, cornell):
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    out, disp = str(tmp_path / "sharpened.bin"), str(tmp_path / "display.bin")
    cmd = [DEMO, "--upscale", "performance", "--output-size", f"{OUTPUT5[0]}x{OUTPUT5[1]}", "--spp", "1", "--bounces", str(BOUNCES5),
           "--frames", str(FRAMES5), "--sharpen", "0.5", "--post", "--out-sharpened", out, "--out-display", disp]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert_same(np.fromfile(out, np.uint16).reshape(OUTPUT5[1], OUTPUT5[0], 4), cornell["sharpened"], "pt_demo --sharpen 0.5")
    assert_same(np.fromfile(disp, np.uint32).reshape(OUTPUT5[1], OUTPUT5[0]), cornell["backbuffer"], "pt_demo --sharpen 0.5 --post")
    # the value is optional (default 0.5) and a flag may follow it
    p = subprocess.run(cmd[:cmd.index("0.5")] + cmd[cmd.index("0.5") + 1:], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert_same(np.fromfile(out, np.uint16).reshape(OUTPUT5[1], OUTPUT5[0], 4), cornell["sharpened"], "pt_demo --sharpen")
    q = subprocess.run([DEMO, "--width", "32", "--height", "16", "--spp", "1", "--bounces", "1", "--out-sharpened", out], capture_output=True, text=True, timeout=120)
    assert q.returncode != 0 and "--out-sharpened needs --sharpen" in q.stderr


# ------------------------------------------------------------------------------------------------------------------------------------
# reported, not gated
def test_report_the_upscalers_pattern_with_and_without_the_pass(gpu, ptamd, pkg, sharpening):
    """the upscaler's band-limited pattern (tests/test_upscaler_rules.py, resolution_figures: 0.35 x 0.3 cycles per output pixel, 20 x 12 ->
    40 x 24, one jitter period) through the device's upscaler, then through the pass: the RMS error against the pattern after upscale +
    sharpen beside the one after the upscale alone. The figure goes into DESIGN.md section 1, "Sharpening", whichever way it comes out;
    what is asserted is only that the device's pass is the restatement on this frame too."""
    L = pkg.layouts
    torch = _torch()
    render, output, frequency = (20, 12), (40, 24), (0.35, 0.3)
    (Rw, Rh), (Ow, Oh) = render, output
    pattern = lambda X, Y: 0.5 + 0.4 * np.cos(2 * np.pi * (frequency[0] * X + 0.1)) * np.cos(2 * np.pi * frequency[1] * Y)
    oy, ox = np.mgrid[0:Oh, 0:Ow]
    truth = pattern(ox + 0.5, oy + 0.5)
    qy, qx = np.mgrid[0:Rh, 0:Rw]
    up = ptamd.Upscaler(gpu)
    up.SetConstants(L.upscaler_settings(render, output))
    up.ResetHistory()
    color = torch.zeros((Oh, Ow, 4), dtype=torch.int16, device=device_of(gpu))
    for frame in range(U.jitter_count(render, output)):
        j = U.jitter(frame, render, output)
        v = pattern((qx + 0.5 + float(j[0])) * Ow / Rw, (qy + 0.5 + float(j[1])) * Oh / Rh)
        tex = U.plain_frame(render, np.repeat(v[..., None], 3, -1))
        dtex = {k: _torch().from_numpy((a.view(np.int16) if a.dtype == np.uint16 else a).copy()).to(device_of(gpu)) for k, a in tex.items()}
        up.Process(j, dict(dtex, Color=color))
    gpu.sync()
    up.ResetHistory()
    upscaled = bits_of(color).copy()
    rms = lambda bits: float(np.sqrt(np.mean((R.f16_to_f32(bits)[..., 0].astype(np.float64) - truth) ** 2)))
    line = [f"upscaled {rms(upscaled):.4f}"]
    for sharpness in (0.25, 0.5, 1.0):
        got = run(gpu, sharpening, L, upscaled, Sharpness=sharpness)
        assert_same(got, R.sharpen(upscaled, Sharpness=sharpness), ("the upscaler's pattern", sharpness))
        line.append(f"upscaled + sharpened at {sharpness}: {rms(got):.4f} (ratio {rms(got) / rms(upscaled):.3f})")
    print("RMS error against the band-limited pattern: " + "; ".join(line))
