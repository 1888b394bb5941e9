"""GPU tests of the temporal upscaler (pt_upscaler_*) against tests/upscaleref.py, the numpy restatement of DESIGN.md section 1,
"Upscaler": the hostile synthetic sequence bit for bit in both forms of the kernel, the properties of the pass, the refusals and the
history's life, and the chain G-buffer -> path tracer -> [pack -> denoiser -> compose] -> upscaler -> post end to end, through both hosts."""
import functools
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import upscaleref as R

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
# 2x; a non-integer ratio that differs per axis and fills no 16 x 16 tile; 3x; native
SIZES = [((20, 12), (40, 24)), ((25, 13), (37, 19)), ((13, 7), (39, 21)), ((37, 19), (37, 19))]
IDS = [f"{r[0]}x{r[1]}-{o[0]}x{o[1]}" for r, o in SIZES]
DEBUG_DIRECT, DEBUG_STAGED = 0x2000, 0x4000
FORMS = [("direct", DEBUG_DIRECT), ("staged", DEBUG_STAGED)]
TEXTURES = ("Radiance", "LinearDepth", "MotionVector")


def _torch():
    import torch
    return torch


def upload(tex, dev):
    torch = _torch()
    out = {}
    for k, v in tex.items():
        a = np.ascontiguousarray(v)
        a = a.view(np.int16) if a.dtype == np.uint16 else a
        out[k] = torch.from_numpy(a.copy()).to(dev)
    return out


def download(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def assert_same(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, label
    assert got.tobytes() == want.tobytes(), (label, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


def f64_of(bits):
    with np.errstate(invalid="ignore"):
        return R.f16_to_f32(bits).astype(np.float64)


@pytest.fixture
def upscaler(gpu, ptamd):
    """the context's upscaler with no history; the debug flags and the sharding are put back behind the test"""
    gpu.set_sharding(0, 1, 16)
    u = ptamd.Upscaler(gpu)
    u.ResetHistory()
    yield u
    gpu.set_debug_flags(0)
    gpu.set_sharding(0, 1, 16)
    u.ResetHistory()


def color_target(gpu, output):
    torch = _torch()
    return torch.full((output[1], output[0], 4), 0x1234, dtype=torch.int16, device=torch.device("cuda", gpu.device_ordinal))


def run_frames(gpu, upscaler, L, render, output, frames, **overrides):
    """the sequence of (textures, jitter) through the device: per frame (Color, n); checks the untouched inputs"""
    dev = _torch().device("cuda", gpu.device_ordinal)
    upscaler.SetConstants(L.upscaler_settings(render, output, **overrides))
    upscaler.ResetHistory()
    out = []
    for host, jitter in frames:
        dtex = upload(host, dev)
        color = color_target(gpu, output)
        upscaler.Process(jitter, dict(dtex, Color=color))
        gpu.sync()
        for name in TEXTURES:
            assert_same(download(dtex[name], host[name]), host[name], ("the call wrote", name))
        out.append((color.cpu().numpy().view(np.uint16), upscaler.DownloadHistory()))
    return out


@functools.lru_cache(maxsize=None)
def reference(render, output, max_frames):
    """per frame of the synthetic sequence: (Color, n, reused) of upscaleref in float32. Computed once."""
    ref = R.Upscaler(render, output, np.float32, MaxAccumulatedFrames=max_frames)
    out = []
    for tex, jitter in R.synthetic_frames(render, output, seed=render[0] * 131 + output[0]):
        color = ref.process(tex, jitter)
        out.append((color, ref.length.copy(), ref.reused.copy()))
    return out


@pytest.mark.parametrize("max_frames", [1, 8])
@pytest.mark.parametrize("render,output", SIZES, ids=IDS)
def test_synthetic_sequence_bit_for_bit(gpu, pkg, upscaler, render, output, max_frames):
    """three consecutive hostile frames, a different Halton jitter each: Color and the downloaded n of every frame equal upscaleref's
    bytes, in the direct and in the staged form"""
    frames = R.synthetic_frames(render, output, seed=render[0] * 131 + output[0])
    assert all((~np.isfinite(t["LinearDepth"])).sum() >= render[0] * render[1] // 10 for t, _ in frames)
    assert len({(float(j[0]), float(j[1])) for _, j in frames}) == len(frames)
    want = reference(render, output, max_frames)
    for form, flag in FORMS:
        gpu.set_debug_flags(flag)
        got = run_frames(gpu, upscaler, pkg.layouts, render, output, frames, MaxAccumulatedFrames=max_frames)
        for f, ((gc, gn), (wc, wn, _)) in enumerate(zip(got, want)):
            assert_same(gn, wn.astype(np.float32), (form, "frame", f, "n"))
            assert_same(gc, wc, (form, "frame", f, "Color"))
    reused = np.stack([w[2] for w in want[1:]])
    assert reused.any() and (~reused).any() and not want[0][2].any()      # the sequence reuses its history in some pixels and loses it in others
    lengths = np.stack([w[1] for w in want[1:]])
    assert (lengths <= max_frames).all()
    if max_frames > 1:
        assert (lengths[reused] > 1).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# properties
@pytest.mark.parametrize("render,output", SIZES, ids=IDS)
def test_a_constant_colour_comes_out_equal(gpu, pkg, upscaler, render, output):
    """the hostile depth, motion and jitter of the synthetic sequence with one fp16-representable colour in every texel. Every tap is the
    same t0 = t(c): the clamp box is [t0, t0], the weighted mean sum(w t0) / sum(w) errs by at most 11 roundings, the blend stays between
    the two, and the inverse map multiplies a relative error by 1 + max3(c) = 2.5: under 40 * 2^-24, against half an fp16 ulp of 2^-12
    relative. So Color is c to the bit, at every ratio and jitter, in both forms."""
    c = np.array([0.7333, 1.5, 0.25], np.float16)
    frames = R.synthetic_frames(render, output, seed=77)
    for tex, _ in frames:
        tex["Radiance"][..., :3] = c.view(np.uint16)
    for form, flag in FORMS:
        gpu.set_debug_flags(flag)
        got = run_frames(gpu, upscaler, pkg.layouts, render, output, frames, MaxAccumulatedFrames=8)
        for color, _ in got:
            assert (color[..., :3] == c.view(np.uint16)).all(), form
            assert (color[..., 3] == R.ONE16).all()


def test_native_size_zero_jitter_one_frame_returns_the_inputs_bits(gpu, pkg, upscaler):
    """RenderSize = OutputSize, jitter 0, MaxAccumulatedFrames = 1, KernelRadius 1: the nearest sample sits on the pixel's centre with
    weight 1, its eight neighbours at distance >= 1 weigh 0, n = min(n + 1, 1) = 1 and a = 1: out = t(c), whatever the history, depth
    and motion are. Color = t / (1 - max3(t)) is c up to (3 + 2 (1 + m)) roundings, m <= 16: under 40 * 2^-24 relative, so the RGB bits
    of every finite, non-negative input come back."""
    render = output = (37, 19)
    frames = R.synthetic_frames(render, output, seed=9)
    rng = np.random.default_rng(4)
    for tex, _ in frames:
        c = R.f16(np.exp2(rng.uniform(-6, 4, (19, 37, 3))))
        c[rng.random((19, 37, 3)) < 0.05] = 0
        tex["Radiance"][..., :3] = c
    frames = [(tex, (0.0, 0.0)) for tex, _ in frames]
    for form, flag in FORMS:
        gpu.set_debug_flags(flag)
        got = run_frames(gpu, upscaler, pkg.layouts, render, output, frames, MaxAccumulatedFrames=1)
        for (tex, _), (color, n) in zip(frames, got):
            assert_same(color[..., :3], tex["Radiance"][..., :3], form)
            assert (n == 1.0).all()


def test_history_lengths_follow_the_motion(gpu, pkg, upscaler):
    """20 x 12 -> 40 x 24 at jitter 0: the nearest sample is a quarter of a render pixel off on each axis, k = (1 - 1 / 8)^2 = 0.765625.
    A static sequence adds k per frame up to MaxAccumulatedFrames. With a motion of three render pixels -- six output pixels -- exactly
    the strip without a predecessor (the last six columns) and the rows whose dilated sample fails the depth test have n = k. All depths
    tie, so the dilation takes the first of the 3 x 3 samples, row c - 1: the render rows 4-5 with the previous depth 1 further are seen
    from c = 5 and 6, the output rows 10-13."""
    render, output = SIZES[0]
    L = pkg.layouts
    rng = np.random.default_rng(3)
    colour = lambda: rng.uniform(0.1, 2.0, (render[1], render[0], 3))
    k = np.float32(0.765625)
    static = [(R.plain_frame(render, colour()), (0.0, 0.0)) for _ in range(8)]
    got = run_frames(gpu, upscaler, L, render, output, static, MaxAccumulatedFrames=4)
    for f, (_, n) in enumerate(got):
        assert (n == min(k * (f + 1), 4.0)).all(), f
    moved = R.plain_frame(render, colour(), motion=(3.0, 0.0, 0.0))
    moved["MotionVector"].view(np.float16)[4:6, :, 2] = 1.0
    got = run_frames(gpu, upscaler, L, render, output, [static[0], (moved, (0.0, 0.0))])
    want = np.full((output[1], output[0]), 2 * k, np.float32)
    want[:, output[0] - 6:] = k
    want[10:14] = k
    assert_same(got[1][1], want, "shifted")
    assert (got[0][1] == k).all()


def test_the_output_is_finite_for_every_finite_input(gpu, pkg, upscaler):
    """every finite fp16 pattern as a colour (negative ones, 65504 and subnormals among them), finite depths and motions: Color is finite,
    at most 65504 in magnitude, alpha 1, and equals the restatement; n stays in [1 / 64, MaxAccumulatedFrames]"""
    render, output = SIZES[1]
    rng = np.random.default_rng(21)
    frames = []
    for f in range(3):
        bits = rng.integers(0, 0x10000, (render[1], render[0], 4)).astype(np.uint16)
        bits = np.where((bits & 0x7C00) == 0x7C00, bits & 0x83FF | 0x7800, bits).astype(np.uint16)      # inf / NaN -> the top finite binade
        bits[rng.random(bits.shape) < 0.05] = 0x7BFF
        tex = R.plain_frame(render, 0.0, depth=rng.uniform(0.5, 50.0, (render[1], render[0])),
                            motion=rng.uniform(-4, 4, (render[1], render[0], 3)))
        tex["Radiance"] = bits
        assert np.isfinite(R.f16_to_f32(bits)).all()
        frames.append((tex, R.jitter(f, render, output)))
    ref = R.Upscaler(render, output, np.float32, MaxAccumulatedFrames=8)
    for form, flag in FORMS:
        gpu.set_debug_flags(flag)
        ref.reset()
        got = run_frames(gpu, upscaler, pkg.layouts, render, output, frames, MaxAccumulatedFrames=8)
        for (tex, jitter), (color, n) in zip(frames, got):
            assert_same(color, ref.process(tex, jitter), form)
            v = f64_of(color)
            assert np.isfinite(v).all() and (np.abs(v[..., :3]) <= 65504).all() and (color[..., 3] == R.ONE16).all()
            assert (n >= 1 / 64).all() and (n <= 8).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals and state
def raw_settings(L, render, output, **fields):
    s = np.zeros((), L.UPSCALER_SETTINGS)
    s["RenderSize"], s["OutputSize"] = render, output
    for k, v in dict(L.UPSCALER_DEFAULTS, **fields).items():
        s[k] = v
    return s


def test_refusals_name_the_field_and_touch_nothing(gpu, ptamd, pkg, upscaler):
    L = pkg.layouts
    torch = _torch()
    render, output = (16, 6), (24, 12)
    dev = torch.device("cuda", gpu.device_ordinal)
    frames = R.synthetic_frames(render, output, seed=5, frames=2)
    upscaler.SetConstants(L.upscaler_settings(render, output))
    dtex = upload(frames[0][0], dev)
    bind = dict(dtex, Color=color_target(gpu, output))
    upscaler.Process(frames[0][1], bind)
    gpu.sync()
    length = upscaler.DownloadHistory()
    color = bind["Color"].cpu().numpy().copy()
    assert length.shape == (output[1], output[0]) and 1 / 64 <= length.min() and length.max() <= 1.0

    def untouched(label):
        gpu.sync()
        assert_same(upscaler.DownloadHistory(), length, (label, "history"))
        assert_same(bind["Color"].cpu().numpy(), color, (label, "Color"))
        for n in TEXTURES:
            assert_same(download(dtex[n], frames[0][0][n]), frames[0][0][n], (label, n))

    # out-of-range settings, by name: refused, the previous settings and the history stay
    bad = [("RenderSize", raw_settings(L, (0, 6), output)), ("RenderSize", raw_settings(L, (16385, 6), (16385, 12))),
           ("OutputSize", raw_settings(L, render, (24, 0))), ("OutputSize", raw_settings(L, (8192, 6), (16385, 12))),
           ("OutputSize", raw_settings(L, render, (15, 12))), ("OutputSize", raw_settings(L, render, (24, 25))),
           ("MaxAccumulatedFrames", raw_settings(L, render, output, MaxAccumulatedFrames=0)),
           ("MaxAccumulatedFrames", raw_settings(L, render, output, MaxAccumulatedFrames=256)),
           ("KernelRadius", raw_settings(L, render, output, KernelRadius=0.7)), ("KernelRadius", raw_settings(L, render, output, KernelRadius=2.01)),
           ("KernelRadius", raw_settings(L, render, output, KernelRadius=np.nan)),
           ("DepthThreshold", raw_settings(L, render, output, DepthThreshold=0.0)), ("DepthThreshold", raw_settings(L, render, output, DepthThreshold=1.5)),
           ("DepthThreshold", raw_settings(L, render, output, DepthThreshold=np.nan))]
    for word, s in bad:
        with pytest.raises(ptamd.PtInvalidArgument, match=word):
            upscaler.SetConstants(s)
        with pytest.raises(ValueError, match=word):
            L.check_upscaler_settings(s)
    untouched("settings")
    # every missing binding and each misalignment, by name
    for name in L.UPSCALER_TEXTURES:
        with pytest.raises(ptamd.PtInvalidArgument, match=name):
            upscaler.Process(frames[0][1], {n: t for n, t in bind.items() if n != name})
        raw = bind[name].reshape(-1).view(torch.uint8)
        shifted = torch.zeros(raw.numel() + 2, dtype=torch.uint8, device=dev)[2:]
        shifted.copy_(raw)
        assert shifted.data_ptr() % 4 == 2
        with pytest.raises(ptamd.PtInvalidArgument, match=name + ".*aligned"):
            upscaler.Process(frames[0][1], dict(bind, **{name: shifted}))
        gpu.sync()
        assert shifted.cpu().numpy().tobytes() == raw.cpu().numpy().tobytes(), name
    untouched("bindings")
    for jitter in ((np.nan, 0.0), (0.0, np.inf), (0.51, 0.0), (0.0, -0.75)):
        with pytest.raises(ptamd.PtInvalidArgument, match="jitter"):
            upscaler.Process(jitter, bind)
    untouched("jitter")
    gpu.set_sharding(0, 2, 16)                                      # a sharded context
    try:
        with pytest.raises(ptamd.PtInvalidArgument, match="sharded"):
            upscaler.Process(frames[0][1], bind)
    finally:
        gpu.set_sharding(0, 1, 16)
    untouched("sharded")
    # the history went on through all of it: the second frame is the reference's second frame
    ref = R.Upscaler(render, output, np.float32)
    ref.process(*frames[0])
    want = ref.process(*frames[1])
    d2 = upload(frames[1][0], dev)
    target = color_target(gpu, output)
    upscaler.Process(frames[1][1], dict(d2, Color=target))
    gpu.sync()
    assert_same(target.cpu().numpy().view(np.uint16), want, "frame 2 after the refusals")
    assert_same(upscaler.DownloadHistory(), ref.length, "frame 2 after the refusals")
    assert ref.reused.any()


def test_process_before_set_constants_is_refused(ptamd, pkg):
    """a context of its own: the session's has had its constants set by other tests"""
    torch = _torch()
    ctx = ptamd.DeviceContext(0)
    try:
        render, output = (8, 4), (16, 8)
        tex, jitter = R.synthetic_frames(render, output, seed=1, frames=1)[0]
        dtex = upload(tex, torch.device("cuda", ctx.device_ordinal))
        color = torch.full((8, 16, 4), 0x1234, dtype=torch.int16, device=dtex["Radiance"].device)
        before = {n: t.cpu().numpy().copy() for n, t in dict(dtex, Color=color).items()}
        u = ptamd.Upscaler(ctx)
        with pytest.raises(ptamd.PtInvalidArgument, match="pt_upscaler_set_constants"):
            u.Process(jitter, dict(dtex, Color=color))
        ctx.sync()
        assert u.DownloadHistory().shape == (0, 0)
        for n, t in dict(dtex, Color=color).items():
            assert t.cpu().numpy().tobytes() == before[n].tobytes(), n
    finally:
        ctx.close()


def test_size_change_settings_change_and_reset_restart_the_history(gpu, pkg, upscaler):
    L = pkg.layouts
    dev = _torch().device("cuda", gpu.device_ordinal)
    rng = np.random.default_rng(2)

    def frame(render, output):
        dtex = upload(R.plain_frame(render, rng.uniform(0.1, 2.0, (render[1], render[0], 3))), dev)
        upscaler.Process((0.0, 0.0), dict(dtex, Color=color_target(gpu, output)))
        return upscaler.DownloadHistory()

    a, b = ((24, 10), (24, 10)), ((20, 12), (20, 12))                # native sizes at jitter 0: k = 1, n counts the frames
    upscaler.SetConstants(L.upscaler_settings(*a))
    assert (frame(*a) == 1).all() and (frame(*a) == 2).all()
    upscaler.SetConstants(L.upscaler_settings(*a))                   # the same settings: the history goes on
    assert (frame(*a) == 3).all()
    upscaler.ResetHistory()
    assert upscaler.DownloadHistory().shape == (0, 0)
    assert (frame(*a) == 1).all() and (frame(*a) == 2).all()
    upscaler.SetConstants(L.upscaler_settings(*b))                   # another size (a smaller frame: the allocation stays)
    got = frame(*b)
    assert got.shape == (12, 20) and (got == 1).all() and (frame(*b) == 2).all()
    upscaler.SetConstants(L.upscaler_settings(*b, DepthThreshold=0.02))   # other settings
    assert (frame(*b) == 1).all()
    upscaler.SetConstants(L.upscaler_settings((20, 12), (50, 30)))   # another OutputSize, a larger frame: the history grows
    got = frame((20, 12), (50, 30))
    assert got.shape == (30, 50) and (got <= 1).all()
    again = frame((20, 12), (50, 30))
    assert (again > got).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end: Cornell "ggx", 24 x 16 -> 48 x 32 (the render size of Performance), 1 spp, 3 bounces, static camera, 16 frames with the
# Halton jitter and FrameIndex 0..15. Truth: the unjittered 48 x 32 frame at TRUTH_SPP samples per pixel, whose own Monte-Carlo error is
# 1 / 64 of a 1 spp frame's: negligible beside both errors compared.
RENDER5, OUTPUT5, BOUNCES5, FRAMES5, TRUTH_SPP = (24, 16), (48, 32), 3, 16, 4096


def _settings5(S, L, size, frame, spp, denoiser=None):
    gs = S.graphics_settings(size[0], size[1], spp=spp, bounces=BOUNCES5, frame_index=frame)
    gs["Denoiser"] = L.DENOISER_NONE if denoiser is None else denoiser
    return gs


@pytest.fixture(scope="module")
def cornell(gpu, ptamd, pkg):
    """frame 15 of the sequence through Renderer.render(..., upscale=..., post=...): Upscaled, BackBuffer, the frame's Radiance, n; and
    the truth. Rendered once."""
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    gpu.set_debug_flags(0)
    host = S.cornell_box(aspect=OUTPUT5[0] / OUTPUT5[1], variant="ggx")
    g = ptamd.Scene(gpu, host)
    out = {}
    assert L.upscaler_render_size(L.SUPER_RESOLUTION_PERFORMANCE, OUTPUT5) == RENDER5
    r = ptamd.Renderer(gpu, g, *RENDER5)
    up = r.upscaler(*OUTPUT5)
    up.ResetHistory()
    post = L.post_processing_settings(*OUTPUT5)
    for f in range(FRAMES5):
        g.desc.camera["Jitter"] = ptamd.upscaler_jitter(f, RENDER5, OUTPUT5)
        r.render(_settings5(S, L, RENDER5, f, 1), upscale=up, post=post)
    gpu.sync()
    t = r.textures
    out["upscaled"] = t["Upscaled"].cpu().numpy().view(np.uint16).copy()
    out["backbuffer"] = t["BackBuffer"].cpu().numpy().view(np.uint32).copy()
    out["radiance"] = ptamd.textures_to_numpy(t)["Radiance"].copy()
    out["n"] = up.DownloadHistory()
    g.desc.camera["Jitter"] = (0.0, 0.0)
    r = ptamd.Renderer(gpu, g, *OUTPUT5)
    r.render(_settings5(S, L, OUTPUT5, 0, TRUTH_SPP))
    gpu.sync()
    out["truth"] = ptamd.textures_to_numpy(r.textures)["Radiance"].copy()
    yield out
    g.close()


def test_the_upscaled_frame_is_closer_to_the_truth_than_a_bilinear_upsample(cornell):
    truth = f64_of(cornell["truth"])[..., :3]
    assert cornell["upscaled"].shape == (OUTPUT5[1], OUTPUT5[0], 4) and cornell["radiance"].shape == (RENDER5[1], RENDER5[0], 4)
    upscaled = f64_of(cornell["upscaled"])[..., :3]
    bilinear = R.bilinear_upsample(f64_of(cornell["radiance"])[..., :3], OUTPUT5)
    rms = {k: float(np.sqrt(((v - truth) ** 2).mean())) for k, v in (("upscaled", upscaled), ("bilinear", bilinear))}
    print(f"Cornell {RENDER5} -> {OUTPUT5}, frame {FRAMES5 - 1}: rms error against {TRUTH_SPP} spp: bilinear upsample of the frame's Radiance "
          f"{rms['bilinear']:.5f}, upscaled {rms['upscaled']:.5f} (ratio {rms['upscaled'] / rms['bilinear']:.4f}); n {cornell['n'].min():.3f}..{cornell['n'].max():.3f}")
    assert np.isfinite(rms["upscaled"]) and rms["upscaled"] < rms["bilinear"]
    assert cornell["n"].max() > 8 and cornell["backbuffer"].shape == (OUTPUT5[1], OUTPUT5[0])


def test_cpp_host_runs_the_same_sequence(tmp_path, cornell):
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    out, disp = str(tmp_path / "upscaled.bin"), str(tmp_path / "display.bin")
    cmd = [DEMO, "--upscale", "performance", "--output-size", f"{OUTPUT5[0]}x{OUTPUT5[1]}", "--spp", "1", "--bounces", str(BOUNCES5),
           "--frames", str(FRAMES5), "--post", "--out-upscaled", out, "--out-display", disp]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert_same(np.fromfile(out, np.uint16).reshape(OUTPUT5[1], OUTPUT5[0], 4), cornell["upscaled"], "pt_demo --upscale performance")
    assert_same(np.fromfile(disp, np.uint32).reshape(OUTPUT5[1], OUTPUT5[0]), cornell["backbuffer"], "pt_demo --upscale performance --post")


def test_the_chain_with_the_denoiser_and_post_writes_the_back_buffer_at_output_size(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=OUTPUT5[0] / OUTPUT5[1], variant="ggx"))
    try:
        r = ptamd.Renderer(gpu, g, *RENDER5, with_denoiser_outputs=True)
        r.denoiser.ResetHistory()
        up = r.upscaler(*OUTPUT5)
        up.ResetHistory()
        for f in range(3):
            g.desc.camera["Jitter"] = ptamd.upscaler_jitter(f, RENDER5, OUTPUT5)
            r.render(_settings5(S, L, RENDER5, f, 1, L.DENOISER_NRD_RELAX), nrd=L.DENOISER_NRD_RELAX, denoise=r.denoiser, upscale=up,
                     post=L.post_processing_settings(*OUTPUT5))
        gpu.sync()
        back = r.textures["BackBuffer"].cpu().numpy()
        assert back.shape == (OUTPUT5[1], OUTPUT5[0]) and r.textures["Upscaled"].shape == (OUTPUT5[1], OUTPUT5[0], 4)
        assert len(np.unique(back)) > 16                          # an image, not a cleared buffer
        assert np.isfinite(f64_of(r.textures["Upscaled"].cpu().numpy().view(np.uint16))).all()
        n = up.DownloadHistory()
        assert n.shape == (OUTPUT5[1], OUTPUT5[0]) and n.max() > 1
        # post at another size than OutputSize is refused when upscale is given; without upscale today's check stays
        with pytest.raises(ptamd.PtInvalidArgument, match="OutputSize"):
            r.render(_settings5(S, L, RENDER5, 3, 1), upscale=up, post=L.post_processing_settings(*RENDER5))
        with pytest.raises(ptamd.PtInvalidArgument, match="renderer's size"):
            r.render(_settings5(S, L, RENDER5, 3, 1), post=L.post_processing_settings(*OUTPUT5))
        other = ptamd.Renderer(gpu, g, 20, 12)
        with pytest.raises(ptamd.PtInvalidArgument, match="RenderSize"):
            other.render(_settings5(S, L, (20, 12), 0, 1), upscale=up)
        gpu.set_sharding(0, 2, 16)
        try:
            with pytest.raises(ptamd.PtInvalidArgument, match="sharded"):
                r.upscaler(*OUTPUT5)
        finally:
            gpu.set_sharding(0, 1, 16)
    finally:
        g.close()
