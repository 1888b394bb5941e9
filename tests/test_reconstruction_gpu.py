"""GPU tests of the ray-reconstruction pass (pt_reconstruction_*) against tests/reconstructref.py, the numpy restatement of DESIGN.md
section 1, "Ray reconstruction": the hostile synthetic sequence bit for bit in both forms of the a-trous kernel, the refusals and the
history's life, the pass against the upscaler alone on the Cornell box, the reference's default configuration (radiance cache, ReSTIR,
ray reconstruction, post) end to end, and the C++ host."""
import functools
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import reconstructref as R
import upscaleref as U

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
# 2x; a non-integer ratio that differs per axis and fills no 16 x 16 tile; 3x; native
SIZES = [((20, 12), (40, 24)), ((25, 13), (37, 19)), ((13, 7), (39, 21)), ((37, 19), (37, 19))]
IDS = [f"{r[0]}x{r[1]}-{o[0]}x{o[1]}" for r, o in SIZES]
DEBUG_DIRECT, DEBUG_STAGED = 0x8000, 0x10000
FORMS = [("direct", DEBUG_DIRECT), ("staged", DEBUG_STAGED)]
INPUTS = ("Radiance", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "Position", "LinearDepth", "MotionVector")


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
def reconstruction(gpu, ptamd):
    """the context's pass with no history; the debug flags and the sharding are put back behind the test"""
    gpu.set_sharding(0, 1, 16)
    u = ptamd.Reconstruction(gpu)
    u.ResetHistory()
    yield u
    gpu.set_debug_flags(0)
    gpu.set_sharding(0, 1, 16)
    u.ResetHistory()


def color_target(gpu, output):
    torch = _torch()
    return torch.full((output[1], output[0], 4), 0x1234, dtype=torch.int16, device=torch.device("cuda", gpu.device_ordinal))


def run_frames(gpu, reconstruction, L, render, output, frames, **overrides):
    """the sequence of (textures, jitter) through the device: per frame (Color, length, filtered, n); checks the untouched inputs"""
    dev = _torch().device("cuda", gpu.device_ordinal)
    reconstruction.SetConstants(L.reconstruction_settings(render, output, **overrides))
    reconstruction.ResetHistory()
    out = []
    for host, jitter in frames:
        dtex = upload(host, dev)
        color = color_target(gpu, output)
        reconstruction.Process(jitter, dict(dtex, Color=color))
        gpu.sync()
        for name in INPUTS:
            assert_same(download(dtex[name], host[name]), host[name], ("the call wrote", name))
        out.append((color.cpu().numpy().view(np.uint16),) + reconstruction.DownloadHistory())
    return out


@functools.lru_cache(maxsize=None)
def hostile(render, output):
    return R.synthetic_frames(render, output, seed=render[0] * 131 + output[0])


@functools.lru_cache(maxsize=None)
def reference(render, output, iterations, max_frames):
    """per frame of the synthetic sequence: (Color, length, filtered, n, reused, reused_out, feature) of reconstructref in float32. Computed once."""
    ref = R.Reconstruction(render, output, np.float32, MaxAccumulatedFrames=max_frames, MaxOutputFrames=max_frames, AtrousIterations=iterations)
    out = []
    for tex, jitter in hostile(render, output):
        color = ref.process(tex, jitter)
        out.append((color, ref.length.copy(), ref.filtered.copy(), ref.n.copy(), ref.reused.copy(), ref.reused_out.copy(), ref.feature.copy()))
    return out


@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
@pytest.mark.parametrize("render,output", SIZES, ids=IDS)
def test_synthetic_sequence_bit_for_bit(gpu, pkg, reconstruction, render, output, iterations):
    """three consecutive hostile frames, a different Halton jitter each, both history caps 1 and 8: Color, the filtered fp32 record the
    resolve read and both downloaded lengths of every frame equal reconstructref's bytes, in the direct and in the staged form of the
    a-trous kernel (5 iterations: steps 8 and 16 run past every one of these frames and take the direct form either way)"""
    frames = hostile(render, output)
    for max_frames in (1, 8):
        want = reference(render, output, iterations, max_frames)
        for form, flag in FORMS:
            gpu.set_debug_flags(flag)
            got = run_frames(gpu, reconstruction, pkg.layouts, render, output, frames, MaxAccumulatedFrames=max_frames, MaxOutputFrames=max_frames,
                             AtrousIterations=iterations)
            for f, ((gc, gl, gf, gn), (wc, wl, wf, wn, *_)) in enumerate(zip(got, want)):
                label = (form, "M", max_frames, "frame", f)
                assert_same(gl, wl.astype(np.float32), label + ("length",))
                assert_same(gf, wf.astype(np.float32), label + ("filtered",))
                assert_same(gn, wn.astype(np.float32), label + ("n",))
                assert_same(gc, wc, label + ("Color",))
        reused = np.stack([w[4] for w in want[1:]])
        reused_out = np.stack([w[5] for w in want[1:]])
        assert reused.any() and (~reused).any() and reused_out.any() and (~reused_out).any() and not want[0][4].any() and not want[0][5].any()
        lengths = np.stack([w[1] for w in want])
        assert (lengths <= max_frames).all() and (lengths == 0).any()
        if max_frames > 1:
            assert (lengths[1:][reused] > 1).any()
            assert any(w[6].any() for w in want[1:])                # the luminance reset dropped a history somewhere
        assert all(np.isfinite(w[2]).all() and np.isfinite(f64_of(w[0])).all() for w in want)


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals and state
def raw_settings(L, render, output, **fields):
    s = np.zeros((), L.RECONSTRUCTION_SETTINGS)
    s["RenderSize"], s["OutputSize"] = render, output
    for k, v in dict(L.RECONSTRUCTION_DEFAULTS, **fields).items():
        s[k] = v
    return s


def test_refusals_name_the_field_and_touch_nothing(gpu, ptamd, pkg, reconstruction):
    L = pkg.layouts
    torch = _torch()
    render, output = (16, 6), (24, 12)
    dev = torch.device("cuda", gpu.device_ordinal)
    frames = R.synthetic_frames(render, output, seed=5, frames=2)
    reconstruction.SetConstants(L.reconstruction_settings(render, output))
    dtex = upload(frames[0][0], dev)
    bind = dict(dtex, Color=color_target(gpu, output))
    reconstruction.Process(frames[0][1], bind)
    gpu.sync()
    history = reconstruction.DownloadHistory()
    color = bind["Color"].cpu().numpy().copy()
    assert history[0].shape == (render[1], render[0]) and history[1].shape == (render[1], render[0], 4) and history[2].shape == (output[1], output[0])
    assert history[0].max() == 1.0 and history[0].min() == 0.0 and 1 / 64 <= history[2].min() and history[2].max() <= 1.0

    def untouched(label):
        gpu.sync()
        for got, want, what in zip(reconstruction.DownloadHistory(), history, ("length", "filtered", "n")):
            assert_same(got, want, (label, what))
        assert_same(bind["Color"].cpu().numpy(), color, (label, "Color"))
        for n in INPUTS:
            assert_same(download(dtex[n], frames[0][0][n]), frames[0][0][n], (label, n))

    # out-of-range settings, by name: refused, the previous settings and the history stay
    bad = [("RenderSize", raw_settings(L, (0, 6), output)), ("RenderSize", raw_settings(L, (16385, 6), (16385, 12))),
           ("OutputSize", raw_settings(L, render, (24, 0))), ("OutputSize", raw_settings(L, (8192, 6), (16385, 12))),
           ("OutputSize", raw_settings(L, render, (15, 12))), ("OutputSize", raw_settings(L, render, (24, 25))),
           ("MaxAccumulatedFrames", raw_settings(L, render, output, MaxAccumulatedFrames=0)),
           ("MaxAccumulatedFrames", raw_settings(L, render, output, MaxAccumulatedFrames=256)),
           ("MaxOutputFrames", raw_settings(L, render, output, MaxOutputFrames=0)), ("MaxOutputFrames", raw_settings(L, render, output, MaxOutputFrames=256)),
           ("AtrousIterations", raw_settings(L, render, output, AtrousIterations=9)),
           ("KernelRadius", raw_settings(L, render, output, KernelRadius=0.7)), ("KernelRadius", raw_settings(L, render, output, KernelRadius=np.nan)),
           ("DepthThreshold", raw_settings(L, render, output, DepthThreshold=0.0)), ("DepthThreshold", raw_settings(L, render, output, DepthThreshold=np.nan)),
           ("NormalCosine", raw_settings(L, render, output, NormalCosine=1.0)), ("NormalCosine", raw_settings(L, render, output, NormalCosine=np.nan)),
           ("LuminanceSigma", raw_settings(L, render, output, LuminanceSigma=0.0)), ("LuminanceSigma", raw_settings(L, render, output, LuminanceSigma=np.inf)),
           ("RoughnessFraction", raw_settings(L, render, output, RoughnessFraction=0.0)),
           ("RoughnessFraction", raw_settings(L, render, output, RoughnessFraction=np.nan))]
    for word, s in bad:
        with pytest.raises(ptamd.PtInvalidArgument, match=word):
            reconstruction.SetConstants(s)
        with pytest.raises(ValueError, match=word):
            L.check_reconstruction_settings(s)
    untouched("settings")
    # every missing binding and each misalignment, by name
    for name in L.RECONSTRUCTION_TEXTURES:
        with pytest.raises(ptamd.PtInvalidArgument, match=name):
            reconstruction.Process(frames[0][1], {n: t for n, t in bind.items() if n != name})
        raw = bind[name].reshape(-1).view(torch.uint8)
        shifted = torch.zeros(raw.numel() + 2, dtype=torch.uint8, device=dev)[2:]
        shifted.copy_(raw)
        assert shifted.data_ptr() % 4 == 2
        with pytest.raises(ptamd.PtInvalidArgument, match=name + ".*aligned"):
            reconstruction.Process(frames[0][1], dict(bind, **{name: shifted}))
        gpu.sync()
        assert shifted.cpu().numpy().tobytes() == raw.cpu().numpy().tobytes(), name
    untouched("bindings")
    # Color over an input: the whole of it, and one that only reaches into its last texel
    room = torch.zeros(render[0] * render[1] * 4 + output[0] * output[1] * 4, dtype=torch.int16, device=dev)
    for name in ("Radiance", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "MotionVector"):
        flat = room[:render[0] * render[1] * 4]
        flat.copy_(bind[name].reshape(-1))
        for start in (0, render[0] * render[1] * 4 - 4):
            with pytest.raises(ptamd.PtInvalidArgument, match="Color overlaps " + name):
                reconstruction.Process(frames[0][1], dict(bind, **{name: flat, "Color": room[start:start + output[0] * output[1] * 4]}))
    big = torch.zeros(max(output[0] * output[1] * 2, render[0] * render[1] * 4), dtype=torch.float32, device=dev)      # room for Color and for Position
    with pytest.raises(ptamd.PtInvalidArgument, match="Color overlaps Position"):
        reconstruction.Process(frames[0][1], dict(bind, Position=big[:render[0] * render[1] * 4], Color=big.view(torch.int16)))
    with pytest.raises(ptamd.PtInvalidArgument, match="Color overlaps LinearDepth"):
        reconstruction.Process(frames[0][1], dict(bind, LinearDepth=big[output[0] * output[1] * 2 - render[0] * render[1]:], Color=big.view(torch.int16)))
    untouched("overlap")
    for jitter in ((np.nan, 0.0), (0.0, np.inf), (0.51, 0.0), (0.0, -0.75)):
        with pytest.raises(ptamd.PtInvalidArgument, match="jitter"):
            reconstruction.Process(jitter, bind)
    untouched("jitter")
    gpu.set_sharding(0, 2, 16)                                      # a sharded context
    try:
        with pytest.raises(ptamd.PtInvalidArgument, match="sharded"):
            reconstruction.Process(frames[0][1], bind)
    finally:
        gpu.set_sharding(0, 1, 16)
    untouched("sharded")
    # the history went on through all of it: the second frame is the reference's second frame
    ref = R.Reconstruction(render, output, np.float32)
    ref.process(*frames[0])
    want = ref.process(*frames[1])
    d2 = upload(frames[1][0], dev)
    target = color_target(gpu, output)
    reconstruction.Process(frames[1][1], dict(d2, Color=target))
    gpu.sync()
    assert_same(target.cpu().numpy().view(np.uint16), want, "frame 2 after the refusals")
    length, filtered, n = reconstruction.DownloadHistory()
    assert_same(length, ref.length, "frame 2 after the refusals")
    assert_same(filtered, ref.filtered, "frame 2 after the refusals")
    assert_same(n, ref.n, "frame 2 after the refusals")
    assert ref.reused.any() and ref.reused_out.any()


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
        u = ptamd.Reconstruction(ctx)
        with pytest.raises(ptamd.PtInvalidArgument, match="pt_reconstruction_set_constants"):
            u.Process(jitter, dict(dtex, Color=color))
        ctx.sync()
        assert [a.shape for a in u.DownloadHistory()] == [(0, 0), (0, 0, 4), (0, 0)]
        for n, t in dict(dtex, Color=color).items():
            assert t.cpu().numpy().tobytes() == before[n].tobytes(), n
    finally:
        ctx.close()


def test_size_change_settings_change_and_reset_restart_the_history(gpu, ptamd, pkg, reconstruction):
    """native sizes at jitter 0 (k = 1) on static plain frames: both lengths count the frames. The upscaler of the same context keeps a
    history of its own through all of it."""
    L = pkg.layouts
    dev = _torch().device("cuda", gpu.device_ordinal)
    rng = np.random.default_rng(2)

    def frame(render, output):
        dtex = upload(R.plain_frame(render, rng.uniform(0.1, 2.0, (render[1], render[0], 3))), dev)
        reconstruction.Process((0.0, 0.0), dict(dtex, Color=color_target(gpu, output)))
        length, _, n = reconstruction.DownloadHistory()
        return length, n

    def both(render, output, count):
        length, n = frame(render, output)
        return length.shape == (render[1], render[0]) and n.shape == (output[1], output[0]) and (length == count).all() and (n == count).all()

    a, b = ((24, 10), (24, 10)), ((20, 12), (20, 12))
    up = ptamd.Upscaler(gpu)
    up.SetConstants(L.upscaler_settings(*a))
    up.ResetHistory()
    utex = upload(U.plain_frame(a[0], 0.5), dev)
    up.Process((0.0, 0.0), dict(utex, Color=color_target(gpu, a[1])))
    reconstruction.SetConstants(L.reconstruction_settings(*a))
    assert both(*a, 1) and both(*a, 2)
    reconstruction.SetConstants(L.reconstruction_settings(*a))       # the same settings: the history goes on
    assert both(*a, 3)
    reconstruction.ResetHistory()
    assert [h.size for h in reconstruction.DownloadHistory()] == [0, 0, 0]
    assert both(*a, 1) and both(*a, 2)
    reconstruction.SetConstants(L.reconstruction_settings(*b))       # another size (a smaller frame: the allocation stays)
    assert both(*b, 1) and both(*b, 2)
    reconstruction.SetConstants(L.reconstruction_settings(*b, LuminanceSigma=3.0))   # other settings
    assert both(*b, 1)
    reconstruction.SetConstants(L.reconstruction_settings(*b, MaxAccumulatedFrames=2, MaxOutputFrames=3))
    assert both(*b, 1)
    length, n = frame(*b)
    assert (length == 2).all() and (n == 2).all()
    length, n = frame(*b)
    assert (length == 2).all() and (n == 3).all()                    # each history has its own cap
    reconstruction.SetConstants(L.reconstruction_settings((20, 12), (50, 30)))   # another OutputSize, a larger frame: the history grows
    length, n = frame((20, 12), (50, 30))
    assert n.shape == (30, 50) and (n <= 1).all() and (length == 1).all()
    length, again = frame((20, 12), (50, 30))
    assert (again > n).all() and (length == 2).all()
    up.Process((0.0, 0.0), dict(utex, Color=color_target(gpu, a[1])))              # the upscaler's own history went on meanwhile
    assert (up.DownloadHistory() == 2).all()
    up.ResetHistory()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end: Cornell "ggx", 24 x 16 -> 48 x 32 (the render size of Performance), 1 spp, 3 bounces, Denoiser = DLSS-RR, static camera, 16
# frames with the Halton jitter and FrameIndex 0..15. Truth: the unjittered 48 x 32 Denoiser = None frame at TRUTH_SPP samples per pixel.
RENDER5, OUTPUT5, BOUNCES5, FRAMES5, TRUTH_SPP = (24, 16), (48, 32), 3, 16, 4096


def _settings5(S, L, size, frame, spp, denoiser, **fields):
    gs = S.graphics_settings(size[0], size[1], spp=spp, bounces=BOUNCES5, frame_index=frame)
    gs["Denoiser"] = denoiser
    for k, v in fields.items():
        gs[k] = v
    return gs


@pytest.fixture(scope="module")
def cornell(gpu, ptamd, pkg):
    """frame 15 of the sequence through Renderer.render(..., reconstruct=..., post=...): Reconstructed, BackBuffer, the lengths; the same
    frames' Radiance through the upscaler alone; and the truth. Rendered once."""
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    gpu.set_debug_flags(0)
    host = S.cornell_box(aspect=OUTPUT5[0] / OUTPUT5[1], variant="ggx")
    g = ptamd.Scene(gpu, host)
    out = {}
    r = ptamd.Renderer(gpu, g, *RENDER5)
    rr = r.reconstruction(*OUTPUT5)
    rr.ResetHistory()
    up = r.upscaler(*OUTPUT5)
    up.ResetHistory()
    alone = color_target(gpu, OUTPUT5)
    post = L.post_processing_settings(*OUTPUT5)
    for f in range(FRAMES5):
        g.desc.camera["Jitter"] = ptamd.upscaler_jitter(f, RENDER5, OUTPUT5)
        r.render(_settings5(S, L, RENDER5, f, 1, L.DENOISER_DLSS_RR), reconstruct=rr, post=post)
        t = r.textures
        up.Process(g.desc.camera["Jitter"], {"Radiance": t["Radiance"], "LinearDepth": t["LinearDepth"], "MotionVector": t["MotionVector"], "Color": alone})
    gpu.sync()
    t = r.textures
    out["reconstructed"] = t["Reconstructed"].cpu().numpy().view(np.uint16).copy()
    out["backbuffer"] = t["BackBuffer"].cpu().numpy().view(np.uint32).copy()
    out["alone"] = alone.cpu().numpy().view(np.uint16).copy()
    out["length"], _, out["n"] = rr.DownloadHistory()
    g.desc.camera["Jitter"] = (0.0, 0.0)
    r = ptamd.Renderer(gpu, g, *OUTPUT5)
    r.render(_settings5(S, L, OUTPUT5, 0, TRUTH_SPP, L.DENOISER_NONE))
    gpu.sync()
    out["truth"] = ptamd.textures_to_numpy(r.textures)["Radiance"].copy()
    yield out
    rr.ResetHistory()
    up.ResetHistory()
    g.close()


def test_the_reconstructed_frame_beats_the_upscaler_alone(cornell):
    """The inequality only; the figures measured on an MI355X are recorded in DESIGN.md section 1, "Ray reconstruction": 0.786 through the
    upscaler alone, 0.750 reconstructed. With stage 1 as the denoiser has it (the depth test alone, no luminance reset) it was 0.798:
    DESIGN.md section 7 has the account."""
    truth = f64_of(cornell["truth"])[..., :3]
    assert cornell["reconstructed"].shape == (OUTPUT5[1], OUTPUT5[0], 4) and cornell["alone"].shape == (OUTPUT5[1], OUTPUT5[0], 4)
    rms = {k: float(np.sqrt(((f64_of(cornell[k])[..., :3] - truth) ** 2).mean())) for k in ("reconstructed", "alone")}
    print(f"Cornell {RENDER5} -> {OUTPUT5}, frame {FRAMES5 - 1}: rms error against {TRUTH_SPP} spp: the upscaler alone {rms['alone']:.5f}, "
          f"reconstructed {rms['reconstructed']:.5f} (ratio {rms['reconstructed'] / rms['alone']:.4f}); length {cornell['length'].min():.0f}.."
          f"{cornell['length'].max():.0f}, n {cornell['n'].min():.3f}..{cornell['n'].max():.3f}")
    assert np.isfinite(rms["reconstructed"]) and rms["reconstructed"] < rms["alone"]
    assert cornell["length"].max() == FRAMES5 and cornell["n"].max() > 4 and cornell["backbuffer"].shape == (OUTPUT5[1], OUTPUT5[0])


def test_cpp_host_runs_the_same_sequence(tmp_path, cornell):
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    out, disp = str(tmp_path / "reconstructed.bin"), str(tmp_path / "display.bin")
    cmd = [DEMO, "--reconstruct", "performance", "--output-size", f"{OUTPUT5[0]}x{OUTPUT5[1]}", "--spp", "1", "--bounces", str(BOUNCES5),
           "--frames", str(FRAMES5), "--post", "--out-reconstructed", out, "--out-display", disp]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert_same(np.fromfile(out, np.uint16).reshape(OUTPUT5[1], OUTPUT5[0], 4), cornell["reconstructed"], "pt_demo --reconstruct performance")
    assert_same(np.fromfile(disp, np.uint32).reshape(OUTPUT5[1], OUTPUT5[0]), cornell["backbuffer"], "pt_demo --reconstruct performance --post")
    for extra, word in ((["--nrd", "relax"], "--nrd"), (["--upscale", "performance"], "--upscale")):
        p = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and word in p.stderr, (extra, p.returncode, p.stderr)


def _default_configuration(ptamd, pkg, frames=4):
    """the reference's default settings on a context of its own: radiance cache, ReSTIR DI (8 candidates, the default reuse), ray
    reconstruction, post. Per frame (Reconstructed, BackBuffer, Radiance)."""
    S, L = pkg.scenes, pkg.layouts
    ctx = ptamd.DeviceContext(0)
    try:
        g = ptamd.Scene(ctx, S.cornell_box(aspect=OUTPUT5[0] / OUTPUT5[1], variant="ggx"))
        r = ptamd.Renderer(ctx, g, *RENDER5, with_denoiser_outputs=True, di_history=True)
        r.sharc.Configure(1 << 16)
        rr = r.reconstruction(*OUTPUT5)
        out = []
        for f in range(frames):
            g.desc.camera["Jitter"] = ptamd.upscaler_jitter(f, RENDER5, OUTPUT5)
            r.render(_settings5(S, L, RENDER5, f, 1, L.DENOISER_DLSS_RR, IsDIEnabled=1), di_samples=8, di_reuse=L.di_resampling_settings(),
                     sharc=L.sharc_settings(), reconstruct=rr, post=L.post_processing_settings(*OUTPUT5))
            ctx.sync()
            t = r.textures
            out.append(tuple(t[n].cpu().numpy().copy() for n in ("Reconstructed", "BackBuffer", "Radiance")))
        length, _, n = rr.DownloadHistory()
        assert length.max() == frames and n.max() > 1
        return out
    finally:
        ctx.close()


def test_the_default_configuration_end_to_end(ptamd, pkg):
    first = _default_configuration(ptamd, pkg)
    for reconstructed, back, radiance in first:
        rec = f64_of(reconstructed.view(np.uint16))
        assert rec.shape == (OUTPUT5[1], OUTPUT5[0], 4) and back.shape == (OUTPUT5[1], OUTPUT5[0])
        assert np.isfinite(rec).all() and np.isfinite(f64_of(radiance.view(np.uint16))).all()
        assert (reconstructed.view(np.uint16)[..., 3] == R.ONE16).all() and len(np.unique(back)) > 16
        bilinear = U.bilinear_upsample(f64_of(radiance.view(np.uint16))[..., :3], OUTPUT5)
        assert np.abs(rec[..., :3] - bilinear).max() > 1e-2 and rec[..., :3].max() > 0.1
    second = _default_configuration(ptamd, pkg)
    for f, (a, b) in enumerate(zip(first, second)):
        for x, y, name in zip(a, b, ("Reconstructed", "BackBuffer", "Radiance")):
            assert x.tobytes() == y.tobytes(), (f, name)


def test_render_refuses_what_the_pass_cannot_serve(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=OUTPUT5[0] / OUTPUT5[1], variant="ggx"))
    try:
        r = ptamd.Renderer(gpu, g, *RENDER5, with_denoiser_outputs=True)
        rr = r.reconstruction(*OUTPUT5, AtrousIterations=2)
        assert int(rr.settings["AtrousIterations"]) == 2
        rr.ResetHistory()
        gs = _settings5(S, L, RENDER5, 0, 1, L.DENOISER_DLSS_RR)
        r.render(gs, reconstruct=rr)
        gpu.sync()
        before = r.textures["Reconstructed"].cpu().numpy().copy()
        history = rr.DownloadHistory()
        up = r.upscaler(*OUTPUT5)
        with pytest.raises(ptamd.PtInvalidArgument, match="upscale"):
            r.render(gs, reconstruct=rr, upscale=up)
        with pytest.raises(ptamd.PtInvalidArgument, match="nrd"):
            r.render(_settings5(S, L, RENDER5, 0, 1, L.DENOISER_NRD_RELAX), reconstruct=rr, nrd=L.DENOISER_NRD_RELAX)
        for other in (L.DENOISER_NONE, L.DENOISER_NRD_RELAX, L.DENOISER_NRD_REBLUR):
            with pytest.raises(ptamd.PtInvalidArgument, match="DENOISER_DLSS_RR"):
                r.render(_settings5(S, L, RENDER5, 0, 1, other), reconstruct=rr)
        with pytest.raises(ptamd.PtInvalidArgument, match="OutputSize"):
            r.render(gs, reconstruct=rr, post=L.post_processing_settings(*RENDER5))
        with pytest.raises(ptamd.PtInvalidArgument, match="Reconstruction"):
            r.render(gs, reconstruct=up)
        other = ptamd.Renderer(gpu, g, 20, 12)
        with pytest.raises(ptamd.PtInvalidArgument, match="RenderSize"):
            other.render(_settings5(S, L, (20, 12), 0, 1, L.DENOISER_DLSS_RR), reconstruct=rr)
        bare = ptamd.Renderer(gpu, g, *RENDER5)
        del bare.textures["DiffuseAlbedo"]
        with pytest.raises(ptamd.PtInvalidArgument, match="DiffuseAlbedo"):
            bare.render(gs, reconstruct=rr)
        gpu.set_sharding(0, 2, 16)
        try:
            with pytest.raises(ptamd.PtInvalidArgument, match="sharded"):
                r.reconstruction(*OUTPUT5)
            with pytest.raises(ptamd.PtInvalidArgument, match="sharded"):
                r.render(gs, reconstruct=rr)
        finally:
            gpu.set_sharding(0, 1, 16)
        gpu.sync()
        assert r.textures["Reconstructed"].cpu().numpy().tobytes() == before.tobytes()
        for got, want in zip(rr.DownloadHistory(), history):
            assert got.tobytes() == want.tobytes()
        rr.ResetHistory()
    finally:
        g.close()
