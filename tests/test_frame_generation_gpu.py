"""GPU tests of the frame interpolator (pt_frame_generation_*) against tests/framegenref.py, the numpy restatement of DESIGN.md section 1,
"Frame generation": the hostile synthetic sequence bit for bit, the call without a previous frame, the refusals, and the chain G-buffer ->
path tracer -> upscaler -> post -> frame generation end to end with a camera that moves."""
import functools
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import framegenref as R

pytestmark = pytest.mark.gpu

# 2x; a non-integer ratio that differs per axis and fills no 16 x 16 tile; 3x; native
SIZES = [((20, 12), (40, 24)), ((25, 13), (37, 19)), ((13, 7), (39, 21)), ((37, 19), (37, 19))]
IDS = [f"{r[0]}x{r[1]}-{o[0]}x{o[1]}" for r, o in SIZES]
INPUTS = ("Color", "LinearDepth", "MotionVector")
DEMO = os.path.join(ge.PKG_DIR, "pt_demo")


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


@pytest.fixture
def framegen(gpu, ptamd):
    """the context's frame generation with no previous frame; the sharding is put back behind the test"""
    gpu.set_sharding(0, 1, 16)
    g = ptamd.FrameGeneration(gpu)
    g.ResetHistory()
    yield g
    gpu.set_sharding(0, 1, 16)
    g.ResetHistory()


def targets(gpu, output):
    torch = _torch()
    dev = torch.device("cuda", gpu.device_ordinal)
    return {"Generated": torch.full((output[1], output[0], 4), 0x1234, dtype=torch.int16, device=dev),
            "Generated8": torch.full((output[1], output[0]), 0x5678, dtype=torch.int32, device=dev)}


def outputs(bind):
    return bind["Generated"].cpu().numpy().view(np.uint16).copy(), bind["Generated8"].cpu().numpy().view(np.uint32).copy()


def run_frames(gpu, framegen, L, render, output, frames, **overrides):
    """the sequence of (textures, jitter) through the device: per frame (Generated, Generated8, generated?, field, classes); checks the
    untouched inputs"""
    dev = _torch().device("cuda", gpu.device_ordinal)
    framegen.SetConstants(L.frame_generation_settings(render, output, **overrides))
    framegen.ResetHistory()
    out = []
    for host, jitter in frames:
        dtex = upload(host, dev)
        bind = dict(dtex, **targets(gpu, output))
        did = framegen.Process(jitter, bind)
        gpu.sync()
        for name in INPUTS:
            assert_same(download(dtex[name], host[name]), host[name], ("the call wrote", name))
        out.append(outputs(bind) + (did,) + framegen.DownloadField())
        for t in dtex.values():                                # the caller may overwrite its textures between calls
            t.zero_()
    return out


@functools.lru_cache(maxsize=None)
def reference(render, output, phi):
    """per frame of the synthetic sequence: (Generated, Generated8, generated?, field, classes) of framegenref. Computed once."""
    ref = R.FrameGeneration(render, output, Phase=phi)
    out = []
    for tex, jitter in R.synthetic_frames(render, output, seed=render[0] * 131 + output[0]):
        g, g8, did = ref.process(tex, jitter)
        out.append((g, g8, did, ref.field, ref.classes, ref.candidates))
    return out


@pytest.mark.parametrize("phi", [0.5, 0.25])
@pytest.mark.parametrize("render,output", SIZES, ids=IDS)
def test_synthetic_sequence_bit_for_bit(gpu, pkg, framegen, render, output, phi):
    """three consecutive hostile frames, a different Halton jitter each: Generated, Generated8, the midpoint field and the class bytes of
    every frame equal framegenref's bytes. (There is one form of the resolve: no staged one was built.)"""
    frames = R.synthetic_frames(render, output, seed=render[0] * 131 + output[0])
    assert all((~np.isfinite(t["LinearDepth"])).sum() >= render[0] * render[1] // 12 for t, _ in frames)
    assert len({(float(j[0]), float(j[1])) for _, j in frames}) == len(frames)
    want = reference(render, output, phi)
    got = run_frames(gpu, framegen, pkg.layouts, render, output, frames, Phase=phi)
    for f, ((gg, g8, did, field, classes), (wg, w8, wdid, wfield, wclasses, _)) in enumerate(zip(got, want)):
        assert did == wdid == (f > 0), f
        if did:
            assert_same(field, wfield, ("frame", f, "field"))
            assert_same(classes, wclasses, ("frame", f, "classes"))
        else:
            assert field.shape == (0, 0) and classes.shape == (0, 0)
        assert_same(gg, wg, ("frame", f, "Generated"))
        assert_same(g8, w8, ("frame", f, "Generated8"))
    seen = set(np.unique(np.concatenate([w[4].ravel() for w in want[1:]])).tolist())
    assert len(seen) >= 3                                      # the sequence warps, loses one side and falls back
    assert max(w[5].max() for w in want[1:]) >= 3              # cells with several candidates: the atomic minimum decides


def test_first_call_reset_and_settings_change_copy_color(gpu, pkg, framegen):
    """no previous frame: out_generated = 0 and Generated is Color bit for bit (Generated8 its four channels); the same after
    ResetHistory and after a change of settings; the same settings again keep the previous frame"""
    L = pkg.layouts
    render, output = SIZES[1]
    frames = R.synthetic_frames(render, output, seed=11, frames=2)
    dev = _torch().device("cuda", gpu.device_ordinal)

    def call(k, generated8=True):
        bind = dict(upload(frames[k][0], dev), **targets(gpu, output))
        if not generated8:
            bind["Generated8"] = None
        did = framegen.Process(frames[k][1], bind)
        gpu.sync()
        g = bind["Generated"].cpu().numpy().view(np.uint16).copy()
        return did, g, (bind["Generated8"].cpu().numpy().view(np.uint32).copy() if generated8 else None)

    def is_copy(result, k):
        did, g, g8 = result
        assert not did
        assert_same(g, frames[k][0]["Color"], "Generated is Color")
        assert_same(g8, R.pack8(frames[k][0]["Color"]), "Generated8")
        f, c = framegen.DownloadField()
        assert f.shape == (0, 0) and c.shape == (0, 0)

    framegen.SetConstants(L.frame_generation_settings(render, output))
    is_copy(call(0), 0)
    ref = R.FrameGeneration(render, output)
    ref.process(*frames[0])
    want = ref.process(*frames[1])
    did, g, g8 = call(1)
    assert did
    assert_same(g, want[0], "second call")
    framegen.SetConstants(L.frame_generation_settings(render, output))           # the same settings: the previous frame stays
    did, g, _ = call(1, generated8=False)                                        # Generated8 is optional
    assert did and framegen.DownloadField()[0].shape == (render[1], render[0])
    framegen.ResetHistory()
    is_copy(call(1), 1)
    assert call(0)[0]
    framegen.SetConstants(L.frame_generation_settings(render, output, Phase=0.25))   # other settings
    is_copy(call(0), 0)
    assert call(1)[0]
    framegen.SetConstants(L.frame_generation_settings(render, (50, 26)))         # another size, a larger output: the buffers grow
    big = R.synthetic_frames(render, (50, 26), seed=12, frames=2)
    bind = dict(upload(big[0][0], dev), **targets(gpu, (50, 26)))
    assert not framegen.Process(big[0][1], bind)
    gpu.sync()
    assert_same(bind["Generated"].cpu().numpy().view(np.uint16), big[0][0]["Color"], "after the size change")
    bind = dict(upload(big[1][0], dev), **targets(gpu, (50, 26)))
    assert framegen.Process(big[1][1], bind)
    ref = R.FrameGeneration(render, (50, 26))
    ref.process(*big[0])
    gpu.sync()
    assert_same(bind["Generated"].cpu().numpy().view(np.uint16), ref.process(*big[1])[0], "the frame after the size change")


def raw_settings(L, render, output, **fields):
    s = np.zeros((), L.FRAME_GENERATION_SETTINGS)
    s["RenderSize"], s["OutputSize"] = render, output
    for k, v in dict(L.FRAME_GENERATION_DEFAULTS, **fields).items():
        s[k] = v
    return s


def test_refusals_name_the_field_and_touch_nothing(gpu, ptamd, pkg, framegen):
    L = pkg.layouts
    torch = _torch()
    render, output = (16, 6), (24, 12)
    dev = torch.device("cuda", gpu.device_ordinal)
    frames = R.synthetic_frames(render, output, seed=5, frames=3)
    framegen.SetConstants(L.frame_generation_settings(render, output))
    ref = R.FrameGeneration(render, output)
    for k in (0, 1):
        dtex = upload(frames[k][0], dev)
        bind = dict(dtex, **targets(gpu, output))
        framegen.Process(frames[k][1], bind)
        ref.process(*frames[k])
    gpu.sync()
    field, classes = framegen.DownloadField()
    generated, generated8 = outputs(bind)
    assert field.shape == (render[1], render[0]) and classes.shape == (output[1], output[0])

    def untouched(label):
        gpu.sync()
        f, c = framegen.DownloadField()
        assert_same(f, field, (label, "field"))
        assert_same(c, classes, (label, "classes"))
        g, g8 = outputs(bind)
        assert_same(g, generated, (label, "Generated"))
        assert_same(g8, generated8, (label, "Generated8"))
        for n in INPUTS:
            assert_same(download(dtex[n], frames[1][0][n]), frames[1][0][n], (label, n))

    bad = [("RenderSize", raw_settings(L, (0, 6), output)), ("RenderSize", raw_settings(L, (16385, 6), (16385, 12))),
           ("OutputSize", raw_settings(L, render, (24, 0))), ("OutputSize", raw_settings(L, (8192, 6), (16385, 12))),
           ("OutputSize", raw_settings(L, render, (15, 12))), ("OutputSize", raw_settings(L, render, (24, 25))),
           ("Phase", raw_settings(L, render, output, Phase=0.0)), ("Phase", raw_settings(L, render, output, Phase=1.0)),
           ("Phase", raw_settings(L, render, output, Phase=np.nan)),
           ("DepthThreshold", raw_settings(L, render, output, DepthThreshold=0.0)), ("DepthThreshold", raw_settings(L, render, output, DepthThreshold=1.5)),
           ("DepthThreshold", raw_settings(L, render, output, DepthThreshold=np.nan))]
    for word, s in bad:
        with pytest.raises(ptamd.PtInvalidArgument, match=word):
            framegen.SetConstants(s)
        with pytest.raises(ValueError, match=word):
            L.check_frame_generation_settings(s)
    untouched("settings")
    for name in L.FRAME_GENERATION_TEXTURES:                   # every missing required binding and each misalignment, by name
        if name != "Generated8":
            with pytest.raises(ptamd.PtInvalidArgument, match=name + " is NULL"):
                framegen.Process(frames[2][1], {n: t for n, t in bind.items() if n != name})
        raw = bind[name].reshape(-1).view(torch.uint8)
        shifted = torch.zeros(raw.numel() + 2, dtype=torch.uint8, device=dev)[2:]
        shifted.copy_(raw)
        assert shifted.data_ptr() % 4 == 2
        with pytest.raises(ptamd.PtInvalidArgument, match=name + " is not aligned"):
            framegen.Process(frames[2][1], dict(bind, **{name: shifted}))
        gpu.sync()
        assert shifted.cpu().numpy().tobytes() == raw.cpu().numpy().tobytes(), name
    untouched("bindings")
    for name in INPUTS:                                        # an output over an input
        with pytest.raises(ptamd.PtInvalidArgument, match="overlaps " + name):
            framegen.Process(frames[2][1], dict(bind, Generated=bind[name]))
    with pytest.raises(ptamd.PtInvalidArgument, match="Generated8 overlaps Generated"):
        framegen.Process(frames[2][1], dict(bind, Generated8=bind["Generated"]))
    untouched("overlap")
    for jitter in ((np.nan, 0.0), (0.0, np.inf), (0.51, 0.0), (0.0, -0.75)):
        with pytest.raises(ptamd.PtInvalidArgument, match="jitter"):
            framegen.Process(jitter, bind)
    untouched("jitter")
    gpu.set_sharding(0, 2, 16)                                 # a sharded context
    try:
        with pytest.raises(ptamd.PtInvalidArgument, match="sharded"):
            framegen.Process(frames[2][1], bind)
    finally:
        gpu.set_sharding(0, 1, 16)
    untouched("sharded")
    # the previous frame went through all of it: the third frame is the reference's third frame
    want = ref.process(*frames[2])
    d2 = upload(frames[2][0], dev)
    b2 = dict(d2, **targets(gpu, output))
    assert framegen.Process(frames[2][1], b2)
    gpu.sync()
    g, g8 = outputs(b2)
    assert_same(g, want[0], "frame 3 after the refusals")
    assert_same(g8, want[1], "frame 3 after the refusals")
    assert_same(framegen.DownloadField()[1], ref.classes, "frame 3 after the refusals")


def test_process_before_set_constants_is_refused(ptamd, pkg):
    """a context of its own: the session's has had its constants set by other tests"""
    torch = _torch()
    ctx = ptamd.DeviceContext(0)
    try:
        render, output = (8, 4), (16, 8)
        tex, jitter = R.synthetic_frames(render, output, seed=1, frames=1)[0]
        dtex = upload(tex, torch.device("cuda", ctx.device_ordinal))
        bind = dict(dtex, Generated=torch.full((8, 16, 4), 0x1234, dtype=torch.int16, device=dtex["Color"].device))
        before = {n: t.cpu().numpy().copy() for n, t in bind.items()}
        g = ptamd.FrameGeneration(ctx)
        with pytest.raises(ptamd.PtInvalidArgument, match="pt_frame_generation_set_constants"):
            g.Process(jitter, bind)
        ctx.sync()
        assert g.DownloadField()[0].shape == (0, 0)
        for n, t in bind.items():
            assert t.cpu().numpy().tobytes() == before[n].tobytes(), n
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end: Cornell "ggx", 24 x 16 -> 48 x 32, SPP5 spp, 3 bounces, the camera translating sideways by STEP5 a frame for FRAMES5 frames,
# the Halton jitter and FrameIndex 0.., through render(..., upscale=, post=, generate=). Truth: the unjittered 48 x 32 frame from the pose
# half a step before the last one at TRUTH_SPP samples per pixel through the same post settings.
RENDER5, OUTPUT5, BOUNCES5, FRAMES5, SPP5, TRUTH_SPP, STEP5, START5 = (24, 16), (48, 32), 3, 6, 64, 2048, 0.08, -0.2


def camera_at(S, x, previous_x, jitter):
    """the Cornell camera at (x, 0, -1.95) whose Previous* members are the camera at previous_x"""
    aspect = OUTPUT5[0] / OUTPUT5[1]
    cam, prev = S.make_camera((x, 0, -1.95), aspect=aspect, jitter=jitter), S.make_camera((previous_x, 0, -1.95), aspect=aspect)
    cam["PreviousPosition"] = prev["Position"]
    for n in ("WorldToProjection", "ProjectionToView", "ViewToWorld"):
        cam["Previous" + n] = prev[n]
    cam["PreviousWorldToView"], cam["PreviousViewToProjection"] = prev["PreviousWorldToView"], prev["PreviousViewToProjection"]
    return cam


@pytest.fixture(scope="module")
def cornell(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    gpu.set_debug_flags(0)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=OUTPUT5[0] / OUTPUT5[1], variant="ggx"))
    out = {}
    r = ptamd.Renderer(gpu, g, *RENDER5)
    up = r.upscaler(*OUTPUT5)
    up.ResetHistory()
    fg = r.frame_generation(*OUTPUT5)
    fg.ResetHistory()
    post = L.post_processing_settings(*OUTPUT5)

    def settings(size, frame, spp):
        gs = S.graphics_settings(size[0], size[1], spp=spp, bounces=BOUNCES5, frame_index=frame)
        gs["Denoiser"] = L.DENOISER_NONE
        return gs

    colors = []
    for f in range(FRAMES5):
        x = START5 + STEP5 * f
        g.desc.camera[...] = camera_at(S, x, x - STEP5 if f else x, ptamd.upscaler_jitter(f, RENDER5, OUTPUT5))
        r.render(settings(RENDER5, f, SPP5), upscale=up, post=post, generate=fg)
        gpu.sync()
        assert r.generated == (f > 0)
        colors.append(r.textures["Color"].cpu().numpy().view(np.uint16).copy())
    out["generated"] = r.textures["Generated"].cpu().numpy().view(np.uint16).copy()
    assert tuple(r.textures["Generated8"].shape) == (OUTPUT5[1], OUTPUT5[0], 4) and r.textures["Generated8"].element_size() == 1
    out["generated8"] = r.textures["Generated8"].cpu().numpy().view(np.uint32).reshape(OUTPUT5[1], OUTPUT5[0]).copy()
    out["previous"], out["current"] = colors[-2], colors[-1]
    out["classes"] = fg.DownloadField()[1]
    x = START5 + STEP5 * (FRAMES5 - 1.5)
    g.desc.camera[...] = camera_at(S, x, x, (0.0, 0.0))
    r = ptamd.Renderer(gpu, g, *OUTPUT5)
    r.render(settings(OUTPUT5, 0, TRUTH_SPP), post=post)
    gpu.sync()
    out["truth"] = r.textures["Color"].cpu().numpy().view(np.uint16).copy()
    yield out
    g.close()


def test_the_generated_frame_is_closer_to_the_middle_pose_than_the_previous_frame(cornell):
    """the inequality only; the figures are recorded in DESIGN.md section 1, "Frame generation" """
    f64 = lambda bits: R.f16_to_f32(bits)[..., :3].astype(np.float64)
    truth = f64(cornell["truth"])
    rms = {k: float(np.sqrt(((f64(cornell[k]) - truth) ** 2).mean())) for k in ("generated", "previous", "current")}
    counts = np.bincount(cornell["classes"].ravel(), minlength=4).tolist()
    print(f"Cornell {RENDER5} -> {OUTPUT5}, {SPP5} spp, camera step {STEP5}: rms error against the middle pose at {TRUTH_SPP} spp: previous frame "
          f"{rms['previous']:.5f}, current frame {rms['current']:.5f}, generated {rms['generated']:.5f} (ratio to the previous frame "
          f"{rms['generated'] / rms['previous']:.4f}); classes both / current / previous / fallback {counts}")
    assert cornell["generated"].shape == (OUTPUT5[1], OUTPUT5[0], 4) and (cornell["generated"][..., 3] == R.ONE16).all()
    assert_same(cornell["generated8"], R.pack8(cornell["generated"]), "Generated8 of the chain")
    assert np.isfinite(rms["generated"]) and rms["generated"] < rms["previous"]
    # no class count is asserted: at 24 x 16 a render pixel of the side walls spans a tenth of its depth, so the nearest-sample depth test
    # (1 %) rejects the previous tap wherever the nearest previous sample is not the surface's own, and most pixels are "current only"
    assert sum(counts) == OUTPUT5[0] * OUTPUT5[1]


def test_cpp_host_runs_the_same_sequence(tmp_path, cornell):
    """pt_demo --frame-generation on that case (the same camera path through --camera-start / --camera-step) writes the harness's bytes:
    Generated, and its 8-bit form as a PNG of the output size"""
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    out, png = str(tmp_path / "generated.bin"), str(tmp_path / "generated.png")
    cmd = [DEMO, "--upscale", "performance", "--output-size", f"{OUTPUT5[0]}x{OUTPUT5[1]}", "--spp", str(SPP5), "--bounces", str(BOUNCES5),
           "--frames", str(FRAMES5), "--post", "--frame-generation", "--camera-start", repr(START5), "--camera-step", repr(STEP5),
           "--out-generated", out, "--png-generated", png]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert_same(np.fromfile(out, np.uint16).reshape(OUTPUT5[1], OUTPUT5[0], 4), cornell["generated"], "pt_demo --frame-generation")
    data = open(png, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and int.from_bytes(data[16:20], "big") == OUTPUT5[0] and int.from_bytes(data[20:24], "big") == OUTPUT5[1]
    for flags, word in ((["--frame-generation"], "--post"), (["--post", "--frame-generation", "--frames", "1"], "--frames"),
                        (["--post", "--fg-phase", "0.25"], "need --frame-generation"),
                        (["--post", "--frame-generation", "--fg-phase", "1.0"], "Phase")):
        q = subprocess.run([DEMO, "--width", "32", "--height", "16", "--spp", "1", "--bounces", "1"] + flags, capture_output=True, text=True, timeout=120)
        assert q.returncode != 0 and word in q.stderr, (flags, q.stderr)


def test_a_static_sequence_is_the_blend_in_both_hosts(tmp_path, gpu, ptamd, pkg):
    """no camera motion, no animation, native 48 x 32, jitter 0: every pixel keeps its depth and its motion vector is 0 up to the fp32
    rounding of the two projections (measured below 2^-8 pixel, not exactly 0), so every pixel is class "both" and the generated frame is
    the restatement's on the downloaded textures, which is prev + (cur - prev) / 2 of the two displayed frames up to those residual
    motions (the largest deviation is printed); pt_demo --frame-generation without a camera path writes the same bytes"""
    S, L = pkg.scenes, pkg.layouts
    size = OUTPUT5
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=size[0] / size[1], variant="ggx"))
    try:
        r = ptamd.Renderer(gpu, g, *size)
        fg = r.frame_generation(*size)
        fg.ResetHistory()
        colors = []
        for frame in (1, 0):                                   # pt_demo's order without a temporal pass: the last frame has FrameIndex 0
            gs = S.graphics_settings(size[0], size[1], spp=4, bounces=2, frame_index=frame)
            gs["Denoiser"] = L.DENOISER_NONE
            r.render(gs, post=L.post_processing_settings(*size), generate=fg)
            gpu.sync()
            colors.append({"Color": r.textures["Color"].cpu().numpy().view(np.uint16).copy(),
                           "LinearDepth": r.textures["LinearDepth"].cpu().numpy().copy(),
                           "MotionVector": r.textures["MotionVector"].cpu().numpy().view(np.uint16).copy()})
        generated = r.textures["Generated"].cpu().numpy().view(np.uint16).copy()
        classes = fg.DownloadField()[1]
    finally:
        g.close()
    assert r.generated and (classes == R.BOTH).all() and colors[0]["Color"].tobytes() != colors[1]["Color"].tobytes()
    motion = np.abs(R.f16_to_f32(colors[1]["MotionVector"])[..., :2]).max()
    assert motion < 2.0 ** -8
    ref = R.FrameGeneration(size, size)
    ref.process(colors[0], (0.0, 0.0))
    assert_same(generated, ref.process(colors[1], (0.0, 0.0))[0], "the restatement on the downloaded frames")
    p0, p1 = R.guarded_rgb(colors[0]["Color"]), R.guarded_rgb(colors[1]["Color"])
    blend = (p0 + (p1 - p0) * np.float32(0.5)).astype(np.float64)
    off = np.abs(R.f16_to_f32(generated)[..., :3].astype(np.float64) - blend)
    print(f"static sequence: largest motion {motion:.3g} pixel, largest deviation from the blend {off.max():.3g} ({int((off > 0).sum())} values)")
    # a tap displaced by d pixels mixes in at most d of a neighbour: colours are in [0, 1] after the tone map, plus the fp16 store
    assert off.max() <= 2.0 * motion + 2.0 ** -11
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    out = str(tmp_path / "generated.bin")
    p = subprocess.run([DEMO, "--width", str(size[0]), "--height", str(size[1]), "--spp", "4", "--bounces", "2", "--frames", "2", "--post",
                        "--frame-generation", "--out-generated", out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert_same(np.fromfile(out, np.uint16).reshape(size[1], size[0], 4), generated, "pt_demo --frame-generation, static")


def test_the_python_layer_refuses_what_it_must(gpu, ptamd, pkg):
    """Renderer.frame_generation on a sharded context; render(generate=) with something that is no FrameGeneration, without constants,
    with a RenderSize or an OutputSize that differs from the renderer's and the post chain's"""
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=OUTPUT5[0] / OUTPUT5[1], variant="ggx"))
    try:
        r = ptamd.Renderer(gpu, g, *RENDER5)
        gs = S.graphics_settings(*RENDER5, spp=1, bounces=1)
        gs["Denoiser"] = L.DENOISER_NONE
        up, post = r.upscaler(*OUTPUT5), L.post_processing_settings(*OUTPUT5)
        fg = r.frame_generation(*OUTPUT5, Phase=0.25)
        assert float(fg.settings["Phase"]) == 0.25 and tuple(fg.settings["OutputSize"]) == OUTPUT5
        with pytest.raises(ValueError, match="Phase"):
            r.frame_generation(*OUTPUT5, Phase=1.0)
        with pytest.raises(ptamd.PtInvalidArgument, match="generate needs post"):
            r.render(gs, upscale=up, generate=fg)
        with pytest.raises(ptamd.PtInvalidArgument, match="must be a FrameGeneration"):
            r.render(gs, upscale=up, post=post, generate=up)
        with pytest.raises(ptamd.PtInvalidArgument, match="must be a FrameGeneration"):
            r.render(gs, upscale=up, post=post, generate=ptamd.FrameGeneration(gpu))       # no constants
        other = ptamd.FrameGeneration(gpu)
        other.SetConstants(L.frame_generation_settings((20, 12), OUTPUT5))
        with pytest.raises(ptamd.PtInvalidArgument, match="RenderSize"):
            r.render(gs, upscale=up, post=post, generate=other)
        other.SetConstants(L.frame_generation_settings(RENDER5, RENDER5))
        with pytest.raises(ptamd.PtInvalidArgument, match="OutputSize"):
            r.render(gs, upscale=up, post=post, generate=other)
        assert "Generated" not in r.textures                   # nothing was allocated or run by a refused call
        gpu.set_sharding(0, 2, 16)
        try:
            with pytest.raises(ptamd.PtInvalidArgument, match="sharded"):
                r.frame_generation(*OUTPUT5)
        finally:
            gpu.set_sharding(0, 1, 16)
        r.render(gs, upscale=up, post=post, generate=fg)       # and the accepted call runs
        gpu.sync()
        assert tuple(r.textures["Generated"].shape) == (OUTPUT5[1], OUTPUT5[0], 4)
    finally:
        g.close()
