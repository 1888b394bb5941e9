"""GPU tests of the denoiser (pt_denoiser_*) against tests/denoiseref.py, the numpy restatement of DESIGN.md section 1, "Denoiser":
the hostile synthetic sequence bit for bit in both forms of the a-trous kernel, the properties of the filter with derived bounds, the
refusals and the history's life, and the chain G-buffer -> path tracer -> pack -> denoiser -> compose end to end."""
import functools
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import denoiseref as R

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
SIZES = [(40, 24), (37, 19)]           # the second fills no 16 x 16 tile, and a step of 4 or 8 reaches across most of it
DEBUG_DIRECT, DEBUG_STAGED = 0x800, 0x1000
FORMS = [("direct", DEBUG_DIRECT), ("staged", DEBUG_STAGED)]
TEXTURES = ("Position", "LinearDepth", "NormalRoughness", "MotionVector", "NoisyDiffuse", "NoisySpecular")


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
def denoiser(gpu, ptamd):
    """the context's denoiser with no history; the debug flags are put back behind the test"""
    d = ptamd.Denoiser(gpu)
    d.ResetHistory()
    yield d
    gpu.set_debug_flags(0)
    d.ResetHistory()


@functools.lru_cache(maxsize=None)
def reference(W, H, iterations, max_frames):
    """per frame of the synthetic sequence: (DenoisedDiffuse, DenoisedSpecular, length) of denoiseref in float32. Computed once."""
    ref = R.Denoiser(W, H, np.float32, AtrousIterations=iterations, MaxAccumulatedFrames=max_frames)
    out = []
    for tex in R.synthetic_frames(W, H, seed=W * 131 + H):
        d, s = ref.process(tex)
        out.append((d, s, ref.length.copy()))
    return out


def run_frames(gpu, denoiser, L, W, H, frames, aliased, **overrides):
    """the sequence through the device: per frame (DenoisedDiffuse, DenoisedSpecular, length); checks the untouched inputs"""
    torch = _torch()
    dev = torch.device("cuda", gpu.device_ordinal)
    denoiser.SetConstants(L.denoiser_settings(W, H, **overrides))
    denoiser.ResetHistory()
    out = []
    for host in frames:
        dtex = upload(host, dev)
        bind = dict(dtex)
        if aliased:
            bind["DenoisedDiffuse"], bind["DenoisedSpecular"] = dtex["NoisyDiffuse"], dtex["NoisySpecular"]
        else:
            bind["DenoisedDiffuse"], bind["DenoisedSpecular"] = (torch.full_like(dtex["NoisyDiffuse"], 0x1234) for _ in range(2))
        denoiser.Process(bind)
        gpu.sync()
        for name in TEXTURES[:4] if aliased else TEXTURES:
            assert_same(download(dtex[name], host[name]), host[name], ("the call wrote", name))
        out.append((download(bind["DenoisedDiffuse"], host["NoisyDiffuse"]), download(bind["DenoisedSpecular"], host["NoisySpecular"]),
                    denoiser.DownloadHistory()))
    return out


@pytest.mark.parametrize("max_frames", [1, 8])
@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic_sequence_bit_for_bit(gpu, pkg, denoiser, size, iterations, max_frames):
    """three consecutive hostile frames: both outputs and the history length of every frame equal denoiseref's bytes, with the Denoised
    pair aliased with the Noisy pair and separate, in the direct and in the staged form of every a-trous step"""
    W, H = size
    frames = R.synthetic_frames(W, H, seed=W * 131 + H)
    assert all((~np.isfinite(f["LinearDepth"])).sum() >= W * H // 10 for f in frames)
    want = reference(W, H, iterations, max_frames)
    for form, flag in FORMS:
        gpu.set_debug_flags(flag)
        for aliased in (True, False):
            got = run_frames(gpu, denoiser, pkg.layouts, W, H, frames, aliased, AtrousIterations=iterations, MaxAccumulatedFrames=max_frames)
            for f, ((gd, gs, gl), (wd, ws, wl)) in enumerate(zip(got, want)):
                label = (form, "aliased" if aliased else "separate", "frame", f)
                assert_same(gl, wl.astype(np.float32), label + ("length",))
                assert_same(gd, wd, label + ("DenoisedDiffuse",))
                assert_same(gs, ws, label + ("DenoisedSpecular",))
    lengths = np.stack([w[2] for w in want[1:]])
    if max_frames > 1:                                # the sequence does reuse its history, and does lose it where it must
        assert (lengths > 1).any() and (lengths == 1).any() and (lengths != np.round(lengths)).any()
    assert (want[0][2] == 0).sum() >= W * H // 10


# ------------------------------------------------------------------------------------------------------------------------------------
# properties
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_a_constant_comes_out_equal_and_missed_pixels_keep_their_bits(gpu, pkg, denoiser, size):
    """(a) the hostile guides and motion of the synthetic sequence with one fp16-representable constant in the noisy pair of every hit
    pixel: every weighted mean of the filter is normalised, so it errs by a few tens of fp32 ulps at most -- far inside half an fp16 ulp
    (2^13 fp32 ulps) -- and the output equals the input. (b) missed pixels carry arbitrary bits through."""
    W, H = size
    c = np.float16(0.7333)
    frames = R.synthetic_frames(W, H, seed=77)
    for f in frames:
        hit = np.isfinite(f["LinearDepth"])
        for name in ("NoisyDiffuse", "NoisySpecular"):
            f[name][hit] = c.view(np.uint16)
    for form, flag in FORMS:
        gpu.set_debug_flags(flag)
        got = run_frames(gpu, denoiser, pkg.layouts, W, H, frames, aliased=False, MaxAccumulatedFrames=8)
        for f, (gd, gs, _) in zip(frames, got):
            hit = np.isfinite(f["LinearDepth"])
            assert (~hit).sum() >= W * H // 10
            for g, name in ((gd, "NoisyDiffuse"), (gs, "NoisySpecular")):
                assert (g[hit] == c.view(np.uint16)).all(), (form, name)
                assert_same(g[~hit], f[name][~hit], (form, "missed", name))


def test_history_lengths_follow_the_motion(gpu, pkg, denoiser):
    """(c) after frame 2 of a static sequence every hit pixel has length 2; with the camera shifted by three pixels exactly the strip
    without a predecessor (the last three columns) and the strip that fails the depth test have length 1"""
    W, H = SIZES[0]
    rng = np.random.default_rng(3)
    colour = lambda: rng.uniform(0.1, 2.0, (H, W, 4))
    L = pkg.layouts
    static = [R.plain_frame(W, H, colour()) for _ in range(2)]
    static[1]["LinearDepth"][5, 7] = np.inf
    got = run_frames(gpu, denoiser, L, W, H, static, aliased=True)
    want = np.full((H, W), 2.0, np.float32); want[5, 7] = 0.0
    assert_same(got[1][2], want, "static")
    assert (got[0][2] == 1.0).all()
    moved = [R.plain_frame(W, H, colour()), R.plain_frame(W, H, colour(), motion=(3.0, 0.0, 0.0))]
    mv = moved[1]["MotionVector"].view(np.float16)
    mv[8:11, :, 2] = 1.0                              # the previous depth would be 6: further than 1 % from the 5 the history holds
    got = run_frames(gpu, denoiser, L, W, H, moved, aliased=True)
    want = np.full((H, W), 2.0, np.float32); want[:, W - 3:] = 1.0; want[8:11] = 1.0
    assert_same(got[1][2], want, "shifted")


def test_noise_goes_down_and_the_edge_does_not_bleed(gpu, pkg, denoiser):
    """(d) eight static frames of two half-planes of radiance 1 and 4 that meet at a depth and normal edge, i.i.d. uniform noise of
    +-0.5 on every channel and frame. Temporal accumulation alone leaves an eighth of the input variance; the a-trous passes only lower
    it; the bound of a quarter leaves room for the sampling spread of a side's few hundred pixels. Every weight of the filter is >= 0
    and every mean normalised, and no tap crosses the edge (the plane distance is 2 against a scale of 0.05, the normals' cosine 0.6
    against 0.8), so no output of a side leaves the range that side's inputs spanned."""
    W, H = SIZES[0]
    rng = np.random.default_rng(11)
    xs = np.mgrid[0:H, 0:W][1]
    sides = [xs < W // 2, xs >= W // 2]
    frames = []
    for _ in range(8):
        c = np.where(sides[1][..., None], 4.0, 1.0) + rng.uniform(-0.5, 0.5, (H, W, 4))
        frames.append(R.plain_frame(W, H, c, edge=True))
    for form, flag in FORMS:
        gpu.set_debug_flags(flag)
        got = run_frames(gpu, denoiser, pkg.layouts, W, H, frames, aliased=False)
        assert (got[-1][2] == 8.0).all()
        for ch, name in ((0, "NoisyDiffuse"), (1, "NoisySpecular")):
            out = R.f16_to_f32(got[-1][ch]).astype(np.float64)
            inputs = np.stack([R.f16_to_f32(f[name]).astype(np.float64) for f in frames])
            for k, side in enumerate(sides):
                v_in, v_out = inputs[-1][side][:, :3].var(), out[side][:, :3].var()
                lo, hi = inputs[:, side].min(), inputs[:, side].max()
                print(f"{form} {name} side {k}: input variance {v_in:.4f}, output variance {v_out:.5f} (ratio {v_out / v_in:.4f}), "
                      f"output range [{out[side].min():.3f}, {out[side].max():.3f}] inside the inputs' [{lo:.3f}, {hi:.3f}]")
                assert v_out < v_in / 4, (form, name, k)
                assert out[side].min() >= lo and out[side].max() <= hi, (form, name, k)


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals and state
def raw_settings(L, W, H, **fields):
    s = np.zeros((), L.DENOISER_SETTINGS)
    s["RenderSize"] = (W, H)
    for k, v in dict(L.DENOISER_DEFAULTS, **fields).items():
        s[k] = v
    return s


def test_refusals_name_the_field_and_touch_nothing(gpu, ptamd, pkg, denoiser):
    L = pkg.layouts
    torch = _torch()
    W, H = 16, 6
    dev = torch.device("cuda", gpu.device_ordinal)
    frames = R.synthetic_frames(W, H, seed=5, frames=2)
    denoiser.SetConstants(L.denoiser_settings(W, H))
    dtex = upload(frames[0], dev)
    bind = dict(dtex, DenoisedDiffuse=torch.zeros_like(dtex["NoisyDiffuse"]), DenoisedSpecular=torch.zeros_like(dtex["NoisySpecular"]))
    denoiser.Process(bind)
    gpu.sync()
    length = denoiser.DownloadHistory()
    outputs = {n: bind[n].cpu().numpy().copy() for n in ("DenoisedDiffuse", "DenoisedSpecular")}
    assert length.shape == (H, W) and length.max() == 1.0

    def untouched(label):
        gpu.sync()
        assert_same(denoiser.DownloadHistory(), length, (label, "history"))
        for n, v in outputs.items():
            assert_same(bind[n].cpu().numpy(), v, (label, n))
        for n in TEXTURES:
            assert_same(download(dtex[n], frames[0][n]), frames[0][n], (label, n))

    # out-of-range settings, by name: refused, the previous settings and the history stay
    bad = [("RenderSize", raw_settings(L, 0, H)), ("RenderSize", raw_settings(L, W, 16385)),
           ("MaxAccumulatedFrames", raw_settings(L, W, H, MaxAccumulatedFrames=0)), ("MaxAccumulatedFrames", raw_settings(L, W, H, MaxAccumulatedFrames=256)),
           ("AtrousIterations", raw_settings(L, W, H, AtrousIterations=9)),
           ("DepthThreshold", raw_settings(L, W, H, DepthThreshold=0.0)), ("DepthThreshold", raw_settings(L, W, H, DepthThreshold=1.5)),
           ("DepthThreshold", raw_settings(L, W, H, DepthThreshold=np.nan)),
           ("NormalCosine", raw_settings(L, W, H, NormalCosine=1.0)), ("NormalCosine", raw_settings(L, W, H, NormalCosine=-0.1)),
           ("DiffuseLuminanceSigma", raw_settings(L, W, H, DiffuseLuminanceSigma=0.0)), ("DiffuseLuminanceSigma", raw_settings(L, W, H, DiffuseLuminanceSigma=np.inf)),
           ("SpecularLuminanceSigma", raw_settings(L, W, H, SpecularLuminanceSigma=-1.0)),
           ("RoughnessFraction", raw_settings(L, W, H, RoughnessFraction=0.0)), ("RoughnessFraction", raw_settings(L, W, H, RoughnessFraction=np.nan))]
    for word, s in bad:
        with pytest.raises(ptamd.PtInvalidArgument, match=word):
            denoiser.SetConstants(s)
        with pytest.raises(ValueError, match=word):
            L.check_denoiser_settings(s)
    untouched("settings")
    # every missing binding and each misalignment, by name
    for name in L.DENOISER_TEXTURES:
        with pytest.raises(ptamd.PtInvalidArgument, match=name):
            denoiser.Process({n: t for n, t in bind.items() if n != name})
        raw = bind[name].reshape(-1).view(torch.uint8)
        shifted = torch.zeros(raw.numel() + 2, dtype=torch.uint8, device=dev)[2:]
        shifted.copy_(raw)
        assert shifted.data_ptr() % 4 == 2
        with pytest.raises(ptamd.PtInvalidArgument, match=name + ".*aligned"):
            denoiser.Process(dict(bind, **{name: shifted}))
        gpu.sync()
        assert shifted.cpu().numpy().tobytes() == raw.cpu().numpy().tobytes(), name
    untouched("bindings")
    # ReBLUR's packing, through the Python wrapper (the C++ one: test_cpp_host_refuses_reblur)
    with pytest.raises(ptamd.PtInvalidArgument, match="ReBLUR"):
        denoiser.SetConstants(L.denoiser_settings(W, H), denoiser=L.DENOISER_NRD_REBLUR)
    untouched("reblur")
    # the history went on through all of it: the second frame is the reference's second frame
    ref = R.Denoiser(W, H, np.float32)
    ref.process(frames[0])
    wd, ws = ref.process(frames[1])
    d2 = upload(frames[1], dev)
    denoiser.Process(dict(d2, DenoisedDiffuse=d2["NoisyDiffuse"], DenoisedSpecular=d2["NoisySpecular"]))
    gpu.sync()
    assert_same(download(d2["NoisyDiffuse"], wd), wd, "frame 2 after the refusals")
    assert_same(download(d2["NoisySpecular"], ws), ws, "frame 2 after the refusals")
    assert_same(denoiser.DownloadHistory(), ref.length, "frame 2 after the refusals")


def test_process_before_set_constants_is_refused(ptamd, pkg):
    """a context of its own: the session's has had its constants set by other tests"""
    torch = _torch()
    ctx = ptamd.DeviceContext(0)
    try:
        W, H = 8, 4
        dtex = upload(R.synthetic_frames(W, H, seed=1, frames=1)[0], torch.device("cuda", ctx.device_ordinal))
        before = {n: t.cpu().numpy().copy() for n, t in dtex.items()}
        d = ptamd.Denoiser(ctx)
        with pytest.raises(ptamd.PtInvalidArgument, match="pt_denoiser_set_constants"):
            d.Process(dict(dtex, DenoisedDiffuse=dtex["NoisyDiffuse"], DenoisedSpecular=dtex["NoisySpecular"]))
        with pytest.raises(ptamd.PtInvalidArgument, match="SetConstants"):
            d(dtex["NoisyDiffuse"], dtex["NoisySpecular"])
        ctx.sync()
        assert d.DownloadHistory().shape == (0, 0)
        for n, t in dtex.items():
            assert t.cpu().numpy().tobytes() == before[n].tobytes(), n
    finally:
        ctx.close()


def test_size_change_settings_change_and_reset_restart_the_history(gpu, pkg, denoiser):
    L = pkg.layouts
    torch = _torch()
    dev = torch.device("cuda", gpu.device_ordinal)
    rng = np.random.default_rng(2)

    def frame(W, H):
        dtex = upload(R.plain_frame(W, H, rng.uniform(0.1, 2.0, (H, W, 4))), dev)
        denoiser.Process(dict(dtex, DenoisedDiffuse=dtex["NoisyDiffuse"], DenoisedSpecular=dtex["NoisySpecular"]))
        return denoiser.DownloadHistory()

    denoiser.SetConstants(L.denoiser_settings(24, 10))
    assert (frame(24, 10) == 1).all() and (frame(24, 10) == 2).all()
    denoiser.SetConstants(L.denoiser_settings(24, 10))               # the same settings: the history goes on
    assert (frame(24, 10) == 3).all()
    denoiser.ResetHistory()
    assert denoiser.DownloadHistory().shape == (0, 0)
    assert (frame(24, 10) == 1).all() and (frame(24, 10) == 2).all()
    denoiser.SetConstants(L.denoiser_settings(20, 12))               # another RenderSize (a smaller frame: the allocation stays)
    got = frame(20, 12)
    assert got.shape == (12, 20) and (got == 1).all() and (frame(20, 12) == 2).all()
    denoiser.SetConstants(L.denoiser_settings(20, 12, NormalCosine=0.7))   # other settings
    assert (frame(20, 12) == 1).all()
    denoiser.SetConstants(L.denoiser_settings(50, 30))               # a larger frame: the history grows
    got = frame(50, 30)
    assert got.shape == (30, 50) and (got == 1).all() and (frame(50, 30) == 2).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end: Cornell "ggx", 48 x 32, ReLAX, 1 spp, 3 bounces, static camera, FrameIndex 0..7. Truth: the Denoiser = None frame at
# TRUTH_SPP samples per pixel, whose own Monte-Carlo error is sqrt(1 / TRUTH_SPP) = 1 / 64 of a 1 spp frame's: negligible beside both
# errors compared.
W5, H5_, BOUNCES5, FRAMES5, TRUTH_SPP = 48, 32, 3, 8, 4096


def _settings5(S, L, denoiser, frame, spp):
    gs = S.graphics_settings(W5, H5_, spp=spp, bounces=BOUNCES5, frame_index=frame)
    gs["Denoiser"] = denoiser
    return gs


@pytest.fixture(scope="module")
def cornell(gpu, ptamd, pkg):
    """the composed Radiance of frame 7 with the denoiser and with the identity, and the truth. Rendered once."""
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    gpu.set_debug_flags(0)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W5 / H5_, variant="ggx"))
    out = {}
    r = ptamd.Renderer(gpu, g, W5, H5_, with_denoiser_outputs=True)
    r.denoiser.ResetHistory()
    r.denoiser.SetConstants(L.denoiser_settings(W5, H5_))
    for f in range(FRAMES5):
        r.render(_settings5(S, L, L.DENOISER_NRD_RELAX, f, 1), nrd=L.DENOISER_NRD_RELAX, denoise=r.denoiser)
    gpu.sync()
    out["denoised"] = ptamd.textures_to_numpy(r.textures)["Radiance"].copy()
    out["length"] = r.denoiser.DownloadHistory()
    r = ptamd.Renderer(gpu, g, W5, H5_, with_denoiser_outputs=True)
    r.render(_settings5(S, L, L.DENOISER_NRD_RELAX, FRAMES5 - 1, 1), nrd=L.DENOISER_NRD_RELAX)
    gpu.sync()
    out["identity"] = ptamd.textures_to_numpy(r.textures)["Radiance"].copy()
    r = ptamd.Renderer(gpu, g, W5, H5_, with_denoiser_outputs=True)
    r.render(_settings5(S, L, L.DENOISER_NONE, 0, TRUTH_SPP))
    gpu.sync()
    out["truth"] = ptamd.textures_to_numpy(r.textures)["Radiance"].copy()
    yield out
    g.close()


def test_the_chain_produces_a_frame_closer_to_the_truth(cornell):
    truth = R.f16_to_f32(cornell["truth"])[..., :3].astype(np.float64)
    rms = {k: float(np.sqrt(((R.f16_to_f32(cornell[k])[..., :3].astype(np.float64) - truth) ** 2).mean())) for k in ("denoised", "identity")}
    print(f"Cornell {W5}x{H5_}, frame {FRAMES5 - 1}: rms error against {TRUTH_SPP} spp: identity {rms['identity']:.5f}, denoised {rms['denoised']:.5f} "
          f"(ratio {rms['denoised'] / rms['identity']:.4f}); history length {cornell['length'].min():.0f}..{cornell['length'].max():.0f}")
    assert np.isfinite(rms["denoised"]) and rms["denoised"] < rms["identity"]
    assert cornell["length"].max() == FRAMES5


def test_cpp_host_runs_the_same_sequence(tmp_path, cornell):
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    out = str(tmp_path / "radiance.bin")
    cmd = [DEMO, "--width", str(W5), "--height", str(H5_), "--spp", "1", "--bounces", str(BOUNCES5), "--frames", str(FRAMES5), "--nrd", "relax",
           "--denoise", "--out-radiance", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "identity" not in p.stderr
    got = np.fromfile(out, np.uint16).reshape(H5_, W5, 4)
    assert_same(got, cornell["denoised"], "pt_demo --nrd relax --denoise")


def test_cpp_host_refuses_reblur(tmp_path):
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    p = subprocess.run([DEMO, "--width", "16", "--height", "8", "--spp", "1", "--bounces", "1", "--frames", "1", "--nrd", "reblur", "--denoise"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "ReBLUR" in p.stderr, p.stderr


def test_render_refuses_the_library_denoiser_for_reblur(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W5 / H5_, variant="ggx"))
    try:
        r = ptamd.Renderer(gpu, g, W5, H5_, with_denoiser_outputs=True)
        with pytest.raises(ptamd.PtInvalidArgument, match="ReBLUR"):
            r.render(_settings5(S, L, L.DENOISER_NRD_REBLUR, 0, 1), nrd=L.DENOISER_NRD_REBLUR, denoise=r.denoiser)
    finally:
        g.close()
