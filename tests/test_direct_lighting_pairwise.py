"""Pairwise bias correction of the DI reuse passes on the GPU (pt_di_set_pairwise): pinned per pixel against the float64 restatement
(tests/pairwiseref.py) on a moving camera, with and without the Visibility word; off is the parent's output bit for bit; unbiased against
the closed form; the setter's and the render's refusals; pt_demo --restir-pairwise."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import bsdfref
import dipins
import pairwiseref as P
import restirref as R
import restirvisref as V
import visscene

NEAR = 1e-5
# W against the float64 restatement, relative. The Basic pins hold 2e-5 (measured 1.3e-5). Measured here, maximum over the frames of
# each configuration: temporal-pairwise-boiling 9.98e-6, spatial-pairwise-1 and -2 1.11e-5, both-pairwise 1.05e-5,
# both-pairwise-visibility 1.05e-5. The limit is 1.5 x the largest ("Pairwise bias correction"); an error above
# 1e-4 would be a rule that differs, not rounding.
W_LIMIT = 1.67e-5


CONFIGS = [  # (name, temporal, spatial samples, boiling, visibility in the reservoirs)
    ("temporal-pairwise-boiling", True, 0, True, False),
    ("spatial-pairwise-1", False, 1, False, False),
    ("spatial-pairwise-2", False, 2, False, False),
    ("both-pairwise", True, 1, False, False),
    ("both-pairwise-visibility", True, 1, False, True),
]


def _pairwise_pin(ptamd, pkg, name, temporal, spatial, boiling, vis, W, H):
    """3 frames of W x H on the pin scene with the camera moving 0.17 per frame, 8 candidates, every pass that is on Pairwise. Each
    frame's final reservoirs match pairwiseref, fed the downloaded G-buffers, motion vectors, light records, last frame's final
    reservoirs and the frame's initial reservoirs (from a second context: temporal-only, Off, history reset before every frame):
    LightIndex, M, Age, U, V (and with visibility the Visibility word) exactly, W to W_LIMIT relative. With visibility
    (di_visibility_settings() defaults: initial visibility, final-visibility reuse) the restatement applies initial visibility and final
    shading itself (tests/restirvisref.py). Pixels within 1e-5 of a decision are left out and counted, and so is every pixel that reused
    such a pixel's reservoir. Both contexts are the test's own: the reuse settings end with them, not on the session's shared context.
    Returns what the restatement counted on the way. Left out, of the valid pixels, measured over the five configurations: 48 x 32 0.7 to
    1.3 %, 37 x 23 0.6 to 1.8 %, 21 x 13 0 to 0.7 %; W rel err max 1.11e-5, 8.8e-6 and 5.0e-6."""
    S, L = pkg.scenes, pkg.layouts
    n, F0 = 8, 40
    gpu = ptamd.DeviceContext(0)
    bsdf = bsdfref.Reference()
    table = R.offset_table()
    basic = L.DI_BIAS_CORRECTION_BASIC
    reuse = L.di_resampling_settings(temporal=temporal, spatial_samples=spatial, temporal_bias=basic, spatial_bias=basic, boiling_filter=boiling)
    pairwise = L.di_pairwise_settings(temporal=True, spatial=True)         # (the flag of a pass that is off is ignored)
    settings = L.di_visibility_settings() if vis else None
    init = L.di_resampling_settings(temporal=True, spatial_samples=0, temporal_bias=L.DI_BIAS_CORRECTION_OFF, boiling_filter=False)
    scene = visscene.pin_scene(S, W / H)
    occ = V.Occluders(scene) if vis else None
    g = ptamd.Scene(gpu, scene)
    ctx2 = ptamd.DeviceContext(0)
    g2 = ptamd.Scene(ctx2, scene)
    r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True, di_history=True)
    r2 = ptamd.Renderer(ctx2, g2, W, H, with_denoiser_outputs=True, di_history=True)
    cam = scene.camera.copy()
    history, excluded, compared, valid_px, worst = None, 0, 0, 0, 0.0
    seen = {}
    for f in range(3):
        if f:
            cam = visscene.move(S, cam, cam, 0.17)
        visscene.set_camera(r, cam); visscene.set_camera(r2, cam)
        gs = S.graphics_settings(W, H, spp=1, bounces=1, frame_index=F0 + f)
        r.render(gs, di_samples=n, di_reuse=reuse, di_visibility=settings, di_pairwise=pairwise); gpu.sync()
        r2.direct_lighting.ResetHistory()
        r2.render(gs, di_samples=n, di_reuse=init); ctx2.sync()
        out = ptamd.textures_to_numpy(r.textures)
        got = R.as_frame(r.direct_lighting.download_reservoirs(), H, W)
        fresh = R.as_frame(r2.direct_lighting.download_reservoirs(), H, W)
        fresh["Age"][:] = 0
        lights = r.direct_lighting.download_lights()
        cur = R.Surfaces(out, cam)
        mv = out["MotionVector"].view(np.float16).astype(np.float32)
        exp, margin = fresh, np.full((H, W), np.inf)
        if vis:
            exp, margin, emptied = V.initial_visibility(cur, fresh, lights, occ, n)
            seen["emptied"] = seen.get("emptied", 0) + int(emptied.sum())
        if temporal:
            prev = R.Surfaces(out, cam, previous=True) if f else None
            exp, margin = P.temporal_pass(cur, prev, mv, exp, history if f else None, lights, F0 + f, bsdf, 20, boiling, 0.2, in_margin=margin, stats=seen)
            if f:
                seen["disoccluded"] = seen.get("disoccluded", 0) + int((cur.valid & (exp["M"] == n)).sum())
        if spatial:
            exp, margin = P.spatial_pass(cur, exp, margin, lights, table, F0 + f, bsdf, spatial, 8, 20, 32.0, stats=seen)
        fields = ["LightIndex", "M", "Age"]
        if vis:
            exp, margin, info = V.final_pass(cur, exp, margin, lights, occ, reuse=True, max_age=4, max_distance=16.0)
            seen["reused"] = seen.get("reused", 0) + int((info["reused"] & (margin >= NEAR)).sum())
            fields.append("Visibility")
        sel = cur.valid & (margin >= NEAR)
        excluded += int((cur.valid & ~sel).sum()); compared += int(sel.sum()); valid_px += int(cur.valid.sum())
        for k in fields:
            bad = sel & (got[k] != exp[k])
            assert not bad.any(), (name, f, k, np.argwhere(bad)[:5].tolist(), got[k][bad][:5], exp[k][bad][:5], margin[bad][:5],
                                   got["LightIndex"][bad][:5], exp["LightIndex"][bad][:5], got["W"][bad][:5], exp["W"][bad][:5])
        for k in ("U", "V"):
            assert np.array_equal(got[k][sel].astype(np.float32), exp[k][sel].astype(np.float32)), (name, f, k)
        rel = np.abs(got["W"][sel] - exp["W"][sel]) / np.maximum(np.abs(exp["W"][sel]), 1e-30)
        rel = np.where((got["W"][sel] == 0) & (exp["W"][sel] == 0), 0.0, rel)
        print(f"{name} frame {f}: W rel err max {rel.max():.2e} p99 {np.quantile(rel, 0.99):.2e}")
        w = np.argwhere(sel)[np.argmax(rel)]
        assert rel.max() <= W_LIMIT, (name, f, rel.max(), w.tolist(), margin[tuple(w)], got["W"][tuple(w)], exp["W"][tuple(w)], got["M"][tuple(w)])
        worst = max(worst, float(rel.max()))
        history = got
    print(f"{name}: {compared} pixels compared, {excluded} within {NEAR} of a decision ({excluded / max(1, valid_px):.3%} of valid), "
          f"W rel err max {worst:.2e}, exercised {seen}")
    assert compared > 0.3 * 3 * W * H
    assert excluded < 0.25 * (compared + excluded)
    if temporal:
        assert seen["disoccluded"] > 0 and seen["from_history"] > 0        # the motion disoccluded pixels; others took the history's sample
    if spatial:
        assert seen["from_centre"] > 0 and seen["from_neighbour"] > 0 and seen["slots_left"] > 0
    if vis:
        assert seen["emptied"] > 0 and seen["reused"] > 0
    del r, r2
    g2.close(); ctx2.close(); g.close(); gpu.close()
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("name,temporal,spatial,boiling,vis", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gpu_pairwise_pinned_per_pixel(ptamd, pkg, name, temporal, spatial, boiling, vis):
    """_pairwise_pin at 48 x 32"""
    _pairwise_pin(ptamd, pkg, name, temporal, spatial, boiling, vis, 48, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", dipins.RAGGED, ids=dipins.size_id)
@pytest.mark.parametrize("name,temporal,spatial,boiling,vis", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gpu_pairwise_pinned_per_pixel_ragged(ptamd, pkg, name, temporal, spatial, boiling, vis, size):
    """_pairwise_pin at the sizes that cut every tile of the DI kernels on both axes (tests/dipins.py): same scene, camera path, settings,
    W_LIMIT and caps, and the run must have reached the edges."""
    W, H = size
    seen = _pairwise_pin(ptamd, pkg, name, temporal, spatial, boiling, vis, W, H)
    dipins.assert_edge_witnesses(seen, W, H, name, temporal=temporal, spatial=spatial > 0, boiling=temporal and boiling)


def _di_bytes(ptamd, r):
    out = ptamd.textures_to_numpy(r.textures)
    return {k: out[k].tobytes() for k in ("Diffuse", "Specular", "Radiance")}, r.direct_lighting.download_reservoirs().tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("bias", ["basic", "off"])
def test_gpu_pairwise_off_is_today(ptamd, pkg, bias):
    """3 frames of temporal + spatial reuse on the Cornell box, Basic or Off: di_pairwise=None and the all-zero struct give the Diffuse /
    Specular / Radiance and reservoir bytes of a context on which pt_di_set_pairwise was never called. A fourth context switches Pairwise on
    for one frame and back off: the history is reset both times (every M is the candidate count again), and from there its frames are
    those of a never-called context started at that frame."""
    S, L = pkg.scenes, pkg.layouts
    W, H, n = 48, 32, 8
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    b = L.DI_BIAS_CORRECTION_BASIC if bias == "basic" else L.DI_BIAS_CORRECTION_OFF
    reuse = L.di_resampling_settings(temporal_bias=b, spatial_bias=b)
    on = L.di_pairwise_settings(temporal=True, spatial=True)

    def run(how, frames, pairwise_at=()):
        ctx = ptamd.DeviceContext(0)
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W, H, with_denoiser_outputs=True, di_history=True)
        if how == "never":
            r.direct_lighting.SetPairwise = lambda settings: None
        off = np.zeros((), L.PT_DI_PAIRWISE_SETTINGS) if how == "zero" else None
        res = []
        for f in frames:
            pw = on if f in pairwise_at else off
            # Pairwise needs Basic: the frame that switches it on runs both passes Basic whatever `bias` is
            ru = L.di_resampling_settings() if f in pairwise_at else reuse
            r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=70 + f), di_samples=n, di_reuse=ru, di_pairwise=pw)
            ctx.sync()
            res.append(_di_bytes(ptamd, r) + (r.direct_lighting.download_reservoirs(),))
        del r
        g.close(); ctx.close()
        return res
    never = run("never", range(3))
    assert (never[2][2]["M"] > n).any()                                    # the history was used
    for how in ("none", "zero"):
        for f, (a, c) in enumerate(zip(run(how, range(3)), never)):
            for k in a[0]:
                assert a[0][k] == c[0][k], (how, f, k)
            assert a[1] == c[1], (how, f)
    # (with Off the switching frame changes the resampling settings too; with Basic the reset is pt_di_set_pairwise's alone)
    toggled = run("none", range(5), pairwise_at=(2,))
    assert (toggled[1][2]["M"] > n).any()
    assert (toggled[2][2]["M"] <= 9 * n).all() and (toggled[2][2]["Age"] == 0).all()      # on: no history (the centre and 8 boosted slots of fresh ones)
    assert (toggled[3][2]["M"] <= 9 * n).all() and (toggled[3][2]["Age"] == 0).all()      # off again: no history either
    restart = run("never", range(3, 5))
    assert (restart[1][2]["M"] > 9 * n).any()
    for f, (a, c) in enumerate(zip(toggled[3:], restart)):
        for k in a[0]:
            assert a[0][k] == c[0][k], (f, k)
        assert a[1] == c[1], f


def _floor_mask(gb):
    pos = gb["Position"][..., :3].astype(np.float64)
    return np.isfinite(pos).all(-1) & (np.abs(pos[..., 1] + 1) < 1e-4) & (pos[..., 0] > -0.55) & (pos[..., 0] < -0.15) & \
        (pos[..., 2] > -0.6) & (pos[..., 2] < -0.45), pos


@pytest.mark.gpu
def test_gpu_pairwise_reuse_unbiased(ptamd, pkg):
    """Temporal + spatial reuse with Pairwise bias correction is unbiased on the unoccluded floor of the Lambertian Cornell box: frame 4 of
    48 independent sequences (history reset between them) against the polygon form-factor closed form, within 4 standard errors of the
    measured spread (+ 2e-3 relative: fp16 storage). The per-pixel variance is printed next to Basic's on the same sequences."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 48
    ext = L.EXT_LAMBERTIAN_ONLY
    scene = S.cornell_box(aspect=W / H, variant="diffuse")
    gpu = ptamd.DeviceContext(0)                                           # its own: the reuse settings end with it
    g = ptamd.Scene(gpu, scene)
    r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True, di_history=True)
    K, F = 48, 4

    def sequences(pairwise):
        vals = []
        for k in range(K):
            r.direct_lighting.ResetHistory()
            for f in range(F):
                r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=2000 + k * F + f, ext_flags=ext), di_samples=4,
                         di_reuse=L.di_resampling_settings(), di_pairwise=pairwise)
            gpu.sync()
            o = ptamd.textures_to_numpy(r.textures)
            vals.append(o["Diffuse"][..., :3].view(np.float16).astype(np.float64) + o["Specular"][..., :3].view(np.float16).astype(np.float64))
        return np.stack(vals), o
    vals, o = sequences(L.di_pairwise_settings(temporal=True, spatial=True))
    assert (r.direct_lighting.download_reservoirs()["M"] > 4 * 9).any()    # history and neighbours were merged
    basic, _ = sequences(None)
    assert not np.array_equal(vals, basic)
    floor, pos = _floor_mask(o)
    assert floor.sum() >= 3
    M = scene.instance_data["ObjectToWorld"][5].reshape(3, 4).astype(np.float64)
    light = scene.nodes[scene.objects[5].node].meshes[0].vertices["Position"].astype(np.float64) @ M[:, :3].T + M[:, 3]
    albedo = o["BaseColorMetalness"][..., :3].astype(np.float64) / 255.0
    expect = np.zeros_like(vals[0])
    for y, x in zip(*np.nonzero(floor)):
        ff = 0.0
        for e in range(4):
            a, b = light[e] - pos[y, x], light[(e + 1) % 4] - pos[y, x]
            a /= np.linalg.norm(a); b /= np.linalg.norm(b)
            c = np.cross(a, b)
            ff += np.arccos(np.clip(a @ b, -1, 1)) * (c / np.linalg.norm(c)) @ np.array([0, 1.0, 0])
        expect[y, x] = albedo[y, x] / np.pi * 15.0 * abs(ff) / 2
    mean, se = vals.mean(0), vals.std(0, ddof=1) / np.sqrt(K)
    tol = 4 * se + 2e-3 * expect
    z = np.abs(mean - expect)[floor] / np.maximum(tol[floor], 1e-12)
    print(f"pairwise: {floor.sum()} floor pixels, max |mean - expected| / (4 sigma) = {z.max():.2f}")
    print(f"per-pixel variance on the floor pixels (mean over pixels and channels): pairwise {vals.var(0, ddof=1)[floor].mean():.3e}, "
          f"basic {basic.var(0, ddof=1)[floor].mean():.3e}")
    assert (z <= 1).all(), z.max()
    del r
    g.close(); gpu.close()


@pytest.mark.gpu
def test_gpu_pairwise_errors(ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H, n = 48, 32, 8
    ctx = ptamd.DeviceContext(0)
    scene = visscene.pin_scene(S, W / H)
    g = ptamd.Scene(ctx, scene)
    r = ptamd.Renderer(ctx, g, W, H, with_denoiser_outputs=True, di_history=True)
    di = r.direct_lighting
    for field, value in (("TemporalPairwise", 2), ("SpatialPairwise", 2), ("Reserved", (1, 0)), ("Reserved", (0, 7))):
        bad = L.di_pairwise_settings(); bad[field] = value
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            di.SetPairwise(bad)
        assert field in str(e.value), (field, str(e.value))
    di.SetPairwise(None); di.SetPairwise(np.zeros((), L.PT_DI_PAIRWISE_SETTINGS)); di.SetPairwise(L.di_pairwise_settings(True, True))
    # pt_di_set_resampling still refuses Pairwise as a mode of its own
    bad = L.di_resampling_settings(); bad["SpatialBiasCorrection"] = 2
    with pytest.raises(ptamd.PtInvalidArgument) as e:
        di.SetResampling(bad)
    assert "Pairwise and Raytraced" in str(e.value)
    gs = lambda f: S.graphics_settings(W, H, spp=1, bounces=1, frame_index=f)
    off = L.DI_BIAS_CORRECTION_OFF
    # Pairwise over a pass whose correction is Off: refused at render, the flag and BASIC named
    for flag, reuse in (("TemporalPairwise", L.di_resampling_settings(temporal_bias=off)), ("SpatialPairwise", L.di_resampling_settings(spatial_bias=off))):
        p = L.di_pairwise_settings(); p[flag] = 1
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            r.render(gs(0), di_samples=n, di_reuse=reuse, di_pairwise=p)
        assert flag in str(e.value) and "BASIC" in str(e.value)
    # Pairwise + Raytraced on one pass: refused, both named; on different passes they render
    for pw, vs, names in ((dict(temporal=True), dict(temporal_raytraced=True), ("TemporalPairwise", "TemporalRaytraced")),
                          (dict(spatial=True), dict(spatial_raytraced=True), ("SpatialPairwise", "SpatialRaytraced"))):
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            r.render(gs(0), di_samples=n, di_reuse=L.di_resampling_settings(), di_visibility=L.di_visibility_settings(**vs),
                     di_pairwise=L.di_pairwise_settings(**pw))
        assert all(nm in str(e.value) for nm in names), str(e.value)
    r.render(gs(0), di_samples=n, di_reuse=L.di_resampling_settings(), di_visibility=L.di_visibility_settings(spatial_raytraced=True),
             di_pairwise=L.di_pairwise_settings(temporal=True))
    # a flag on a pass that is off renders, whatever that pass's correction says; so does the plain pass
    r.render(gs(1), di_samples=n, di_reuse=L.di_resampling_settings(temporal=True, spatial_samples=0, spatial_bias=off),
             di_pairwise=L.di_pairwise_settings(temporal=True, spatial=True))
    r.render(gs(2), di_samples=n, di_reuse=L.di_resampling_settings(temporal=False, spatial_samples=1, temporal_bias=off),
             di_pairwise=L.di_pairwise_settings(temporal=True, spatial=True))
    r.render(gs(3), di_samples=n, di_pairwise=L.di_pairwise_settings(temporal=True, spatial=True))
    ctx.sync()
    # a changed value resets the history, the same value keeps it
    reuse = L.di_resampling_settings(temporal=True, spatial_samples=0, boiling_filter=False)
    pw = L.di_pairwise_settings(temporal=True)
    for f in range(2):
        r.render(gs(10 + f), di_samples=n, di_reuse=reuse, di_pairwise=pw)
    ctx.sync()
    assert (di.download_reservoirs()["M"] > n).any()
    r.render(gs(12), di_samples=n, di_reuse=reuse, di_pairwise=pw); ctx.sync()
    assert (di.download_reservoirs()["M"] > n).any()
    r.render(gs(13), di_samples=n, di_reuse=reuse, di_pairwise=L.di_pairwise_settings(temporal=True, spatial=True)); ctx.sync()
    res = di.download_reservoirs()
    valid = R.Surfaces(ptamd.textures_to_numpy(r.textures), scene.camera).valid.reshape(-1)
    assert valid.sum() > 0.5 * W * H and (res["M"][valid] == n).all()
    del r
    g.close(); ctx.close()


@pytest.mark.gpu
def test_cpp_host_restir_pairwise_matches_python(tmp_path, ptamd, pkg):
    """pt_demo --di --restir --restir-pairwise --frames 3 exits 0: the C++ host's BiasCorrectionMode::Pairwise in both passes (BASIC + the
    flags), bit-identical to the Python sequence and different from the run without the flag; --restir-pairwise without --restir and
    together with --restir-raytraced is refused"""
    demo = os.path.join(ge.PKG_DIR, "pt_demo")
    S, L = pkg.scenes, pkg.layouts
    W, H, spp, bounces, frames = 96, 64, 1, 2, 3
    out, out_plain = str(tmp_path / "pairwise.bin"), str(tmp_path / "basic.bin")
    common = ["--di-samples", "8", "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces), "--frames", str(frames)]
    subprocess.check_call([demo, "--di", "--restir", "--restir-pairwise"] + common + ["--out", out], timeout=300)
    subprocess.check_call([demo, "--di", "--restir"] + common + ["--out", out_plain], timeout=300)
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    plain = np.fromfile(out_plain, np.float32).reshape(H, W, 4)
    assert not np.array_equal(got.view(np.uint32), plain.view(np.uint32))  # the flag did something
    for args, message in ((["--di", "--restir-pairwise"], "--restir-pairwise needs --restir"),
                          (["--di", "--restir", "--restir-pairwise", "--restir-visibility", "--restir-raytraced"], "two bias corrections")):
        refused = subprocess.run([demo] + args + common, capture_output=True, text=True, timeout=300)
        assert refused.returncode != 0 and message in refused.stderr + refused.stdout, (args, refused.stderr)
    ctx = ptamd.DeviceContext(0)
    g = ptamd.Scene(ctx, S.cornell_box(aspect=W / H, variant="ggx"))
    r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True, di_history=True)
    for fi in [12345] + list(range(frames - 1, -1, -1)):                    # pt_demo's warm-up frame, then N-1 .. 0
        gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=fi)
        gs["IsDIEnabled"] = 1
        r.render(gs, di_samples=8, di_reuse=L.di_resampling_settings(), di_pairwise=L.di_pairwise_settings(temporal=True, spatial=True))
    ctx.sync()
    ref = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    assert (r.direct_lighting.download_reservoirs()["M"] > 8).any()        # the history was used
    g.close(); ctx.close()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
