"""Visibility in the DI reservoirs on the GPU (pt_di_set_visibility): off is the parent's output bit for bit; every rule pinned per pixel
against the float64 restatement (tests/restirref.py, tests/restirvisref.py) on a moving camera; final-visibility reuse exact where it must be; Raytraced
unbiased in a penumbra where Basic is not; the setter's and the render's refusals; pt_demo --restir-visibility."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import bsdfref
import dipins
import restirref as R
import restirvisref as V
import visscene

NEAR = 1e-5


def _di_bytes(ptamd, r):
    out = ptamd.textures_to_numpy(r.textures)
    return {k: out[k].tobytes() for k in ("Diffuse", "Specular", "Radiance")}, r.direct_lighting.download_reservoirs()


@pytest.mark.gpu
def test_gpu_visibility_off_is_today(ptamd, pkg):
    """3 frames of temporal + spatial reuse on the Cornell box: di_visibility=None and the all-zero struct give the Diffuse / Specular /
    Radiance and reservoir bytes of a context on which pt_di_set_visibility was never called, and Visibility stays 0."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    results = []
    for how in ("never", "none", "zero"):
        ctx = ptamd.DeviceContext(0)
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W, H, with_denoiser_outputs=True, di_history=True)
        if how == "never":
            r.direct_lighting.SetVisibility = lambda settings: None
        vis = np.zeros((), L.PT_DI_VISIBILITY_SETTINGS) if how == "zero" else None
        frames = []
        for f in range(3):
            r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=70 + f), di_samples=8, di_reuse=L.di_resampling_settings(),
                     di_visibility=vis)
            ctx.sync()
            frames.append(_di_bytes(ptamd, r))
        results.append(frames)
        del r
        g.close(); ctx.close()
    assert (results[0][2][1]["M"] > 8).any()                              # the history was used
    for how, frames in zip(("none", "zero"), results[1:]):
        for f, ((tex, res), (tex0, res0)) in enumerate(zip(frames, results[0])):
            for k in tex:
                assert tex[k] == tex0[k], (how, f, k)
            assert res.tobytes() == res0.tobytes(), (how, f)
            assert (res["Visibility"] == 0).all()


CONFIGS = [  # (name, temporal, spatial samples, boiling, visibility settings)
    ("initial-spatial-basic", False, 1, False, dict(final_reuse=False)),
    ("temporal-raytraced", True, 0, False, dict(final_reuse=False, temporal_raytraced=True)),
    ("spatial-raytraced", False, 2, False, dict(final_reuse=False, spatial_raytraced=True)),
    ("both-raytraced-boiling", True, 1, True, dict(final_reuse=False, temporal_raytraced=True, spatial_raytraced=True)),
    ("both-raytraced-reuse", True, 1, False, dict(final_reuse=True, max_age=2, temporal_raytraced=True, spatial_raytraced=True)),
    ("both-raytraced-reuse-discard", True, 1, False, dict(final_reuse=True, max_age=2, temporal_raytraced=True, spatial_raytraced=True,
                                                          discard_invisible=True)),
]


def _visibility_pin(gpu, ptamd, pkg, name, temporal, spatial, boiling, vis, W, H):
    """4 frames of W x H on the pin scene with the camera moving 0.17 per frame, 8 candidates, initial visibility on. Each frame's final
    reservoirs match the restatement, fed the downloaded G-buffers, motion vectors, light records, last frame's final reservoirs and the
    frame's initial reservoirs (from a second context without visibility; the restatement applies initial visibility itself):
    LightIndex, M, Age, U, V and the Visibility word exactly, W to 2e-5 relative (the new arithmetic only zeroes terms; measured up to 1.5e-5,
    as without visibility). Pixels within 1e-5 of a
    decision -- restirref's, and every ray's edge values and tmin / tmax -- are left out and counted, and so is every pixel that reused
    one (measured, of the valid pixels: 48 x 32 0.8 to 1.5 %, 37 x 23 1.8 to 2.3 %, 21 x 13 0.2 to 0.5 %; 10 to 22 % at 48 x 32 with a
    spatial pass while the pin scene's roughness tie counted as a decision at risk, restirref.roughness_margin). Each configuration must
    have exercised its rule. Returns what the restatement counted on the way."""
    S, L = pkg.scenes, pkg.layouts
    n, F0 = 8, 40
    edges = {}
    bsdf = bsdfref.Reference()
    table = R.offset_table()
    basic = L.DI_BIAS_CORRECTION_BASIC
    reuse = L.di_resampling_settings(temporal=temporal, spatial_samples=spatial, temporal_bias=basic, spatial_bias=basic, boiling_filter=boiling)
    settings = L.di_visibility_settings(initial=True, **vis)
    init = L.di_resampling_settings(temporal=True, spatial_samples=0, temporal_bias=L.DI_BIAS_CORRECTION_OFF, boiling_filter=False)
    tr, sr = vis.get("temporal_raytraced", False), vis.get("spatial_raytraced", False)
    gpu.set_sharding(0, 1, 16)
    scene = visscene.pin_scene(S, W / H)
    occ = V.Occluders(scene)
    g = ptamd.Scene(gpu, scene)
    ctx2 = ptamd.DeviceContext(0)
    g2 = ptamd.Scene(ctx2, scene)
    r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True, di_history=True)
    r2 = ptamd.Renderer(ctx2, g2, W, H, with_denoiser_outputs=True, di_history=True)
    cam = scene.camera.copy()
    history, excluded, compared, valid_px = None, 0, 0, 0
    seen = {"emptied": 0, "zeroed": 0, "reused": 0, "expired": 0, "discarded": 0}
    worst = 0.0
    for f in range(4):
        if f:
            cam = visscene.move(S, cam, cam, 0.17)
        visscene.set_camera(r, cam); visscene.set_camera(r2, cam)
        gs = S.graphics_settings(W, H, spp=1, bounces=1, frame_index=F0 + f)
        r.render(gs, di_samples=n, di_reuse=reuse, di_visibility=settings); gpu.sync()
        r2.direct_lighting.ResetHistory()
        r2.render(gs, di_samples=n, di_reuse=init); ctx2.sync()
        out = ptamd.textures_to_numpy(r.textures)
        got = R.as_frame(r.direct_lighting.download_reservoirs(), H, W)
        fresh = R.as_frame(r2.direct_lighting.download_reservoirs(), H, W)
        fresh["Age"][:] = 0
        lights = r.direct_lighting.download_lights()
        cur = R.Surfaces(out, cam)
        mv = out["MotionVector"].view(np.float16).astype(np.float32)
        st = edges                                                         # the edge counters run over the frames; "zeroed" is per frame
        st["zeroed"] = 0
        exp, margin, emptied = V.initial_visibility(cur, fresh, lights, occ, n)
        seen["emptied"] += int(emptied.sum())
        if temporal:
            prev = R.Surfaces(out, cam, previous=True) if f else None
            exp, margin = R.temporal_pass(cur, prev, mv, exp, history if f else None, lights, F0 + f, bsdf, 20, True, boiling, 0.2,
                                          in_margin=margin, occ=occ, raytraced=tr, stats=st)
        if spatial:
            exp, margin = R.spatial_pass(cur, exp, margin, lights, table, F0 + f, bsdf, spatial, 8, 20, 32.0, True, occ=occ, raytraced=sr, stats=st)
        age_in = (exp["Visibility"] >> 27) & 15
        exp, margin, info = V.final_pass(cur, exp, margin, lights, occ, reuse=vis["final_reuse"], max_age=vis.get("max_age", 4),
                                         max_distance=16.0, discard=vis.get("discard_invisible", False))
        sel = cur.valid & (margin >= NEAR)
        seen["zeroed"] += st.get("zeroed", 0)
        seen["reused"] += int((info["reused"] & sel).sum()); seen["discarded"] += int((info["discarded"] & sel).sum())
        seen["expired"] += int((info["traced"] & sel & (age_in > vis.get("max_age", 4))).sum())
        excluded += int((cur.valid & ~sel).sum()); compared += int(sel.sum()); valid_px += int(cur.valid.sum())
        for k in ("LightIndex", "M", "Age", "Visibility"):
            bad = sel & (got[k] != exp[k])
            assert not bad.any(), (name, f, k, np.argwhere(bad)[:5].tolist(), got[k][bad][:5], exp[k][bad][:5], margin[bad][:5],
                                   got["LightIndex"][bad][:5], exp["LightIndex"][bad][:5], got["W"][bad][:5], exp["W"][bad][:5])
        for k in ("U", "V"):
            assert np.array_equal(got[k][sel].astype(np.float32), exp[k][sel].astype(np.float32)), (name, f, k)
        rel = np.abs(got["W"][sel] - exp["W"][sel]) / np.maximum(np.abs(exp["W"][sel]), 1e-30)
        rel = np.where((got["W"][sel] == 0) & (exp["W"][sel] == 0), 0.0, rel)
        print(f"{name} frame {f}: W rel err max {rel.max():.2e} p99 {np.quantile(rel, 0.99):.2e}")
        w = np.argwhere(sel)[np.argmax(rel)]
        assert rel.max() <= 2e-5, (name, f, rel.max(), w.tolist(), margin[tuple(w)], got["W"][tuple(w)], exp["W"][tuple(w)], got["M"][tuple(w)])
        worst = max(worst, float(rel.max()))
        history = got
    print(f"{name}: {compared} pixels compared, {excluded} within {NEAR} of a decision ({excluded / max(1, valid_px):.3%} of valid), "
          f"W rel err max {worst:.2e}, exercised {seen}")
    assert compared > 0.3 * 4 * W * H
    assert excluded < 0.25 * valid_px
    assert seen["emptied"] > 0
    if tr or sr:
        assert seen["zeroed"] > 0
    if vis["final_reuse"]:
        assert seen["reused"] > 0 and seen["expired"] > 0                  # shaded from a reused visibility, and re-traced after MaxAge = 2
    if vis.get("discard_invisible"):
        assert seen["discarded"] > 0
    del r, r2
    g2.close(); ctx2.close(); g.close()
    return edges


@pytest.mark.gpu
@pytest.mark.parametrize("name,temporal,spatial,boiling,vis", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gpu_visibility_pinned_per_pixel(gpu, ptamd, pkg, name, temporal, spatial, boiling, vis):
    """_visibility_pin at 48 x 32"""
    _visibility_pin(gpu, ptamd, pkg, name, temporal, spatial, boiling, vis, 48, 32)


RAGGED_CONFIGS = [c for c in CONFIGS if c[0] in ("initial-spatial-basic", "both-raytraced-boiling", "both-raytraced-reuse")]


@pytest.mark.gpu
@pytest.mark.parametrize("size", dipins.RAGGED, ids=dipins.size_id)
@pytest.mark.parametrize("name,temporal,spatial,boiling,vis", RAGGED_CONFIGS, ids=[c[0] for c in RAGGED_CONFIGS])
def test_gpu_visibility_pinned_per_pixel_ragged(gpu, ptamd, pkg, name, temporal, spatial, boiling, vis, size):
    """_visibility_pin at the sizes that cut every tile of the DI kernels on both axes (tests/dipins.py), for a Basic row, a Raytraced row
    with the boiling filter and a Raytraced row with final-visibility reuse on -- the carried pixel offset of a reused visibility goes
    through `history index % width`, with an odd width here. Same scene, camera path, settings, tolerances and caps; the run must have
    reached the edges."""
    W, H = size
    seen = _visibility_pin(gpu, ptamd, pkg, name, temporal, spatial, boiling, vis, W, H)
    dipins.assert_edge_witnesses(seen, W, H, name, temporal=temporal, spatial=spatial > 0, boiling=temporal and boiling)


@pytest.mark.gpu
def test_gpu_final_visibility_reuse_is_exact_on_a_static_view(ptamd, pkg):
    """a static camera and temporal-only reuse (the history pixel is the pixel itself: d = 0) behind opaque occluders: a reused visibility is
    the one the ray would give, so FinalVisibilityReuse on (MaxAge 4) and off shade bit-identically on each of 5 frames; with it on, from
    frame 2 more than half of the valid reservoirs with W > 0 carry a visibility of age >= 1 (they were shaded without a ray)."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = visscene.pin_scene(S, W / H)
    reuse = L.di_resampling_settings(temporal=True, spatial_samples=0)
    frames = {}
    for on in (True, False):
        ctx = ptamd.DeviceContext(0)
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W, H, with_denoiser_outputs=True, di_history=True)
        frames[on] = []
        for f in range(5):
            r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=300 + f), di_samples=8, di_reuse=reuse,
                     di_visibility=L.di_visibility_settings(final_reuse=on, max_age=4))
            ctx.sync()
            out = ptamd.textures_to_numpy(r.textures)
            frames[on].append((out["Diffuse"].tobytes(), out["Specular"].tobytes(), r.direct_lighting.download_reservoirs(), R.Surfaces(out, scene.camera).valid))
        del r
        g.close(); ctx.close()
    for f in range(5):
        a, b = frames[True][f], frames[False][f]
        assert a[0] == b[0] and a[1] == b[1], f
        assert np.frombuffer(a[0], np.uint16).any()
        for k in ("LightIndex", "U", "V", "W", "M", "Age"):
            assert np.array_equal(a[2][k], b[2][k]), (f, k)
        lit = a[3].reshape(-1) & (a[2]["W"] > 0)
        age_on, age_off = L.di_unpack_visibility(a[2]["Visibility"])[3], L.di_unpack_visibility(b[2]["Visibility"])[3]
        assert (age_off[b[3].reshape(-1) & (b[2]["W"] > 0)] == 0).all()     # off: every shaded reservoir was traced this frame
        share = (age_on[lit] >= 1).mean()
        print(f"frame {f}: {int(lit.sum())} shaded reservoirs, {share:.1%} shaded from a stored visibility, ages up to {int(age_on[lit].max())}")
        assert age_on[lit].max() <= 4
        if f >= 2:
            assert share > 0.5, (f, share)


def _di_sum(r):
    d = r.textures["Diffuse"].detach().cpu().numpy().view(np.float16)[..., :3].astype(np.float64)
    s = r.textures["Specular"].detach().cpu().numpy().view(np.float16)[..., :3].astype(np.float64)
    return d + s


@pytest.mark.gpu
def test_gpu_raytraced_unbiased_where_basic_is_not(gpu, ptamd, pkg):
    """the pin scene's bar over the floor, static view, 64 x 48, no final-visibility reuse. The mask: floor pixels that the bar shadows by 20
    to 80 % (1 - luminance with the bar / without it, 256-frame no-reuse means of each; 355 pixels). Frame 4 of 48 independent sequences
    with initial visibility + temporal and spatial Raytraced: the per-pixel mean is within 4 standard errors (+ 2e-3 relative, fp16 storage)
    of the no-reuse mean on the mask (measured: at most 0.89 of that bound; mask mean 0.0885 against 0.0899). The same with the Raytraced
    flags off (initial visibility + Basic) is darker: its mask-averaged mean lies below the reference by more than 4 of its standard errors
    (measured: 0.0822, 11.8 standard errors below) -- the scene tells the two apart. The no-reuse reference draws 32 candidates per pixel
    (see plain_mean)."""
    S, L = pkg.scenes, pkg.layouts
    W, H, K, F = 64, 48, 48, 4
    gpu.set_sharding(0, 1, 16)
    scene = visscene.pin_scene(S, W / H)
    open_scene = visscene.pin_scene(S, W / H)
    open_scene.instance_masks[2] = 0                                       # the bar hidden
    ctx2 = ptamd.DeviceContext(0)                                          # a context holds one scene
    g, g_open = ptamd.Scene(gpu, scene), ptamd.Scene(ctx2, open_scene)

    def plain_mean(ctx, gs_scene):
        # 32 candidates per pixel: the no-reuse estimator's expectation does not depend on the candidate count, its spread and its tails do,
        # and a reference whose own standard error is underestimated at one pixel fails every estimator there (seen with 4 candidates: the
        # same single pixel 4.4 to 4.8 standard errors off for Raytraced, Basic and the pass without visibility alike)
        plain = ptamd.Renderer(ctx, gs_scene, W, H, with_denoiser_outputs=True)
        acc = []
        for f in range(256):
            plain.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=9000 + f), di_samples=32); ctx.sync()
            acc.append(_di_sum(plain))
        acc = np.stack(acc)
        return acc.mean(0), acc.std(0, ddof=1) / np.sqrt(len(acc)), ptamd.textures_to_numpy(plain.textures)
    ref, ref_se, gb = plain_mean(gpu, g)
    lit, _, gb_open = plain_mean(ctx2, g_open)
    g_open.close(); ctx2.close()
    pos = gb["Position"][..., :3].astype(np.float64)
    floor = np.isfinite(pos).all(-1) & (np.abs(pos[..., 1]) < 1e-3) & np.isfinite(gb_open["Position"][..., :3]).all(-1) & \
        (np.abs(gb_open["Position"][..., 1].astype(np.float64)) < 1e-3)
    with np.errstate(divide="ignore", invalid="ignore"):
        shadowed = 1.0 - (ref @ R.LUMA) / (lit @ R.LUMA)
    mask = floor & (shadowed >= 0.2) & (shadowed <= 0.8)
    print(f"{int(floor.sum())} floor pixels, {int(mask.sum())} shadowed by 20-80 %")
    assert mask.sum() >= 50

    def sequences(raytraced):
        r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True, di_history=True)
        vis = L.di_visibility_settings(initial=True, final_reuse=False, temporal_raytraced=raytraced, spatial_raytraced=raytraced)
        vals = []
        for k in range(K):
            r.direct_lighting.ResetHistory()
            for f in range(F):
                r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=2000 + k * F + f), di_samples=4,
                         di_reuse=L.di_resampling_settings(), di_visibility=vis)
            gpu.sync()
            vals.append(_di_sum(r))
        vals = np.stack(vals)
        return vals.mean(0), vals.std(0, ddof=1) / np.sqrt(K), vals
    mean, se, _ = sequences(True)
    tol = 4 * np.sqrt(se ** 2 + ref_se ** 2) + 2e-3 * ref
    z = np.abs(mean - ref)[mask] / np.maximum(tol[mask], 1e-12)
    print(f"Raytraced: max |mean - reference| / (4 sigma) = {z.max():.2f}; mask mean {mean[mask].mean():.5f} against {ref[mask].mean():.5f}")
    assert (z <= 1).all(), z.max()
    bmean, _, bvals = sequences(False)
    per_seq = bvals[:, mask].mean((1, 2))                                  # the mask average of each sequence: independent draws
    ref_mask = ref[mask].mean()
    b_se = np.sqrt(per_seq.std(ddof=1) ** 2 / K + (ref_se[mask] ** 2).sum() / (3 * mask.sum()) ** 2)
    print(f"Basic: mask mean {per_seq.mean():.5f} against {ref_mask:.5f}: {(ref_mask - per_seq.mean()) / b_se:.1f} standard errors below")
    assert per_seq.mean() < ref_mask - 4 * b_se
    g.close()


@pytest.mark.gpu
def test_gpu_visibility_errors_and_history_reset(ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H, n = 48, 32, 8
    ctx = ptamd.DeviceContext(0)
    scene = visscene.pin_scene(S, W / H)
    g = ptamd.Scene(ctx, scene)
    r = ptamd.Renderer(ctx, g, W, H, with_denoiser_outputs=True, di_history=True)
    di = r.direct_lighting
    base = L.di_visibility_settings()
    for field, value in (("InitialVisibility", 2), ("FinalVisibilityReuse", 2), ("FinalVisibilityMaxAge", 0), ("FinalVisibilityMaxAge", 15),
                         ("FinalVisibilityMaxDistance", 0.0), ("FinalVisibilityMaxDistance", 31.5), ("FinalVisibilityMaxDistance", float("nan")),
                         ("DiscardInvisibleSamples", 7), ("TemporalRaytraced", 2), ("SpatialRaytraced", 3)):
        bad = base.copy(); bad[field] = value
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            di.SetVisibility(bad)
        assert field in str(e.value), (field, str(e.value))
    di.SetVisibility(None); di.SetVisibility(np.zeros((), L.PT_DI_VISIBILITY_SETTINGS)); di.SetVisibility(base)
    # pt_di_set_resampling still refuses Raytraced as a mode of its own
    bad = L.di_resampling_settings(); bad["TemporalBiasCorrection"] = 3
    with pytest.raises(ptamd.PtInvalidArgument) as e:
        di.SetResampling(bad)
    assert "Pairwise and Raytraced" in str(e.value)
    # Raytraced over a pass whose correction is Off: refused at render, the field named; a pass that is off does not mind
    gs = lambda f: S.graphics_settings(W, H, spp=1, bounces=1, frame_index=f)
    off = L.DI_BIAS_CORRECTION_OFF
    for flag, reuse in (("TemporalRaytraced", L.di_resampling_settings(temporal_bias=off)), ("SpatialRaytraced", L.di_resampling_settings(spatial_bias=off))):
        v = L.di_visibility_settings(); v[flag] = 1
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            r.render(gs(0), di_samples=n, di_reuse=reuse, di_visibility=v)
        assert flag in str(e.value) and "BASIC" in str(e.value)
    v = L.di_visibility_settings(spatial_raytraced=True)
    r.render(gs(0), di_samples=n, di_reuse=L.di_resampling_settings(temporal=True, spatial_samples=0, spatial_bias=off), di_visibility=v)
    r.render(gs(0), di_samples=n, di_visibility=v)                          # the plain pass: no reservoir, the setting does nothing
    # a changed value resets the history
    reuse = L.di_resampling_settings(temporal=True, spatial_samples=0, boiling_filter=False)
    for f in range(2):
        r.render(gs(10 + f), di_samples=n, di_reuse=reuse, di_visibility=base)
    ctx.sync()
    res = di.download_reservoirs()
    assert (res["M"] > n).any() and (res["Visibility"] != 0).any()
    r.render(gs(12), di_samples=n, di_reuse=reuse, di_visibility=base); ctx.sync()
    assert (di.download_reservoirs()["M"] > n).any()                      # the same value again: the history stays
    r.render(gs(13), di_samples=n, di_reuse=reuse, di_visibility=L.di_visibility_settings(max_age=5)); ctx.sync()
    res = di.download_reservoirs()
    valid = R.Surfaces(ptamd.textures_to_numpy(r.textures), scene.camera).valid.reshape(-1)
    assert valid.sum() > 0.5 * W * H and (res["M"][valid] == n).all()
    del r
    g.close(); ctx.close()


@pytest.mark.gpu
def test_cpp_host_restir_visibility_matches_python(tmp_path, gpu, ptamd, pkg):
    """pt_demo --di --restir --restir-visibility --restir-raytraced --frames 4: the C++ host's SetVisibility at its defaults with both
    Raytraced flags, bit-identical to the Python sequence; --restir-visibility without --restir is refused"""
    demo = os.path.join(ge.PKG_DIR, "pt_demo")
    S, L = pkg.scenes, pkg.layouts
    W, H, spp, bounces, frames = 96, 64, 1, 2, 4
    out = str(tmp_path / "radiance.bin")
    common = ["--di-samples", "8", "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces), "--frames", str(frames), "--out", out]
    subprocess.check_call([demo, "--di", "--restir", "--restir-visibility", "--restir-raytraced"] + common, timeout=300)
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    refused = subprocess.run([demo, "--di", "--restir-visibility"] + common, capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--restir-visibility needs --restir" in refused.stderr + refused.stdout
    gpu.set_sharding(0, 1, 16)
    ctx = ptamd.DeviceContext(0)
    g = ptamd.Scene(ctx, S.cornell_box(aspect=W / H, variant="ggx"))
    r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True, di_history=True)
    vis = L.di_visibility_settings(temporal_raytraced=True, spatial_raytraced=True)
    for fi in [12345] + list(range(frames - 1, -1, -1)):                    # pt_demo's warm-up frame, then N-1 .. 0
        gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=fi)
        gs["IsDIEnabled"] = 1
        r.render(gs, di_samples=8, di_reuse=L.di_resampling_settings(), di_visibility=vis)
    ctx.sync()
    ref = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    res = r.direct_lighting.download_reservoirs()
    assert (res["M"] > 8).any() and (L.di_unpack_visibility(res["Visibility"])[3] >= 1).any()   # history and stored visibilities were used
    plain = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True, di_history=True)
    for fi in [12345] + list(range(frames - 1, -1, -1)):
        gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=fi)
        gs["IsDIEnabled"] = 1
        plain.render(gs, di_samples=8, di_reuse=L.di_resampling_settings())
    ctx.sync()
    without = ptamd.textures_to_numpy(plain.textures)["RadianceF32"]
    g.close(); ctx.close()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(ref.view(np.uint32), without.view(np.uint32))   # the flags did something
