"""Reservoir reuse pinned per pixel against the float64 restatement (tests/restirref.py), on a moving camera; unbiasedness of the Basic
normalisation against a closed form and the no-reuse pass; a history reset by a hidden emitter instance; pt_demo --restir."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import bsdfref
import dipins
import restirref as R
import visscene

NEAR = 1e-5


CONFIGS = [  # (name, temporal, spatial samples, basic, boiling)
    ("temporal-basic-boiling", True, 0, True, True),
    ("temporal-off", True, 0, False, False),
    ("spatial-basic", False, 1, True, False),
    ("spatial-off", False, 2, False, False),
    ("both-basic-boiling", True, 1, True, True),
    ("both-off", True, 1, False, False),
]


def _reuse_pin(gpu, ptamd, pkg, name, temporal, spatial, basic, boiling, W, H):
    """3 frames of W x H with the camera moving 0.17 per frame (~2 px at 48 x 32). Each frame's final reservoirs match restirref, fed the
    downloaded G-buffers, motion vectors, light records, last frame's final reservoirs and the frame's initial reservoirs: LightIndex, M,
    Age, U, V exactly, W to 2e-5 relative (float32 against float64 p-hat; measured up to 1.3e-5). Pixels within 1e-5 of a decision (a coin,
    a threshold, the boiling cut, the rounding of p + mv, a cosine where the BSDF or p-hat turns ill-conditioned) are left out and counted,
    and so is every pixel that reused such a pixel's reservoir. Returns what the restatement counted on the way (restirref.note).
    Left out, of the valid pixels compared or left out, measured over the six configurations: 48 x 32 0.3 to 1.2 %, 37 x 23 0.6 to 1.8 %,
    21 x 13 0 to 0.2 %. (With the pin scene's roughness tie counted as a decision at risk -- restirref.roughness_margin -- a spatial pass
    left out 22 % at 48 x 32, 44 % at 37 x 23 and 38 % at 21 x 13: every pixel that drew a bar pixel among its eight neighbours.)"""
    S, L = pkg.scenes, pkg.layouts
    n = 8
    seen = {}
    bsdf = bsdfref.Reference()
    table = R.offset_table()
    bias = L.DI_BIAS_CORRECTION_BASIC if basic else L.DI_BIAS_CORRECTION_OFF
    reuse = L.di_resampling_settings(temporal=temporal, spatial_samples=spatial, temporal_bias=bias, spatial_bias=bias, boiling_filter=boiling)
    # the initial reservoirs of each frame come from a second context: temporal-only, Off, no boiling, history reset before every frame
    init = L.di_resampling_settings(temporal=True, spatial_samples=0, temporal_bias=L.DI_BIAS_CORRECTION_OFF, boiling_filter=False)
    gpu.set_sharding(0, 1, 16)
    scene = visscene.pin_scene(S, W / H)
    g = ptamd.Scene(gpu, scene)
    ctx2 = ptamd.DeviceContext(0)
    g2 = ptamd.Scene(ctx2, scene)
    r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True, di_history=True)
    r2 = ptamd.Renderer(ctx2, g2, W, H, with_denoiser_outputs=True, di_history=True)
    cam = scene.camera.copy()
    history, excluded, compared, disoccluded = None, 0, 0, 0
    for f in range(3):
        if f:
            cam = visscene.move(S, cam, cam, 0.17)
        visscene.set_camera(r, cam); visscene.set_camera(r2, cam)
        gs = S.graphics_settings(W, H, spp=1, bounces=1, frame_index=40 + f)
        r.render(gs, di_samples=n, di_reuse=reuse); gpu.sync()
        r2.direct_lighting.ResetHistory()
        r2.render(gs, di_samples=n, di_reuse=init); ctx2.sync()
        out = ptamd.textures_to_numpy(r.textures)
        got = R.as_frame(r.direct_lighting.download_reservoirs(), H, W)
        fresh = R.as_frame(r2.direct_lighting.download_reservoirs(), H, W)
        lights = r.direct_lighting.download_lights()
        cur = R.Surfaces(out, cam)
        mv = out["MotionVector"].view(np.float16).astype(np.float32)
        if temporal:
            prev = R.Surfaces(out, cam, previous=True) if f else None
            exp, margin = R.temporal_pass(cur, prev, mv, fresh, history if f else None, lights, 40 + f, bsdf, 20, basic, boiling, 0.2, stats=seen)
            if f:
                disoccluded += int((cur.valid & (exp["M"] == n)).sum())
        else:
            exp = fresh
            exp["Age"][:] = 0
            margin = np.full((H, W), np.inf)
        if spatial:
            exp, margin = R.spatial_pass(cur, exp, margin, lights, table, 40 + f, bsdf, spatial, 8, 20, 32.0, basic, stats=seen)
        sel = cur.valid & (margin >= NEAR)
        excluded += int((cur.valid & (margin < NEAR)).sum()); compared += int(sel.sum())
        for k in ("LightIndex", "M", "Age"):
            bad = sel & (got[k] != exp[k])
            assert not bad.any(), (name, f, k, np.argwhere(bad)[:5].tolist(), got[k][bad][:5], exp[k][bad][:5], margin[bad][:5],
                                   got["LightIndex"][bad][:5], exp["LightIndex"][bad][:5], got["W"][bad][:5], exp["W"][bad][:5])
        for k in ("U", "V"):
            assert np.array_equal(got[k][sel].astype(np.float32), exp[k][sel].astype(np.float32)), (name, f, k)
        rel = np.abs(got["W"][sel] - exp["W"][sel]) / np.maximum(np.abs(exp["W"][sel]), 1e-30)
        rel = np.where((got["W"][sel] == 0) & (exp["W"][sel] == 0), 0.0, rel)
        print(f"{name} frame {f}: W rel err max {rel.max():.2e} p99 {np.quantile(rel, 0.99):.2e}")
        worst = np.argwhere(sel)[np.argmax(rel)]
        assert rel.max() <= 2e-5, (name, f, rel.max(), worst.tolist(), margin[tuple(worst)], got["W"][tuple(worst)], exp["W"][tuple(worst)],
                                   got["M"][tuple(worst)])
        history = got
    print(f"{name}: {compared} pixels compared, {excluded} within {NEAR} of a decision ({excluded / max(1, compared + excluded):.3%}), "
          f"{disoccluded} without history after motion")
    assert compared > 0.3 * 3 * W * H
    # the exclusion spreads: a spatial pixel that reused any uncertain neighbour (8 disocclusion-boost samples each) is left out too,
    # and pixels on the emitters themselves see samples of their own triangle edge-on. Measured: the docstring has the shares.
    assert excluded < 0.25 * (compared + excluded)
    if temporal:
        assert disoccluded > 0                                           # the motion disoccluded pixels
    del r, r2
    g2.close(); ctx2.close(); g.close()
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("name,temporal,spatial,basic,boiling", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gpu_reuse_pinned_per_pixel(gpu, ptamd, pkg, name, temporal, spatial, basic, boiling):
    """_reuse_pin at 48 x 32"""
    _reuse_pin(gpu, ptamd, pkg, name, temporal, spatial, basic, boiling, 48, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", dipins.RAGGED, ids=dipins.size_id)
@pytest.mark.parametrize("name,temporal,spatial,basic,boiling", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gpu_reuse_pinned_per_pixel_ragged(gpu, ptamd, pkg, name, temporal, spatial, basic, boiling, size):
    """_reuse_pin at the sizes that cut the 16 x 16 block and the boiling filter's 8 x 8 tile on both axes, with an odd width behind
    every pixel index: same scene, camera path, settings, tolerances and caps. The run must have reached the edges
    (dipins.assert_edge_witnesses)."""
    W, H = size
    seen = _reuse_pin(gpu, ptamd, pkg, name, temporal, spatial, basic, boiling, W, H)
    dipins.assert_edge_witnesses(seen, W, H, name, temporal=temporal, spatial=spatial > 0, boiling=temporal and boiling)


def _floor_mask(gb):
    pos = gb["Position"][..., :3].astype(np.float64)
    return np.isfinite(pos).all(-1) & (np.abs(pos[..., 1] + 1) < 1e-4) & (pos[..., 0] > -0.55) & (pos[..., 0] < -0.15) & \
        (pos[..., 2] > -0.6) & (pos[..., 2] < -0.45), pos


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["diffuse", "ggx"])
def test_gpu_basic_reuse_unbiased(gpu, ptamd, pkg, variant):
    """Temporal + spatial reuse with Basic bias correction is unbiased on the unoccluded floor of the Cornell box: frame 4 of 48
    independent sequences (history reset between them) against the polygon form-factor closed form (Lambertian) or the no-reuse pass's
    256-frame mean (GGX), within 4 standard errors of the measured spread."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 48
    ext = L.EXT_LAMBERTIAN_ONLY if variant == "diffuse" else 0
    scene = S.cornell_box(aspect=W / H, variant=variant)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True, di_history=True)
    K, F = 48, 4
    vals = []
    for k in range(K):
        r.direct_lighting.ResetHistory()
        for f in range(F):
            r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=2000 + k * F + f, ext_flags=ext), di_samples=4,
                     di_reuse=L.di_resampling_settings())
        gpu.sync()
        o = ptamd.textures_to_numpy(r.textures)
        vals.append(o["Diffuse"][..., :3].view(np.float16).astype(np.float64) + o["Specular"][..., :3].view(np.float16).astype(np.float64))
    vals = np.stack(vals)
    floor, pos = _floor_mask(o)
    assert floor.sum() >= 3
    if variant == "diffuse":
        M = scene.instance_data["ObjectToWorld"][5].reshape(3, 4).astype(np.float64)
        light = scene.nodes[scene.objects[5].node].meshes[0].vertices["Position"].astype(np.float64) @ M[:, :3].T + M[:, 3]
        albedo = o["BaseColorMetalness"][..., :3].astype(np.float64) / 255.0
        expect = np.zeros_like(vals[0]); ref_se = np.zeros_like(vals[0])
        for y, x in zip(*np.nonzero(floor)):
            ff = 0.0
            for e in range(4):
                a, b = light[e] - pos[y, x], light[(e + 1) % 4] - pos[y, x]
                a /= np.linalg.norm(a); b /= np.linalg.norm(b)
                c = np.cross(a, b)
                ff += np.arccos(np.clip(a @ b, -1, 1)) * (c / np.linalg.norm(c)) @ np.array([0, 1.0, 0])
            expect[y, x] = albedo[y, x] / np.pi * 15.0 * abs(ff) / 2
    else:
        plain = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True)
        ref = []
        for f in range(256):
            plain.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=9000 + f), di_samples=4); gpu.sync()
            p = ptamd.textures_to_numpy(plain.textures)
            ref.append(p["Diffuse"][..., :3].view(np.float16).astype(np.float64) + p["Specular"][..., :3].view(np.float16).astype(np.float64))
        ref = np.stack(ref)
        expect, ref_se = ref.mean(0), ref.std(0, ddof=1) / np.sqrt(len(ref))
    mean, se = vals.mean(0), vals.std(0, ddof=1) / np.sqrt(K)
    tol = 4 * np.sqrt(se ** 2 + ref_se ** 2) + 2e-3 * expect                  # + fp16 storage
    z = np.abs(mean - expect)[floor] / np.maximum(tol[floor], 1e-12)
    print(f"{variant}: {floor.sum()} floor pixels, max |mean - expected| / (4 sigma) = {z.max():.2f}")
    assert (z <= 1).all(), z.max()
    g.close()


@pytest.mark.gpu
def test_gpu_hidden_emitter_resets_history(gpu, ptamd, pkg):
    """hiding an emitter instance rebuilds the light list (the top level's instance hash): the next temporal frame has no history"""
    S, L = pkg.scenes, pkg.layouts
    W, H, n = 48, 32, 8
    scene = visscene.pin_scene(S, W / H)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True, di_history=True)
    reuse = L.di_resampling_settings(temporal=True, spatial_samples=0, boiling_filter=False)
    for f in range(2):
        r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=f), di_samples=n, di_reuse=reuse)
    gpu.sync()
    res = r.direct_lighting.download_reservoirs()
    assert (res["M"] > n).any() and r.direct_lighting.light_count() == 5
    scene.instance_masks[3] = 0                                            # the second emitter instance
    g._descs = None
    g._build_top_level()
    r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=2), di_samples=n, di_reuse=reuse); gpu.sync()
    assert r.direct_lighting.light_count() == 3
    out = ptamd.textures_to_numpy(r.textures)
    res = r.direct_lighting.download_reservoirs()
    valid = R.Surfaces(out, scene.camera).valid.reshape(-1)
    assert valid.sum() > 0.5 * W * H
    assert (res["M"][valid] == n).all() and (res["Age"] == 0).all()
    assert (res["LightIndex"][res["LightIndex"] != 0xFFFFFFFF] < 3).all()
    g.close()


@pytest.mark.gpu
def test_cpp_host_restir_matches_python(tmp_path, gpu, ptamd, pkg):
    """pt_demo --di --restir --frames 4: the C++ host's DirectLighting with reuse and the Previous* swap, bit-identical to Python"""
    demo = os.path.join(ge.PKG_DIR, "pt_demo")
    S, L = pkg.scenes, pkg.layouts
    W, H, spp, bounces, frames = 96, 64, 1, 2, 4
    out = str(tmp_path / "radiance.bin")
    subprocess.check_call([demo, "--di", "--restir", "--di-samples", "8", "--width", str(W), "--height", str(H), "--spp", str(spp),
                           "--bounces", str(bounces), "--frames", str(frames), "--out", out], timeout=300)
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    gpu.set_sharding(0, 1, 16)
    ctx = ptamd.DeviceContext(0)
    g = ptamd.Scene(ctx, S.cornell_box(aspect=W / H, variant="ggx"))
    r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True, di_history=True)
    for fi in [12345] + list(range(frames - 1, -1, -1)):                    # pt_demo's warm-up frame, then N-1 .. 0
        gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=fi)
        gs["IsDIEnabled"] = 1
        r.render(gs, di_samples=8, di_reuse=L.di_resampling_settings())
    ctx.sync()
    ref = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    assert (r.direct_lighting.download_reservoirs()["M"] > 8).any()        # the history was used
    g.close(); ctx.close()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
