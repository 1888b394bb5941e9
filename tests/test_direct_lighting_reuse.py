"""Reservoir reuse of the DI pass (pt_di_set_resampling, pt_di_render_with_history): the default path is unchanged, the history
lifecycle, the error paths, determinism, and that temporal + spatial reuse lowers the error of a many-light scene."""
import numpy as np
import pytest

import restirref as R


def _valid(out):
    depth = out["LinearDepth"][..., 0]
    rough = np.maximum(out["NormalRoughness"][..., 3].astype(np.float64) / 32767.0, -1.0)
    return np.isfinite(depth) & (rough >= 0.05)


def _many_lights_scene(S, aspect, n=256):
    """a diffuse floor under n small emissive triangles of one material whose areas (hence powers) span 100x"""
    floor = S.quad_mesh((-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3), (0, 1, 0), S.material((0.7, 0.7, 0.7), roughness=0.6))
    rng = np.random.default_rng(5)
    pos, k = [], int(np.sqrt(n))
    for i in range(n):
        cx, cz = -2.4 + 4.8 * (i % k) / (k - 1), -2.4 + 4.8 * (i // k) / (k - 1)
        s = 0.02 * np.sqrt(10.0 ** (2.0 * rng.random()))                  # area ~ s^2: 100x span
        y = 1.2 + 0.3 * rng.random()
        pos += [(cx - s, y, cz - s), (cx + s, y, cz - s), (cx, y, cz + s)]
    pos = np.array(pos, np.float32)
    tris = S.Mesh(S.make_vertices(pos, np.tile(np.float32([0, -1, 0]), (len(pos), 1))), S.make_indices(list(range(len(pos)))), True,
                  S.material((0.5, 0.5, 0.5), emissive=(1.0, 0.9, 0.8), strength=40.0))
    nodes = [S.MeshNode([floor]), S.MeshNode([tris])]
    objects = [S.RenderObject(0, S.trs()), S.RenderObject(1, S.trs())]
    cam = S.make_camera((0, 2.5, -3.2), forward=(0, -0.7, 1), hfov_deg=70.0, aspect=aspect)
    return S.Scene(nodes, objects, cam, S.make_scene_data((0, 0, 0, 1)), name="many_lights").finalize()


def _direct(out):
    d = out["Diffuse"][..., :3].view(np.float16).astype(np.float64) + out["Specular"][..., :3].view(np.float16).astype(np.float64)
    return d @ R.LUMA


def _seq(ptamd, S, L, ctx, g, W, H, frames, reuse, samples=8, first=0, r=None):
    r = r or ptamd.Renderer(ctx, g, W, H, with_denoiser_outputs=True, di_history=True)
    outs, res = [], []
    for f in range(frames):
        r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=first + f), di_samples=samples, di_reuse=reuse)
        ctx.sync()
        outs.append(ptamd.textures_to_numpy(r.textures))
        res.append(r.direct_lighting.download_reservoirs())
    return r, outs, res


@pytest.mark.gpu
def test_gpu_default_path_unchanged(gpu, ptamd, pkg):
    """resampling never set, set to None, or set with both passes off: the plain pass, bit for bit (Diffuse / Specular and Radiance)"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 48
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W / H, variant="ggx"))
    for bounces in (1, 0):
        gs = S.graphics_settings(W, H, spp=1, bounces=bounces, frame_index=3)
        plain = ptamd.Renderer(gpu, g, W, H, with_f32=True, with_denoiser_outputs=True)
        plain.render(gs, di_samples=8); gpu.sync()
        ref = ptamd.textures_to_numpy(plain.textures)
        hist = ptamd.Renderer(gpu, g, W, H, with_f32=True, with_denoiser_outputs=True, di_history=True)
        for reuse in (None, L.di_resampling_settings(temporal=False, spatial_samples=0)):
            for _ in range(2):
                hist.render(gs, di_samples=8, di_reuse=reuse); gpu.sync()
                got = ptamd.textures_to_numpy(hist.textures)
                for k in ("Diffuse", "Specular", "Radiance", "RadianceF32"):
                    assert np.array_equal(got[k], ref[k]), (bounces, k)
                assert len(hist.direct_lighting.download_reservoirs()) == 0
        assert (ref["Diffuse"][..., :3] != 0).any() or (ref["Radiance"] != 0).any()
    g.close()


@pytest.mark.gpu
def test_gpu_history_lifecycle(gpu, ptamd, pkg):
    """After the first render, pt_di_reset_history, a settings change, a size change or a rebuilt light list, a temporal-only frame
    finds no history: M == LocalLightSamples at every valid pixel and the samples are the plain pass's."""
    S, L = pkg.scenes, pkg.layouts
    W, H, n = 64, 48, 8
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    reuse = L.di_resampling_settings(temporal=True, spatial_samples=0, boiling_filter=False)

    def fresh(out, res, frame, r):
        v = _valid(out).reshape(-1)
        assert v.sum() > 0.5 * W * H
        assert (res["M"][v] == n).all() and (res["M"][~v] == 0).all()
        assert (res["Age"] == 0).all()
        # the plain pass of the same frame: the same samples, so the same fp16 outputs within one code (W's normalisation rounds
        # differently: Σw·p / (p·M·p) against Σw / M / p)
        p = ptamd.Renderer(gpu, g, r.width, r.height, with_denoiser_outputs=True)
        p.render(S.graphics_settings(r.width, r.height, spp=1, bounces=1, frame_index=frame), di_samples=n); gpu.sync()
        a = ptamd.textures_to_numpy(p.textures)
        for k in ("Diffuse", "Specular"):
            d = np.abs(a[k][..., :3].astype(np.int32) - out[k][..., :3].astype(np.int32))
            assert d.max() <= 1, (k, d.max())
            assert np.array_equal(a[k][..., 3], out[k][..., 3]), k          # the light distance: the same sample point
        return True

    r, outs, res = _seq(ptamd, S, L, gpu, g, W, H, 2, reuse, samples=n)
    assert fresh(outs[0], res[0], 0, r)
    v = _valid(outs[1]).reshape(-1)
    assert (res[1]["M"][v] > n).mean() > 0.9                                   # the static second frame reuses its history
    assert (res[1]["Age"][v] > 0).any()
    r.direct_lighting.ResetHistory()
    _, o2, r2 = _seq(ptamd, S, L, gpu, g, W, H, 1, reuse, samples=n, first=2, r=r)
    assert fresh(o2[0], r2[0], 2, r)
    # a settings change
    _seq(ptamd, S, L, gpu, g, W, H, 1, reuse, samples=n, first=3, r=r)
    reuse2 = reuse.copy(); reuse2["MaxHistoryLength"] = 10
    _, o3, r3 = _seq(ptamd, S, L, gpu, g, W, H, 1, reuse2, samples=n, first=4, r=r)
    assert fresh(o3[0], r3[0], 4, r)
    # a size change (the same context, another renderer)
    r4, o4, r4s = _seq(ptamd, S, L, gpu, g, 48, 40, 1, reuse2, samples=n, first=5)
    assert fresh(o4[0], r4s[0], 5, r4)
    # a rebuilt light list (pt_invalidate_object_data: the light list is listed again, its indices may move)
    _seq(ptamd, S, L, gpu, g, W, H, 1, reuse2, samples=n, first=6, r=r)
    gpu.invalidate_object_data()
    _, o5, r5 = _seq(ptamd, S, L, gpu, g, W, H, 1, reuse2, samples=n, first=7, r=r)
    assert r.direct_lighting.light_count() == 2
    assert fresh(o5[0], r5[0], 7, r)
    g.close()


@pytest.mark.gpu
def test_gpu_errors_and_determinism(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    ctx = ptamd.DeviceContext(0)
    g = ptamd.Scene(ctx, S.cornell_box(aspect=W / H))
    di = ptamd.DirectLighting(ctx)
    base = L.di_resampling_settings()
    for field, value in (("TemporalBiasCorrection", 2), ("SpatialBiasCorrection", 3)):
        bad = base.copy(); bad[field] = value
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            di.SetResampling(bad)
        assert "Pairwise" in str(e.value)
    for field, value, word in (("MaxHistoryLength", 0, "MaxHistoryLength"), ("MaxHistoryLength", 65, "MaxHistoryLength"),
                               ("SpatialSamples", 33, "SpatialSamples"), ("DisocclusionBoostSamples", 33, "DisocclusionBoostSamples"),
                               ("SpatialSamplingRadius", 0.0, "SpatialSamplingRadius"), ("SpatialSamplingRadius", 65.0, "SpatialSamplingRadius"),
                               ("BoilingFilterStrength", 1.5, "BoilingFilterStrength"), ("TemporalResampling", 2, "TemporalResampling")):
        bad = base.copy(); bad[field] = value
        with pytest.raises(ptamd.PtInvalidArgument) as e:
            di.SetResampling(bad)
        assert word in str(e.value), (field, str(e.value))
    # temporal reuse without the previous textures
    r = ptamd.Renderer(ctx, g, W, H, with_denoiser_outputs=True)
    with pytest.raises(ptamd.PtInvalidArgument) as e:
        r.render(S.graphics_settings(W, H, spp=1, bounces=1), di_samples=8, di_reuse=base)
    assert "Previous" in str(e.value)
    # a sharded context
    ctx.set_sharding(0, 2, 8)
    rs = ptamd.Renderer(ctx, g, W, H, with_denoiser_outputs=True, di_history=True)
    with pytest.raises(ptamd.PtInvalidArgument) as e:
        rs.render(S.graphics_settings(W, H, spp=1, bounces=1), di_samples=8, di_reuse=base)
    assert "unsharded" in str(e.value)
    ctx.set_sharding(0, 1, 16)
    del rs, r
    # two runs of the same sequence, each in a fresh context: bit-identical outputs and reservoirs
    runs = []
    for _ in range(2):
        c = ptamd.DeviceContext(0)
        gg = ptamd.Scene(c, S.cornell_box(aspect=W / H, variant="ggx"))
        _, outs, res = _seq(ptamd, S, L, c, gg, W, H, 3, base)
        runs.append((outs, res))
        gg.close(); c.close()
    for f in range(3):
        for k in ("Diffuse", "Specular"):
            assert np.array_equal(runs[0][0][f][k], runs[1][0][f][k]), (f, k)
        assert runs[0][1][f].tobytes() == runs[1][1][f].tobytes(), f
    g.close(); ctx.close()


@pytest.mark.gpu
def test_gpu_reuse_lowers_error(gpu, ptamd, pkg):
    """256 small emitters (powers over 100x), 4 candidates per pixel, a static view: frame 8 of temporal + spatial reuse (Basic) has at
    least 2x lower MSE against a converged no-reuse reference than the plain pass of the same frame."""
    S, L = pkg.scenes, pkg.layouts
    W, H, n = 64, 64, 4
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, _many_lights_scene(S, W / H))
    plain = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True)
    acc, F = 0.0, 128
    for f in range(F):
        plain.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=10000 + f), di_samples=32); gpu.sync()
        acc = acc + _direct(ptamd.textures_to_numpy(plain.textures))
    ref = acc / F
    mse_plain, mse_reuse = [], []
    for seq in range(4):
        first = 100 * seq
        _, outs, res = _seq(ptamd, S, L, gpu, g, W, H, 8, L.di_resampling_settings(), samples=n, first=first)
        valid = _valid(outs[-1])
        plain.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=first + 7), di_samples=n); gpu.sync()
        p = _direct(ptamd.textures_to_numpy(plain.textures))
        mse_plain.append(np.mean((p - ref)[valid] ** 2)); mse_reuse.append(np.mean((_direct(outs[-1]) - ref)[valid] ** 2))
    ratio = np.mean(mse_plain) / np.mean(mse_reuse)
    print(f"reuse MSE ratio (no reuse / temporal + spatial) at frame 8: {ratio:.2f}")
    assert ratio >= 2.0, ratio
    # and not biased: the mean over the frame agrees with the reference within 5 %
    assert abs(np.mean(_direct(outs[-1])[valid]) / np.mean(ref[valid]) - 1) < 0.05
    g.close()
