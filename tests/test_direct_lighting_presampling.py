"""Local-light sampling on the GPU (pt_di_set_light_sampling): the Power_RIS tiles and ReGIR cells pinned against tests/presamplingref.py,
the initial reservoirs of every mode pinned per pixel, unbiasedness against the power CDF, ReGIR's variance, the default path, the
lifecycle, sharding, the error paths and pt_demo --light-sampling."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import bsdfref
import dipins
import presamplingref as P
import restirref as R

MODES = ["uniform", "power_ris", "regir"]
NEAR = 1e-5


def _ls(L, mode):
    return None if mode is None else L.di_light_sampling_settings(mode)


def _renderer(ptamd, ctx, g, W, H, history=False):
    return ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True, di_history=history)


def _frame(S, r, W, H, frame, ls, samples=8, reuse=None, bounces=0):
    """Bounces 0: DI is the last render pass and its estimate is added to Radiance; Bounces 1: it writes Diffuse / Specular, which the
    path tracer consumes"""
    gs = S.graphics_settings(W, H, spp=1, bounces=bounces, frame_index=frame)
    gs["IsDIEnabled"] = 1
    r.render(gs, di_samples=samples, di_reuse=reuse, di_light_sampling=ls)
    r.ctx.sync()


def _lum(r, ptamd):
    return ptamd.textures_to_numpy(r.textures)["RadianceF32"][..., :3].astype(np.float64) @ R.LUMA


@pytest.mark.gpu
def test_gpu_presampled_tiles_and_cells_pinned(gpu, ptamd, pkg):
    """Power_RIS tiles: LightIndex exact, InvSourcePdf within 1 ulp. ReGIR cells (48 cells around the camera, 24 k slots) restated in
    float32 in the kernel's order: LightIndex exact and the weight within 2e-5 relative on all but a measured fraction of slots."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 32, 24
    gpu.set_sharding(0, 1, 16)
    scene = S.emitter_field(16, aspect=W / H)
    g = ptamd.Scene(gpu, scene)
    r = _renderer(ptamd, gpu, g, W, H)
    _frame(S, r, W, H, 21, L.di_light_sampling_settings("regir", cell_size=0.7, build_samples=6))
    lights = r.direct_lighting.download_lights()
    tiles = r.direct_lighting.download_presampled(0)
    cells = r.direct_lighting.download_presampled(1)
    assert len(tiles) == 128 * 1024 and len(cells) == 4096 * 512
    li, inv = P.presample_tiles(lights["Power"], 21)
    assert np.array_equal(tiles["LightIndex"].astype(np.int64), li)
    ulp = np.abs(tiles["InvSourcePdf"].view(np.int32).astype(np.int64) - inv.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, ulp.max()
    centre = scene.camera["Position"].astype(np.float32)
    sel = np.array([(z * 16 + y) * 16 + x for z in (6, 8, 10, 12) for y in (4, 8, 11, 12) for x in (5, 8, 11)])
    exp_li, exp_w = P.regir_build(lights, tiles["LightIndex"].astype(np.int64).astype(np.int64), tiles["InvSourcePdf"], sel, centre, 0.7, 6, 21)
    got = cells.reshape(4096, 512)[sel]
    got_li = np.where(got["LightIndex"] == 0xFFFFFFFF, -1, got["LightIndex"].astype(np.int64))
    same = got_li == exp_li
    rel = np.abs(got["InvSourcePdf"].astype(np.float64) - exp_w) / np.maximum(np.abs(exp_w), 1e-30)
    rel = np.where((exp_w == 0) & (got["InvSourcePdf"] == 0), 0.0, rel)
    print(f"ReGIR cells: {same.mean():.6f} of slots with the same light, weight rel err max {rel[same].max():.2e}; "
          f"{(exp_li >= 0).mean():.3f} of slots filled")
    assert (exp_li >= 0).mean() > 0.2 and (exp_li < 0).any()           # cells above the emitters are culled
    assert same.mean() >= 0.999
    assert rel[same].max() <= 2e-5
    g.close()


def _pin_initial(ptamd, S, L, gpu, scene, mode, W, H, frame, n=8):
    g = ptamd.Scene(gpu, scene)
    r = _renderer(ptamd, gpu, g, W, H, history=True)
    init = L.di_resampling_settings(temporal=True, spatial_samples=0, temporal_bias=L.DI_BIAS_CORRECTION_OFF, boiling_filter=False)
    r.direct_lighting.ResetHistory()
    _frame(S, r, W, H, frame, _ls(L, mode), samples=n, reuse=init)
    out = ptamd.textures_to_numpy(r.textures)
    got = r.direct_lighting.download_reservoirs().reshape(H, W)
    lights = r.direct_lighting.download_lights()
    tiles = r.direct_lighting.download_presampled(0)
    cells = r.direct_lighting.download_presampled(1)
    g.close()
    return out, got, lights, tiles, cells


def _initial_pin(gpu, ptamd, pkg, mode, W, H):
    """Temporal on, Off, no boiling, frame 0 after a reset: the reservoirs are the initial ones. LightIndex, M, U, V exact, W within 2e-5
    (float32 against float64 p-hat); pixels within 1e-5 of a coin or an ill-conditioned cosine are left out and counted. Returns the
    compared pixels of the screen tiles that the frame's right or bottom edge cuts: how many there were, and how many of them drew their
    candidates from their screen tile's light tile (Power_RIS: all of them; ReGIR: those outside the grid, its fallback). Left out,
    measured: none of the 814 valid pixels at 37 x 23 and none of the 252 at 21 x 13, in any mode; there 334 and 252 compared pixels lie in
    cut screen tiles, of which ReGIR's fallback serves 11 and 21."""
    S, L = pkg.scenes, pkg.layouts
    n, frame = 8, 3
    cut_x, cut_y = (W // P.SCREEN_TILE if W % P.SCREEN_TILE else -1), (H // P.SCREEN_TILE if H % P.SCREEN_TILE else -1)
    in_cut = from_tile = 0
    gpu.set_sharding(0, 1, 16)
    scene = S.emitter_field(64, aspect=W / H)
    out, got, lights, tiles, cells = _pin_initial(ptamd, S, L, gpu, scene, mode, W, H, frame, n)
    bsdf = bsdfref.Reference()
    cur = R.Surfaces(out, scene.camera)
    tl = tiles["LightIndex"].astype(np.int64); tl[tiles["LightIndex"] == 0xFFFFFFFF] = -1
    cl = cells["LightIndex"].astype(np.int64) if len(cells) else None
    if cl is not None:
        cl[cells["LightIndex"] == 0xFFFFFFFF] = -1
    centre = scene.camera["Position"].astype(np.float32)
    compared = excluded = fallback = 0
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x]:
                continue
            Pw = cur.P[y, x].astype(np.float32)
            c = P.candidates(mode, x, y, frame, n, Pw, len(lights), tl, tiles["InvSourcePdf"], cl,
                             cells["InvSourcePdf"] if len(cells) else None, centre, 1.0)
            li, U, V, Wt, M, margin = P.initial_reservoir(cur, (y, x), c, lights, bsdf, n)
            tile = mode == "power_ris"
            if mode == "regir":
                st = P.rng_states(np.uint64(x), np.uint64(y), frame, R.SALT_INITIAL)
                j = []
                for _ in range(3):
                    st, rr = P.rng_next(st); j.append(rr)
                tile = bool(P.regir_cell(Pw, np.array(j, np.float32), centre, 1.0) < 0)
                fallback += int(tile)
            if margin < NEAR:
                excluded += 1
                continue
            compared += 1
            if x // P.SCREEN_TILE == cut_x or y // P.SCREEN_TILE == cut_y:
                in_cut += 1; from_tile += int(tile)
            gr = got[y, x]
            gli = -1 if gr["LightIndex"] == 0xFFFFFFFF else int(gr["LightIndex"])
            assert (gli, int(gr["M"])) == (li, M), (mode, x, y, gli, li, int(gr["M"]))
            if li >= 0:
                assert np.float32(gr["U"]) == np.float32(U) and np.float32(gr["V"]) == np.float32(V), (mode, x, y)
                assert abs(float(gr["W"]) - Wt) <= 2e-5 * Wt, (mode, x, y, float(gr["W"]), Wt)
            else:
                assert float(gr["W"]) == 0.0
    print(f"{mode} at {W} x {H}: {compared} pixels compared, {excluded} within {NEAR} of a decision ({excluded / max(1, compared + excluded):.3%}), "
          f"{fallback} ReGIR fallbacks; in cut screen tiles {in_cut} compared, {from_tile} of them drawing from the light tile")
    assert compared > 0.5 * W * H and excluded < 0.05 * (compared + excluded)
    return in_cut, from_tile


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_initial_reservoirs_pinned(gpu, ptamd, pkg, mode):
    """_initial_pin at 40 x 24"""
    _initial_pin(gpu, ptamd, pkg, mode, 40, 24)


@pytest.mark.gpu
@pytest.mark.parametrize("size", dipins.RAGGED, ids=dipins.size_id)
@pytest.mark.parametrize("mode", MODES)
def test_gpu_initial_reservoirs_pinned_ragged(gpu, ptamd, pkg, mode, size):
    """_initial_pin at the sizes that cut the 16-pixel screen tile on both axes (37 wide: the last tile is 5 pixels wide; 23 and 13 high:
    7 and 13 rows in the last one), the 16 x 16 block and the 8 x 8 wave tile: same scene, settings, tolerances and caps. Pixels of the cut
    screen tiles must be among the compared ones, and under Power_RIS every one of them draws from its tile's light tile."""
    W, H = size
    in_cut, from_tile = _initial_pin(gpu, ptamd, pkg, mode, W, H)
    assert in_cut > 0
    if mode == "power_ris":
        assert from_tile == in_cut


def _means(ptamd, S, L, ctx, g, W, H, mode, frames, base, samples=8, reuse=None):
    r = _renderer(ptamd, ctx, g, W, H, history=reuse is not None)
    v = []
    for f in range(frames):
        _frame(S, r, W, H, base + f, _ls(L, mode), samples=samples, reuse=reuse)
        v.append(_lum(r, ptamd))
    return np.stack(v)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES + ["regir-reuse"])
def test_gpu_unbiased_against_the_power_cdf(gpu, ptamd, pkg, mode):
    """emitter_field(64) (8 k lights, the floor sees them all unoccluded): the per-pixel mean over K frames matches the power-CDF mean
    within a bound from the measured per-pixel variance; ReGIR with temporal + spatial reuse (Basic) too."""
    S, L = pkg.scenes, pkg.layouts
    W, H, K = 48, 32, 48
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.emitter_field(64, aspect=W / H))
    ref = _means(ptamd, S, L, gpu, g, W, H, None, K, 1000)
    if mode == "regir-reuse":
        got = _means(ptamd, S, L, gpu, g, W, H, "regir", K, 2000, reuse=L.di_resampling_settings())
    else:
        got = _means(ptamd, S, L, gpu, g, W, H, mode, K, 2000)
    g.close()
    sel = (ref.mean(0) > 0) & (got.mean(0) > 0)
    assert sel.sum() > 0.5 * W * H
    se = np.sqrt(ref.var(0, ddof=1) / K + got.var(0, ddof=1) / K)[sel]
    d = (got.mean(0) - ref.mean(0))[sel]
    if mode == "regir-reuse":
        se = se * 3.0                  # temporal reuse correlates consecutive frames: the per-frame variance understates the error of the mean
    z = np.abs(d) / np.maximum(se, 1e-30)
    rel = d.mean() / ref.mean(0)[sel].mean()
    print(f"{mode}: {np.mean(z > 4):.4f} of pixels beyond 4 standard errors, image-mean difference {rel:+.4f}")
    assert np.mean(z > 4) < 0.02
    assert abs(rel) < 0.02


@pytest.mark.gpu
def test_gpu_regir_lowers_the_error(gpu, ptamd, pkg):
    """8 candidates on emitter_field(64): ReGIR's per-pixel MSE against a 32-candidate x 48-frame power-CDF reference is below the
    power CDF's. Measured on an MI355X: ratio 0.398; the threshold keeps a margin."""
    S, L = pkg.scenes, pkg.layouts
    W, H, K = 48, 32, 24
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.emitter_field(64, aspect=W / H))
    ref = _means(ptamd, S, L, gpu, g, W, H, None, 48, 5000, samples=32).mean(0)
    cdf = _means(ptamd, S, L, gpu, g, W, H, None, K, 7000)
    regir = _means(ptamd, S, L, gpu, g, W, H, "regir", K, 7000)
    g.close()
    sel = ref > 0
    mse_cdf = ((cdf - ref) ** 2)[:, sel].mean()
    mse_regir = ((regir - ref) ** 2)[:, sel].mean()
    print(f"MSE ratio ReGIR / power CDF: {mse_regir / mse_cdf:.3f}")
    assert mse_regir < 0.6 * mse_cdf


@pytest.mark.gpu
def test_gpu_default_path_and_lifecycle(gpu, ptamd, pkg):
    """ReGIR then NULL: bit-identical to a context that never set it. A changed setting resets the history. Each viewer of a shared scene
    presamples its own buffers. (Bounces 1: the DI outputs are the Diffuse / Specular textures, cleared by every render.)"""
    S, L = pkg.scenes, pkg.layouts
    keys = ("Diffuse", "Specular", "RadianceF32")
    W, H = 48, 32
    scene = S.emitter_field(32, aspect=W / H)
    gpu.set_sharding(0, 1, 16)
    a = ptamd.DeviceContext(0)
    ga = ptamd.Scene(a, scene)
    ra = _renderer(ptamd, a, ga, W, H)
    _frame(S, ra, W, H, 5, L.di_light_sampling_settings("regir"), bounces=1)
    assert len(ra.direct_lighting.download_presampled(1)) == 4096 * 512
    _frame(S, ra, W, H, 6, None, bounces=1)
    assert len(ra.direct_lighting.download_presampled(0)) == 0 and len(ra.direct_lighting.download_presampled(1)) == 0
    oa = ptamd.textures_to_numpy(ra.textures)
    gb = ptamd.Scene(gpu, scene)
    rb = _renderer(ptamd, gpu, gb, W, H)
    _frame(S, rb, W, H, 6, None, bounces=1)
    ob = ptamd.textures_to_numpy(rb.textures)
    for k in keys:
        assert np.array_equal(oa[k], ob[k]), k
    assert (oa["Diffuse"][..., :3] != 0).any()
    # history: two reuse frames build it up; a changed light-sampling setting resets it
    rh = _renderer(ptamd, gpu, gb, W, H, history=True)
    reuse = L.di_resampling_settings(temporal=True, spatial_samples=0, boiling_filter=False)
    _frame(S, rh, W, H, 1, L.di_light_sampling_settings("power_ris"), reuse=reuse)
    _frame(S, rh, W, H, 2, L.di_light_sampling_settings("power_ris"), reuse=reuse)
    assert (rh.direct_lighting.download_reservoirs()["M"] > 8).any()
    _frame(S, rh, W, H, 3, L.di_light_sampling_settings("regir"), reuse=reuse)
    assert (rh.direct_lighting.download_reservoirs()["M"] <= 8).all()
    _frame(S, rh, W, H, 4, L.di_light_sampling_settings("regir"), reuse=reuse)
    assert (rh.direct_lighting.download_reservoirs()["M"] > 8).any()
    del rh
    # a shared scene: the viewer presamples its own buffers, with the owner's bits
    v = ptamd.SharedScene(a, gb)
    rv = _renderer(ptamd, a, v, W, H)
    _frame(S, rv, W, H, 9, L.di_light_sampling_settings("regir"), bounces=1)
    _frame(S, rb, W, H, 9, L.di_light_sampling_settings("regir"), bounces=1)
    for which in (0, 1):
        tv, tb = rv.direct_lighting.download_presampled(which), rb.direct_lighting.download_presampled(which)
        assert len(tv) and np.array_equal(tv, tb)
    ov, ob = ptamd.textures_to_numpy(rv.textures), ptamd.textures_to_numpy(rb.textures)
    for k in keys:
        assert np.array_equal(ov[k], ob[k]), k
    del ra, rb, rv
    v.close(); ga.close(); a.close(); gb.close()


@pytest.mark.gpu
def test_gpu_no_emitters(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = S.cornell_box(aspect=W / H)
    scene.object_data["Material"]["EmissiveStrength"] = 0.0
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    r = _renderer(ptamd, gpu, g, W, H)
    for mode in MODES:
        gs = S.graphics_settings(W, H, spp=1, bounces=2)
        gs["IsDIEnabled"] = 1
        r.textures["Diffuse"].fill_(0x3C00)
        r.render(gs, di_samples=8, di_light_sampling=L.di_light_sampling_settings(mode)); gpu.sync()
        assert int(r.textures["Diffuse"].abs().sum()) == 0
        assert len(r.direct_lighting.download_presampled(0)) == 0 and len(r.direct_lighting.download_presampled(1)) == 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_sharding_bit_identical(gpu, ptamd, pkg, mode):
    """two emulated ranks (8-row bands) reproduce the unsharded frame bit for bit"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 48
    scene = S.emitter_field(32, aspect=W / H)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    r = _renderer(ptamd, gpu, g, W, H)
    _frame(S, r, W, H, 7, L.di_light_sampling_settings(mode))
    full = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    del r
    bands = []
    for rank in range(2):
        gpu.set_sharding(rank, 2, 8)
        rr = _renderer(ptamd, gpu, g, W, H)
        _frame(S, rr, W, H, 7, L.di_light_sampling_settings(mode))
        bands.append(ptamd.textures_to_numpy(rr.textures)["RadianceF32"])
        del rr
    gpu.set_sharding(0, 1, 16)
    rows = [None] * H
    for rank in range(2):
        lr = 0
        for b in range(rank, (H + 7) // 8, 2):
            for y in range(b * 8, min(H, b * 8 + 8)):
                rows[y] = bands[rank][lr]; lr += 1
    assert np.array_equal(np.stack(rows).view(np.uint32), full.view(np.uint32))
    assert (full[..., :3] > 0).any()
    g.close()


@pytest.mark.gpu
def test_gpu_invalid_settings_refused(gpu, ptamd, pkg):
    """every out-of-range field is refused with a message and leaves the previous setting active"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 32, 16
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.emitter_field(8, aspect=W / H))
    r = _renderer(ptamd, gpu, g, W, H)
    r.direct_lighting.SetLightSampling(L.di_light_sampling_settings("regir"))
    bad = [dict(mode=4), dict(cell_size=0.05), dict(cell_size=10.5), dict(cell_size=float("nan")), dict(cell_size=float("inf")),
           dict(build_samples=0), dict(build_samples=33)]
    for kw in bad:
        with pytest.raises(ptamd.PtInvalidArgument):
            r.direct_lighting.SetLightSampling(L.di_light_sampling_settings(**kw))
    gs = S.graphics_settings(W, H, spp=1, bounces=0, frame_index=1)
    gs["IsDIEnabled"] = 1
    r.direct_lighting.SetConstants(L.di_settings(W, H, 1, 8, 0, last_pass=True))
    r.direct_lighting.Render(g.GetTopLevelAccelerationStructure())      # the ReGIR setting is still the active one
    gpu.sync()
    assert len(r.direct_lighting.download_presampled(1)) == 4096 * 512
    with pytest.raises(ptamd.PtInvalidArgument):
        r.direct_lighting.download_presampled(2)
    g.close()


@pytest.mark.gpu
def test_cpp_host_light_sampling_matches_python(tmp_path, gpu, ptamd, pkg):
    """pt_demo --di --light-sampling regir: the C++ host's DirectLighting with ReGIR, bit-identical to the Python-driven frame"""
    demo = os.path.join(ge.PKG_DIR, "pt_demo")
    S, L = pkg.scenes, pkg.layouts
    W, H, spp, bounces = 160, 90, 2, 3
    out = str(tmp_path / "radiance.bin")
    subprocess.check_call([demo, "--di", "--di-samples", "6", "--light-sampling", "regir", "--width", str(W), "--height", str(H),
                           "--spp", str(spp), "--bounces", str(bounces), "--frames", "1", "--out", out], timeout=300)
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W / H, variant="ggx"))
    r = ptamd.Renderer(gpu, g, W, H, with_f32=True, with_denoiser_outputs=True)
    gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=0)
    gs["IsDIEnabled"] = 1
    r.render(gs, di_samples=6, di_light_sampling=L.di_light_sampling_settings("regir")); gpu.sync()
    ref = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    r.render(gs, di_samples=6); gpu.sync()
    cdf = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    g.close()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(ref, cdf)
