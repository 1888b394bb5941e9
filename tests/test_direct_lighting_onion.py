"""The ReGIR Onion layout on the GPU (pt_di_set_regir_layout): the built cells and the initial reservoirs pinned against
tests/onionref.py, unbiasedness against the power CDF, the error at a small cell size against the Grid's, the default path and the
lifecycle, sharding, and pt_demo --regir-layout."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import bsdfref
import dipins
import onionref as O
import presamplingref as P
import restirref as R

NEAR, NEAR_THRESHOLD = 1e-5, 1e-6
KEYS = ("Diffuse", "Specular", "RadianceF32")


@pytest.fixture(scope="module")
def tables(ptamd):
    return O.Tables(*[ptamd.onion_table(w) for w in range(4)])


@pytest.fixture(autouse=True)
def _shared_context_back_to_defaults(gpu):
    """the session's context is shared with every other test file: leave its DI settings as a fresh context has them"""
    yield
    lib = gpu.lib
    for call in (lib.pt_di_set_light_sampling, lib.pt_di_set_regir_layout, lib.pt_di_set_resampling, lib.pt_di_set_visibility, lib.pt_di_set_pairwise):
        gpu.check(call(gpu.handle, None))
    gpu.set_sharding(0, 1, 16)


def _renderer(ptamd, ctx, g, W, H, history=False):
    return ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True, di_history=history)


def _frame(S, r, W, H, frame, ls, layout, samples=8, reuse=None, bounces=0):
    gs = S.graphics_settings(W, H, spp=1, bounces=bounces, frame_index=frame)
    gs["IsDIEnabled"] = 1
    r.render(gs, di_samples=samples, di_reuse=reuse, di_light_sampling=ls, di_regir_layout=layout)
    r.ctx.sync()


def _lum(r, ptamd):
    return ptamd.textures_to_numpy(r.textures)["RadianceF32"][..., :3].astype(np.float64) @ R.LUMA


def _signed(a):
    return np.where(a == 0xFFFFFFFF, -1, a.astype(np.int64))


def _pinned_cells():
    """cell 0 and, in eight layers that cover the five groups, six cells: two of ring 0, ring 1 north and south, the two polar caps"""
    sel = [0]
    for layer in (0, 1, 2, 3, 4, 7, 10, 14):
        g = O.LAYER_GROUP[layer]
        n0, n1 = O.RING_CELLS[g][0], O.RING_CELLS[g][1]
        base, end = O.LAYER_BASE[layer], O.LAYER_BASE[layer] + O.LAYER_CELLS[layer]
        sel += [base + 1, base + n0 // 2, base + n0 + n1 // 3, base + n0 + n1 + (2 * n1) // 3, end - 2, end - 1]
    return np.array(sel)


@pytest.mark.gpu
def test_gpu_onion_cells_pinned(gpu, ptamd, pkg, tables):
    """49 cells of the Onion (cell 0; all five groups, both hemispheres, polar caps) restated in float32 in the kernel's order, at the Grid
    test's limits: the same light on >= 0.999 of the slots and the weight within 2e-5 relative."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 32, 24
    gpu.set_sharding(0, 1, 16)
    scene = S.emitter_field(16, aspect=W / H)
    g = ptamd.Scene(gpu, scene)
    r = _renderer(ptamd, gpu, g, W, H)
    _frame(S, r, W, H, 21, L.di_light_sampling_settings("regir", cell_size=0.7, build_samples=6), L.di_regir_layout_settings("onion"))
    lights = r.direct_lighting.download_lights()
    tiles = r.direct_lighting.download_presampled(0)
    cells = r.direct_lighting.download_presampled(1)
    g.close()
    assert len(tiles) == 128 * 1024 and len(cells) == O.CELLS * 512
    centre = scene.camera["Position"].astype(np.float32).reshape(3)
    sel = _pinned_cells()
    assert len(sel) == 49 and len(set(sel.tolist())) == 49 and sel.max() < O.CELLS
    assert (tables.cells[sel, 1] > 0).sum() > 10 and (tables.cells[sel, 1] < 0).sum() > 10
    exp_li, exp_w = O.onion_build(tables, lights, _signed(tiles["LightIndex"]), tiles["InvSourcePdf"], sel, centre, 0.7, 6, 21)
    got = cells.reshape(O.CELLS, 512)[sel]
    got_li = _signed(got["LightIndex"])
    same = got_li == exp_li
    rel = np.abs(got["InvSourcePdf"].astype(np.float64) - exp_w) / np.maximum(np.abs(exp_w), 1e-30)
    rel = np.where((exp_w == 0) & (got["InvSourcePdf"] == 0), 0.0, rel)
    filled = (exp_li >= 0).mean(1)
    print(f"Onion cells: {same.mean():.6f} of slots with the same light, weight rel err max {rel[same].max():.2e}; "
          f"{(exp_li >= 0).mean():.3f} of slots filled, {int((filled == 0).sum())} cells empty, {int((filled > 0.5).sum())} more than half full")
    assert (filled == 0).any() and (filled > 0.5).any()             # cells above the emitters are culled
    assert same.mean() >= 0.999
    assert rel[same].max() <= 2e-5


def _onion_initial_pin(gpu, ptamd, pkg, tables, cell_size, W, H):
    """Temporal on, Off, no boiling, frame 0 after a reset: the reservoirs are the initial ones. LightIndex, M, U, V exact, W within 2e-5;
    pixels within 1e-5 of a coin, or within 1e-6 relative of a layer, ring or azimuth threshold, are left out and counted. At cell size
    0.3 the Grid would send most of the frame to its Power_RIS fallback, the Onion none of it. Returns how many of the compared pixels lie
    in a screen tile that the frame's right or bottom edge cuts. Left out, measured: none at 37 x 23 (814 valid pixels) and 21 x 13 (252)."""
    S, L = pkg.scenes, pkg.layouts
    n, frame = 8, 3
    cut_x, cut_y = (W // P.SCREEN_TILE if W % P.SCREEN_TILE else -1), (H // P.SCREEN_TILE if H % P.SCREEN_TILE else -1)
    in_cut = 0
    gpu.set_sharding(0, 1, 16)
    scene = S.emitter_field(64, aspect=W / H)
    g = ptamd.Scene(gpu, scene)
    r = _renderer(ptamd, gpu, g, W, H, history=True)
    init = L.di_resampling_settings(temporal=True, spatial_samples=0, temporal_bias=L.DI_BIAS_CORRECTION_OFF, boiling_filter=False)
    r.direct_lighting.ResetHistory()
    _frame(S, r, W, H, frame, L.di_light_sampling_settings("regir", cell_size=cell_size), L.di_regir_layout_settings("onion"), samples=n, reuse=init)
    out = ptamd.textures_to_numpy(r.textures)
    got = r.direct_lighting.download_reservoirs().reshape(H, W)
    lights = r.direct_lighting.download_lights()
    tiles = r.direct_lighting.download_presampled(0)
    cells = r.direct_lighting.download_presampled(1)
    g.close()
    assert len(cells) == O.CELLS * 512
    bsdf = bsdfref.Reference()
    cur = R.Surfaces(out, scene.camera)
    tl, cl = _signed(tiles["LightIndex"]), _signed(cells["LightIndex"])
    centre = scene.camera["Position"].astype(np.float32).reshape(3)
    compared = excluded = near_threshold = valid = onion_fallback = grid_fallback = 0
    for y in range(H):
        for x in range(W):
            if not cur.valid[y, x]:
                continue
            valid += 1
            Pw = cur.P[y, x].astype(np.float32)
            m = []
            c, cell = O.candidates(tables, x, y, frame, n, Pw, tl, tiles["InvSourcePdf"], cl, cells["InvSourcePdf"], centre, cell_size, margins=m)
            onion_fallback += cell < 0
            grid_fallback += int(P.regir_cell(Pw, O.pixel_jitter(x, y, frame)[1], centre, cell_size)) < 0
            li, U, V, Wt, M, margin = P.initial_reservoir(cur, (y, x), c, lights, bsdf, n)
            if margin < NEAR or m[0] < NEAR_THRESHOLD:
                excluded += 1
                near_threshold += m[0] < NEAR_THRESHOLD
                continue
            compared += 1
            in_cut += int(x // P.SCREEN_TILE == cut_x or y // P.SCREEN_TILE == cut_y)
            gr = got[y, x]
            gli = -1 if gr["LightIndex"] == 0xFFFFFFFF else int(gr["LightIndex"])
            assert (gli, int(gr["M"])) == (li, M), (x, y, gli, li, int(gr["M"]), cell)
            if li >= 0:
                assert np.float32(gr["U"]) == np.float32(U) and np.float32(gr["V"]) == np.float32(V), (x, y)
                assert abs(float(gr["W"]) - Wt) <= 2e-5 * Wt, (x, y, float(gr["W"]), Wt)
            else:
                assert float(gr["W"]) == 0.0
    print(f"cell size {cell_size} at {W} x {H}: {compared} pixels compared ({in_cut} in cut screen tiles), {excluded} left out "
          f"({excluded / max(1, compared + excluded):.3%}; {near_threshold} near a cell threshold), fallbacks: Onion {onion_fallback}, Grid {grid_fallback} of {valid}")
    assert compared > 0.5 * W * H and excluded < 0.05 * (compared + excluded)
    if cell_size == 0.3:
        assert grid_fallback > 0.5 * valid and onion_fallback == 0
    return in_cut


@pytest.mark.gpu
@pytest.mark.parametrize("cell_size", [1.0, 0.3])
def test_gpu_onion_initial_reservoirs_pinned(gpu, ptamd, pkg, tables, cell_size):
    """_onion_initial_pin at 40 x 24"""
    _onion_initial_pin(gpu, ptamd, pkg, tables, cell_size, 40, 24)


@pytest.mark.gpu
@pytest.mark.parametrize("size", dipins.RAGGED, ids=dipins.size_id)
@pytest.mark.parametrize("cell_size", [1.0, 0.3])
def test_gpu_onion_initial_reservoirs_pinned_ragged(gpu, ptamd, pkg, tables, cell_size, size):
    """_onion_initial_pin at the sizes that cut the 16 x 16 block, the 8 x 8 wave tile and the 16-pixel screen tile on both axes: same
    scene, settings, tolerances and caps; pixels of the cut screen tiles must be among the compared ones. (No pixel of this scene leaves
    the Onion, so none draws from its screen tile's light tile: that witness is test_direct_lighting_presampling.py's, under Power_RIS.)"""
    W, H = size
    assert _onion_initial_pin(gpu, ptamd, pkg, tables, cell_size, W, H) > 0


def _means(ptamd, S, L, ctx, g, W, H, ls, layout, frames, base, samples=8, reuse=None):
    r = _renderer(ptamd, ctx, g, W, H, history=reuse is not None)
    v = []
    for f in range(frames):
        _frame(S, r, W, H, base + f, ls, layout, samples=samples, reuse=reuse)
        v.append(_lum(r, ptamd))
    return np.stack(v)


@pytest.fixture(scope="module")
def field64(gpu, ptamd, pkg):
    """emitter_field(64) at 48 x 32 and what the statistical tests share: the power CDF's frames, computed once"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.emitter_field(64, aspect=W / H))
    cdf = _means(ptamd, S, L, gpu, g, W, H, None, None, 48, 1000)
    cdf.setflags(write=False)
    yield g, W, H, cdf
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("reuse", [False, True], ids=["onion", "onion-reuse"])
def test_gpu_onion_unbiased_against_the_power_cdf(gpu, ptamd, pkg, field64, reuse):
    """the per-pixel mean over 48 frames matches the power-CDF mean within a bound from the measured per-pixel variance: fewer than 2 % of
    pixels beyond 4 standard errors (x 3 with temporal + spatial reuse at the defaults, which correlates the frames), image mean within 2 %"""
    S, L = pkg.scenes, pkg.layouts
    g, W, H, ref = field64
    K = len(ref)
    gpu.set_sharding(0, 1, 16)
    got = _means(ptamd, S, L, gpu, g, W, H, L.di_light_sampling_settings("regir"), L.di_regir_layout_settings("onion"), K, 2000,
                 reuse=L.di_resampling_settings() if reuse else None)
    sel = (ref.mean(0) > 0) & (got.mean(0) > 0)
    assert sel.sum() > 0.5 * W * H
    se = np.sqrt(ref.var(0, ddof=1) / K + got.var(0, ddof=1) / K)[sel] * (3.0 if reuse else 1.0)
    d = (got.mean(0) - ref.mean(0))[sel]
    z = np.abs(d) / np.maximum(se, 1e-30)
    rel = d.mean() / ref.mean(0)[sel].mean()
    print(f"onion{'-reuse' if reuse else ''}: {np.mean(z > 4):.4f} of pixels beyond 4 standard errors, image-mean difference {rel:+.4f}")
    assert np.mean(z > 4) < 0.02
    assert abs(rel) < 0.02


MEASURED_MSE_RATIO = 0.542     # Onion / Grid at cell size 0.3, measured on an MI355X


@pytest.mark.gpu
def test_gpu_onion_lowers_the_error_at_a_small_cell_size(gpu, ptamd, pkg, field64):
    """8 candidates, ReGIRCellSize 0.3, 24 frames against a 32-candidate x 48-frame power-CDF reference: the Onion's per-pixel MSE is below
    the Grid's, which serves most of this frame from its Power_RIS fallback (622 of 920 valid pixels in the 40 x 24 pin). Measured on an
    MI355X: ratio 0.542; the threshold keeps half of the measured gain, 1 - (1 - 0.542) / 2 = 0.771."""
    S, L = pkg.scenes, pkg.layouts
    g, W, H, _ = field64
    K = 24
    gpu.set_sharding(0, 1, 16)
    ls = L.di_light_sampling_settings("regir", cell_size=0.3)
    ref = _means(ptamd, S, L, gpu, g, W, H, None, None, 48, 5000, samples=32).mean(0)
    grid = _means(ptamd, S, L, gpu, g, W, H, ls, L.di_regir_layout_settings("grid"), K, 7000)
    onion = _means(ptamd, S, L, gpu, g, W, H, ls, L.di_regir_layout_settings("onion"), K, 7000)
    sel = ref > 0
    mse_grid = ((grid - ref) ** 2)[:, sel].mean()
    mse_onion = ((onion - ref) ** 2)[:, sel].mean()
    print(f"MSE ratio Onion / Grid at cell size 0.3: {mse_onion / mse_grid:.3f}")
    assert mse_onion < mse_grid
    assert mse_onion < (1.0 - (1.0 - MEASURED_MSE_RATIO) / 2.0) * mse_grid


@pytest.mark.gpu
def test_gpu_onion_default_path_and_lifecycle(gpu, ptamd, pkg):
    """Onion then NULL, and Layout = GRID, are bit-identical to a context that never set a layout; Grid <-> Onion resets the history; the
    cell download follows the layout; the layout changes no bit under power_ris; a viewer of a shared scene gets the owner's bits; an
    unknown Layout is refused and the previous one stays."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = S.emitter_field(32, aspect=W / H)
    regir, onion, grid = L.di_light_sampling_settings("regir"), L.di_regir_layout_settings("onion"), L.di_regir_layout_settings("grid")
    gpu.set_sharding(0, 1, 16)
    a = ptamd.DeviceContext(0)                                      # a fresh context that never hears of a layout
    ga = ptamd.Scene(a, scene)
    ra = _renderer(ptamd, a, ga, W, H)
    ra.direct_lighting.SetReGIRLayout = lambda settings: None
    gb = ptamd.Scene(gpu, scene)
    rb = _renderer(ptamd, gpu, gb, W, H)

    def tex(r):
        return ptamd.textures_to_numpy(r.textures)

    def same(x, y):
        return all(np.array_equal(x[k], y[k]) for k in KEYS)

    _frame(S, ra, W, H, 6, regir, None, bounces=1)
    never, never_cells = tex(ra), ra.direct_lighting.download_presampled(1)
    assert len(never_cells) == 4096 * 512 and (never["Diffuse"][..., :3] != 0).any()
    _frame(S, rb, W, H, 5, regir, onion, bounces=1)
    assert len(rb.direct_lighting.download_presampled(1)) == O.CELLS * 512
    _frame(S, rb, W, H, 6, regir, onion, bounces=1)
    as_onion = tex(rb)
    assert not same(as_onion, never)
    _frame(S, rb, W, H, 6, regir, None, bounces=1)                    # Onion, then NULL
    assert same(tex(rb), never) and np.array_equal(rb.direct_lighting.download_presampled(1), never_cells)
    _frame(S, rb, W, H, 6, regir, onion, bounces=1)
    _frame(S, rb, W, H, 6, regir, grid, bounces=1)                    # Onion, then Layout = GRID
    assert same(tex(rb), never) and np.array_equal(rb.direct_lighting.download_presampled(1), never_cells)
    # an unknown layout is refused; the Onion stays (the next frame makes no layout call of its own)
    rb.direct_lighting.SetReGIRLayout(onion)
    with pytest.raises(ptamd.PtInvalidArgument):
        rb.direct_lighting.SetReGIRLayout(L.di_regir_layout_settings(2))
    rb.direct_lighting.SetReGIRLayout = lambda settings: None
    _frame(S, rb, W, H, 6, regir, None, bounces=1)
    del rb.direct_lighting.SetReGIRLayout
    assert len(rb.direct_lighting.download_presampled(1)) == O.CELLS * 512 and same(tex(rb), as_onion)
    # the layout acts only in ReGIR mode
    pr = L.di_light_sampling_settings("power_ris")
    _frame(S, rb, W, H, 8, pr, None, bounces=1)
    plain = tex(rb)
    _frame(S, rb, W, H, 8, pr, onion, bounces=1)
    assert same(tex(rb), plain) and len(rb.direct_lighting.download_presampled(1)) == 0
    _frame(S, rb, W, H, 8, None, onion, bounces=1)
    cdf = tex(rb)
    _frame(S, rb, W, H, 8, None, None, bounces=1)
    assert same(tex(rb), cdf)
    # history: two reuse frames build it up; Grid <-> Onion resets it
    rh = _renderer(ptamd, gpu, gb, W, H, history=True)
    reuse = L.di_resampling_settings(temporal=True, spatial_samples=0, boiling_filter=False)
    for frame, layout, grown in ((1, grid, False), (2, grid, True), (3, onion, False), (4, onion, True), (5, grid, False), (6, None, True)):
        _frame(S, rh, W, H, frame, regir, layout, reuse=reuse)
        M = rh.direct_lighting.download_reservoirs()["M"]
        assert (M > 8).any() if grown else (M <= 8).all(), (frame, int(M.max()))
    del rh
    # a shared scene: the viewer builds its own cells, with the owner's bits
    v = ptamd.SharedScene(a, gb)
    rv = _renderer(ptamd, a, v, W, H)
    _frame(S, rv, W, H, 9, regir, onion, bounces=1)
    _frame(S, rb, W, H, 9, regir, onion, bounces=1)
    for which in (0, 1):
        tv, tb = rv.direct_lighting.download_presampled(which), rb.direct_lighting.download_presampled(which)
        assert len(tv) and np.array_equal(tv, tb)
    assert same(tex(rv), tex(rb))
    del ra, rb, rv
    v.close(); ga.close(); a.close(); gb.close()


@pytest.mark.gpu
def test_gpu_onion_sharding_bit_identical(gpu, ptamd, pkg):
    """two emulated ranks (8-row bands) reproduce the unsharded Onion frame bit for bit"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 48
    scene = S.emitter_field(32, aspect=W / H)
    ls, onion = L.di_light_sampling_settings("regir"), L.di_regir_layout_settings("onion")
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    r = _renderer(ptamd, gpu, g, W, H)
    _frame(S, r, W, H, 7, ls, onion)
    full = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    _frame(S, r, W, H, 7, ls, None)
    as_grid = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    del r
    bands = []
    for rank in range(2):
        gpu.set_sharding(rank, 2, 8)
        rr = _renderer(ptamd, gpu, g, W, H)
        _frame(S, rr, W, H, 7, ls, onion)
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
    assert (full[..., :3] > 0).any() and not np.array_equal(full, as_grid)
    g.close()


@pytest.mark.gpu
def test_cpp_host_onion_matches_python(tmp_path, gpu, ptamd, pkg):
    """pt_demo --di --light-sampling regir --regir-layout onion: the C++ host's frame, bit-identical to the Python-driven one and not the
    Grid's; --regir-layout without ReGIR is refused before any GPU work"""
    demo = os.path.join(ge.PKG_DIR, "pt_demo")
    S, L = pkg.scenes, pkg.layouts
    W, H, spp, bounces = 160, 90, 2, 3
    out = str(tmp_path / "radiance.bin")
    size = ["--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces), "--frames", "1"]
    subprocess.check_call([demo, "--di", "--di-samples", "6", "--light-sampling", "regir", "--regir-layout", "onion", *size, "--out", out], timeout=300)
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W / H, variant="ggx"))
    r = ptamd.Renderer(gpu, g, W, H, with_f32=True, with_denoiser_outputs=True)
    gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=0)
    gs["IsDIEnabled"] = 1
    ls = L.di_light_sampling_settings("regir")
    r.render(gs, di_samples=6, di_light_sampling=ls, di_regir_layout=L.di_regir_layout_settings("onion")); gpu.sync()
    ref = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    r.render(gs, di_samples=6, di_light_sampling=ls); gpu.sync()
    grid = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    g.close()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(ref, grid)
    bad = subprocess.run([demo, "--di", "--light-sampling", "power_ris", "--regir-layout", "onion", *size], stderr=subprocess.PIPE, text=True, timeout=300)
    assert bad.returncode != 0 and "--regir-layout" in bad.stderr
