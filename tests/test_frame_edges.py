"""Frames that do not fill a tile: the G-buffer, the path tracer in every form and the hand-offs between them at sizes that cut the 16 x 16
block, the 8 x 8 wave tile and the 256-pixel queue tile, at frames smaller than a workgroup or a wave, and on ranks that hold no rows.

  (37, 23)  851 pixels: cuts the block and the wave tile on both axes, odd width and height; the last queue tile holds 83 pixels
  (21, 13)  273 pixels: 2 x 1 blocks, 3 x 2 wave tiles, all cut; the second queue tile holds 17 pixels
  (17, 5)   85 pixels: less than one workgroup; one queue tile with a wave of 21 lanes and two empty waves
  (1, 1)    one lane          (67, 1)  one row, 67 pixels: a full wave and 3 lanes          (1, 67)  one column, one pixel per row

What is compared: with the CPU oracle bit for bit (G-buffer, RadianceF32, Radiance, the denoiser-facing outputs, ray counts); with
tests/pathref.py where the oracle has nothing to say (IsDIEnabled fed by the DI pass of the same frame), at test_estimator_reference.py's
tolerance and risky cap; and the library against itself, sharded into bands that leave ranks without rows. The forms of a frame (fused /
streaming, flat / phased, unfused, lock-step, chained) at these sizes are tests/test_frame_forms.py's; the per-pixel DI pins at ragged
sizes are in the DI test files (tests/dipins.py).

The CPU half (not marked gpu) shows that the oracle renders every size with something to compare, and that pathref agrees with it at the
two sizes where pathref is the reference."""
import numpy as np
import pytest

import __graft_entry__ as ge
import pathref as P
import surfaceref as R
from test_estimator_reference import RISKY_CAP
from test_gpu_parity import GB_KEYS, assert_gbuffer_identical

ENV = (0.3, 0.4, 0.5, 1.0)
SPP, BOUNCES, FRAME = 8, 6, 3                  # (2 spp x 4 bounces leave 46 of the 851 pixels of 37 x 23 with any radiance; this: 149)

# size: what differs from (aspect W / H, SPP, FRAME). A single row or column gets a camera of the test's choosing, so that the frame has
# hits and misses: the Cornell camera's 90 degrees see only the inside of the box along a row (the opening spans 93), 110 see past it;
# aspect 0.5 opens a column to 127 degrees (aspect 1 / 67 would leave one hit pixel). The single pixel is black at 8 spp in every
# FrameIndex 0..11 but 9 (GGX) and 10 (diffuse); 32 spp at FrameIndex 5 reach the light in both scenes. All chosen on the oracle alone.
SIZES = {
    (37, 23): {}, (21, 13): {}, (17, 5): {},
    (1, 1): dict(spp=32, frame=5),
    (67, 1): dict(camera=dict(hfov_deg=110.0, aspect=67.0), misses=True),
    (1, 67): dict(camera=dict(hfov_deg=90.0, aspect=0.5), misses=True),
}
VARIANTS = {"ggx_glass": ("ggx", True), "diffuse": ("diffuse", False), "ggx": ("ggx", False)}
SCENES = ("ggx_glass", "diffuse")              # test_cornell_bit_identical_to_oracle's: with and without the glass sphere ("ggx": pathref's, as in test_estimator_reference.py)
CASES = [(name, size) for name in SCENES for size in SIZES]
RAGGED = [(37, 23), (17, 5)]
_cache = {}


def _id(v):
    return f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)


def make_scene(S, name, size, env=None, jitter=(0.0, 0.0)):
    W, H = size
    variant, glass = VARIANTS[name]
    sc = S.cornell_box(aspect=W / H, variant=variant, glass_sphere=glass, jitter=jitter)
    cam = SIZES[size].get("camera")
    if cam:
        sc.camera = S.make_camera((0, 0, -1.95), **cam)
    if env is not None:
        sc.scene_data = S.make_scene_data(env)
        sc.finalize()
    return sc


def make_settings(S, size, denoiser=0, di=False):
    gs = S.graphics_settings(size[0], size[1], spp=SIZES[size].get("spp", SPP), bounces=BOUNCES, frame_index=SIZES[size].get("frame", FRAME))
    gs["Denoiser"] = denoiser
    gs["IsDIEnabled"] = 1 if di else 0
    return gs


def oracle_frame(oracle, pkg, name, size, denoiser=0):
    """(G-buffer textures with the final Radiance and the denoiser outputs, rays, RadianceF32), computed once; read-only"""
    key = (name, size, denoiser)
    if key not in _cache:
        S, L = pkg.scenes, pkg.layouts
        flags = 0xFFFFFFFF if denoiser else 0xFFFFFFFF & ~0xC0                  # App.cpp:1223-1224
        gb, rays, f32 = oracle.render(make_scene(S, name, size), make_settings(S, size, denoiser), gbuffer_flags=flags, accel_mode=0, want_f32=True, layouts=L)
        for a in list(gb.values()) + [f32]:
            a.setflags(write=False)
        _cache[key] = (gb, int(rays), f32)
    return _cache[key]


# ----------------------------------------------------------------------------------------------
# the CPU half
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", CASES, ids=[f"{n}-{_id(s)}" for n, s in CASES])
def test_oracle_renders_every_size(name, size, oracle, pkg):
    """every size has primary hits, paths that go on (more rays than pixels) and radiance that is not zero, so that a comparison with it
    says something; the single row and the single column have misses too"""
    W, H = size
    gb, rays, f32 = oracle_frame(oracle, pkg, name, size)
    hit = np.isfinite(gb["Position"][..., 3])
    lit = (f32[..., :3] > 0).any(-1)
    print(f"{name} {W} x {H}: {int(hit.sum())} hits, {int((~hit).sum())} misses, {rays} rays, {int(lit.sum())} pixels with radiance")
    assert gb["Position"].shape == (H, W, 4) and hit.any() and lit.any() and rays > W * H
    assert (lit & hit).any() and not f32[~hit].any()                        # RadianceF32 is written at primary hits only
    if SIZES[size].get("misses"):
        assert (~hit).any() and hit.sum() >= 8 and (~hit).sum() >= 8
        assert np.isinf(gb["Position"][~hit]).all()


def _replay_scene(pkg, size):
    if ("replay scene", size) not in _cache:
        # test_estimator_reference.py's Cornell: its environment and its jitter. (Unjittered, the centred camera puts pixel centres on the
        # seams between the walls at any size -- 48 x 32 too -- where the replay and an fp32 tracer may take different faces.)
        sc = make_scene(pkg.scenes, "ggx", size, env=ENV, jitter=(0.2, -0.35))
        _cache["replay scene", size] = (sc, R.Surface(sc))
    return _cache["replay scene", size]


def _assert_matches_replay(out, f32, rep, gs, size, what):
    """test_estimator_reference.assert_frame_matches for a frame of this size: its share of kept pixels, its risky cap, pathref's tolerance"""
    fails, fig = P.compare(out, rep, gs, f32)
    assert fig["kept"] > 0.5 * size[0] * size[1] * 0.6, (what, fig)
    assert fig["risky_share"] <= RISKY_CAP, f"{what}: {fig['risky_share']:.3%} of the primary-hit pixels are risky"
    assert not fails, f"{what}: kept pixels outside tolerance {fails}; figures {fig}"
    return fig


@pytest.mark.parametrize("size", RAGGED, ids=_id)
@pytest.mark.parametrize("denoiser", [0, 2], ids=["none", "nrd_reblur"])
def test_pathref_agrees_with_the_oracle(size, denoiser, oracle, pkg):
    """pathref is the reference of the IsDIEnabled frames below: at these sizes it must first agree with the oracle where both speak"""
    S, L = pkg.scenes, pkg.layouts
    W, H = size
    scene, surface = _replay_scene(pkg, size)
    gs = make_settings(S, size, denoiser)
    gb = {k: np.zeros((H, W, c), dt) for k, (dt, c) in list(L.GBUFFER_FORMATS.items()) + list(L.DENOISER_FORMATS.items())}
    k = np.zeros((), L.GBUFFER_CONSTANTS)
    k["RenderSize"] = (W, H)
    k["Flags"] = 0xFFFFFFFF if denoiser else L.GBufferFlags.DefaultNoDenoiser
    osc = oracle.OracleScene(scene)
    osc.gbuffer(k, gb)
    out = {n: v.copy() for n, v in gb.items()}
    f32 = np.zeros((H, W, 4), np.float32)
    rays = osc.raytrace(gs, out, radiance_f32=f32)
    osc.close()
    rep = P.replay(scene, gs, gb, scene.camera, scene.scene_data, surface=surface)
    fig = _assert_matches_replay(out, f32, rep, gs, size, f"oracle {W} x {H}, denoiser {denoiser}")
    print(size, denoiser, fig)
    kept = int(rep["segments"][~rep["risky"]].sum())
    assert kept <= rays <= kept + int(rep["risky"].sum()) * int(gs["SamplesPerPixel"]) * BOUNCES


# ----------------------------------------------------------------------------------------------
# the device
# ----------------------------------------------------------------------------------------------
def gpu_frame(ptamd, ctx, scene, gs, size, sharding=(0, 1, 16), di_samples=0):
    """Renderer.render on the shared context: (every texture, counters)"""
    ctx.set_sharding(*sharding)
    try:
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, size[0], size[1], with_f32=True, with_denoiser_outputs=True)
        ctx.reset_counters()
        r.render(gs, di_samples=di_samples)
        ctx.sync()
        out, c = ptamd.textures_to_numpy(r.textures), ctx.counters()
        del r
        g.close()
    finally:
        ctx.set_sharding(0, 1, 16)
    return out, c


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", CASES, ids=[f"{n}-{_id(s)}" for n, s in CASES])
def test_gbuffer_and_path_tracer_bit_identical_to_oracle(name, size, gpu, ptamd, oracle, pkg):
    S = pkg.scenes
    W, H = size
    ref_gb, ref_rays, ref_f32 = oracle_frame(oracle, pkg, name, size)
    out, c = gpu_frame(ptamd, gpu, make_scene(S, name, size), make_settings(S, size), size)
    assert c.StackOverflows == 0
    assert_gbuffer_identical(out, ref_gb)
    assert c.PrimaryRays == W * H and c.PrimaryRays + c.SecondaryRays == ref_rays
    assert np.array_equal(out["RadianceF32"].view(np.uint32), ref_f32.view(np.uint32)), ge.compare_radiance(out["RadianceF32"], ref_f32)
    assert np.array_equal(out["Radiance"], ref_gb["Radiance"])


@pytest.mark.gpu
@pytest.mark.parametrize("size", RAGGED, ids=_id)
@pytest.mark.parametrize("denoiser", [2, 3], ids=["nrd_reblur", "nrd_relax"])
def test_denoiser_outputs_bit_identical_to_oracle(size, denoiser, gpu, ptamd, oracle, pkg):
    """the per-pixel aux array (hit distance, is-diffuse) behind Diffuse / Specular, and the albedo planes of the G-buffer call with every flag"""
    S = pkg.scenes
    ref_gb, ref_rays, _ = oracle_frame(oracle, pkg, "ggx_glass", size, denoiser)
    out, c = gpu_frame(ptamd, gpu, make_scene(S, "ggx_glass", size), make_settings(S, size, denoiser), size)
    assert c.PrimaryRays + c.SecondaryRays == ref_rays
    assert_gbuffer_identical(out, ref_gb)
    for k in ("Radiance", "Diffuse", "Specular", "SpecularHitDistance", "DiffuseAlbedo", "SpecularAlbedo"):
        assert np.array_equal(out[k], ref_gb[k]), (denoiser, k)
    dif, spc = (out[k].view(np.float16).astype(np.float32)[..., :3].sum(-1) for k in ("Diffuse", "Specular"))
    assert ((dif > 0) | (spc > 0)).any() and not ((dif > 0) & (spc > 0)).any()     # a pixel is either diffuse or specular


@pytest.mark.gpu
@pytest.mark.parametrize("size", RAGGED, ids=_id)
@pytest.mark.parametrize("denoiser", [0, 2, 3], ids=["none", "nrd_reblur", "nrd_relax"])
def test_path_tracer_consumes_the_di_pass_of_the_frame(size, denoiser, gpu, ptamd, pkg):
    """G-buffer, the plain DI pass (4 candidates), then the path tracer with IsDIEnabled: the frame against pathref.replay(di=True) fed the
    textures as the tracer found them -- the DI pass's own Diffuse / Specular among them"""
    S, L = pkg.scenes, pkg.layouts
    W, H = size
    scene, surface = _replay_scene(pkg, size)
    gs = make_settings(S, size, denoiser, di=True)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    try:
        r = ptamd.Renderer(gpu, g, W, H, with_f32=True, with_denoiser_outputs=True)
        tlas = g.GetTopLevelAccelerationStructure()
        r.constants["Flags"] = 0xFFFFFFFF if denoiser else L.GBufferFlags.DefaultNoDenoiser
        r.gbuffer.Render(tlas, r.constants)
        di = r.direct_lighting
        di.SetConstants(L.di_settings(W, H, int(gs["FrameIndex"]), 4, denoiser, last_pass=False, ext_flags=0))
        for reset in (di.SetResampling, di.SetLightSampling, di.SetVisibility, di.SetPairwise, di.SetReGIRLayout):
            reset(None)
        di.Render(tlas)
        gpu.sync()
        gbuffer = {k: v.copy() for k, v in ptamd.textures_to_numpy(r.textures).items()}
        gpu.reset_counters()
        r.raytracing.SetConstants(gs)
        r.raytracing.Render(tlas)
        gpu.sync()
        rays = int(gpu.counters().SecondaryRays)
        out = ptamd.textures_to_numpy({k: r.textures[k] for k in ("Radiance", "RadianceF32", "Diffuse", "Specular", "SpecularHitDistance")})
        del r
    finally:
        g.close()
    rep = P.replay(scene, gs, gbuffer, scene.camera, scene.scene_data, di=True, surface=surface)
    hit = rep["primary_hit"]
    print(f"{W} x {H}, denoiser {denoiser}: DI valid at {int(rep['di_valid'].sum())} of {int(hit.sum())} primary hits, {rays} rays")
    assert rep["di_valid"].sum() > 0.25 * hit.sum()                          # the hand-off is really in the frame
    _assert_matches_replay(out, out["RadianceF32"], rep, gs, size, f"direct lighting at {W} x {H}, denoiser {denoiser}")
    kept = int(rep["segments"][~rep["risky"]].sum())
    assert kept <= rays <= kept + int(rep["risky"].sum()) * int(gs["SamplesPerPixel"]) * BOUNCES


SHARDED = [((37, 23), 3, 4), ((37, 23), 3, 16), ((17, 5), 3, 16)]          # 23 rows: 6 bands of 4 (the last 3 rows) or 2 bands of 16 (the last 7 rows, rank 2 empty); 5 rows: ranks 1 and 2 empty


@pytest.mark.gpu
@pytest.mark.parametrize("size,world,band", SHARDED, ids=[f"{_id(s)}-{w}x{b}" for s, w, b in SHARDED])
def test_sharded_ragged_frame_equals_the_unsharded_one(size, world, band, gpu, ptamd, pkg):
    """The G-buffer, the plain DI pass and the path tracer that consumes it, as rank r of `world`: every texture, assembled by
    sharding.deinterleave, equals the unsharded frame bit for bit, and the ranks' rays add up to its rays. A rank without rows holds
    textures of zero bytes, renders without a launch and counts no ray."""
    S = pkg.scenes
    import dxpbrt_amd.sharding as SH
    W, H = size
    scene = make_scene(S, "ggx_glass", size)
    gs = make_settings(S, size, di=True)
    full, cf = gpu_frame(ptamd, gpu, scene, gs, size, di_samples=4)
    assert (full["Diffuse"][..., :3] != 0).any() and cf.SecondaryRays > 0
    pieces, primary, secondary, empty = [], 0, 0, 0
    for rank in range(world):
        out, c = gpu_frame(ptamd, gpu, scene, gs, size, sharding=(rank, world, band), di_samples=4)
        rows = SH.local_rows(H, rank, world, band)
        assert all(v.shape[0] == rows for v in out.values())
        if rows == 0:
            empty += 1
            assert c.PrimaryRays == 0 and c.SecondaryRays == 0
        pieces.append(out); primary += c.PrimaryRays; secondary += c.SecondaryRays
    assert empty == {((37, 23), 3, 4): 0, ((37, 23), 3, 16): 1, ((17, 5), 3, 16): 2}[size, world, band]
    assert (primary, secondary) == (cf.PrimaryRays, cf.SecondaryRays)
    for k in GB_KEYS + ("Transmission", "Radiance", "RadianceF32", "Diffuse", "Specular"):
        whole = SH.deinterleave([p[k] for p in pieces], H, band)
        assert np.array_equal(whole.view(np.uint8), full[k].view(np.uint8)), k
