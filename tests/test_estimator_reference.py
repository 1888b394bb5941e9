"""The path estimator against tests/pathref.py, a float64 replay of Raytracing.hlsl's RayGeneration taken from the shader: the CPU oracle
here, the HIP paths (k_round, k_shade + k_extend2, streaming) under -m gpu, where the IsDIEnabled half -- which the oracle does not have --
is replayed as well, from synthetic direct-lighting textures."""
import numpy as np
import pytest

import pathref as P
import surfaceref as R

W, H = 48, 32
RISKY_CAP = 0.05
ENV = (0.3, 0.4, 0.5, 1.0)
UNFUSED = 0x10                                           # PT_DEBUG_UNFUSED_ROUNDS, as tests/test_frame_forms.py selects it
BLOB_LDS_MAX = 40 * 1024                                 # beyond it a scene renders in the streaming form (test_frame_forms.py)


def cornell(S, variant, env=ENV):
    sc = S.cornell_box(aspect=W / H, variant=variant, jitter=(0.2, -0.35))
    sc.scene_data = S.make_scene_data(env)
    return sc.finalize()


SCENES = {
    "ggx": lambda S: cornell(S, "ggx"),
    "diffuse": lambda S: cornell(S, "diffuse"),
    "sky": lambda S: cornell(S, "ggx", env=(0.0, 0.0, 0.0, -1.0)),
    "transformed": lambda S: R.transformed(S, emissive=True, aspect=W / H),
    "overflow": lambda S: R.transformed(S, emissive=3e38, aspect=W / H),       # four samples of it do not fit fp32: the non-finite guard
    "large": lambda S: R.transformed(S, emissive=True, aspect=W / H, subdiv=3, mirrored_sphere=False),   # beyond LDS: the streaming form
}

# row: scene, spp, bounces, roulette, ThroughputThreshold, ExtFlags, Denoiser
ROWS = {
    "ggx_s1_b1": ("ggx", 1, 1, True, 1e-3, 0, 0),
    "ggx_s2_b6": ("ggx", 2, 6, True, 1e-3, 0, 0),
    "ggx_s4_b8": ("ggx", 4, 8, True, 1e-3, 0, 0),
    "ggx_s2_b6_no_roulette": ("ggx", 2, 6, False, 1e-3, 0, 0),
    "ggx_s4_b8_threshold": ("ggx", 4, 8, True, 0.2, 0, 0),
    "diffuse_s2_b6_threshold_no_roulette": ("diffuse", 2, 6, False, 0.2, 0, 0),
    "diffuse_lambertian_s4_b8": ("diffuse", 4, 8, True, 1e-3, 1, 0),
    "sky_s2_b6": ("sky", 2, 6, True, 1e-3, 0, 0),
    "transformed_emissive_s2_b6": ("transformed", 2, 6, True, 1e-3, 0, 0),
    "overflow_s4_b2": ("overflow", 4, 2, True, 1e-3, 0, 0),
    "ggx_s2_b6_dlss_rr": ("ggx", 2, 6, True, 1e-3, 0, 1),
    "ggx_s2_b6_reblur": ("ggx", 2, 6, True, 1e-3, 0, 2),
    "transformed_emissive_s2_b6_relax": ("transformed", 2, 6, True, 1e-3, 0, 3),
}
_cache = {}


def scene_of(pkg, name):
    if ("scene", name) not in _cache:
        sc = SCENES[name](pkg.scenes)
        _cache["scene", name] = (sc, R.Surface(sc))
    return _cache["scene", name]


def settings_of(pkg, row):
    scene, spp, bounces, rr, thr, ext, denoiser = ROWS[row]
    gs = pkg.scenes.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=3, russian_roulette=rr, ext_flags=ext, throughput_threshold=thr)
    gs["Denoiser"] = denoiser
    return gs


def oracle_frame(oracle, pkg, row, rows=None):
    """The oracle's frame of a row: the G-buffer textures as the path tracer found them, its outputs, RadianceF32 and ray count."""
    key = ("oracle", row, rows)
    if key in _cache:
        return _cache[key]
    L = pkg.layouts
    scene, _ = scene_of(pkg, ROWS[row][0])
    gs = settings_of(pkg, row)
    if ("gbuffer", row) not in _cache:
        gb = {k: np.zeros((H, W, c), dt) for k, (dt, c) in L.GBUFFER_FORMATS.items()}
        gb.update({k: np.zeros((H, W, c), dt) for k, (dt, c) in L.DENOISER_FORMATS.items()})
        k = np.zeros((), L.GBUFFER_CONSTANTS)
        k["RenderSize"] = (W, H)
        k["Flags"] = 0xFFFFFFFF if int(gs["Denoiser"]) else L.GBufferFlags.DefaultNoDenoiser
        osc = oracle.OracleScene(scene)
        osc.gbuffer(k, gb)
        osc.close()
        _cache["gbuffer", row] = gb
    gbuffer = _cache["gbuffer", row]
    out = {k: v.copy() for k, v in gbuffer.items()}
    f32 = np.zeros((H, W, 4), np.float32)
    osc = oracle.OracleScene(scene)
    rays = osc.raytrace(gs, out, radiance_f32=f32, rows=rows)
    osc.close()
    _cache[key] = {"gbuffer": gbuffer, "out": out, "f32": f32, "rays": int(rays), "settings": gs}
    return _cache[key]


def replayed(pkg, row, gbuffer, mutations=(), di=None):
    key = ("replay", row, tuple(mutations), id(gbuffer))
    if key not in _cache:
        scene, surface = scene_of(pkg, ROWS[row][0])
        _cache[key] = (gbuffer, P.replay(scene, settings_of(pkg, row), gbuffer, scene.camera, scene.scene_data, di=di, mutations=mutations,
                                         surface=surface))
    return _cache[key][1]


def assert_frame_matches(out, f32, rep, gs, what):
    fails, fig = P.compare(out, rep, gs, f32)
    assert fig["kept"] > 0.5 * W * H * 0.6, (what, fig)
    assert fig["risky_share"] <= RISKY_CAP, f"{what}: {fig['risky_share']:.3%} of the primary-hit pixels are risky"
    assert not fails, f"{what}: kept pixels outside tolerance {fails}; risky share {fig['risky_share']:.3%}, figures {fig}"
    return fig


@pytest.mark.parametrize("row", list(ROWS))
def test_oracle_estimator_matches_replay(row, oracle, pkg):
    fr = oracle_frame(oracle, pkg, row)
    rep = replayed(pkg, row, fr["gbuffer"])
    fig = assert_frame_matches(fr["out"], fr["f32"], rep, fr["settings"], row)
    print(row, fig)
    if row == "overflow_s4_b2":
        zeroed = rep["primary_hit"] & ~rep["risky"] & (rep["budget"].max(1) > 0) & (rep["radiance"] == 0).all(1)
        assert zeroed.sum() > 20, int(zeroed.sum())                            # the guard really acts in this row
    if "threshold" in row:
        assert rep["segments"].sum() < 0.8 * replay_segments_without_threshold(pkg, row, fr), row    # the threshold really ends paths


def replay_segments_without_threshold(pkg, row, fr):
    scene, surface = scene_of(pkg, ROWS[row][0])
    gs = fr["settings"].copy()
    gs["ThroughputThreshold"] = 1e-3
    return P.replay(scene, gs, fr["gbuffer"], scene.camera, scene.scene_data, surface=surface)["segments"].sum()


def test_estimator_invariants(oracle, pkg):
    # rays traced: per image row of the oracle against the replay's segments -- equal where no pixel of the row is risky, and overall within
    # what the risky pixels can trace at most
    row = "transformed_emissive_s2_b6"
    fr = oracle_frame(oracle, pkg, row)
    rep = replayed(pkg, row, fr["gbuffer"])
    spp, bounces = ROWS[row][1], ROWS[row][2]
    seg, risky = rep["segments"].reshape(H, W), rep["risky"].reshape(H, W)
    clean = 0
    for y in range(H):
        if not risky[y].any():
            assert oracle_frame(oracle, pkg, row, rows=(y, y + 1))["rays"] == seg[y].sum(), y
            clean += 1
    assert clean >= H // 4, clean
    kept = int(seg[~risky].sum())
    assert kept <= fr["rays"] <= kept + int(risky.sum()) * spp * bounces
    # a primary miss is untouched: the G-buffer's environment colour stays, RadianceF32 is never written
    miss = ~rep["primary_hit"].reshape(H, W)
    assert miss.sum() > 100
    assert np.array_equal(fr["out"]["Radiance"][miss], fr["gbuffer"]["Radiance"][miss]) and not fr["f32"][miss].any()
    assert (rep["segments"][~rep["primary_hit"]] == 0).all()
    # Bounces = 1: one segment per sample, and the frame is emission plus one bounce as the replay has it
    row = "ggx_s1_b1"
    fr = oracle_frame(oracle, pkg, row)
    rep = replayed(pkg, row, fr["gbuffer"])
    assert (rep["segments"] <= 1).all() and fr["rays"] <= rep["primary_hit"].sum()
    assert_frame_matches(fr["out"], fr["f32"], rep, fr["settings"], row)


MUTATION_ROW = {
    "roulette_from_3": "ggx_s4_b8", "roulette_no_divide": "ggx_s4_b8", "threshold_before_roulette": "ggx_s4_b8_threshold",
    "bounce_exclusive": "ggx_s1_b1", "emission_after_throughput": "ggx_s1_b1", "divide_before_finite": "overflow_s4_b2",
    "rng_per_sample": "ggx_s2_b6", "hit_distance_bounce0": "ggx_s2_b6_reblur", "is_diffuse_last_sample": "ggx_s2_b6_reblur",
}


assert set(MUTATION_ROW) == set(P.MUTATIONS) - set(P.DI_MUTATIONS) - set(P.TEXTURE_MUTATIONS)      # those: tests/test_textured_estimator.py


@pytest.mark.parametrize("mutation,row", list(MUTATION_ROW.items()), ids=[f"{m}-{r}" for m, r in MUTATION_ROW.items()])
def test_mutated_replay_is_caught(mutation, row, oracle, pkg):
    fr = oracle_frame(oracle, pkg, row)
    wrong = replayed(pkg, row, fr["gbuffer"], mutations=(mutation,))
    fails, _ = P.compare(fr["out"], wrong, fr["settings"], fr["f32"])
    assert fails, f"the comparison on {row} does not notice {mutation}"
    print(mutation, row, fails)


# ----------------------------------------------------------------------------------------------
# the device
# ----------------------------------------------------------------------------------------------
OUT_KEYS = ("Radiance", "RadianceF32", "Diffuse", "Specular", "SpecularHitDistance")


def gpu_frame(ptamd, ctx, pkg, scene, gs, debug_flags=0, direct=None, streaming=None):
    """gbuffer.Render, the textures copied out, raytracing.Render: (G-buffer textures, outputs, SecondaryRays). direct: (Diffuse, Specular)
    half-bit arrays written into the textures between the two passes, in place of a DI pass. streaming: the form the scene must take."""
    L = pkg.layouts
    g = ptamd.Scene(ctx, scene)
    try:
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True)
        if streaming is not None:
            assert (ctx.accel_stats().BlobBytes > BLOB_LDS_MAX) == streaming, ctx.accel_stats().BlobBytes
        tlas = g.GetTopLevelAccelerationStructure()
        r.constants["Flags"] = 0xFFFFFFFF if int(gs["Denoiser"]) else L.GBufferFlags.DefaultNoDenoiser
        r.gbuffer.Render(tlas, r.constants)
        if direct is not None:
            import torch
            for name, bits in zip(("Diffuse", "Specular"), direct):
                r.textures[name].copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)))
        ctx.sync()
        gbuffer = {k: v.copy() for k, v in ptamd.textures_to_numpy(r.textures).items()}
        try:
            ctx.set_debug_flags(debug_flags)
            ctx.reset_counters()
            r.raytracing.SetConstants(gs)
            r.raytracing.Render(tlas)
            ctx.sync()
        finally:
            ctx.set_debug_flags(0)
        rays = int(ctx.counters().SecondaryRays)
        out = ptamd.textures_to_numpy({k: r.textures[k] for k in OUT_KEYS})
    finally:
        g.close()
    return gbuffer, out, rays


def assert_gpu_row(ptamd, gpu, pkg, row, debug_flags, scene_name=None, streaming=False):
    scene_name = scene_name or ROWS[row][0]
    scene, surface = scene_of(pkg, scene_name)
    gs = settings_of(pkg, row)
    gbuffer, out, rays = gpu_frame(ptamd, gpu, pkg, scene, gs, debug_flags, streaming=streaming)
    rep = P.replay(scene, gs, gbuffer, scene.camera, scene.scene_data, surface=surface)
    what = f"{row} on {scene_name}, debug flags {debug_flags:#x}"
    assert_frame_matches(out, out["RadianceF32"], rep, gs, what)
    kept = int(rep["segments"][~rep["risky"]].sum())
    assert kept <= rays <= kept + int(rep["risky"].sum()) * ROWS[row][1] * ROWS[row][2], what


@pytest.mark.gpu
@pytest.mark.parametrize("row", list(ROWS))
def test_gpu_estimator_matches_replay(row, gpu, ptamd, pkg):
    assert_gpu_row(ptamd, gpu, pkg, row, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["unfused", "streaming"])
def test_gpu_estimator_forms_match_replay(form, gpu, ptamd, pkg):
    """the (2, 6) rows again as k_shade + k_extend2, and on a scene beyond LDS, which renders in the streaming form"""
    if form == "unfused":
        assert_gpu_row(ptamd, gpu, pkg, "ggx_s2_b6", UNFUSED)
    else:
        assert_gpu_row(ptamd, gpu, pkg, "transformed_emissive_s2_b6", 0, scene_name="large", streaming=True)


def lit_room(S):
    """a floor and a box under a wide emissive panel: most first bounces off the floor end on the panel"""
    white = (0.73, 0.73, 0.73)
    nodes = [S.MeshNode([S.quad_mesh((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2), (0, 1, 0), S.material(white))]),
             S.MeshNode([S.quad_mesh((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, -1, 0), S.material((0.8, 0.8, 0.8), emissive=(1.0, 0.9, 0.7), strength=5.0))]),
             S.MeshNode([S.box_mesh(S.material((0.9, 0.6, 0.3), metallic=1.0, roughness=0.3))])]
    objects = [S.RenderObject(0, S.trs()), S.RenderObject(1, S.trs((0.0, 1.2, 0.3), 0.0, (1.5, 1.0, 1.5))),
               S.RenderObject(2, S.trs((0.6, 0.25, 0.5), 30.0, (0.5, 0.5, 0.5)))]
    cam = S.make_camera((0.0, 0.8, -2.4), forward=(0.0, -0.35, 1.0), hfov_deg=60.0, aspect=W / H, jitter=(0.1, 0.3))
    return S.Scene(nodes, objects, cam, S.make_scene_data(ENV), name="lit_room").finalize()


DI_DENOISERS = {"none": 0, "dlss_rr": 1, "nrd_reblur": 2}


@pytest.fixture(scope="module")
def di_frames(gpu, ptamd, pkg):
    """One device frame per denoiser with IsDIEnabled and synthetic Diffuse / Specular textures (no DI pass runs): rgb from a seeded
    generator in four pixel classes (both zero: DI invalid; diffuse only; specular only; both), junk in .w."""
    S = pkg.scenes
    scene = lit_room(S)
    surface = R.Surface(scene)
    rng = np.random.default_rng(11)
    cls = rng.integers(0, 4, (H, W))
    dif = np.zeros((H, W, 4), np.float16); spc = np.zeros((H, W, 4), np.float16)
    dif[..., :3] = rng.random((H, W, 3)) * 2.0 * ((cls == 1) | (cls == 3))[..., None]
    spc[..., :3] = rng.random((H, W, 3)) * 0.5 * ((cls == 2) | (cls == 3))[..., None]
    lone = rng.integers(0, 3, (H, W, 1)) == np.arange(3)                       # half of the pixels keep one channel only: any() is not all()
    some = np.where(rng.random((H, W, 1)) < 0.5, lone, True)
    dif[..., :3] *= some; spc[..., :3] *= some
    dif[..., 3] = rng.random((H, W)) * 100.0 - 50.0; spc[..., 3] = np.float16(np.nan)
    frames = {}
    for name, denoiser in DI_DENOISERS.items():
        gs = S.graphics_settings(W, H, spp=2, bounces=4, frame_index=5)
        gs["Denoiser"] = denoiser
        gs["IsDIEnabled"] = 1
        gbuffer, out, rays = gpu_frame(ptamd, gpu, pkg, scene, gs, direct=(dif.view(np.uint16), spc.view(np.uint16)))
        frames[name] = {"scene": scene, "surface": surface, "settings": gs, "gbuffer": gbuffer, "out": out, "rays": rays, "classes": cls.reshape(-1)}
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("denoiser", list(DI_DENOISERS))
def test_gpu_estimator_consumes_direct_lighting(denoiser, di_frames):
    fr = di_frames[denoiser]
    scene = fr["scene"]
    rep = P.replay(scene, fr["settings"], fr["gbuffer"], scene.camera, scene.scene_data, di=True, surface=fr["surface"])
    hit = rep["primary_hit"]
    share = (rep["emissive_at_bounce_1"] & hit).sum() / hit.sum()
    assert share >= 0.10, f"{share:.1%} of the pixels meet the emitter at bounce 1"
    for c in range(4):
        assert (hit & (fr["classes"] == c)).sum() > 100
    assert (rep["di_valid"] == (hit & (fr["classes"] != 0))).all()
    assert_frame_matches(fr["out"], fr["out"]["RadianceF32"], rep, fr["settings"], f"direct lighting, denoiser {denoiser}")


DI_MUTATION_DENOISER = {"di_suppress_bounce2": "none", "di_before_divide": "none", "di_swapped": "nrd_reblur", "di_valid_all": "dlss_rr"}


assert set(DI_MUTATION_DENOISER) == set(P.DI_MUTATIONS)


@pytest.mark.gpu
@pytest.mark.parametrize("mutation,denoiser", list(DI_MUTATION_DENOISER.items()), ids=[f"{m}-{d}" for m, d in DI_MUTATION_DENOISER.items()])
def test_gpu_mutated_di_replay_is_caught(mutation, denoiser, di_frames):
    fr = di_frames[denoiser]
    scene = fr["scene"]
    wrong = P.replay(scene, fr["settings"], fr["gbuffer"], scene.camera, scene.scene_data, di=True, mutations=(mutation,), surface=fr["surface"])
    fails, _ = P.compare(fr["out"], wrong, fr["settings"], fr["out"]["RadianceF32"])
    assert fails, f"the comparison does not notice {mutation}"
