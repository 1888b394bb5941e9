"""The textured G-buffer pass and path estimator against the float64 replay (tests/surfaceref.py, tests/pathref.py, sampling through
tests/texref.py) on the scenes of tests/texscene.py: the CPU oracle here, the device under -m gpu in every form a frame can take. Until
these, a textured frame was only checked device == oracle, both written from the same reading of the shaders.

Inside a rendered frame this pins: both UV sets interpolated from f16 at oblique hits on transformed and mirrored instances; the tangent
through ObjectToWorld and its negation on a back face; EvaluateMaterial fed from bounce hits, normal map included; the alpha test of every
candidate in closest-hit traversal (each walker rebuilds instance, geometry and primitive itself); the lat-long and cube environment under
EnvironmentLightTransform; the frames that compile alpha test or transmission out. Every switch of the three references' MUTATIONS that
concerns textures is shown to fail the comparison, on the oracle's frame and on the device's.

A render samples through the objects' resolved texture slots; nothing switches a render to the heap descriptors (they stay with
pt_trace_visibility, tests/test_texture_reference.py), so the device rows run the one texture source a frame has. The replay of a row is
computed once from the device's G-buffer and shared by every form: the forms share the G-buffer pass, which is asserted byte for byte.
The conditions -- unsafe share of the G-buffer, risky share and kept pixels of the estimator -- are computed from the reference alone and
asserted before any comparison."""
import numpy as np
import pytest

import pathref as P
import surfaceref as R
import texref
import texscene as T

W, H = T.SIZE
RISKY_CAP = 0.05                                         # tests/test_estimator_reference.py
UNSAFE_CAP = 0.03                                        # tests/test_gbuffer_reference.py
KEPT_FLOOR = 0.5 * W * H * 0.6                           # tests/test_estimator_reference.py
BLOB_LDS_MAX = 40 * 1024                                 # beyond it a scene renders in the streaming form (test_frame_forms.py)
V1, PHASED, UNFUSED, LOCKSTEP, GENERIC = 0x4, 0x8, 0x10, 0x20, 0x400      # include/ptamd.h PT_DEBUG_*, as tests/test_frame_forms.py selects them

SCENES = {
    "textured": lambda S: T.textured(S),
    "large": lambda S: T.textured(S, large=True),
    "latlong": lambda S: T.textured(S, env="latlong"),
    "cube": lambda S: T.textured(S, env="cube"),
    "plain": lambda S: T.textured(S, masked=False, transmissive=False),          # no alpha-tested geometry, no transmission: the compiled-out forms
    "plain_masked": lambda S: T.textured(S, masked=True, transmissive=False),
    "plain_transmissive": lambda S: T.textured(S, masked=False, transmissive=True),
}
# row: scene, spp, bounces, roulette, Denoiser
ROWS = {
    "textured_s1_b1": ("textured", 1, 1, True, 0),
    "textured_s2_b6": ("textured", 2, 6, True, 0),
    "textured_s2_b6_no_roulette": ("textured", 2, 6, False, 0),
    "textured_s2_b6_reblur": ("textured", 2, 6, True, 2),
    "textured_s2_b6_dlss_rr": ("textured", 2, 6, True, 1),
    "latlong_s2_b6": ("latlong", 2, 6, True, 0),
    "cube_s2_b6": ("cube", 2, 6, True, 0),
    "plain_s2_b6": ("plain", 2, 6, True, 0),
    "plain_masked_s2_b6": ("plain_masked", 2, 6, True, 0),
    "plain_transmissive_s2_b6": ("plain_transmissive", 2, 6, True, 0),
    "large_s2_b6": ("large", 2, 6, True, 0),
}
_cache = {}


def scene_of(pkg, name):
    if ("scene", name) not in _cache:
        sc = SCENES[name](pkg.scenes)
        assert sc.triangle_count <= 2000, sc.triangle_count
        _cache["scene", name] = (sc, R.Surface(sc))
    return _cache["scene", name]


def surface_render(pkg, name):
    if ("render", name) not in _cache:
        sc, surface = scene_of(pkg, name)
        _cache["render", name] = surface.render(sc.camera, W, H)
    return _cache["render", name]


def settings_of(pkg, row):
    _, spp, bounces, rr, denoiser = ROWS[row]
    gs = pkg.scenes.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=3, russian_roulette=rr)
    gs["Denoiser"] = denoiser
    return gs


def mutant(pkg, scene_name, mutation):
    """(Surface, replay mutations) with one switch of surfaceref / texref / pathref set"""
    sc, _ = scene_of(pkg, scene_name)
    if mutation in R.TEXTURE_MUTATIONS:
        return R.Surface(sc, **{mutation: True}), ()
    if mutation in texref.MUTATIONS:
        return R.Surface(sc, tex=texref.Reference(**{mutation: True})), ()
    assert mutation in P.TEXTURE_MUTATIONS, mutation
    return scene_of(pkg, scene_name)[1], (mutation,)


def oracle_frame(oracle, pkg, row):
    """The oracle's frame of a row: the G-buffer textures (every flag set) as the path tracer finds them, its outputs and RadianceF32"""
    if ("oracle", row) in _cache:
        return _cache["oracle", row]
    L = pkg.layouts
    scene, _ = scene_of(pkg, ROWS[row][0])
    gs = settings_of(pkg, row)
    gkey = ("gbuffer", ROWS[row][0], bool(int(gs["Denoiser"])))
    if gkey not in _cache:
        gb = {k: np.zeros((H, W, c), dt) for k, (dt, c) in L.GBUFFER_FORMATS.items()}
        gb.update({k: np.zeros((H, W, c), dt) for k, (dt, c) in L.DENOISER_FORMATS.items()})
        k = np.zeros((), L.GBUFFER_CONSTANTS)
        k["RenderSize"] = (W, H)
        k["Flags"] = 0xFFFFFFFF if int(gs["Denoiser"]) else L.GBufferFlags.DefaultNoDenoiser
        osc = oracle.OracleScene(scene)
        osc.gbuffer(k, gb)
        osc.close()
        _cache[gkey] = gb
    gbuffer = _cache[gkey]
    out = {k: v.copy() for k, v in gbuffer.items()}
    f32 = np.zeros((H, W, 4), np.float32)
    osc = oracle.OracleScene(scene)
    osc.raytrace(gs, out, radiance_f32=f32)
    osc.close()
    _cache["oracle", row] = {"gbuffer": gbuffer, "out": out, "f32": f32, "settings": gs}
    return _cache["oracle", row]


def replayed(pkg, row, gbuffer, tag, mutation=None):
    """the replay of a row from the G-buffer textures `gbuffer` (tag: whose they are), computed once"""
    key = ("replay", row, tag, mutation)
    if key not in _cache:
        scene, surface = scene_of(pkg, ROWS[row][0])
        mutations = ()
        if mutation is not None:
            surface, mutations = mutant(pkg, ROWS[row][0], mutation)
        _cache[key] = P.replay(scene, settings_of(pkg, row), gbuffer, scene.camera, scene.scene_data, mutations=mutations, surface=surface)
    return _cache[key]


def assert_gbuffer_matches(gb, ref, surface, what, flags=0xFFFFFFFF):
    fails, fig = R.compare(gb, ref, surface, flags)
    assert ref["hit"].any() and (~ref["hit"]).any(), what
    assert fig["unsafe_share"] <= UNSAFE_CAP, f"{what}: {fig['unsafe_share']:.4%} of the hit pixels are unsafe"
    assert not fails, f"{what}: kept pixels outside tolerance {fails}; unsafe share {fig['unsafe_share']:.4%}, figures {fig}"
    return fig


def assert_frame_matches(out, f32, rep, gs, what):
    fails, fig = P.compare(out, rep, gs, f32)
    print(what, fig)
    assert fig["kept"] > KEPT_FLOOR, (what, fig)
    assert fig["risky_share"] <= RISKY_CAP, f"{what}: {fig['risky_share']:.3%} of the primary-hit pixels are risky"
    assert not fails, f"{what}: kept pixels outside tolerance {fails}; risky share {fig['risky_share']:.3%}, figures {fig}"
    return fig


# ----------------------------------------------------------------------------------------------
# the scenes carry what they claim (reference only)
# ----------------------------------------------------------------------------------------------
def test_scenes_cover_the_cases(pkg):
    sc, surface = scene_of(pkg, "textured")
    ref = surface_render(pkg, "textured")
    hit = ref["hit"] & ~ref["unsafe"]
    tris = surface.tris
    formats = {(item.width, item.height, item.fmt) for item in sc.heap if item.kind == 1}
    for size in ((1, 1), (5, 3), (16, 16)):
        for fmt in (texref.FMT_RGBA8, texref.FMT_RGBA8_SRGB, texref.FMT_RGBA32F):
            assert size + (fmt,) in formats, (size, fmt)
    slots = {i: set(s) for i, (_, s) in enumerate(surface.objects)}
    seen = np.unique(ref["object"][hit])
    used = set().union(*(slots[i] for i in seen))
    assert used == set(texref.SLOTS), used                                   # every slot is in view
    uv_sets = {idx for i in seen for (_, _, idx) in surface.objects[i][1].values()}
    assert uv_sets == {0, 1}
    mirrored = np.linalg.det(tris.o2w[:, :, :3]) < 0
    normal_mapped = np.array(["Normal" in slots[i] for i in ref["object"]]) & tris.has_t[ref["tri"]]
    assert (hit & normal_mapped & mirrored[ref["instance"]]).sum() > 20 and (hit & normal_mapped & ~ref["front"]).sum() > 20
    no_tangents = np.array(["Normal" in slots[i] for i in ref["object"]]) & ~tris.has_t[ref["tri"]]
    assert (hit & no_tangents).sum() > 20
    assert np.array_equal(ref["shading"][hit & no_tangents], surface.reconstruct(ref["tri"], ref["u"], ref["v"], ref["direction"])["shading"][hit & no_tangents])
    perturbed = 1.0 - R.dot(ref["shading"], surface.reconstruct(ref["tri"], ref["u"], ref["v"], ref["direction"])["shading"])
    assert (perturbed[hit & normal_mapped] > 1e-3).mean() > 0.5             # the normal map really turns the normal
    masked = ~tris.opaque
    assert masked.any() and (hit & masked[ref["tri"]]).sum() > 20
    bare = surface.tris.closest(ref["origin"], ref["direction"], ref["tmin"], ref["tmax"])
    through = hit & bare["hit"] & masked[bare["tri"]] & (bare["tri"] != ref["tri"])
    assert through.sum() > 20                                                # primary rays pass through holes
    two = [i for i, (first, count) in enumerate(sc.blas) if count == 2]
    assert len(two) == 1 and int(sc.geometry[sc.blas[two[0]][0]][0].material["AlphaMode"]) == 0 and int(sc.geometry[sc.blas[two[0]][0] + 1][0].material["AlphaMode"]) == 1
    for kind in ("latlong", "cube"):
        e = scene_of(pkg, kind)[0]
        assert e.env_texture.data.dtype == np.float32 and e.env_texture.data.max() > 1.0
        M = np.asarray(e.scene_data["EnvironmentLightTransform"], np.float64).reshape(3, 4)[:, :3]
        assert np.abs(M - M.T).max() > 0.1 and np.abs(M - np.eye(3)).max() > 0.1
    for name in ("plain", "plain_transmissive"):
        assert scene_of(pkg, name)[1].tris.opaque.all()
    for name in ("plain", "plain_masked"):
        assert not (scene_of(pkg, name)[0].object_data["Material"]["Transmission"] > 0).any()


# ----------------------------------------------------------------------------------------------
# CPU tier: the oracle against the replay
# ----------------------------------------------------------------------------------------------
GBUFFER_SCENES = ("textured", "latlong", "cube", "plain", "plain_masked", "plain_transmissive", "large")
ROW_OF_SCENE = {"textured": "textured_s2_b6_reblur", "latlong": "latlong_s2_b6", "cube": "cube_s2_b6", "plain": "plain_s2_b6",
                "plain_masked": "plain_masked_s2_b6", "plain_transmissive": "plain_transmissive_s2_b6", "large": "large_s2_b6"}


def gbuffer_flags(pkg, row):
    return 0xFFFFFFFF if ROWS[row][4] else int(pkg.layouts.GBufferFlags.DefaultNoDenoiser)


@pytest.mark.parametrize("name", GBUFFER_SCENES)
def test_oracle_gbuffer_matches_textured_surface(name, oracle, pkg):
    row = ROW_OF_SCENE[name]
    fr = oracle_frame(oracle, pkg, row)
    fig = assert_gbuffer_matches(fr["gbuffer"], surface_render(pkg, name), scene_of(pkg, name)[1], name, gbuffer_flags(pkg, row))
    print(name, fig)


@pytest.mark.parametrize("row", list(ROWS))
def test_oracle_estimator_matches_replay(row, oracle, pkg):
    fr = oracle_frame(oracle, pkg, row)
    rep = replayed(pkg, row, fr["gbuffer"], "oracle")
    assert_frame_matches(fr["out"], fr["f32"], rep, fr["settings"], row)
    if ROWS[row][2] > 1 and ROWS[row][0] in ("textured", "large", "plain_masked"):
        assert rep["rejected"].sum() > 50, int(rep["rejected"].sum())     # bounce rays really meet holes


# switch -> the row whose estimator frame shows it (bounce hits, bounce rays and misses: a (1, 1) row only adds the emission met at bounce 1,
# so the material switches need the six-bounce row). Those that reach the primary surface are also shown on the G-buffer comparison alone, below.
#   UVs from corner 0: uv_corner0             TextureCoordinateIndex ignored: texref ignore_uv_index      cutoff exclusive: texref cutoff_gt
#   alpha test skipped for bounce rays only: alpha_skip_bounce                                             OPAQUE flag ignored: alpha_ignores_opaque_flag
#   the rule on geometry 0's material: alpha_geometry0       tangent kept on back faces: tangent_no_back_flip
#   every bounce at the primary hit's UVs: material_at_primary_uv        a rejected candidate draws: rejected_draws_random
MUTATION_ROW = {
    "uv_corner0": "textured_s2_b6", "ignore_uv_index": "textured_s2_b6", "alpha_skip_bounce": "textured_s2_b6", "cutoff_gt": "textured_s2_b6",
    "alpha_ignores_opaque_flag": "textured_s2_b6", "alpha_geometry0": "textured_s2_b6", "tangent_no_back_flip": "textured_s2_b6",
    "normal_map_ignored": "textured_s2_b6", "normal_map_without_tangents": "textured_s2_b6", "emissive_texture_ignored": "textured_s1_b1",
    "transmission_gate_on_factor": "textured_s2_b6", "env_no_transform": "latlong_s2_b6", "env_transposed": "cube_s2_b6",
    "material_at_primary_uv": "textured_s1_b1", "rejected_draws_random": "textured_s2_b6",
    # texref's own switches, carried through the frame
    "swap_mr_channels": "textured_s2_b6", "no_half_texel": "textured_s2_b6", "clamp_uv": "textured_s2_b6",
    "swap_wh": "textured_s2_b6", "flip_cube_face_sc": "cube_s2_b6", "cube_clamp": "cube_s2_b6",
}
# (texref's srgb_alpha is not among them: the masks here hold alpha 0 and 255 only, which decode the same either way; test_texture_reference.py owns it)
assert set(MUTATION_ROW) == set(R.TEXTURE_MUTATIONS) | set(P.TEXTURE_MUTATIONS) | (set(texref.MUTATIONS) - {"srgb_alpha"})


@pytest.mark.parametrize("mutation,row", list(MUTATION_ROW.items()), ids=[f"{m}-{r}" for m, r in MUTATION_ROW.items()])
def test_mutated_replay_is_caught_on_the_oracle(mutation, row, oracle, pkg):
    fr = oracle_frame(oracle, pkg, row)
    wrong = replayed(pkg, row, fr["gbuffer"], "oracle", mutation)
    fails, _ = P.compare(fr["out"], wrong, fr["settings"], fr["f32"])
    assert fails, f"the comparison on {row} does not notice {mutation}"
    print(mutation, row, fails)


# the switches that reach the primary surface, on the G-buffer comparison alone
GBUFFER_MUTATION_SCENE = {
    "uv_corner0": "textured", "ignore_uv_index": "textured", "cutoff_gt": "textured", "alpha_ignores_opaque_flag": "textured",
    "alpha_geometry0": "textured", "tangent_no_back_flip": "textured", "normal_map_ignored": "textured", "normal_map_without_tangents": "textured",
    "emissive_texture_ignored": "textured", "transmission_gate_on_factor": "textured", "env_no_transform": "latlong", "env_transposed": "cube",
    "swap_mr_channels": "textured", "no_half_texel": "textured", "clamp_uv": "textured", "swap_wh": "textured", "flip_cube_face_sc": "cube",
    "cube_clamp": "cube",
}


def mutated_gbuffer_fails(pkg, mutation, gbuffer):
    name = GBUFFER_MUTATION_SCENE[mutation]
    key = ("mutated render", name, mutation)
    if key not in _cache:
        wrong, _ = mutant(pkg, name, mutation)
        _cache[key] = (wrong, wrong.render(scene_of(pkg, name)[0].camera, W, H))
    wrong, ref = _cache[key]
    return R.compare(gbuffer, ref, wrong, gbuffer_flags(pkg, ROW_OF_SCENE[name]))[0]


@pytest.mark.parametrize("mutation", list(GBUFFER_MUTATION_SCENE))
def test_mutated_surface_is_caught_on_the_oracle(mutation, oracle, pkg):
    fails = mutated_gbuffer_fails(pkg, mutation, oracle_frame(oracle, pkg, ROW_OF_SCENE[GBUFFER_MUTATION_SCENE[mutation]])["gbuffer"])
    assert fails, f"the G-buffer comparison does not notice {mutation}"
    print(mutation, fails)


def test_untextured_replay_has_no_texture_terms(pkg):
    """an untextured scene takes none of the textured branches: no slack, no bounds, the alpha rule tests nothing"""
    sc = R.transformed(pkg.scenes, emissive=True, aspect=W / H)
    surface = R.Surface(sc)
    assert not surface.textured and not len(surface.alpha_rule.tested)
    ref = surface.render(sc.camera, W, H)
    assert not any(k.endswith("_error") and k not in ("position_error", "linear_depth_error", "normalized_depth_error", "motion_error", "radiance_error")
                   for k in ref) and not ref["radiance_error"].any()


# ----------------------------------------------------------------------------------------------
# GPU tier
# ----------------------------------------------------------------------------------------------
OUT_KEYS = ("Radiance", "RadianceF32", "Diffuse", "Specular", "SpecularHitDistance")


def gpu_frame(ptamd, ctx, pkg, row, debug_flags=0, streaming=False):
    """gbuffer.Render, the textures copied out, raytracing.Render under the debug flags: (G-buffer textures, outputs)"""
    key = ("gpu", row, debug_flags)
    if key in _cache:
        return _cache[key]
    L = pkg.layouts
    scene, _ = scene_of(pkg, ROWS[row][0])
    gs = settings_of(pkg, row)
    g = ptamd.Scene(ctx, scene)
    try:
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True)
        assert (ctx.accel_stats().BlobBytes > BLOB_LDS_MAX) == streaming, ctx.accel_stats().BlobBytes
        tlas = g.GetTopLevelAccelerationStructure()
        r.constants["Flags"] = gbuffer_flags(pkg, row)
        r.gbuffer.Render(tlas, r.constants)
        ctx.sync()
        gbuffer = {k: v.copy() for k, v in ptamd.textures_to_numpy(r.textures).items()}
        try:
            ctx.set_debug_flags(debug_flags)
            r.raytracing.SetConstants(gs)
            r.raytracing.Render(tlas)
            ctx.sync()
        finally:
            ctx.set_debug_flags(0)
        out = ptamd.textures_to_numpy({k: r.textures[k] for k in OUT_KEYS})
    finally:
        g.close()
    _cache[key] = (gbuffer, out)
    return _cache[key]


def gpu_replay(pkg, row, gbuffer, mutation=None):
    """the replay of a row from the device's G-buffer, once for every form: the forms share the G-buffer pass, byte for byte"""
    if ("gpu gbuffer", row) not in _cache:
        _cache["gpu gbuffer", row] = gbuffer
    first = _cache["gpu gbuffer", row]
    for k in first:
        if k not in OUT_KEYS:
            assert np.array_equal(first[k].view(np.uint8), gbuffer[k].view(np.uint8)), (row, k)
    return replayed(pkg, row, first, "gpu", mutation)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GBUFFER_SCENES)
def test_gpu_gbuffer_matches_textured_surface(name, gpu, ptamd, pkg):
    row = ROW_OF_SCENE[name]
    gbuffer, _ = gpu_frame(ptamd, gpu, pkg, row, 0, streaming=(name == "large"))
    assert_gbuffer_matches(gbuffer, surface_render(pkg, name), scene_of(pkg, name)[1], name, gbuffer_flags(pkg, row))


# form: debug flags. The fused round; k_shade + k_extend2; the TLAS-walking schedule; the interleaved walk of k_extend; and the same frame with
# the alpha test and the transmission lobe kept in where the scene would compile them out.
SMALL_FORMS = {"fused": 0, "unfused": UNFUSED, "phased": PHASED, "unfused_phased": UNFUSED | PHASED, "v1": V1, "generic": GENERIC}
LARGE_FORMS = {"streaming": 0, "lockstep": LOCKSTEP, "unfused": UNFUSED, "lockstep_phased": LOCKSTEP | PHASED}


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r for r in ROWS if r != "large_s2_b6"])
def test_gpu_estimator_matches_replay(row, gpu, ptamd, pkg):
    gbuffer, out = gpu_frame(ptamd, gpu, pkg, row, 0)
    assert_frame_matches(out, out["RadianceF32"], gpu_replay(pkg, row, gbuffer), settings_of(pkg, row), f"{row}, fused")


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["textured_s2_b6", "plain_s2_b6", "plain_masked_s2_b6", "plain_transmissive_s2_b6"])
@pytest.mark.parametrize("form", [f for f in SMALL_FORMS if f != "fused"])
def test_gpu_estimator_forms_match_replay(form, row, gpu, ptamd, pkg):
    gbuffer, out = gpu_frame(ptamd, gpu, pkg, row, SMALL_FORMS[form])
    assert_frame_matches(out, out["RadianceF32"], gpu_replay(pkg, row, gbuffer), settings_of(pkg, row), f"{row}, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(LARGE_FORMS))
def test_gpu_estimator_beyond_lds_matches_replay(form, gpu, ptamd, pkg):
    row = "large_s2_b6"
    gbuffer, out = gpu_frame(ptamd, gpu, pkg, row, LARGE_FORMS[form], streaming=True)
    assert_frame_matches(out, out["RadianceF32"], gpu_replay(pkg, row, gbuffer), settings_of(pkg, row), f"{row}, {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("mutation,row", list(MUTATION_ROW.items()), ids=[f"{m}-{r}" for m, r in MUTATION_ROW.items()])
def test_mutated_replay_is_caught_on_the_device(mutation, row, gpu, ptamd, pkg):
    gbuffer, out = gpu_frame(ptamd, gpu, pkg, row, 0)
    wrong = gpu_replay(pkg, row, gbuffer, mutation)
    fails, _ = P.compare(out, wrong, settings_of(pkg, row), out["RadianceF32"])
    assert fails, f"the comparison on the device's {row} does not notice {mutation}"


@pytest.mark.gpu
@pytest.mark.parametrize("mutation", list(GBUFFER_MUTATION_SCENE))
def test_mutated_surface_is_caught_on_the_device(mutation, gpu, ptamd, pkg):
    name = GBUFFER_MUTATION_SCENE[mutation]
    gbuffer, _ = gpu_frame(ptamd, gpu, pkg, ROW_OF_SCENE[name], 0)
    assert mutated_gbuffer_fails(pkg, mutation, gbuffer), f"the G-buffer comparison on the device's {name} does not notice {mutation}"
