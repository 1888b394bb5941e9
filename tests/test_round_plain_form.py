"""The plain form of the fused round kernel: a frame of a scene that has neither non-opaque geometry nor a transmissive material
(FramePlan::alpha / ::transmission, one switch) runs a k_round that, beyond the alpha test and the third lobe being compiled out, samples
the BSDF with the merged BSDFSample::Sample: what the diffuse and the specular branch both contain -- sincos_2pi(rnd[1]), the rotation out of
the shading basis, the test against the geometric normal -- is executed once by a wave that holds lanes of both lobes.

PT_DEBUG_GENERIC_SCENE forces the generic kernel, PT_DEBUG_UNFUSED_ROUNDS the k_shade + k_extend2 pair, which has the two-branch Sample. Every
comparison is the library against itself: every output texture byte for byte plus the ray counters (frames), every result word bit for bit
(pt_bsdf_sample, which runs the merged Sample unless PT_DEBUG_GENERIC_SCENE is set). The frames are those of
tests/test_scene_specialisation.py: 64 x 48, 4 spp, 8 bounces, Russian roulette on -- twelve tiles at the start, a partly filled last tile and
restarts in every round.

The CPU case holds the C ABI where it was: no struct of include/ptamd.h changes size, no debug bit is added or moved."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, UNFUSED = 0x400, 0x10                      # PT_DEBUG_GENERIC_SCENE, PT_DEBUG_UNFUSED_ROUNDS
W, H, SPP, BOUNCES = 64, 48, 4, 8
FLOOR, CEILING, BACK, LEFT_WALL, RIGHT_WALL, LIGHT, TALL_BOX, SHORT_BOX = range(8)      # scenes.cornell_box: object (= node = instance) indices
K_MIN_ROUGHNESS = 2e-3                              # pt_math.hpp kMinRoughness

# every PT_DEBUG_* bit of the parent commit's header
DEBUG_BITS = {"PT_DEBUG_TRAVERSAL_STATS": 0x1, "PT_DEBUG_BRUTE_FORCE": 0x2, "PT_DEBUG_TRAVERSAL_V1": 0x4, "PT_DEBUG_TRAVERSAL_PHASED": 0x8,
              "PT_DEBUG_UNFUSED_ROUNDS": 0x10, "PT_DEBUG_LOCKSTEP": 0x20, "PT_DEBUG_GATHER_LOCAL_ONLY": 0x40, "PT_DEBUG_GATHER_SELF_EXCHANGE": 0x80,
              "PT_DEBUG_SHARC_LOG_PATHS": 0x100, "PT_DEBUG_SHARC_SKIP_UPDATE": 0x200, "PT_DEBUG_GENERIC_SCENE": 0x400}


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_abi_unchanged(tmp_path):
    sizes = _module("test_scene_specialisation").STRUCT_SIZES           # sizeof of every struct, as the parent commit's header gives them
    header = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    names = [n for n in re.findall(r"typedef struct (\w+)", header) if n != "PtContext"]
    assert sorted(names) == sorted(sizes)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ptamd.h"\nint main(void) {\n'
                   + "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines()))
    assert got == sizes
    bits = {n: int(v, 16) for n, v in re.findall(r"#define (PT_DEBUG_\w+)\s+(0x[0-9a-fA-F]+)u", header)}
    assert bits == DEBUG_BITS                                           # none added, none moved


# ---------------------------------------------------------------------------------------------- frames
def _settings(S, L, denoiser=None):
    gs = S.graphics_settings(W, H, spp=SPP, bounces=BOUNCES, russian_roulette=True)
    gs["Denoiser"] = L.DENOISER_NONE if denoiser is None else denoiser
    return gs


def _frame(ptamd, ctx, r, gs, flags=0):
    """One frame (G-buffer + path tracer) under the debug flags: every output texture as bytes, primary and secondary ray counts."""
    try:
        ctx.set_debug_flags(flags)
        ctx.reset_counters()
        r.render(gs)
        ctx.sync()
    finally:
        ctx.set_debug_flags(0)
    c = ctx.counters()
    assert c.StackOverflows == 0
    return {k: v.tobytes() for k, v in ptamd.textures_to_numpy(r.textures).items()}, (c.PrimaryRays, c.SecondaryRays)


def _same(a, b, what=""):
    assert a[1] == b[1], (what, "ray counts", a[1], b[1])
    assert a[0].keys() == b[0].keys()
    for k in a[0]:
        assert a[0][k] == b[0][k], (what, k)


def _differ(a, b):
    return a[0]["RadianceF32"] != b[0]["RadianceF32"]


def _three_forms(ptamd, ctx, r, gs, what, unfused=True):
    """the planned frame, the generic kernel and the two-kernel form (the code of before) give the same frame; returns it"""
    planned = _frame(ptamd, ctx, r, gs)
    assert planned[1][0] == W * H and planned[1][1] > W * H
    _same(planned, _frame(ptamd, ctx, r, gs, GENERIC), (what, "generic kernel"))
    if unfused:
        _same(planned, _frame(ptamd, ctx, r, gs, UNFUSED), (what, "two-kernel form"))
    _same(planned, _frame(ptamd, ctx, r, gs), (what, "planned again"))
    return planned


@pytest.mark.gpu
@pytest.mark.parametrize("denoiser", ["none", "nrd"])
def test_plain_form_equals_generic_and_unfused(ptamd, pkg, denoiser):
    S, L = pkg.scenes, pkg.layouts
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    assert scene.scene_data["EnvironmentLightTextureDescriptor"] == L.NONE and not scene.object_data["Material"]["Transmission"].any()
    ctx = ptamd.DeviceContext(0)
    try:
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True)
        _three_forms(ptamd, ctx, r, _settings(S, L, L.DENOISER_NRD_REBLUR if denoiser == "nrd" else None), denoiser)
    finally:
        ctx.close()


def _material_variants(S, case):
    """The ggx box with materials over IOR < 1, = 1, 1.5 and large, Metallic 0, 0.5 and 1, roughness below kMinRoughness, two emitters.
    Both lobes are sampled at every kind of surface, from both sides. Back-face hits (IORi = IOR, IORo = 1):
      "flipped"  the vertex normals of the ceiling, the back wall and the left wall point out of the box: single-sided walls seen from
                 behind by every ray that reaches them, beside front-face hits on everything else;
      "inside"   the camera sits inside the tall box, whose normals point outward: every hit, primary and bounce, is a back-face hit."""
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    if case == "flipped":
        quads = {CEILING: ((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1), (0, 1, 0)), BACK: ((-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1), (0, 0, 1)),
                 LEFT_WALL: ((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1), (-1, 0, 0))}
        for node, (p0, p1, p2, p3, n) in quads.items():
            scene.nodes[node].meshes[0] = S.quad_mesh(p0, p1, p2, p3, n, scene.nodes[node].meshes[0].material)
        scene.finalize()
    m = scene.object_data["Material"]
    m["IOR"][FLOOR], m["Metallic"][FLOOR] = 0.8, 0.0
    m["IOR"][CEILING], m["Metallic"][CEILING] = 1.0, 0.5
    m["IOR"][BACK], m["Metallic"][BACK], m["Roughness"][BACK] = 1.5, 0.5, 0.3
    m["IOR"][LEFT_WALL], m["Roughness"][LEFT_WALL] = 50.0, K_MIN_ROUGHNESS / 4
    m["IOR"][RIGHT_WALL], m["Metallic"][RIGHT_WALL], m["Roughness"][RIGHT_WALL] = 1e30, 1.0, 0.0
    m["IOR"][SHORT_BOX], m["Metallic"][SHORT_BOX] = 2.4, 0.5
    m["EmissiveColor"][SHORT_BOX], m["EmissiveStrength"][SHORT_BOX] = (0.2, 0.5, 1.0), 0.75
    if case == "inside":
        m["IOR"][TALL_BOX], m["Metallic"][TALL_BOX], m["Roughness"][TALL_BOX] = 0.8, 0.5, 0.25
        m["EmissiveColor"][TALL_BOX], m["EmissiveStrength"][TALL_BOX] = (1.0, 0.6, 0.3), 0.5
        scene.camera = S.make_camera((-0.35, -0.4, 0.35), forward=(0.3, 0.2, 1.0), hfov_deg=90.0, aspect=W / H)
    return scene


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["front", "flipped", "inside"])
def test_material_variants(ptamd, pkg, case):
    """"inside" is held to the generic kernel only: with that camera the two-kernel form renders another frame than EITHER fused kernel, and did
    so before the plain form existed (71 730 secondary rays fused, 72 230 through k_pt_init + k_shade + k_extend2 and through both validation
    traversals, with the parent commit's library as with this one; the CPU oracle traces 72 230 too. Open)."""
    S, L = pkg.scenes, pkg.layouts
    scene = _material_variants(S, case)
    ctx = ptamd.DeviceContext(0)
    try:
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True)
        frame = _three_forms(ptamd, ctx, r, _settings(S, L), case, unfused=case != "inside")
        rad = np.frombuffer(frame[0]["RadianceF32"], np.float32)
        assert np.isfinite(rad).all() and rad.max() > 0.0                # the emitters are seen: the frame is not black
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- merged Sample
@pytest.mark.gpu
def test_merged_sample_equals_plain_sample(gpu, oracle):
    """pt_bsdf_sample on the query set of tests/test_bsdf_reference.py: queries without a third-lobe weight go through the merged Sample
    unless PT_DEBUG_GENERIC_SCENE is set; direction, pdf, weight, lobe weights, lobe and verdict are the same bits either way.
    Both arms come from one entry point under one flag, so this alone would also pass if the flag stopped reaching the launch: what holds the
    default (merged) path to something outside the library is tests/test_bsdf_reference.py::test_gpu_bsdf_sample_matches_oracle_and_float64,
    the same queries against the CPU oracle bit for bit and against the float64 reference."""
    T = _module("test_bsdf_reference")
    q = T.sample_queries()
    r = T.oracle_sample(oracle, q)
    q = np.concatenate([q, T.on_lobe_boundaries(q[:30000], r[:30000, 7:10])])
    try:
        gpu.set_debug_flags(0)
        merged = T.gpu_run(gpu, gpu.lib.pt_bsdf_sample, q, 12)
        gpu.set_debug_flags(GENERIC)
        plain = T.gpu_run(gpu, gpu.lib.pt_bsdf_sample, q, 12)
    finally:
        gpu.set_debug_flags(0)
    two_lobes = merged[:, 9] == 0.0                                            # the rows that took the merged form
    lobes = merged[:, 10].view(np.uint32)
    assert two_lobes.sum() > len(q) // 4 and (lobes[two_lobes] == 0).any() and (lobes[two_lobes] == 1).any()
    a, b = merged.view(np.uint32), plain.view(np.uint32)
    assert np.array_equal(a, b), f"{int((a != b).any(1).sum())} of {len(q)} rows differ, first {int(np.nonzero((a != b).any(1))[0][0])}"
