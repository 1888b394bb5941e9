"""Scene specialisation: a frame of a scene that has neither non-opaque geometry nor a transmissive material runs a fused round kernel with the
alpha test and the third lobe compiled out (FramePlan::alpha / ::transmission, from SceneRefs::hasNonOpaque and Context::hasTransmission;
the two-kernel and streaming forms take no switch today and are held to the same comparisons). PT_DEBUG_GENERIC_SCENE forces the generic kernel. Every comparison is the library against itself, every output
texture bit for bit:

  * specialised against generic on the plain ggx Cornell box (fused rounds, the k_shade + k_extend2 pair) and on a scene beyond LDS (the
    streaming form), without a denoiser and with an NRD mode (the per-pixel auxiliary record), ray counts included;
  * scenes that HAVE the features (glass sphere; alpha-masked lattice + transmission texture) are the same with and without the bit, and equal
    the two-kernel validation form, which is the code of before the specialisation;
  * the facts follow the scene: a material made transmissive (announced with pt_invalidate_object_data), a wall made non-opaque (a bottom-level
    rebuild), in the context that owns the scene and through a SharedScene; and back.

The CPU case holds the C ABI where it was: no struct of include/ptamd.h changes size, the new debug bit collides with no other."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, UNFUSED = 0x400, 0x10                      # PT_DEBUG_GENERIC_SCENE, PT_DEBUG_UNFUSED_ROUNDS
BLOB_LDS_MAX = 40 * 1024                            # pt_kernels.hip kBlobLdsMax
W, H, SPP, BOUNCES = 64, 48, 4, 8                   # 3072 pixels: twelve 256-entry tiles at the start, a partly filled last tile and restarts in every round after
SHORT_BOX, LEFT_WALL = 7, 3                         # scenes.cornell_box: object (= node = instance) indices

# sizeof of every struct include/ptamd.h declares, as the parent commit's header gives them (cc, x86-64)
STRUCT_SIZES = {"PtVertexDesc": 32, "PtMeshDescriptors": 16, "PtMaterial": 64, "PtTextureMapInfo": 16, "PtObjectData": 224, "PtInstanceData": 112,
                "PtSceneData": 80, "PtCamera": 608, "PtGraphicsSettings": 80, "PtGBufferConstants": 12, "PtTextures": 136, "PtGeometryDesc": 40,
                "PtInstanceDesc": 64, "PtAccelStats": 80, "PtSharding": 16, "PtBandMessage": 40, "PtDISettings": 32, "PtTriangleLight": 80,
                "PtDIResamplingSettings": 64, "PtDIReservoir": 32, "PtDIPreviousTextures": 48, "PtDIVisibilitySettings": 32, "PtDIPairwiseSettings": 16,
                "PtDILightSamplingSettings": 16, "PtDIPresampledLight": 8, "PtDIReGIRLayoutSettings": 16, "PtRayDesc": 32, "PtBsdfQuery": 80,
                "PtBsdfResult": 32, "PtBsdfSampleQuery": 96, "PtBsdfSampleResult": 48, "PtPostProcessSettings": 48, "PtPostTextures": 32,
                "PtSHARCSettings": 28, "PtSHARCEntry": 32, "PtSHARCQueryResult": 16, "PtSHARCPathVertex": 64, "PtSHARCPathScatter": 128,
                "PtCounters": 64, "PtBlobLayout": 32, "PtClosestHit": 32}


def test_abi_and_layout_mirror_unchanged(tmp_path, pkg, ptamd):
    header = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    names = [n for n in re.findall(r"typedef struct (\w+)", header) if n != "PtContext"]
    assert sorted(names) == sorted(STRUCT_SIZES)                                # no struct added or removed
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ptamd.h"\nint main(void) {\n'
                   + "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines()))
    assert got == STRUCT_SIZES
    bits = {n: int(v, 16) for n, v in re.findall(r"#define (PT_DEBUG_\w+)\s+(0x[0-9a-fA-F]+)u", header)}
    assert bits["PT_DEBUG_GENERIC_SCENE"] == GENERIC
    assert len(set(bits.values())) == len(bits) and all(v & (v - 1) == 0 for v in bits.values())   # one bit each, none shared
    assert ptamd.load_library().pt_abi_version() == 4
    # the Python mirror: the layouts and ctypes structures the ABI test pins, where they were
    L = pkg.layouts
    assert (L.OBJECT_DATA.itemsize, L.MATERIAL.itemsize, L.GRAPHICS_SETTINGS.itemsize, L.INSTANCE_DATA.itemsize) == (224, 64, 80, 112)
    assert L.MATERIAL.fields["Transmission"][1] == 44 and L.MATERIAL.fields["AlphaCutoff"][1] == 52
    assert (C.sizeof(ptamd.GeometryDesc), C.sizeof(ptamd.InstanceDesc), C.sizeof(ptamd.Textures), C.sizeof(ptamd.Counters), C.sizeof(ptamd.AccelStats)) == (40, 64, 136, 64, 80)


def _settings(S, L, denoiser):
    gs = S.graphics_settings(W, H, spp=SPP, bounces=BOUNCES, russian_roulette=True)
    gs["Denoiser"] = denoiser
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


@pytest.mark.gpu
@pytest.mark.parametrize("denoiser", ["none", "nrd"])
@pytest.mark.parametrize("form", ["fused", "unfused", "streaming"])
def test_specialised_equals_generic(ptamd, pkg, form, denoiser):
    S, L = pkg.scenes, pkg.layouts
    # neither scene has a geometry without the OPAQUE flag or a transmissive material: both switches are off in the planned frame
    scene = S.sponza_scale(n_side=48, aspect=W / H) if form == "streaming" else S.cornell_box(aspect=W / H, variant="ggx")
    assert not scene.object_data["Material"]["Transmission"].any() and not scene.object_data["Material"]["AlphaMode"].any()
    base = UNFUSED if form == "unfused" else 0
    ctx = ptamd.DeviceContext(0)
    try:
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True)
        assert (ctx.accel_stats().BlobBytes > BLOB_LDS_MAX) == (form == "streaming")
        gs = _settings(S, L, L.DENOISER_NRD_REBLUR if denoiser == "nrd" else L.DENOISER_NONE)
        planned = _frame(ptamd, ctx, r, gs, base)
        generic = _frame(ptamd, ctx, r, gs, base | GENERIC)
        assert planned[1][0] == W * H and planned[1][1] > W * H
        _same(planned, generic, (form, denoiser))
        _same(_frame(ptamd, ctx, r, gs, base), planned, "planned again")        # the switch back re-captures the specialised frame
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["glass_sphere", "textured"])
def test_scenes_with_the_features_stay_generic(ptamd, pkg, name):
    S, L = pkg.scenes, pkg.layouts
    scene = S.cornell_box(aspect=W / H, variant="ggx", glass_sphere=True) if name == "glass_sphere" else S.cornell_box_textured(aspect=W / H)
    assert scene.object_data["Material"]["Transmission"].any()
    assert scene.object_data["Material"]["AlphaMode"].any() == (name == "textured")
    ctx = ptamd.DeviceContext(0)
    try:
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True)
        gs = _settings(S, L, L.DENOISER_NONE)
        planned = _frame(ptamd, ctx, r, gs)
        _same(planned, _frame(ptamd, ctx, r, gs, GENERIC), "debug bit")
        # k_shade + k_extend2: with the features present both run the code they ran before the switches existed
        _same(planned, _frame(ptamd, ctx, r, gs, UNFUSED), "two-kernel validation form")
        _same(planned, _frame(ptamd, ctx, r, gs, UNFUSED | GENERIC), "two-kernel validation form, debug bit")
    finally:
        ctx.close()


class _Rig:
    """The plain ggx box in a context of its own; shared: the frames are rendered by a second context that views the scene (pt_share_scene).
    The owner refuses to rebuild a bottom level while it is viewed, so a shared rig takes a fresh viewer for every state of the scene."""

    def __init__(self, ptamd, pkg, shared):
        self.ptamd, self.S, self.L, self.shared = ptamd, pkg.scenes, pkg.layouts, shared
        self.desc = self.S.cornell_box(aspect=W / H, variant="ggx")
        self.owner = ptamd.DeviceContext(0)
        self.g = ptamd.Scene(self.owner, self.desc)
        self.viewer = None
        self.gs = _settings(self.S, self.L, self.L.DENOISER_NONE)
        self._attach()

    def _attach(self):
        if self.shared:
            self.viewer = self.ptamd.DeviceContext(0)
            self.ctx = self.viewer
            self.r = self.ptamd.Renderer(self.viewer, self.ptamd.SharedScene(self.viewer, self.g), W, H, with_f32=True)
        elif self.viewer is None:
            self.ctx, self.viewer = self.owner, self.owner
            self.r = self.ptamd.Renderer(self.owner, self.g, W, H, with_f32=True)

    def detach(self):
        if self.shared and self.viewer is not None:
            self.r = None
            self.viewer.close(); self.viewer = None

    def frame(self, flags=0):
        return _frame(self.ptamd, self.ctx, self.r, self.gs, flags)

    def upload_objects(self, invalidate=True):
        self.owner.sync()
        self.g.object_data.copy_(self.ptamd.to_device(self.desc.object_data, self.g.device))     # in place: same device pointer, same count
        self.owner.sync()
        if invalidate:
            self.owner.invalidate_object_data()                                                  # reaches the contexts that view the scene too

    def close(self):
        self.detach()
        self.g.close()
        self.owner.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
def test_transmission_fact_follows_the_object_data(ptamd, pkg, shared):
    rig = _Rig(ptamd, pkg, shared)
    try:
        first = rig.frame()
        _same(first, rig.frame(GENERIC), "plain box")
        rig.desc.object_data[SHORT_BOX]["Material"]["Transmission"] = 1.0
        # rewritten in place and not announced: the rounds are still planned for a scene without transmission, so this is not yet the frame of
        # the glass box -- which shows that the plain box does run the kernel without the third lobe (the generic one reads
        # Material.Transmission at every hit and would render the glass, announced or not)
        rig.upload_objects(invalidate=False)
        stale = rig.frame()
        rig.owner.invalidate_object_data()
        glass = rig.frame()
        assert _differ(glass, first) and _differ(glass, stale)
        _same(glass, rig.frame(GENERIC), "glass box")
        rig.desc.object_data[SHORT_BOX]["Material"]["Transmission"] = 0.0
        rig.upload_objects()
        _same(rig.frame(), first, "back to the plain box")
    finally:
        rig.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
def test_alpha_fact_follows_the_bottom_levels(ptamd, pkg, shared):
    rig = _Rig(ptamd, pkg, shared)
    try:
        first = rig.frame()
        wall = rig.desc.nodes[LEFT_WALL].meshes[0]

        def set_wall(alpha_mode, cutoff):
            """The left wall's geometry with / without the OPAQUE flag (Scene._geometry_descs reads AlphaMode), through a rebuild of its bottom
            level under its id and a new top level. Cut-off 2: the alpha test rejects every candidate, the wall is not there for any ray."""
            rig.detach()
            wall.material["AlphaMode"] = alpha_mode
            rig.desc.object_data[LEFT_WALL]["Material"]["AlphaMode"] = alpha_mode
            rig.desc.object_data[LEFT_WALL]["Material"]["AlphaCutoff"] = cutoff
            rig.upload_objects()
            rig.g.UpdateAccelerationStructures(LEFT_WALL)
            rig.owner.sync()
            rig._attach()

        set_wall(1, 2.0)
        gone = rig.frame()
        assert _differ(gone, first)                 # a frame still planned without the alpha test would have kept the wall
        _same(gone, rig.frame(GENERIC), "wall without the OPAQUE flag")
        set_wall(0, 0.5)
        _same(rig.frame(), first, "back to the opaque wall")
    finally:
        rig.close()
