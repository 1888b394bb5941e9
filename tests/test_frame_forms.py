"""The template and schedule matrix of a frame: every form the host launch path can give a frame (fused or streaming, flat or phased, one
fused kernel or the k_shade + k_extend2 pair, the statistics variants, several chains) under every kernel instantiation the run-time
switches select (direct lighting off / on, SHARC query off / on, textured or not).

The comparisons are the library against itself under other schedules, bit for bit, which is how test_traversal_schedules_agree pins the
plain path: within a cell (direct lighting, SHARC) every schedule must give the same RadianceF32 and the same SecondaryRays; with direct
lighting off, the query of an empty cache is the plain render. A wrong rung in a variant dispatch, or a launcher that reads a stale frame
input, shows as a differing image or ray count here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATS, V1, PHASED, UNFUSED, LOCKSTEP, SHARC_SKIP_UPDATE = 0x1, 0x4, 0x8, 0x10, 0x20, 0x200
BLOB_LDS_MAX, FLAT_INSTANCES = 40 * 1024, 32          # pt_kernels.hip kBlobLdsMax, pt_trace2.hpp kFlatInstances

# name: (scene, (W, H), streaming, phased). The class is asserted through accel_stats(): BlobBytes against 40 KiB, InstanceCount against 32.
SCENES = {
    "fused_flat": (lambda S, a: S.cornell_box(aspect=a, variant="ggx", glass_sphere=True), (96, 64), False, False),
    "fused_flat_textured": (lambda S, a: S.cornell_box_textured(env=None, aspect=a), (96, 64), False, False),
    "fused_phased": (lambda S, a: S.instanced_grid(n=6, aspect=a, subdiv=1), (96, 64), False, True),   # the smallest n beyond 32 instances: 38 (n = 8 has 45 008 B, beyond LDS)
    "streaming_flat": (lambda S, a: S.sponza_scale(n_side=48, aspect=a), (128, 80), True, False),
    "streaming_phased": (lambda S, a: S.instanced_grid(n=24, aspect=a), (128, 80), True, True),
}
CHAINED = ("fused_flat", "streaming_flat")             # the direct-lighting + SHARC cell again with pt_set_round_chains(3)


# Frames that do not fill a tile (tests/test_frame_edges.py): 37 x 23 cuts the 16 x 16 block and the 8 x 8 wave tile on both axes and leaves 83 pixels
# in the last 256-pixel queue tile; 17 x 5 is less than one workgroup -- one queue tile, a wave of 21 lanes and two empty ones, and more sub-queues
# than tiles in every form.
RAGGED_SIZES = [(37, 23), (17, 5)]
RAGGED_SCENES = ("fused_flat", "fused_phased", "streaming_flat", "streaming_phased")


def _forms_agree(ptamd, pkg, name, size=None):
    """size: None, the scene's own; or a frame size, at which every texture and the primary rays are compared too, not RadianceF32 and the
    secondary rays alone"""
    S, L = pkg.scenes, pkg.layouts
    make, (W, H), streaming, phased = SCENES[name]
    every_texture = size is not None
    if size is not None:
        W, H = size
    ctx = ptamd.DeviceContext(0)                        # a context of its own: debug flags, chains and the cache do not leak into other tests
    try:
        g = ptamd.Scene(ctx, make(S, W / H))
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True)
        r.sharc.Configure(1 << 16)
        st = ctx.accel_stats()
        assert (st.BlobBytes > BLOB_LDS_MAX) == streaming and (st.InstanceCount > FLAT_INSTANCES) == phased, (st.BlobBytes, st.InstanceCount)

        def frame(di, sharc, flags):
            gs = S.graphics_settings(W, H, spp=2, bounces=5)
            gs["IsDIEnabled"] = 1 if di else 0
            try:
                ctx.set_debug_flags(flags | (SHARC_SKIP_UPDATE if sharc else 0))      # the cache stays empty
                ctx.reset_counters()
                r.render(gs, di_samples=4 if di else 0, sharc=L.sharc_settings() if sharc else None)
                ctx.sync()
            finally:
                ctx.set_debug_flags(0)
            c = ctx.counters()
            assert c.StackOverflows == 0
            if every_texture:
                assert c.PrimaryRays == W * H
                return np.concatenate([a.reshape(-1).view(np.uint8) for _, a in sorted(ptamd.textures_to_numpy(r.textures).items())]), c.SecondaryRays
            return ptamd.textures_to_numpy({"RadianceF32": r.textures["RadianceF32"]})["RadianceF32"].view(np.uint32).copy(), c.SecondaryRays

        cells = {}
        for di in (False, True):
            for sharc in (False, True):
                schedules = [0, PHASED, UNFUSED, UNFUSED | PHASED, STATS]
                if streaming:
                    schedules += [LOCKSTEP, LOCKSTEP | STATS]
                if not sharc:
                    schedules += [V1]                   # (the SHARC entry point refuses it: no hit distance)
                img, rays = cells[di, sharc] = frame(di, sharc, 0)
                assert rays > 0
                for flags in schedules[1:]:
                    other, other_rays = frame(di, sharc, flags)
                    assert other_rays == rays and np.array_equal(other, img), (di, sharc, hex(flags))
        assert cells[False, True][1] == cells[False, False][1] and np.array_equal(cells[False, True][0], cells[False, False][0])

        if name in CHAINED:                             # default stream: three chains launched one after the other
            try:
                ctx.set_round_chains(3)
                img, rays = frame(True, True, 0)
            finally:
                ctx.set_round_chains(0)
            assert rays == cells[True, True][1] and np.array_equal(img, cells[True, True][0])
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_frame_forms_agree(ptamd, pkg, name):
    _forms_agree(ptamd, pkg, name)


@pytest.mark.parametrize("size", RAGGED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", RAGGED_SCENES)
def test_frame_forms_agree_at_ragged_sizes(ptamd, pkg, name, size):
    """the same matrix -- the class assertion through accel_stats() included, so the small frame really takes the form its scene claims --
    with every output texture compared byte for byte"""
    _forms_agree(ptamd, pkg, name, size)
