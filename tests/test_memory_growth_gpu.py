"""Context-owned device memory grows through one helper (csrc/pt_memory.hpp grow()): fresh buffers, one wait, moved in. Here every group
of buffers that grows with the frame, the cache, the top level or the animation states is taken small -> large -> small on ONE context,
and every frame of the sequence must equal, byte for byte, the frame of a fresh context that only ever saw that step -- a buffer that
grew, or one larger than its frame needs, changes nothing a caller can see. Frame sizes: 17 x 9 (ragged, less than a tile), 64 x 40
(several tiles), 17 x 9 again. Three frames in flight, as the benchmark renders.

The helper's own contract, the refused growth among it, is pt_memory_check's (the stand-alone program of csrc/Makefile), run here on the
device. No test exhausts memory through the library."""
import numpy as np
import pytest

from test_memory_growth import run_check

SIZES = [(17, 9), (64, 40), (17, 9)]
FIXED = (37, 23)                               # the frame of the groups whose growth is not the frame's


def _copy(ptamd, textures):
    return {k: v.copy() for k, v in ptamd.textures_to_numpy(textures).items()}


def _assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, k)


def assert_sequence_equals_fresh_contexts(ptamd, steps, run):
    """run(ctx, step) -> {name: array}: one context through `steps` in order, against a fresh context per distinct step (computed once)"""
    def context():
        ctx = ptamd.DeviceContext(0)
        ctx.set_sharding(0, 1, 16)
        ctx.set_frames_in_flight(3)
        return ctx

    grown = context()
    try:
        got = [run(grown, step) for step in steps]
    finally:
        grown.close()
    fresh = {}
    for step in steps:
        if step not in fresh:
            ctx = context()
            try:
                fresh[step] = run(ctx, step)
            finally:
                ctx.close()
    for i, step in enumerate(steps):
        assert any(np.ascontiguousarray(v).view(np.uint8).any() for v in got[i].values()), (i, step)      # the frame holds something
        _assert_same(got[i], fresh[step], f"step {i}: {step}")


def _render(ptamd, ctx, scene, size, frames, outputs=None, renderer=None, **kw):
    """`frames` settings rendered in turn by one renderer on ctx: every texture of every frame, the ray counts, and what outputs(r) adds"""
    W, H = size
    g = ptamd.Scene(ctx, scene)
    out = {}
    try:
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True, **(renderer or {}))
        for f, gs in enumerate(frames):
            ctx.reset_counters()
            r.render(gs, **kw)
            ctx.sync()
            c = ctx.counters()
            out.update({f"{k}[{f}]": v for k, v in _copy(ptamd, r.textures).items()})
            out[f"rays[{f}]"] = np.array([c.PrimaryRays, c.SecondaryRays], np.uint64)
            if outputs:
                out.update({f"{k}[{f}]": v for k, v in outputs(r).items()})
        del r
    finally:
        g.close()
    return out


def _settings(S, size, frame=3, spp=4, bounces=4, **fields):
    gs = S.graphics_settings(size[0], size[1], spp=spp, bounces=bounces, frame_index=frame)
    for k, v in fields.items():
        gs[k] = v
    return gs


@pytest.mark.gpu
def test_growth_contract_on_the_device():
    status, lines = run_check()
    assert lines[0] == "mode: device"
    steps = lines[1:]
    assert len(steps) == 9 and all(s.startswith("ok: ") for s in steps), steps
    assert [s[4] for s in steps] == list("112333345")
    assert status == 0


@pytest.mark.gpu
@pytest.mark.parametrize("denoiser", [0, 3], ids=["none", "nrd_relax"])
def test_path_tracer_through_a_larger_frame_and_back(denoiser, ptamd, pkg):
    """the path queues, the primary records, the counters and, with a denoiser, the per-pixel aux words"""
    S = pkg.scenes

    def run(ctx, size):
        scene = S.cornell_box(aspect=size[0] / size[1], variant="ggx", glass_sphere=True)
        return _render(ptamd, ctx, scene, size, [_settings(S, size, Denoiser=denoiser)])
    assert_sequence_equals_fresh_contexts(ptamd, SIZES, run)


@pytest.mark.gpu
def test_reservoir_reuse_through_a_larger_frame_and_back(ptamd, pkg):
    """temporal and spatial reuse, two frames per size: the first frame after the reservoirs grew is a first frame (no history), the second
    reuses it"""
    S, L = pkg.scenes, pkg.layouts

    def run(ctx, size):
        scene = S.cornell_box(aspect=size[0] / size[1], variant="ggx")
        frames = [_settings(S, size, frame=f, spp=1, bounces=2, IsDIEnabled=1) for f in (0, 1)]
        return _render(ptamd, ctx, scene, size, frames, renderer=dict(di_history=True), di_samples=4, di_reuse=L.di_resampling_settings(),
                       outputs=lambda r: {"reservoirs": r.direct_lighting.download_reservoirs()})
    assert_sequence_equals_fresh_contexts(ptamd, SIZES, run)


@pytest.mark.gpu
def test_brdf_candidates_through_a_larger_frame_and_back(ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts

    def run(ctx, size):
        scene = S.cornell_box(aspect=size[0] / size[1], variant="ggx")
        frames = [_settings(S, size, spp=1, bounces=2, IsDIEnabled=1)]
        return _render(ptamd, ctx, scene, size, frames, di_samples=4, di_brdf=L.di_brdf_settings(samples=2),
                       outputs=lambda r: {"candidates": r.direct_lighting.download_brdf_candidates()})
    assert_sequence_equals_fresh_contexts(ptamd, SIZES, run)


@pytest.mark.gpu
def test_sharc_through_a_larger_cache_and_back(ptamd, pkg):
    """Configure(1 << 15), (1 << 16), (1 << 15), two frames through the cache after each; the second frame of each reads what the first
    left in the cache. What is compared is what the frames write and how many entries live. The entries' own bytes are not: at these
    capacities they differ between two fresh contexts too (measured: the first step, itself a fresh context, against the fresh one)."""
    S, L = pkg.scenes, pkg.layouts
    scene = S.cornell_box(aspect=FIXED[0] / FIXED[1], variant="diffuse")

    def run(ctx, capacity):
        ctx.check(ctx.lib.pt_sharc_configure(ctx.handle, capacity))
        frames = [_settings(S, FIXED, frame=f, spp=2, bounces=5) for f in (0, 1)]
        return _render(ptamd, ctx, scene, FIXED, frames, sharc=L.sharc_settings(downscale=2),
                       outputs=lambda r: {"live entries": np.array([len(r.sharc.download())])})
    assert_sequence_equals_fresh_contexts(ptamd, [1 << 15, 1 << 16, 1 << 15], run)


@pytest.mark.gpu
def test_top_level_through_more_instances_and_back(ptamd, pkg):
    """2, 40 and 2 instances: the instance records, the top level's nodes and the build's upload"""
    S = pkg.scenes
    full = S.instanced_grid(n=7, aspect=FIXED[0] / FIXED[1], subdiv=1)             # 49 spheres, then the ground and the light

    def run(ctx, count):
        objects = full.objects[-2:] + full.objects[:count - 2]
        scene = S.Scene(full.nodes, objects, full.camera, full.scene_data, name=f"grid of {count}").finalize()
        out = _render(ptamd, ctx, scene, FIXED, [_settings(S, FIXED)])
        out["instances"] = np.array([len(objects)])
        return out
    assert_sequence_equals_fresh_contexts(ptamd, [2, 40, 2], run)


@pytest.mark.gpu
def test_animation_states_through_more_objects_and_back(ptamd, pkg):
    """pt_anim_evaluate with 1, 5 and 1 states: the device copy of the states"""
    obj = pkg.scenes.animated_scene().animations[0]

    def run(ctx, count):
        anim = ptamd.Animation(ctx, [obj] * count)
        try:
            for i in range(count):
                anim.SetSelectedIndex(i, i % 2)
                anim.SetTime(0.15 + 0.2 * i, i)
            anim.Evaluate(None)
            return {f"globals[{i}]": anim.download_globals(i) for i in range(count)}
        finally:
            anim.close()
    assert_sequence_equals_fresh_contexts(ptamd, [1, 5, 1], run)
