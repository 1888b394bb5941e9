"""The G-buffer pass against tests/surfaceref.py, a float64 restatement of the primary surface taken from the shaders: the CPU oracle here,
the HIP kernel (k_gbuffer, reconstruct_hit, generate_pinhole_ray) under -m gpu. The scenes are the ones the parity scenes lack: mirrored and
strongly non-uniform instances, a hidden instance, 32-bit indices, moving instances, vertices and camera, finite and infinite far planes."""
import numpy as np
import pytest

import surfaceref as R

W, H = R.SIZE
UNSAFE_CAP = 0.03
_cache = {}


def reference(pkg, name):
    """(scene, Surface, its render) of a scene of surfaceref.SCENES, computed once"""
    if name not in _cache:
        scene = R.SCENES[name](pkg.scenes)
        surface = R.Surface(scene)
        _cache[name] = (scene, surface, surface.render(scene.camera, W, H))
    return _cache[name]


def oracle_gbuffer(oracle, pkg, scene, camera=None):
    L = pkg.layouts
    gb = {k: np.zeros((H, W, c), dt) for k, (dt, c) in L.GBUFFER_FORMATS.items()}
    k = np.zeros((), L.GBUFFER_CONSTANTS)
    k["RenderSize"] = (W, H); k["Flags"] = 0xFFFFFFFF
    o = oracle.OracleScene(scene)
    o.gbuffer(k, gb, camera=camera)
    o.close()
    return gb


def oracle_textures(oracle, pkg, name):
    if ("oracle", name) not in _cache:
        _cache["oracle", name] = oracle_gbuffer(oracle, pkg, reference(pkg, name)[0])
    return _cache["oracle", name]


def assert_matches(gb, ref, surface, what):
    fails, fig = R.compare(gb, ref, surface)
    assert ref["hit"].any() and (~ref["hit"]).any(), what
    assert fig["unsafe_share"] <= UNSAFE_CAP, f"{what}: {fig['unsafe_share']:.4%} of the hit pixels are unsafe"
    assert not fails, f"{what}: kept pixels outside tolerance {fails}; unsafe share {fig['unsafe_share']:.4%}, figures {fig}"
    return fig


@pytest.mark.parametrize("name", list(R.SCENES))
def test_oracle_gbuffer_matches_float64(name, oracle, pkg):
    scene, surface, ref = reference(pkg, name)
    fig = assert_matches(oracle_textures(oracle, pkg, name), ref, surface, name)
    print(name, fig)
    if name.startswith("depth"):
        assert (~ref["hit"]).mean() >= 0.25                                # a quarter of the frame and more looks past the geometry
    if name == "moved":
        m = np.abs(ref["motion"][ref["hit"], :2]).max()
        assert m > 4.0, m                                                  # the motion is pixels, not rounding


def test_far_plane_clips(pkg):
    """the finite far plane really ends rays the infinite one lets through"""
    assert reference(pkg, "depth_far50")[2]["hit"].sum() < reference(pkg, "depth_infinite")[2]["hit"].sum()


@pytest.mark.parametrize("name", list(R.SCENES) + ["scale_far", "scale_near"])
def test_position_lies_within_its_offset_of_the_plane(name, oracle, pkg):
    """SelfIntersectionAvoidance's claim: the stored position is no further from the exact plane of its triangle than its own
    PositionOffset. `scale` puts that to a fan of 1e-2 units at 1e3 and to one of 1e-3 units at the origin: it holds at both on the CPU
    oracle (the distance stays below 0.15 of the offset in every scene here), so no scale limit is recorded."""
    if name.startswith("scale"):
        if "scale" not in _cache:
            scene, cams = R.scale(pkg.scenes)
            _cache["scale"] = (scene, cams, R.Surface(scene))
        scene, cams, surface = _cache["scale"]
        cam = cams[name[len("scale_"):]]
        ref = surface.render(cam, W, H)
        gb = oracle_gbuffer(oracle, pkg, scene, camera=cam)
        ref["unsafe"] = ref["unsafe"] & False                              # one planar fan per camera: every candidate shares the plane
    else:
        scene, surface, ref = reference(pkg, name)
        gb = oracle_textures(oracle, pkg, name)
    P = gb["Position"].reshape(-1, 4).astype(np.float64)
    on = ref["hit"] & np.isfinite(P[:, 3]) & ~ref["unsafe"]
    assert on.sum() > 500, name
    distance = np.abs(R.dot(P[on, :3] - surface.tris.world[ref["tri"][on], 0], ref["flat"][on]))
    assert (P[on, 3] > 0).all()
    worst = (distance / P[on, 3]).max()
    assert worst <= 1.0, f"{name}: a position lies {worst:.3f} of its PositionOffset off its triangle's plane"


MUTATION_SCENE = {"normal_by_matrix": "transformed", "no_front_flip": "transformed", "mv_current_camera": "moved",
                  "mv_no_vertex_term": "moved", "v_not_flipped": "moved"}


assert set(MUTATION_SCENE) == set(R.MUTATIONS) - set(R.TEXTURE_MUTATIONS)                              # those: tests/test_textured_estimator.py


@pytest.mark.parametrize("mutation", list(MUTATION_SCENE))
def test_mutated_surface_is_caught(mutation, oracle, pkg):
    name = MUTATION_SCENE[mutation]
    scene, surface, ref = reference(pkg, name)
    wrong = R.Surface(scene, **{mutation: True})
    fails, _ = R.compare(oracle_textures(oracle, pkg, name), wrong.render(scene.camera, W, H), wrong)
    assert fails, f"the comparison on {name} does not notice {mutation}"
    print(mutation, fails)


GB_KEYS = ("Position", "FlatNormal", "GeometricNormal", "LinearDepth", "NormalizedDepth", "MotionVector", "BaseColorMetalness",
           "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "IOR", "Transmission", "Radiance")


def gpu_gbuffer(ptamd, ctx, scene, sharding):
    """Renderer.gbuffer.Render with every flag set, under the sharding given; the local rows of every G-buffer texture"""
    ctx.set_sharding(*sharding)
    try:
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W, H)
        r.constants["Flags"] = 0xFFFFFFFF
        r.gbuffer.Render(g.GetTopLevelAccelerationStructure(), r.constants)
        ctx.sync()
        out = ptamd.textures_to_numpy({k: r.textures[k] for k in GB_KEYS})
        g.close()
    finally:
        ctx.set_sharding(0, 1, 16)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.SCENES))
def test_gpu_gbuffer_matches_float64(name, gpu, ptamd, oracle, pkg):
    import dxpbrt_amd.sharding as SH
    scene, surface, ref = reference(pkg, name)
    want = oracle_textures(oracle, pkg, name)
    whole = gpu_gbuffer(ptamd, gpu, scene, (0, 1, 16))
    pieces = [gpu_gbuffer(ptamd, gpu, scene, (rank, 2, 8)) for rank in range(2)]
    banded = {k: SH.deinterleave([p[k] for p in pieces], H, 8) for k in GB_KEYS}
    for what, gb in (("unsharded", whole), ("two ranks, bands of 8", banded)):
        assert_matches(gb, ref, surface, f"{name}, {what}")
        for k in GB_KEYS:
            a, b = gb[k], want[k]
            if a.dtype.kind == "f":
                a, b = a.view(np.uint32), b.view(np.uint32)
            assert np.array_equal(a, b), f"{name}, {what}: G-buffer texture {k} differs from the oracle"
