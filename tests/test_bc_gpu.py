"""Block-compressed textures on the GPU: a BC1 / BC3 texture samples to exactly the bits of its RGBA8(_SRGB) expansion, a BC4 / BC5 texture
to the bits of its R32G32B32A32_FLOAT expansion (DESIGN.md "Arithmetic spec"). Every case renders twice, once with the block texture and
once with bc.decode's expansion in the matching existing format, and every output must be byte-identical; the small cases are also held
against the oracle's render of the expansion scene, bit for bit like the existing parity tests."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import bcscene

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
W_IMG = 64
SIZES = [(4, 4), (10, 7), (12, 20)]                     # (w, h): every wrap tap in one block; partial edge blocks; several blocks both ways
UNFUSED, LOCKSTEP = 0x10, 0x20                          # debug flags (tests/test_frame_forms.py)
BLOB_LDS_MAX = 40 * 1024
GB_EXACT = ("Position", "FlatNormal", "GeometricNormal", "LinearDepth", "NormalizedDepth", "BaseColorMetalness", "NormalRoughness", "IOR",
            "Transmission", "Radiance")


@pytest.fixture(scope="module")
def bc(pkg):
    import dxpbrt_amd.bc as m
    return m


def render(ptamd, ctx, S, scene, W=W_IMG, H=W_IMG, spp=2, bounces=3, flags=0, di=0, stats=None):
    """every texture the frame writes as bytes, and the ray counts; stats: a dict that receives the scene's BlobBytes"""
    ctx.set_sharding(0, 1, 16)
    g = ptamd.Scene(ctx, scene)
    try:
        r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=bool(di))
        gs = S.graphics_settings(W, H, spp=spp, bounces=bounces)
        gs["IsDIEnabled"] = 1 if di else 0
        try:
            ctx.set_debug_flags(flags)
            ctx.reset_counters()
            r.render(gs, di_samples=di)
            ctx.sync()
        finally:
            ctx.set_debug_flags(0)
        c = ctx.counters()
        assert c.StackOverflows == 0
        if stats is not None:
            stats["BlobBytes"] = ctx.accel_stats().BlobBytes
        out = {k: np.ascontiguousarray(v).view(np.uint8).copy() for k, v in ptamd.textures_to_numpy(r.textures).items()}
        return out, (c.PrimaryRays, c.SecondaryRays)
    finally:
        g.close()


def assert_same_frame(a, b, what):
    (ta, ra), (tb, rb) = a, b
    assert ra == rb, (what, "ray counts", ra, rb)
    assert set(ta) == set(tb)
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), (what, k, int((ta[k] != tb[k]).sum()))


def assert_matches_oracle(oracle, pkg, frame, scene, what, spp=2, bounces=3):
    S, L = pkg.scenes, pkg.layouts
    gb, rays, f32 = oracle.render(scene, S.graphics_settings(W_IMG, W_IMG, spp=spp, bounces=bounces), accel_mode=0, want_f32=True, layouts=L)
    tex, (primary, secondary) = frame
    assert primary + secondary == rays, what
    for k in GB_EXACT:
        assert np.array_equal(tex[k], np.ascontiguousarray(gb[k]).view(np.uint8)), (what, k)
    assert np.array_equal(tex["RadianceF32"], np.ascontiguousarray(f32).view(np.uint8)), (what, "RadianceF32")


def expanded(bc, S, scene_builder):
    """the scene built again with every block texture replaced by its expansion"""
    return bcscene.swap_textures(bc, scene_builder(), lambda t: bc.expansion(t) if isinstance(t, S.BlockTexture) else t)


def slots_a(bc, S, w, h, seed):
    """base colour, emissive (second coordinate set), packed metallic-roughness, normal"""
    t = lambda fmt, k: bcscene.random_texture(bc, S, fmt, w, h, seed + k)       # noqa: E731
    return {"BaseColor": (t(S.FMT_BC3_UNORM_SRGB, 0), 0), "EmissiveColor": (t(S.FMT_BC1_UNORM_SRGB, 1), 1),
            "MetallicRoughness": (t(S.FMT_BC1_UNORM, 2), 0), "Normal": (t(S.FMT_BC5_UNORM, 3), 0)}


def slots_b(bc, S, w, h, seed):
    """base colour BC1, separate metallic / roughness / transmission maps as BC4, a BC3 emissive on the second set"""
    t = lambda fmt, k: bcscene.random_texture(bc, S, fmt, w, h, seed + k)       # noqa: E731
    return {"BaseColor": (t(S.FMT_BC1_UNORM_SRGB, 0), 1), "Metallic": (t(S.FMT_BC4_UNORM, 1), 0), "Roughness": (t(S.FMT_BC4_UNORM, 2), 0),
            "Transmission": (t(S.FMT_BC4_UNORM, 3), 0), "EmissiveColor": (t(S.FMT_BC3_UNORM, 4), 1), "Normal": (t(S.FMT_BC5_UNORM, 5), 0)}


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("which", ["a", "b"])
def test_block_textures_render_the_bits_of_their_expansion(gpu, ptamd, oracle, pkg, bc, which, w, h):
    S = pkg.scenes
    if which == "a":
        mat = S.material((1, 1, 1), emissive=(1, 0.9, 0.8), strength=2.0, metallic=0.8, roughness=0.7)
        build = lambda: bcscene.quad_scene(S, mat, slots_a(bc, S, w, h, 10 * w + h))                        # noqa: E731
    else:
        mat = S.material((1, 1, 1), emissive=(0.5, 0.5, 0.5), strength=1.5, metallic=0.9, roughness=0.9, transmission=0.8)
        build = lambda: bcscene.quad_scene(S, mat, slots_b(bc, S, w, h, 20 * w + h))                        # noqa: E731
    scene = build()
    if (w, h) == (12, 20):                              # a condition on the inputs: both modes of every switch occur in the BC3 and BC5 textures
        for slot, (t, _) in scene.nodes[0].meshes[0].textures.items():
            for name, f in bcscene.mode_fractions(bc, t.data, t.fmt).items():
                assert 0.2 <= f <= 0.8, (slot, name, f)
    for item in scene.heap:                             # the buffers hold exactly the blocks
        if item.kind == S.KIND_TEXTURE2D:
            assert item.array.nbytes == bc.block_count(w, h) * S.FMT_BLOCK_BYTES[item.fmt]
    flat = expanded(bc, S, build)
    assert {item.fmt for item in flat.heap if item.kind == S.KIND_TEXTURE2D} <= {S.FMT_RGBA8_UNORM, S.FMT_RGBA8_UNORM_SRGB, S.FMT_RGBA32_FLOAT}
    got = render(ptamd, gpu, S, scene)
    assert_same_frame(got, render(ptamd, gpu, S, flat), (which, w, h))
    assert np.isfinite(got[0]["Position"].view(np.float32)).any() and got[1][1] > 0
    assert_matches_oracle(oracle, pkg, got, flat, (which, w, h))
    # the k_shade + k_extend2 pair instead of the fused round
    assert_same_frame(render(ptamd, gpu, S, scene, flags=UNFUSED), got, (which, w, h, "unfused"))


def test_bc1_three_colour_alpha_cuts_the_quad(gpu, ptamd, oracle, pkg, bc):
    """AlphaMode mask over a BC1_SRGB base colour whose three-colour blocks carry transparent texels: the closest-hit alpha test decides
    the coverage of the quad, and a pane behind it shows through the holes."""
    S = pkg.scenes
    masked = S.material((1, 1, 1)); masked["AlphaMode"] = 1; masked["AlphaCutoff"] = 0.5
    back = S.material((0.2, 0.8, 0.3))

    def build():
        tex = bcscene.random_texture(bc, S, S.FMT_BC1_UNORM_SRGB, 12, 20, 77)
        return bcscene.quad_scene(S, masked, {"BaseColor": (tex, 0)}, extra=[(2.0, back, {}, 0.0)])
    scene = build()
    f = bcscene.mode_fractions(bc, scene.nodes[0].meshes[0].textures["BaseColor"][0].data, S.FMT_BC1_UNORM_SRGB)["c0>c1"]
    assert 0.2 <= f <= 0.8
    flat = expanded(bc, S, build)
    got = render(ptamd, gpu, S, scene)
    assert_same_frame(got, render(ptamd, gpu, S, flat), "alpha mask")
    assert_matches_oracle(oracle, pkg, got, flat, "alpha mask")
    depth = got[0]["Position"].view(np.float32).reshape(W_IMG, W_IMG, -1)[..., 2]
    front, behind = int((np.abs(depth - 1.0) < 1e-3).sum()), int((np.abs(depth - 2.0) < 1e-3).sum())
    assert front > 200 and behind > 20, (front, behind)                  # the mask opens part of the quad (an eighth of the texels is transparent), not all of it


def visibility_rays(n=4000, seed=3):
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3)); o[:, 2] = -1.0
    target = np.concatenate([rng.uniform(-0.78, 0.78, (n, 2)), np.ones((n, 1))], 1)
    dd = target - o; ln = np.linalg.norm(dd, axis=1, keepdims=True); dd /= ln
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = o; rays[:, 3] = 1e-3; rays[:, 4:7] = dd; rays[:, 7] = ln[:, 0] + 1.5
    return rays


def trace_visibility(ptamd, ctx, scene, rays):
    import torch
    ctx.set_sharding(0, 1, 16)
    g = ptamd.Scene(ctx, scene)
    try:
        dr = torch.from_numpy(rays).cuda(); dv = torch.zeros((len(rays), 4), dtype=torch.float32, device="cuda")
        ctx.check(ctx.lib.pt_trace_visibility(ctx.handle, C.c_void_p(dr.data_ptr()), len(rays), C.c_void_p(dv.data_ptr())))
        ctx.sync()
        return dv.cpu().numpy()
    finally:
        g.close()


def test_shadow_rays_through_block_textured_panes(gpu, ptamd, oracle, pkg, bc):
    """pt_trace_visibility (the coloured-visibility IsOpaque of a shadow ray) through two panes, the arrangement of
    test_gpu_visibility_through_textured_panes with block textures: an alpha-masked BC1 / BC3 pane in front of a pane that transmits
    through BC4 transmission and metallic maps under a BC3 base colour."""
    S = pkg.scenes
    masked = S.material((1, 1, 1)); masked["AlphaMode"] = 1; masked["AlphaCutoff"] = 0.5
    glass = S.material((0.9, 0.95, 1.0), metallic=0.6, transmission=1.0)
    rays = visibility_rays()
    for front_fmt in (S.FMT_BC1_UNORM_SRGB, S.FMT_BC3_UNORM_SRGB):
        def build():
            t = lambda fmt, k: bcscene.random_texture(bc, S, fmt, 10, 7, 300 + k)       # noqa: E731
            return bcscene.quad_scene(S, masked, {"BaseColor": (t(front_fmt, front_fmt), 0)},
                                      extra=[(1.5, glass, {"BaseColor": (t(S.FMT_BC3_UNORM_SRGB, 1), 1), "Transmission": (t(S.FMT_BC4_UNORM, 2), 0),
                                                           "Metallic": (t(S.FMT_BC4_UNORM, 3), 0)}, 0.0)])
        flat = expanded(bc, S, build)
        got = trace_visibility(ptamd, gpu, build(), rays)
        want = trace_visibility(ptamd, gpu, flat, rays)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), front_fmt
        ref = np.zeros((len(rays), 4), np.float32)
        osc = oracle.OracleScene(flat, accel_mode=0)
        oracle.lib().or_trace_visibility(osc.handle, rays.ctypes.data, len(rays), ref.ctypes.data)
        osc.close()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), front_fmt
        blocked = got[:, 3] != 1.0
        partial = (got[:, :3].max(1) > 0) & (got[:, :3].max(1) < 1)
        assert blocked.mean() > 0.1 and partial.mean() > 0.02, (blocked.mean(), partial.mean())      # both panes decide rays


def test_streaming_form_samples_block_textures(ptamd, pkg, bc):
    """k_shade<true> / k_extend_stream: a scene whose bottom level does not fit LDS (what makes tests/test_frame_forms.py's streaming scenes
    stream), base colour BC3_SRGB with an alpha lattice on the masked strips (the alpha test inside the traversal), normals BC5,
    metallic-roughness BC1."""
    S = pkg.scenes
    fmts = {"BaseColor": S.FMT_BC3_UNORM_SRGB, "Normal": S.FMT_BC5_UNORM, "MetallicRoughness": S.FMT_BC1_UNORM}
    W, H = 128, 80

    def build():
        sc = S.sponza_scale(n_side=48, aspect=W / H, textured=True, texture_size=20)
        return bc.map_textures(sc, lambda slot, t: bc.block_texture(t, fmts[slot]))
    ctx = ptamd.DeviceContext(0)                        # debug flags stay in a context of their own
    try:
        scene, flat = build(), expanded(bc, S, build)
        stats = {}
        got = render(ptamd, ctx, S, scene, W, H, spp=2, bounces=3, stats=stats)
        assert stats["BlobBytes"] > BLOB_LDS_MAX                # the bottom level does not fit LDS: the frame streams
        assert_same_frame(got, render(ptamd, ctx, S, flat, W, H, spp=2, bounces=3), "streaming")
        assert got[1][1] > 0
        for flags in (LOCKSTEP, UNFUSED):
            assert_same_frame(render(ptamd, ctx, S, scene, W, H, spp=2, bounces=3, flags=flags), got, ("streaming", hex(flags)))
    finally:
        ctx.close()


def test_direct_lighting_from_a_block_textured_emitter(gpu, ptamd, pkg, bc):
    """pt_di_render, 8 candidates: the light records take their radiance from a centroid tap of the emissive texture (BC1_SRGB here)"""
    S = pkg.scenes

    def build():
        sc = S.cornell_box_textured(env=None, aspect=1.0)
        return bc.map_textures(sc, lambda slot, t: bc.block_texture(t, S.FMT_BC1_UNORM_SRGB) if slot == "EmissiveColor" else t)
    scene, flat = build(), expanded(bc, S, build)
    assert S.FMT_BC1_UNORM_SRGB in [item.fmt for item in scene.heap if item.kind == S.KIND_TEXTURE2D]
    got = render(ptamd, gpu, S, scene, spp=1, bounces=2, di=8)
    want = render(ptamd, gpu, S, flat, spp=1, bounces=2, di=8)
    for k in ("Diffuse", "Specular"):
        assert np.array_equal(got[0][k], want[0][k]), k
    assert_same_frame(got, want, "direct lighting")
    assert got[0]["Diffuse"].view(np.float16).astype(np.float32).max() > 0


def test_refused_block_textures_leave_the_descriptor_alone(ptamd, pkg, bc):
    import torch
    S = pkg.scenes
    tex = S.Texture(np.random.default_rng(2).integers(0, 256, (8, 8, 4)).astype(np.uint8), srgb=True)
    scene = bcscene.quad_scene(S, S.material((1, 1, 1)), {"BaseColor": (tex, 0)})
    d = int(scene.object_data[0]["TextureMapInfoArray"][0]["Descriptor"])
    ctx = ptamd.DeviceContext(0)
    try:
        ctx.set_sharding(0, 1, 16)
        g = ptamd.Scene(ctx, scene)
        r = ptamd.Renderer(ctx, g, W_IMG, W_IMG, with_f32=True)

        def frame():
            r.render(S.graphics_settings(W_IMG, W_IMG, spp=1, bounces=1)); ctx.sync()
            return ptamd.textures_to_numpy(r.textures)["RadianceF32"].view(np.uint32).copy()
        before = frame()
        buf = torch.zeros(6 * 64 + 64, dtype=torch.uint8, device="cuda")
        p = buf.data_ptr()
        assert p % 16 == 0
        refused = {"a block-compressed cube": (p, 8, 8, S.FMT_BC1_UNORM, 1), "format 9": (p, 8, 8, 9, 0),
                   "BC1 at 4 bytes": (p + 4, 8, 8, S.FMT_BC1_UNORM_SRGB, 0), "BC4 at 4 bytes": (p + 4, 8, 8, S.FMT_BC4_UNORM, 0),
                   "BC3 at 8 bytes": (p + 8, 8, 8, S.FMT_BC3_UNORM, 0), "BC5 at 8 bytes": (p + 8, 8, 8, S.FMT_BC5_UNORM, 0)}
        for name, (ptr, w, h, fmt, cube) in refused.items():
            st = ctx.lib.pt_heap_set_texture(ctx.handle, d, C.c_void_p(ptr), w, h, fmt, cube)
            assert st != 0, name
            assert len(ctx.lib.pt_last_error(ctx.handle).decode()) > 10, name
            with pytest.raises((ptamd.PtInvalidArgument, ptamd.PtError)):
                ctx.check(st)
        assert np.array_equal(frame(), before)          # the descriptor still names the RGBA8 texture
        g.close()
    finally:
        ctx.close()


def test_cpp_host_renders_a_dds_gltf_like_the_harness(tmp_path, gpu, ptamd, pkg, bc):
    """pt_demo --scene on a glTF whose textures carry MSFT_texture_dds images: header parsing in pt_ingest.hpp, the blocks uploaded under
    their block formats; the same radiance bytes as ingest.py + the Python binding."""
    import dxpbrt_amd.ingest as I
    S = pkg.scenes
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    W, H, spp, bounces = 64, 64, 2, 3
    path, _ = bcscene.dds_gltf(I, S, bc, str(tmp_path))
    out = str(tmp_path / "radiance.bin")
    line = subprocess.check_output([DEMO, "--scene", path, "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces),
                                    "--frames", "1", "--out", out], text=True)
    assert json.loads(line.strip().splitlines()[-1])["host"] == "c++"
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    scene = I.load_scene(path, aspect=W / H)
    assert sorted(item.fmt for item in scene.heap if item.kind == S.KIND_TEXTURE2D) == [S.FMT_BC1_UNORM, S.FMT_BC3_UNORM_SRGB, S.FMT_BC5_UNORM]
    tex, _ = render(ptamd, gpu, S, scene, W, H, spp=spp, bounces=bounces)
    assert np.array_equal(got.view(np.uint8).reshape(-1), tex["RadianceF32"].reshape(-1))
    assert got[..., :3].mean() > 0.01
