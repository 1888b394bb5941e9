"""Direct lighting, pinned per pixel: one emissive triangle and one candidate restated from the documented RNG spec
and checked against the CPU oracle's BSDF evaluate and shadow rays; a scene without emitters; a shared scene; the C++ host's --di frame."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import dipins

M32 = 0xFFFFFFFF


# ---- the RNG of the DI pass, restated (pt_math.hpp Rng::Hash; DI salt 0x44490001) --------------------------------------------
def lowbias32(x):
    x = x & M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32; x ^= x >> 15; x = (x * 0x846CA68B) & M32; x ^= x >> 16
    return x


def di_seed(px, py, frame):
    seed = lowbias32(frame + 0x035F9F29)
    v = ((px << 16) | (py & 0xFFFF)) & M32
    st = seed ^ ((lowbias32(v) + 0x9E3779B9 + ((seed << 6) & M32) + (seed >> 2)) & M32)
    return lowbias32(st ^ 0x44490001)


def di_draws(px, py, frame, n):
    st, out = di_seed(px, py, frame), []
    for _ in range(n):
        st = (st * 1664525 + 1013904223) & M32
        out.append(np.float32(lowbias32(st) >> 8) * np.float32(1.0 / 16777216.0))
    return out


def test_rng_restatement_is_the_path_tracers_generator():
    """The same lowbias32 / LCG the oracle's path tracer uses: the first draws of a known state (not GPU-dependent)."""
    a = di_draws(3, 5, 7, 4)
    b = di_draws(3, 5, 8, 4)
    assert all(0.0 <= x < 1.0 for x in a + b) and a != b
    assert lowbias32(0) == 0 and lowbias32(1) != 1


def _pin_scene(S, L, aspect):
    """a GGX-ish floor, one emissive triangle above it, an opaque bar between them (its shadow is on the floor)"""
    floor = S.quad_mesh((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2), (0, 1, 0), S.material((0.6, 0.5, 0.4), roughness=0.4, metallic=0.3))
    tri = S.Mesh(S.make_vertices(np.array([(-0.6, 1.5, -0.3), (0.7, 1.6, 0.1), (0.0, 1.4, 0.8)], np.float32),
                                 np.tile(np.float32([0, -1, 0]), (3, 1))), S.make_indices([0, 1, 2]), True,
                 S.material((0.5, 0.5, 0.5), emissive=(1.0, 0.8, 0.6), strength=6.0))
    bar = S.quad_mesh((-1.5, 0.7, -0.1), (1.5, 0.7, -0.1), (1.5, 0.7, 0.15), (-1.5, 0.7, 0.15), (0, -1, 0), S.material((0.2, 0.2, 0.2)))
    nodes = [S.MeshNode([floor]), S.MeshNode([tri]), S.MeshNode([bar])]
    ident = S.trs()
    objects = [S.RenderObject(0, ident), S.RenderObject(1, ident), S.RenderObject(2, ident)]
    cam = S.make_camera((0, 2.2, -2.6), forward=(0, -0.6, 1), hfov_deg=70.0, aspect=aspect)
    return S.Scene(nodes, objects, cam, S.make_scene_data((0, 0, 0, 1)), name="di_pin").finalize()


def _snorm(q):
    return np.maximum(q.astype(np.float64) / 32767.0, -1.0)


def _oct_decode(e):
    x, y = e[..., 0], e[..., 1]
    z = 1.0 - np.abs(x) - np.abs(y)
    t = np.maximum(-z, 0.0)
    x = x + np.where(x >= 0, -t, t); y = y + np.where(y >= 0, -t, t)
    v = np.stack([x, y, z], -1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _one_sample_pin(gpu, ptamd, pkg, oracle, W, H):
    """The plain pass with one candidate on a scene with one emissive triangle, restated per pixel from the downloaded G-buffer and light
    record: the sample point from the documented draws, the BSDF from the oracle's evaluate, the shadow ray from the oracle's brute-force
    visibility. The floors on what the frame must show (shadowed and lit floor pixels) are stated for 80 x 60 and taken as the same
    share of another size (dipins.more_than)."""
    S, L = pkg.scenes, pkg.layouts
    frame = 11
    scene = _pin_scene(S, L, W / H)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True)
    di = r.direct_lighting
    r.gbuffer.Render(g.GetTopLevelAccelerationStructure(), r.constants)
    di.SetConstants(L.di_settings(W, H, frame, samples=1))
    di.Render(g.GetTopLevelAccelerationStructure())
    gpu.sync()
    out = ptamd.textures_to_numpy(r.textures)
    lights = di.download_lights()
    assert len(lights) == 1
    lt = lights[0]
    base, e0, e1 = (lt[k].astype(np.float64) for k in ("Base", "Edge0", "Edge1"))
    nrm, area, Le = lt["Normal"].astype(np.float64), float(lt["Area"]), lt["Radiance"].astype(np.float64)

    cam = scene.camera
    p2v, v2w = cam["ProjectionToView"].reshape(4, 4).astype(np.float64), cam["ViewToWorld"].reshape(4, 4).astype(np.float64)
    depth = out["LinearDepth"][..., 0].astype(np.float64)
    nr = out["NormalRoughness"]
    rough = _snorm(nr[..., 3])
    gn = _oct_decode(_snorm(out["GeometricNormal"]))
    sn = _snorm(nr[..., :3])
    bcm = out["BaseColorMetalness"].astype(np.float64) / 255.0
    ior = out["IOR"][..., 0].view(np.float16).astype(np.float64)
    trans = np.where(bcm[..., 3] < 1, out["Transmission"][..., 0].astype(np.float64) / 255.0, 0.0)
    camp = cam["Position"].astype(np.float64)

    pix, queries, rays, pdfs = [], [], [], []
    for y in range(H):
        for x in range(W):
            if not np.isfinite(depth[y, x]) or rough[y, x] < 0.05:
                continue
            u, v = (x + 0.5) / W, (y + 0.5) / H
            q = np.array([u * 2 - 1, v * -2 + 1, 0.5, 1.0]) @ p2v
            P = (np.array([q[0] / q[2] * depth[y, x], q[1] / q[2] * depth[y, x], depth[y, x], 1.0]) @ v2w)[:3]
            V = camp - P; V /= np.linalg.norm(V)
            front = gn[y, x] @ V > 0
            r0, r1, r2, r3 = di_draws(x, y, frame, 4)
            s = np.sqrt(np.float64(r1))
            pos = base + e0 * (s * (1 - r2)) + e1 * (s * r2)
            d = pos - P; dist = np.linalg.norm(d); dn = d / dist
            pdf = (1 / area) * dist * dist / abs(dn @ -nrm)
            pix.append((y, x)); pdfs.append(pdf)
            queries.append(np.concatenate([bcm[y, x, :3], [bcm[y, x, 3], rough[y, x], ior[y, x], trans[y, x], 1.0 if front else 0.0],
                                           gn[y, x], sn[y, x], V, dn]))
            rays.append(np.concatenate([P, [1e-3], dn, [max(0.0, dist - 2e-3)]]))
    assert len(pix) > 0.5 * W * H
    qa = np.ascontiguousarray(np.array(queries, np.float32)); res = np.zeros((len(qa), 8), np.float32)
    oracle.lib().or_bsdf_evaluate(qa.ctypes.data, len(qa), res.ctypes.data)
    ra = np.ascontiguousarray(np.array(rays, np.float32)); vis = np.zeros((len(ra), 4), np.float32)
    osc = oracle.OracleScene(scene, accel_mode=0)
    oracle.lib().or_trace_visibility(osc.handle, ra.ctypes.data, len(ra), vis.ctypes.data)
    osc.close()
    pdfs = np.array(pdfs)
    exp_d = res[:, 0:3].astype(np.float64) * Le / pdfs[:, None] * vis[:, :3]
    exp_s = res[:, 3:6].astype(np.float64) * Le / pdfs[:, None] * vis[:, :3]
    ys, xs = np.array(pix).T
    got_d = out["Diffuse"][ys, xs].view(np.float16).astype(np.float64)
    got_s = out["Specular"][ys, xs].view(np.float16).astype(np.float64)

    occluded = vis[:, 3] == 0
    lit = ~occluded & ((exp_d + exp_s).max(1) > 0)
    print(f"one-sample pin at {W} x {H}: {len(pix)} pixels restated, {int(occluded.sum())} occluded, {int(lit.sum())} lit")
    assert dipins.more_than(occluded.sum(), 20, W, H, 80, 60) and dipins.more_than(lit.sum(), 200, W, H, 80, 60)   # both the shadow and the lit floor are in view
    # occluded: exactly 0 -- except where the float32 surface point of the pass and this float64 one fall on either side of the bar's edge
    flip = occluded & ((got_d[:, :3] != 0).any(1) | (got_s[:, :3] != 0).any(1))
    assert flip.sum() <= max(2, 0.01 * occluded.sum()), flip.sum()
    # ... and the other way round: lit here, shadowed in the pass
    flip = flip | (lit & (got_d[:, :3] == 0).all(1) & (got_s[:, :3] == 0).all(1) & ((exp_d + exp_s).max(1) > 1e-4))
    assert flip.sum() <= max(4, 0.01 * occluded.sum()), flip.sum()
    # lit: the same value within fp16 storage (2^-11) and float32 surface / sample-point rounding
    sel = lit & ~flip
    for got, exp in ((got_d, exp_d), (got_s, exp_s)):
        err = np.abs(got[sel, :3] - exp[sel]) / np.maximum(np.abs(exp[sel]), 1e-6)
        assert np.quantile(err, 0.99) < 2e-3 and np.all(err[exp[sel] > 1e-4] < 1e-2), (np.quantile(err, 0.99), err.max())
    g.close()


@pytest.mark.gpu
def test_gpu_one_sample_pin(gpu, ptamd, pkg, oracle):
    """_one_sample_pin at 80 x 60"""
    _one_sample_pin(gpu, ptamd, pkg, oracle, 80, 60)


@pytest.mark.gpu
@pytest.mark.parametrize("size", dipins.RAGGED + [(17, 5)], ids=dipins.size_id)
def test_gpu_one_sample_pin_ragged(gpu, ptamd, pkg, oracle, size):
    """_one_sample_pin where k_di's 16 x 16 block and 8 x 8 wave tile are cut on both axes, and at 17 x 5: 85 pixels, less than one
    workgroup, the second block column one pixel wide. The lanes outside the frame leave before the shadow ray's walk, whose stack is the
    group's in LDS."""
    _one_sample_pin(gpu, ptamd, pkg, oracle, *size)


@pytest.mark.gpu
def test_gpu_no_emitters_clears_and_changes_nothing(gpu, ptamd, pkg):
    import torch
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = S.cornell_box(aspect=W / H)
    scene.object_data["Material"]["EmissiveStrength"] = 0.0
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    r = ptamd.Renderer(gpu, g, W, H, with_f32=True, with_denoiser_outputs=True)
    assert r.direct_lighting.light_count() == 0
    gs = S.graphics_settings(W, H, spp=1, bounces=2)
    r.render(gs); gpu.sync()
    off = {k: v.clone() for k, v in r.textures.items()}
    r.textures["Diffuse"].fill_(0x3C00); r.textures["Specular"].fill_(0x3C00)   # 1.0h everywhere: the pass must clear it
    gs["IsDIEnabled"] = 1
    r.render(gs, di_samples=8); gpu.sync()
    assert int(r.textures["Diffuse"].abs().sum()) == 0 and int(r.textures["Specular"].abs().sum()) == 0
    for k in ("Radiance", "RadianceF32"):
        assert torch.equal(r.textures[k], off[k]), k
    g.close()


@pytest.mark.gpu
def test_gpu_di_on_a_shared_scene(gpu, ptamd, pkg):
    """pt_share_scene: a second context lists the same lights from the owner's scene and renders the same DI bits, frame after frame,
    with the two contexts rendering in turn."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 40
    owner = ptamd.DeviceContext(0); viewer = ptamd.DeviceContext(0)
    scene = S.cornell_box(aspect=W / H)
    g = ptamd.Scene(owner, scene)
    v = ptamd.SharedScene(viewer, g)
    ro = ptamd.Renderer(owner, g, W, H, with_f32=True, with_denoiser_outputs=True)
    rv = ptamd.Renderer(viewer, v, W, H, with_f32=True, with_denoiser_outputs=True)
    gs = S.graphics_settings(W, H, spp=1, bounces=2, frame_index=4)
    gs["IsDIEnabled"] = 1
    outs = []
    for _ in range(2):
        for r, c in ((ro, owner), (rv, viewer)):
            r.render(gs, di_samples=8); c.sync()
            outs.append(ptamd.textures_to_numpy(r.textures))
    assert ro.direct_lighting.light_count() == rv.direct_lighting.light_count() == 2
    for o in outs[1:]:
        for k in ("Diffuse", "Specular", "RadianceF32"):
            assert np.array_equal(o[k], outs[0][k]), k
    assert (outs[0]["Diffuse"][..., :3] != 0).any()
    del ro, rv
    viewer.close(); g.close(); owner.close()


@pytest.mark.gpu
def test_cpp_host_di_frame_matches_python(tmp_path, gpu, ptamd, pkg):
    """pt_demo --di: DirectLighting of host/ptamd.hpp between the G-buffer and the path tracer, bit-identical to the Python-driven frame."""
    demo = os.path.join(ge.PKG_DIR, "pt_demo")
    S, L = pkg.scenes, pkg.layouts
    W, H, spp, bounces = 160, 90, 2, 3
    out = str(tmp_path / "radiance.bin")
    subprocess.check_call([demo, "--di", "--di-samples", "6", "--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces),
                           "--frames", "1", "--out", out])
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W / H, variant="ggx"))
    r = ptamd.Renderer(gpu, g, W, H, with_f32=True, with_denoiser_outputs=True)
    gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=0)
    gs["IsDIEnabled"] = 1
    r.render(gs, di_samples=6); gpu.sync()
    ref = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    r.render(S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=0)); gpu.sync()
    off = ptamd.textures_to_numpy(r.textures)["RadianceF32"]
    g.close()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(ref, off)                             # the DI frame is not the plain one
