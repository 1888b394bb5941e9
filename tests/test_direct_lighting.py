"""Direct lighting over emissive triangles (pt_di_*, IsDIEnabled): light preparation against a float64 restatement, the DI pass
against the path tracer it feeds, bit-exactness where it contributes nothing, determinism, sharding and the error paths."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields, off = {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = decl.split(None, 1)
        assert typ in ("float", "uint32_t"), decl
        for item in rest.split(","):
            item = item.strip()
            m = re.match(r"(\w+)(?:\[(\d+)\])?", item)
            n = int(m.group(2) or 1)
            fields[m.group(1)] = (off, n)
            off += 4 * n
    return fields, off


def test_di_struct_layouts_match_header(pkg):
    L = pkg.layouts
    for dt, cname in ((L.DI_SETTINGS, "PtDISettings"), (L.TRIANGLE_LIGHT, "PtTriangleLight")):
        fields, size = _header_struct(cname)
        assert dt.itemsize == size
        for name, (off, n) in fields.items():
            if name.startswith("_"):
                continue
            assert dt.fields[name][1] == off, (cname, name)
            sub = dt.fields[name][0]
            assert (sub.shape[0] if sub.shape else 1) == n, (cname, name)


# ---- float64 restatements ----------------------------------------------------------------------------------------------------
LUMA = np.array([0.2990, 0.5870, 0.1140])


def reference_lights(scene):
    """LightPreparation.hlsl in float64: (instance, geometry, triangle) order, hidden instances skipped."""
    rows = []
    tr = scene.instance_data["ObjectToWorld"].reshape(-1, 3, 4).astype(np.float64)
    for i in range(len(scene.objects)):
        if scene.instance_masks[i] == 0:
            continue
        fg, gc = scene.blas[scene.instance_blas[i]]
        for g in range(gc):
            mesh = scene.geometry[fg + g][0]
            od = scene.object_data[scene.instance_ids[i] + g]
            em = od["Material"]["EmissiveColor"].astype(np.float64) * np.float64(od["Material"]["EmissiveStrength"])
            if not (em > 0).any():
                continue
            pos = mesh.vertices["Position"].astype(np.float64)
            idx = mesh.indices.astype(np.int64).reshape(-1, 3)
            for t, (a, b, c) in enumerate(idx):
                p = [tr[i][:, :3] @ pos[k] + tr[i][:, 3] for k in (a, b, c)]
                e0, e1 = p[1] - p[0], p[2] - p[0]
                n = np.cross(e0, e1); ln = np.linalg.norm(n)
                rows.append(dict(inst=i, geom=g, prim=t, base=p[0], e0=e0, e1=e1, normal=n / ln if ln > 0 else 0 * n,
                                 area=ln / 2, radiance=em.copy(), mesh=mesh, tri=(a, b, c), obj=scene.instance_ids[i] + g))
    return rows


def check_lights(got, rows, scene):
    assert len(got) == len(rows)
    assert [(int(r["InstanceIndex"]), int(r["GeometryIndex"]), int(r["PrimitiveIndex"])) for r in got] == \
           [(w["inst"], w["geom"], w["prim"]) for w in rows]
    scale = max(1.0, max(np.abs(w["base"]).max() for w in rows))
    for r, w in zip(got, rows):
        tol = 8 * np.finfo(np.float32).eps * scale
        assert np.allclose(r["Base"], w["base"], atol=tol, rtol=0)
        assert np.allclose(r["Edge0"], w["e0"], atol=tol, rtol=0) and np.allclose(r["Edge1"], w["e1"], atol=tol, rtol=0)
        assert np.allclose(r["Normal"], w["normal"], atol=1e-5, rtol=0)
        assert np.isclose(r["Area"], w["area"], rtol=2e-5, atol=1e-12)
    return True


def emissive_texture_factor(scene, w, texref):
    """the emissive texture at the fp16-UV centroid (bilinear mip 0), or 1"""
    od = scene.object_data[w["obj"]]
    info = od["TextureMapInfoArray"][1]
    if info["Descriptor"] == 0xFFFFFFFF:
        return np.ones(3)
    set_ = int(info["TextureCoordinateIndex"])
    uv = w["mesh"].vertices["TexCoord%d" % set_].astype(np.float32).astype(np.float64)[list(w["tri"])]
    c = uv.astype(np.float32).sum(0) / np.float32(3)
    item = scene.heap[int(info["Descriptor"])]
    ref = texref.Reference()
    tex = ref.decode(item.array.reshape(item.height, item.width, -1), item.fmt)
    return np.asarray(ref.sample2d(tex, np.array([c[0]], np.float64), np.array([c[1]], np.float64)), np.float64).reshape(-1)[:3]


# ---- GPU helpers -------------------------------------------------------------------------------------------------------------
def _frame(ptamd, L, ctx, gscene, W, H, spp, bounces, frame, di, samples=8, denoiser=0, ext=0):
    import torch
    S = __import__("dxpbrt_amd.scenes", fromlist=["x"])
    r = ptamd.Renderer(ctx, gscene, W, H, with_f32=True, with_denoiser_outputs=True)
    gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=frame, ext_flags=ext)
    gs["IsDIEnabled"] = 1 if di else 0
    gs["Denoiser"] = denoiser
    r.render(gs, di_samples=samples if di else 0)
    ctx.sync()
    out = ptamd.textures_to_numpy(r.textures)
    del r
    torch.cuda.synchronize()
    return out


def _half(a):
    return a.view(np.float16).astype(np.float32)


@pytest.mark.gpu
def test_gpu_light_preparation_matches_float64(gpu, ptamd, pkg):
    import texref
    S, L = pkg.scenes, pkg.layouts
    scene = S.cornell_box_textured(env=None)
    scene.instance_data["ObjectToWorld"][-1] = S.trs((0.1, -0.2, 0.05), 25.0, (0.5, 0.7, 0.5))     # a moved instance
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    di = ptamd.DirectLighting(gpu)
    rows = reference_lights(scene)
    assert di.light_count() == len(rows) > 0
    W, H = 64, 36
    r = ptamd.Renderer(gpu, g, W, H, with_denoiser_outputs=True)
    r.render(S.graphics_settings(W, H, spp=1, bounces=1), di_samples=4)
    got = di.download_lights()
    check_lights(got, rows, scene)
    for rec, w in zip(got, rows):
        rad = w["radiance"] * emissive_texture_factor(scene, w, texref)
        assert np.allclose(rec["Radiance"], rad, rtol=1e-5, atol=1e-6)
        assert np.isclose(rec["Power"], w["area"] * np.pi * (LUMA @ rad), rtol=4e-5, atol=1e-9)
    assert any((emissive_texture_factor(scene, w, texref) != 1).any() for w in rows)      # the emissive texture is exercised

    # instanced_grid: many instances, one emissive quad at the end of the list
    scene2 = S.instanced_grid(n=12)
    g2 = ptamd.Scene(gpu, scene2)
    r2 = ptamd.Renderer(gpu, g2, W, H, with_denoiser_outputs=True)
    r2.render(S.graphics_settings(W, H, spp=1, bounces=1), di_samples=2)
    rows2 = reference_lights(scene2)
    check_lights(di.download_lights(), rows2, scene2)
    # the records follow a transform change and a rebuilt top level
    k = len(scene2.objects) - 1
    scene2.instance_data["ObjectToWorld"][k] = S.trs((0.5, 5.0, 9.0), 30.0, (3, 1, 3))
    g2._descs = None
    g2._build_top_level()
    r2.render(S.graphics_settings(W, H, spp=1, bounces=1), di_samples=2)
    check_lights(di.download_lights(), reference_lights(scene2), scene2)
    g2.close()


@pytest.mark.gpu
def test_gpu_di_exact_where_zero_unbiased_and_deterministic(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H = 96, 64
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W / H, variant="ggx"))
    off = _frame(ptamd, L, gpu, g, W, H, 1, 1, 3, False)
    on = _frame(ptamd, L, gpu, g, W, H, 1, 1, 3, True)
    zero = (on["Diffuse"][..., :3] == 0).all(-1) & (on["Specular"][..., :3] == 0).all(-1)
    assert zero.any() and (~zero).mean() > 0.5
    assert np.array_equal(on["RadianceF32"][zero], off["RadianceF32"][zero])
    assert np.array_equal(on["Radiance"][zero], off["Radiance"][zero])
    again = _frame(ptamd, L, gpu, g, W, H, 1, 1, 3, True)
    for k in ("Diffuse", "Specular", "Radiance", "RadianceF32"):
        assert np.array_equal(again[k], on[k]), k

    # unbiased against DI off (Bounces 1, no environment). A DI-off path finds the small light about one time in fifty, so the means
    # compare frames of 64 spp (DI is added once per frame, its mean is the same); the variance ratio compares 1-spp frames.
    def lum(o):
        return o["RadianceF32"][..., :3].astype(np.float64) @ LUMA

    def direct(o):
        return _half(o["Diffuse"])[..., :3] + _half(o["Specular"])[..., :3]

    # the pixels are chosen on the 1-spp frames (DI > 0 in every one of them), the means come from the other frames: choosing
    # them on the same frames would keep only the pixels whose shadow rays happened never to be blocked
    F1, F2 = 48, 32
    v_on, v_off, valid = [], [], np.ones((H, W), bool)
    for f in range(F1):
        o1 = _frame(ptamd, L, gpu, g, W, H, 1, 1, 100 + f, True)
        valid &= (direct(o1) > 0).any(-1)
        v_on.append(lum(o1)); v_off.append(lum(_frame(ptamd, L, gpu, g, W, H, 1, 1, 100 + f, False)))
    m_on, m_off = [], []
    for f in range(F2):
        o1 = _frame(ptamd, L, gpu, g, W, H, 64, 1, 500 + f, True)
        m_on.append(lum(o1)); m_off.append(lum(_frame(ptamd, L, gpu, g, W, H, 64, 1, 500 + f, False)))
    m_on, m_off = np.stack(m_on), np.stack(m_off)
    se = np.sqrt(m_on.var(0, ddof=1) / F2 + m_off.var(0, ddof=1) / F2)
    # The ceiling faces the way the light does, 2 mm above it: it sees the light only edge-on, a DI-off path finds it through that gap
    # a handful of times in 2048 samples and the per-pixel standard error cannot describe so rare an event. Those pixels are left out.
    ceiling = (off["NormalRoughness"][..., 1].astype(np.float32) / 32767) < -0.9
    sel = valid & (se > 0) & ~ceiling
    assert sel.sum() > 0.3 * W * H
    d = (m_on.mean(0) - m_off.mean(0))[sel]
    z = np.abs(d) / se[sel]
    assert np.mean(z > 4) < 0.01, f"{np.mean(z > 4):.4f} of pixels beyond 4 standard errors"
    assert abs(d.mean()) < 4 * np.sqrt((se[sel] ** 2).sum()) / sel.sum()          # no bias over the whole lit set
    # per-sample variance: DI on from the 1-spp frames; DI off, whose 1-spp frames mostly never meet the light, as 64 x the variance of
    # its 64-spp frame means (the samples of a frame are independent)
    ratio = np.median(np.stack(v_on).var(0, ddof=1)[sel]) / np.median(64.0 * m_off.var(0, ddof=1)[sel])
    assert ratio <= 0.5, ratio
    g.close()


@pytest.mark.gpu
def test_gpu_di_lambertian_closed_form_and_sharding(gpu, ptamd, pkg):
    """Cornell box (diffuse variant, PT_EXT_LAMBERTIAN_ONLY): specular is exactly zero; the DI estimate over frames matches
    albedo/pi * L * (polygon form factor) on the unoccluded floor; two emulated ranks reproduce the unsharded frame bit for bit."""
    S, L = pkg.scenes, pkg.layouts
    import torch
    W, H = 64, 48
    scene = S.cornell_box(aspect=W / H, variant="diffuse")
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, scene)
    full = _frame(ptamd, L, gpu, g, W, H, 1, 1, 7, True, samples=4, ext=L.EXT_LAMBERTIAN_ONLY)
    assert (full["Specular"][..., :3] == 0).all()
    bands = []
    for rank in range(2):
        gpu.set_sharding(rank, 2, 8)
        bands.append(_frame(ptamd, L, gpu, g, W, H, 1, 1, 7, True, samples=4, ext=L.EXT_LAMBERTIAN_ONLY))
    gpu.set_sharding(0, 1, 16)
    for k in ("Diffuse", "RadianceF32"):
        rows = [None] * H
        for rank in range(2):
            lr = 0
            for b in range(rank, (H + 7) // 8, 2):
                for y in range(b * 8, min(H, b * 8 + 8)):
                    rows[y] = bands[rank][k][lr]; lr += 1
        assert np.array_equal(np.stack(rows), full[k]), k

    # closed form on the floor: E = L * sum over edges of the polygon form factor (Lambert), float64
    M = scene.instance_data["ObjectToWorld"][5].reshape(3, 4).astype(np.float64)             # the light quad's instance
    light = scene.nodes[scene.objects[5].node].meshes[0].vertices["Position"].astype(np.float64) @ M[:, :3].T + M[:, 3]
    assert (scene.object_data[scene.instance_ids[5]]["Material"]["EmissiveStrength"] > 0)
    Le = 15.0
    F = 64
    acc = []
    for f in range(F):
        o = _frame(ptamd, L, gpu, g, W, H, 1, 1, 1000 + f, True, samples=4, ext=L.EXT_LAMBERTIAN_ONLY)
        acc.append(_half(o["Diffuse"])[..., :3].astype(np.float64))
    acc = np.stack(acc)
    gb = _frame(ptamd, L, gpu, g, W, H, 1, 1, 0, False)
    pos = gb["Position"][..., :3].astype(np.float64)
    # floor near the opening, left of the short box: nothing between it and the light
    floor = np.isfinite(pos).all(-1) & (np.abs(pos[..., 1] + 1) < 1e-4) & (pos[..., 0] > -0.55) & (pos[..., 0] < -0.15) & (pos[..., 2] > -0.6) & (pos[..., 2] < -0.45)
    assert floor.sum() >= 3
    albedo = (gb["BaseColorMetalness"][..., :3].astype(np.float64) / 255.0)
    n = np.array([0, 1.0, 0])
    for y, x in zip(*np.nonzero(floor)):
        p = pos[y, x]
        ff = 0.0
        for k in range(4):
            a, b = light[k] - p, light[(k + 1) % 4] - p
            a /= np.linalg.norm(a); b /= np.linalg.norm(b)
            c = np.cross(a, b)
            ff += np.arccos(np.clip(a @ b, -1, 1)) * (c / np.linalg.norm(c)) @ n
        E = Le * abs(ff) / 2                                           # pi * L * form factor
        expect = albedo[y, x] / np.pi * E
        mean, sd = acc[:, y, x].mean(0), acc[:, y, x].std(0, ddof=1)
        assert np.all(np.abs(mean - expect) <= 4 * sd / np.sqrt(F) + 2e-3 * expect), (y, x, mean, expect)
    g.close()


@pytest.mark.gpu
def test_gpu_di_errors_and_output_variants(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H = 32, 24
    ctx = ptamd.DeviceContext(0)
    g = ptamd.Scene(ctx, S.cornell_box(aspect=W / H))
    r = ptamd.Renderer(ctx, g, W, H, with_f32=True, with_denoiser_outputs=True)
    di = ptamd.DirectLighting(ctx)
    di.Textures = r.textures
    with pytest.raises(ptamd.PtError) as e:
        di.Render(None)
    assert "pt_di_set_constants" in str(e.value)
    for bad in (0, 33):
        with pytest.raises(ptamd.PtInvalidArgument):
            di.SetConstants(L.di_settings(W, H, samples=bad))
    gs = S.graphics_settings(W, H, spp=1, bounces=1)
    gs["IsDIEnabled"] = 1
    rt = ptamd.Raytracing(ctx)
    rt.GPUBuffers = dict(r.raytracing.GPUBuffers)
    rt.Textures = {k: v for k, v in r.textures.items() if k not in ("Diffuse", "Specular")}
    rt.SetConstants(gs)
    with pytest.raises(ptamd.PtInvalidArgument) as e:
        rt.Render(None)
    assert "Diffuse" in str(e.value)
    # last pass (Bounces 0), Denoiser None: the DI result is added to Radiance, Diffuse / Specular stay clear
    r.render(S.graphics_settings(W, H, spp=1, bounces=0))
    ctx.sync()
    base = ptamd.textures_to_numpy(r.textures)
    r.render(S.graphics_settings(W, H, spp=1, bounces=0), di_samples=8)
    ctx.sync()
    last = ptamd.textures_to_numpy(r.textures)
    assert (_half(last["Radiance"])[..., :3] >= _half(base["Radiance"])[..., :3]).all()
    assert (_half(last["Radiance"])[..., :3] > _half(base["Radiance"])[..., :3]).any()
    assert (last["Diffuse"] == 0).all() and (last["Specular"] == 0).all()
    # RadianceF32: the fp32 value whose fp16 rounding is stored to Radiance (as the path tracer writes the pair)
    touched = (last["Radiance"] != base["Radiance"]).any(-1)
    assert touched.any()
    assert np.array_equal(last["RadianceF32"][touched][:, :3].astype(np.float16).view(np.uint16), last["Radiance"][touched][:, :3])
    # NRD, last pass: Diffuse / Specular carry (radiance, light distance)
    gs = S.graphics_settings(W, H, spp=1, bounces=0); gs["Denoiser"] = L.DENOISER_NRD_REBLUR
    r.render(gs, di_samples=8)
    ctx.sync()
    nrd = ptamd.textures_to_numpy(r.textures)
    d = _half(nrd["Diffuse"])
    lit = (d[..., :3] > 0).any(-1)
    assert lit.any() and (d[..., 3][lit] > 0).all() and (d[..., 3][lit] < 4.0).all()
    g.close(); ctx.close()
