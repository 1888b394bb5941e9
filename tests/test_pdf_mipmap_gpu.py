"""The local-light PDF texture on the GPU: pt_mipmap_generate bit for bit against tests/pdfmipref.py, the DI pass's texture, the Power_RIS
tiles of its descent, the ReGIR builds fed those tiles, the off path, the estimator, the BRDF candidates' source pdf, both hosts, viewers
and shards. Every test that turns the setting on works on a context of its own: the setting lives in the context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import brdfcandref as B
import brdfscene
import bsdfref
import onionref as O
import pdfmipref as M
import presamplingref as P
import restirref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
NEAR = 1e-5
W_BAND = 2.5e-4                  # the BRDF pin's band on W (tests/test_direct_lighting_brdf.py), taken over as it stands there
SENTINEL = f32(-12345.5)
SIZES = [(1, 1), (2, 1), (2, 2), (4, 2), (32, 32), (64, 32), (64, 64), (1024, 512), (2048, 1024)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _signed(a):
    return np.where(a == 0xFFFFFFFF, -1, a.astype(np.int64))


def _half(a):
    return a.view(np.float16).astype(np.float64)


class _Session:
    """a device context of its own, a scene and a renderer"""

    def __init__(self, ptamd, scene, W, H, history=False, sharding=None):
        self.ptamd = ptamd
        self.ctx = ptamd.DeviceContext(0)
        if sharding:
            self.ctx.set_sharding(*sharding)
        self.g = ptamd.Scene(self.ctx, scene)
        self.r = ptamd.Renderer(self.ctx, self.g, W, H, with_f32=True, with_denoiser_outputs=True, di_history=history)
        self.dl = self.r.direct_lighting

    def frame(self, S, W, H, frame, ls, pdf=None, samples=8, reuse=None, bounces=0, **kw):
        gs = S.graphics_settings(W, H, spp=1, bounces=bounces, frame_index=frame)
        gs["IsDIEnabled"] = 1
        self.r.render(gs, di_samples=samples, di_reuse=reuse, di_light_sampling=ls, di_pdf_mipmap=pdf, **kw)
        self.ctx.sync()
        return self.ptamd.textures_to_numpy(self.r.textures)

    def close(self):
        del self.r, self.dl
        self.g.close(); self.ctx.close()


# ---- 1. the operator -----------------------------------------------------------------------------------------------------------------
def _run_operator(ptamd, gpu, level0, mip_levels=None):
    """level 0 and sentinel-filled buffers for every level of the full chain on the device; Process over mip_levels of them; the buffers back"""
    import torch
    h, w = level0.shape
    full = max(w, h).bit_length()
    bufs = [torch.from_numpy(np.ascontiguousarray(level0)).cuda()]
    for k in range(1, full):
        lw, lh = M.level_size(w, h, k)
        bufs.append(torch.full((lh, lw), float(SENTINEL), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    op = ptamd.MipmapGeneration(gpu)
    op.SetTexture(bufs[:full if mip_levels is None else mip_levels], w, h)
    op.Process()
    gpu.sync()
    return [b.cpu().numpy() for b in bufs]


def _assert_levels_equal(got, exp):
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape, k
        nan = np.isnan(e)
        assert np.array_equal(np.isnan(g), nan), k                          # a NaN is a NaN on both sides, whatever its payload
        assert np.array_equal(_bits(g)[~nan], _bits(e)[~nan]), (k, np.argwhere(_bits(g) != _bits(e))[:4].tolist())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_operator_bit_for_bit(gpu, ptamd, size):
    """full chains, 2:1 shapes, the order switches at levels 6 and 11, a first tile that is not full, one to three launches"""
    w, h = size
    rng = np.random.default_rng(w * 7 + h)
    level0 = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (h, w))).astype(f32)
    exp = M.build(level0)
    got = _run_operator(ptamd, gpu, level0)
    assert len(got) == len(exp) == max(w, h).bit_length() and got[-1].shape == (1, 1)
    _assert_levels_equal(got, exp)
    if len(exp) > 6:                                                         # the order rule is live in this case: the other order gives other bits
        other = M.build(level0, quad_levels=())
        assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(exp, other))


def test_operator_hostile_texels(gpu, ptamd):
    """zeros, 1e-30, pairs of 3e38 that overflow, negatives, NaN -- and subnormals, which the library's build keeps"""
    rng = np.random.default_rng(5)
    level0 = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (32, 64))).astype(f32)
    flat = level0.reshape(-1)
    pick = rng.permutation(flat.size)
    flat[pick[:200]] = 0.0
    flat[pick[200:300]] = 1e-30
    flat[pick[300:360]] = -flat[pick[300:360]]
    flat[pick[360:380]] = np.nan
    flat[pick[380:440]] = f32(1e-40)                                        # subnormal
    flat[pick[440:460]] = -0.0
    level0[10, 20:22] = 3e38; level0[11, 20] = 3e38                         # one quad: the sum overflows to +inf
    level0[20, 40] = 3e38; level0[21, 41] = -3e38                           # +big and -big in one quad
    level0[4:6, 8:10] = f32(1e-45); level0[5, 9] = 0.0                      # three times the smallest subnormal: the quarter of the sum rounds
    level0[0, 0] = np.inf; level0[0, 1] = -np.inf                           # inf - inf: NaN
    exp = M.build(level0)
    assert np.isinf(exp[1]).any() and np.isnan(exp[1]).any() and (exp[1] < 0).any()
    assert ((exp[1] != 0) & (np.abs(exp[1]) < np.finfo(f32).tiny)).any()    # subnormal results are part of the comparison
    _assert_levels_equal(_run_operator(ptamd, gpu, level0), exp)


def test_operator_partial_chain_and_refusals(gpu, ptamd):
    import torch
    rng = np.random.default_rng(9)
    level0 = rng.uniform(0.5, 2.0, (32, 64)).astype(f32)
    exp = M.build(level0)
    for mips in (1, 3, 6):                                                   # 6: one launch of five levels; the seventh level stays untouched
        got = _run_operator(ptamd, gpu, level0, mips)
        _assert_levels_equal(got[:mips], exp[:mips])
        for k in range(mips, len(got)):
            assert (got[k] == SENTINEL).all(), (mips, k)
    # refusals: a message each, nothing enqueued (the buffers keep the sentinel)
    bufs = [torch.full((max(1, 32 >> k), max(1, 64 >> k)), float(SENTINEL), dtype=torch.float32, device="cuda") for k in range(7)]
    op = ptamd.MipmapGeneration(gpu)
    cases = [(bufs, 0, 32, "width"), (bufs, 48, 32, "width"), (bufs, 32768, 32, "width"), (bufs, 64, 0, "height"), (bufs, 64, 24, "height"),
             (bufs, 64, 32768, "height"), ([], 64, 32, "mip_levels"), (bufs + [bufs[-1]], 64, 32, "mip_levels"), (bufs * 3, 64, 32, "mip_levels"),
             (bufs[:3] + [0] + bufs[4:], 64, 32, "NULL")]
    for levels, w, h, word in cases:
        op.SetTexture(levels, w, h)
        with pytest.raises(ptamd.PtInvalidArgument, match=word):
            op.Process()
    with pytest.raises(ptamd.PtInvalidArgument, match="NULL"):
        gpu.check(gpu.lib.pt_mipmap_generate(gpu.handle, None, 64, 32, 7))
    table = (C.c_void_p * 17)(*([bufs[0].data_ptr()] * 17))
    with pytest.raises(ptamd.PtInvalidArgument, match="mip_levels"):       # above 16
        gpu.check(gpu.lib.pt_mipmap_generate(gpu.handle, C.cast(table, C.c_void_p), 16384, 16384, 17))
    gpu.sync()
    for b in bufs:
        assert (b.cpu().numpy() == SENTINEL).all()


# ---- 2. the PDF texture of a scene ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,shape", [(11, (16, 16)), (16, (32, 16))], ids=["square", "two_to_one"])
def test_pdf_texture_of_a_scene(ptamd, pkg, n, shape):
    S, L = pkg.scenes, pkg.layouts
    W, H = 32, 24
    s = _Session(ptamd, S.emitter_field(n, aspect=W / H), W, H)
    s.frame(S, W, H, 3, None)
    assert s.dl.download_pdf_texture() == []                                # the setting is off: 0 x 0
    s.frame(S, W, H, 3, None, pdf=True)                                     # built in every mode, here the power CDF
    levels = s.dl.download_pdf_texture()
    lights = s.dl.download_lights()
    assert len(lights) == 2 * n * n
    w, h, mips = M.texture_size(len(lights))
    assert (w, h) == shape == ptamd.pdf_texture_size(len(lights))[:2] and len(levels) == mips
    assert levels[0].shape == (h, w)
    exp0 = M.level0(lights["Power"], w, h)
    assert np.array_equal(_bits(levels[0]), _bits(exp0)) and (exp0 > 0).sum() == len(lights)
    _assert_levels_equal(levels, M.build(exp0))
    # a level the texture does not have, and the call's contract
    wv, hv = C.c_uint32(9), C.c_uint32(9)
    s.ctx.check(s.ctx.lib.pt_di_download_pdf_texture(s.ctx.handle, mips, None, 0, C.byref(wv), C.byref(hv)))
    assert (wv.value, hv.value) == (0, 0)
    with pytest.raises(ptamd.PtInvalidArgument):
        s.ctx.check(s.ctx.lib.pt_di_download_pdf_texture(s.ctx.handle, 16, None, 0, C.byref(wv), C.byref(hv)))
    with pytest.raises(ptamd.PtInvalidArgument):
        s.ctx.check(s.ctx.lib.pt_di_set_pdf_mipmap(s.ctx.handle, 2))
    s.frame(S, W, H, 4, None)                                               # the refused value left the setting on
    assert len(s.dl.download_pdf_texture()) == mips
    s.frame(S, W, H, 4, None, pdf=False)
    assert s.dl.download_pdf_texture() == []
    s.close()
    # a scene without emitters builds none
    scene = S.cornell_box(aspect=W / H)
    scene.object_data["Material"]["EmissiveStrength"] = 0.0
    s = _Session(ptamd, scene, W, H)
    s.frame(S, W, H, 1, L.di_light_sampling_settings("power_ris"), pdf=True, bounces=2)
    assert s.dl.download_pdf_texture() == [] and len(s.dl.download_presampled(0)) == 0
    s.close()


# ---- 3. the tiles --------------------------------------------------------------------------------------------------------------------
def _field_with_dark_lights(S, n, aspect, dark):
    """emitter_field(n) with the quads `dark` collapsed to a segment: their triangles have no area and their lights no power"""
    scene = S.emitter_field(n, aspect=aspect)
    pos = scene.nodes[1].meshes[0].vertices["Position"]
    for q in dark:
        pos[4 * q + 1] = pos[4 * q]; pos[4 * q + 2] = pos[4 * q + 3]
    return scene.finalize()


@pytest.fixture(scope="module")
def dark_field(ptamd, pkg):
    S = pkg.scenes
    W, H = 32, 24
    dark = [0, 7, 100, 101, 333, 528]
    s = _Session(ptamd, _field_with_dark_lights(S, 23, W / H, dark), W, H)
    yield s, W, H, dark
    s.close()


@pytest.mark.parametrize("frame", [4, 77])
def test_tiles_bit_for_bit(dark_field, pkg, frame):
    S, L = pkg.scenes, pkg.layouts
    s, W, H, dark = dark_field
    s.frame(S, W, H, frame, L.di_light_sampling_settings("power_ris"), pdf=True)
    levels, lights, tiles = s.dl.download_pdf_texture(), s.dl.download_lights(), s.dl.download_presampled(0)
    assert len(lights) == 1058 and levels[0].shape == (32, 64) and len(levels) - 1 >= 6           # six levels to descend
    zero = np.nonzero(lights["Power"] == 0)[0]
    assert sorted(zero.tolist()) == sorted(k for q in dark for k in (2 * q, 2 * q + 1))
    li, inv = M.descend(levels, len(lights), frame)
    got = _signed(tiles["LightIndex"])
    assert len(tiles) == 128 * 1024 and np.array_equal(got, li)
    assert np.array_equal(_bits(tiles["InvSourcePdf"]), _bits(inv))
    assert (got >= 0).all() and not np.isin(got, zero).any()
    assert len(np.unique(got)) > 950                                         # of 1046 lights with power (the dimmest expect about 4 entries)
    s.frame(S, W, H, frame, L.di_light_sampling_settings("power_ris"), pdf=False)
    assert not np.array_equal(_signed(s.dl.download_presampled(0)["LightIndex"]), li)      # the prefix sum's tiles are others


# ---- 4. ReGIR consumes the tiles unchanged -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["grid", "onion"])
def test_regir_builds_from_the_descents_tiles(ptamd, pkg, layout):
    """the existing restatements of the builds fed the downloaded tiles, at the existing pins' limits: the same light on >= 0.999 of the
    slots, the weight within 2e-5 relative"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 32, 24
    scene = S.emitter_field(16, aspect=W / H)
    s = _Session(ptamd, scene, W, H)
    s.frame(S, W, H, 21, L.di_light_sampling_settings("regir", cell_size=0.7, build_samples=6), pdf=True,
            di_regir_layout=L.di_regir_layout_settings(layout))
    levels, lights, tiles, cells = s.dl.download_pdf_texture(), s.dl.download_lights(), s.dl.download_presampled(0), s.dl.download_presampled(1)
    s.close()
    li, inv = M.descend(levels, len(lights), 21)
    assert np.array_equal(_signed(tiles["LightIndex"]), li) and np.array_equal(_bits(tiles["InvSourcePdf"]), _bits(inv))
    centre = scene.camera["Position"].astype(np.float32).reshape(3)
    if layout == "grid":
        sel = np.array([(z * 16 + y) * 16 + x for z in (6, 8, 10, 12) for y in (4, 8, 11, 12) for x in (5, 8, 11)])
        exp_li, exp_w = P.regir_build(lights, li, tiles["InvSourcePdf"], sel, centre, 0.7, 6, 21)
        got = cells.reshape(4096, 512)[sel]
    else:
        tables = O.Tables(*[ptamd.onion_table(w) for w in range(4)])
        sel = [0]
        for layer in (0, 1, 2, 3, 4, 7, 10, 14):
            n0, n1 = O.RING_CELLS[O.LAYER_GROUP[layer]][0], O.RING_CELLS[O.LAYER_GROUP[layer]][1]
            base, end = O.LAYER_BASE[layer], O.LAYER_BASE[layer] + O.LAYER_CELLS[layer]
            sel += [base + 1, base + n0 // 2, base + n0 + n1 // 3, base + n0 + n1 + (2 * n1) // 3, end - 2, end - 1]
        sel = np.array(sel)
        exp_li, exp_w = O.onion_build(tables, lights, li, tiles["InvSourcePdf"], sel, centre, 0.7, 6, 21)
        got = cells.reshape(O.CELLS, 512)[sel]
    same = _signed(got["LightIndex"]) == exp_li
    rel = np.abs(got["InvSourcePdf"].astype(np.float64) - exp_w) / np.maximum(np.abs(exp_w), 1e-30)
    rel = np.where((exp_w == 0) & (got["InvSourcePdf"] == 0), 0.0, rel)
    print(f"{layout}: {same.mean():.6f} of slots with the same light, weight rel err max {rel[same].max():.2e}, {(exp_li >= 0).mean():.3f} filled")
    assert (exp_li >= 0).mean() > 0.2
    assert same.mean() >= 0.999
    assert rel[same].max() <= 2e-5


# ---- 5. off is the parent ------------------------------------------------------------------------------------------------------------
def test_off_is_the_parent_and_the_setting_resets_the_history(ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    keys = ("Diffuse", "Specular", "RadianceF32")
    modes = [None, "uniform", "power_ris", "regir"]
    ls = {m: (None if m is None else L.di_light_sampling_settings(m)) for m in modes}
    s = _Session(ptamd, S.emitter_field(16, aspect=W / H), W, H)
    before = {}
    for m in modes:                                                          # the setting never touched
        out = s.frame(S, W, H, 6, ls[m], bounces=1)
        before[m] = ({k: out[k].copy() for k in keys}, s.dl.download_presampled(0).copy(), s.dl.download_presampled(1).copy())
    assert (before[None][0]["Diffuse"][..., :3] != 0).any()
    s.dl.SetPdfMipmap(True); s.dl.SetPdfMipmap(False)
    for m in modes:
        out = s.frame(S, W, H, 6, ls[m], bounces=1)
        for k in keys:
            assert np.array_equal(out[k], before[m][0][k]), (m, k)
        assert np.array_equal(s.dl.download_presampled(0), before[m][1]) and np.array_equal(s.dl.download_presampled(1), before[m][2]), m
    for m in modes:                                                          # on: the power CDF and Uniform keep their bits, the RIS modes do not
        out = s.frame(S, W, H, 6, ls[m], pdf=True, bounces=1)
        same = all(np.array_equal(out[k], before[m][0][k]) for k in keys)
        assert same == (m in (None, "uniform")), m
        assert len(s.dl.download_pdf_texture()) == 6
    s.close()
    # the history: reset by a change of the setting, and only by a change
    s = _Session(ptamd, S.emitter_field(16, aspect=W / H), W, H, history=True)
    reuse = L.di_resampling_settings(temporal=True, spatial_samples=0, boiling_filter=False)
    pr = L.di_light_sampling_settings("power_ris")
    grown = lambda: bool((s.dl.download_reservoirs()["M"] > 8).any())
    s.frame(S, W, H, 1, pr, reuse=reuse)
    s.frame(S, W, H, 2, pr, reuse=reuse)
    assert grown()
    s.frame(S, W, H, 3, pr, pdf=False, reuse=reuse)                          # 0 -> 0: no change
    assert grown()
    s.frame(S, W, H, 4, pr, pdf=True, reuse=reuse)                           # 0 -> 1
    assert not grown()
    s.frame(S, W, H, 5, pr, pdf=True, reuse=reuse)                           # 1 -> 1
    assert grown()
    s.frame(S, W, H, 6, pr, pdf=False, reuse=reuse)                          # 1 -> 0
    assert not grown()
    s.close()


# ---- 6. the same estimator -----------------------------------------------------------------------------------------------------------
def test_same_estimator(ptamd, pkg):
    """Power_RIS with the prefix sum and with the descent estimate the same image: the whole-image mean of Diffuse + Specular over 64 frame
    indices agrees within 4 standard errors of the difference, the standard error taken from the per-frame differences of the means"""
    S, L = pkg.scenes, pkg.layouts
    W, H, K = 64, 36, 64
    s = _Session(ptamd, S.emitter_field(16, aspect=W / H), W, H)
    pr = L.di_light_sampling_settings("power_ris")
    means = {}
    for on in (False, True):
        v = []
        for f in range(K):
            out = s.frame(S, W, H, 300 + f, pr, pdf=on, bounces=1)
            v.append((_half(out["Diffuse"])[..., :3] + _half(out["Specular"])[..., :3]).mean())
        means[on] = np.array(v)
    s.close()
    d = means[True] - means[False]
    se = d.std(ddof=1) / np.sqrt(K)
    print(f"mean off {means[False].mean():.6f}, on {means[True].mean():.6f}, difference {d.mean():+.3e}, standard error {se:.3e} "
          f"({abs(d.mean()) / se:.2f} standard errors)")
    assert means[False].mean() > 0 and means[True].mean() > 0
    assert abs(d.mean()) <= 4 * se


# ---- 7. BRDF candidates: q_L = Power / (top * M^2) -----------------------------------------------------------------------------------
def _initial_power_ris_brdf(S_, lights, rec, tiles, levels, frame, n_l, n_b, cutoff, bsdf):
    """brdfcandref.initial_sampling with Power_RIS light candidates (presamplingref.candidates over the downloaded tiles) and the BRDF
    candidates' light pdf from the PDF texture; the same float64 terms, blended pdf, stream and W"""
    H, W = S_.H, S_.W
    N = n_l + n_b
    out = {k: np.zeros((H, W), np.float64 if k in ("U", "V", "W") else np.int64) for k in ("LightIndex", "U", "V", "W", "M")}
    out["LightIndex"][:] = -1
    margin = np.full((H, W), np.inf)
    ys, xs = np.nonzero(S_.valid)
    n = len(ys)
    count = len(lights)
    q_source = M.source_pdf(lights["Power"], levels)
    tl, tinv = _signed(tiles["LightIndex"]), tiles["InvSourcePdf"]
    li = np.zeros((n, N), np.int64); U = np.zeros((n, N), f32); V = np.zeros((n, N), f32); coin = np.zeros((n, N), f32)
    ql = np.zeros((n, N))
    for i, (y, x) in enumerate(zip(ys, xs)):
        for k, (l, pdf, r1, r2, r3) in enumerate(P.candidates("power_ris", int(x), int(y), frame, n_l, None, count, tl, tinv)):
            li[i, k], ql[i, k], U[i, k], V[i, k], coin[i, k] = l, float(pdf), r1, r2, r3
        d = B.brdf_draws(int(x), int(y), frame, n_b)
        for j in range(n_b):
            c = rec[y, x, j]
            l = int(c["LightIndex"])
            li[i, n_l + j] = l if l < count else -1
            U[i, n_l + j], V[i, n_l + j], coin[i, n_l + j] = c["U"], c["V"], d[j, 4]
            if l < count:
                ql[i, n_l + j] = float(q_source[l])
    p = np.zeros((n, N)); w = np.zeros((n, N))
    for k in range(N):
        pk, pdf, qb, dist, mk, _ = B.sample_terms(S_, ys, xs, lights, li[:, k], U[:, k], V[:, k], bsdf)
        p[:, k] = pk
        for i in range(n):
            if li[i, k] < 0:
                continue
            margin[ys[i], xs[i]] = min(margin[ys[i], xs[i]], mk[i])
            if not pk[i] > 0:
                continue
            if cutoff > 0 and qb[i] > 0:
                margin[ys[i], xs[i]] = min(margin[ys[i], xs[i]], R._margin(dist[i], float(np.sqrt((1.0 / cutoff - 1.0) * qb[i]))))
            w[i, k] = pk[i] / B.blended_pdf(n_l, n_b, ql[i, k], qb[i], pdf[i], dist[i], cutoff)
    for i, (y, x) in enumerate(zip(ys, xs)):
        sel, wsum, m = B.stream(list(w[i]), list(coin[i]), None)
        margin[y, x] = min(margin[y, x], m)
        out["M"][y, x] = N
        if sel >= 0 and p[i, sel] > 0:
            out["LightIndex"][y, x], out["U"][y, x], out["V"][y, x] = li[i, sel], U[i, sel], V[i, sel]
            out["W"][y, x] = B.reservoir_weight(wsum, N, p[i, sel])
    return out, margin


def test_brdf_candidates_source_pdf(ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H, frame, n_l, n_b = 48, 32, 40, 2, 4
    scene = brdfscene.glossy_scene(S, W / H)
    init = L.di_resampling_settings(temporal=True, spatial_samples=0, temporal_bias=L.DI_BIAS_CORRECTION_OFF, boiling_filter=False)
    s = _Session(ptamd, scene, W, H, history=True)
    s.dl.ResetHistory()
    out = s.frame(S, W, H, frame, L.di_light_sampling_settings("power_ris"), pdf=True, samples=n_l, reuse=init, bounces=1,
                  di_brdf=L.di_brdf_settings(n_b, brdfscene.CUTOFF))
    got = R.as_frame(s.dl.download_reservoirs(), H, W)
    rec = s.dl.download_brdf_candidates().reshape(H, W, n_b)
    lights, tiles, levels = s.dl.download_lights(), s.dl.download_presampled(0), s.dl.download_pdf_texture()
    s.close()
    cur = R.Surfaces(out, scene.camera)
    exp, margin = _initial_power_ris_brdf(cur, lights, rec, tiles, levels, frame, n_l, n_b, brdfscene.CUTOFF, bsdfref.Reference())
    sel = cur.valid & (margin >= NEAR)
    excluded = int((cur.valid & (margin < NEAR)).sum())
    assert (got["M"][cur.valid] == n_l + n_b).all()
    for k in ("LightIndex", "M"):
        bad = sel & (got[k] != exp[k])
        assert not bad.any(), (k, np.argwhere(bad)[:5].tolist(), got[k][bad][:5], exp[k][bad][:5])
    for k in ("U", "V"):
        assert np.array_equal(got[k][sel].astype(np.float32), exp[k][sel].astype(np.float32)), k
    rel = np.abs(got["W"][sel] - exp["W"][sel]) / np.maximum(np.abs(exp["W"][sel]), 1e-30)
    rel = np.where((got["W"][sel] == 0) & (exp["W"][sel] == 0), 0.0, rel)
    held = ((got["LightIndex"][..., None] == rec["LightIndex"].astype(np.int64)) & (got["U"][..., None].astype(np.float32) == rec["U"]) &
            (got["V"][..., None].astype(np.float32) == rec["V"])).any(-1) & sel
    print(f"{sel.sum()} pixels compared, {excluded} within {NEAR} of a decision, W rel err max {rel.max():.2e}; {held.sum()} reservoirs hold a BRDF sample")
    assert sel.sum() > 0.4 * W * H and excluded < 0.05 * cur.valid.sum()
    assert rel.max() <= W_BAND
    assert held.sum() > 10


# ---- 8. both hosts -------------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_python(tmp_path, ptamd, pkg):
    demo = os.path.join(ge.PKG_DIR, "pt_demo")
    S, L = pkg.scenes, pkg.layouts
    W, H, spp, bounces = 160, 90, 2, 3
    out = str(tmp_path / "radiance.bin")
    size = ["--width", str(W), "--height", str(H), "--spp", str(spp), "--bounces", str(bounces), "--frames", "1"]
    run = subprocess.run([demo, "--di", "--di-samples", "6", "--light-sampling", "power_ris", "--di-pdf-mipmap", *size, "--out", out],
                         stdout=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and '"di_pdf_mipmap": true' in run.stdout
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    s = _Session(ptamd, S.cornell_box(aspect=W / H, variant="ggx"), W, H)
    gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=0)
    gs["IsDIEnabled"] = 1
    pr = L.di_light_sampling_settings("power_ris")
    s.r.render(gs, di_samples=6, di_light_sampling=pr, di_pdf_mipmap=True); s.ctx.sync()
    ref = ptamd.textures_to_numpy(s.r.textures)["RadianceF32"].copy()
    levels = s.dl.download_pdf_texture()
    s.close()
    # (the box has two lights of one power: the descent and the prefix sum pick alike there, so the frame is not compared with the off one)
    assert [v.shape for v in levels] == [(1, 2), (1, 1)] and (ref[..., :3] > 0).any()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    bad = subprocess.run([demo, "--di-pdf-mipmap", *size], stderr=subprocess.PIPE, text=True, timeout=300)
    assert bad.returncode != 0 and "--di-pdf-mipmap" in bad.stderr


# ---- 9. viewer and shard -------------------------------------------------------------------------------------------------------------
def test_viewer_and_shard(ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 48
    pr = L.di_light_sampling_settings("power_ris")
    owner = _Session(ptamd, S.emitter_field(16, aspect=W / H), W, H)
    full = owner.frame(S, W, H, 9, pr, pdf=True)["RadianceF32"].copy()
    own_levels, own_tiles = owner.dl.download_pdf_texture(), owner.dl.download_presampled(0)
    assert len(own_levels) == 6 and (full[..., :3] > 0).any()
    # a context that views the owner's scene builds a texture of its own, with the owner's bits
    vctx = ptamd.DeviceContext(0)
    view = ptamd.SharedScene(vctx, owner.g)
    rv = ptamd.Renderer(vctx, view, W, H, with_f32=True, with_denoiser_outputs=True)
    assert rv.direct_lighting.download_pdf_texture() == []
    gs = S.graphics_settings(W, H, spp=1, bounces=0, frame_index=9)
    gs["IsDIEnabled"] = 1
    rv.render(gs, di_samples=8, di_light_sampling=pr, di_pdf_mipmap=True); vctx.sync()
    _assert_levels_equal(rv.direct_lighting.download_pdf_texture(), own_levels)
    assert np.array_equal(rv.direct_lighting.download_presampled(0), own_tiles)
    assert np.array_equal(ptamd.textures_to_numpy(rv.textures)["RadianceF32"].view(np.uint32), full.view(np.uint32))
    del rv
    view.close(); vctx.close()
    # two emulated ranks (8-row bands): the tiles do not depend on the band, and the bands are the unsharded frame
    rows = [None] * H
    for rank in range(2):
        owner.ctx.set_sharding(rank, 2, 8)
        rr = ptamd.Renderer(owner.ctx, owner.g, W, H, with_f32=True, with_denoiser_outputs=True)
        rr.render(gs, di_samples=8, di_light_sampling=pr, di_pdf_mipmap=True); owner.ctx.sync()
        assert np.array_equal(rr.direct_lighting.download_presampled(0), own_tiles), rank
        band = ptamd.textures_to_numpy(rr.textures)["RadianceF32"]
        lr = 0
        for b in range(rank, (H + 7) // 8, 2):
            for y in range(b * 8, min(H, b * 8 + 8)):
                rows[y] = band[lr]; lr += 1
        del rr
    owner.ctx.set_sharding(0, 1, 16)
    assert np.array_equal(np.stack(rows).view(np.uint32), full.view(np.uint32))
    owner.close()
