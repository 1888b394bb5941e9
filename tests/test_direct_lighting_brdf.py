"""BRDF candidates of the DI pass's initial sampling on the GPU ("BRDF candidates"): off is the parent's frame bit
for bit; the candidate records equal the CPU oracle's replay bit for bit; the initial reservoirs match the float64 restatement
(tests/brdfcandref.py) per pixel; the estimate is unbiased and its variance on a glossy plane is below light sampling's; sharding,
reuse + visibility + pairwise, the C++ host and the setter's refusals."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import brdfcandref as B
import brdfscene
import bsdfref
import dipins
import restirref as R

NEAR = 1e-5
W_BAND = 2.5e-4      # relative band of W against float64: twice the measured maximum, 1.25e-4 (test_gpu_initial_reservoirs_pinned)
LUMA = R.LUMA


def _half(a):
    return a.view(np.float16).astype(np.float64)


class _Session:
    """a device context of its own (the BRDF setting lives in the context: the shared one never sees it), a scene and a renderer"""

    def __init__(self, ptamd, scene, W, H, di_history=False, sharding=None, with_f32=False):
        self.ptamd = ptamd
        self.ctx = ptamd.DeviceContext(0)
        if sharding:
            self.ctx.set_sharding(*sharding)
        self.g = ptamd.Scene(self.ctx, scene)
        self.r = ptamd.Renderer(self.ctx, self.g, W, H, with_denoiser_outputs=True, di_history=di_history, with_f32=with_f32)

    def textures(self):
        self.ctx.sync()
        return self.ptamd.textures_to_numpy(self.r.textures)

    def close(self):
        del self.r
        self.g.close(); self.ctx.close()


# ---- 1. off is today --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "reuse-basic", "regir"])
def test_gpu_off_is_the_parents_frame(ptamd, pkg, mode):
    """Three renders of the same two frames: the setter never called, called through the binding's None (0 samples, cutoff 0), called
    with BrdfSamples = 0 and a cutoff, which then means nothing. Every output texture and every downloaded reservoir is byte-identical across them, and no candidate record
    exists."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = brdfscene.glossy_scene(S, W / H)
    reuse = L.di_resampling_settings() if mode == "reuse-basic" else None
    ls = L.di_light_sampling_settings("regir") if mode == "regir" else None
    outs = []
    for variant in ("never", "null", "zero"):
        s = _Session(ptamd, scene, W, H, di_history=reuse is not None)
        if variant == "null":
            s.r.direct_lighting.SetBrdfSampling(None)
        elif variant == "zero":
            s.r.direct_lighting.SetBrdfSampling(L.di_brdf_settings(samples=0, cutoff=0.5))
        for f in range(2):
            s.r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=70 + f), di_samples=8, di_reuse=reuse, di_light_sampling=ls)
        o = s.textures()
        o["__reservoirs"] = s.r.direct_lighting.download_reservoirs().view(np.uint8)
        assert len(s.r.direct_lighting.download_brdf_candidates()) == 0
        outs.append(o)
        s.close()
    assert (_half(outs[0]["Diffuse"])[..., :3] > 0).any()
    if reuse is not None:
        assert outs[0]["__reservoirs"].size == W * H * 32
    for o in outs[1:]:
        assert o.keys() == outs[0].keys()
        for k in o:
            assert np.array_equal(o[k], outs[0][k]), (mode, k)


# ---- 2. candidates pinned exactly ---------------------------------------------------------------------------------------------------------
def _records_vs_oracle(ptamd, pkg, oracle, scene, W, H, n_b, cutoff, frame):
    S, L = pkg.scenes, pkg.layouts
    s = _Session(ptamd, scene, W, H)
    s.r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=frame), di_samples=2, di_brdf=L.di_brdf_settings(n_b, cutoff))
    out = s.textures()
    got = s.r.direct_lighting.download_brdf_candidates()
    lights = s.r.direct_lighting.download_lights()
    overflows = s.ctx.counters().StackOverflows
    s.close()
    assert overflows == 0
    assert got.shape == (W * H * n_b,)
    got = got.reshape(H, W, n_b)
    sf = B.surfaces_f32(out, scene.camera)
    osc = oracle.OracleScene(scene, accel_mode=0)
    exp, info = B.replay_candidates(oracle, osc, sf, lights, frame, n_b, cutoff)
    osc.close()
    return got, exp, info, sf


RECORD_CASES = [(1, 0.0), (3, 0.0), (1, brdfscene.CUTOFF), (3, brdfscene.CUTOFF)]


def _candidates_pin(ptamd, pkg, oracle, n_b, cutoff, W, H):
    """download_brdf_candidates against the replay: or_bsdf_sample_batch on the surfaces rebuilt (float32, the device's steps) from the
    downloaded G-buffer, or_bsdf_evaluate for the all-lobe pdf, or_trace_closest. LightIndex equal; U, V and the pdf equal in their
    float32 bits; at every pixel (the empty surfaces hold empty records) and every candidate. No tolerance, nothing left out. The floors
    on what the frame must show (candidates on a light, rays that miss every light, rays the cutoff ends) are stated for 48 x 32 and
    taken as the same share of another size (dipins.more_than)."""
    S = pkg.scenes
    more = lambda value, count: dipins.more_than(value, count, W, H, 48, 32)
    got, exp, info, sf = _records_vs_oracle(ptamd, pkg, oracle, brdfscene.glossy_scene(S, W / H), W, H, n_b, cutoff, 40)
    lit = exp["LightIndex"] != 0xFFFFFFFF
    print(f"N_B {n_b} cutoff {cutoff} at {W} x {H}: {sf['valid'].sum()} valid pixels, {lit.sum()} candidates on a light, "
          f"{(exp['BrdfPdf'] > 0).sum()} rays traced")
    assert more(lit.sum(), 50) and more((~lit & (exp["BrdfPdf"] > 0)).sum(), 50)
    assert np.array_equal(got["LightIndex"], exp["LightIndex"])
    for k in ("U", "V", "BrdfPdf"):
        bad = got[k].view(np.uint32) != exp[k].view(np.uint32)
        assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[k][bad][:5], exp[k][bad][:5])
    if cutoff > 0:
        assert more(info["beyond"].sum(), 20)                             # rays that ended before a light they were heading for


@pytest.mark.gpu
@pytest.mark.parametrize("n_b,cutoff", RECORD_CASES)
def test_gpu_candidates_equal_the_oracle_replay(ptamd, pkg, oracle, n_b, cutoff):
    """_candidates_pin at 48 x 32"""
    _candidates_pin(ptamd, pkg, oracle, n_b, cutoff, 48, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", dipins.RAGGED, ids=dipins.size_id)
@pytest.mark.parametrize("n_b,cutoff", RECORD_CASES)
def test_gpu_candidates_equal_the_oracle_replay_ragged(ptamd, pkg, oracle, n_b, cutoff, size):
    """_candidates_pin at the sizes that cut the 16 x 16 block and the 8 x 8 wave tile of k_di_brdf_rays on both axes: the records are
    indexed (row * width + x) * N_B with an odd width, and the lanes outside the frame leave before the closest-hit walk"""
    _candidates_pin(ptamd, pkg, oracle, n_b, cutoff, *size)


@pytest.mark.gpu
def test_gpu_candidates_through_an_alpha_masked_pane(ptamd, pkg, oracle):
    """an alpha-masked pane between the glossy floor and the emitter: the closest-hit walk runs the alpha test, so rays go through the
    holes to the light and stop on the texels -- both happen, and every record equals the oracle's"""
    S = pkg.scenes
    W, H = 48, 32
    scene = brdfscene.glossy_scene(S, W / H, pane=True, bar=False)
    got, exp, info, sf = _records_vs_oracle(ptamd, pkg, oracle, scene, W, H, 1, 0.0, 40)
    pane = len(scene.objects) - 1
    floor_px = sf["valid"] & (np.abs(sf["P"][..., 1]) < 1e-3)
    through = (got["LightIndex"][..., 0] < 2) & floor_px
    stopped = (info["stopped"][..., 0] == pane) & floor_px & (got["LightIndex"][..., 0] == 0xFFFFFFFF)
    print(f"pane: {through.sum()} floor rays reach the quad light, {stopped.sum()} stop on the pane")
    assert through.sum() > 20 and stopped.sum() > 20
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


# ---- 3. reservoirs pinned per pixel ---------------------------------------------------------------------------------------------------------
RESERVOIR_CASES = [(8, 1, 0.0), (1, 1, 0.0), (2, 4, brdfscene.CUTOFF)]


def _brdf_reservoir_pin(ptamd, pkg, n_l, n_b, cutoff, source, W, H):
    """The initial reservoirs (temporal-only, Off, no boiling, history reset: the temporal pass stores them as they are) against
    brdfcandref fed the downloaded G-buffer, lights and candidate records. LightIndex, M, U, V exact; W relative to the float64
    value over the pixels at least 1e-5 away from every decision; those left out are counted and stay under 5 % of the valid pixels.
    The band on W: the reuse pins' 2e-5 does not hold here. Measured maxima: (8, 1) 6.4e-5 cdf / 8.9e-5 uniform, (1, 1) 1.18e-4 / 1.21e-4,
    (2, 4) with the cutoff 1.25e-4 / 1.25e-4 (p99 4.7e-5 to 7.3e-5), so the bound is twice the largest, 2.5e-4. The cause is the number
    format, not the weights: at this floor's roughness 0.25 (alpha^2 = 0.0039) one float32 ulp of NoH moves GGX's D by up to 4 / alpha^2
    ulps near the peak -- the oracle's float32 all-lobe pdf is 4.2e-5 away from float64 on identical inputs here, against 8e-6 at the
    reuse pins' roughness 0.4 -- and with BRDF candidates that pdf enters every weight through the blended pdf, where the light-only
    W = sum w / (M p-hat) cancels p-hat's share of it."""
    S, L = pkg.scenes, pkg.layouts
    frame = 40
    scene = brdfscene.glossy_scene(S, W / H)
    init = L.di_resampling_settings(temporal=True, spatial_samples=0, temporal_bias=L.DI_BIAS_CORRECTION_OFF, boiling_filter=False)
    s = _Session(ptamd, scene, W, H, di_history=True)
    s.r.direct_lighting.ResetHistory()
    s.r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=frame), di_samples=n_l, di_reuse=init,
               di_light_sampling=L.di_light_sampling_settings(source), di_brdf=L.di_brdf_settings(n_b, cutoff))
    out = s.textures()
    got = R.as_frame(s.r.direct_lighting.download_reservoirs(), H, W)
    rec = s.r.direct_lighting.download_brdf_candidates().reshape(H, W, n_b)
    lights = s.r.direct_lighting.download_lights()
    s.close()
    cur = R.Surfaces(out, scene.camera)
    exp, margin = B.initial_sampling(cur, lights, rec, frame, n_l, n_b, cutoff, source, bsdfref.Reference())
    sel = cur.valid & (margin >= NEAR)
    excluded = int((cur.valid & (margin < NEAR)).sum())
    assert (got["M"][cur.valid] == n_l + n_b).all()
    for k in ("LightIndex", "M"):
        bad = sel & (got[k] != exp[k])
        assert not bad.any(), (k, np.argwhere(bad)[:5].tolist(), got[k][bad][:5], exp[k][bad][:5], margin[bad][:5])
    for k in ("U", "V"):
        assert np.array_equal(got[k][sel].astype(np.float32), exp[k][sel].astype(np.float32)), k
    rel = np.abs(got["W"][sel] - exp["W"][sel]) / np.maximum(np.abs(exp["W"][sel]), 1e-30)
    rel = np.where((got["W"][sel] == 0) & (exp["W"][sel] == 0), 0.0, rel)
    print(f"({n_l}, {n_b}) {source} cutoff {cutoff} at {W} x {H}: {sel.sum()} pixels compared, {excluded} within {NEAR} of a decision "
          f"({excluded / max(1, int(cur.valid.sum())):.3%} of valid), W rel err max {rel.max():.2e} p99 {np.quantile(rel, 0.99):.2e}")
    assert sel.sum() > 0.4 * W * H and excluded < 0.05 * cur.valid.sum()
    assert rel.max() <= W_BAND, (rel.max(), np.argwhere(sel)[np.argmax(rel)].tolist())
    # some reservoirs hold a BRDF candidate's sample: a (U, V) that is one of the pixel's records
    held = (got["LightIndex"][..., None] == rec["LightIndex"].astype(np.int64)) & (got["U"][..., None].astype(np.float32) == rec["U"]) & \
        (got["V"][..., None].astype(np.float32) == rec["V"])
    assert dipins.more_than((held.any(-1) & sel).sum(), 10, W, H, 48, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["cdf", "uniform"])
@pytest.mark.parametrize("n_l,n_b,cutoff", RESERVOIR_CASES)
def test_gpu_initial_reservoirs_pinned(ptamd, pkg, n_l, n_b, cutoff, source):
    """_brdf_reservoir_pin at 48 x 32"""
    _brdf_reservoir_pin(ptamd, pkg, n_l, n_b, cutoff, source, 48, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", dipins.RAGGED, ids=dipins.size_id)
@pytest.mark.parametrize("source", ["cdf", "uniform"])
@pytest.mark.parametrize("n_l,n_b,cutoff", RESERVOIR_CASES)
def test_gpu_initial_reservoirs_pinned_ragged(ptamd, pkg, n_l, n_b, cutoff, source, size):
    """_brdf_reservoir_pin -- the MIS weights of the BRDF candidates inside the initial reservoirs -- at the sizes that cut every tile of
    the DI kernels on both axes: same scene, settings, band and caps (the floor on reservoirs that hold a BRDF candidate's sample is the
    48 x 32 one's share of the frame). Measured: nothing left out at either size; W rel err max 7.9e-5 at 37 x 23, 7.3e-5 at 21 x 13."""
    _brdf_reservoir_pin(ptamd, pkg, n_l, n_b, cutoff, source, *size)


# ---- 4. unbiased, and worth having ----------------------------------------------------------------------------------------------------------
def _direct(o):
    return _half(o["Diffuse"])[..., :3] + _half(o["Specular"])[..., :3]


@pytest.mark.gpu
def test_gpu_brdf_candidates_unbiased(ptamd, pkg):
    """Cornell box (GGX): the per-pixel means of (8, 1) and (8, 0) over the same frame indices agree within 4 standard errors on all but
    1 % of the selected pixels, with no bias over the whole set. The pixels are selected on other frames (DI > 0 in each of them)."""
    S, L = pkg.scenes, pkg.layouts
    W, H = 96, 64
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    on, off = _Session(ptamd, scene, W, H), _Session(ptamd, scene, W, H)
    valid = np.ones((H, W), bool)
    for f in range(16):
        off.r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=100 + f), di_samples=8)
        valid &= (_direct(off.textures()) > 0).any(-1)
    F = 128
    m_on, m_off = [], []
    for f in range(F):
        gs = S.graphics_settings(W, H, spp=1, bounces=1, frame_index=500 + f)
        on.r.render(gs, di_samples=8, di_brdf=L.di_brdf_settings(1))
        off.r.render(gs, di_samples=8)
        m_on.append(_direct(on.textures()) @ LUMA); m_off.append(_direct(off.textures()) @ LUMA)
    ceiling = (off.textures()["NormalRoughness"][..., 1].astype(np.float32) / 32767) < -0.9     # sees the light edge-on only
    on.close(); off.close()
    m_on, m_off = np.stack(m_on), np.stack(m_off)
    se = np.sqrt(m_on.var(0, ddof=1) / F + m_off.var(0, ddof=1) / F)
    sel = valid & (se > 0) & ~ceiling
    assert sel.sum() > 0.3 * W * H
    d = (m_on.mean(0) - m_off.mean(0))[sel]
    z = np.abs(d) / se[sel]
    print(f"unbiased: {sel.sum()} pixels, {np.mean(z > 4):.4f} beyond 4 standard errors, mean difference {d.mean():.3e} "
          f"(4 se of it {4 * np.sqrt((se[sel] ** 2).sum()) / sel.sum():.3e})")
    assert not np.array_equal(m_on, m_off)
    assert np.mean(z > 4) < 0.01
    assert abs(d.mean()) < 4 * np.sqrt((se[sel] ** 2).sum()) / sel.sum()


@pytest.mark.gpu
def test_gpu_brdf_candidates_cut_the_variance_on_a_glossy_plane(ptamd, pkg):
    """A rough-0.1 metallic plane seen from above, under a quad light that covers most of its upper hemisphere; two candidates per pixel
    either way: the variance of Specular over the frames with (1, 1) against (2, 0). The median of the per-pixel ratios is below 1 by
    more than its bootstrap standard error (measured: see DESIGN.md section 1, "BRDF candidates"), and the two means, averaged over the
    plane frame by frame, agree within 4 standard errors of their difference."""
    S, L = pkg.scenes, pkg.layouts
    W, H, F = 64, 48, 96
    scene = brdfscene.glossy_scene(S, W / H, roughness=0.1, metallic=1.0, bar=False, quad=((-3, 3), (-2, 4)), eye=((0, 1.0, -1.2), (0, -1, 0.8)))
    a, b = _Session(ptamd, scene, W, H), _Session(ptamd, scene, W, H)
    va, vb = [], []
    for f in range(F):
        gs = S.graphics_settings(W, H, spp=1, bounces=1, frame_index=900 + f)
        a.r.render(gs, di_samples=1, di_brdf=L.di_brdf_settings(1))
        b.r.render(gs, di_samples=2)
        va.append(_half(a.textures()["Specular"])[..., :3] @ LUMA); vb.append(_half(b.textures()["Specular"])[..., :3] @ LUMA)
    pos = a.textures()["Position"][..., :3]
    a.close(); b.close()
    va, vb = np.stack(va), np.stack(vb)
    floor = np.isfinite(pos).all(-1) & (np.abs(pos[..., 1]) < 1e-3)
    floor &= (vb.var(0) > 0) & (va.var(0) > 0)
    assert floor.sum() > 0.5 * W * H
    ratio = va[:, floor].var(0, ddof=1) / vb[:, floor].var(0, ddof=1)
    med = float(np.median(ratio))
    rng = np.random.default_rng(3)
    boot = np.array([np.median(rng.choice(ratio, len(ratio))) for _ in range(400)])
    d = va[:, floor].mean(1) - vb[:, floor].mean(1)                        # per frame: the frames are independent
    z = abs(d.mean()) / (d.std(ddof=1) / np.sqrt(F))
    print(f"glossy plane: {floor.sum()} pixels, median variance ratio (1, 1) / (2, 0) = {med:.4f} +- {boot.std(ddof=1):.4f} (bootstrap); "
          f"plane means {va[:, floor].mean():.4f} and {vb[:, floor].mean():.4f}, difference {z:.2f} standard errors")
    assert med + boot.std(ddof=1) < 1.0
    assert z < 4


# ---- 5. composition -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_two_ranks_reproduce_the_unsharded_frame(ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 48
    scene = brdfscene.glossy_scene(S, W / H)
    gs = S.graphics_settings(W, H, spp=1, bounces=1, frame_index=7)
    brdf = L.di_brdf_settings(1)
    full = _Session(ptamd, scene, W, H, with_f32=True)
    full.r.render(gs, di_samples=4, di_brdf=brdf)
    ref = full.textures()
    ref_rec = full.r.direct_lighting.download_brdf_candidates().reshape(H, W)
    full.close()
    bands, recs = [], []
    for rank in range(2):
        s = _Session(ptamd, scene, W, H, sharding=(rank, 2, 8), with_f32=True)
        s.r.render(gs, di_samples=4, di_brdf=brdf)
        bands.append(s.textures())
        recs.append(s.r.direct_lighting.download_brdf_candidates().reshape(-1, W))
        s.close()
    for k in ("Diffuse", "Specular", "RadianceF32", "__records"):
        rows = [None] * H
        for rank in range(2):
            lr = 0
            for b in range(rank, (H + 7) // 8, 2):
                for y in range(b * 8, min(H, b * 8 + 8)):
                    rows[y] = (recs[rank] if k == "__records" else bands[rank][k])[lr]; lr += 1
        assert np.array_equal(np.stack(rows), ref_rec if k == "__records" else ref[k]), k
    assert (ref_rec["LightIndex"] != 0xFFFFFFFF).sum() > 50 and (_half(ref["Specular"])[..., :3] > 0).any()


@pytest.mark.gpu
def test_gpu_reuse_visibility_pairwise_with_brdf_candidates(ptamd, pkg):
    """reuse + visibility + Pairwise on, N_B = 1: a four-frame sequence is deterministic across two runs and finite, uses its history,
    and differs from the same sequence without BRDF candidates"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 64, 48
    scene = brdfscene.glossy_scene(S, W / H)

    def run(brdf):
        s = _Session(ptamd, scene, W, H, di_history=True)
        for f in range(4):
            s.r.render(S.graphics_settings(W, H, spp=1, bounces=1, frame_index=20 + f), di_samples=4, di_reuse=L.di_resampling_settings(),
                       di_visibility=L.di_visibility_settings(), di_pairwise=L.di_pairwise_settings(temporal=True, spatial=True), di_brdf=brdf)
        o = s.textures()
        res = s.r.direct_lighting.download_reservoirs()
        s.close()
        return o, res
    o1, r1 = run(L.di_brdf_settings(1))
    o2, r2 = run(L.di_brdf_settings(1))
    o0, r0 = run(None)
    for k in ("Diffuse", "Specular"):
        assert np.array_equal(o1[k], o2[k]), k
        assert np.isfinite(_half(o1[k])).all()
    assert np.array_equal(r1.view(np.uint8), r2.view(np.uint8))
    assert np.isfinite(r1["W"]).all() and (r1["W"] >= 0).all() and (r1["M"] > 5).any() and (r0["M"] > 4).any()
    assert (r1["M"][r1["M"] > 0] % 1 == 0).all() and r1["M"].max() > r0["M"].max()           # five candidates a frame against four
    assert not np.array_equal(o1["Specular"], o0["Specular"])


@pytest.mark.gpu
def test_cpp_host_brdf_frame_matches_python(tmp_path, ptamd, pkg):
    """pt_demo --di --di-brdf-samples 1: the C++ host's DirectLighting::SetBrdfSampling writes the radiance bytes of the Python binding"""
    demo = os.path.join(ge.PKG_DIR, "pt_demo")
    S, L = pkg.scenes, pkg.layouts
    W, H, spp, bounces = 96, 64, 1, 2
    out = str(tmp_path / "radiance.bin")
    subprocess.check_call([demo, "--di", "--di-samples", "6", "--di-brdf-samples", "1", "--width", str(W), "--height", str(H), "--spp", str(spp),
                           "--bounces", str(bounces), "--frames", "1", "--out", out], timeout=300)
    got = np.fromfile(out, np.float32).reshape(H, W, 4)
    scene = S.cornell_box(aspect=W / H, variant="ggx")
    s = _Session(ptamd, scene, W, H, with_f32=True)
    gs = S.graphics_settings(W, H, spp=spp, bounces=bounces, frame_index=0)
    gs["IsDIEnabled"] = 1
    s.r.render(gs, di_samples=6, di_brdf=L.di_brdf_settings(1))
    ref = s.textures()["RadianceF32"]
    s.r.render(gs, di_samples=6)
    off = s.textures()["RadianceF32"]
    s.close()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(ref, off)


@pytest.mark.gpu
def test_gpu_setter_refuses_and_keeps_the_previous_setting(ptamd, pkg):
    """9 samples, a negative cutoff, a NaN cutoff and a cutoff of 1 are refused; the frame after a refusal is byte-identical to the frame
    before it (the same frame index: the previous setting, N_B = 2 with a cutoff, is still the active one)"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 48, 32
    scene = brdfscene.glossy_scene(S, W / H)
    s = _Session(ptamd, scene, W, H)
    gs = S.graphics_settings(W, H, spp=1, bounces=1, frame_index=5)
    s.r.render(gs, di_samples=4, di_brdf=L.di_brdf_settings(2, brdfscene.CUTOFF))
    before = s.textures()
    rec_before = s.r.direct_lighting.download_brdf_candidates()
    assert rec_before.shape == (W * H * 2,)
    for bad in (L.di_brdf_settings(9), L.di_brdf_settings(1, -0.1), L.di_brdf_settings(1, float("nan")), L.di_brdf_settings(1, 1.0),
                L.di_brdf_settings(0, 1.5)):
        with pytest.raises((ptamd.PtInvalidArgument, ptamd.PtError, ValueError)):
            s.r.direct_lighting.SetBrdfSampling(bad)
        s.r._di_brdf_set = False                                           # render() leaves the setter alone
        s.r.render(gs, di_samples=4)
        after = s.textures()
        for k in ("Diffuse", "Specular", "Radiance"):
            assert np.array_equal(after[k], before[k]), k
        assert np.array_equal(s.r.direct_lighting.download_brdf_candidates().view(np.uint8), rec_before.view(np.uint8))
    s.r.direct_lighting.SetBrdfSampling(None)
    s.r.render(gs, di_samples=4)
    assert len(s.r.direct_lighting.download_brdf_candidates()) == 0
    assert not np.array_equal(s.textures()["Specular"], before["Specular"])
    s.close()
