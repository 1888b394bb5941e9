"""GPU tests of the post-processing chain (pt_post_set_constants / pt_post_render / pt_post_download_bloom) against the numpy restatement
of its spec (tests/postref.py).

Bounds (fp16 ulps on the ordered line; NaN matches NaN only):
  stages 2-8        bit for bit, each stage fed the device's own image of the stage before
  stages 0-1        <= 1 ulp of the float64 Karis weight (powf on the device)
  Color             <= 1 ulp of the restatement's resolve of the device's Radiance and stage-8 image (powf in the tone map)
  BackBuffer / Display8   exactly the encodes of the device's Color
  end to end        Color <= 4 ulps, BackBuffer / Display8 <= 1 code of the restatement run on Radiance alone
Every mutation of postref.MUTATIONS breaks one of these bounds against the device output."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import postref as R
from test_post_processing_rules import MUTATION_SETTINGS, RAW_CASES, SETTINGS_CASES, settings_args

pytestmark = pytest.mark.gpu

STAGE01_ULPS, COLOR_ULPS, E2E_COLOR_ULPS, E2E_CODES = 1, 1, 4, 1
SIZES = [(1920, 1080), (1917, 1083), (64, 33), (32, 2), (2, 32)]
DEMO = os.path.join(ge.PKG_DIR, "pt_demo")


def _torch():
    import torch
    return torch


def run(ctx, ptamd, L, radiance, settings, outputs=("Color", "BackBuffer", "Display8"), op=None):
    """one pt_post_render of `radiance` (fp16 bits, (H, W, 4)): the bound outputs and, with bloom on, the nine stage images"""
    torch = _torch()
    H, W = radiance.shape[:2]
    dev = torch.device("cuda", ctx.device_ordinal)
    rad = torch.from_numpy(radiance.view(np.int16).copy()).to(dev)
    outs = ptamd.alloc_post_textures(W, H, dev)
    op = op or ptamd.PostProcessing(ctx)
    op.SetConstants(settings)
    op.Render({"Radiance": rad, **{k: outs[k] for k in outputs}})
    ctx.sync()
    res = {k: outs[k].cpu().numpy().view(np.dtype(L.POST_FORMATS[k][0])) for k in outputs}
    res["stages"] = [op.download_bloom(s) for s in range(R.STAGES)] if int(np.asarray(settings)["IsBloomEnabled"]) else []
    return res


def stage_ulps(res, radiance, s, mut=()):
    """fp16-ulp distance of the device's stage s image from the restatement fed the device's image of stage s - 1"""
    H, W = radiance.shape[:2]
    _, _, din, dout = R.stage_table(W, H)[s]
    src = R.h2f(radiance[..., :3]) if s == 0 else R.h2f(res["stages"][s - 1][..., :3])
    down = R.h2f(res["stages"][2 * (R.MIPS - 1) - s][..., :3]) if s >= R.MIPS else None
    if "fp32_levels" in mut and s >= 3:              # the stage before, kept unrounded
        dout2 = R.stage_table(W, H)[s - 1][3]
        src = np.asarray(R.stage(s - 1, R.h2f(res["stages"][s - 2][..., :3]), dout2, mut), np.float32)
    got = res["stages"][s]
    assert got.shape == (dout[1], dout[0], 4) and np.all(got[..., 3] == 0)          # the float3 store leaves 0 in alpha
    return R.f16_ulps(got[..., :3], R.f16(R.stage(s, src, dout, mut, down)))


def resolve_ulps(res, radiance, settings, mut=()):
    blur = res["stages"][-1] if res["stages"] else None
    color, back, d8 = R.resolve(radiance, blur, settings, mut)
    return R.f16_ulps(res["Color"], color)


def check_against_restatement(res, radiance, settings, label, end_to_end=True):
    stats = {}
    for s in range(len(res["stages"])):
        d = stage_ulps(res, radiance, s)
        stats[f"stage{s}"] = (int(d.max()), float((d > 0).mean()))
        assert d.max() <= (STAGE01_ULPS if s < 2 else 0), (label, s, stats[f"stage{s}"])
    d = resolve_ulps(res, radiance, settings)
    stats["color"] = (int(d.max()), float((d > 0).mean()))
    assert d.max() <= COLOR_ULPS, (label, stats["color"])
    back, d8 = R.encode(res["Color"])
    assert np.array_equal(res["BackBuffer"], back) and np.array_equal(res["Display8"], d8), label
    if end_to_end:
        _, color, back_r, d8_r = R.post_process(radiance, settings)
        d = R.f16_ulps(res["Color"], color)
        codes = max(int(np.abs(((res["BackBuffer"][..., None] >> np.array([0, 10, 20], np.uint32)) & 1023).astype(np.int64)
                               - ((back_r[..., None] >> np.array([0, 10, 20], np.uint32)) & 1023).astype(np.int64)).max()),
                    int(np.abs(res["Display8"].astype(np.int64) - d8_r.astype(np.int64)).max()))
        stats["e2e_color"] = (int(d.max()), float((d > 0).mean()))
        stats["e2e_codes"] = codes
        assert d.max() <= E2E_COLOR_ULPS and codes <= E2E_CODES, (label, stats)
    print(label, json.dumps(stats))
    return stats


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_bloom_stages_and_outputs_match_the_restatement(gpu, ptamd, pkg, size):
    W, H = size
    L = pkg.layouts
    radiance = R.make_frame(W, H, seed=W * 7 + H)
    s = L.post_processing_settings(W, H)
    res = run(gpu, ptamd, L, radiance, s)
    assert [x.shape[:2] for x in res["stages"]] == [(d[1], d[0]) for _, _, _, d in R.stage_table(W, H)]
    check_against_restatement(res, radiance, s, f"{W}x{H}")


SETTINGS_GRID = [dict(operator="saturate"), dict(operator="reinhard"), dict(operator="aces_filmic", exposure=-10.0),
                 dict(exposure=3.5), dict(strength=0.0), dict(strength=1.0), dict(bloom=False), dict(bloom=False, operator="reinhard"),
                 dict(hdr=True, rotation="hdtv_to_uhdtv"), dict(hdr=True, rotation="dci_p3_d65_to_uhdtv"),
                 dict(hdr=True, rotation="hdtv_to_dci_p3_d65", paper_white_nits=1000.0), dict(hdr=True, bloom=False)]


@pytest.mark.parametrize("kw", SETTINGS_GRID, ids=["-".join(f"{k}={v}" for k, v in kw.items()) for kw in SETTINGS_GRID])
def test_every_setting_matches_the_restatement(gpu, ptamd, pkg, kw):
    L = pkg.layouts
    W, H = 131, 77
    radiance = R.make_frame(W, H, seed=11)
    radiance[..., 3] = R.f16(np.float32(0.75))                 # bloom off passes Radiance's alpha through
    s = L.post_processing_settings(W, H, **kw)
    res = run(gpu, ptamd, L, radiance, s)
    check_against_restatement(res, radiance, s, str(kw))
    assert np.all(res["Color"][..., 3] == (0 if kw.get("bloom", True) else R.f16(np.float32(0.75))))


def test_every_mutation_exceeds_the_bounds(gpu, ptamd, pkg):
    L = pkg.layouts
    W, H = 96, 54
    radiance = R.make_frame(W, H, seed=13)
    cache = {}
    for mut in R.MUTATIONS:
        kw = MUTATION_SETTINGS.get(mut, {})
        key = tuple(sorted(kw.items()))
        s = L.post_processing_settings(W, H, **kw)
        if key not in cache:
            cache[key] = run(gpu, ptamd, L, radiance, s)
            check_against_restatement(cache[key], radiance, s, f"unmutated {kw}", end_to_end=False)
        res = cache[key]
        worst = {}
        for st in range(R.STAGES):
            worst[f"stage{st}"] = int(stage_ulps(res, radiance, st, (mut,)).max())
        worst["color"] = int(resolve_ulps(res, radiance, s, (mut,)).max())
        back, d8 = R.encode(res["Color"], (mut,))
        exceeded = (any(worst[f"stage{st}"] > (STAGE01_ULPS if st < 2 else 0) for st in range(R.STAGES)) or worst["color"] > COLOR_ULPS
                    or not np.array_equal(back, res["BackBuffer"]) or not np.array_equal(d8, res["Display8"]))
        print(mut, json.dumps(worst))
        assert exceeded, (mut, worst)


def test_refusals_keep_the_previous_settings(ptamd, pkg):
    L = pkg.layouts
    torch = _torch()
    ctx = ptamd.DeviceContext(0)
    try:
        dev = torch.device("cuda", 0)
        W, H = 64, 33
        radiance = R.make_frame(W, H, seed=17)
        op = ptamd.PostProcessing(ctx)
        rad = torch.from_numpy(radiance.view(np.int16).copy()).to(dev)
        outs = ptamd.alloc_post_textures(W, H, dev)
        with pytest.raises(ptamd.PtError):                           # PT_ERROR_NOT_READY before any settings
            op.Render({"Radiance": rad, "Color": outs["Color"]})
        good = L.post_processing_settings(W, H, bloom=False, operator="reinhard")
        first = run(ctx, ptamd, L, radiance, good, op=op)
        for over, ok in SETTINGS_CASES:
            w, h, kw = settings_args(over)
            s = L.post_processing_settings(64, 33)              # the case's fields written raw: the library does its own checks
            s["RenderSize"] = (w, h)
            for k, v in kw.items():
                field = {"strength": "BloomStrength", "exposure": "Exposure", "paper_white_nits": "PaperWhiteNits", "operator": "ToneMappingOperator",
                         "rotation": "ColorPrimaryRotation", "hdr": "IsHDREnabled", "bloom": "IsBloomEnabled"}[k]
                if k == "operator" and isinstance(v, str):
                    v = L.TONE_MAP_OPERATORS[v]
                if k == "rotation" and isinstance(v, str):
                    v = L.COLOR_ROTATIONS[v]
                s[field] = v
            st = ctx.lib.pt_post_set_constants(ctx.handle, C.c_void_p(s.ctypes.data))
            assert (st == 0) == ok, (over, st)
            op.SetConstants(good)
        for field, value in RAW_CASES:
            s = L.post_processing_settings(W, H)
            s[field] = value
            with pytest.raises(ptamd.PtInvalidArgument):
                op.SetConstants(s)
        s = L.post_processing_settings(W, H)
        s["ToneMappingOperator"] = 9
        with pytest.raises(ptamd.PtInvalidArgument):
            op.SetConstants(s)
        again = run(ctx, ptamd, L, radiance, good, op=op)           # SetConstants(good) again inside run: same image as before the refusals
        for k in ("Color", "BackBuffer", "Display8"):
            assert np.array_equal(first[k], again[k]), k
        # a refused SetConstants leaves the previous settings active: render without setting them again
        bad = L.post_processing_settings(W, H)
        bad["Exposure"] = 11.0
        with pytest.raises(ptamd.PtInvalidArgument):
            op.SetConstants(bad)
        op.Render({"Radiance": rad, **outs}); ctx.sync()
        assert np.array_equal(outs["Color"].cpu().numpy().view(np.uint16), first["Color"])
        # too small for five mips with bloom on; NULL Radiance; no output bound
        for w, h in ((31, 31), (33, 1), (1, 40)):
            small = L.post_processing_settings(w, h)
            op.SetConstants(small)
            r = torch.zeros((h, w, 4), dtype=torch.int16, device=dev)
            c = torch.zeros((h, w, 4), dtype=torch.int16, device=dev)
            with pytest.raises(ptamd.PtInvalidArgument):
                op.Render({"Radiance": r, "Color": c})
        op.SetConstants(good)
        with pytest.raises(ptamd.PtInvalidArgument):
            op.Render({"Color": outs["Color"]})
        with pytest.raises(ptamd.PtInvalidArgument):
            op.Render({"Radiance": rad})
        with pytest.raises(ptamd.PtInvalidArgument):
            op.download_bloom(9)
    finally:
        ctx.close()


def test_two_runs_are_bit_identical_and_a_size_change_works(gpu, ptamd, pkg):
    L = pkg.layouts
    a_rad = R.make_frame(1920, 1080, seed=23)
    s = L.post_processing_settings(1920, 1080, strength=0.5)
    small = R.make_frame(64, 33, seed=29)
    s_small = L.post_processing_settings(64, 33)
    op = ptamd.PostProcessing(gpu)
    first_small = run(gpu, ptamd, L, small, s_small, op=op)
    a = run(gpu, ptamd, L, a_rad, s, op=op)                          # grows the pyramid
    b = run(gpu, ptamd, L, a_rad, s, op=op)
    for k in ("Color", "BackBuffer", "Display8"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["stages"], b["stages"]))
    again_small = run(gpu, ptamd, L, small, s_small, op=op)          # back to the small size in the grown pyramid
    for k in ("Color", "BackBuffer", "Display8"):
        assert np.array_equal(first_small[k], again_small[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(first_small["stages"], again_small["stages"]))
    off = run(gpu, ptamd, L, small, L.post_processing_settings(64, 33, bloom=False), op=op)
    assert off["stages"] == []
    assert op.download_bloom(8).shape == first_small["stages"][8].shape   # the last render with bloom on


def test_independent_of_scene_and_sharding_and_destroy_after_use(ptamd, pkg):
    L, S = pkg.layouts, pkg.scenes
    W, H = 160, 90
    radiance = R.make_frame(W, H, seed=31)
    s = L.post_processing_settings(W, H)
    plain = ptamd.DeviceContext(0)
    ref = run(plain, ptamd, L, radiance, s)
    plain.close()                                                    # pt_destroy after use
    ctx = ptamd.DeviceContext(0)
    try:
        scene = ptamd.Scene(ctx, S.cornell_box(aspect=W / H))
        ctx.set_sharding(1, 2, 16)
        got = run(ctx, ptamd, L, radiance, s)
        for k in ("Color", "BackBuffer", "Display8"):
            assert np.array_equal(ref[k], got[k]), k
        assert all(np.array_equal(x, y) for x, y in zip(ref["stages"], got["stages"]))
        scene.close()
    finally:
        ctx.close()


def test_c2_cornell_1080p_then_the_chain_at_the_reference_defaults(gpu, ptamd, pkg):
    """C2 (1920 x 1080, 4 spp, 8 bounces), then Bloom + Merge + ToneMap + Copy at MyAppData's defaults: the outputs are the restatement
    applied to the frame's downloaded Radiance; a sharded renderer refuses post"""
    S, L = pkg.scenes, pkg.layouts
    W, H = 1920, 1080
    gpu.set_sharding(0, 1, 16)
    scene = ptamd.Scene(gpu, S.cornell_box(aspect=W / H, variant="ggx"))
    r = ptamd.Renderer(gpu, scene, W, H)
    s = L.post_processing_settings(W, H)
    r.render(S.graphics_settings(W, H, spp=4, bounces=8), post=s)
    gpu.sync()
    out = ptamd.textures_to_numpy(r.textures)
    res = {k: out[k] for k in ("Color", "BackBuffer", "Display8")}
    res["stages"] = [r.post.download_bloom(st) for st in range(R.STAGES)]
    stats = check_against_restatement(res, out["Radiance"], s, "C2 1080p")
    assert out["Display8"][..., :3].mean() > 20 and stats["e2e_codes"] <= 1
    gpu.set_sharding(0, 2, 16)
    try:
        sharded = ptamd.Renderer(gpu, scene, W, H)
        with pytest.raises(ptamd.PtInvalidArgument):
            sharded.render(S.graphics_settings(W, H, spp=1, bounces=1), post=s)
    finally:
        gpu.set_sharding(0, 1, 16)
        scene.close()


def test_pt_demo_post_png_is_the_python_display8(tmp_path, gpu, ptamd, pkg):
    from PIL import Image
    S, L = pkg.scenes, pkg.layouts
    W, H = 160, 90
    png, disp = str(tmp_path / "f.png"), str(tmp_path / "f.bin")
    subprocess.check_call([DEMO, "--width", str(W), "--height", str(H), "--spp", "2", "--bounces", "4", "--frames", "2", "--post",
                           "--png", png, "--out-display", disp])
    gpu.set_sharding(0, 1, 16)
    scene = ptamd.Scene(gpu, S.cornell_box(aspect=W / H, variant="ggx"))
    r = ptamd.Renderer(gpu, scene, W, H)
    r.render(S.graphics_settings(W, H, spp=2, bounces=4, frame_index=0), post=L.post_processing_settings(W, H))
    gpu.sync()
    out = ptamd.textures_to_numpy(r.textures)
    scene.close()
    im = np.asarray(Image.open(png))
    assert im.shape == (H, W, 3) and np.array_equal(im, out["Display8"][..., :3])
    assert np.array_equal(np.fromfile(disp, np.uint32).reshape(H, W), out["BackBuffer"])
    # the multi-rank path (child process per rank, gather, then the chain on rank 0) gives the same back buffer
    disp1 = str(tmp_path / "r1.bin")
    subprocess.check_call([DEMO, "--width", str(W), "--height", str(H), "--spp", "2", "--bounces", "4", "--frames", "2", "--post",
                           "--out-display", disp1, "--ranks", "1"])
    assert np.array_equal(np.fromfile(disp1, np.uint32), np.fromfile(disp, np.uint32))
