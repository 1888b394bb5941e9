"""GPU tests of the NRD composition pass (pt_nrd_composition_process) against tests/nrdref.py, the numpy restatement of DESIGN.md
section 1, "NRD composition": synthetic hostile textures bit for bit in both launch forms, aliased against separate denoised textures,
the refusals, the round trip through the identity denoiser that closes DESIGN.md section 0 row f4 against the Denoiser = None frame, a
sharded context, the C++ host and the post-processing chain behind the pass."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import nrdref as R

pytestmark = pytest.mark.gpu

DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
SIZES = [(37, 23), (130, 3)]          # partial waves; 390 pixels = 195 lanes of the two-pixel form, and 851 pixels: an odd last pixel
# The alpha of the two ReBLUR-packed textures is the one value that is not bit-pinned (exp2f in the hit-distance normalisation). Largest
# deviation from nrdref's correctly rounded exp2, in fp16 ulps, measured over this file's synthetic inputs on an MI355X (both forms,
# both sizes, the defaults and the second parameter set); the limit is that plus one ulp.
REBLUR_ALPHA_MEASURED_ULPS = 0
REBLUR_ALPHA_LIMIT_ULPS = REBLUR_ALPHA_MEASURED_ULPS + 1
HIT_DISTANCE_SETS = [None, (1.5, 0.25, 8.0, -6.0)]


def _torch():
    import torch
    return torch


def hostile_textures(W, H, seed):
    """Random textures of a W x H frame with every hostile texel of the issue seeded in: albedo channels of 0, zero over zero, negative /
    NaN / +-inf radiance, 65504 and values that overflow fp16 after the division, hit distances 0 / subnormal / inf / NaN, roughness 0
    and 1, non-finite LinearDepth on a tenth of the pixels, negative LinearDepth. uint16 fp16 bits (H, W, 4), depth float32 (H, W),
    NormalRoughness int16 (H, W, 4)."""
    rng = np.random.default_rng(seed)
    n = W * H

    def f16(x):
        with np.errstate(over="ignore"):
            return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)

    def colour(lo, hi):
        return f16(np.exp2(rng.uniform(lo, hi, (n, 4))))

    def seed_in(t, values, share=0.04, channels=(0, 1, 2)):
        for v in values:
            m = rng.random((n, len(channels))) < share
            sub = t[:, list(channels)]
            sub[m] = v
            t[:, list(channels)] = sub

    nan_a, nan_b, inf, ninf = 0x7E00, 0xFC01, 0x7C00, 0xFC00          # a quiet NaN, a signalling one with a sign, +-inf
    tex = {}
    for name in ("DiffuseAlbedo", "SpecularAlbedo"):
        t = colour(-7, 0)
        seed_in(t, [0x0000, 0x8000, f16(0.01), f16(1.0), 0x0001], 0.05)           # 0, -0, the G-buffer's floor, 1, the smallest subnormal
        tex[name] = t
    for name in ("NoisyDiffuse", "NoisySpecular", "DenoisedDiffuse", "DenoisedSpecular"):
        t = colour(-12, 9)
        seed_in(t, [0x0000, f16(-2.5), nan_a, nan_b, inf, ninf, f16(65504.0), f16(60000.0), 0x0001, 0x03FF], 0.03)
        seed_in(t, [0x0000, 0x0001, 0x03FF, inf, ninf, nan_a, nan_b, f16(-1.0), f16(65504.0), f16(1e-7)], 0.06, channels=(3,))   # hit distance
        tex[name] = t
    zero_over_zero = rng.random(n) < 0.05
    for a, q in (("DiffuseAlbedo", "NoisyDiffuse"), ("SpecularAlbedo", "NoisySpecular")):
        tex[a][zero_over_zero, 1] = 0
        tex[q][zero_over_zero, 1] = 0
    t = colour(-10, 6)
    seed_in(t, [0x0000, nan_a, inf, ninf, f16(-1.0), f16(65504.0)], 0.03)
    t[:, 3] = rng.integers(0, 65536, n).astype(np.uint16)                          # Radiance's alpha: any bits, NaN patterns included
    tex["Radiance"] = t
    nr = rng.integers(-32768, 32768, (n, 4)).astype(np.int16)
    nr[rng.random(n) < 0.1, 3] = 0
    nr[rng.random(n) < 0.1, 3] = 32767
    nr[rng.random(n) < 0.02, 3] = -32768
    tex["NormalRoughness"] = nr
    depth = np.exp2(rng.uniform(-6, 12, n)).astype(np.float32)
    depth[rng.random(n) < 0.15] *= np.float32(-1.0)
    depth[rng.random(n) < 0.02] = 0.0
    dead = rng.permutation(n)[: max(3, n // 10)]
    depth[dead] = np.array([np.inf, -np.inf, np.nan], np.float32)[np.arange(len(dead)) % 3]
    out = {k: v.reshape(H, W, 4) for k, v in tex.items()}
    out["LinearDepth"] = depth.reshape(H, W)
    return out


def upload(tex, dev, one_texel_aligned=False):
    """device tensors of the textures. one_texel_aligned: every tensor is a view that starts one texel into its allocation, so that it is
    aligned to its texel (8 bytes; LinearDepth 4) and not to two: the library then launches the one-pixel form."""
    torch = _torch()
    out = {}
    for k, v in tex.items():
        flat = np.ascontiguousarray(v).view(np.int16 if v.dtype.itemsize == 2 else v.dtype).reshape(-1)
        lead = (4 if v.dtype.itemsize == 2 else 1) if one_texel_aligned else 0
        buf = torch.zeros(lead + flat.size, dtype=torch.from_numpy(flat[:1]).dtype, device=dev)
        t = buf[lead:].view(v.shape)
        t.copy_(torch.from_numpy(flat.copy()).view(v.shape))
        assert t.data_ptr() % (2 * flat.itemsize * (4 if v.ndim == 3 else 1)) == (lead * flat.itemsize)
        out[k] = t
    return out


def download(dtex, like):
    return {k: dtex[k].cpu().numpy().view(like[k].dtype).reshape(like[k].shape) for k in like}


def raw_constants(L, W, H, denoiser, is_pack, hit_distance=None):
    """PtNRDCompositionConstants without the helper's checks (the refusal tests hand the library what the helper would not)"""
    k = np.zeros((), L.NRD_COMPOSITION_CONSTANTS)
    k["RenderSize"] = (W, H); k["IsPack"] = is_pack; k["Denoiser"] = denoiser
    k["ReBLURHitDistance"] = L.NRD_REBLUR_HIT_DISTANCE_DEFAULTS if hit_distance is None else hit_distance
    return k


def alpha_ulps(got, want):
    """deviation of fp16 alphas in fp16 ulps of the expected value, compared in float64"""
    g, w = R.f16_to_f32(got).astype(np.float64), R.f16_to_f32(want).astype(np.float64)
    assert np.isfinite(g).all() and np.isfinite(w).all()
    return float((np.abs(g - w) / R.ulp16(w)).max())


def assert_same(got, want, label):
    assert got.dtype == want.dtype and np.array_equal(got, want), (label, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


@pytest.fixture(scope="module")
def nrd_stats():
    stats = {"reblur_alpha_ulps": 0.0}
    yield stats
    print("\nNRD composition: largest ReBLUR alpha deviation %.3f fp16 ulps (limit %d)" % (stats["reblur_alpha_ulps"], REBLUR_ALPHA_LIMIT_ULPS))


@pytest.mark.parametrize("one_pixel_form", [False, True], ids=["two-pixel-form", "one-pixel-form"])
@pytest.mark.parametrize("denoiser", [0, 1, 2, 3], ids=["none", "dlss-rr", "reblur", "relax"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic_textures_bit_for_bit(gpu, ptamd, pkg, nrd_stats, size, denoiser, one_pixel_form):
    L = pkg.layouts
    W, H = size
    dev = _torch().device("cuda", gpu.device_ordinal)
    op = ptamd.NRDComposition(gpu)
    for hd in HIT_DISTANCE_SETS if denoiser == L.DENOISER_NRD_REBLUR else [None]:
        P = R.REBLUR_HIT_DISTANCE_DEFAULTS if hd is None else hd
        host = hostile_textures(W, H, seed=W * 131 + H)
        assert (~np.isfinite(host["LinearDepth"])).sum() >= W * H // 10
        dtex = upload(host, dev, one_texel_aligned=one_pixel_form)
        for pack in (True, False):                         # the form the library takes for these tensors: what this case is about
            assert ptamd.nrd_composition_pixels_per_lane({n: t.data_ptr() for n, t in dtex.items()},
                                                         L.nrd_composition_constants(W, H, denoiser, pack, hd)) == (1 if one_pixel_form else 2)
        # ---- the pack
        op.Process(dtex, L.nrd_composition_constants(W, H, denoiser, True, hd))
        gpu.sync()
        got = download(dtex, host)
        want_d, want_s = R.pack(denoiser, host["LinearDepth"], host["DiffuseAlbedo"], host["SpecularAlbedo"], host["NormalRoughness"],
                                host["NoisyDiffuse"], host["NoisySpecular"], P)
        for name, want in (("NoisyDiffuse", want_d), ("NoisySpecular", want_s)):
            assert_same(got[name][..., :3], want[..., :3], ("pack rgb", name, denoiser))
            dead = ~np.isfinite(host["LinearDepth"])
            assert_same(got[name][dead], host[name][dead], ("pack untouched", name))
            if denoiser == L.DENOISER_NRD_REBLUR:
                u = alpha_ulps(got[name][..., 3][~dead], want[..., 3][~dead])
                nrd_stats["reblur_alpha_ulps"] = max(nrd_stats["reblur_alpha_ulps"], u)
                print(f"ReBLUR alpha {name} {W}x{H} one_pixel_form={one_pixel_form} P={P}: {u:.3f} fp16 ulps")
                assert u <= REBLUR_ALPHA_LIMIT_ULPS, (name, u)
            else:
                assert_same(got[name][..., 3], want[..., 3], ("pack alpha", name, denoiser))
        for name in ("LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "DenoisedDiffuse", "DenoisedSpecular", "Radiance"):
            assert got[name].tobytes() == host[name].tobytes(), ("the pack wrote", name)
        # ---- the compose, once on the device's own packed pair (aliased: the identity denoiser), once on hostile denoised textures
        for den_d, den_s in (("NoisyDiffuse", "NoisySpecular"), ("DenoisedDiffuse", "DenoisedSpecular")):
            before = download(dtex, host)
            bind = dict(dtex, DenoisedDiffuse=dtex[den_d], DenoisedSpecular=dtex[den_s])
            op.Process(bind, L.nrd_composition_constants(W, H, denoiser, False, hd))
            gpu.sync()
            after = download(dtex, host)
            want = R.compose(denoiser, before["LinearDepth"], before["DiffuseAlbedo"], before["SpecularAlbedo"], before[den_d], before[den_s],
                             before["Radiance"])
            assert_same(after["Radiance"], want, ("compose", den_d, denoiser))
            assert_same(after["Radiance"][..., 3], before["Radiance"][..., 3], "Radiance alpha")
            for name in before:
                if name != "Radiance":
                    assert after[name].tobytes() == before[name].tobytes(), ("the compose wrote", name)


@pytest.mark.parametrize("denoiser", [2, 3], ids=["reblur", "relax"])
def test_aliased_and_separate_denoised_textures_agree(gpu, ptamd, pkg, denoiser):
    L = pkg.layouts
    W, H = SIZES[0]
    dev = _torch().device("cuda", gpu.device_ordinal)
    op = ptamd.NRDComposition(gpu)
    host = hostile_textures(W, H, seed=5)
    results = []
    for aliased in (True, False):
        dtex = upload(host, dev)
        op.Process(dtex, L.nrd_composition_constants(W, H, denoiser, True))
        if aliased:
            bind = dict(dtex, DenoisedDiffuse=dtex["NoisyDiffuse"], DenoisedSpecular=dtex["NoisySpecular"])
        else:
            bind = dict(dtex, DenoisedDiffuse=dtex["NoisyDiffuse"].clone(), DenoisedSpecular=dtex["NoisySpecular"].clone())
        op.Process(bind, L.nrd_composition_constants(W, H, denoiser, False))
        gpu.sync()
        results.append(dtex["Radiance"].cpu().numpy().view(np.uint16))
    assert np.array_equal(results[0], results[1]) and not np.array_equal(results[0], host["Radiance"])


def test_refusals_name_the_field_and_write_nothing(gpu, ptamd, pkg):
    L = pkg.layouts
    W, H = 16, 4
    dev = _torch().device("cuda", gpu.device_ordinal)
    op = ptamd.NRDComposition(gpu)
    host = hostile_textures(W, H, seed=9)
    dtex = upload(host, dev)
    nan = (3.0, float("nan"), 20.0, -25.0)
    cases = []
    for pack, names in ((1, ["LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NoisyDiffuse", "NoisySpecular"]),
                        (0, ["LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "DenoisedDiffuse", "DenoisedSpecular", "Radiance"])):
        for den in (L.DENOISER_NRD_RELAX, L.DENOISER_NRD_REBLUR, L.DENOISER_NONE):
            for name in names:
                cases.append((raw_constants(L, W, H, den, pack), name, name))
    cases.append((raw_constants(L, W, H, L.DENOISER_NRD_REBLUR, 1), "NormalRoughness", "NormalRoughness"))
    for pack in (0, 1):
        cases += [(raw_constants(L, W, H, 4, pack), None, "Denoiser"), (raw_constants(L, W, H, 0xFFFFFFFF, pack), None, "Denoiser"),
                  (raw_constants(L, 0, H, L.DENOISER_NRD_RELAX, pack), None, "RenderSize"), (raw_constants(L, W, 0, L.DENOISER_NRD_RELAX, pack), None, "RenderSize"),
                  (raw_constants(L, 16385, H, L.DENOISER_NRD_RELAX, pack), None, "RenderSize"),
                  (raw_constants(L, W, H, L.DENOISER_NRD_REBLUR, pack, nan), None, "ReBLURHitDistance"),
                  (raw_constants(L, W, H, L.DENOISER_NRD_RELAX, pack, (3.0, 0.1, float("inf"), -25.0)), None, "ReBLURHitDistance")]
    cases.append((raw_constants(L, W, H, L.DENOISER_NRD_RELAX, 2), None, "IsPack"))
    for k, missing, word in cases:
        bind = {n: t for n, t in dtex.items() if n != missing}
        with pytest.raises(ptamd.PtInvalidArgument, match=word):
            op.Process(bind, k)
    # a ReLAX pack does not read NormalRoughness: unbound is fine there (and the pass runs after the refusals)
    op.Process({n: t for n, t in dtex.items() if n not in ("NormalRoughness", "DenoisedDiffuse", "DenoisedSpecular", "Radiance")},
               L.nrd_composition_constants(W, H, L.DENOISER_NRD_RELAX, True))
    gpu.sync()
    after = download(dtex, host)
    for name in host:
        if name not in ("NoisyDiffuse", "NoisySpecular"):
            assert after[name].tobytes() == host[name].tobytes(), name
    want_d, want_s = R.pack(L.DENOISER_NRD_RELAX, host["LinearDepth"], host["DiffuseAlbedo"], host["SpecularAlbedo"], host["NormalRoughness"],
                            host["NoisyDiffuse"], host["NoisySpecular"])
    assert_same(after["NoisyDiffuse"], want_d, "first accepted call after the refusals")      # the refused calls wrote nothing
    assert_same(after["NoisySpecular"], want_s, "first accepted call after the refusals")


def test_a_texture_not_aligned_to_its_texel_is_refused(gpu, ptamd, pkg):
    """a view that starts 2 bytes into an allocation (LinearDepth: likewise, as bytes) is aligned to no texel: refused, nothing written"""
    L = pkg.layouts
    torch = _torch()
    W, H = 16, 4
    dev = torch.device("cuda", gpu.device_ordinal)
    op = ptamd.NRDComposition(gpu)
    host = hostile_textures(W, H, seed=11)
    for pack, names in ((1, ["LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "NormalRoughness", "NoisyDiffuse", "NoisySpecular"]),
                        (0, ["LinearDepth", "DiffuseAlbedo", "SpecularAlbedo", "DenoisedDiffuse", "DenoisedSpecular", "Radiance"])):
        for name in names:
            dtex = upload(host, dev)
            raw = dtex[name].reshape(-1).view(torch.int16)
            shifted = torch.zeros(raw.numel() + 1, dtype=torch.int16, device=dev)[1:]
            shifted.copy_(raw)
            assert shifted.data_ptr() % 4 == 2
            bind = dict(dtex, **{name: shifted})
            k = raw_constants(L, W, H, L.DENOISER_NRD_REBLUR, pack)
            assert ptamd.nrd_composition_pixels_per_lane({n: t.data_ptr() for n, t in bind.items()}, k) == 0
            with pytest.raises(ptamd.PtInvalidArgument, match="aligned"):
                op.Process(bind, k)
            gpu.sync()
            after = download(dtex, host)
            for n in host:
                assert after[n].tobytes() == host[n].tobytes(), (name, n)
            assert shifted.cpu().numpy().tobytes() == np.ascontiguousarray(host[name]).tobytes(), name


def test_refused_calls_leave_every_texture_as_it_was(gpu, ptamd, pkg):
    L = pkg.layouts
    W, H = 16, 4
    dev = _torch().device("cuda", gpu.device_ordinal)
    op = ptamd.NRDComposition(gpu)
    host = hostile_textures(W, H, seed=10)
    dtex = upload(host, dev)
    for k, missing in ((raw_constants(L, W, H, 4, 1), None), (raw_constants(L, W, H, 3, 2), None), (raw_constants(L, 0, H, 3, 1), None),
                       (raw_constants(L, W, H, 2, 0, (float("nan"), 0.1, 20.0, -25.0)), None), (raw_constants(L, W, H, 3, 1), "SpecularAlbedo"),
                       (raw_constants(L, W, H, 3, 0), "DenoisedSpecular")):
        with pytest.raises(ptamd.PtInvalidArgument):
            op.Process({n: t for n, t in dtex.items() if n != missing}, k)
    gpu.sync()
    after = download(dtex, host)
    for name in host:
        assert after[name].tobytes() == host[name].tobytes(), name


# ------------------------------------------------------------------------------------------------------------------------------------
# the round trip that closes row f4: Cornell "ggx", 48 x 32, 2 spp, 3 bounces, one FrameIndex; DI off and di_samples = 8
W4, H4, SPP4, BOUNCES4, FRAME4, DI4 = 48, 32, 2, 3, 0, 8
KEEP = ("Radiance", "Diffuse", "Specular", "DiffuseAlbedo", "SpecularAlbedo", "LinearDepth", "NormalRoughness")


def _settings(S, L, denoiser, di):
    gs = S.graphics_settings(W4, H4, spp=SPP4, bounces=BOUNCES4, frame_index=FRAME4)
    gs["Denoiser"] = denoiser
    gs["IsDIEnabled"] = 1 if di else 0
    return gs


@pytest.fixture(scope="module")
def frames(gpu, ptamd, pkg):
    """Per DI setting: frame A (Denoiser None), the un-packed NRD-mode frame ("pre": what the pack reads) and frames B (ReLAX, ReBLUR
    through render(..., nrd=...) with the identity denoiser). Rendered once, shared by the tests below, never modified."""
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    scene = S.cornell_box(aspect=W4 / H4, variant="ggx")
    g = ptamd.Scene(gpu, scene)
    out = {}
    for di in (False, True):
        def frame(denoiser, **kw):
            r = ptamd.Renderer(gpu, g, W4, H4, with_denoiser_outputs=True)
            r.render(_settings(S, L, denoiser, di), di_samples=DI4 if di else 0, **kw)
            gpu.sync()
            t = ptamd.textures_to_numpy(r.textures)
            return {k: t[k].copy() for k in KEEP}
        out[di] = {"A": frame(L.DENOISER_NONE), "pre": frame(L.DENOISER_NRD_RELAX),
                   L.DENOISER_NRD_RELAX: frame(L.DENOISER_NRD_RELAX, nrd=L.DENOISER_NRD_RELAX),
                   L.DENOISER_NRD_REBLUR: frame(L.DENOISER_NRD_REBLUR, nrd=L.DENOISER_NRD_REBLUR)}
    yield out
    g.close()


def h16(v):
    """half an fp16 ulp at |v| (float64), taken at the neighbour above so that a value just below a binade edge is covered: what one
    fp16 store can add to the value it rounds: relative 2^-11, or 2^-25 in the subnormal range"""
    return R.ulp16(np.abs(np.asarray(v, np.float64)) * (1 + 2.0 ** -10)) / 2


def round_trip_bound(denoiser, A, B, pre):
    """The derived bound on |B - A| per channel (float64, (H, W, 3)) -- see test_round_trip_through_the_identity_denoiser."""
    a, b = (R.f16_to_f32(t["Radiance"])[..., :3].astype(np.float64) for t in (A, B))
    bound = h16(a) + h16(b)                                                   # A's own store, the composed store
    slop = np.abs(a) + np.abs(b)
    for tex, alb in (("Diffuse", "DiffuseAlbedo"), ("Specular", "SpecularAlbedo")):
        x = R.f16_to_f32(pre[tex])[..., :3].astype(np.float64)               # the stored Diffuse / Specular
        al = R.f16_to_f32(pre[alb])[..., :3].astype(np.float64)
        with np.errstate(all="ignore"):
            c = x / al
        if denoiser == R.DENOISER_NRD_REBLUR:
            ycc = R.ycocg(c.astype(np.float32)).astype(np.float64)
            packed = h16(ycc).sum(-1, keepdims=True)                          # R = Y - Cg + Co, G = Y + Cg, B = Y - Cg - Co: at most all three
            slop = slop + 8 * np.abs(c).max(-1, keepdims=True) * al           # the fp32 sums of the transform and its inverse: <= 4 ulp32 of 2 max
        else:
            packed = h16(c)
        bound = bound + h16(x) + al * packed                                  # the store of Diffuse / Specular; the packed store, times the albedo
        slop = slop + np.abs(x)
    return bound + 16 * 2.0 ** -24 * slop                                     # every fp32 rounding of both routes: a handful, each <= 2^-24 relative


def round_trip_excluded(A, B, pre):
    """the pixels the round trip leaves out: an albedo channel is 0 while the noisy channel is not, or a radiance that is not finite"""
    a, b = (R.f16_to_f32(t["Radiance"])[..., :3] for t in (A, B))
    excluded = ~np.isfinite(a).all(-1) | ~np.isfinite(b).all(-1)
    for tex, alb in (("Diffuse", "DiffuseAlbedo"), ("Specular", "SpecularAlbedo")):
        excluded |= ((R.f16_to_f32(pre[alb])[..., :3] == 0) & (R.f16_to_f32(pre[tex])[..., :3] != 0)).any(-1)
    return excluded


@pytest.mark.parametrize("di", [False, True], ids=["di-off", "di-8"])
@pytest.mark.parametrize("denoiser", [3, 2], ids=["relax", "reblur"])
def test_round_trip_through_the_identity_denoiser(frames, pkg, di, denoiser):
    """Frame A renders with Denoiser None; frame B renders the same frame with an NRD value through render(..., nrd=...), i.e. G-buffer
    emission in Radiance, Diffuse / Specular packed, handed to the identity and composed back. Pixels the G-buffer missed must agree
    bit for bit. Excluded: pixels where an albedo channel is 0 while the noisy channel is not (the pack drops that energy) and pixels
    whose radiance is not finite -- at most 2 % of the hit pixels (on this scene: none; the G-buffer's albedos have a floor of 0.01:
    test_round_trip_exclusions_on_the_oracles_nrd_outputs counts them on the CPU from the oracle's NRD outputs). The box fills this
    frame, so there is no missed pixel here: that clause holds vacuously, and untouched pixels are the synthetic test's. Every other pixel: |B - A| per channel within the bound below, derived, not fitted.

    Route A stores f16(out [+ DI]) once. Route B stores Diffuse / Specular = f16(indirect [+ DI]) (x), then the pack stores
    f16(x / albedo) (c; for ReBLUR its Y, Co, Cg), then the compose stores f16(e + c_d albedo_d + c_s albedo_s), e being the G-buffer
    emission both routes start from (out - e, clamped at 0, is what Diffuse / Specular split). Each fp16 store adds at most half an
    fp16 ulp of the value it rounds, h(v) = 2^-11 |v| (2^-25 in the subnormal range):
        |B - A| <= h(A) + h(B) + sum over the two textures of [ h(x) + albedo * h(c) ]
    with h(c) replaced by h(Y) + h(Co) + h(Cg) for ReBLUR (each of r, g, b is a signed sum of at most those three), plus the fp32
    roundings of both routes (the subtraction of e, the division, the products and sums of the compose, the YCoCg sums), a handful of
    2^-24-relative terms bounded by 16 * 2^-24 of the magnitudes involved. h is evaluated at the stored values' upper neighbour."""
    L = pkg.layouts
    f = frames[di]
    A, B, pre = f["A"], f[denoiser], f["pre"]
    hit = np.isfinite(pre["LinearDepth"][..., 0])
    assert hit.any()                                  # (the box fills this frame: the untouched pixels are the synthetic test's)
    assert np.array_equal(A["LinearDepth"], B["LinearDepth"]) and np.array_equal(pre["DiffuseAlbedo"], B["DiffuseAlbedo"])
    assert_same(A["Radiance"][~hit], B["Radiance"][~hit], "pixels the G-buffer missed")
    # B is nrdref's pack and compose of the un-packed frame (rgb bit for bit): the operator ran on what the frame wrote
    want_d, want_s = R.pack(denoiser, pre["LinearDepth"][..., 0], pre["DiffuseAlbedo"], pre["SpecularAlbedo"], pre["NormalRoughness"],
                            pre["Diffuse"], pre["Specular"])
    assert_same(B["Diffuse"][..., :3], want_d[..., :3], "packed Diffuse")
    assert_same(B["Specular"][..., :3], want_s[..., :3], "packed Specular")
    assert_same(B["Radiance"], R.compose(denoiser, pre["LinearDepth"][..., 0], pre["DiffuseAlbedo"], pre["SpecularAlbedo"], B["Diffuse"],
                                         B["Specular"], pre["Radiance"]), "composed Radiance")
    a, b = (R.f16_to_f32(t["Radiance"])[..., :3].astype(np.float64) for t in (A, B))
    excluded = round_trip_excluded(A, B, pre) & hit
    assert excluded.sum() <= 0.02 * hit.sum(), (int(excluded.sum()), int(hit.sum()))
    check = hit & ~excluded
    bound = round_trip_bound(denoiser, A, B, pre)
    err = np.abs(b - a)
    ratio = float((err[check] / bound[check]).max())
    print(f"round trip denoiser={denoiser} di={di}: {int(check.sum())} pixels, {int(excluded.sum())} excluded, largest |B - A| / bound = {ratio:.3f}, "
          f"largest |B - A| = {float(err[check].max()):.3e}, pixels that differ: {int((err[check] > 0).any(-1).sum())}")
    assert (err[check] <= bound[check]).all(), ratio
    assert (a[check] > 0).any() and (R.f16_to_f32(pre["Diffuse"])[..., :3][check] > 0).any() and (R.f16_to_f32(pre["Specular"])[..., :3][check] > 0).any()


def test_render_refuses_nrd_without_its_inputs(gpu, ptamd, pkg):
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W4 / H4, variant="ggx"))
    try:
        r = ptamd.Renderer(gpu, g, W4, H4)                                      # no Diffuse / Specular
        with pytest.raises(ptamd.PtInvalidArgument, match="with_denoiser_outputs"):
            r.render(_settings(S, L, L.DENOISER_NRD_RELAX, False), nrd=L.DENOISER_NRD_RELAX)
        r = ptamd.Renderer(gpu, g, W4, H4, with_denoiser_outputs=True)
        with pytest.raises(ptamd.PtInvalidArgument, match="Denoiser"):           # the frame would not write the NRD outputs (nor the albedos)
            r.render(_settings(S, L, L.DENOISER_NONE, False), nrd=L.DENOISER_NRD_RELAX)
        with pytest.raises(ptamd.PtInvalidArgument, match="nrd"):
            r.render(_settings(S, L, L.DENOISER_DLSS_RR, False), nrd=L.DENOISER_DLSS_RR)
        with pytest.raises(ptamd.PtInvalidArgument, match="denoise"):
            r.render(_settings(S, L, L.DENOISER_NONE, False), denoise=lambda d, s: (d, s))
    finally:
        g.close()


def test_denoise_callback_sees_the_packed_pair_and_feeds_the_compose(gpu, ptamd, pkg, frames):
    """a denoiser that returns fresh tensors (copies): the same Radiance as the aliased identity"""
    S, L = pkg.scenes, pkg.layouts
    gpu.set_sharding(0, 1, 16)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W4 / H4, variant="ggx"))
    try:
        seen = {}

        def denoise(d, s):
            seen["d"], seen["s"] = d.cpu().numpy().view(np.uint16).copy(), s.cpu().numpy().view(np.uint16).copy()
            return d.clone(), s.clone()
        r = ptamd.Renderer(gpu, g, W4, H4, with_denoiser_outputs=True)
        r.render(_settings(S, L, L.DENOISER_NRD_REBLUR, True), di_samples=DI4, nrd=L.DENOISER_NRD_REBLUR, denoise=denoise)
        gpu.sync()
        want = frames[True][L.DENOISER_NRD_REBLUR]
        assert np.array_equal(seen["d"], want["Diffuse"]) and np.array_equal(seen["s"], want["Specular"])
        assert np.array_equal(ptamd.textures_to_numpy(r.textures)["Radiance"], want["Radiance"])
    finally:
        g.close()


@pytest.mark.parametrize("denoiser", [3, 2], ids=["relax", "reblur"])
def test_sharded_context_runs_the_pass_on_its_band(gpu, ptamd, pkg, frames, denoiser):
    """rank 0 of 2 with bands of 8 rows owns rows 0-7 and 16-23 of the 32: its frame through render(..., nrd=...) equals those rows of
    the unsharded frame B bit for bit, in Radiance and in the packed pair"""
    S, L = pkg.scenes, pkg.layouts
    rows = np.r_[0:8, 16:24]
    for rank in (0, 1):
        gpu.set_sharding(rank, 2, 8)
        try:
            g = ptamd.Scene(gpu, S.cornell_box(aspect=W4 / H4, variant="ggx"))
            r = ptamd.Renderer(gpu, g, W4, H4, with_denoiser_outputs=True)
            assert r.local_rows == 16
            r.render(_settings(S, L, denoiser, False), nrd=denoiser)
            gpu.sync()
            t = ptamd.textures_to_numpy(r.textures)
            g.close()
        finally:
            gpu.set_sharding(0, 1, 16)
        want = frames[False][denoiser]
        for k in ("Radiance", "Diffuse", "Specular"):
            assert_same(t[k], want[k][rows + 8 * rank], (k, rank))


@pytest.mark.parametrize("di", [False, True], ids=["di-off", "di-8"])
@pytest.mark.parametrize("name, denoiser", [("relax", 3), ("reblur", 2)])
def test_cpp_host_writes_the_same_radiance(tmp_path, frames, name, denoiser, di):
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    out = str(tmp_path / "radiance.bin")
    cmd = [DEMO, "--width", str(W4), "--height", str(H4), "--spp", str(SPP4), "--bounces", str(BOUNCES4), "--frames", "1", "--nrd", name,
           "--out-radiance", out] + (["--di", "--di-samples", str(DI4)] if di else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "identity" in p.stderr
    got = np.fromfile(out, np.uint16).reshape(H4, W4, 4)
    assert_same(got, frames[di][denoiser]["Radiance"], "pt_demo --nrd " + name)


def test_pixels_in_one_call(gpu, ptamd, pkg, frames):
    """render(..., nrd=RELAX, post=...) is post applied to the composed Radiance of the round-trip test, bit for bit"""
    S, L = pkg.scenes, pkg.layouts
    torch = _torch()
    gpu.set_sharding(0, 1, 16)
    post = L.post_processing_settings(W4, H4)
    g = ptamd.Scene(gpu, S.cornell_box(aspect=W4 / H4, variant="ggx"))
    try:
        r = ptamd.Renderer(gpu, g, W4, H4, with_denoiser_outputs=True)
        r.render(_settings(S, L, L.DENOISER_NRD_RELAX, True), di_samples=DI4, nrd=L.DENOISER_NRD_RELAX, post=post)
        gpu.sync()
        one = ptamd.textures_to_numpy(r.textures)
    finally:
        g.close()
    composed = frames[True][L.DENOISER_NRD_RELAX]["Radiance"]
    assert_same(one["Radiance"], composed, "Radiance")
    dev = torch.device("cuda", gpu.device_ordinal)
    tex = dict(ptamd.alloc_post_textures(W4, H4, dev), Radiance=torch.from_numpy(composed.view(np.int16).copy()).to(dev))
    op = ptamd.PostProcessing(gpu)
    op.SetConstants(post)
    op.Render(tex)
    gpu.sync()
    for k in ("Color", "BackBuffer", "Display8"):
        assert_same(one[k], tex[k].cpu().numpy().view(np.dtype(L.POST_FORMATS[k][0])).reshape(one[k].shape), k)
    assert one["Display8"][..., :3].max() > 0
