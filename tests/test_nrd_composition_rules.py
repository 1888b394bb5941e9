"""CPU tests of the NRD composition boundary (pt_nrd_composition_process): the struct layouts of include/ptamd.h against the numpy /
ctypes mirrors (a gcc-compiled probe), the hit-distance defaults, the checks of the layouts helper, and self-checks of tests/nrdref.py,
the numpy restatement of DESIGN.md section 1, "NRD composition", that the GPU tests hold the kernel against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import nrdref as R

NEW = ["pt_nrd_composition_process", "pt_nrd_reblur_hit_distance_defaults"]


def test_entry_points_are_declared_exported_and_bound(ptamd):
    header = open(os.path.join(ge.ROOT, "include", "ptamd.h")).read()
    lib = ptamd.load_library()
    assert "int  pt_nrd_composition_process(" in header and "void pt_nrd_reblur_hit_distance_defaults(" in header
    for name in NEW:
        assert hasattr(lib, name) and name in ptamd.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert "#define PTAMD_ABI_VERSION 4" in header and lib.pt_abi_version() == 4          # new entry points only


def test_struct_layouts_match_a_compiled_probe(tmp_path, pkg, ptamd):
    L = pkg.layouts
    fields = ["RenderSize", "IsPack", "Denoiser", "ReBLURHitDistance"]
    tex = L.NRD_COMPOSITION_TEXTURES
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "include/ptamd.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(struct PtNRDCompositionConstants), sizeof(struct PtNRDCompositionTextures));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(struct PtNRDCompositionConstants, {f}));\n' for f in fields)
                   + "".join(f'  printf("%zu\\n", offsetof(struct PtNRDCompositionTextures, {f}));\n' for f in tex)
                   + '  printf("%d %d %d %d\\n", PT_DENOISER_NONE, PT_DENOISER_DLSS_RAY_RECONSTRUCTION, PT_DENOISER_NRD_REBLUR,'
                     ' PT_DENOISER_NRD_RELAX);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", ge.ROOT, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    size_k, size_t = (int(v) for v in out[0].split())
    assert size_k == L.NRD_COMPOSITION_CONSTANTS.itemsize == 32
    assert size_t == C.sizeof(ptamd.NRDCompositionTextures) == 9 * C.sizeof(C.c_void_p) and len(tex) == 9
    assert [int(v) for v in out[1:1 + len(fields)]] == [L.NRD_COMPOSITION_CONSTANTS.fields[f][1] for f in fields] == [0, 8, 12, 16]
    assert [int(v) for v in out[1 + len(fields):1 + len(fields) + 9]] == [getattr(ptamd.NRDCompositionTextures, f).offset for f in tex]
    assert [int(v) for v in out[1 + len(fields) + 9].split()] == [L.DENOISER_NONE, L.DENOISER_DLSS_RR, L.DENOISER_NRD_REBLUR,
                                                                   L.DENOISER_NRD_RELAX]
    assert (R.DENOISER_NONE, R.DENOISER_DLSS_RR, R.DENOISER_NRD_REBLUR, R.DENOISER_NRD_RELAX) == (0, 1, 2, 3)


def test_hit_distance_defaults(pkg, ptamd):
    got = ptamd.nrd_reblur_hit_distance_defaults()
    assert got.dtype == np.float32 and got.tolist() == [np.float32(v) for v in (3.0, 0.1, 20.0, -25.0)]
    assert tuple(pkg.layouts.NRD_REBLUR_HIT_DISTANCE_DEFAULTS) == R.REBLUR_HIT_DISTANCE_DEFAULTS == (3.0, 0.1, 20.0, -25.0)
    k = pkg.layouts.nrd_composition_constants(48, 32, pkg.layouts.DENOISER_NRD_REBLUR, True)
    assert np.array_equal(k["ReBLURHitDistance"], got) and k["RenderSize"].tolist() == [48, 32] and int(k["IsPack"]) == 1
    k = pkg.layouts.nrd_composition_constants(1, 16384, pkg.layouts.DENOISER_NRD_RELAX, False, (1, 2, 3, 4))
    assert k["ReBLURHitDistance"].tolist() == [1, 2, 3, 4] and int(k["IsPack"]) == 0 and int(k["Denoiser"]) == 3


@pytest.mark.parametrize("kwargs, word", [
    (dict(width=0), "RenderSize"), (dict(height=0), "RenderSize"), (dict(width=16385), "RenderSize"), (dict(height=16385), "RenderSize"),
    (dict(denoiser=4), "Denoiser"), (dict(is_pack=2), "IsPack"), (dict(hit_distance=(3.0, float("nan"), 20.0, -25.0)), "ReBLURHitDistance"),
    (dict(hit_distance=(float("inf"), 0.1, 20.0, -25.0)), "ReBLURHitDistance"), (dict(width=-1), "RenderSize"), (dict(denoiser=1 << 32), "Denoiser"),
])
def test_layouts_helper_refuses_what_the_library_refuses(pkg, kwargs, word):
    args = dict(width=8, height=8, denoiser=pkg.layouts.DENOISER_NRD_RELAX, is_pack=1)
    args.update(kwargs)
    with pytest.raises(ValueError, match=word):
        pkg.layouts.nrd_composition_constants(**args)


def ulp32(x):
    """spacing of the (normal) fp32 grid at |x|, float64"""
    return 2.0 ** (np.floor(np.log2(np.abs(np.asarray(x, np.float64)))) - 23)


def test_reblur_pack_unpack_returns_the_colour_within_2_ulp():
    """ReBLUR's YCoCg pack followed by the back-end unpack, on finite non-negative fp32 colours and without the fp16 store: every
    channel comes back within 2 ulp, the ulp being U = ulp(M) of the pixel's largest channel M = max(r, g, b). (A small channel cannot
    be held to its own ulp: red comes back as (Y - Cg) + Co, and the roundings of Y and Cg are of the size of ulp(g).)

    What the docstring can derive, and where it stops. The products by 0.25 and 0.5 are exact, so only the seven sums round, each by
    at most half an ulp of its own result. The results and their sizes: p = r/4 + g/2 <= 3M/4 (<= U/2; U/4 when p is below M's
    binade) and Y = p + b/4 <= M (<= U/2); q = g/2 - r/4, Cg = q - b/4 and Co = r/2 - b/2 lie in [-M/2, M/2], a binade below M
    (<= U/4 each); t = Y - Cg = (r + b)/2 <= M (<= U/2); the final sum is a channel <= M (<= U/2).
      green = Y + Cg collects p, Y, q, Cg and the final sum: 1/2 + 1/2 + 1/4 + 1/4 + 1/2 = 2 U. Derived.
      red, blue = t +- Co collect p, Y, q, Cg, t, Co and the final sum: 2.75 U when every term is taken at its own maximum.
    The seven maxima of red and blue exclude each other: t, the final sum and Co at their maxima need (r + b)/2 and r in M's binade and
    |r - b| >= M's binade floor, hence r >= 1.5 and b < 1 in units of that floor; Cg at its maximum then needs g < 0.5, which puts
    p = r/4 + g/2 below the binade and halves its term; and where t is small, Y - Cg subtracts neighbours and is exact. A case split
    over the binades of all seven results that closes the gap from 2.75 U to 2 U is not written down here: for red and blue the 2 ulp
    of the issue are asserted, not derived. They are asserted on 200 000 random colours over fp16's range plus the stress rows below
    (all channels at the top of a binade, greys, one channel dominant, pairs one binade apart); the observed maximum, printed, is
    2.000 U (a search over 8e7 colours with one channel in [1, 2) and the others up to three binades below found nothing above it). max(., 0) only moves a negative result towards the true value >= 0."""
    rng = np.random.default_rng(20260)
    n = 200000
    c = np.exp2(rng.uniform(-20, 15.99, (n, 3))).astype(np.float32)                     # up to fp16's range, the pass's own
    c[rng.random((n, 3)) < 0.1] = 0
    c[:1000] = np.float32(65504.0) * (1 - rng.integers(0, 4, (1000, 3)).astype(np.float32) * np.float32(2.0 ** -24))  # all channels at the top of a binade
    c[1000:2000, 1:] = c[1000:2000, :1]                                                 # grey
    c[2000:3000] = np.float32(1.0) + rng.integers(0, 1 << 23, (1000, 3)).astype(np.float32) * np.float32(2.0 ** -23)   # all three in one binade
    c[3000:4000, 0] = np.float32(1.5) + rng.integers(0, 1 << 22, 1000).astype(np.float32) * np.float32(2.0 ** -23)     # r >= 1.5, b < 1, g small:
    c[3000:4000, 2] = np.float32(0.5) + rng.integers(0, 1 << 22, 1000).astype(np.float32) * np.float32(2.0 ** -24)     # the corner of the docstring
    c[3000:4000, 1] = rng.uniform(0, 0.5, 1000).astype(np.float32)
    c[4000:5000, 1] = np.minimum(c[4000:5000, 1] * np.float32(1024.0), np.float32(65504.0))   # green dominant
    c = c[c.max(-1) > 0]
    back = R.ycocg_to_rgb(R.ycocg(c))
    assert back.dtype == np.float32
    U = ulp32(c.max(-1, keepdims=True))
    err = np.abs(back.astype(np.float64) - c.astype(np.float64))
    print("ReBLUR pack -> unpack: max error %.3f ulp of the largest channel (green %.3f)" % (float((err / U).max()), float((err / U)[:, 1].max())))
    assert np.all(err <= 2 * U)
    # and through the whole of the pack: sanitize changes nothing on such colours
    v, _ = R.pack_values(R.DENOISER_NRD_REBLUR, c, np.ones(len(c), np.float32), np.ones(len(c), np.float32), R.REBLUR_HIT_DISTANCE_DEFAULTS,
                         np.ones(len(c), np.float32))
    assert np.array_equal(v, R.ycocg(c))


def test_sanitize_zeroes_the_whole_vector():
    for bad in (np.nan, np.inf, -np.inf):
        for ch in range(3):
            v = np.array([1.0, 2.0, 3.0], np.float32)
            v[ch] = bad
            assert np.array_equal(R.sanitize(v), np.zeros(3, np.float32))
    assert np.array_equal(R.sanitize(np.array([-1.0, 70000.0, 0.5], np.float32)), np.array([0.0, 65504.0, 0.5], np.float32))
    assert not np.signbit(R.sanitize(np.array([-0.0, 0.0, 1.0], np.float32))).any()
    for den in (R.DENOISER_NRD_REBLUR, R.DENOISER_NRD_RELAX):
        c, _ = R.pack_values(den, np.array([[1.0, np.nan, 3.0]], np.float32), np.ones(1, np.float32), np.ones(1, np.float32),
                             R.REBLUR_HIT_DISTANCE_DEFAULTS, np.ones(1, np.float32))
        assert np.array_equal(c, np.zeros((1, 3), np.float32))


def _pack_alpha(den, a, z=1.0, r=0.5):
    f = lambda v: np.full(1, v, np.float32)
    _, out = R.pack_values(den, np.ones((1, 3), np.float32), f(a), f(z), R.REBLUR_HIT_DISTANCE_DEFAULTS, f(r))
    return R.f32_to_f16(out)[0]


def test_hit_distance_edges():
    one, zero = R.f32_to_f16(np.float32(1.0)), R.f32_to_f16(np.float32(0.0))
    assert _pack_alpha(R.DENOISER_NRD_RELAX, np.inf) == zero and _pack_alpha(R.DENOISER_NRD_REBLUR, np.inf) == one
    assert _pack_alpha(R.DENOISER_NRD_RELAX, np.nan) == zero and _pack_alpha(R.DENOISER_NRD_REBLUR, np.nan) == zero
    assert _pack_alpha(R.DENOISER_NRD_RELAX, -np.inf) == zero and _pack_alpha(R.DENOISER_NRD_REBLUR, -np.inf) == zero
    tiny = R.f32_to_f16(np.float32(1e-7))                       # 2 * 2^-24: the fp16 neighbour of 1e-7, not 0
    assert tiny == 2
    for den in (R.DENOISER_NRD_RELAX, R.DENOISER_NRD_REBLUR):
        assert _pack_alpha(den, 1e-9) == tiny
        assert _pack_alpha(den, 0.0) == zero and _pack_alpha(den, -0.0) == zero and _pack_alpha(den, -3.0) == zero
    assert _pack_alpha(R.DENOISER_NRD_RELAX, 70000.0) == R.f32_to_f16(np.float32(65504.0))
    # ReBLUR at roughness 1, depth 1: f = (3 + 0.1) * (1 + 2^-25 * 19), a = f / 2 -> 0.5
    f = np.float32(np.float32(3.0) + np.float32(0.1)) * (np.float32(1) + np.float32(2.0 ** -25) * np.float32(19))
    assert _pack_alpha(R.DENOISER_NRD_REBLUR, np.float32(f) / np.float32(2), z=-1.0, r=1.0) == R.f32_to_f16(np.float32(0.5))


def test_store_rounds_to_nearest_even_and_canonicalises_nan():
    assert R.f32_to_f16(np.float32(np.nan)) == 0x7E00 and R.f32_to_f16(-np.float32(np.nan)) == 0x7E00
    assert R.f32_to_f16(np.float32(65520.0)) == 0x7C00 and R.f32_to_f16(np.float32(65519.0)) == 0x7BFF
    assert R.f32_to_f16(np.float32(1.0 + 2.0 ** -11)) == 0x3C00 and R.f32_to_f16(np.float32(1.0 + 3 * 2.0 ** -11)) == 0x3C02


def test_untouched_pixels_and_alpha():
    rng = np.random.default_rng(3)
    n = 64
    tex = lambda: rng.integers(0, 0x7C00, (n, 4)).astype(np.uint16)
    depth = rng.uniform(0.1, 10, n).astype(np.float32)
    depth[::3] = np.inf; depth[1::7] = np.nan
    da, sa, nd, ns, rad = tex(), tex(), tex(), tex(), tex()
    nr = rng.integers(-32768, 32768, (n, 4)).astype(np.int16)
    dead = ~np.isfinite(depth)
    for den in range(4):
        d, s = R.pack(den, depth, da, sa, nr, nd, ns)
        assert np.array_equal(d[dead], nd[dead]) and np.array_equal(s[dead], ns[dead])
        if den < 2:
            assert np.array_equal(d[..., 3], nd[..., 3]) and np.array_equal(s[..., 3], ns[..., 3])
        out = R.compose(den, depth, da, sa, d, s, rad)
        assert np.array_equal(out[dead], rad[dead]) and np.array_equal(out[..., 3], rad[..., 3])
    assert not np.array_equal(R.pack(2, depth, da, sa, nr, nd, ns)[0], R.pack(3, depth, da, sa, nr, nd, ns)[0])


def test_pixels_per_lane_follows_the_alignment_of_the_textures(pkg, ptamd):
    """pt_nrd_composition_pixels_per_lane is the decision pt_nrd_composition_process takes (one function in the library): two pixels per
    lane when every texture the call touches is aligned to two texels, one when one of them is aligned to its texel only, refused (0)
    below that. Textures the call does not touch do not count."""
    L = pkg.layouts
    base = {n: 0x7F0000000000 + 0x100000 * i for i, n in enumerate(L.NRD_COMPOSITION_TEXTURES)}
    form = lambda ptrs, den, pack: ptamd.nrd_composition_pixels_per_lane(ptrs, L.nrd_composition_constants(37, 23, den, pack))
    for den in (L.DENOISER_NONE, L.DENOISER_NRD_REBLUR, L.DENOISER_NRD_RELAX):
        for pack in (True, False):
            assert form(base, den, pack) == 2
            touched = ["LinearDepth", "DiffuseAlbedo", "SpecularAlbedo"] + (["NoisyDiffuse", "NoisySpecular"] if pack else
                                                                          ["DenoisedDiffuse", "DenoisedSpecular", "Radiance"])
            if pack and den == L.DENOISER_NRD_REBLUR:
                touched.append("NormalRoughness")
            for name in L.NRD_COMPOSITION_TEXTURES:
                texel = 4 if name == "LinearDepth" else 8
                assert form(dict(base, **{name: base[name] + texel}), den, pack) == (1 if name in touched else 2), (name, den, pack)
                assert form(dict(base, **{name: base[name] + 2 * texel}), den, pack) == 2
                assert form(dict(base, **{name: base[name] + 2}), den, pack) == (0 if name in touched else 2), (name, den, pack)
                assert form({k: v for k, v in base.items() if k != name}, den, pack) == (0 if name in touched else 2)
    raw = np.zeros((), L.NRD_COMPOSITION_CONSTANTS)                    # RenderSize 0: refused
    assert ptamd.nrd_composition_pixels_per_lane(base, raw) == 0


@pytest.mark.parametrize("bad", [None, 0, np.zeros((), np.dtype([("RenderSize", "<u4", 2)])), np.zeros(2, np.uint32)], ids=["none", "int", "other-record", "array"])
def test_constants_of_another_type_are_refused_before_the_library_reads_them(pkg, ptamd, bad):
    with pytest.raises(ptamd.PtInvalidArgument, match="PtNRDCompositionConstants"):
        ptamd.nrd_composition_pixels_per_lane({}, bad)
    with pytest.raises(ptamd.PtInvalidArgument, match="PtNRDCompositionConstants"):
        ptamd.NRDComposition(None).Process({}, bad)
    two = np.zeros(2, pkg.layouts.NRD_COMPOSITION_CONSTANTS)
    with pytest.raises(ptamd.PtInvalidArgument, match="one PtNRDCompositionConstants"):
        ptamd.NRDComposition(None).Process({}, two)


def test_round_trip_exclusions_on_the_oracles_nrd_outputs(oracle, pkg):
    """The round trip of tests/test_nrd_composition_gpu.py excludes pixels where an albedo channel is 0 while the noisy channel is not
    (the pack drops that energy) and pixels whose radiance is not finite, at most 2 % of the hit pixels. Here the count is taken on the
    CPU, from the oracle's NRD-mode outputs of the same frame (Cornell "ggx", 48 x 32, 2 spp, 3 bounces, DI off): none is excluded --
    the G-buffer's albedos have a floor of 0.01 --, every pixel is a hit (the box fills the frame), and nrdref's pack and compose of that
    frame stay within the round trip's derived bound of the oracle's Denoiser = None frame."""
    import test_nrd_composition_gpu as T
    S, L = pkg.scenes, pkg.layouts
    scene = S.cornell_box(aspect=T.W4 / T.H4, variant="ggx")

    def frame(den):
        gs = S.graphics_settings(T.W4, T.H4, spp=T.SPP4, bounces=T.BOUNCES4, frame_index=T.FRAME4)
        gs["Denoiser"] = den
        return oracle.render(scene, gs, gbuffer_flags=0xFFFFFFFF if den else 0xFFFFFFFF & ~0xC0, layouts=L)[0]
    A, pre = frame(L.DENOISER_NONE), frame(L.DENOISER_NRD_RELAX)
    depth = pre["LinearDepth"][..., 0]
    hit = np.isfinite(depth)
    assert hit.all() and np.array_equal(A["LinearDepth"], pre["LinearDepth"])
    for alb in ("DiffuseAlbedo", "SpecularAlbedo"):
        assert R.f16_to_f32(pre[alb])[..., :3][hit].min() >= 0.0099
    for den in (L.DENOISER_NRD_RELAX, L.DENOISER_NRD_REBLUR):
        d, s = R.pack(den, depth, pre["DiffuseAlbedo"], pre["SpecularAlbedo"], pre["NormalRoughness"], pre["Diffuse"], pre["Specular"])
        B = dict(pre, Diffuse=d, Specular=s, Radiance=R.compose(den, depth, pre["DiffuseAlbedo"], pre["SpecularAlbedo"], d, s, pre["Radiance"]))
        excluded = T.round_trip_excluded(A, B, pre) & hit
        a, b = (R.f16_to_f32(t["Radiance"])[..., :3].astype(np.float64) for t in (A, B))
        check = hit & ~excluded
        ratio = float((np.abs(b - a)[check] / T.round_trip_bound(den, A, B, pre)[check]).max())
        print(f"oracle frame, denoiser {den}: {int(hit.sum())} hit pixels, {int(excluded.sum())} excluded, largest |B - A| / bound = {ratio:.3f}")
        assert excluded.sum() == 0 and ratio <= 1.0
