"""CPU tests of the ray-reconstruction pass's rules ("Ray reconstruction"): the Python mirrors of the structs against
include/ptamd.h (a gcc-compiled probe), the settings helper's refusals, tests/reconstructref.py against tests/upscaleref.py where the two
must agree, what the pass is for -- a noisy jittered sequence comes out closer to its truth than through the upscaler alone -- and the
C++ host's argument refusals. No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import reconstructref as R
import upscaleref as U

EPS32 = 2.0 ** -24                     # half an fp32 ulp, relative: what one rounded fp32 operation adds
DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
ENTRY_POINTS = ("pt_reconstruction_set_constants", "pt_reconstruction_process", "pt_reconstruction_reset_history",
                "pt_reconstruction_download_history")
# the noise test's sequence: fixed after looking at the figures of seeds 1-3 on the CPU (docstring of the test)
NOISE = {"render": (20, 12), "output": (40, 24), "frames": 16, "seed": 1, "sigma": 0.9, "contrast": 0.25}


def f64_of(bits):
    with np.errstate(invalid="ignore"):
        return R.f16_to_f32(bits).astype(np.float64)


def test_struct_layouts_match_a_compiled_probe(tmp_path, pkg, ptamd):
    """sizes and offsets of PtReconstructionSettings and PtReconstructionTextures as the host compiler lays them out, against
    layouts.RECONSTRUCTION_SETTINGS and ptamd.ReconstructionTextures; the two debug bits; the defaults the header states"""
    L = pkg.layouts
    fields = [n for n in L.RECONSTRUCTION_SETTINGS.names]
    tex = L.RECONSTRUCTION_TEXTURES
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "include/ptamd.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(struct PtReconstructionSettings), sizeof(struct PtReconstructionTextures));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(struct PtReconstructionSettings, {f}));\n' for f in fields)
                   + "".join(f'  printf("%zu\\n", offsetof(struct PtReconstructionTextures, {f}));\n' for f in tex)
                   + '  printf("%u %u %d\\n", PT_RECONSTRUCTION_FORM_DIRECT, PT_RECONSTRUCTION_FORM_STAGED, PTAMD_ABI_VERSION);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", ge.ROOT, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    size_s, size_t = (int(v) for v in out[0].split())
    assert size_s == L.RECONSTRUCTION_SETTINGS.itemsize == 64 and size_s % 16 == 0
    assert size_t == C.sizeof(ptamd.ReconstructionTextures) == 8 * C.sizeof(C.c_void_p) and len(tex) == 8
    offsets = [int(v) for v in out[1:1 + len(fields) + len(tex)]]
    assert offsets[:len(fields)] == [L.RECONSTRUCTION_SETTINGS.fields[f][1] for f in fields]
    assert offsets[len(fields):] == [getattr(ptamd.ReconstructionTextures, n).offset for n in tex]
    assert [f[0] for f in ptamd.ReconstructionTextures._fields_] == tex
    direct, staged, abi = (int(v) for v in out[1 + len(fields) + len(tex)].split())
    assert (direct, staged) == (0x8000, 0x10000) == (L.RECONSTRUCTION_FORM_DIRECT, L.RECONSTRUCTION_FORM_STAGED)
    assert abi == 4                                                 # new entry points only

    text = open(os.path.join(ge.ROOT, "include", "ptamd.h")).read()
    body = re.search(r"struct PtReconstructionSettings \{[^\n]*\n(.*?)\};\s*/\* 64 B \*/", text, re.S).group(1)
    decl = re.findall(r"^\s*(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?;(?:\s*/\*\s*default ([0-9.]+))?", body, re.M)
    assert [d[1] for d in decl] == fields
    for ctype, name, _, default in decl:
        assert L.RECONSTRUCTION_SETTINGS[name].base == np.dtype("<u4" if ctype == "uint32_t" else "<f4"), name
        if default:
            assert float(default) == L.RECONSTRUCTION_DEFAULTS[name] == R.DEFAULTS[name], name
    assert set(L.RECONSTRUCTION_DEFAULTS) == set(R.DEFAULTS) == set(fields) - {"RenderSize", "OutputSize", "_pad"}
    # the namesakes' defaults, LuminanceSigma 2
    assert {k: L.RECONSTRUCTION_DEFAULTS[k] for k in ("DepthThreshold", "NormalCosine", "RoughnessFraction", "MaxAccumulatedFrames", "AtrousIterations")} \
        == {k: L.DENOISER_DEFAULTS[k] for k in ("DepthThreshold", "NormalCosine", "RoughnessFraction", "MaxAccumulatedFrames", "AtrousIterations")}
    assert L.RECONSTRUCTION_DEFAULTS["KernelRadius"] == L.UPSCALER_DEFAULTS["KernelRadius"] and L.RECONSTRUCTION_DEFAULTS["LuminanceSigma"] == 2.0
    assert L.RECONSTRUCTION_DEFAULTS["MaxOutputFrames"] == L.UPSCALER_DEFAULTS["MaxAccumulatedFrames"] == 16
    bits = {n: int(v, 16) for n, v in re.findall(r"#define (PT_(?:DEBUG|DENOISER_FORM|UPSCALER_FORM|RECONSTRUCTION_FORM)_\w+)\s+(0x[0-9a-fA-F]+)u", text)}
    assert len(set(bits.values())) == len(bits) and all(v & (v - 1) == 0 for v in bits.values())       # one bit each, none shared
    for s in ENTRY_POINTS:
        assert s in ptamd.EXPORTS and re.search(r"\bint\s+%s\(" % s, text), s
    assert sorted(s for s in ptamd.EXPORTS if s.startswith("pt_reconstruction_")) == sorted(ENTRY_POINTS)
    assert sorted(set(re.findall(r"\b(pt_reconstruction_\w+)\(", text))) == sorted(ENTRY_POINTS)


def test_the_library_exports_every_entry_point(ptamd):
    lib = ptamd.load_library()
    assert lib.pt_abi_version() == 4
    for s in ENTRY_POINTS:
        assert hasattr(lib, s), s


def test_settings_helper_refuses_what_the_library_refuses(pkg):
    L = pkg.layouts
    s = L.reconstruction_settings((960, 540), (1920, 1080))
    assert (int(s["MaxAccumulatedFrames"]), int(s["MaxOutputFrames"]), int(s["AtrousIterations"])) == (30, 16, 5)
    assert float(s["LuminanceSigma"]) == 2.0 and tuple(s["OutputSize"]) == (1920, 1080) and not s["_pad"].any()
    assert L.reconstruction_settings((1, 4096), (4, 16384), MaxAccumulatedFrames=1, MaxOutputFrames=1, AtrousIterations=0, KernelRadius=0.75,
                                     DepthThreshold=1.0, NormalCosine=0.0) is not None
    assert L.reconstruction_settings((37, 19), (37, 19), MaxAccumulatedFrames=255, MaxOutputFrames=255, AtrousIterations=8, KernelRadius=2.0) is not None
    for word, kw in (("MaxAccumulatedFrames", {"MaxAccumulatedFrames": 0}), ("MaxAccumulatedFrames", {"MaxAccumulatedFrames": 256}),
                     ("MaxOutputFrames", {"MaxOutputFrames": 0}), ("MaxOutputFrames", {"MaxOutputFrames": 256}),
                     ("AtrousIterations", {"AtrousIterations": 9}),
                     ("KernelRadius", {"KernelRadius": 0.7}), ("KernelRadius", {"KernelRadius": 2.5}), ("KernelRadius", {"KernelRadius": float("nan")}),
                     ("DepthThreshold", {"DepthThreshold": 0.0}), ("DepthThreshold", {"DepthThreshold": 1.01}),
                     ("NormalCosine", {"NormalCosine": 1.0}), ("NormalCosine", {"NormalCosine": -0.1}),
                     ("LuminanceSigma", {"LuminanceSigma": 0.0}), ("LuminanceSigma", {"LuminanceSigma": float("inf")}),
                     ("RoughnessFraction", {"RoughnessFraction": -1.0}), ("RoughnessFraction", {"RoughnessFraction": float("nan")}),
                     ("no field", {"DiffuseLuminanceSigma": 0.5}), ("32-bit", {"MaxOutputFrames": -1})):
        with pytest.raises(ValueError, match=word):
            L.reconstruction_settings((32, 32), (64, 64), **kw)
    for word, render, output in (("RenderSize", (0, 8), (8, 8)), ("RenderSize", (16385, 8), (16385, 8)), ("OutputSize", (8, 8), (8, 0)),
                                 ("OutputSize", (8192, 8), (16385, 8)), ("4 RenderSize", (8, 8), (7, 8)), ("4 RenderSize", (8, 8), (8, 33)),
                                 ("32-bit", (-1, 8), (8, 8))):
        with pytest.raises(ValueError, match=word):
            L.reconstruction_settings(render, output)


@pytest.mark.parametrize("render,output", [((20, 12), (40, 24)), ((25, 13), (37, 19)), ((37, 19), (37, 19))], ids=["2x", "odd", "native"])
def test_without_a_filter_the_pass_is_the_upscaler_up_to_the_two_roundings_of_the_albedo(render, output):
    """AtrousIterations = 0, MaxAccumulatedFrames = 1 and one albedo everywhere, on three frames with seeded colours in [0, 4), a depth
    edge, a motion of 0.4 pixels and the Halton jitter. The frames' normals alternate between two perpendicular directions, so the
    render-size history is never valid and the signal is the demodulated input itself (with a valid tap, MaxAccumulatedFrames = 1 gives
    hist + (cur - hist), the input only up to a rounding: DESIGN.md). The resolve then sees c' = (c / A) A per channel where the upscaler
    sees c: one division and one product, |c' - c| <= (2 EPS32 + EPS32^2) |c|.

    In the tone-mapped space t = c / (1 + max3 c): the numerator moves by 2 EPS32, the denominator fl(1 + m) by 2 EPS32 and a rounding in
    each evaluation, the division rounds in each: |t' - t| <= 8 EPS32 |t|, |t| < 1. Everything behind it is a convex combination (the
    kernel-weighted mean, the blend) or a clamp into a box of such values: none amplifies a difference of its inputs, and the weights,
    the validity of every tap and n depend on geometry alone, so they are the same bits. What the two evaluations add is their own
    roundings, at most 34 each per frame (the count of tests/test_upscaler_rules.py), on values below 1. After frame f (from 0) the
    stored histories differ by at most (8 + 68 (f + 1)) EPS32, and n is equal. Color is the inverse map of that, (1 + m)^2 <= 25 times
    as far apart at most: under 6e-4 of a value whose fp16 spacing is at least 2^-11 of it wherever it matters, so the two fp16 results
    are equal or neighbours."""
    rng = np.random.default_rng(11)
    Rw, Rh = render
    xs = np.mgrid[0:Rh, 0:Rw][1]
    rr = R.Reconstruction(render, output, AtrousIterations=0, MaxAccumulatedFrames=1)
    up = U.Upscaler(render, output)
    albedo = ((0.5, 0.25, 0.75), (0.125, 0.0625, 0.03125))
    worst = 0.0
    for f in range(3):
        tex = R.plain_frame(render, rng.uniform(0.0, 4.0, (Rh, Rw, 3)), albedo=albedo, depth=np.where(xs >= Rw // 2, 7.0, 5.0),
                            motion=(0.4, 0.0, 0.0), normal=(0.0, 0.0, -1.0) if f % 2 == 0 else (1.0, 0.0, 0.0))
        j = R.jitter(f, render, output)
        a, b = rr.process(tex, j), up.process(R.upscaler_textures(tex), j)
        assert not rr.reused.any() and (rr.length == 1).all()
        assert np.array_equal(rr.filtered[..., :3] * rr.albedo, (R.f16_to_f32(tex["Radiance"])[..., :3] / rr.albedo) * rr.albedo)
        assert rr.n.tobytes() == up.length.tobytes()
        assert np.array_equal(rr.reused_out, up.reused) and (f == 0 or up.reused.any())
        d = np.abs(rr.out_hist["colour_n"][..., :3].astype(np.float64) - up.hist["colour_n"][..., :3].astype(np.float64))
        bound = (8 + 68 * (f + 1)) * EPS32
        worst = max(worst, float(d.max() / bound))
        assert (d <= bound).all(), (f, float(d.max()), bound)
        ca, cb = f64_of(a), f64_of(b)
        assert (np.abs(ca - cb) <= R.ulp16(np.maximum(np.abs(ca), np.abs(cb)))).all()
        assert (a[..., 3] == R.ONE16).all()
    print(f"{render}->{output}: largest |reconstructref - upscaleref| / bound in the stored history = {worst:.3f}")


def test_the_synthetic_sequence_is_hostile():
    """what the bit-for-bit test leans on: missed pixels, albedo sums under the floor, albedos that are not finite, both sides of the
    specular-dominance test under motion, a different jitter each frame"""
    for render, output in (((20, 12), (40, 24)), ((25, 13), (37, 19)), ((13, 7), (39, 21)), ((37, 19), (37, 19))):
        frames = R.synthetic_frames(render, output, seed=render[0] * 131 + output[0])
        assert len({(float(j[0]), float(j[1])) for _, j in frames}) == len(frames)
        for tex, _ in frames:
            n = render[0] * render[1]
            assert (~np.isfinite(tex["LinearDepth"])).sum() >= n // 10
            with np.errstate(invalid="ignore"):
                ad, sp = R.f16_to_f32(tex["DiffuseAlbedo"])[..., :3], R.f16_to_f32(tex["SpecularAlbedo"])[..., :3]
                total = ad + sp
                lum = lambda c: 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]
                assert (total < R.ALBEDO_FLOOR).any() and (total == 0).any() and (~np.isfinite(total)).any()
                assert (lum(sp) > lum(ad)).sum() > n // 5 and (lum(sp) < lum(ad)).sum() > n // 5
            assert (~np.isfinite(R.f16_to_f32(tex["Radiance"]))).any() and (tex["Radiance"] == R.f16(65504.0)).any()


def noise_figures():
    """RMS errors of the 16th frame of the noise sequence against its truth: (through reconstructref, through upscaleref alone, through
    upscaleref on the same sequence without noise)"""
    n = NOISE
    out = []
    for sigma in (n["sigma"], 0.0):
        seq, truth = R.noisy_sequence(n["render"], n["output"], n["frames"], n["seed"], sigma, n["contrast"])
        rr, up = R.Reconstruction(n["render"], n["output"]), U.Upscaler(n["render"], n["output"])
        for tex, j in seq:
            a, b = rr.process(tex, j), up.process(R.upscaler_textures(tex), j)
        rms = lambda c: float(np.sqrt(((f64_of(c)[..., :3] - truth) ** 2).mean()))
        out += [rms(a), rms(b)]
        if sigma:
            assert rr.length.min() >= 8 and rr.n.max() > 4          # both histories were in use
    return out[0], out[1], out[3]


def test_a_noisy_sequence_comes_out_closer_to_the_truth_than_through_the_upscaler_alone():
    """reconstructref.noisy_sequence: 20 x 12 -> 40 x 24, 16 frames under the Halton jitter; two planes with a depth and a normal edge
    between them, one lighting value a plane, a checker albedo whose cells are the output pixels (the dark cells 0.75 of the bright
    ones), and the lighting of every sample multiplied by 1 + 0.9 u, u uniform in [-1, 1). The inequality only; the figures are
    recorded in DESIGN.md section 1, "Ray reconstruction": 0.137 through the pass against 0.193 through the upscaler alone, whose
    noise-free residual on this checker is 0.136 (at 2x every sample of a frame sees the same checker colour: the residual is the
    checker's, and both passes have it). Seeds 2 and 3 give 0.134 / 0.191 and 0.143 / 0.194; seed 1 it is."""
    reconstructed, upscaled, residual = noise_figures()
    print(f"RMS error of frame 16 against the truth: reconstructed {reconstructed:.4f}, upscaler alone {upscaled:.4f} "
          f"(ratio {reconstructed / upscaled:.3f}); the upscaler alone without noise {residual:.4f}")
    assert upscaled > 1.25 * residual                                # the noise is what the upscaler's figure measures
    assert reconstructed < upscaled


# ------------------------------------------------------------------------------------------------------------------------------------
# the C++ host parses its arguments before it opens a device
def _demo(*args):
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    return subprocess.run([DEMO, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,word", [
    (("--reconstruct", "performance", "--output-size", "48x32", "--upscale", "performance"), "--upscale"),
    (("--reconstruct", "performance", "--output-size", "48x32", "--nrd", "relax"), "--nrd"),
    (("--reconstruct", "sharpest", "--output-size", "48x32"), "--reconstruct"),
    (("--reconstruct", "performance"), "--output-size"),
    (("--reconstruct-iterations", "3"), "--reconstruct"),
    (("--reconstruct", "performance", "--output-size", "48x32", "--reconstruct-iterations", "9"), "--reconstruct-iterations"),
    (("--out-reconstructed", "r.bin"), "--reconstruct"),
], ids=["upscale", "nrd", "mode", "no-size", "iterations-alone", "iterations-range", "out-alone"])
def test_cpp_host_refuses_argument_combinations_by_name(args, word):
    p = _demo(*args)
    assert p.returncode != 0 and word in p.stderr, (p.returncode, p.stderr)
