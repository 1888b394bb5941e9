"""Texture sampling, material evaluation and environment lookup against the float64 reference in texref.py.

The oracle and the HIP code were written by the same hand, so GPU == oracle parity cannot see a mistake both share.
These tests pin both to an independent float64 restatement of the reference's HLSL and the D3D sampling rules:
the oracle's exported samplers directly, oracle renders of closed-form scenes (CPU tier), the same scenes and
visibility rays on the GPU (-m gpu). Mutation tests show the tolerances are tight enough to catch each of a list of
plausible mistakes.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import __graft_entry__ as ge

_spec = importlib.util.spec_from_file_location("texref", os.path.join(os.path.dirname(__file__), "texref.py"))
texref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(texref)

REF = texref.Reference()
FMTS = (texref.FMT_RGBA8, texref.FMT_RGBA8_SRGB, texref.FMT_RGBA32F)
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17), (64, 64)]          # (W, H)


def make_texels(W, H, fmt, seed, faces=None):
    rng = np.random.default_rng(seed)
    shape = ((faces,) if faces else ()) + (H, W, 4)
    if fmt == texref.FMT_RGBA32F:
        return (rng.random(shape) * 4.0).astype(np.float32)               # values above 1
    return rng.integers(0, 256, shape).astype(np.uint8)


def heap_entry(oracle, data, W, H, fmt, cube=False):
    e = oracle.HeapEntry()
    e.Ptr, e.Bytes, e.Stride, e.Kind = data.ctypes.data, W | (H << 32), fmt, 2 if cube else 1
    return e


def oracle_sample2d(oracle, e, u, v):
    L = oracle.lib()
    out = np.zeros((len(u), 4), np.float32); o4 = (C.c_float * 4)()
    for i in range(len(u)):
        L.or_texture_sample(C.byref(e), C.c_float(u[i]), C.c_float(v[i]), o4)
        out[i] = o4[:]
    return out


def oracle_sample_cube(oracle, e, d):
    L = oracle.lib()
    d = np.ascontiguousarray(d, np.float32)
    out = np.zeros((len(d), 4), np.float32); o4 = (C.c_float * 4)()
    fp = C.POINTER(C.c_float)
    for i in range(len(d)):
        L.or_cube_sample(C.byref(e), d[i].ctypes.data_as(fp), o4)
        out[i] = o4[:]
    return out


def uv_classes(W, H, rng, n):
    """Per class: float32 (u, v). Texel centres, texel edges, integers, -2^-12, [-5, 0), [1, 40), near 1000 (fp16 steps),
    NaN / inf."""
    def grid(off):
        i = rng.integers(0, W, n); j = rng.integers(0, H, n)
        return ((i + off) / W).astype(np.float32), ((j + off) / H).astype(np.float32)
    k = rng.integers(-6, 7, (2, n)).astype(np.float32)
    near1000 = (np.float16(1000.0) + rng.integers(-8, 9, (2, n)) * 0.5).astype(np.float16).astype(np.float32)
    nan = np.array([np.nan, np.inf, -np.inf, 0.25], np.float32)[rng.integers(0, 4, (2, n))]
    return {
        "centre": grid(0.5), "edge": grid(0.0), "integer": (k[0], k[1]),
        "minus_2^-12": (np.full(n, -2.0 ** -12, np.float32), np.full(n, -2.0 ** -12, np.float32)),
        "negative": tuple(rng.uniform(-5, 0, (2, n)).astype(np.float32)),
        "wraps": tuple(rng.uniform(1, 40, (2, n)).astype(np.float32)),
        "near1000": (near1000[0] + rng.random(n).astype(np.float32) * 0.5, near1000[1]),
        "nan_inf": (nan[0], nan[1]),
    }


# ---------------------------------------------------------------------- sampler checks (return a list of failures)
def check_sample2d(ref, oracle, W, H, fmt, n=500, seed=0):
    rng = np.random.default_rng(seed + 17 * W + H + 1000 * fmt)
    data = make_texels(W, H, fmt, seed + W * 131 + H + fmt)
    e = heap_entry(oracle, data, W, H, fmt)
    tex = ref.decode(data, fmt)
    true_tex = REF.decode(data, fmt)
    fails = []
    for cls, (u, v) in uv_classes(W, H, rng, n).items():
        got = oracle_sample2d(oracle, e, u, v).astype(np.float64)
        want = ref.sample2d(tex, u, v)
        diff, mag = REF.footprint2d(true_tex, u, v)
        mag_uv = np.maximum(np.abs(np.where(np.isfinite(u), u, 0)), np.abs(np.where(np.isfinite(v), v, 0)))
        tol = texref.value_tolerance(texref.texel_position_error(max(W, H), mag_uv), diff, mag)[:, None]
        bad = np.abs(got - want) > tol
        if bad.any():
            i = np.argwhere(bad.any(1))[0, 0]
            fails.append(f"{W}x{H} fmt {fmt} {cls}: {int(bad.any(1).sum())}/{n} off, e.g. uv=({u[i]!r},{v[i]!r}) got {got[i]} want {want[i]}")
        if cls == "centre":
            # fp32 coordinates that land exactly on the centre must return the texel exactly
            exact = (u.astype(np.float64) * W - 0.5 == np.floor(u.astype(np.float64) * W)) & \
                    (v.astype(np.float64) * H - 0.5 == np.floor(v.astype(np.float64) * H))
            if exact.any() and not np.array_equal(got[exact], want[exact].astype(np.float32).astype(np.float64)):
                fails.append(f"{W}x{H} fmt {fmt}: a texel centre does not return its texel exactly")
    return fails


def cube_dirs(N, rng, n):
    """Face centres, points within half a texel of every face edge, points near all eight corners (no exact ties)."""
    out = []
    for f, (ma, ms, (sa, ss), (ta, ts)) in enumerate(texref.Reference.CUBE):
        def mk(S, T):
            d = np.zeros((len(S), 3)); d[:, ma] = ms; d[:, sa] = ss * S; d[:, ta] = ts * T
            return d
        c = rng.integers(0, N, (2, n // 8)); out.append(mk((2 * c[0] + 1) / N - 1, (2 * c[1] + 1) / N - 1))
        near = 1 - rng.random(n // 4) * (1.0 / N) * 0.999 - 1e-6            # within half a texel of the edge (texel = 2/N)
        along = rng.uniform(-0.999, 0.999, n // 4)
        sgn = rng.choice([-1.0, 1.0], n // 4)
        out.append(mk(sgn * near, along)); out.append(mk(along, sgn * near))
        cs = rng.choice([-1.0, 1.0], (2, n // 8))
        out.append(mk(cs[0] * (1 - rng.random(n // 8) / N * 0.999 - 1e-6), cs[1] * (1 - rng.random(n // 8) / N * 0.999 - 1e-6)))
    d = np.concatenate(out).astype(np.float32)
    a = np.abs(d.astype(np.float64))
    ties = (a[:, 0] == a[:, 1]) | (a[:, 0] == a[:, 2]) | (a[:, 1] == a[:, 2])
    return d[~ties]


def check_cube(ref, oracle, N, fmt, n=400, seed=0, count=None):
    rng = np.random.default_rng(seed + N + 10 * fmt)
    data = make_texels(N, N, fmt, seed + 7 * N + fmt, faces=6)
    e = heap_entry(oracle, data, N, N, fmt, cube=True)
    d = cube_dirs(N, rng, n)
    got = oracle_sample_cube(oracle, e, d).astype(np.float64)
    want = ref.sample_cube(ref.decode(data, fmt), d)
    diff, mag = REF.cube_footprint(REF.decode(data, fmt), d)
    tol = texref.value_tolerance(texref.texel_position_error(N, 1.0), diff, mag)[:, None]
    bad = (np.abs(got - want) > tol).any(1)
    if count is not None:
        count["samples"] = count.get("samples", 0) + len(d); count["off"] = count.get("off", 0) + int(bad.sum())
    if bad.any():
        i = np.argmax(bad)
        return [f"cube N={N} fmt {fmt}: {int(bad.sum())}/{len(d)} off, e.g. d={d[i]} got {got[i]} want {want[i]}"]
    return []


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("fmt", FMTS)
def test_oracle_texture_sample_matches_float64(W, H, fmt, oracle):
    assert check_sample2d(REF, oracle, W, H, fmt) == []


@pytest.mark.parametrize("N", [1, 2, 8])
@pytest.mark.parametrize("fmt", FMTS)
def test_oracle_cube_sample_matches_float64_seamless(N, fmt, oracle):
    count = {}
    assert check_cube(REF, oracle, N, fmt, n=2400, count=count) == []
    assert count["samples"] > 1000


# ---------------------------------------------------------------------- closed-form scenes
W_IMG = 64
QUAD = [(-0.8, -0.8, 1.0), (0.8, -0.8, 1.0), (0.8, 0.8, 1.0), (-0.8, 0.8, 1.0)]
CORNERS = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float64)
BACKGROUND = (0.1, 0.2, 0.3, 1.0)


class Case:
    """A camera-facing quad at z = 1 seen from the origin (or only the environment), and what texref needs to predict it."""

    def __init__(self, S, name, mat=None, textures=None, uv0=(0.0, 1.0), uv1=None, tangent=(1, 0, 0), back=False,
                 env=BACKGROUND, env_texture=None, env_transform=None, camera=None, quad=True):
        self.name = name
        self.textures = textures or {}
        normal = (0, 0, 1) if back else (0, 0, -1)
        uvs0 = uv0[0] + CORNERS * uv0[1]
        uvs1 = None if uv1 is None else uv1[0] + CORNERS * uv1[1]
        self.vb = S.make_vertices(np.array(QUAD, np.float32), np.tile(normal, (4, 1)), uvs0, np.tile(tangent, (4, 1)), uvs1)
        self.ib = S.make_indices([0, 1, 2, 0, 2, 3])
        self.mat = mat if mat is not None else S.material((1, 1, 1))
        self.uv_mag = float(np.abs(texref.f16_values(self.vb["TexCoord0"])).max()) + 1
        if uv1 is not None:
            self.uv_mag = max(self.uv_mag, float(np.abs(texref.f16_values(self.vb["TexCoord1"])).max()) + 1)
        mesh = S.Mesh(self.vb, self.ib, True, self.mat, has_tangents=True, has_uv=(True, uv1 is not None),
                      textures={k: (t, i) for k, (t, i) in self.textures.items()})
        cam = camera if camera is not None else S.make_camera((0, 0, 0), hfov_deg=90.0, aspect=1.0)
        # environment-only frame: the quad's instance is masked out (instance mask 0)
        self.scene = S.Scene([S.MeshNode([mesh])], [S.RenderObject(0, S.trs(), visible=quad)], cam, S.make_scene_data(env))
        self.scene.env_texture = env_texture
        if env_transform is not None:
            self.scene.scene_data["EnvironmentLightTransform"] = env_transform
        self.scene.finalize()
        self.env_texture, self.quad = env_texture, quad

    def ref_textures(self):
        return {k: (t.data, t.fmt, i) for k, (t, i) in self.textures.items()}


def oracle_gbuffer(oracle, L, scene, W, H):
    gb = {k: np.zeros((H, W, c), dt) for k, (dt, c) in L.GBUFFER_FORMATS.items()}
    consts = np.zeros((), L.GBUFFER_CONSTANTS)
    consts["RenderSize"] = (W, H); consts["Flags"] = 0xFFFFFFFF & ~0xC0
    osc = oracle.OracleScene(scene, 0)
    osc.gbuffer(consts, gb)
    osc.close()
    return gb


def neighbour_diff(tex):
    d = 0.0
    for ax in (0, 1):
        if tex.shape[ax] > 1:
            d = max(d, float(np.abs(tex - np.roll(tex, 1, axis=ax)).max()))
    return d


def check_case(ref, case, gb, W=W_IMG, stats=None):
    """Compare a rendered G-buffer with texref's prediction; returns a list of failures. Pixels within the tolerance of the
    quad's outline are excluded and counted."""
    H = W
    fails = []
    cam = case.scene.camera
    o, d = texref.pinhole_rays(cam, W, H)
    sd = case.scene.scene_data
    env_data = case.env_texture.data if case.env_texture is not None else None
    env_fmt = case.env_texture.fmt if case.env_texture is not None else 0
    hits = texref.quad_hits(o, d, case.vb, case.ib)
    # outline distance in barycentric units: the shared diagonal (b1 = 0 of triangle 0, b2 = 0 of triangle 1) is not an edge
    b0 = 1 - hits["b1"] - hits["b2"]
    outline = np.where(hits["tri"] == 0, np.minimum(b0, hits["b2"]), np.minimum(b0, hits["b1"]))
    near_edge = np.abs(outline) < 1e-4
    hit_gpu = np.isfinite(gb["Position"][..., 0])
    hit_ref = hits["hit"] if case.quad else np.zeros((H, W), bool)
    if stats is not None:
        stats["edge_excluded"] = stats.get("edge_excluded", 0) + int(near_edge.sum())
    if (hit_gpu != hit_ref)[~near_edge].any():
        fails.append(f"{case.name}: coverage differs at {int(((hit_gpu != hit_ref) & ~near_edge).sum())} pixels")
    use = hit_gpu & hit_ref & ~near_edge
    miss = ~hit_gpu & ~hit_ref
    rad = gb["Radiance"].view(np.float16).astype(np.float64)
    # environment on misses
    if miss.any():
        env = ref.environment(sd, env_data, env_fmt, d[miss])
        if env_data is not None:
            size = max(env_data.shape[-3], env_data.shape[-2])
            w = d[miss] @ np.asarray(sd["EnvironmentLightTransform"], np.float64).reshape(3, 4)[:, :3].T
            w /= np.linalg.norm(w, axis=-1, keepdims=True)
            r = np.hypot(w[:, 0], w[:, 2])
            pos_err = texref.texel_position_error(size, 1.0)
            if not int(sd["IsEnvironmentLightTextureCubeMap"]):
                pos_err = pos_err + size * 2.0 ** -21 / np.maximum(r, 1e-6)     # atan2 near the poles
            dec = REF.decode(env_data, env_fmt)
            tol = texref.value_tolerance(pos_err, neighbour_diff(dec) if dec.ndim == 3 else np.ptp(dec), np.abs(dec).max())
        else:
            tol = 2e-6 * np.maximum(np.abs(env), 1)                              # constant colour; sky: powf in fp32
        tol = np.broadcast_to(np.reshape(tol, (-1, 1)) if np.ndim(tol) == 1 else tol, env.shape)
        ok = texref.codes_agree(gb["Radiance"][miss][:, :3], env, tol, "f16")
        if not ok.all():
            i = np.argwhere(~ok.all(1))[0, 0]
            fails.append(f"{case.name}: environment radiance off at {int((~ok.all(1)).sum())} pixels, e.g. got {rad[miss][i, :3]} want {env[i]}")
    if not use.any():
        return fails
    uv, N, T, front = texref.hit_attributes(case.vb, case.ib, {k: v[use] for k, v in hits.items()}, d[use])
    texs = case.ref_textures()
    m = ref.evaluate_material(case.mat, texs, uv, N, T)
    # tolerance: texel-position error x largest neighbour difference of any texture bound, plus fp32 ulps
    sizes = [max(t[0].shape[0], t[0].shape[1]) for t in texs.values()] or [1]
    diffs = [neighbour_diff(REF.decode(t[0], t[1])) for t in texs.values()] or [0.0]
    mags = [np.abs(REF.decode(t[0], t[1])).max() for t in texs.values()] or [1.0]
    tol = texref.value_tolerance(texref.texel_position_error(max(sizes), case.uv_mag), max(diffs), max(mags), ulps=16)
    bcm = gb["BaseColorMetalness"][use].astype(np.float64)
    checks = [("BaseColor", bcm[:, :3], m["BaseColor"][:, :3], "unorm8"), ("Metallic", bcm[:, 3], m["Metallic"], "unorm8"),
              ("Roughness", gb["NormalRoughness"][use][:, 3], np.maximum(texref.MIN_ROUGHNESS, m["Roughness"]), "snorm16"),
              ("Normal", gb["NormalRoughness"][use][:, :3], m["Normal"], "snorm16"),
              ("Emission", gb["Radiance"][use][:, :3], m["Emission"], "f16"),
              ("IOR", gb["IOR"][use][:, 0], m["IOR"], "f16")]
    tm = m["Metallic"] < 1
    checks.append(("Transmission", gb["Transmission"][use][tm][:, 0], m["Transmission"][tm], "unorm8"))
    for name, got, want, kind in checks:
        t = tol * (8 if name == "Normal" else 1) * (float(case.mat["EmissiveStrength"]) if name == "Emission" else 1)
        ok = texref.codes_agree(got, want, t, kind)
        if not ok.all():
            bad = ~ok if ok.ndim == 1 else ~ok.all(-1)
            i = np.argmax(bad)
            fails.append(f"{case.name}: {name} off at {int(bad.sum())} pixels, e.g. got {got[i]} want {want[i]}")
    return fails


def texture(S, W, H, fmt, seed, alpha=None):
    data = make_texels(W, H, fmt, seed)
    if alpha is not None:
        data[..., 3] = alpha
    return S.Texture(data, srgb=(fmt == texref.FMT_RGBA8_SRGB))


UV_CASES = {"unit": (0.0, 1.0), "negative": (-4.6, 3.1), "wraps": (1.0, 37.0), "near1000": (999.7, 1.6)}


def make_cases(S):
    """Every closed-form scene of the suite (a list of Case)."""
    cases = []
    for fmt in FMTS:
        for (W, H) in [(1, 7), (5, 3), (33, 17), (64, 64)]:
            for uvname, uv0 in UV_CASES.items():
                tex = texture(S, W, H, fmt, W * 7 + H + fmt)
                mat = S.material((1, 1, 1), emissive=(1, 1, 1), strength=2.0, metallic=0.5, roughness=0.5)
                cases.append(Case(S, f"quad_{fmt}_{W}x{H}_{uvname}", mat,
                                  {"BaseColor": (tex, 0), "EmissiveColor": (tex, 0), "MetallicRoughness": (tex, 0)}, uv0=uv0))
    t8 = texture(S, 8, 8, texref.FMT_RGBA8, 3); t5 = texture(S, 5, 3, texref.FMT_RGBA8, 4); t33 = texture(S, 33, 17, texref.FMT_RGBA8, 5)
    cases.append(Case(S, "uv_set_1", S.material((1, 1, 1), metallic=1.0, roughness=1.0),
                      {"BaseColor": (t8, 1), "Metallic": (t5, 0), "Roughness": (t33, 1)}, uv0=(0.0, 1.0), uv1=(-2.3, 3.7)))
    # gating: a zero factor skips the tap; an all-zero BaseColor skips it; MetallicRoughness wins over separate maps;
    # Transmission only where Metallic < 1 (after texturing)
    cases.append(Case(S, "gate_zero_metallic", S.material((1, 1, 1), metallic=0.0, roughness=0.7),
                      {"Metallic": (t8, 0), "Roughness": (t5, 0)}, uv0=(0.3, 2.0)))
    cases.append(Case(S, "gate_zero_basecolor", S.material((0, 0, 0)), {"BaseColor": (t8, 0)}, uv0=(0.3, 2.0)))
    cases.append(Case(S, "mr_precedence", S.material((1, 1, 1), metallic=0.9, roughness=0.8),
                      {"MetallicRoughness": (t33, 0), "Metallic": (t8, 0), "Roughness": (t5, 0)}, uv0=(0.1, 1.3)))
    mtex = np.zeros((4, 4, 4), np.uint8); mtex[..., 0] = 255; mtex[::2, ::2, 0] = 90; mtex[..., 3] = 255
    cases.append(Case(S, "transmission_metal_gate", S.material((1, 1, 1), metallic=1.0, transmission=1.0),
                      {"Metallic": (S.Texture(mtex), 0), "Transmission": (t33, 0)}, uv0=(0.0, 1.0)))
    # normal mapping, front and back face, non-orthogonal tangent
    nm = make_texels(16, 16, texref.FMT_RGBA8, 9); nm[..., :2] = 64 + nm[..., :2] // 2
    for back in (False, True):
        cases.append(Case(S, f"normal_map_{'back' if back else 'front'}", S.material((0.5, 0.5, 0.5)),
                          {"Normal": (S.Texture(nm), 0)}, uv0=(0.2, 1.7), tangent=(0.8, 0.6, 0.0), back=back))
    return cases


def env_cases(S):
    rng = np.random.default_rng(21)
    ang = 0.7
    M = np.zeros((3, 4), np.float32)                     # rotation about an oblique axis (not symmetric)
    ax = np.array([0.3, 0.8, 0.52]); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M[:, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    ll = (rng.random((16, 32, 4)) * 3).astype(np.float32)
    cube = (rng.random((6, 8, 8, 4)) * 3).astype(np.float32)
    out = []
    cams = {"front": S.make_camera((0, 0, 0), forward=(0.2, 0.1, -1), hfov_deg=120.0, aspect=1.0),       # lat-long seam (-z)
            "pole": S.make_camera((0, 0, 0), forward=(0.01, 1, 0.013), up=(0, 0, 1), hfov_deg=110.0, aspect=1.0),
            "corner": S.make_camera((0, 0, 0), forward=(1, 1.03, 0.97), hfov_deg=100.0, aspect=1.0)}
    for cname, cam in cams.items():
        out.append(Case(S, f"env_constant_{cname}", quad=False, camera=cam, env=(0.25, 0.5, 2.0, 1.0)))
        out.append(Case(S, f"env_sky_{cname}", quad=False, camera=cam, env=(0, 0, 0, -1)))
        for tname, tex in (("latlong", ll), ("cube", cube)):
            out.append(Case(S, f"env_{tname}_{cname}", quad=False, camera=cam, env_texture=S.Texture(tex)))
            out.append(Case(S, f"env_{tname}_{cname}_rotated", quad=False, camera=cam, env_texture=S.Texture(tex), env_transform=M))
    return out


def alpha_case(S):
    """An alpha-masked quad in front of a constant background. AlphaCutoff 1.0 and texels of alpha 255: a footprint of
    such texels samples to exactly 1.0 in fp32 (fma(1, w, 1 - w) rounds to 1), so those pixels sit exactly at the cutoff."""
    a = np.zeros((8, 8, 4), np.uint8); a[..., :3] = 200
    a[..., 3] = np.where((np.arange(8)[:, None] // 2 + np.arange(8)[None, :] // 2) % 2 == 0, 255, 0)
    mat = S.material((1, 1, 1)); mat["AlphaMode"] = 1; mat["AlphaCutoff"] = 1.0
    return Case(S, "alpha_mask", mat, {"BaseColor": (S.Texture(a, srgb=True), 0)}, uv0=(0.0, 1.0))


def check_alpha(ref, case, gb, W=W_IMG, stats=None):
    o, d = texref.pinhole_rays(case.scene.camera, W, W)
    hits = texref.quad_hits(o, d, case.vb, case.ib)
    b0 = 1 - hits["b1"] - hits["b2"]
    outline = np.where(hits["tri"] == 0, np.minimum(b0, hits["b2"]), np.minimum(b0, hits["b1"]))
    inside = hits["hit"] & (np.abs(outline) > 1e-4)
    uv, _, _, _ = texref.hit_attributes(case.vb, case.ib, {k: v[inside] for k, v in hits.items()}, d[inside])
    opaque, alpha = ref.is_opaque(case.mat, case.ref_textures(), uv)
    # a 2x2 footprint of equal texels samples exactly; elsewhere the value moves with the position error
    tex = REF.decode(case.textures["BaseColor"][0].data, case.textures["BaseColor"][0].fmt)
    diff, _ = REF.footprint2d(tex, uv[0][0], uv[0][1])
    tol = texref.value_tolerance(texref.texel_position_error(8, case.uv_mag), diff, 1.0)
    # exact where every position within the error bound samples the same 0 or 1
    e = texref.texel_position_error(8, case.uv_mag) / 8
    shifted = [REF.sample2d(tex, uv[0][0] + su * e, uv[0][1] + sv * e)[..., 3] for su in (-1, 1) for sv in (-1, 1)]
    uniform = np.isin(alpha, (0.0, 1.0)) & np.all([x == alpha for x in shifted], 0)
    borderline = (np.abs(alpha - float(case.mat["AlphaCutoff"])) <= tol) & ~uniform
    got = np.isfinite(gb["Position"][..., 0])[inside]
    if stats is not None:
        stats["cutoff_excluded"] = int(borderline.sum()); stats["at_cutoff"] = int((uniform & (alpha == 1.0)).sum())
    bad = (got != opaque) & ~borderline
    return [f"alpha_mask: {int(bad.sum())} pixels disagree on opacity"] if bad.any() else []


@pytest.fixture(scope="module")
def cases(pkg):
    return make_cases(pkg.scenes) + env_cases(pkg.scenes)


def test_oracle_renders_match_float64(cases, oracle, pkg):
    stats, fails = {}, []
    for case in cases:
        fails += check_case(REF, case, oracle_gbuffer(oracle, pkg.layouts, case.scene, W_IMG, W_IMG), stats=stats)
    assert fails == []
    assert stats["edge_excluded"] < 0.01 * len(cases) * W_IMG * W_IMG, stats


def test_oracle_alpha_cutoff_is_inclusive(oracle, pkg):
    case = alpha_case(pkg.scenes)
    stats = {}
    assert check_alpha(REF, case, oracle_gbuffer(oracle, pkg.layouts, case.scene, W_IMG, W_IMG), stats=stats) == []
    assert stats["at_cutoff"] > 100, stats                # many pixels test alpha == AlphaCutoff exactly


# ---------------------------------------------------------------------- mutations: each must be caught
def run_all_checks(ref, oracle, pkg, cases):
    fails = []
    for (W, H) in [(1, 7), (5, 3), (33, 17)]:
        for fmt in FMTS:
            fails += check_sample2d(ref, oracle, W, H, fmt, n=60)
    for N in (1, 2, 8):
        fails += check_cube(ref, oracle, N, texref.FMT_RGBA32F, n=400)
    for case in cases:
        fails += check_case(ref, case, oracle_gbuffer(oracle, pkg.layouts, case.scene, 32, 32), W=32)
    case = alpha_case(pkg.scenes)
    fails += check_alpha(ref, case, oracle_gbuffer(oracle, pkg.layouts, case.scene, W_IMG, W_IMG))
    return fails


@pytest.mark.parametrize("mutation", texref.MUTATIONS)
def test_mutated_reference_is_caught(mutation, oracle, pkg, cases):
    fails = run_all_checks(texref.Reference(**{mutation: True}), oracle, pkg, cases)
    assert fails, f"mutation {mutation} passed every comparison: the tolerances are too loose"


# ---------------------------------------------------------------------- GPU tier
def gpu_gbuffer(ptamd, ctx, scene, W, H):
    ge.load_package()
    import dxpbrt_amd.scenes as S
    ctx.set_sharding(0, 1, 16)
    g = ptamd.Scene(ctx, scene)
    r = ptamd.Renderer(ctx, g, W, H, with_f32=True)
    r.render(S.graphics_settings(W, H, spp=1, bounces=0))
    ctx.sync()
    return ptamd.textures_to_numpy(r.textures)


GB_EXACT = ("Position", "FlatNormal", "GeometricNormal", "LinearDepth", "NormalizedDepth", "BaseColorMetalness",
            "NormalRoughness", "IOR", "Transmission", "Radiance")


def assert_same_gbuffer(out, ref, name):
    for k in GB_EXACT:
        a, b = out[k], ref[k]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), f"{name}: G-buffer {k} differs from the oracle"


@pytest.mark.gpu
def test_gpu_renders_match_float64_and_oracle(gpu, ptamd, oracle, pkg, cases):
    fails = []
    for case in cases + [alpha_case(pkg.scenes)]:
        out = gpu_gbuffer(ptamd, gpu, case.scene, W_IMG, W_IMG)
        fails += (check_alpha if case.name == "alpha_mask" else check_case)(REF, case, out)
        ref = oracle_gbuffer(oracle, pkg.layouts, case.scene, W_IMG, W_IMG)
        if "latlong" in case.name or "sky" in case.name:        # atan2f / acosf / powf: libm, not bit-pinned
            for k in GB_EXACT[:-1]:
                a, b = out[k], ref[k]
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{case.name}: {k}"
        else:
            assert_same_gbuffer(out, ref, case.name)
    assert fails == []


def visibility_panes(S):
    rng = np.random.default_rng(3)
    a = np.zeros((8, 8, 4), np.uint8); a[..., :3] = rng.integers(0, 256, (8, 8, 3)); a[..., 3] = rng.choice([0, 255], (8, 8))
    masked = S.material((1, 1, 1)); masked["AlphaMode"] = 1; masked["AlphaCutoff"] = 0.5
    mt = np.full((4, 4, 4), 255, np.uint8); mt[2:, :, 0] = 128             # a band of 255 samples to exactly 1.0
    metal = S.material((0.9, 0.8, 0.7), metallic=1.0, transmission=1.0)     # passes light only where the texture lowers Metallic
    tr = texture(S, 5, 3, texref.FMT_RGBA8, 6); bc = texture(S, 7, 1, texref.FMT_RGBA8_SRGB, 7)
    glass = S.material((0.9, 0.95, 1.0), transmission=1.0)
    return [Case(S, "masked", masked, {"BaseColor": (S.Texture(a, srgb=True), 0)}, uv0=(-1.3, 2.1)),
            Case(S, "metal", metal, {"Metallic": (S.Texture(mt), 0)}, uv0=(-1.3, 2.1)),
            Case(S, "glass", glass, {"Transmission": (tr, 0), "BaseColor": (bc, 0)}, uv0=(-1.3, 2.1))]


def visibility_rays(n=4000, seed=3):
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3)); o[:, 2] = -1.0
    target = np.concatenate([rng.uniform(-0.78, 0.78, (n, 2)), np.ones((n, 1))], 1)
    dd = target - o; ln = np.linalg.norm(dd, axis=1, keepdims=True); dd /= ln
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = o; rays[:, 3] = 1e-3; rays[:, 4:7] = dd; rays[:, 7] = ln[:, 0] + 1.0
    return rays


def check_visibility(case, rays, got):
    """got: [n, 4] (visibility rgb, 1 = unoccluded) from a visibility kernel; compared with texref's coloured-visibility
    IsOpaque at the UV each ray hits."""
    o = rays[:, 0:3].astype(np.float64); dd = rays[:, 4:7].astype(np.float64)
    hits = texref.quad_hits(o, dd, case.vb, case.ib)
    assert hits["hit"].all()
    uv, _, _, _ = texref.hit_attributes(case.vb, case.ib, hits, dd)
    blocks, vis, alpha, metallic = REF.is_opaque_visibility(case.mat, case.ref_textures(), uv, np.ones(3))
    tex_diff = max(neighbour_diff(REF.decode(t.data, t.fmt)) for t, _ in case.textures.values())
    tol = texref.value_tolerance(texref.texel_position_error(8, case.uv_mag), tex_diff, 1.0, ulps=16)
    # rays whose decisive value lies within the tolerance of a threshold are not judged on the flag
    if case.name == "masked":
        borderline = np.abs(alpha - 0.5) <= tol
    elif case.name == "metal":
        borderline = (np.abs(metallic - 1.0) <= tol) & (metallic != 1.0)
    else:
        borderline = vis.max(1) <= tol
    got = got.astype(np.float64)
    assert borderline.mean() < 0.05, case.name
    assert np.array_equal(got[~borderline, 3] == 1.0, ~blocks[~borderline]), case.name
    assert (np.abs(got[~borderline, :3] - vis[~borderline]) <= tol).all(), case.name
    if case.name == "glass":                                   # coloured, partial visibility
        assert ((vis.max(1) > 0) & (vis.max(1) < 1)).mean() > 0.9
    else:                                                      # both outcomes occur
        assert blocks.any() and (~blocks).any(), case.name


def oracle_visibility(oracle, case, rays):
    ref = np.zeros((len(rays), 4), np.float32)
    osc = oracle.OracleScene(case.scene, accel_mode=0)
    oracle.lib().or_trace_visibility(osc.handle, rays.ctypes.data, len(rays), ref.ctypes.data)
    osc.close()
    return ref


def test_oracle_visibility_through_textured_panes(oracle, pkg):
    for case in visibility_panes(pkg.scenes):
        rays = visibility_rays()
        check_visibility(case, rays, oracle_visibility(oracle, case, rays))


@pytest.mark.gpu
def test_gpu_visibility_through_textured_panes(gpu, ptamd, oracle, pkg):
    """pt_trace_visibility (heap path sample_map, where renders use the resolved slots) against texref's coloured-visibility
    IsOpaque: rays aimed at textured panes at known UVs. Panes: alpha-masked, metallic exactly 1 after the texture,
    transmission + base-colour maps. Also bit-exact with the oracle."""
    import torch
    for case in visibility_panes(pkg.scenes):
        rays = visibility_rays()
        n = len(rays)
        gpu.set_sharding(0, 1, 16)
        g = ptamd.Scene(gpu, case.scene)
        dr = torch.from_numpy(rays).cuda(); dv = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        gpu.check(gpu.lib.pt_trace_visibility(gpu.handle, C.c_void_p(dr.data_ptr()), n, C.c_void_p(dv.data_ptr())))
        gpu.sync()
        got = dv.cpu().numpy()
        del g
        check_visibility(case, rays, got)
        assert np.array_equal(got.view(np.uint32), oracle_visibility(oracle, case, rays).view(np.uint32)), case.name
