"""Textured scenes for the float64 replay of the G-buffer pass and the path estimator (tests/test_textured_estimator.py): surfaceref's
`transformed` -- mirrored and strongly non-uniform instances, a hidden instance, 32-bit indices, a quad seen from behind -- with UV sets and
textures on every piece, alpha-masked panes, and a lat-long or cube environment. At most 2 000 triangles, rendered at 48 x 32.

What carries what (object index = instance order; sizes are width x height):
  sphere   (two instances, one mirrored; Metallic 1, no tangents)  BaseColor 16x16 sRGB on TexCoord1, MetallicRoughness 5x3 RGBA8 on TexCoord0,
           a Normal texture that must NOT perturb: the mesh has no tangents
  box      (mirrored instance; tangents)  Normal 16x16 RGBA8, BaseColor 5x3 RGBA32F
  bare     (no vertex normals; dielectric, IOR 1.33; transmissive=)  Transmission 16x16 RGBA8, BaseColor 1x1 sRGB
  wide     (32-bit indices; Metallic FACTOR 1 lowered by its texture, so the Transmission tap is gated on the textured value)
           Metallic 5x3 RGBA32F, Roughness 1x1 RGBA8, Transmission 5x3 RGBA8 (transmissive=)
  quad     (the emitter, seen from behind; tangents)  EmissiveColor 16x16 RGBA32F, Normal 16x16 RGBA8, Roughness 1x1 RGBA32F
  floor    BaseColor 5x3 sRGB at UVs up to 3 (wraps), back wall BaseColor 16x16 RGBA8
  solid    AlphaMode Opaque with a holed base colour and AlphaCutoff 0.5: flagged OPAQUE, it must block
  masked=: a pane in front of the emitter, a pane between the floor and the back wall, and a two-geometry bottom level whose second
           geometry alone is AlphaMode Mask (its first one is plain and opaque), with AlphaCutoff 1: its solid cells stand AT the cutoff
Texels are low-frequency waves (one fp32 ulp of UV moves a value by little); alpha masks are cells of 4 x 4 (8 x 8) hard 0 / 255 texels."""
import numpy as np

import texref

SIZE = (48, 32)


def wave(w, h, fmt, seed, lo=0.15, hi=0.95, alpha=None):
    """smooth texels: per channel a product of one low-frequency sine per axis, in [lo, hi]; RGBA32F reaches above 1 when hi does"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 4))
    for c in range(4):
        px, py, fx, fy = rng.random(4)
        img[..., c] = 0.5 + 0.5 * np.sin(2 * np.pi * ((x + 0.5) / max(w, 1) * (0.5 + fx) + px)) * np.cos(2 * np.pi * ((y + 0.5) / max(h, 1) * (0.5 + fy) + py))
    img = lo + (hi - lo) * img
    img[..., 3] = 1.0
    if fmt == texref.FMT_RGBA32F:
        return img.astype(np.float32)
    out = np.floor(np.clip(img, 0, 1) * 255 + 0.5).astype(np.uint8)
    if alpha is not None:
        out[..., 3] = alpha
    return out


def cells(n=16, cell=4, phase=0):
    """hard 0 / 255 alpha in cells of `cell` texels, checkerboard"""
    y, x = np.mgrid[0:n, 0:n]
    return np.where(((x // cell + y // cell + phase) % 2) == 0, 255, 0).astype(np.uint8)


def normal_map(seed):
    """tangent-space xy within 0.5 +- 0.2 (far from the rim x^2 + y^2 = 1), smooth"""
    t = wave(16, 16, texref.FMT_RGBA8, seed, lo=0.3, hi=0.7)
    t[..., 2] = 255
    return t


def add_uvs(S, mesh, uv0=None, uv1=None, tangents=None, textures=None):
    """give an existing mesh UV sets / tangents (per vertex arrays) and textures"""
    if uv0 is not None:
        mesh.vertices["TexCoord0"] = np.asarray(uv0, np.float16)
    if uv1 is not None:
        mesh.vertices["TexCoord1"] = np.asarray(uv1, np.float16)
    if tangents is not None:
        mesh.vertices["Tangent"] = S.encode_snorm16(tangents)
        mesh.has_tangents = True
    mesh.has_uv = (uv0 is not None, uv1 is not None)
    mesh.textures = textures
    return mesh


def box_uvs(mesh):
    """per face of scenes.box_mesh: the two in-face coordinates as UV (0.1 .. 0.9 so that f16 stores them inexactly), the first in-face axis as
    tangent"""
    p = np.asarray(mesh.vertices["Position"], np.float64)
    uv, tan = np.zeros((len(p), 2)), np.zeros((len(p), 3))
    for f in range(len(p) // 4):
        q = p[4 * f:4 * f + 4]
        axis = [k for k in range(3) if np.ptp(q[:, k]) == 0][0]
        a, b = (axis + 1) % 3, (axis + 2) % 3
        uv[4 * f:4 * f + 4] = np.stack([q[:, a] * 0.8 + 0.5, q[:, b] * 0.8 + 0.5], -1)
        tan[4 * f:4 * f + 4, a] = 1.0
    return uv, tan


def rotation(axis, angle):
    ax = np.asarray(axis, np.float64); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M = np.zeros((3, 4), np.float32)
    M[:, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    return M


def environment(S, kind):
    """RGBA32F with values above 1, smooth, under an oblique rotation (not symmetric: its transpose is another rotation)"""
    if kind == "latlong":
        return S.Texture(wave(16, 8, texref.FMT_RGBA32F, 41, lo=0.1, hi=3.0)), rotation((0.3, 0.8, 0.52), 0.7)
    faces = np.stack([wave(4, 4, texref.FMT_RGBA32F, 50 + f, lo=0.2 + 0.3 * f, hi=1.0 + 0.4 * f) for f in range(6)])
    return S.Texture(faces), rotation((0.6, -0.3, 0.74), 1.1)


def textured(S, masked=True, transmissive=True, env=None, large=False, aspect=SIZE[0] / SIZE[1]):
    """masked / transmissive: with the alpha-tested geometry / the transmissive objects (without both, the frame compiles the alpha test and
    the transmission lobe out). env: None (a constant colour), "latlong" or "cube". large: a finer sphere without its mirrored twin, whose
    traversal copy exceeds the LDS limit, so the streaming form renders it."""
    F8, FS, FF = texref.FMT_RGBA8, texref.FMT_RGBA8_SRGB, texref.FMT_RGBA32F
    tex = lambda w, h, fmt, seed, **kw: S.Texture(wave(w, h, fmt, seed, **kw), srgb=(fmt == FS))
    sphere = S.icosphere_mesh(3 if large else 2, S.material((0.9, 0.8, 0.7), metallic=1.0, roughness=0.6))
    p = np.asarray(sphere.vertices["Position"], np.float64)
    add_uvs(S, sphere, uv0=p[:, [0, 1]] * 0.45 + 0.5, uv1=p[:, [2, 1]] * 0.9 + 0.3,
            textures={"BaseColor": (tex(16, 16, FS, 1, lo=0.3), 1), "MetallicRoughness": (tex(5, 3, F8, 2, lo=0.3, hi=0.9), 0),
                      "Normal": (S.Texture(normal_map(3)), 0)})
    box = S.box_mesh(S.material((0.9, 0.9, 0.9), roughness=0.4))
    uv, tan = box_uvs(box)
    add_uvs(S, box, uv0=uv, tangents=tan, textures={"Normal": (S.Texture(normal_map(4)), 0), "BaseColor": (tex(5, 3, FF, 5, lo=0.2, hi=0.9), 0)})
    bare = S.box_mesh(S.material((0.8, 0.9, 0.9), roughness=0.3, ior=1.33, transmission=0.8 if transmissive else 0.0), has_normals=False)
    add_uvs(S, bare, uv0=box_uvs(bare)[0], textures={"Transmission": (tex(16, 16, F8, 6, lo=0.3), 0), "BaseColor": (tex(1, 1, FS, 7, lo=0.6), 0)})
    wide = S.box_mesh(S.material((0.6, 0.3, 0.6), metallic=1.0, roughness=0.5, transmission=0.6 if transmissive else 0.0))
    wide.indices = wide.indices.astype(np.uint32)
    add_uvs(S, wide, uv0=box_uvs(wide)[0], textures={"Metallic": (tex(5, 3, FF, 8, lo=0.2, hi=0.7), 0), "Roughness": (tex(1, 1, F8, 9, lo=0.5), 0),
                                                      "Transmission": (tex(5, 3, F8, 10, lo=0.4), 0)})
    quad = S.quad_mesh((-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0), (0, 0, -1),
                       S.material((0.9, 0.9, 0.2), emissive=(1.0, 0.8, 0.6), strength=6.0, roughness=0.8), uv_scale=0.9,
                       textures={"EmissiveColor": (tex(16, 16, FF, 11, lo=0.2, hi=1.6), 0), "Normal": (S.Texture(normal_map(12)), 0),
                                 "Roughness": (tex(1, 1, FF, 13, lo=0.7), 0)})
    floor = S.quad_mesh((-1, 0, -1), (-1, 0, 1), (1, 0, 1), (1, 0, -1), (0, 1, 0), S.material((0.8, 0.8, 0.8)), uv_scale=3.0,
                        textures={"BaseColor": (tex(5, 3, FS, 14, lo=0.3), 0)})
    wall = S.quad_mesh((-1, -1, 0), (-1, 1, 0), (1, 1, 0), (1, -1, 0), (0, 0, -1), S.material((0.8, 0.8, 0.8)), uv_scale=0.95,
                       textures={"BaseColor": (tex(16, 16, F8, 15, lo=0.3), 0)})
    holed = lambda seed, phase: S.Texture(wave(16, 16, FS, seed, lo=0.4, alpha=cells(16, 4, phase)), srgb=True)
    solid_mat = S.material((0.7, 0.5, 0.3)); solid_mat["AlphaCutoff"] = 0.5                  # AlphaMode Opaque: the holes do not count
    solid = S.quad_mesh((-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0), (0, 0, -1), solid_mat, uv_scale=0.97,
                        textures={"BaseColor": (holed(16, 1), 0)})
    nodes = [S.MeshNode([m]) for m in (sphere, box, bare, wide, quad, floor, wall, solid)]
    objects = [
        S.RenderObject(0, S.trs((-1.6, 0.3, 0.2), 25.0, (1.0, 0.3, 0.6), pitch_deg=15.0)),
        S.RenderObject(1, S.trs((-0.1, 0.1, 0.6), -35.0, (-0.8, 0.5, 0.5), pitch_deg=-20.0)),       # mirrored, with the normal map
        S.RenderObject(2, S.trs((1.7, 0.0, 1.4), 50.0, (3.0, 0.2, 1.5), pitch_deg=10.0)),
        S.RenderObject(0, S.trs((0.9, 0.9, 0.4), -10.0, (-1.0, 0.4, 2.0), pitch_deg=30.0)),        # mirrored sphere
        S.RenderObject(3, S.trs((-0.9, -0.5, 0.0), 20.0, (0.5, 0.4, 0.7), pitch_deg=-5.0)),
        S.RenderObject(1, S.trs((0.0, 0.0, -1.5), 0.0, (3.0, 3.0, 0.1)), visible=False),          # would hide everything
        S.RenderObject(4, S.trs((0.6, -0.55, -0.4), 155.0, (0.9, 0.7, 1.0), pitch_deg=20.0)),          # the emitter, seen from behind
        S.RenderObject(5, S.trs((0.0, -1.0, 1.0), 0.0, (4.0, 1.0, 3.0))),
        S.RenderObject(6, S.trs((0.0, 0.2, 3.2), 0.0, (3.5, 1.3, 1.0))),                            # the back wall
        S.RenderObject(7, S.trs((-1.9, -0.45, 0.9), -40.0, (0.8, 0.8, 1.0))),                       # flagged OPAQUE
    ]
    if large:
        del objects[3]
    if masked:
        mask = S.material((0.9, 0.9, 0.9)); mask["AlphaMode"] = 1; mask["AlphaCutoff"] = 0.5
        pane = lambda seed, phase, scale: S.quad_mesh((-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0), (0, 0, -1), mask.copy(), uv_scale=scale,
                                                      textures={"BaseColor": (holed(seed, phase), 0)})
        plain = S.quad_mesh((-1.0, -0.5, 0), (0.0, -0.5, 0), (0.0, 0.5, 0), (-1.0, 0.5, 0), (0, 0, -1), S.material((0.3, 0.6, 0.4)))
        at_one = mask.copy(); at_one["AlphaCutoff"] = 1.0                     # solid cells sample to exactly 1.0: alpha == AlphaCutoff must commit
        second = S.quad_mesh((0.0, -0.5, 0), (1.0, -0.5, 0), (1.0, 0.5, 0), (0.0, 0.5, 0), (0, 0, -1), at_one, uv_scale=0.93,
                             textures={"BaseColor": (S.Texture(wave(16, 16, FS, 19, lo=0.4, alpha=cells(16, 8, 0)), srgb=True), 0)})
        first = len(nodes)
        nodes += [S.MeshNode([pane(17, 0, 0.9)]), S.MeshNode([pane(18, 1, 1.9)]), S.MeshNode([plain, second])]
        objects += [
            S.RenderObject(first, S.trs((0.55, -0.45, -0.75), 150.0, (1.1, 0.9, 1.0), pitch_deg=15.0)),  # in front of the emitter
            S.RenderObject(first + 1, S.trs((0.0, -0.2, 2.6), 5.0, (3.2, 1.4, 1.0), pitch_deg=-20.0)),    # between the floor and the back wall
            S.RenderObject(first + 2, S.trs((-0.95, 0.95, 1.5), 10.0, (1.3, 0.8, 1.0), pitch_deg=25.0)),    # two geometries, the second one masked
        ]
    cam = S.make_camera((0.15, 0.35, -3.2), forward=(0.02, -0.08, 1.0), hfov_deg=70.0, aspect=aspect, jitter=(0.23, -0.31))
    sc = S.Scene(nodes, objects, cam, S.make_scene_data((0.3, 0.4, 0.5, 1.0)), name="textured")
    if env is not None:
        sc.env_texture, M = environment(S, env)
        sc.scene_data["EnvironmentLightTransform"] = M
    return sc.finalize()
