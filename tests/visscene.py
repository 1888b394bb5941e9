"""What the reservoir-reuse and reservoir-visibility tests share: the pin scene (a floor, an opaque bar over it, five emissive triangles),
camera motion, the light records of a scene computed on the host, and a synthetic reservoir frame."""
import numpy as np

import restirref as R


BAR = ((-1.5, 1.5), 0.7, (-0.1, 0.15))        # the pin scene's occluder: x range, height, z range


def pin_scene(S, aspect, bar=BAR):
    """a GGX-ish floor, an opaque bar over it (its shadow crosses the view; parallax disocclusion as the camera moves), five emissive
    triangles on two instances. bar: another extent for the occluder (a wider plate shadows more of the floor from more of the lights)"""
    (bx0, bx1), by, (bz0, bz1) = bar
    floor = S.quad_mesh((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2), (0, 1, 0), S.material((0.6, 0.5, 0.4), roughness=0.4, metallic=0.3))
    bar = S.quad_mesh((bx0, by, bz0), (bx1, by, bz0), (bx1, by, bz1), (bx0, by, bz1), (0, -1, 0), S.material((0.9, 0.9, 0.9), roughness=0.8))

    def tris(pts, strength, color):
        pos = np.array(pts, np.float32)
        return S.Mesh(S.make_vertices(pos, np.tile(np.float32([0, -1, 0]), (len(pos), 1))), S.make_indices(list(range(len(pos)))), True,
                      S.material((0.5, 0.5, 0.5), emissive=color, strength=strength))
    a = tris([(-0.6, 1.5, -0.3), (0.7, 1.6, 0.1), (0.0, 1.4, 0.8), (-1.5, 1.3, 0.5), (-1.2, 1.3, 0.6), (-1.3, 1.35, 0.9),
              (1.0, 1.2, -0.8), (1.3, 1.2, -0.7), (1.1, 1.25, -0.4)], 6.0, (1.0, 0.8, 0.6))
    b = tris([(0.2, 1.1, 1.2), (0.5, 1.1, 1.3), (0.3, 1.15, 1.6), (-0.9, 1.0, -1.2), (-0.6, 1.0, -1.1), (-0.8, 1.05, -0.8)], 20.0, (0.6, 0.8, 1.0))
    nodes = [S.MeshNode([floor]), S.MeshNode([a]), S.MeshNode([bar]), S.MeshNode([b])]
    objects = [S.RenderObject(i, S.trs()) for i in range(4)]
    cam = S.make_camera((0, 2.2, -2.6), forward=(0, -0.6, 1), hfov_deg=70.0, aspect=aspect)
    return S.Scene(nodes, objects, cam, S.make_scene_data((0, 0, 0, 1)), name="di_reuse_pin").finalize()


def move(S, cam, prev, dx):
    """the camera shifted by dx along x, with Previous* from the last frame's camera (static geometry: IsStatic)"""
    c = S.make_camera(cam["Position"].astype(np.float64) + (dx, 0, 0), forward=cam["ForwardDirection"].astype(np.float64), hfov_deg=70.0,
                      aspect=float(np.linalg.norm(cam["RightDirection"]) / np.linalg.norm(cam["UpDirection"])))
    c["PreviousPosition"] = prev["Position"]
    for k in ("WorldToProjection", "ProjectionToView", "ViewToWorld"):
        c["Previous" + k] = prev[k]
    c["PreviousWorldToView"], c["PreviousViewToProjection"] = prev["PreviousWorldToView"], prev["PreviousViewToProjection"]
    return c


def set_camera(r, cam):
    for op in (r.gbuffer, r.raytracing, r.direct_lighting):
        op.GPUBuffers["Camera"] = cam


def host_lights(scene, L):
    """the emissive triangles of an untextured scene as TRIANGLE_LIGHT records, list order (instance, geometry, triangle): what
    TriangleLight::Initialize makes of them, in float64 rounded to the record's float32"""
    rec = []
    for i, ro in enumerate(scene.objects):
        M = np.asarray(scene.instance_data["ObjectToWorld"][i], np.float64).reshape(3, 4)
        for g, mesh in enumerate(scene.nodes[ro.node].meshes):
            m = mesh.material
            Le = np.asarray(m["EmissiveColor"], np.float64)[:3] * float(m["EmissiveStrength"])
            if not (Le > 0).any():
                continue
            p = mesh.vertices["Position"].astype(np.float64) @ M[:, :3].T + M[:, 3]
            for t, (a, b, c) in enumerate(np.asarray(mesh.indices, np.int64).reshape(-1, 3)):
                e0, e1 = p[b] - p[a], p[c] - p[a]
                n = np.cross(e0, e1)
                ln = np.linalg.norm(n)
                r = np.zeros((), L.TRIANGLE_LIGHT)
                r["Base"], r["Edge0"], r["Edge1"], r["Normal"], r["Area"], r["Radiance"] = p[a], e0, e1, n / ln, ln / 2, Le
                r["Power"] = ln / 2 * np.pi * float(R.LUMA @ Le)
                r["InstanceIndex"], r["GeometryIndex"], r["PrimitiveIndex"] = i, g, t
                rec.append(r)
    return np.array(rec, L.TRIANGLE_LIGHT)


def synthetic_frame(surf, lights, bsdf, seed, samples=8, with_visibility=False):
    """a reservoir frame over surfaces surf as initial sampling could have left it: a uniformly drawn light and point per valid pixel with
    its p-hat there, a weight around 1 / p-hat, M = samples; pixels whose p-hat is 0 are empty"""
    rng = np.random.default_rng(seed)
    H, W = surf.H, surf.W
    f = {k: np.zeros((H, W), np.float64 if k in ("U", "V", "W", "TargetPdf") else np.int64)
         for k in ("LightIndex", "U", "V", "W", "M", "TargetPdf", "Age", "Visibility")}
    f["LightIndex"][:] = -1
    pix = [(y, x) for y in range(H) for x in range(W) if surf.valid[y, x]]
    li = rng.integers(0, len(lights), len(pix))
    U, V = rng.random(len(pix)).astype(np.float32), rng.random(len(pix)).astype(np.float32)
    p = R.target_pdfs(surf, pix, lights, li, U, V, bsdf)
    for c, l, u, v, pp, k in zip(pix, li, U, V, p, rng.random(len(pix))):
        f["M"][c] = samples
        if pp > 0:
            f["LightIndex"][c], f["U"][c], f["V"][c], f["TargetPdf"][c] = l, u, v, float(np.float32(pp))
            f["W"][c] = float(np.float32((0.5 + k) / pp))
            if with_visibility:
                f["Age"][c] = int(k * 5)
    return f
