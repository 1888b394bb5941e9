"""The scenes of the BRDF-candidate tests: a glossy floor under a large emissive quad (the case light sampling is weakest at), with a
second emitter instance, an opaque bar, and optionally an alpha-masked pane between the floor and the emitter."""
import numpy as np

CUTOFF = 0.25        # the positive BrdfCutoff of the tests: a ray of pdf q reaches sqrt(3 q), around the floor-to-emitter distance at q ~ 1


def oracle_gbuffer(oracle, L, scene, W, H):
    """the scene's G-buffer as the CPU oracle renders it (the planes of textures_to_numpy), and the oracle scene (close() it)"""
    gb = {k: np.zeros((H, W, c), dt) for k, (dt, c) in L.GBUFFER_FORMATS.items()}
    consts = np.zeros((), L.GBUFFER_CONSTANTS)
    consts["RenderSize"] = (W, H); consts["Flags"] = L.GBufferFlags.DefaultNoDenoiser
    osc = oracle.OracleScene(scene, accel_mode=0)
    osc.gbuffer(consts, gb)
    return gb, osc


def glossy_scene(S, aspect, roughness=0.25, metallic=0.6, pane=False, bar=True, quad=((-1.2, 1.2), (-0.6, 1.4)), eye=((0, 0.9, -2.8), (0, -0.25, 1))):
    """floor y = 0 (GGX, `roughness`, `metallic`); a down-facing emissive quad of 2.4 x 2.0 at y = 1.2 and one emissive triangle on a second
    instance (light indices 0-1 and 2); an opaque bar at y = 0.5 that some reflected rays stop on; pane: an alpha-masked (AlphaMode Mask)
    checker lattice at y = 0.6 under the quad, rays go through its holes and stop on its texels. The camera sits below the emitter.
    quad: the x and z extent of the emissive quad; eye: the camera's position and forward direction.
    The emitters are smoother than MinRoughness, so their own pixels are empty surfaces (a pixel on an emitter sees its own triangle edge-on)."""
    floor = S.quad_mesh((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2), (0, 1, 0), S.material((0.7, 0.6, 0.5), roughness=roughness, metallic=metallic))
    (qx0, qx1), (qz0, qz1) = quad
    quad = S.quad_mesh((qx0, 1.2, qz0), (qx1, 1.2, qz0), (qx1, 1.2, qz1), (qx0, 1.2, qz1), (0, -1, 0),
                       S.material((0.5, 0.5, 0.5), emissive=(1.0, 0.9, 0.7), strength=5.0, roughness=0.02))
    pos = np.array([(-1.6, 0.9, 0.2), (-1.3, 1.0, 0.9), (-1.7, 0.8, 0.8)], np.float32)
    tri = S.Mesh(S.make_vertices(pos, np.tile(np.float32([1, -1, 0]) / np.sqrt(np.float32(2)), (3, 1))), S.make_indices([0, 1, 2]), True,
                 S.material((0.5, 0.5, 0.5), emissive=(0.6, 0.8, 1.0), strength=20.0, roughness=0.02))
    nodes = [S.MeshNode([floor]), S.MeshNode([quad]), S.MeshNode([tri])]
    if bar:
        nodes.append(S.MeshNode([S.quad_mesh((-0.5, 0.5, 0.1), (0.5, 0.5, 0.1), (0.5, 0.5, 0.35), (-0.5, 0.5, 0.35), (0, -1, 0),
                                             S.material((0.9, 0.9, 0.9), roughness=0.8))]))
    if pane:
        n, cells = 16, 4
        y, x = np.mgrid[0:n, 0:n]
        hole = (((x * cells) // n + (y * cells) // n) % 2).astype(bool)
        img = np.zeros((n, n, 4), np.uint8)
        img[~hole] = (200, 200, 40, 255)
        img[hole] = (10, 10, 10, 0)
        mask = S.material((1, 1, 1), roughness=0.9); mask["AlphaMode"] = 1; mask["AlphaCutoff"] = 0.5
        nodes.append(S.MeshNode([S.quad_mesh((-1.0, 0.6, -0.4), (1.0, 0.6, -0.4), (1.0, 0.6, 1.0), (-1.0, 0.6, 1.0), (0, -1, 0), mask, uv_scale=1.0,
                                             textures={"BaseColor": (S.Texture(img, srgb=True), 0)})]))
    objects = [S.RenderObject(i, S.trs()) for i in range(len(nodes))]
    cam = S.make_camera(eye[0], forward=eye[1], hfov_deg=70.0, aspect=aspect)
    return S.Scene(nodes, objects, cam, S.make_scene_data((0, 0, 0, 1)), name="di_brdf_glossy").finalize()
