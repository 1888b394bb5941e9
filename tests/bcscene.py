"""What the block-compression tests share: seeded random block streams with both modes of every block kind present, a textured quad,
and a glTF whose textures carry both a PNG and an MSFT_texture_dds image."""
import json
import os

import numpy as np


def random_blocks(bc, fmt, n, seed):
    """n blocks of uniform random bytes: about half of the colour blocks have c0 > c1, half of the alpha-layout blocks a0 > a1"""
    return np.random.default_rng(seed).integers(0, 256, (n, bc.FMT_BLOCK_BYTES[fmt]), dtype=np.uint8)


def mode_fractions(bc, blocks, fmt):
    """{name: fraction of the blocks in the first mode} for every mode switch of the format (BC1: c0 > c1; alpha layout: a0 > a1)"""
    b = np.asarray(blocks).astype(np.int64)
    out = {}
    if fmt in bc.BC1_FORMATS:
        out["c0>c1"] = float(((b[:, 0] | (b[:, 1] << 8)) > (b[:, 2] | (b[:, 3] << 8))).mean())
    if fmt in bc.BC3_FORMATS or fmt in (bc.FMT_BC4_UNORM, bc.FMT_BC5_UNORM):
        out["a0>a1"] = float((b[:, 0] > b[:, 1]).mean())
    if fmt == bc.FMT_BC5_UNORM:
        out["g0>g1"] = float((b[:, 8] > b[:, 9]).mean())
    return out


def random_texture(bc, S, fmt, w, h, seed):
    return S.BlockTexture(random_blocks(bc, fmt, bc.block_count(w, h), seed), w, h, fmt)


QUAD = [(-0.8, -0.8, 1.0), (0.8, -0.8, 1.0), (0.8, 0.8, 1.0), (-0.8, 0.8, 1.0)]
CORNERS = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float64)
UV0, UV1 = (-1.5, 4.0), (-0.7, 2.3)                  # offset, scale: coordinates over [-1.5, 2.5] and [-0.7, 1.6]: WRAP crosses block and image edges


def quad_scene(S, mat, textures, env=(0.1, 0.2, 0.3, 1.0), tangent=(0.8, 0.6, 0.0), z=1.0, extra=()):
    """A camera-facing quad at z seen from the origin in front of a constant environment. textures: slot -> (texture, coordinate set);
    extra: further panes (quad z, material, textures, yaw in degrees about the y axis)."""
    def mesh(zq, m, tex):
        pos = np.array(QUAD, np.float32); pos[:, 2] = zq
        vb = S.make_vertices(pos, np.tile((0, 0, -1), (4, 1)), UV0[0] + CORNERS * UV0[1], np.tile(tangent, (4, 1)), UV1[0] + CORNERS * UV1[1])
        return S.Mesh(vb, S.make_indices([0, 1, 2, 0, 2, 3]), True, m, has_tangents=True, has_uv=(True, True), textures=dict(tex))
    nodes = [S.MeshNode([mesh(z, mat, textures)])] + [S.MeshNode([mesh(*e[:3])]) for e in extra]
    objects = [S.RenderObject(0, S.trs())] + [S.RenderObject(i + 1, S.trs(yaw_deg=e[3])) for i, e in enumerate(extra)]
    cam = S.make_camera((0, 0, 0), hfov_deg=90.0, aspect=1.0)
    return S.Scene(nodes, objects, cam, S.make_scene_data(env)).finalize()


def swap_textures(bc, scene, fn):
    return bc.map_textures(scene, lambda slot, tex: fn(tex))


def dds_gltf(I, S, bc, directory, unsupported=False):
    """A quad whose base-colour, metallic-roughness and normal textures each reference a PNG and, through MSFT_texture_dds, a DDS file
    (BC3 / BC1 / BC5, UNORM headers). unsupported: the base-colour DDS carries a BC7 header instead. Returns (scene json path, the
    block textures by slot as the DDS files hold them)."""
    rng = np.random.default_rng(5)
    png = {k: S.Texture(rng.integers(0, 256, (12, 20, 4)).astype(np.uint8), srgb=(k == "BaseColor")) for k in ("BaseColor", "MetallicRoughness", "Normal")}
    mat = S.material((1, 1, 1), metallic=1.0, roughness=1.0)
    scene = quad_scene(S, mat, {k: (t, 0) for k, t in png.items()}, tangent=(1, 0, 0))
    path = I.export_scene(scene, directory, "ddsquad")
    gpath = os.path.join(directory, "ddsquad_node0.gltf")
    g = json.load(open(gpath))
    fmts = {"BaseColor": S.FMT_BC3_UNORM, "MetallicRoughness": S.FMT_BC1_UNORM, "Normal": S.FMT_BC5_UNORM}
    m = g["materials"][0]
    index = {"BaseColor": m["pbrMetallicRoughness"]["baseColorTexture"]["index"], "MetallicRoughness": m["pbrMetallicRoughness"]["metallicRoughnessTexture"]["index"],
             "Normal": m["normalTexture"]["index"]}
    blocks = {}
    for slot, fmt in fmts.items():
        bt = random_texture(bc, S, fmt, 20, 12, 40 + fmt)
        data = bc.write_dds(bt.data, fmt, 20, 12, header="dx10" if slot != "MetallicRoughness" else "legacy", mip_count=3 if slot == "Normal" else 1)
        if unsupported and slot == "BaseColor":
            data = data[:128] + np.uint32(98).tobytes() + data[132:]          # DXGI_FORMAT_BC7_UNORM
        name = slot + ".dds"
        open(os.path.join(directory, name), "wb").write(data)
        g["images"].append({"uri": name} if slot != "Normal" else {"uri": "normal.bin", "mimeType": "image/vnd-ms.dds"})
        if slot == "Normal":
            os.replace(os.path.join(directory, name), os.path.join(directory, "normal.bin"))
        g["textures"][index[slot]]["extensions"] = {"MSFT_texture_dds": {"source": len(g["images"]) - 1}}
        blocks[slot] = bt
    g.setdefault("extensionsUsed", []).append("MSFT_texture_dds")
    json.dump(g, open(gpath, "w"))
    return path, blocks
