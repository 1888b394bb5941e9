"""Block-compressed textures, the rules (no GPU): the decode arithmetic of DESIGN.md "Arithmetic spec" on hand-derived blocks, the layout
against Pillow's DDS decoder, the device's copy of the arithmetic (csrc/pt_bc.hpp, compiled for the host under sanitizers) against bc.py
bit for bit, the DDS container, and both hosts' glTF ingest of MSFT_texture_dds images."""
import io
import json
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as ge
import bcscene

DEMO = os.path.join(ge.PKG_DIR, "pt_demo")
SIZES = [(1, 1), (3, 5), (4, 4), (10, 7), (12, 20)]                     # (w, h)
N_RANDOM = 4096


@pytest.fixture(scope="module")
def bc(pkg):
    import dxpbrt_amd.bc as m
    return m


def all_formats(S):
    return (S.FMT_BC1_UNORM, S.FMT_BC1_UNORM_SRGB, S.FMT_BC3_UNORM, S.FMT_BC3_UNORM_SRGB, S.FMT_BC4_UNORM, S.FMT_BC5_UNORM)


def color_block(c0, c1, indices):
    return np.frombuffer(struct.pack("<HHI", c0, c1, sum(k << (2 * i) for i, k in enumerate(indices))), np.uint8)


def alpha_block(a0, a1, indices):
    bits = sum(k << (3 * i) for i, k in enumerate(indices))
    return np.frombuffer(bytes([a0, a1]) + bits.to_bytes(6, "little"), np.uint8)


def round_f32(q):
    """the correctly rounded float32 of a Fraction, found exactly"""
    f = np.float32(float(q))
    cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    err = [abs(Fraction(float(c)) - q) for c in cands]
    assert sorted(err)[0] < sorted(err)[1]                                # no tie
    return cands[int(np.argmin(err))]


# ---------------------------------------------------------------------- hand-derived blocks
def test_bc1_four_colour_block(bc, pkg):
    S = pkg.scenes
    assert struct.pack("<I", 0xE4E4E4E4) == bytes(color_block(0, 0, [0, 1, 2, 3] * 4)[4:])       # every row holds the indices 0 1 2 3
    img = bc.decode(color_block(0xFFFF, 0x0000, [0, 1, 2, 3] * 4)[None], S.FMT_BC1_UNORM, 4, 4)
    assert img.dtype == np.uint8 and img.shape == (4, 4, 4)
    for y in range(4):
        assert img[y, :, 0].tolist() == [255, 0, 170, 85] and img[y, :, 1].tolist() == [255, 0, 170, 85] and img[y, :, 2].tolist() == [255, 0, 170, 85]
        assert img[y, :, 3].tolist() == [255, 255, 255, 255]


def test_bc1_three_colour_block_has_a_transparent_index(bc, pkg):
    S = pkg.scenes
    img = bc.decode(color_block(0x0000, 0xFFFF, [0, 1, 2, 3] * 4)[None], S.FMT_BC1_UNORM_SRGB, 4, 4)
    for y in range(4):
        assert img[y, :, 0].tolist() == [0, 255, 128, 0] and img[y, :, 2].tolist() == [0, 255, 128, 0]
        assert img[y, :, 3].tolist() == [255, 255, 255, 0]
    # equal endpoints are c0 <= c1: three-colour mode
    img = bc.decode(color_block(0x8410, 0x8410, [3] * 16)[None], S.FMT_BC1_UNORM, 4, 4)
    assert (img == 0).all()
    # the colour half of BC3 is four-colour whatever the order: index 3 is (e0 + 2 e1 + 1) / 3 = (0 + 510 + 1) / 3 = 170, alpha from its own block
    b3 = np.concatenate([alpha_block(9, 9, [0] * 16), color_block(0x0000, 0xFFFF, [0, 1, 2, 3] * 4)])
    img = bc.decode(b3[None], S.FMT_BC3_UNORM, 4, 4)
    assert img[0, :, 0].tolist() == [0, 255, 85, 170] and (img[..., 3] == 9).all()


def test_endpoints_expand_by_bit_replication(bc, pkg):
    S = pkg.scenes
    img = bc.decode(color_block(1 << 11, 1 << 5, [0, 1] * 8)[None], S.FMT_BC1_UNORM, 4, 4)       # r5 = 1 ; g6 = 1
    assert img[0, 0].tolist() == [8, 0, 0, 255] and img[0, 1].tolist() == [0, 4, 0, 255]
    img = bc.decode(color_block((30 << 11) | (33 << 5) | 17, 0, [0] * 16)[None], S.FMT_BC1_UNORM, 4, 4)
    assert img[0, 0].tolist() == [(30 << 3) | (30 >> 2), (33 << 2) | (33 >> 4), (17 << 3) | (17 >> 2), 255] == [247, 134, 140, 255]


def test_bc3_alpha_block_both_modes(bc, pkg):
    S = pkg.scenes
    col = color_block(0xFFFF, 0xFFFF, [0] * 16)
    order = [0, 1, 2, 3, 4, 5, 6, 7] * 2
    img = bc.decode(np.concatenate([alpha_block(255, 0, order), col])[None], S.FMT_BC3_UNORM, 4, 4)
    assert img[0, :, 3].tolist() + img[1, :, 3].tolist() == [255, 0, 219, 182, 146, 109, 73, 36]
    assert img[2, :, 3].tolist() + img[3, :, 3].tolist() == [255, 0, 219, 182, 146, 109, 73, 36]
    assert (img[..., :3] == 255).all()
    img = bc.decode(np.concatenate([alpha_block(0, 255, order), col])[None], S.FMT_BC3_UNORM_SRGB, 4, 4)       # six-value mode
    assert img[0, :, 3].tolist() + img[1, :, 3].tolist() == [0, 255, 51, 102, 153, 204, 0, 255]
    img = bc.decode(np.concatenate([alpha_block(100, 200, order), col])[None], S.FMT_BC3_UNORM, 4, 4)
    assert img[0, :, 3].tolist() + img[1, :, 3].tolist() == [100, 200, 120, 140, 160, 180, 0, 255]


def test_bc4_values_are_correctly_rounded_fp32_and_bc5_channel_order(bc, pkg):
    S = pkg.scenes
    order = [0, 1, 2, 3, 4, 5, 6, 7] * 2
    img = bc.decode(alpha_block(200, 10, order)[None], S.FMT_BC4_UNORM, 4, 4)
    assert img.dtype == np.float32 and img.shape == (4, 4, 4)
    want = [Fraction(200, 255), Fraction(10, 255)] + [Fraction((8 - k) * 200 + (k - 1) * 10, 1785) for k in range(2, 8)]
    got = img[0, :, 0].tolist() + img[1, :, 0].tolist()
    assert [np.float32(g).view(np.uint32) for g in got] == [round_f32(q).view(np.uint32) for q in want]
    assert (img[..., 1] == 0).all() and (img[..., 2] == 0).all() and (img[..., 3] == 1).all()
    img = bc.decode(alpha_block(10, 200, order)[None], S.FMT_BC4_UNORM, 4, 4)                                     # six-value mode
    want = [Fraction(10, 255), Fraction(200, 255)] + [Fraction((6 - k) * 10 + (k - 1) * 200, 1275) for k in range(2, 6)] + [Fraction(0), Fraction(1)]
    got = img[0, :, 0].tolist() + img[1, :, 0].tolist()
    assert [np.float32(g).view(np.uint32) for g in got] == [round_f32(q).view(np.uint32) for q in want]
    # BC5: red in bytes 0..7, green in 8..15
    img = bc.decode(np.concatenate([alpha_block(255, 0, [0] * 16), alpha_block(255, 0, [1] * 16)])[None], S.FMT_BC5_UNORM, 4, 4)
    assert (img[..., 0] == 1).all() and (img[..., 1] == 0).all() and (img[..., 2] == 0).all() and (img[..., 3] == 1).all()
    img = bc.decode(np.concatenate([alpha_block(51, 0, [0] * 16), alpha_block(102, 0, [0] * 16)])[None], S.FMT_BC5_UNORM, 4, 4)
    assert img[0, 0, 0] == np.float32(0.2) and img[0, 0, 1] == np.float32(0.4)


def test_constant_division_is_the_correctly_rounded_quotient():
    """(float)((double)num * (1.0 / (double)c)), the form the device evaluates, for every numerator of both BC4 modes"""
    for c in (1785, 1275):
        num = np.arange(c + 1, dtype=np.int64)
        got = (num.astype(np.float64) * (1.0 / float(c))).astype(np.float32)
        want = np.array([round_f32(Fraction(int(n), c)) for n in num], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), c
        assert got[0] == 0.0 and got[-1] == 1.0


# ---------------------------------------------------------------------- layout against Pillow
def pillow_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im.mode, np.asarray(im)


@pytest.mark.parametrize("which", ["BC1", "BC3", "BC4", "BC5"])
def test_layout_agrees_with_pillow(bc, pkg, which):
    S = pkg.scenes
    fmt = {"BC1": S.FMT_BC1_UNORM, "BC3": S.FMT_BC3_UNORM, "BC4": S.FMT_BC4_UNORM, "BC5": S.FMT_BC5_UNORM}[which]
    blocks = bcscene.random_blocks(bc, fmt, N_RANDOM, 100 + fmt)
    for name, f in bcscene.mode_fractions(bc, blocks, fmt).items():       # a condition on the inputs: both modes of every switch are there
        assert 0.25 <= f <= 0.75, (name, f)
    w = h = 256                                                           # 64 x 64 blocks
    ours = bc.decode(blocks, fmt, w, h)
    mode, theirs = pillow_decode(bc.write_dds(blocks, fmt, w, h, header="dx10"))
    b = blocks.astype(np.int64)
    tiles = lambda per_block: bc._untile(per_block, w, h)                 # noqa: E731  per-block index arrays in image order
    if which in ("BC1", "BC3"):
        assert mode == "RGBA" and theirs.shape == ours.shape
        d = np.abs(ours.astype(np.int64) - theirs.astype(np.int64))
        assert d.max() <= 1
        col = blocks if which == "BC1" else blocks[:, 8:]
        k = tiles(bc._color_indices(col[:, 4:8])[:, :, None])[..., 0]
        assert (d[..., :3][k <= 1] == 0).all()                            # an endpoint index: exact
        if which == "BC1":
            assert np.array_equal(ours[..., 3], theirs[..., 3]) and (ours[..., 3] == 0).any() and (ours[..., 3] == 255).any()
        else:
            ka = tiles(bc._alpha_indices(blocks[:, 2:8])[:, :, None])[..., 0]
            six = tiles(np.repeat((b[:, 0] <= b[:, 1])[:, None, None], 16, 1))[..., 0]
            assert (d[..., 3][(ka <= 1) | (six & (ka >= 6))] == 0).all()
    else:
        nch = 1 if which == "BC4" else 2
        theirs = theirs.reshape(h, w, -1).astype(np.float64)
        for c in range(nch):
            half = blocks[:, 8 * c: 8 * c + 8]
            d = np.abs(ours[..., c].astype(np.float64) - theirs[..., c] / 255.0)
            assert d.max() <= 1.0 / 255.0
            ka = tiles(bc._alpha_indices(half[:, 2:8])[:, :, None])[..., 0]
            six = tiles(np.repeat((half[:, 0] <= half[:, 1])[:, None, None], 16, 1))[..., 0]
            exact = (ka <= 1) | (six & (ka >= 6))
            assert np.array_equal(ours[..., c][exact], (theirs[..., c][exact] / 255.0).astype(np.float32))
        assert (ours[..., nch:3] == 0).all() and (ours[..., 3] == 1).all()


# ---------------------------------------------------------------------- sizes
@pytest.mark.parametrize("w,h", SIZES)
def test_block_count_and_untiling(bc, pkg, w, h):
    S = pkg.scenes
    for fmt in all_formats(S):
        n = ((w + 3) // 4) * ((h + 3) // 4)
        assert bc.block_count(w, h) == n
        blocks = bcscene.random_blocks(bc, fmt, n, 7 * w + h + fmt)
        img = bc.decode(blocks, fmt, w, h)
        assert img.shape == (h, w, 4)
        bw = (w + 3) // 4
        for y in range(h):
            for x in range(w):                                            # texel (x, y) is texel (x & 3, y & 3) of block (y / 4) bw + x / 4, decoded alone
                one = bc.decode(blocks[(y // 4) * bw + x // 4][None], fmt, 4, 4)
                assert np.array_equal(img[y, x], one[y & 3, x & 3]), (fmt, x, y)
        with pytest.raises(ValueError):
            bc.decode(blocks[:-1] if n > 1 else np.zeros((0, blocks.shape[1]), np.uint8), fmt, w, h)


def test_encoder_round_trip_is_close(bc, pkg):
    S = pkg.scenes
    y, x = np.mgrid[0:20, 0:12]
    img = np.stack([8 * x + 20, 5 * y + 40, 3 * (x + y) + 30, np.where((x // 4 + y // 4) % 2 == 0, 255, 0)], -1).astype(np.uint8)
    for fmt in all_formats(S):
        blocks = bc.encode(img, fmt)
        assert blocks.shape == (15, S.FMT_BLOCK_BYTES[fmt]) and blocks.dtype == np.uint8
        out = bc.decode(blocks, fmt, 12, 20)
        if fmt in bc.BC1_FORMATS:
            assert np.array_equal(out[..., 3], img[..., 3])               # three-colour mode where a block has alpha < 128
            opaque = img[..., 3] == 255
            assert np.abs(out[..., :3].astype(int) - img[..., :3].astype(int))[opaque].max() <= 24
            assert bcscene.mode_fractions(bc, blocks, fmt)["c0>c1"] < 1.0
        elif fmt in bc.BC3_FORMATS:
            assert np.abs(out.astype(int) - img.astype(int)).max() <= 24
        else:
            nch = 1 if fmt == S.FMT_BC4_UNORM else 2
            assert np.abs(out[..., :nch] * 255.0 - img[..., :nch]).max() <= 4


# ---------------------------------------------------------------------- the device's arithmetic on the host
@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bc_host") / "bc_decode")
    src = os.path.join(os.path.dirname(__file__), "host", "bc_decode.cpp")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    return exe


def test_device_arithmetic_on_the_host_equals_bc_py_bit_for_bit(bc, pkg, host_decoder, tmp_path):
    """csrc/pt_bc.hpp (what texel_fetch calls after its load) as a stand-alone host program under AddressSanitizer and UBSan: the random
    block streams and the size cases, every texel compared with bc.decode as bytes."""
    S = pkg.scenes
    records = []
    for fmt in all_formats(S):
        records.append((fmt, 256, 256, bcscene.random_blocks(bc, fmt, N_RANDOM, 100 + fmt)))
        for (w, h) in SIZES:
            records.append((fmt, w, h, bcscene.random_blocks(bc, fmt, bc.block_count(w, h), 7 * w + h + fmt)))
    # every endpoint pair of the alpha layout with every index: all numerators of both modes
    a0, a1 = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    grid = np.zeros((256 * 256, 8), np.uint8)
    grid[:, 0], grid[:, 1] = a0.reshape(-1), a1.reshape(-1)
    grid[:, 2:8] = np.frombuffer(sum(k << (3 * i) for i, k in enumerate([0, 1, 2, 3, 4, 5, 6, 7] * 2)).to_bytes(6, "little"), np.uint8)
    records.append((S.FMT_BC4_UNORM, 1024, 1024, grid))
    records.append((S.FMT_BC3_UNORM, 1024, 1024, np.concatenate([grid, bcscene.random_blocks(bc, S.FMT_BC1_UNORM, len(grid), 3)], 1)))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for fmt, w, h, blocks in records:
            f.write(struct.pack("<3I", fmt, w, h)); f.write(np.ascontiguousarray(blocks).tobytes())
    p = subprocess.run([host_decoder, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-2000:]
    raw = open(fout, "rb").read()
    off = 0
    for fmt, w, h, blocks in records:
        want = bc.decode(blocks, fmt, w, h).tobytes()
        assert raw[off:off + len(want)] == want, (fmt, w, h)
        off += len(want)
    assert off == len(raw)


# ---------------------------------------------------------------------- DDS container
def test_dds_round_trips_for_every_accepted_header(bc, pkg):
    S = pkg.scenes
    w, h = 10, 7
    forms = [(fmt, "dx10") for fmt in all_formats(S)] + [(S.FMT_BC1_UNORM, "legacy"), (S.FMT_BC3_UNORM, "legacy"), (S.FMT_BC4_UNORM, "legacy"),
             (S.FMT_BC4_UNORM, "legacy:BC4U"), (S.FMT_BC5_UNORM, "legacy"), (S.FMT_BC5_UNORM, "legacy:BC5U")]
    for fmt, header in forms:
        blocks = bcscene.random_blocks(bc, fmt, bc.block_count(w, h), fmt)
        for mips in (1, 3):
            data = bc.write_dds(blocks, fmt, w, h, header=header, mip_count=mips)
            assert bc.is_dds(data)
            got = bc.read_dds(data)
            assert (got.fmt, got.width, got.height) == (fmt, w, h) and np.array_equal(got.data, blocks), (fmt, header, mips)
    texels = np.random.default_rng(1).integers(0, 256, (h, w, 4)).astype(np.uint8)
    for fmt, header in ((S.FMT_RGBA8_UNORM, "dx10"), (S.FMT_RGBA8_UNORM_SRGB, "dx10"), (S.FMT_RGBA8_UNORM, "legacy")):
        got = bc.read_dds(bc.write_dds(texels, fmt, w, h, header=header, mip_count=2))
        assert (got.fmt, got.width, got.height) == (fmt, w, h) and np.array_equal(got.data, texels)


def test_dds_reader_refuses_what_it_does_not_load(bc, pkg):
    S = pkg.scenes
    w, h = 12, 20
    blocks = bcscene.random_blocks(bc, S.FMT_BC3_UNORM, bc.block_count(w, h), 1)
    good = bc.write_dds(blocks, S.FMT_BC3_UNORM, w, h)
    bc.read_dds(good)

    def patched(data, off, value):
        return data[:off] + struct.pack("<I", value) + data[off + 4:]
    cases = {
        "truncated": good[:-1],
        "truncated header": good[:100],
        "truncated dx10 header": good[:140],
        "mip count overruns the file": patched(patched(good, 28, 4), 8, struct.unpack_from("<I", good, 8)[0] | 0x20000),
        "absurd mip count": patched(patched(good, 28, 40), 8, struct.unpack_from("<I", good, 8)[0] | 0x20000),
        "zero width": patched(good, 16, 0),
        "zero height": patched(good, 12, 0),
        "BC2": patched(good, 128, 74),
        "BC6H": patched(good, 128, 95),
        "BC7": patched(good, 128, 98),
        "BC4 SNORM": patched(good, 128, 81),
        "BC1 typeless": patched(good, 128, 70),
        "volume (dx10)": patched(good, 132, 4),
        "volume (caps2)": patched(patched(patched(good, 112, 0x200000), 24, 4), 8, struct.unpack_from("<I", good, 8)[0] | 0x800000),
        "array": patched(good, 140, 6),
        "cube": patched(good, 136, 4),
        "no magic": b"DDX " + good[4:],
        "width beyond the file": patched(good, 16, 4096),
    }
    legacy = bc.write_dds(blocks, S.FMT_BC3_UNORM, w, h, header="legacy")
    cases["DXT3"] = legacy[:84] + b"DXT3" + legacy[88:]
    for name, data in cases.items():
        with pytest.raises(ValueError):
            bc.read_dds(data)
            pytest.fail(name + " was accepted")


# ---------------------------------------------------------------------- ingest: both hosts
def walk_dump(dump, info, scene):
    """the texture entries of a pt_demo --dump-scene file: [(slot, w, h, srgb, coordinate set, format or None, bytes)] per mesh, in order"""
    raw = open(dump, "rb").read()
    off, out = 0, []
    for n, node in enumerate(scene.nodes):
        for m, mesh in enumerate(node.meshes):
            meta = info["nodes"][n][m]
            off += mesh.vertices.nbytes + mesh.indices.nbytes + 64
            entries = []
            for e in meta["textures"]:
                fmt = e[5] if len(e) > 5 else None
                nb = ((e[1] + 3) // 4) * ((e[2] + 3) // 4) * (16 if fmt in (5, 6, 8) else 8) if fmt is not None else e[1] * e[2] * 4
                entries.append((e[0], e[1], e[2], e[3], e[4], fmt, raw[off:off + nb])); off += nb
            out.append(entries)
    return out


def test_ingest_prefers_the_dds_image_and_forces_srgb_on_base_colour(bc, pkg, tmp_path):
    import dxpbrt_amd.ingest as I
    S = pkg.scenes
    path, blocks = bcscene.dds_gltf(I, S, bc, str(tmp_path))
    scene = I.load_scene(path, aspect=1.0)
    mesh = scene.nodes[0].meshes[0]
    assert set(mesh.textures) == {"BaseColor", "MetallicRoughness", "Normal"} and not mesh.skipped_textures
    want_fmt = {"BaseColor": S.FMT_BC3_UNORM_SRGB, "MetallicRoughness": S.FMT_BC1_UNORM, "Normal": S.FMT_BC5_UNORM}     # forceSRGB on base colour only
    for slot, (tex, uvi) in mesh.textures.items():
        assert isinstance(tex, S.BlockTexture) and (tex.width, tex.height, tex.fmt, uvi) == (20, 12, want_fmt[slot], 0), slot
        assert np.array_equal(tex.data, blocks[slot].data), slot
    heap_fmts = sorted(item.fmt for item in scene.heap if item.kind == S.KIND_TEXTURE2D)
    assert heap_fmts == sorted(want_fmt.values())
    # the C++ host: the same block bytes, sizes and formats
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    dump = str(tmp_path / "dump.bin")
    p = subprocess.run([DEMO, "--scene", path, "--dump-scene", dump], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    assert "not loaded" not in p.stderr
    entries = walk_dump(dump, json.loads(p.stdout), scene)[0]
    assert sorted(e[0] for e in entries) == sorted(S.TEX_SLOTS.index(s) for s in want_fmt)
    for slot_index, w, h, srgb, tc, fmt, data in entries:
        slot = S.TEX_SLOTS[slot_index]
        assert (w, h, fmt, tc) == (20, 12, want_fmt[slot], 0) and bool(srgb) == (slot == "BaseColor"), slot
        assert data == np.ascontiguousarray(mesh.textures[slot][0].data).tobytes(), slot


def test_an_unsupported_dds_is_listed_and_skipped_by_both_hosts(bc, pkg, tmp_path):
    import dxpbrt_amd.ingest as I
    S = pkg.scenes
    path, _ = bcscene.dds_gltf(I, S, bc, str(tmp_path), unsupported=True)
    scene = I.load_scene(path, aspect=1.0)
    mesh = scene.nodes[0].meshes[0]
    assert mesh.skipped_textures == ["BaseColor"] and set(mesh.textures) == {"MetallicRoughness", "Normal"}
    assert os.path.exists(DEMO), "pt_demo is not built: run __graft_entry__.build()"
    p = subprocess.run([DEMO, "--scene", path, "--dump-scene", str(tmp_path / "dump.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    assert "BaseColor texture of a material not loaded" in p.stderr
    assert sorted(e[0] for e in json.loads(p.stdout)["nodes"][0][0]["textures"]) == sorted(S.TEX_SLOTS.index(s) for s in mesh.textures)
