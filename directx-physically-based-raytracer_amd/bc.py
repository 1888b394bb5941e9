"""Block-compressed textures (BC1, BC3, BC4, BC5) on the harness side: the decode rules of DESIGN.md "Arithmetic spec" in numpy, a
simple range-fit encoder, and a DDS container reader / writer (mip 0).

  decode(blocks, fmt, w, h)   the expansion the device samples to the bits of: uint8 [h, w, 4] for BC1 / BC3 (an RGBA8(_SRGB) texture),
                              float32 [h, w, 4] for BC4 (r, 0, 0, 1) and BC5 (r, g, 0, 1) (an R32G32B32A32_FLOAT texture)
  encode(image, fmt)          per-block min / max endpoints and the nearest index; no quality claim beyond decode(encode(x)) ~ x
  read_dds / write_dds        DX10 headers (DXGI 28, 29, 71, 72, 77, 78, 80, 83), the legacy FourCCs DXT1, DXT5, ATI1 / BC4U, ATI2 / BC5U and
                              legacy 32-bit RGBA masks; everything else (BC2, BC6H, BC7, SNORM, typeless, volumes, arrays, cubes) raises

Block layout (csrc/pt_bc.hpp is the device's copy of the same arithmetic): texel (x, y) of a block is i = 4 (y & 3) + (x & 3); blocks are
row-major, ceil(w / 4) per row, tightly packed; texels of an edge block beyond the image are ignored.
"""
import struct
from collections import namedtuple

import numpy as np

from .scenes import (FMT_RGBA8_UNORM, FMT_RGBA8_UNORM_SRGB, FMT_BC1_UNORM, FMT_BC1_UNORM_SRGB, FMT_BC3_UNORM, FMT_BC3_UNORM_SRGB,
                     FMT_BC4_UNORM, FMT_BC5_UNORM, FMT_BLOCK_BYTES)

BC1_FORMATS = (FMT_BC1_UNORM, FMT_BC1_UNORM_SRGB)
BC3_FORMATS = (FMT_BC3_UNORM, FMT_BC3_UNORM_SRGB)
SRGB_OF = {FMT_RGBA8_UNORM: FMT_RGBA8_UNORM_SRGB, FMT_BC1_UNORM: FMT_BC1_UNORM_SRGB, FMT_BC3_UNORM: FMT_BC3_UNORM_SRGB}   # forceSRGB


def block_count(w, h):
    return ((w + 3) // 4) * ((h + 3) // 4)


# ----------------------------------------------------------------------------------------------
# palettes
# ----------------------------------------------------------------------------------------------
def _expand565(c):
    r5, g6, b5 = (c >> 11) & 31, (c >> 5) & 63, c & 31
    return np.stack([(r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2)], -1)        # bit replication


def color_palette(c0, c1, bc1):
    """[n, 4, 4] RGBA codes of the four indices. Four-colour mode: BC1 with c0 > c1, BC3 always; three-colour mode: BC1 with c0 <= c1,
    whose index 3 is transparent black."""
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    e0, e1 = _expand565(c0), _expand565(c1)
    four = (c0 > c1) if bc1 else np.ones(c0.shape, bool)
    f = four[:, None]
    p2 = np.where(f, (2 * e0 + e1 + 1) // 3, (e0 + e1 + 1) >> 1)         # thirds: the exact rational rounded to nearest, no ties
    p3 = np.where(f, (e0 + 2 * e1 + 1) // 3, 0)
    pal = np.zeros((len(c0), 4, 4), np.int64)
    pal[:, 0, :3], pal[:, 1, :3], pal[:, 2, :3], pal[:, 3, :3] = e0, e1, p2, p3
    pal[:, :, 3] = 255
    pal[:, 3, 3] = np.where(four, 255, 0)
    return pal


def alpha_palette(a0, a1):
    """The eight codes of an alpha-layout block as numerators: (num [n, 8], den [n], fixed [n, 8]). Eight-value mode (a0 > a1): den = 7,
    a0 -> 7 a0, a1 -> 7 a1, k = 2..7 -> (8 - k) a0 + (k - 1) a1. Six-value mode: den = 5, k = 2..5 -> (6 - k) a0 + (k - 1) a1, codes 6 and
    7 are the constants 0 and 1 (fixed = 0 / 1, elsewhere -1)."""
    a0, a1 = np.asarray(a0, np.int64)[:, None], np.asarray(a1, np.int64)[:, None]
    k = np.arange(8, dtype=np.int64)[None, :]
    den = np.where(a0 > a1, 7, 5)
    num = np.where(k == 0, a0 * den, np.where(k == 1, a1 * den, (den + 1 - k) * a0 + (k - 1) * a1))
    fixed = np.where((den == 5) & (k >= 6), k - 6, -1)
    return np.where(fixed >= 0, 0, num), den[:, 0], fixed


def _alpha_codes8(num, den, fixed):
    """BC3 alpha: 8-bit codes, integer division to nearest (sevenths and fifths never tie)"""
    d = den[:, None]
    return np.where(fixed >= 0, fixed * 255, (num + d // 2) // d)


def _bc4_values(num, den, fixed):
    """BC4 / BC5: the correctly rounded fp32 of num / (255 den), evaluated as the device does: in double, times the rounded reciprocal"""
    recip = np.where(den == 7, 1.0 / 1785.0, 1.0 / 1275.0)[:, None]
    v = (num.astype(np.float64) * recip).astype(np.float32)
    return np.where(fixed >= 0, fixed.astype(np.float32), v).astype(np.float32)


def _color_indices(b4):
    word = b4[:, 0].astype(np.uint32) | (b4[:, 1].astype(np.uint32) << 8) | (b4[:, 2].astype(np.uint32) << 16) | (b4[:, 3].astype(np.uint32) << 24)
    return ((word[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).astype(np.int64)


def _alpha_indices(b6):
    bits = np.zeros(len(b6), np.uint64)
    for j in range(6):
        bits |= b6[:, j].astype(np.uint64) << np.uint64(8 * j)
    return ((bits[:, None] >> (3 * np.arange(16, dtype=np.uint64))[None, :]) & np.uint64(7)).astype(np.int64)


def _u16(b2):
    return b2[:, 0].astype(np.int64) | (b2[:, 1].astype(np.int64) << 8)


def _untile(per_block, w, h):
    """[n, 16, C] per-block texels -> [h, w, C]"""
    bw, bh = (w + 3) // 4, (h + 3) // 4
    c = per_block.shape[-1]
    return np.ascontiguousarray(per_block.reshape(bh, bw, 4, 4, c).transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, c)[:h, :w])


def _tile(image):
    """[h, w, C] -> [n, 16, C], the image padded to whole blocks by repeating its last row / column"""
    h, w, c = image.shape
    bw, bh = (w + 3) // 4, (h + 3) // 4
    p = np.pad(image, ((0, bh * 4 - h), (0, bw * 4 - w), (0, 0)), mode="edge")
    return p.reshape(bh, 4, bw, 4, c).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, c)


def _check_blocks(blocks, fmt, w, h):
    if fmt not in FMT_BLOCK_BYTES:
        raise ValueError(f"format {fmt} is not block-compressed")
    if w < 1 or h < 1:
        raise ValueError("texture size is zero")
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, FMT_BLOCK_BYTES[fmt])
    if len(b) != block_count(w, h):
        raise ValueError(f"{w}x{h} needs {block_count(w, h)} blocks, got {len(b)}")
    return b


def decode(blocks, fmt, w, h):
    b = _check_blocks(blocks, fmt, w, h)
    if fmt in BC1_FORMATS or fmt in BC3_FORMATS:
        col = b if fmt in BC1_FORMATS else b[:, 8:]
        pal = color_palette(_u16(col[:, 0:2]), _u16(col[:, 2:4]), fmt in BC1_FORMATS)
        texels = np.take_along_axis(pal, _color_indices(col[:, 4:8])[:, :, None], 1)                   # [n, 16, 4]
        if fmt in BC3_FORMATS:
            codes = _alpha_codes8(*alpha_palette(b[:, 0], b[:, 1]))
            texels[:, :, 3] = np.take_along_axis(codes, _alpha_indices(b[:, 2:8]), 1)
        return _untile(texels.astype(np.uint8), w, h)
    out = np.zeros((len(b), 16, 4), np.float32)
    out[:, :, 3] = 1.0
    for c in range(1 if fmt == FMT_BC4_UNORM else 2):
        half = b[:, 8 * c: 8 * c + 8]
        out[:, :, c] = np.take_along_axis(_bc4_values(*alpha_palette(half[:, 0], half[:, 1])), _alpha_indices(half[:, 2:8]), 1)
    return _untile(out, w, h)


# ----------------------------------------------------------------------------------------------
# encoder: range fit
# ----------------------------------------------------------------------------------------------
def _encode_alpha_blocks(v):
    """v: [n, 16] codes 0..255 -> [n, 8] bytes: a0 = max, a1 = min (eight-value mode; a constant block lands in six-value mode, whose
    first six codes are that constant), the nearest of the eight codes per texel"""
    v = v.astype(np.int64)
    a0, a1 = v.max(1), v.min(1)
    num, den, fixed = alpha_palette(a0, a1)
    pal = np.where(fixed >= 0, fixed * 255.0, num / den[:, None].astype(np.float64))
    idx = np.abs(v[:, :, None] - pal[:, None, :]).argmin(2).astype(np.uint64)
    bits = (idx << (3 * np.arange(16, dtype=np.uint64))[None, :]).sum(1, dtype=np.uint64)
    out = np.zeros((len(v), 8), np.uint8)
    out[:, 0], out[:, 1] = a0, a1
    for j in range(6):
        out[:, 2 + j] = ((bits >> np.uint64(8 * j)) & np.uint64(0xFF)).astype(np.uint8)
    return out


def _encode_color_blocks(t, bc1):
    """t: [n, 16, 4] RGBA codes -> [n, 8] bytes. Endpoints: the per-channel max and min of the block in R5G6B5. BC1: a block with a
    texel of alpha < 128 is written in three-colour mode (c0 <= c1), those texels get index 3."""
    t = t.astype(np.int64)

    def q565(e):
        r, g, b = (e[:, 0] * 31 + 127) // 255, (e[:, 1] * 63 + 127) // 255, (e[:, 2] * 31 + 127) // 255
        return (r << 11) | (g << 5) | b
    hi, lo = q565(t[:, :, :3].max(1)), q565(t[:, :, :3].min(1))
    clear = t[:, :, 3] < 128 if bc1 else np.zeros(t.shape[:2], bool)
    three = clear.any(1)
    c0, c1 = np.where(three, np.minimum(hi, lo), np.maximum(hi, lo)), np.where(three, np.maximum(hi, lo), np.minimum(hi, lo))
    pal = color_palette(c0, c1, bc1)
    d = ((t[:, :, None, :3] - pal[:, None, :, :3]) ** 2).sum(-1).astype(np.float64)
    d = np.where(pal[:, None, :, 3] == 0, np.inf, d)                      # an opaque texel never takes the transparent index
    idx = np.where(clear, 3, d.argmin(2)).astype(np.uint32)
    word = (idx << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(1, dtype=np.uint32)
    out = np.zeros((len(t), 8), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = c0 & 0xFF, c0 >> 8, c1 & 0xFF, c1 >> 8
    for j in range(4):
        out[:, 4 + j] = (word >> np.uint32(8 * j)) & np.uint32(0xFF)
    return out


def encode(image, fmt):
    """image: [h, w, C] uint8 codes (float images in [0, 1] are rounded to codes first); C >= 4 for BC1 / BC3, >= 1 for BC4, >= 2 for BC5.
    Returns the block stream, uint8 [blocks, 8 | 16]."""
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[:, :, None]
    if image.dtype != np.uint8:
        image = np.floor(np.clip(image.astype(np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    if fmt not in FMT_BLOCK_BYTES:
        raise ValueError(f"format {fmt} is not block-compressed")
    t = _tile(image)
    if fmt in BC1_FORMATS:
        return _encode_color_blocks(t[:, :, :4], True)
    if fmt in BC3_FORMATS:
        return np.concatenate([_encode_alpha_blocks(t[:, :, 3]), _encode_color_blocks(t[:, :, :4], False)], 1)
    if fmt == FMT_BC4_UNORM:
        return _encode_alpha_blocks(t[:, :, 0])
    return np.concatenate([_encode_alpha_blocks(t[:, :, 0]), _encode_alpha_blocks(t[:, :, 1])], 1)


# ----------------------------------------------------------------------------------------------
# scenes.Texture <-> scenes.BlockTexture
# ----------------------------------------------------------------------------------------------
def block_texture(tex, fmt):
    """A scenes.Texture of 8-bit texels, encoded"""
    from .scenes import BlockTexture
    h, w = tex.data.shape[:2]
    return BlockTexture(encode(tex.data, fmt), w, h, fmt)


def expansion(bt):
    """The scenes.Texture a block texture samples to the bits of: RGBA8 (sRGB for the _SRGB formats), or float32 for BC4 / BC5"""
    from .scenes import Texture
    return Texture(decode(bt.data, bt.fmt, bt.width, bt.height), srgb=bt.fmt in (FMT_BC1_UNORM_SRGB, FMT_BC3_UNORM_SRGB))


def map_textures(scene, fn):
    """Replace every material texture of a scene by fn(slot, texture) -- once per distinct texture -- and lay the heap out again."""
    done = {}
    for node in scene.nodes:
        for mesh in node.meshes:
            for slot, (tex, uvi) in list((mesh.textures or {}).items()):
                if id(tex) not in done:
                    done[id(tex)] = (tex, fn(slot, tex))                 # (the old texture is kept alive: ids stay unique)
                mesh.textures[slot] = (done[id(tex)][1], uvi)
    return scene.finalize()


# ----------------------------------------------------------------------------------------------
# DDS container, mip 0
# ----------------------------------------------------------------------------------------------
DDSImage = namedtuple("DDSImage", "fmt width height data")        # data: [blocks, 8 | 16] (BC) or [h, w, 4] (RGBA8), uint8

_DXGI = {28: FMT_RGBA8_UNORM, 29: FMT_RGBA8_UNORM_SRGB, 71: FMT_BC1_UNORM, 72: FMT_BC1_UNORM_SRGB, 77: FMT_BC3_UNORM, 78: FMT_BC3_UNORM_SRGB,
         80: FMT_BC4_UNORM, 83: FMT_BC5_UNORM}
_DXGI_OF = {v: k for k, v in _DXGI.items()}
_FOURCC = {b"DXT1": FMT_BC1_UNORM, b"DXT5": FMT_BC3_UNORM, b"ATI1": FMT_BC4_UNORM, b"BC4U": FMT_BC4_UNORM, b"ATI2": FMT_BC5_UNORM, b"BC5U": FMT_BC5_UNORM}
_FOURCC_OF = {FMT_BC1_UNORM: b"DXT1", FMT_BC3_UNORM: b"DXT5", FMT_BC4_UNORM: b"ATI1", FMT_BC5_UNORM: b"ATI2"}
_DXGI_NAMES = {70: "BC1_TYPELESS", 73: "BC2_TYPELESS", 74: "BC2_UNORM", 75: "BC2_UNORM_SRGB", 76: "BC3_TYPELESS", 79: "BC4_TYPELESS", 81: "BC4_SNORM",
               82: "BC5_TYPELESS", 84: "BC5_SNORM", 94: "BC6H_TYPELESS", 95: "BC6H_UF16", 96: "BC6H_SF16", 97: "BC7_TYPELESS", 98: "BC7_UNORM",
               99: "BC7_UNORM_SRGB", 27: "R8G8B8A8_TYPELESS"}
_DDSD_CAPS, _DDSD_HEIGHT, _DDSD_WIDTH, _DDSD_PIXELFORMAT, _DDSD_MIPMAPCOUNT, _DDSD_LINEARSIZE, _DDSD_DEPTH = 0x1, 0x2, 0x4, 0x1000, 0x20000, 0x80000, 0x800000
_DDPF_ALPHAPIXELS, _DDPF_FOURCC, _DDPF_RGB = 0x1, 0x4, 0x40
_CAPS_COMPLEX, _CAPS_TEXTURE, _CAPS_MIPMAP, _CAPS2_CUBEMAP, _CAPS2_VOLUME = 0x8, 0x1000, 0x400000, 0x200, 0x200000
_RGBA_MASKS = (0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000)


def _mip_bytes(fmt, w, h):
    return block_count(w, h) * FMT_BLOCK_BYTES[fmt] if fmt in FMT_BLOCK_BYTES else w * h * 4


def is_dds(data):
    return bytes(data[:4]) == b"DDS "


def read_dds(data):
    """Mip 0 of a 2D DDS texture as a DDSImage. Raises ValueError for a malformed file and for everything outside the accepted formats."""
    data = bytes(data)
    if len(data) < 128 or data[:4] != b"DDS ":
        raise ValueError("DDS: the file is shorter than its header" if data[:4] == b"DDS " else "DDS: no 'DDS ' magic")
    size, flags, height, width, _pitch, depth, mips = struct.unpack_from("<7I", data, 4)
    pf_size, pf_flags, fourcc, bitcount, rm, gm, bm, am = struct.unpack_from("<2I4s5I", data, 76)
    _caps, caps2 = struct.unpack_from("<2I", data, 108)
    if size != 124 or pf_size != 32:
        raise ValueError("DDS: bad header size")
    if width == 0 or height == 0:
        raise ValueError("DDS: zero width or height")
    if width > 65536 or height > 65536:
        raise ValueError("DDS: texture larger than 65536 texels a side")
    if (caps2 & _CAPS2_VOLUME) or ((flags & _DDSD_DEPTH) and depth > 1):
        raise ValueError("DDS: volume textures are not supported")
    if caps2 & _CAPS2_CUBEMAP:
        raise ValueError("DDS: cube maps are not supported")
    off = 128
    if (pf_flags & _DDPF_FOURCC) and fourcc == b"DX10":
        if len(data) < 148:
            raise ValueError("DDS: the file is shorter than its DX10 header")
        dxgi, dimension, misc, array_size, _misc2 = struct.unpack_from("<5I", data, 128)
        off = 148
        if dimension != 3:
            raise ValueError("DDS: only 2D textures are supported" if dimension != 4 else "DDS: volume textures are not supported")
        if misc & 0x4:
            raise ValueError("DDS: cube maps are not supported")
        if array_size > 1:
            raise ValueError("DDS: texture arrays are not supported")
        if dxgi not in _DXGI:
            raise ValueError(f"DDS: unsupported DXGI format {_DXGI_NAMES.get(dxgi, dxgi)}")
        fmt = _DXGI[dxgi]
    elif pf_flags & _DDPF_FOURCC:
        if fourcc not in _FOURCC:
            raise ValueError(f"DDS: unsupported FourCC {fourcc!r}")
        fmt = _FOURCC[fourcc]
    elif (pf_flags & _DDPF_RGB) and bitcount == 32 and (rm, gm, bm) == _RGBA_MASKS[:3] and (am == _RGBA_MASKS[3] and (pf_flags & _DDPF_ALPHAPIXELS)):
        fmt = FMT_RGBA8_UNORM
    else:
        raise ValueError("DDS: unsupported pixel format")
    mips = mips if (flags & _DDSD_MIPMAPCOUNT) and mips > 0 else 1
    if mips > max(width, height).bit_length():
        raise ValueError(f"DDS: {mips} mips for a {width}x{height} texture")
    total = sum(_mip_bytes(fmt, max(1, width >> m), max(1, height >> m)) for m in range(mips))
    if off + total > len(data):
        raise ValueError(f"DDS: the file holds {len(data) - off} bytes of texels, its header asks for {total}")
    n = _mip_bytes(fmt, width, height)                                   # the further mips are skipped
    raw = np.frombuffer(data, np.uint8, n, off).copy()
    if fmt in FMT_BLOCK_BYTES:
        return DDSImage(fmt, width, height, raw.reshape(-1, FMT_BLOCK_BYTES[fmt]))
    return DDSImage(fmt, width, height, raw.reshape(height, width, 4))


def write_dds(data, fmt, width, height, header="dx10", mip_count=1):
    """A DDS file of one texture. header: "dx10", or "legacy" (a FourCC -- "legacy:BC4U" / "legacy:BC5U" / ... name another accepted
    spelling -- or the RGBA masks; the legacy forms have no sRGB variants). mip_count > 1 appends zeroed further mips."""
    data = np.ascontiguousarray(data, np.uint8)
    if data.size != _mip_bytes(fmt, width, height):
        raise ValueError(f"{width}x{height} of format {fmt} is {_mip_bytes(fmt, width, height)} bytes, got {data.size}")
    block = fmt in FMT_BLOCK_BYTES
    flags = _DDSD_CAPS | _DDSD_HEIGHT | _DDSD_WIDTH | _DDSD_PIXELFORMAT | (_DDSD_LINEARSIZE if block else 0x8) | (_DDSD_MIPMAPCOUNT if mip_count > 1 else 0)
    pitch = data.size if block else width * 4
    caps = _CAPS_TEXTURE | ((_CAPS_COMPLEX | _CAPS_MIPMAP) if mip_count > 1 else 0)
    extra = b""
    if header == "dx10":
        pf = struct.pack("<2I4s5I", 32, _DDPF_FOURCC, b"DX10", 0, 0, 0, 0, 0)
        extra = struct.pack("<5I", _DXGI_OF[fmt], 3, 0, 1, 0)
    elif header.startswith("legacy"):
        if block:
            fourcc = header.split(":", 1)[1].encode() if ":" in header else _FOURCC_OF.get(fmt)
            if fourcc is None or _FOURCC.get(fourcc) != fmt:
                raise ValueError(f"format {fmt} has no legacy header {header!r}")
            pf = struct.pack("<2I4s5I", 32, _DDPF_FOURCC, fourcc, 0, 0, 0, 0, 0)
        elif fmt == FMT_RGBA8_UNORM:
            pf = struct.pack("<2I4s5I", 32, _DDPF_RGB | _DDPF_ALPHAPIXELS, b"\0\0\0\0", 32, *_RGBA_MASKS)
        else:
            raise ValueError(f"format {fmt} has no legacy header")
    else:
        raise ValueError(f"unknown header form {header!r}")
    head = b"DDS " + struct.pack("<7I", 124, flags, height, width, pitch, 0, mip_count if mip_count > 1 else 0) + bytes(44) + pf + \
        struct.pack("<5I", caps, 0, 0, 0, 0)
    assert len(head) == 128
    tail = b"".join(bytes(_mip_bytes(fmt, max(1, width >> m), max(1, height >> m))) for m in range(1, mip_count))
    return head + extra + data.tobytes() + tail
