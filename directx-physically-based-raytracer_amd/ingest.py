"""Scene-JSON + glTF 2.0 ingest in the reference's schema and conventions.

What it mirrors (host side of the path, upstream of the acceleration-structure build):
  scene descriptor   Source/MyScene.ixx:33-90, Source/JSONConverters.ixx:12-33, Source/Scene.ixx:33-73
                     {Camera{Position,Rotation}, EnvironmentLight{Color,Rotation,Texture}, Models{name:path},
                      RenderObjects[{Name,Transform{Translation,Rotation,Scale},IsVisible,Model}]}
  glTF loader        Source/GLTFHelpers.ixx:142-537 (ProcessPrimitive, LoadModel): triangles only, index array written
                     BACKWARDS when flipWindingOrder (always, Scene.ixx:90), u16 indices iff count <= 65535,
                     tangents ALWAYS recomputed when NORMAL + TEXCOORD_0 exist (the loader asks for an attribute called
                     "Tangent", which glTF never has, :193), materials incl. KHR_materials_emissive_strength / ior /
                     transmission, base colour + emissive textures forced to sRGB, normal texture only with tangents
  instance transform Source/Scene.ixx:195-231: world = GlobalTransform * Scale(1,1,-1) * RenderObject.Transform()
                     (SimpleMath row-vector convention), AffineTransform = Scale * Rotation * Translation (Math.ixx:17-19)
Texture *files* are decoded with PIL (PNG/JPEG); a DDS image -- a texture's MSFT_texture_dds source wins over its PNG, as in the
reference (GLTFHelpers.ixx:87-90,103,451) -- is read by bc.read_dds and its BC1 / BC3 / BC4 / BC5 blocks are handed on as they are; a DDS
outside those formats is listed in Mesh.skipped_textures and the material keeps its factors. EXR/HDR stay out of scope (TextureHelpers.ixx).
[DirectXMesh spec] ComputeTangentFrame is an un-vendored dependency: restated as Lengyel's per-vertex accumulation with
Gram-Schmidt against the normal.
What both hosts accept of a file is stated in DESIGN.md section 2 ("what the hosts accept"); host/pt_ingest.hpp refuses the same files.
"""
import base64
import io
import json
import math
import os
import re
import struct

import numpy as np

from . import bc
from . import layouts as L
from . import scenes as S

_COMPONENT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}
MAX_JSON_DEPTH = 128                                                      # kMaxJsonDepth of host/pt_ingest.hpp
_JSON_STRING_OR_BRACKET = re.compile(rb'"(?:[^"\\]|\\.)*"|[\[{\]}]')


def _index(v, n):
    """A file value that indexes a list of n entries (or states a size below n): a non-negative int below n, nothing else. Python
    itself would take -1 for the last entry, True for 1 and a float wherever it only slices."""
    if type(v) is not int or not 0 <= v < n:
        raise ValueError(f"{v!r} where an integer from 0 to {n - 1} is expected")
    return v


def _loads(text):
    """json.loads of a file's text, refusing arrays and objects nested deeper than MAX_JSON_DEPTH (the C++ reader recurses per level)."""
    depth = 0
    for m in _JSON_STRING_OR_BRACKET.finditer(text):
        c = m.group()[:1]
        depth += 1 if c in b"[{" else -1 if c in b"]}" else 0
        if depth > MAX_JSON_DEPTH:
            raise ValueError(f"JSON: arrays and objects nested deeper than {MAX_JSON_DEPTH}")
    return json.loads(text.decode("utf-8"))


# ----------------------------------------------------------------------------------------------
# SimpleMath / DirectXMath conventions (row vectors: v' = v M)
# ----------------------------------------------------------------------------------------------
def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, s, 0], [0, -s, c, 0], [0, 0, 0, 1]], np.float64)


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0, 0, 0, 1]], np.float64)


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, s, 0, 0], [-s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)


def matrix_from_quaternion(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w), 0],
                     [2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w), 0],
                     [2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y), 0],
                     [0, 0, 0, 1]], np.float64)


def rotation_from_json(j):
    """JSONConverters.ixx:18-26: {Yaw,Pitch,Roll} in degrees -> CreateFromYawPitchRoll(yaw, -pitch, -roll) (roll about Z
    first, then pitch about X, then yaw about Y); all three zero -> raw quaternion {X,Y,Z,W} (default identity)."""
    if j is None:
        return np.eye(4)
    yaw, pitch, roll = float(j.get("Yaw", 0)), float(j.get("Pitch", 0)), float(j.get("Roll", 0))
    if yaw == 0 and pitch == 0 and roll == 0:
        q = (float(j.get("X", 0)), float(j.get("Y", 0)), float(j.get("Z", 0)), float(j.get("W", 1)))
        n = math.sqrt(sum(c * c for c in q)) or 1.0
        return matrix_from_quaternion(tuple(c / n for c in q))
    return rot_z(math.radians(-roll)) @ rot_x(math.radians(-pitch)) @ rot_y(math.radians(yaw))


def vec3_from_json(j, default):
    if j is None:
        return np.array(default, np.float64)
    return np.array([float(j.get("X", default[0])), float(j.get("Y", default[1])), float(j.get("Z", default[2]))], np.float64)


def affine_from_json(j):
    """Math::AffineTransform::operator(): Scale * Rotation * Translation (row-vector)."""
    j = j or {}
    s = vec3_from_json(j.get("Scale"), (1, 1, 1)); t = vec3_from_json(j.get("Translation"), (0, 0, 0))
    m = np.diag([s[0], s[1], s[2], 1.0]) @ rotation_from_json(j.get("Rotation"))
    tr = np.eye(4); tr[3, :3] = t
    return m @ tr


def store_float3x4(m_row):
    """XMStoreFloat3x4: the column-vector affine [R|t] = top 3 rows of the transpose."""
    return np.ascontiguousarray(m_row.T[:3, :], np.float32)


# ----------------------------------------------------------------------------------------------
# scene descriptor
# ----------------------------------------------------------------------------------------------
def load_scene_desc(path):
    with open(path) as f:
        j = json.load(f)
    base = os.path.dirname(os.path.abspath(path))

    def resolve(p):
        return p if (not p or os.path.isabs(p)) else os.path.join(base, p)

    env = j.get("EnvironmentLight", {}) or {}
    col = env.get("Color") or {}
    desc = {
        "Camera": {"Position": vec3_from_json((j.get("Camera") or {}).get("Position"), (0, 0, 0)),
                   "Rotation": rotation_from_json((j.get("Camera") or {}).get("Rotation"))},
        "EnvironmentLight": {"Color": (float(col.get("R", 0)), float(col.get("G", 0)), float(col.get("B", 0)), float(col.get("A", -1))),
                             "Rotation": rotation_from_json(env.get("Rotation")), "Texture": resolve(env.get("Texture", ""))},
        "Models": {k: resolve(v) for k, v in (j.get("Models") or {}).items()},
        "Animations": {k: resolve(v) for k, v in (j.get("Animations") or {}).items()},
        "RenderObjects": [],
    }
    for ro in j.get("RenderObjects") or []:
        model = ro.get("Model", "")
        if model and model not in desc["Models"]:                      # MyScene.ixx:57-70
            name = ("RenderObject " + ro["Name"]) if ro.get("Name") else "Unnamed RenderObject"
            raise RuntimeError(f"{path}: {name}: Models {model} not found")
        anim = ro.get("Animation", "")
        if anim and anim not in desc["Animations"]:                    # MyScene.ixx:69
            name = ("RenderObject " + ro["Name"]) if ro.get("Name") else "Unnamed RenderObject"
            raise RuntimeError(f"{path}: {name}: Animations {anim} not found")
        desc["RenderObjects"].append({"Name": ro.get("Name", ""), "Transform": affine_from_json(ro.get("Transform")),
                                      "IsVisible": bool(ro.get("IsVisible", True)), "Model": model, "Animation": anim})
    return desc


# ----------------------------------------------------------------------------------------------
# glTF
# ----------------------------------------------------------------------------------------------
class _Asset:
    def __init__(self, path):
        self.dir = os.path.dirname(os.path.abspath(path))
        raw = open(path, "rb").read()
        self.bin_chunk = None
        if raw[:4] == b"glTF":
            _, _, length = struct.unpack_from("<III", raw, 0)
            if not 12 <= length <= len(raw):
                raise ValueError("GLB: the length in the header does not lie inside the file")
            off = 12
            while off < length:
                if length - off < 8:
                    raise ValueError("GLB: a chunk header reaches beyond the file")
                clen, ctype = struct.unpack_from("<II", raw, off)
                if clen > length - off - 8:
                    raise ValueError("GLB: a chunk reaches beyond the file")
                data = raw[off + 8: off + 8 + clen]
                if ctype == 0x4E4F534A:
                    self.j = _loads(data)
                elif ctype == 0x004E4942:
                    self.bin_chunk = data
                off += 8 + clen
        else:
            self.j = _loads(raw)
        self.buffers = {}

    def buffer(self, i):
        if i not in self.buffers:
            b = self.j["buffers"][_index(i, len(self.j["buffers"]))]
            uri = b.get("uri")
            if uri is None:
                self.buffers[i] = self.bin_chunk
            elif uri.startswith("data:"):
                self.buffers[i] = base64.b64decode(uri.split(",", 1)[1])
            else:
                self.buffers[i] = open(os.path.join(self.dir, uri), "rb").read()
        return self.buffers[i]

    def view_bytes(self, vi):
        v = self.j["bufferViews"][_index(vi, len(self.j["bufferViews"]))]
        b = self.buffer(v["buffer"])
        off = _index(v.get("byteOffset", 0), len(b) + 1)
        return b[off: off + _index(v["byteLength"], len(b) - off + 1)], _index(v.get("byteStride", 0), 253)     # inside its buffer

    def accessor(self, ai):
        a = self.j["accessors"][_index(ai, len(self.j["accessors"]))]
        dt = np.dtype(_COMPONENT[a["componentType"]]); nc = _NCOMP[a["type"]]
        data, stride = self.view_bytes(a["bufferView"])
        count = _index(a["count"], len(data) + 1)                         # frombuffer keeps the accessor inside its view
        off = _index(a.get("byteOffset", 0), len(data) + 1)
        elem = dt.itemsize * nc
        if stride in (0, elem):
            arr = np.frombuffer(data, dt, count * nc, off).reshape(count, nc)
        else:
            arr = np.stack([np.frombuffer(data, dt, nc, off + i * stride) for i in range(count)])
        if a.get("normalized") and dt.kind in "iu":
            arr = arr.astype(np.float32) / float(np.iinfo(dt).max)
        return arr

    def image_bytes(self, ii):
        im = self.j["images"][_index(ii, len(self.j["images"]))]
        if "uri" in im:
            uri = im["uri"]
            return base64.b64decode(uri.split(",", 1)[1]) if uri.startswith("data:") else open(os.path.join(self.dir, uri), "rb").read()
        return self.view_bytes(im["bufferView"])[0]

    def image_is_dds(self, ii, data):
        im = self.j["images"][ii]
        uri = im.get("uri", "")
        return im.get("mimeType") == "image/vnd-ms.dds" or (not uri.startswith("data:") and uri.lower().endswith(".dds")) or bc.is_dds(data)

    def image(self, ii):
        from PIL import Image
        return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(self.image_bytes(ii))).convert("RGBA"), np.uint8))

    def texture(self, ii, force_srgb):
        """Image ii as a scenes.Texture, or -- a DDS file, whose blocks go to the device as they are (TextureHelpers.ixx:65-78) -- a
        scenes.BlockTexture. forceSRGB (base colour, emissive): a UNORM DDS gets the _SRGB format (TextureHelpers.ixx:68).
        None: a DDS this host does not load (bc.read_dds says which)."""
        data = self.image_bytes(ii)
        if not self.image_is_dds(ii, data):
            return S.Texture(self.image(ii), srgb=force_srgb)
        try:
            dds = bc.read_dds(data)
        except ValueError:
            return None
        fmt = bc.SRGB_OF.get(dds.fmt, dds.fmt) if force_srgb else dds.fmt
        if fmt in S.FMT_BLOCK_BYTES:
            return S.BlockTexture(dds.data, dds.width, dds.height, fmt)
        return S.Texture(dds.data, srgb=(fmt == S.FMT_RGBA8_UNORM_SRGB))


def compute_tangents(positions, normals, uvs, indices):
    """[DirectXMesh spec] ComputeTangentFrame (tangent output only)."""
    tan = np.zeros((len(positions), 3), np.float64)
    tri = np.asarray(indices, np.int64).reshape(-1, 3)
    p = positions.astype(np.float64); t = uvs.astype(np.float64)
    for a, b, c in tri:
        e1, e2 = p[b] - p[a], p[c] - p[a]
        du1, dv1 = t[b] - t[a]; du2, dv2 = t[c] - t[a]
        det = du1 * dv2 - du2 * dv1
        if abs(det) < 1e-20:
            continue
        sdir = (e1 * dv2 - e2 * dv1) / det
        tan[a] += sdir; tan[b] += sdir; tan[c] += sdir
    n = normals.astype(np.float64)
    tan = tan - n * (n * tan).sum(1, keepdims=True)
    ln = np.linalg.norm(tan, axis=1, keepdims=True)
    fallback = np.cross(n, np.array([0.0, 1.0, 0.0]))
    fl = np.linalg.norm(fallback, axis=1, keepdims=True)
    fallback = np.where(fl > 1e-8, fallback / np.maximum(fl, 1e-30), np.array([1.0, 0.0, 0.0]))
    return np.where(ln > 1e-12, tan / np.maximum(ln, 1e-30), fallback)


def _node_matrix(node):
    """glTF column-vector local matrix."""
    if "matrix" in node:
        return np.array(node["matrix"], np.float64).reshape(4, 4).T
    t = np.eye(4); r = np.eye(4); s = np.eye(4)
    if "translation" in node:
        t[:3, 3] = node["translation"]
    if "rotation" in node:
        r = matrix_from_quaternion(node["rotation"]).T          # column-vector form
    if "scale" in node:
        s = np.diag(list(node["scale"]) + [1.0])
    return t @ r @ s


def load_model(path, flip_winding_order=True):
    """GLTFHelpers::LoadModel. Returns a list of (MeshNode, GlobalTransform row-vector 4x4)."""
    asset = _Asset(path)
    j = asset.j
    tex_cache = {}

    def texture_for(info, force_srgb):
        tex = j["textures"][_index(info["index"], len(j["textures"]))]
        dds = (tex.get("extensions") or {}).get("MSFT_texture_dds") or {}
        src = dds.get("source", tex.get("source"))                        # the DDS image wins over the PNG (GLTFHelpers.ixx:87-90,103,451)
        key = (src, force_srgb)
        if key not in tex_cache:
            tex_cache[key] = asset.texture(src, force_srgb)
        return tex_cache[key]

    def process_primitive(prim):
        if _index(prim.get("mode", 4), 65536) != 4 or "POSITION" not in prim["attributes"] or "indices" not in prim:
            return None                                                   # :150-152,169-171,191-193
        attrs = prim["attributes"]
        pos = asset.accessor(attrs["POSITION"]).astype(np.float32)
        idx = asset.accessor(prim["indices"])
        if idx.dtype.kind != "u":
            raise ValueError("glTF: indices are not unsigned integers")
        idx = idx.reshape(-1).astype(np.int64)
        if idx.size and idx.max() >= len(pos):
            raise ValueError("glTF: vertex index beyond the POSITION accessor")
        if flip_winding_order:
            idx = idx[::-1].copy()                                        # slot count-1-i <- index i (:179)
        indices = idx.astype(np.uint16 if idx.size <= 65535 else np.uint32)
        has_uv = [False, False]; uvs = [None, None]
        for i in (0, 1):
            if f"TEXCOORD_{i}" in attrs:
                uvs[i] = asset.accessor(attrs[f"TEXCOORD_{i}"]).astype(np.float32); has_uv[i] = True
        nrm = tan = None
        if "NORMAL" in attrs:
            nrm = asset.accessor(attrs["NORMAL"]).astype(np.float32)
            if uvs[0] is not None:                                        # "Tangent" is never found -> always recomputed (:251-275)
                tan = compute_tangents(pos, nrm, uvs[0], indices)
        vb = S.make_vertices(pos, nrm, uvs[0], tan, uvs[1])
        mesh = S.Mesh(vb, indices, has_normals=nrm is not None, material=None, has_tangents=tan is not None, has_uv=tuple(has_uv))
        if "JOINTS_0" in attrs and "WEIGHTS_0" in attrs:                  # :278-304: the 48-byte skeletal vertex + a motion-vector buffer
            joints = asset.accessor(attrs["JOINTS_0"]); weights = asset.accessor(attrs["WEIGHTS_0"])
            if joints.dtype not in (np.uint8, np.uint16) or joints.shape[1] != 4:
                raise ValueError("glTF: JOINTS_0 is not a VEC4 of unsigned bytes or shorts")
            if weights.shape[1] != 4 or len(joints) != len(pos) or len(weights) != len(pos):
                raise ValueError("glTF: JOINTS_0 / WEIGHTS_0 do not match the POSITION accessor")
            if weights.dtype.kind in "iu":                                # normalised integers (accessor() converts the flagged ones)
                weights = weights.astype(np.float32) / float(np.iinfo(weights.dtype).max)
            sk = np.zeros(len(pos), L.SKELETAL_VERTEX)
            sk["Position"] = vb["Position"]; sk["Normal"] = vb["Normal"]; sk["Tangent"] = vb["Tangent"]
            sk["Joints"] = joints.astype(np.uint16)                       # u8 and u16 components both become XMUSHORT4
            sk["Weights"] = weights.astype(np.float32)
            mesh.skeletal_vertices = sk
            mesh.motion_vectors = np.zeros((len(pos), 4), np.uint16)
        if "material" in prim:
            m = j["materials"][_index(prim["material"], len(j["materials"]))]
            pbr = m.get("pbrMetallicRoughness", {})
            ext = m.get("extensions", {})
            mat = L.default_material()
            mat["BaseColor"] = tuple(pbr.get("baseColorFactor", (1, 1, 1, 1)))
            mat["EmissiveStrength"] = ext.get("KHR_materials_emissive_strength", {}).get("emissiveStrength", 1.0)
            mat["EmissiveColor"] = tuple(m.get("emissiveFactor", (0, 0, 0)))
            mat["Metallic"] = pbr.get("metallicFactor", 1.0)
            mat["Roughness"] = pbr.get("roughnessFactor", 1.0)
            mat["IOR"] = ext.get("KHR_materials_ior", {}).get("ior", 1.5)
            mat["AlphaMode"] = {"OPAQUE": 0, "MASK": 1, "BLEND": 2}[m.get("alphaMode", "OPAQUE")]
            mat["AlphaCutoff"] = m.get("alphaCutoff", 0.5)
            tr = ext.get("KHR_materials_transmission")
            if tr:
                mat["Transmission"] = tr.get("transmissionFactor", 0.0)
            mesh.material = mat
            if has_uv[0] or has_uv[1]:                                    # :370-428
                slots = {"BaseColor": (pbr.get("baseColorTexture"), True), "EmissiveColor": (m.get("emissiveTexture"), True),
                         "MetallicRoughness": (pbr.get("metallicRoughnessTexture"), False),
                         "Transmission": ((tr or {}).get("transmissionTexture"), False),
                         "Normal": (m.get("normalTexture") if tan is not None else None, False)}
                textures = {}
                for slot, (info, srgb) in slots.items():
                    if info is not None and _index(info.get("texCoord", 0), 2 ** 32) < 2 and has_uv[info.get("texCoord", 0)]:
                        t = texture_for(info, srgb)
                        if t is None:                                     # listed and skipped: the material keeps its factors
                            mesh.skipped_textures = (mesh.skipped_textures or []) + [slot]
                        else:
                            textures[slot] = (t, info.get("texCoord", 0))
                mesh.textures = textures or None
        return mesh

    out = []
    skins = {}
    scene = j["scenes"][_index(j.get("scene", 0), len(j["scenes"]))]
    nodes = j.get("nodes", [])
    visited = set()
    pending = [(ni, np.eye(4)) for ni in reversed(scene.get("nodes", []))]   # depth first, children in file order, without recursion
    while pending:
        ni, parent = pending.pop()
        if _index(ni, len(nodes)) in visited:                             # glTF wants a strict tree
            raise ValueError(f"glTF: node {ni} is reached twice (a cycle, or a second parent)")
        visited.add(ni)
        node = nodes[ni]
        m = parent @ _node_matrix(node)
        if "mesh" in node:
            prims = j["meshes"][_index(node["mesh"], len(j["meshes"]))].get("primitives", [])
            if prims:
                meshes = [x for x in (process_primitive(p) for p in prims) if x is not None]
                mesh_node = S.MeshNode(meshes)
                mesh_node.name = node.get("name", "")
                if "skin" in node:                                        # :477-512: joint names + inverse bind matrices, shared per skin index
                    si = _index(node["skin"], len(j.get("skins", [])))
                    if si not in skins:
                        skin = j["skins"][si]
                        skins[si] = None
                        if "inverseBindMatrices" in skin:                 # a skin without them is ignored (:484)
                            ibm = asset.accessor(skin["inverseBindMatrices"])
                            if ibm.dtype != np.float32 or ibm.shape[1] != 16:
                                raise ValueError("glTF: inverseBindMatrices is not a MAT4 of floats")
                            names = [nodes[_index(jn, len(nodes))].get("name", "") for jn in skin.get("joints", [])]
                            if len(ibm) > len(names):
                                raise ValueError("glTF: more inverse bind matrices than joints")
                            # glTF's column-major column-vector matrix, reinterpreted as a row-vector Matrix (:492): the floats as they lie
                            skins[si] = (names[:len(ibm)], np.ascontiguousarray(ibm, np.float32).reshape(-1, 4, 4))
                    mesh_node.skin = skins[si]
                out.append((mesh_node, m.T.copy()))                     # GlobalTransform reinterpreted as a row-vector Matrix
        pending.extend((c, m) for c in reversed(node.get("children", [])))
    return out


# ----------------------------------------------------------------------------------------------
# animations
# ----------------------------------------------------------------------------------------------
def decompose(m_col):
    """fastgltf's DecomposeNodeMatrices on a column-vector matrix: translation, rotation (x, y, z, w), scale. The scale is the length of
    each basis column (the first negated when the basis is left-handed), the rotation what remains."""
    m = np.asarray(m_col, np.float64)
    t = m[:3, 3].copy()
    sc = np.linalg.norm(m[:3, :3], axis=0)
    if np.linalg.det(m[:3, :3]) < 0:
        sc[0] = -sc[0]
    r = m[:3, :3] / np.where(sc == 0, 1.0, sc)
    tr = r[0, 0] + r[1, 1] + r[2, 2]
    if tr > 0:
        k = math.sqrt(tr + 1.0) * 2
        q = ((r[2, 1] - r[1, 2]) / k, (r[0, 2] - r[2, 0]) / k, (r[1, 0] - r[0, 1]) / k, 0.25 * k)
    elif r[0, 0] > r[1, 1] and r[0, 0] > r[2, 2]:
        k = math.sqrt(1.0 + r[0, 0] - r[1, 1] - r[2, 2]) * 2
        q = (0.25 * k, (r[0, 1] + r[1, 0]) / k, (r[0, 2] + r[2, 0]) / k, (r[2, 1] - r[1, 2]) / k)
    elif r[1, 1] > r[2, 2]:
        k = math.sqrt(1.0 + r[1, 1] - r[0, 0] - r[2, 2]) * 2
        q = ((r[0, 1] + r[1, 0]) / k, 0.25 * k, (r[1, 2] + r[2, 1]) / k, (r[0, 2] - r[2, 0]) / k)
    else:
        k = math.sqrt(1.0 + r[2, 2] - r[0, 0] - r[1, 1]) * 2
        q = ((r[0, 2] + r[2, 0]) / k, (r[1, 2] + r[2, 1]) / k, 0.25 * k, (r[1, 0] - r[0, 1]) / k)
    return t, np.array(q), sc


_PATHS = {"translation": (0, 3), "rotation": (1, 4), "scale": (2, 3)}


def load_animation(path):
    """GLTFHelpers::LoadAnimation (GLTFHelpers.ixx:539-663) -> scenes.Rig: the default scene's node forest flattened depth first with its
    decomposed TRS, one clip per glTF animation. LINEAR samplers only (STEP and CUBICSPLINE channels are skipped, :582-584), channels
    without a target node are skipped, and per node NAME and path the first channel wins (:593, :616, :639); a clip's duration is the
    largest key time of the channels it accepted.

    The reference keeps keyframes and global transforms in maps keyed by node name. Names are resolved to indices HERE, with the maps'
    semantics: the keyframes of a name apply to every node of the forest that carries it (ComputeTransforms looks them up per node,
    Animation.ixx:123), and a lookup BY name (a mesh node, a joint: find_node) finds the LAST node of that name in traversal order,
    because m_globalTransforms[name] is overwritten (:138)."""
    asset = _Asset(path)
    j = asset.j
    nodes = j.get("nodes", [])
    scene = j["scenes"][_index(j.get("scene", 0), len(j["scenes"]))]
    parents, rest, names, visited = [], [], [], set()
    pending = [(ni, -1) for ni in reversed(scene.get("nodes", []))]
    while pending:
        ni, parent = pending.pop()
        if _index(ni, len(nodes)) in visited:
            raise ValueError(f"glTF: node {ni} is reached twice (a cycle, or a second parent)")
        visited.add(ni)
        node = nodes[ni]
        if "matrix" in node:
            t, q, sc = decompose(np.array(node["matrix"], np.float64).reshape(4, 4).T)
        else:
            t, q, sc = (np.array(node.get(k, d), np.float64) for k, d in (("translation", (0, 0, 0)), ("rotation", (0, 0, 0, 1)), ("scale", (1, 1, 1))))
        if t.shape != (3,) or q.shape != (4,) or sc.shape != (3,):
            raise ValueError(f"glTF: node {ni}: translation / rotation / scale of the wrong length")
        me = len(parents)
        parents.append(parent); rest.append(np.concatenate([t, q, sc])); names.append(node.get("name", ""))
        pending.extend((c, me) for c in reversed(node.get("children", [])))
    n = len(parents)
    anims = j.get("animations", [])
    channels = np.zeros((len(anims), n, 3, 2), np.uint32)
    key_times, key_values, durations, clip_names = [], [], [], []
    for ci, anim in enumerate(anims):
        duration = np.float32(0)
        taken = {}                                                        # (node name, path) -> (FirstKey, KeyCount): the first channel wins
        samplers = anim.get("samplers", [])
        for ch in anim.get("channels", []):
            target = ch.get("target") or {}
            if "node" not in target:
                continue
            sampler = samplers[_index(ch["sampler"], len(samplers))]
            if sampler.get("interpolation", "LINEAR") != "LINEAR":
                continue
            if target.get("path") not in _PATHS:                          # weights: morph targets are out of scope
                continue
            slot, ncomp = _PATHS[target["path"]]
            name = nodes[_index(target["node"], len(nodes))].get("name", "")
            if (name, slot) in taken:
                continue
            times = asset.accessor(sampler["input"]); values = asset.accessor(sampler["output"])
            if times.dtype != np.float32 or times.shape[1] != 1:
                raise ValueError("glTF: an animation sampler's input is not a SCALAR of floats")
            if values.shape[1] != ncomp or values.dtype.kind != "f":
                raise ValueError(f"glTF: an animation sampler's output does not fit the {target['path']} path")
            if len(times) != len(values):
                raise ValueError("glTF: an animation sampler's input and output counts differ")
            if len(times) == 0:
                continue                                                  # an empty channel leaves the slot empty: a later one may take it
            times = times.reshape(-1)
            if not np.all(np.isfinite(times)) or not np.all(np.isfinite(values)) or np.any(np.diff(times) <= 0):
                raise ValueError("glTF: key times must be finite and strictly ascending, key values finite")
            taken[(name, slot)] = (len(key_times), len(times))
            key_times += times.tolist()
            key_values += np.pad(values.astype(np.float32), ((0, 0), (0, 4 - ncomp))).tolist()
            duration = max(duration, np.float32(times.max()))
        for ni in range(n):                                               # the keyframes of a name apply to every node that carries it
            for slot in range(3):
                if (names[ni], slot) in taken:
                    channels[ci, ni, slot] = taken[(names[ni], slot)]
        durations.append(float(duration)); clip_names.append(anim.get("name", ""))
    if not anims:
        raise ValueError(f"{path}: the file holds no animation")
    return S.Rig(np.asarray(parents, np.int32), np.asarray(rest, np.float32).reshape(n, 10), np.asarray(durations, np.float64), channels,
                 np.asarray(key_times, np.float32), np.asarray(key_values, np.float32).reshape(-1, 4), names=names, clip_names=clip_names)


def find_node(rig, name):
    """m_globalTransforms.find(name): the LAST node of that name in traversal order (the map entry is overwritten), or NO_NODE."""
    for ni in range(len(rig.names) - 1, -1, -1):
        if rig.names[ni] == name:
            return ni
    return S.NO_NODE


# ----------------------------------------------------------------------------------------------
# Scene::Load + Refresh
# ----------------------------------------------------------------------------------------------
def camera_from_desc(desc, aspect, hfov_deg=90.0, near=0.01):
    """App::ResetCamera: CameraController::SetPosition / SetRotation (Source/Camera.ixx:84-97), default lens."""
    r = desc["Camera"]["Rotation"]
    fwd = np.array([0, 0, 1, 0]) @ r
    right = np.array([1, 0, 0, 0]) @ r
    up = np.cross(fwd[:3], right[:3])
    return S.make_camera(desc["Camera"]["Position"], forward=fwd[:3], up=up, hfov_deg=hfov_deg, aspect=aspect, near=near)


def _copy_mesh(m):
    import copy
    c = copy.copy(m)
    c.vertices = m.vertices.copy(); c.motion_vectors = m.motion_vectors.copy() if m.motion_vectors is not None else None
    return c


def load_scene(path, aspect=16 / 9):
    desc = load_scene_desc(path)
    models, rigs = {}, {}
    nodes, objects, animations = [], [], []
    zflip = np.diag([1.0, 1.0, -1.0, 1.0])
    for ro in desc["RenderObjects"]:
        if not ro["Model"]:
            continue
        if ro["Model"] not in models:
            models[ro["Model"]] = load_model(desc["Models"][ro["Model"]], flip_winding_order=True)    # Scene.ixx:90
        rig = None
        if ro["Animation"]:                                               # Scene.ixx:165-168: a copy of the collection, bound to the model's skins
            if ro["Animation"] not in rigs:
                rigs[ro["Animation"]] = load_animation(desc["Animations"][ro["Animation"]])
            rig = rigs[ro["Animation"]]
        binding_nodes, binding_instances, binding_globals, skins = [], [], [], []
        # Model.SkinJoints is a dictionary keyed by the mesh node's name: the last skin stored under a name serves every mesh node of that name
        skin_of = {mn.name: mn.skin for mn, _ in models[ro["Model"]] if getattr(mn, "skin", None) is not None}
        for mesh_node, g in models[ro["Model"]]:
            if rig is not None and any(m.skeletal_vertices is not None for m in mesh_node.meshes):
                # the skinning pass rewrites the vertex buffer in place: a skinned mesh node is instanced once per animated render object
                mesh_node = S.MeshNode([_copy_mesh(m) for m in mesh_node.meshes], name=mesh_node.name, skin=mesh_node.skin)
            key = id(mesh_node)
            if key not in [id(n) for n in nodes]:
                nodes.append(mesh_node)
            world = g @ zflip @ ro["Transform"]                           # Scene.ixx:199-214
            if rig is not None:
                binding_nodes.append(find_node(rig, mesh_node.name)); binding_instances.append(len(objects)); binding_globals.append(g)
                skin = skin_of.get(mesh_node.name)
                if skin is not None:
                    skins.append(S.Skin(find_node(rig, mesh_node.name), np.array([find_node(rig, nm) for nm in skin[0]], np.uint32), skin[1],
                                        scene_node=[id(n) for n in nodes].index(key)))
            objects.append(S.RenderObject([id(n) for n in nodes].index(key), store_float3x4(world), ro["IsVisible"]))
        if rig is not None:
            animations.append(S.AnimatedObject(rig, ro["Transform"].astype(np.float32), np.array(binding_nodes, np.uint32),
                                               np.array(binding_instances, np.uint32), np.array(binding_globals, np.float32).reshape(-1, 4, 4), skins))
    sd = S.make_scene_data(desc["EnvironmentLight"]["Color"])
    sd["EnvironmentLightTransform"] = store_float3x4(desc["EnvironmentLight"]["Rotation"])     # App.cpp:1019
    if animations:
        sd["IsStatic"] = 0
    sc = S.Scene(nodes, objects, camera_from_desc(desc, aspect), sd, name=os.path.basename(path))
    sc.animations = animations
    tex = desc["EnvironmentLight"]["Texture"]
    if tex:
        from PIL import Image
        img = np.asarray(Image.open(tex).convert("RGBA"), np.float32) / 255.0
        sc.env_texture = S.Texture(np.ascontiguousarray(img))
    return sc.finalize()


# ----------------------------------------------------------------------------------------------
# writer (tests / fixtures): a scenes.Scene -> .gltf + .bin + scene .json that load_scene() maps back onto it
# ----------------------------------------------------------------------------------------------
def export_scene(scene, directory, name="scene", yaw_pitch_roll=None):
    """Every mesh node becomes one glTF file node (identity node transform, vertices z-negated so that the loader's
    Scale(1,1,-1) restores them); every RenderObject keeps its transform as a raw matrix decomposition is avoided by
    storing Translation / Rotation(quaternion) / Scale recovered from the 3x4."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    blob = bytearray(); views = []; accessors = []; images = []; textures = []; materials = []; meshes = []; gl_nodes = []
    img_index = {}

    def add_view(data, target=None):
        while len(blob) % 4:
            blob.append(0)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(data), **({"target": target} if target else {})})
        blob.extend(data)
        return len(views) - 1

    def add_accessor(arr, ctype, atype, target=None, minmax=False):
        v = add_view(np.ascontiguousarray(arr).tobytes(), target)
        a = {"bufferView": v, "componentType": ctype, "count": len(arr), "type": atype}
        if minmax:
            a["min"] = [float(x) for x in arr.min(0)]; a["max"] = [float(x) for x in arr.max(0)]
        accessors.append(a)
        return len(accessors) - 1

    def add_texture(tex):
        if id(tex) not in img_index:
            buf = io.BytesIO(); Image.fromarray(tex.data).save(buf, "PNG")
            images.append({"bufferView": add_view(buf.getvalue()), "mimeType": "image/png"})
            textures.append({"source": len(images) - 1})
            img_index[id(tex)] = len(textures) - 1
        return img_index[id(tex)]

    for node in scene.nodes:
        prims = []
        for mesh in node.meshes:
            vb = mesh.vertices
            pos = vb["Position"].astype(np.float32) * np.array([1, 1, -1], np.float32)
            attrs = {"POSITION": add_accessor(pos, 5126, "VEC3", 34962, True)}
            if mesh.has_normals:
                n = np.maximum(vb["Normal"].astype(np.float32) / 32767.0, -1.0) * np.array([1, 1, -1], np.float32)
                attrs["NORMAL"] = add_accessor(n, 5126, "VEC3", 34962)
            if mesh.has_uv[0]:
                attrs["TEXCOORD_0"] = add_accessor(vb["TexCoord0"].astype(np.float32), 5126, "VEC2", 34962)
            if mesh.has_uv[1]:
                attrs["TEXCOORD_1"] = add_accessor(vb["TexCoord1"].astype(np.float32), 5126, "VEC2", 34962)
            idx = mesh.indices[::-1].astype(np.uint32)                  # the loader writes them back to front
            prim = {"attributes": attrs, "indices": add_accessor(idx, 5125, "SCALAR", 34963), "mode": 4}
            if mesh.material is not None:
                m = mesh.material
                pbr = {"baseColorFactor": [float(x) for x in m["BaseColor"]], "metallicFactor": float(m["Metallic"]), "roughnessFactor": float(m["Roughness"])}
                gm = {"pbrMetallicRoughness": pbr, "emissiveFactor": [float(x) for x in m["EmissiveColor"]],
                      "alphaMode": ["OPAQUE", "MASK", "BLEND"][int(m["AlphaMode"])], "alphaCutoff": float(m["AlphaCutoff"]),
                      "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": float(m["EmissiveStrength"])},
                                     "KHR_materials_ior": {"ior": float(m["IOR"])}}}
                if float(m["Transmission"]) > 0 or (mesh.textures and "Transmission" in mesh.textures):
                    gm["extensions"]["KHR_materials_transmission"] = {"transmissionFactor": float(m["Transmission"])}
                for slot, (tex, uvi) in (mesh.textures or {}).items():
                    info = {"index": add_texture(tex), "texCoord": uvi}
                    if slot == "BaseColor":
                        pbr["baseColorTexture"] = info
                    elif slot == "MetallicRoughness":
                        pbr["metallicRoughnessTexture"] = info
                    elif slot == "EmissiveColor":
                        gm["emissiveTexture"] = info
                    elif slot == "Normal":
                        gm["normalTexture"] = info
                    elif slot == "Transmission":
                        gm["extensions"]["KHR_materials_transmission"]["transmissionTexture"] = info
                materials.append(gm); prim["material"] = len(materials) - 1
            prims.append(prim)
        meshes.append({"primitives": prims})
        gl_nodes.append({"mesh": len(meshes) - 1, "name": f"node{len(gl_nodes)}"})
    models, render_objects = {}, []
    for ni in range(len(scene.nodes)):
        g = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [gl_nodes[ni]],
             "meshes": meshes, "materials": materials, "accessors": accessors, "bufferViews": views, "images": images, "textures": textures,
             "buffers": [{"uri": name + ".bin", "byteLength": len(blob)}],
             "extensionsUsed": ["KHR_materials_emissive_strength", "KHR_materials_ior", "KHR_materials_transmission"]}
        g["nodes"] = [dict(gl_nodes[ni])]
        with open(os.path.join(directory, f"{name}_node{ni}.gltf"), "w") as f:
            json.dump(g, f)
        models[f"node{ni}"] = f"{name}_node{ni}.gltf"
    open(os.path.join(directory, name + ".bin"), "wb").write(bytes(blob))
    for i, ro in enumerate(scene.objects):
        m = np.asarray(ro.transform, np.float64)                          # column-vector [R|t]; R = Rot * diag(scale)
        scale = np.linalg.norm(m[:, :3], axis=0)
        rot_col = m[:, :3] / scale
        if np.linalg.det(rot_col) < 0:
            scale[2] = -scale[2]; rot_col[:, 2] = -rot_col[:, 2]
        r = rot_col.T                                                      # row-vector rotation matrix
        w = math.sqrt(max(0.0, 1 + r[0, 0] + r[1, 1] + r[2, 2])) / 2
        if w > 1e-6:
            q = ((r[1, 2] - r[2, 1]) / (4 * w), (r[2, 0] - r[0, 2]) / (4 * w), (r[0, 1] - r[1, 0]) / (4 * w), w)
        else:
            x = math.sqrt(max(0.0, 1 + r[0, 0] - r[1, 1] - r[2, 2])) / 2
            y = math.sqrt(max(0.0, 1 - r[0, 0] + r[1, 1] - r[2, 2])) / 2
            z = math.sqrt(max(0.0, 1 - r[0, 0] - r[1, 1] + r[2, 2])) / 2
            q = (x, math.copysign(y, r[0, 1] + r[1, 0]), math.copysign(z, r[0, 2] + r[2, 0]), 0.0)
        render_objects.append({"Name": f"object{i}", "IsVisible": bool(ro.visible), "Model": f"node{ro.node}",
                               "Transform": {"Translation": dict(zip("XYZ", map(float, m[:, 3]))),
                                             "Rotation": dict(zip("XYZW", map(float, q))),
                                             "Scale": dict(zip("XYZ", map(float, scale)))}})
    cam = scene.camera
    desc = {"Camera": {"Position": dict(zip("XYZ", map(float, cam["Position"]))), "Rotation": yaw_pitch_roll or {"X": 0, "Y": 0, "Z": 0, "W": 1}},
            "EnvironmentLight": {"Color": dict(zip("RGBA", map(float, scene.scene_data["EnvironmentLightColor"])))},
            "Models": models, "RenderObjects": render_objects}
    out = os.path.join(directory, name + ".json")
    with open(out, "w") as f:
        json.dump(desc, f, indent=1)
    return out
