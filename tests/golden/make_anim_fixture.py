"""Writes tests/golden/anim/column.gltf + column.bin + scene.json: the smallest asset through which skins and animations reach both hosts.
Uses struct, math and json ONLY -- nothing of ingest.py, so that the fixture cannot share a misreading with the code it checks. The three
files are committed; this script documents how they were made.

The asset, node by node (default scene: roots 0, 8, 9):
  0 root    translation, scale           children 1, 2, 5, 6, 7
  1 column  mesh 0, skin 0               the skinned column: two primitives (u8 joints + float weights | u16 joints + normalised u16 weights)
  2 joint0                               child 3
  3 joint1  translation (0, 0.5, 0)
  4 (not in the scene)                   named "joint1" as well: never traversed, its channel still feeds the NAME joint1
  5 box     mesh 1                       the rigid child
  6 box     (no mesh)                    the SAME name later in traversal order: a lookup of "box" finds this one
  7 spare
  8 floor   mesh 2
  9 light   mesh 3, given as a matrix    decomposed by the animation loader
Skin 0: joints (2, 3), inverse binds identity and Translate(0, -0.5, 0): the rest pose skins to the identity.
Clip 0 "bend" (duration 1: the STEP channel's key at 3 s does not count):
  joint1 rotation LINEAR | "joint1" rotation LINEAR again, through node 4 (doubled: ignored) | joint1 translation STEP (skipped) | box rotation LINEAR |
  a channel without a target node (skipped)
Clip 1 "lift" (duration 2): joint0 rotation | box translation | box scale
"""
import json, math, os, struct

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "anim")
SEGMENTS = 4
blob = bytearray(); views = []; accessors = []


def add(data, ctype, atype, count, normalized=False, minmax=None):
    while len(blob) % 4:
        blob.append(0)
    views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)})
    blob.extend(data)
    a = {"bufferView": len(views) - 1, "componentType": ctype, "count": count, "type": atype}
    if normalized:
        a["normalized"] = True
    if minmax:
        a["min"], a["max"] = minmax
    accessors.append(a)
    return len(accessors) - 1


def f3(rows):
    return b"".join(struct.pack("<3f", *r) for r in rows)


def minmax(rows):
    return [min(r[k] for r in rows) for k in range(3)], [max(r[k] for r in rows) for k in range(3)]


def qz(deg):
    a = math.radians(deg) / 2
    return (0.0, 0.0, math.sin(a), math.cos(a))


def qy(deg):
    a = math.radians(deg) / 2
    return (0.0, math.sin(a), 0.0, math.cos(a))


def column_sides(sides):
    pos, nrm, idx, h = [], [], [], []
    for side in sides:
        a = side * math.pi / 2
        n = (math.cos(a), 0.0, math.sin(a)); t = (-math.sin(a), 0.0, math.cos(a))
        base = len(pos)
        for k in range(SEGMENTS + 1):
            y = k / SEGMENTS
            for e in (-1, 1):
                pos.append((n[0] * 0.12 + t[0] * 0.12 * e, y, n[2] * 0.12 + t[2] * 0.12 * e)); nrm.append(n); h.append(y)
        for k in range(SEGMENTS):
            i0 = base + 2 * k
            idx += [i0, i0 + 2, i0 + 1, i0 + 1, i0 + 2, i0 + 3]
    return pos, nrm, idx, h


def quad(p, n):
    return list(p), [n] * 4, [0, 1, 2, 0, 2, 3]


def box():
    pos, nrm, idx = [], [], []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            n = [0.0, 0.0, 0.0]; n[axis] = sgn
            a, b = (axis + 1) % 3, (axis + 2) % 3
            base = len(pos)
            for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = [0.0, 0.0, 0.0]; p[axis] = 0.5 * sgn; p[a] = 0.5 * sa; p[b] = 0.5 * sb
                pos.append(tuple(p)); nrm.append(tuple(n))
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return pos, nrm, idx


prims = []
# primitive 0: sides 0, 1 -- JOINTS_0 as unsigned bytes, WEIGHTS_0 as floats
pos, nrm, idx, h = column_sides((0, 1))
prims.append({"attributes": {"POSITION": add(f3(pos), 5126, "VEC3", len(pos), minmax=minmax(pos)), "NORMAL": add(f3(nrm), 5126, "VEC3", len(nrm)),
                             "JOINTS_0": add(b"".join(struct.pack("<4B", 0, 1, 0, 0) for _ in pos), 5121, "VEC4", len(pos)),
                             "WEIGHTS_0": add(b"".join(struct.pack("<4f", 1 - y, y, 0, 0) for y in h), 5126, "VEC4", len(pos))},
              "indices": add(struct.pack("<%dH" % len(idx), *idx), 5123, "SCALAR", len(idx)), "material": 0})
# primitive 1: sides 2, 3 -- JOINTS_0 as unsigned shorts, WEIGHTS_0 as normalised unsigned shorts
pos, nrm, idx, h = column_sides((2, 3))
prims.append({"attributes": {"POSITION": add(f3(pos), 5126, "VEC3", len(pos), minmax=minmax(pos)), "NORMAL": add(f3(nrm), 5126, "VEC3", len(nrm)),
                             "JOINTS_0": add(b"".join(struct.pack("<4H", 0, 1, 0, 0) for _ in pos), 5123, "VEC4", len(pos)),
                             "WEIGHTS_0": add(b"".join(struct.pack("<4H", 65535 - round(65535 * y), round(65535 * y), 0, 0) for y in h), 5123, "VEC4",
                                              len(pos), normalized=True)},
              "indices": add(struct.pack("<%dH" % len(idx), *idx), 5123, "SCALAR", len(idx)), "material": 0})
meshes = [{"name": "column", "primitives": prims}]
for name, (pos, nrm, idx), mat in (("box", box(), 1),
                                   ("floor", quad(((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)), (0, 1, 0)), 2),
                                   ("light", quad(((-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5)), (0, -1, 0)), 3)):
    meshes.append({"name": name, "primitives": [{"attributes": {"POSITION": add(f3(pos), 5126, "VEC3", len(pos), minmax=minmax(pos)),
                                                                "NORMAL": add(f3(nrm), 5126, "VEC3", len(nrm))},
                                                 "indices": add(struct.pack("<%dH" % len(idx), *idx), 5123, "SCALAR", len(idx)), "material": mat}]})

ibm = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] + [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, -0.5, 0, 1]
ibm_acc = add(struct.pack("<32f", *ibm), 5126, "MAT4", 2)


def times(ts):
    return add(struct.pack("<%df" % len(ts), *ts), 5126, "SCALAR", len(ts), minmax=([min(ts)], [max(ts)]))


def vec(rows, n):
    return add(b"".join(struct.pack("<%df" % n, *r) for r in rows), 5126, "VEC%d" % n, len(rows))


t3 = times([0.0, 0.5, 1.0])
bend = {"name": "bend", "samplers": [
    {"input": t3, "output": vec([qz(0), qz(40), qz(-25)], 4), "interpolation": "LINEAR"},
    {"input": t3, "output": vec([qz(0), qz(-80), qz(80)], 4), "interpolation": "LINEAR"},
    {"input": times([0.0, 3.0]), "output": vec([(0, 0.5, 0), (0, 5.0, 0)], 3), "interpolation": "STEP"},
    {"input": times([0.25, 0.75]), "output": vec([qy(0), tuple(-v for v in qy(90))], 4)},      # the other sign of the same rotation: a negative dot
    {"input": t3, "output": vec([(9, 9, 9)] * 3, 3), "interpolation": "LINEAR"}],
    "channels": [{"sampler": 0, "target": {"node": 3, "path": "rotation"}}, {"sampler": 1, "target": {"node": 4, "path": "rotation"}},
                 {"sampler": 2, "target": {"node": 3, "path": "translation"}}, {"sampler": 3, "target": {"node": 5, "path": "rotation"}},
                 {"sampler": 4, "target": {"path": "translation"}}]}
lift = {"name": "lift", "samplers": [
    {"input": times([0.0, 2.0]), "output": vec([qz(0), qz(30)], 4), "interpolation": "LINEAR"},
    {"input": times([0.0, 1.0, 2.0]), "output": vec([(-0.6, 0.3, -0.1), (-0.6, 0.7, -0.1), (-0.6, 0.3, -0.1)], 3), "interpolation": "LINEAR"},
    {"input": times([0.0, 2.0]), "output": vec([(0.2, 0.2, 0.2), (0.3, 0.2, 0.2)], 3), "interpolation": "LINEAR"}],
    "channels": [{"sampler": 0, "target": {"node": 2, "path": "rotation"}}, {"sampler": 1, "target": {"node": 6, "path": "translation"}},
                 {"sampler": 2, "target": {"node": 5, "path": "scale"}}]}

gltf = {
    "asset": {"version": "2.0"}, "extensionsUsed": ["KHR_materials_emissive_strength"],
    "scene": 0, "scenes": [{"name": "column", "nodes": [0, 8, 9]}],
    "nodes": [
        {"name": "root", "translation": [0.1, 0, 0.2], "scale": [1, 1.2, 1], "children": [1, 2, 5, 6, 7]},
        {"name": "column", "mesh": 0, "skin": 0},
        {"name": "joint0", "children": [3]},
        {"name": "joint1", "translation": [0, 0.5, 0]},
        {"name": "joint1"},
        {"name": "box", "mesh": 1, "translation": [-0.9, 0.2, -0.1], "scale": [0.2, 0.2, 0.2]},
        {"name": "box", "translation": [-0.6, 0.3, -0.1], "scale": [0.2, 0.2, 0.2]},
        {"name": "spare"},
        {"name": "floor", "mesh": 2},
        {"name": "light", "mesh": 3, "matrix": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 2.2, 0, 1]},
    ],
    "skins": [{"joints": [2, 3], "inverseBindMatrices": ibm_acc}],
    "animations": [bend, lift],
    "meshes": meshes,
    "materials": [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.5, 0.2, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.4}},
                  {"pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.5, 0.8, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.6}},
                  {"pbrMetallicRoughness": {"baseColorFactor": [0.73, 0.73, 0.73, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.5}},
                  {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.5},
                   "emissiveFactor": [1.0, 1.0, 1.0], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 10.0}}}],
    "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(blob), "uri": "column.bin"}],
}
scene = {
    "Camera": {"Position": {"X": 0, "Y": 0.9, "Z": -2.2}, "Rotation": {"X": 0, "Y": 0, "Z": 0, "W": 1}},
    "EnvironmentLight": {"Color": {"R": 0.05, "G": 0.06, "B": 0.08, "A": 1.0}},
    "Models": {"actor": "column.gltf"},
    "Animations": {"moves": "column.gltf"},
    "RenderObjects": [{"Name": "actor", "Model": "actor", "Animation": "moves",
                       "Transform": {"Translation": {"X": 0.05, "Y": 0, "Z": 0}, "Rotation": {"Yaw": 15}, "Scale": {"X": 1, "Y": 1, "Z": 1}}}],
}
os.makedirs(HERE, exist_ok=True)
json.dump(gltf, open(os.path.join(HERE, "column.gltf"), "w"), indent=1)
open(os.path.join(HERE, "column.bin"), "wb").write(bytes(blob))
json.dump(scene, open(os.path.join(HERE, "scene.json"), "w"), indent=1)
