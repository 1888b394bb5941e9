"""Host ingest against files it did not write (no GPU): host/pt_ingest.hpp as a stand-alone program (tests/host/ingest_probe.cpp) under
AddressSanitizer and UBSan with float-cast-overflow. Valid files and benign mutations of them load, PNG texels are PIL's byte for byte, every
row of a table of hostile files is refused -- by the C++ host with its own error, by ingest.py with an exception that is no RecursionError
or MemoryError -- and no truncation of a valid file gets past `loaded` / `refused` to a sanitizer report."""
import base64
import copy
import io
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
import bcscene

HERE = os.path.dirname(__file__)
FIXTURES = os.path.join(HERE, "golden", "ingest")
MAX_JSON_DEPTH = 128                                                      # kMaxJsonDepth of host/pt_ingest.hpp
HOSTILE_NUMBERS = [-1, 0.5, 1e300, "x"]                                   # and, per field, one past its list or limit
TRUNCATE_EVERY_BYTE_UP_TO = 4096
TRUNCATE_STRIDE = 97                                                      # of a longer file; a prime, so that the cuts fall on every alignment


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ingest_probe") / "ingest_probe")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "host", "ingest_probe.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def ingest(pkg):
    import dxpbrt_amd.ingest as I
    return I


def run_probe(probe, cases, directory):
    """cases: [(kind, path) or (kind, path, out)] -> {path: "loaded" | "refused <message>"}; one process, no sanitizer report, every case answered"""
    listing = os.path.join(str(directory), "cases_%d.txt" % len(os.listdir(str(directory))))
    with open(listing, "w") as f:
        for c in cases:
            f.write(" ".join(c) + "\n")
    p = subprocess.run([probe, listing], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="max_allocation_size_mb=256"))
    lines = p.stdout.splitlines()
    assert p.returncode == 0 and p.stderr == "", (lines[-2:], p.stderr[-3000:])
    assert len(lines) == 2 * len(cases)
    out = {}
    for c, begin, answer in zip(cases, lines[0::2], lines[1::2]):
        assert begin == "begin " + c[1] and (answer == "loaded" or answer.startswith("refused ")), (begin, answer)
        out[c[1]] = answer
    return out


def write(directory, name, data):
    path = os.path.join(str(directory), name)
    with open(path, "wb") as f:
        f.write(data if isinstance(data, bytes) else data.encode())
    return path


# ---------------------------------------------------------------------- PNG files written here
def png_chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_filter(rows, bpp):
    """scanline y filtered with type y % 5 (PNG spec 9.2): all five filters, the first row of each included"""
    rows = rows.astype(np.int64)
    out = bytearray()
    for y, cur in enumerate(rows):
        up = rows[y - 1] if y else np.zeros_like(cur)
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]]); c = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]])
        p = a + up - c
        pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        pred = [np.zeros_like(cur), a, up, (a + up) // 2, paeth][y % 5]
        out += bytes([y % 5]) + ((cur - pred) % 256).astype(np.uint8).tobytes()
    return bytes(out)


DEFLATE = {"stored": lambda: zlib.compressobj(0), "fixed": lambda: zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED),
           "dynamic": lambda: zlib.compressobj(9)}
BTYPE = {"stored": 0, "fixed": 1, "dynamic": 2}


def make_png(w, h, ctype, samples, deflate="dynamic", palette=None, trns=None, idat_pieces=1, ihdr=None, idat=None):
    """an 8-bit non-interlaced PNG of colour type ctype from samples (h, w, channels); ihdr / idat replace those chunks' bodies"""
    bpp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    if idat is None:
        z = DEFLATE[deflate]()
        idat = z.compress(png_filter(samples.reshape(h, w * bpp), bpp)) + z.flush()
        assert (idat[2] >> 1) & 3 == BTYPE[deflate], "the first deflate block is not " + deflate      # a condition on the input
    out = b"\x89PNG\r\n\x1a\n" + png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0) if ihdr is None else ihdr)
    if palette is not None:
        out += png_chunk(b"PLTE", palette)
    if trns is not None:
        out += png_chunk(b"tRNS", trns)
    step = -(-len(idat) // idat_pieces)
    for k in range(0, len(idat), step):
        out += png_chunk(b"IDAT", idat[k:k + step])
    return out + png_chunk(b"IEND", b"")


def valid_pngs(rng):
    """{name: bytes}: colour types 0, 2, 3, 4, 6, each with stored, fixed and dynamic deflate blocks; sizes that are no multiple of anything"""
    out = {}
    w, h = 61, 47
    y, x = np.mgrid[0:h, 0:w]
    for ctype, nch in ((0, 1), (2, 3), (3, 1), (4, 2), (6, 4)):
        smooth = np.stack([(3 * x + 5 * y + 40 * c) % 256 for c in range(nch)], -1)
        samples = ((smooth + rng.integers(0, 4, smooth.shape)) % 256).astype(np.uint8)       # compressible: zlib picks dynamic codes for it
        extra = dict(palette=rng.integers(0, 256, 768, dtype=np.uint8).tobytes(), trns=rng.integers(0, 256, 100, dtype=np.uint8).tobytes()) if ctype == 3 else {}
        for deflate in DEFLATE:
            out["t%d_%s.png" % (ctype, deflate)] = make_png(w, h, ctype, samples, deflate, idat_pieces=3 if deflate == "dynamic" else 1, **extra)
    return out


def inflate_bomb():
    """a zlib stream of about 1 MiB that inflates to 1 GiB of zeros: one self-contained megabyte (closed by a full flush), repeated"""
    z = zlib.compressobj(9)
    mib = bytes(1 << 20)
    first = z.compress(mib) + z.flush(zlib.Z_FULL_FLUSH)
    again = z.compress(mib) + z.flush(zlib.Z_FULL_FLUSH)
    stream = first + again * 1023 + b"\x01\x00\x00\xff\xff" + b"\0\0\0\0"
    d = zlib.decompressobj()
    assert len(d.decompress(stream, 3 << 20)) == 3 << 20 and len(d.unconsumed_tail) > len(again) * 1000      # it goes on and on
    return stream


def hostile_pngs():
    one = np.zeros((1, 1, 4), np.uint8)
    ihdr = lambda w, h: struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)      # noqa: E731
    return {
        "ihdr_empty.png": make_png(1, 1, 6, one, "fixed", ihdr=b""),
        "width_ffffffff.png": make_png(1, 1, 6, one, "fixed", ihdr=ihdr(0xFFFFFFFF, 1)),
        "width_65537.png": make_png(1, 1, 6, one, "fixed", ihdr=ihdr(65537, 1)),
        "sides_wrap.png": make_png(1, 1, 6, one, "fixed", ihdr=ihdr(0x80000000, 0x80000000)),          # w * h * 4 = 2^64
        "sides_wrap_32.png": make_png(1, 1, 6, one, "fixed", ihdr=ihdr(0x10000, 0x10001)),             # w * h = 2^32 + 65536
        "bomb.png": make_png(1, 1, 6, one, idat=inflate_bomb()),
    }


# ---------------------------------------------------------------------- the glTF the table is cut from
def base_gltf(ingest, pkg, directory):
    """node 0 of an exported textured Cornell box (positions, normals, two UV sets, u32 indices, three textures from bufferViews, an
    external .bin) with the optional members spelled out -- byteStride, both byteOffsets, a child node -- so that the table can set each"""
    path = ingest.export_scene(pkg.scenes.cornell_box_textured(env=None), str(directory), "base")
    g = json.load(open(os.path.join(str(directory), "base_node0.gltf")))
    prim = g["meshes"][0]["primitives"][0]
    pos = g["accessors"][prim["attributes"]["POSITION"]]
    g["bufferViews"][pos["bufferView"]]["byteStride"] = 12
    pos["byteOffset"] = 0
    g["nodes"] = [dict(g["nodes"][0], children=[1]), {"name": "leaf"}]
    return path, g


def set_at(g, where, value):
    g = copy.deepcopy(g)
    at = g
    for k in where[:-1]:
        at = at[k]
    at[where[-1]] = value
    return g


def hostile_gltfs(g, bin_size):
    """{name: glTF text}, every one to be refused: each index or size member in turn -1, 0.5, 1e300, a string and one past its list or limit"""
    prim = ["meshes", 0, "primitives", 0]
    p = g["meshes"][0]["primitives"][0]
    mat = ["materials", p["material"]]
    info = mat + ["pbrMetallicRoughness", "baseColorTexture"]
    tex = g["materials"][p["material"]]["pbrMetallicRoughness"]["baseColorTexture"]["index"]
    pa = p["attributes"]["POSITION"]
    pv = g["accessors"][pa]["bufferView"]
    view = g["bufferViews"][pv]
    n_acc = len(g["accessors"])
    fields = [                                                             # (where, one past its list or limit)
        (prim + ["attributes", "POSITION"], n_acc), (prim + ["attributes", "NORMAL"], n_acc), (prim + ["attributes", "TEXCOORD_0"], n_acc),
        (prim + ["attributes", "TEXCOORD_1"], n_acc), (prim + ["indices"], n_acc), (prim + ["material"], len(g["materials"])),
        (["accessors", pa, "bufferView"], len(g["bufferViews"])), (["accessors", pa, "componentType"], 5127),
        (["accessors", pa, "count"], g["accessors"][pa]["count"] + 1),    # the view holds exactly count elements
        (["accessors", pa, "byteOffset"], view["byteLength"] + 1),
        (["bufferViews", pv, "buffer"], len(g["buffers"])), (["bufferViews", pv, "byteStride"], 253),                       # glTF: at most 252
        (["bufferViews", pv, "byteOffset"], bin_size + 1), (["bufferViews", pv, "byteLength"], bin_size - view["byteOffset"] + 1),
        (["images", g["textures"][tex]["source"], "bufferView"], len(g["bufferViews"])), (["textures", tex, "source"], len(g["images"])),
        (info + ["index"], len(g["textures"])), (info + ["texCoord"], 2 ** 32),                # any set is valid glTF; the hosts keep two
        (["nodes", 0, "mesh"], len(g["meshes"])), (["nodes", 0, "children", 0], len(g["nodes"])),
        (["scene"], len(g["scenes"])), (["scenes", 0, "nodes", 0], len(g["nodes"])),
    ]
    out = {}
    for where, past in fields:
        for value in HOSTILE_NUMBERS + [past]:
            name = "_".join(str(k) for k in where[-3:]) + "_" + str(value).replace("-", "m").replace(".", "p").replace("+", "")
            out[name + ".gltf"] = json.dumps(set_at(g, where, value))
    text = json.dumps(g)
    count = '"count": %d' % g["accessors"][pa]["count"]
    assert count in text
    for spelling in ("NaN", "Infinity", "-Infinity", "nan", "inf", "0x3"):    # what strtod reads beyond JSON's numbers
        out["count_%s.gltf" % spelling.replace("-", "m")] = text.replace(count, '"count": ' + spelling, 1)
    # the three that crashed the loader before it had its checked primitives
    out["brackets.gltf"] = "[" * 200000
    out["cycle.gltf"] = json.dumps({"scenes": [{"nodes": [0]}], "nodes": [{"children": [0]}]})
    out["stride_2_63.gltf"] = json.dumps(set_at(set_at(g, ["bufferViews", pv, "byteStride"], 9223372036854775808), ["accessors", pa, "count"], 3))
    # an accessor that overruns its view, not its buffer
    assert view["byteOffset"] + view["byteLength"] + 4 <= bin_size
    out["accessor_beyond_view.gltf"] = json.dumps(set_at(g, ["bufferViews", pv, "byteLength"], view["byteLength"] - 4))
    two = copy.deepcopy(g)
    two["nodes"] = [{"children": [2]}, {"children": [2]}, g["nodes"][0] | {"children": []}]
    two["scenes"][0]["nodes"] = [0, 1]
    out["two_parents.gltf"] = json.dumps(two)
    out["nesting_past_the_limit.gltf"] = json.dumps(nested(g, MAX_JSON_DEPTH + 1))
    out["bad_unicode_escape.gltf"] = text.replace('"name": "leaf"', '"name": "\\u12G4"', 1)
    assert "\\u12G4" in out["bad_unicode_escape.gltf"]
    return out


def nested(g, depth):
    """g with an extras member that nests arrays to the given depth, the document's own object counted"""
    extras = 0
    for _ in range(depth - 1):
        extras = [extras]
    return dict(g, extras=extras)


def hostile_glbs(glb):
    """{name: GLB bytes}: the header's length and each chunk's length one past the file and 0xFFFFFFFF"""
    json_len = struct.unpack_from("<I", glb, 12)[0]
    offsets = {"header": 8, "json_chunk": 12, "bin_chunk": 20 + json_len}
    assert glb[offsets["bin_chunk"] + 4: offsets["bin_chunk"] + 8] == b"BIN\0"
    out = {}
    for name, off in offsets.items():
        for value in (len(glb) + 1, 0xFFFFFFFF):
            out["%s_%x.glb" % (name, value)] = glb[:off] + struct.pack("<I", value) + glb[off + 4:]
    return out


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, ingest, pkg, bc_module):
    """Everything the tests run, written once from fixed seeds: valid = [(kind, path)], png = {path: bytes}, refused = [(kind, path)]"""
    rng = np.random.default_rng(20240)
    root = tmp_path_factory.mktemp("corpus")
    valid = [("gltf", os.path.join(FIXTURES, "fixture.gltf")), ("gltf", os.path.join(FIXTURES, "fixture.glb")),
             ("scene", os.path.join(FIXTURES, "scene.json")), ("scene", os.path.join(FIXTURES, "scene_glb.json"))]
    scene_path, g = base_gltf(ingest, pkg, root / "export")
    valid += [("scene", scene_path), ("gltf", os.path.join(os.path.dirname(scene_path), "base_node0.gltf"))]
    dds_scene, _ = bcscene.dds_gltf(ingest, pkg.scenes, bc_module, str(root / "dds"))
    valid += [("scene", dds_scene)] + [("dds", os.path.join(str(root / "dds"), n)) for n in ("BaseColor.dds", "MetallicRoughness.dds", "normal.bin")]
    os.makedirs(str(root / "png"))
    pngs = {write(root / "png", name, data): data for name, data in valid_pngs(rng).items()}
    valid += [("png", p) for p in pngs]
    table = root / "table"                                                # beside a base.bin, which its glTF rows refer to
    os.makedirs(str(table))
    shutil.copy(os.path.join(str(root / "export"), "base.bin"), str(table))
    base = write(table, "base_spelled_out.gltf", json.dumps(g))
    bin_size = os.path.getsize(os.path.join(str(table), "base.bin"))
    refused = [("gltf", write(table, n, d)) for n, d in hostile_gltfs(g, bin_size).items()]
    refused += [("gltf", write(table, n, d)) for n, d in hostile_glbs(open(os.path.join(FIXTURES, "fixture.glb"), "rb").read()).items()]
    refused_png = [("png", write(table, n, d)) for n, d in hostile_pngs().items()]
    at_limit = write(table, "nesting_at_the_limit.gltf", json.dumps(nested(g, MAX_JSON_DEPTH)))

    class Corpus:
        pass
    c = Corpus()
    c.root, c.valid, c.pngs, c.base, c.g, c.refused, c.refused_png, c.at_limit, c.rng = root, valid, pngs, base, g, refused, refused_png, at_limit, rng
    return c


@pytest.fixture(scope="module")
def bc_module(pkg):
    import dxpbrt_amd.bc as m
    return m


# ---------------------------------------------------------------------- the tests
def test_valid_files_load_and_png_texels_are_pils(probe, corpus, tmp_path):
    from PIL import Image
    cases = [(k, p) if k != "png" else (k, p, str(tmp_path / (os.path.basename(p) + ".rgba"))) for k, p in corpus.valid + [("gltf", corpus.base)]]
    answers = run_probe(probe, cases, tmp_path)
    assert [p for p, a in answers.items() if a != "loaded"] == []
    assert len(corpus.pngs) == 15
    for path, data in corpus.pngs.items():
        want = Image.open(io.BytesIO(data)).convert("RGBA").tobytes()
        assert open(str(tmp_path / (os.path.basename(path) + ".rgba")), "rb").read() == want, path


def test_benign_mutations_still_load(probe, corpus, ingest, tmp_path):
    """what keeps a loader that refuses everything from passing: payload bytes, a factor and the order of keys are not its business"""
    g = json.load(open(os.path.join(FIXTURES, "fixture.gltf")))
    prefix, payload = g["buffers"][0]["uri"].split(",", 1)
    blob = bytearray(base64.b64decode(payload))
    cases = []
    for n in range(8):
        m, b = copy.deepcopy(g), bytearray(blob)
        for mesh in m["meshes"]:
            for prim in mesh["primitives"]:
                pos, idx = m["accessors"][prim["attributes"]["POSITION"]], m["accessors"][prim["indices"]]
                for a in (pos, idx):
                    assert "byteStride" not in m["bufferViews"][a["bufferView"]]
                start = m["bufferViews"][pos["bufferView"]].get("byteOffset", 0) + pos.get("byteOffset", 0)
                for k in corpus.rng.integers(0, 12 * pos["count"], 6):     # any bits are a float
                    b[start + k] ^= 1 << int(corpus.rng.integers(0, 8))
                start = m["bufferViews"][idx["bufferView"]].get("byteOffset", 0) + idx.get("byteOffset", 0)
                dt = {5121: np.uint8, 5123: np.uint16, 5125: np.uint32}[idx["componentType"]]
                new = corpus.rng.integers(0, pos["count"], idx["count"]).astype(dt).tobytes()      # other indices, all in range
                b[start:start + len(new)] = new
        m["buffers"][0]["uri"] = prefix + "," + base64.b64encode(bytes(b)).decode()
        cases.append(("gltf", write(tmp_path, "flipped_%d.gltf" % n, json.dumps(m))))
    m = copy.deepcopy(g)
    m["materials"][0].setdefault("pbrMetallicRoughness", {})["roughnessFactor"] = 0.123
    cases.append(("gltf", write(tmp_path, "factor.gltf", json.dumps(m))))
    cases.append(("gltf", write(tmp_path, "sorted_keys.gltf", json.dumps(g, sort_keys=True))))
    reverse = lambda o: {k: reverse(o[k]) for k in reversed(list(o))} if isinstance(o, dict) else [reverse(x) for x in o] if isinstance(o, list) else o   # noqa: E731
    cases.append(("gltf", write(tmp_path, "reversed_keys.gltf", json.dumps(reverse(g)))))
    answers = run_probe(probe, cases, tmp_path)
    assert [(p, a) for p, a in answers.items() if a != "loaded"] == []
    for _, path in cases:
        ingest.load_model(path)


def test_hostile_table_is_refused_by_the_cpp_host(probe, corpus, tmp_path):
    answers = run_probe(probe, corpus.refused + corpus.refused_png + [("gltf", corpus.at_limit)], tmp_path)
    assert answers.pop(corpus.at_limit) == "loaded"                       # at the limit the content decides, and the content is valid
    assert len(answers) == len(corpus.refused) + len(corpus.refused_png) >= 22 * 5 + 6 + 7 + 6 + 6
    assert [os.path.basename(p) for p, a in answers.items() if not a.startswith("refused ")] == []
    uncaught = [a for a in answers.values() if "stoul" in a or "std::" in a or "basic_string" in a or "vector" in a]
    assert uncaught == []                                                 # the loader's own messages, not the standard library's


def test_hostile_table_is_refused_by_the_harness(corpus, ingest):
    accepted = []
    for _, path in corpus.refused:
        try:
            ingest.load_model(path)
            accepted.append(os.path.basename(path))
        except (RecursionError, MemoryError) as e:
            pytest.fail("%s: %r" % (os.path.basename(path), e))
        except Exception:
            pass
    assert accepted == []
    assert len(ingest.load_model(corpus.at_limit)) == 1 and len(ingest.load_model(corpus.base)) == 1


@pytest.mark.parametrize("kind,fewest", [("gltf", 4000), ("scene", 5000), ("dds", 1000), ("png", 15000)])
def test_truncations_end_in_loaded_or_refused(probe, corpus, tmp_path, kind, fewest):
    """every valid input cut short, at every byte if it has at most 4 KiB, else at every 97th; the models, images and .bin files that a
    cut file names stay whole beside it"""
    cases, homes = [], {}
    for path in [p for k, p in corpus.valid if k == kind]:
        data = open(path, "rb").read()
        if os.path.dirname(path) not in homes:
            homes[os.path.dirname(path)] = str(tmp_path / ("from_%d" % len(homes)))
            shutil.copytree(os.path.dirname(path), homes[os.path.dirname(path)])
        for cut in range(0, len(data), 1 if len(data) <= TRUNCATE_EVERY_BYTE_UP_TO else TRUNCATE_STRIDE):
            cases.append((kind, write(homes[os.path.dirname(path)], "cut_%d_%s" % (cut, os.path.basename(path)), data[:cut])))
    assert len(cases) > fewest
    run_probe(probe, cases, tmp_path)
