"""Animation rules on the CPU ("Animation"): key lookup and the clock, the slerp branches, what the ingest makes of the
fixture under tests/golden/anim (written by tests/golden/make_anim_fixture.py), and that the error bound of tests/animref.py is not loose."""
import importlib.util
import json
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "anim", "scene.json")
DEMO = os.path.join(ROOT, "directx-physically-based-raytracer_amd", "pt_demo")
NO_NODE = 0xFFFFFFFF


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref():
    return _module("animref")


@pytest.fixture(scope="module")
def sets():
    return _module("animsets")


@pytest.fixture(scope="module")
def ingest(pkg):
    import dxpbrt_amd.ingest as I
    return I


@pytest.fixture(scope="module")
def fixture(ingest):
    return ingest.load_scene(FIXTURE)


def qz(deg):
    a = math.radians(deg) / 2
    return np.array([0.0, 0.0, math.sin(a), math.cos(a)])


# ------------------------------------------------------------------------------------------------------------------------------ key lookup
def test_key_lookup(ref):
    times = [0.5, 1.0, 2.0]
    values = np.array([[1.0, 0, 0, 0], [3.0, 0, 0, 0], [7.0, 0, 0, 0]])
    at = lambda t: float(ref.interpolate(times, values, t, False).v[0])
    assert at(0.1) == 1.0                                                # before the first key: the first value
    assert at(2.0) == 7.0 and at(9.0) == 7.0                             # at and after the last key: the last value
    assert at(0.5) == 1.0 and at(1.0) == 3.0                             # exactly on a key: that key (upper_bound - 1, t = 0)
    assert at(0.75) == 2.0 and at(1.5) == 5.0
    assert ref.find_key(times, 1.0) == 1 and ref.find_key(times, 0.5) == 0 and ref.find_key(times, 2.0) == 3 and ref.find_key(times, 1.99) == 1
    one = lambda t: float(ref.interpolate([1.0], values[:1], t, False).v[0])
    assert one(0.0) == one(1.0) == one(5.0) == 1.0                       # a single key


def test_clock_tick_wraps_and_set_time_clamps(ptamd, pkg):
    S = pkg.scenes
    sc = S.animated_scene()
    clock = ptamd.Animation(None, sc.animations)                         # no device: clips and times only
    assert clock.duration(0) == 1.0
    clock.Tick(0.75); assert clock.times[0] == 0.75
    clock.Tick(0.5); assert clock.times[0] == math.fmod(1.25, 1.0)       # Animation::Tick: fmod(time + elapsed, duration)
    clock.SetTime(7.0); assert clock.times[0] == 1.0                     # Animation::SetTime: clamp
    clock.SetTime(-1.0); assert clock.times[0] == 0.0
    clock.SetSelectedIndex(0, 9); assert clock.clips[0] == 1             # AnimationCollection::SetSelectedIndex: min(index, size - 1)
    clock.SetTime(1.5); clock.Tick(1.0); assert clock.times[0] == 0.5    # across clip 1's duration of 2
    sc.animations[0].rig.durations[1] = 0.0                              # the deliberate divergence: Duration 0 stays at time 0 (the reference: NaN)
    clock.Tick(0.3); assert clock.times[0] == 0.0


# ----------------------------------------------------------------------------------------------------------------------------------- slerp
@pytest.mark.parametrize("a, b, t, branch, want", [
    (0.0, 0.2, 0.3, "lerp", None),                                       # dot = cos(0.1 deg) > 1 - 1e-5: the weights are (1 - t, t)
    (0.0, 200.0, 0.25, "slerp", -40.0),                                  # dot < 0: q1 is negated, the short way round (-160 degrees)
    (0.0, 90.0, 0.3, "slerp", 27.0),
    (10.0, 189.9, 0.6, "slerp", 10.0 + 0.6 * 179.9),
])
def test_slerp_branches(ref, a, b, t, branch, want):
    q, took = ref.slerp(ref.Bd(qz(a)), ref.Bd(qz(b)), ref.Bd(t))
    assert took == branch
    if want is None:
        assert np.allclose(q.v, (1 - t) * qz(a) + t * qz(b), atol=1e-15)
    else:
        w = qz(want)
        assert np.allclose(q.v, w, atol=1e-12) or np.allclose(q.v, -w, atol=1e-12)
    assert np.all(q.e < 1e-5) and np.all(q.e[2:] > 0)
    # a fp32 replay of the stated order lies within the bound
    f = np.float32
    q0, q1 = qz(a).astype(f), qz(b).astype(f)
    exact, _ = ref.slerp(ref.Bd(q0.astype(np.float64)), ref.Bd(q1.astype(np.float64)), ref.Bd(float(f(t))))
    c = f(f(f(q0[0] * q1[0]) + f(q0[1] * q1[1])) + f(q0[2] * q1[2])); c = f(c + f(q0[3] * q1[3]))
    if c < 0:
        c, q1 = -c, -q1
    if c > f(1.0) - f(1e-5):
        w0, w1 = f(1) - f(t), f(t)
    else:
        s = np.sqrt(f(1) - f(c * c), dtype=f); om = f(np.arctan2(s, c))
        w0, w1 = f(np.sin(f(f(f(1) - f(t)) * om), dtype=f) / s), f(np.sin(f(f(t) * om), dtype=f) / s)
    got = (f(w0) * q0 + f(w1) * q1).astype(np.float64)
    assert np.all(np.abs(got - exact.v) <= 2.0 * exact.e)


# ---------------------------------------------------------------------------------------------------------------------------------- ingest
def test_ingest_resolves_names_to_indices(fixture):
    a = fixture.animations[0]
    rig = a.rig
    assert rig.names == ["root", "column", "joint0", "joint1", "box", "box", "spare", "floor", "light"]      # node 4 of the file is not in the scene
    assert rig.parents.tolist() == [-1, 0, 0, 2, 0, 0, 0, -1, -1]                                            # depth first, parent < own index
    assert rig.clip_names == ["bend", "lift"]
    # the mesh nodes in traversal order: column, box, floor, light -> instances 0..3
    assert a.binding_instances.tolist() == [0, 1, 2, 3]
    assert a.binding_nodes.tolist() == [1, 5, 7, 8]                      # "box" is looked up by name: the LAST node of that name wins
    assert len(a.skins) == 1 and a.skins[0].mesh_node == 1 and a.skins[0].joint_nodes.tolist() == [2, 3] and a.skins[0].scene_node == 0
    ib = a.skins[0].inverse_binds
    assert ib.shape == (2, 4, 4) and np.array_equal(ib[0], np.eye(4)) and ib[1][3].tolist() == [0, -0.5, 0, 1]
    assert np.allclose(rig.rest[8], [0, 2.2, 0, 0, 0, 0, 1, 1, 1, 1])    # the light's matrix, decomposed
    assert np.allclose(rig.rest[0], [0.1, 0, 0.2, 0, 0, 0, 1, 1, 1.2, 1])
    assert fixture.scene_data["IsStatic"] == 0


def test_ingest_channel_rules(fixture):
    rig = fixture.animations[0].rig
    ch = rig.channels
    # the first channel wins: joint1's rotation is sampler 0 (0, 40, -25 degrees), not the doubled channel that reaches the name through node 4
    first, count = ch[0, 3, 1]
    assert count == 3 and rig.key_times[first:first + 3].tolist() == [0.0, 0.5, 1.0]
    assert np.allclose(rig.key_values[first:first + 3], [qz(0), qz(40), qz(-25)], atol=1e-7)
    assert ch[0, 3, 0, 1] == 0                                           # the STEP translation channel is skipped: the rest value stays
    assert ch[0].sum(axis=(0, 1))[1] == 3 + 2 + 2                        # and nothing else took keys: joint1, and "box" twice over
    # the keyframes of a name apply to every node that carries it: both "box" nodes share the same keys
    assert np.array_equal(ch[:, 4], ch[:, 5]) and ch[0, 4, 1, 1] == 2 and ch[1, 4, 0, 1] == 3 and ch[1, 4, 2, 1] == 2
    assert rig.durations.tolist() == [1.0, 2.0]                          # the largest accepted key time: the STEP channel's 3 s does not count
    assert np.all(ch[:, [0, 1, 6, 7, 8]] == 0)


def test_ingest_skeletal_vertices(fixture, pkg):
    L = pkg.layouts
    u8, u16 = fixture.nodes[0].meshes
    for mesh in (u8, u16):
        sk = mesh.skeletal_vertices
        assert sk.dtype == L.SKELETAL_VERTEX and len(sk) == len(mesh.vertices) == 20
        assert sk["Joints"].dtype == np.uint16 and np.all(sk["Joints"] == (0, 1, 0, 0))       # u8 and u16 components both become XMUSHORT4
        assert np.array_equal(sk["Position"], mesh.vertices["Position"]) and np.array_equal(sk["Normal"], mesh.vertices["Normal"])
        assert mesh.motion_vectors.shape == (20, 4) and mesh.motion_vectors.dtype == np.uint16
        h = mesh.vertices["Position"][:, 1]
        assert np.allclose(sk["Weights"][:, 1], h, atol=1e-5) and np.allclose(sk["Weights"][:, 0], 1 - h, atol=1e-5)
    assert np.array_equal(u8.skeletal_vertices["Weights"][:, 1], u8.vertices["Position"][:, 1])           # floats as they are
    q = np.round(65535 * u16.vertices["Position"][:, 1].astype(np.float64))
    assert np.array_equal(u16.skeletal_vertices["Weights"][:, 1], (q / 65535).astype(np.float32))          # normalised integers converted
    assert all(m.skeletal_vertices is None for n in fixture.nodes[1:] for m in n.meshes)


def test_ingest_unknown_animation_is_the_references_error(ingest, tmp_path):
    desc = json.load(open(FIXTURE))
    desc["Models"] = {"actor": os.path.join(os.path.dirname(FIXTURE), "column.gltf")}
    desc["RenderObjects"][0]["Animation"] = "nope"
    p = tmp_path / "scene.json"
    p.write_text(json.dumps(desc))
    with pytest.raises(RuntimeError) as e:
        ingest.load_scene(str(p))
    assert str(e.value) == f"{p}: RenderObject actor: Animations nope not found"


def test_ingest_refuses_hostile_animation_files(ingest, tmp_path):
    """the Python host on the hostile files: a truncated key accessor, a sampler whose counts differ, a joint beyond the nodes, a cycle"""
    v = _hostile_variants(tmp_path)
    for name in ("truncated", "counts", "cycle"):
        with pytest.raises((ValueError, IndexError)):
            ingest.load_animation(v[name])
    with pytest.raises(ValueError):
        ingest.load_model(v["joint"])


def _hostile_variants(tmp_path):
    """the fixture's .gltf with one thing wrong each, next to a copy of its .bin: name -> path"""
    src = os.path.join(os.path.dirname(FIXTURE), "column.gltf")
    (tmp_path / "column.bin").write_bytes(open(os.path.join(os.path.dirname(FIXTURE), "column.bin"), "rb").read())

    def truncated(g):
        acc = g["accessors"][g["animations"][0]["samplers"][0]["input"]]
        g["bufferViews"][acc["bufferView"]]["byteLength"] = 8           # three float keys need 12
    def counts(g):
        g["animations"][0]["samplers"][0]["input"] = g["animations"][0]["samplers"][3]["input"]      # 2 times, 3 values
    def joint(g):
        g["skins"][0]["joints"] = [2, 99]
    def cycle(g):
        g["nodes"][3]["children"] = [0]
    out = {}
    for name, edit in (("truncated", truncated), ("counts", counts), ("joint", joint), ("cycle", cycle)):
        g = json.load(open(src))
        edit(g)
        (tmp_path / (name + ".gltf")).write_text(json.dumps(g))
        out[name] = str(tmp_path / (name + ".gltf"))
    return out


# -------------------------------------------------------------------------------------------------------------------------- the C++ host
def test_both_hosts_resolve_the_same_rig(tmp_path, fixture):
    """pt_demo --dump-scene against ingest.py on the fixture: the resolved rig (parents, rest, durations, channels, keys), the object's bindings,
    the skin's joint nodes and inverse binds, and the skeletal vertices -- byte for byte, behind everything else in the dump."""
    dump = str(tmp_path / "anim.bin")
    info = json.loads(subprocess.check_output([DEMO, "--scene", FIXTURE, "--dump-scene", dump], text=True))
    a = fixture.animations[0]
    rig = a.rig
    parts = [rig.parents.astype("<i4"), rig.rest.astype("<f4"), rig.durations.astype("<f8"), rig.channels.astype("<u4"), rig.key_times.astype("<f4"),
             rig.key_values.astype("<f4"), np.asarray(a.transform, "<f4"), a.binding_nodes.astype("<u4"), a.binding_instances.astype("<u4"),
             np.asarray(a.binding_globals, "<f4")]
    for s in a.skins:
        parts += [s.joint_nodes.astype("<u4"), np.asarray(s.inverse_binds, "<f4")]
    skinned = [(n, m) for n, node in enumerate(fixture.nodes) for m, mesh in enumerate(node.meshes) if mesh.skeletal_vertices is not None]
    parts += [fixture.nodes[n].meshes[m].skeletal_vertices for n, m in skinned]
    want = b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
    raw = open(dump, "rb").read()
    assert raw[len(raw) - len(want):] == want
    (got,) = info["animations"]
    assert got["parents"] == rig.parents.tolist() and got["nodes"] == len(rig.parents) and got["clips"] == 2 and got["keys"] == len(rig.key_times)
    assert got["key_counts"] == rig.channels[..., 1].reshape(-1).tolist()
    assert got["binding_nodes"] == a.binding_nodes.tolist() and got["binding_instances"] == a.binding_instances.tolist()
    assert got["skins"] == [{"mesh_node": 1, "scene_node": 0, "joints": [2, 3]}]
    assert info["skeletal"] == [list(x) for x in skinned] == [[0, 0], [0, 1]]


def test_cpp_host_refuses_hostile_animation_files(tmp_path):
    """a truncated key accessor, a sampler whose input and output counts differ, a joint index beyond the nodes, a children cycle: each a clean
    non-zero exit with a message from pt_demo --dump-scene, not a crash"""
    for name, path in _hostile_variants(tmp_path).items():
        desc = json.load(open(FIXTURE))
        desc["Models"] = {"actor": path}; desc["Animations"] = {"moves": path}
        scene = tmp_path / (name + ".json")
        scene.write_text(json.dumps(desc))
        q = subprocess.run([DEMO, "--scene", str(scene), "--dump-scene", str(tmp_path / "x.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert q.returncode == 1 and q.stderr.startswith("pt_demo: ") and len(q.stderr) > 12, (name, q.returncode, q.stderr)
    desc = json.load(open(FIXTURE))
    desc["Models"] = {"actor": os.path.join(os.path.dirname(FIXTURE), "column.gltf")}
    desc["RenderObjects"][0]["Animation"] = "nope"
    scene = tmp_path / "unknown.json"
    scene.write_text(json.dumps(desc))
    q = subprocess.run([DEMO, "--scene", str(scene), "--dump-scene", str(tmp_path / "x.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert q.returncode == 1 and q.stderr.strip() == f"pt_demo: {scene}: RenderObject actor: Animations nope not found"


# ---------------------------------------------------------------------------------------------------------------- the bound is not loose
def _everything(ref, obj, clip, time, mutant=None):
    g = ref.pose(obj.rig, clip, time, mutant)
    out = list(g) + ref.instance_transforms(obj, g, mutant)
    for k in range(len(obj.skins)):
        out += [m for m in ref.skeletal_transforms(obj, g, k, mutant) if m is not None]
    return out


def test_the_bound_is_not_loose(ref, sets, pkg, fixture):
    """Each of four wrong poses -- T.R.S for S.R.T, t for 1 - t, the missing sign flip, untransposed storage -- moves some entry, on the
    fixtures, by more than 100 times the largest bound animref issues there: a device that made one of these mistakes cannot hide in it."""
    cases = [(o, c, t) for pair in sets.STATES for o, (c, t) in zip(sets.parity_objects(pkg.scenes), pair)]
    cases += [(fixture.animations[0], c, t) for c, t in ((0, 0.37), (0, 0.6), (1, 0.8), (1, 1.7))]
    cases += [(pkg.scenes.animated_scene().animations[0], c, t) for c, t in ((0, 0.4), (1, 1.1))]
    for rig_cases in (cases[:24], cases[24:28], cases[28:]):             # per fixture: the parity set, the glTF fixture, the animated scene
        good = [_everything(ref, o, c, t) for o, c, t in rig_cases]
        largest = max(float(m.e.max()) for ms in good for m in ms)
        assert 0 < largest < 1e-3
        for mutant in ref.MUTANTS:
            moved = max(float(np.abs(a.v - b.v).max()) for (o, c, t), ms in zip(rig_cases, good) for a, b in zip(ms, _everything(ref, o, c, t, mutant)))
            assert moved > 100.0 * largest, (mutant, moved, largest)
    for o, c, t in cases:                                                # the condition the neglected second-order terms rest on
        g = ref.pose(o.rig, c, t)
        for s in o.skins:
            if int(s.mesh_node) != NO_NODE:
                assert ref.condition(g[int(s.mesh_node)].v) <= 1e3
