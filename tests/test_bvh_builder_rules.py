"""tests/bvhref.py without a GPU: what its checks accept and what they notice.

bvhref.build() emits the restatement's own optimal tree as node records; put into a hand-assembled traversal copy it must pass
bvhref.check and bvh_check.check_blob. Then ONE rule is damaged at a time on the way to an otherwise valid tree (bvh_check.check_blob,
the weaker check, still passes) and the part of bvhref.check named for that rule must say so. tests/test_bvh_builder_gpu.py asks the same
checks of the trees the device builds."""
import re

import numpy as np
import pytest

import bvh_check
import bvhref

f32 = np.float32


# the builder's constants, restated (pt_trace.hpp blas_leaf_tris / kMaxLeafTris, pt_bvh.hip kCostTriangle / kCostInstance / kCostNode /
# kTlasCubicCells / kTlasLargeFraction, and the arguments of build_wide_tree in build_blas_device / build_tlas_device)
def leaf_rule(n):
    return 2 if n <= 32 else 1


def blas_params(n):
    return bvhref.Params(leaf_size=leaf_rule(n), max_leaf_items=3, cost_item=0.6, cubic=True, large_first=False, cost_node=1.0)


TLAS = bvhref.Params(leaf_size=1, max_leaf_items=1, cost_item=1.0, cubic=True, large_first=True, cost_node=1.0, large_fraction=0.25)


class Layout:
    pass


def assemble(meshes, objects, blas_hooks=None, tlas_hooks=None):
    """meshes: [n, 3, 3] float32 triangle arrays (one geometry each); objects: (mesh, 3x4 objectToWorld). -> (layout, buf, trees): a
    traversal copy as pt_debug_download_blob lays it out, every tree built by bvhref.build (the hooks go to the bottom level of mesh 0
    and to the top level)."""
    packets, rows, node_secs, entries, trees = [], [], [], [], []
    tri_base = 0
    for m, tris in enumerate(meshes):
        tris = np.asarray(tris, f32).reshape(-1, 3, 3)
        nodes, item_at, T, slot_at = bvhref.build(tris.min(1), tris.max(1), blas_params(len(tris)), **((blas_hooks or {}) if m == 0 else {}))
        p = np.zeros(len(tris), bvh_check.TRI_DT)
        p["v0"], p["v1"], p["v2"], p["prim"] = tris[item_at, 0], tris[item_at, 1], tris[item_at, 2], item_at
        r = np.zeros((len(tris), 4), np.uint32); r[:, :3] = 3 * item_at[:, None] + np.arange(3)
        packets.append(p); rows.append(r); node_secs.append(nodes)
        entries.append((tri_base, len(tris))); trees.append((T, item_at, slot_at))
        tri_base += len(tris)
    inst = np.zeros(len(objects), bvh_check.INST_DT)
    tlas_capacity = len(objects) + 1
    node_base = np.cumsum([tlas_capacity] + [len(n) for n in node_secs])
    for i, (m, M) in enumerate(objects):
        M = np.asarray(M, f32).reshape(3, 4)
        A = np.eye(4); A[:3] = M.astype(np.float64)
        inst[i]["objectToWorld"] = M.reshape(-1)
        inst[i]["worldToObject"] = np.linalg.inv(A)[:3].astype(f32).reshape(-1)
        inst[i]["nodeBase"], (inst[i]["triBase"], inst[i]["triCount"]) = node_base[m], entries[m]
        inst[i]["mask"], inst[i]["instanceID"], inst[i]["instanceIndex"] = 0xFF, i, i
    tris_all = np.concatenate(packets)
    lo, hi = bvhref.instance_boxes(inst, tris_all, lambda i: trees[objects[i][0]][0].root_bounds())
    inst["boxLo"], inst["boxHi"] = bvhref.pad_boxes(lo, hi)
    tnodes, order, TT, tslot = bvhref.build(lo, hi, TLAS, **(tlas_hooks or {}))
    tsec = np.zeros(tlas_capacity, bvh_check.NODE_DT); tsec[:len(tnodes)] = tnodes
    lay = Layout()                                           # (child indices of a bottom level are relative to its own root)
    secs = [inst, np.concatenate([tsec] + node_secs), tris_all, np.concatenate(rows), inst[order]]
    offs = np.cumsum([0] + [s.nbytes for s in secs])
    lay.InstanceOffset16, lay.NodeOffset16, lay.TriangleOffset16, lay.LeafInstanceOffset16 = (int(offs[k]) // 16 for k in (0, 1, 2, 4))
    lay.InstanceCount, lay.NodeCount, lay.TriangleCount = len(inst), len(secs[1]), len(tris_all)
    buf = np.concatenate([s.view(np.uint8).reshape(-1) for s in secs])
    return lay, buf, dict(blas=trees, tlas=(TT, order, tslot), tlas_boxes=(lo, hi))


IDENTITY = np.eye(3, 4, dtype=f32)


def soup(n, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * 0.05).astype(f32)


def flat_grid(n=12, half=3.0):
    xs = np.linspace(-half, half, n + 1)
    t = []
    for j in range(n):
        for i in range(n):
            p = [(xs[i], 0, xs[j]), (xs[i + 1], 0, xs[j]), (xs[i + 1], 0, xs[j + 1]), (xs[i], 0, xs[j + 1])]
            t += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    return np.array(t, f32)


def identical(n=70):
    return np.tile(np.array([[(0.25, 0.5, 1.0), (1.25, 0.5, 1.5), (0.5, 1.5, 1.25)]], f32), (n, 1, 1))


def field(n=60, seed=3):
    """n small tetrahedra, a ground plane under them and a box around them: a top level with large and small instances"""
    rng = np.random.default_rng(seed)
    tet = np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 0), (0, 1, 0), (0, 0, 1)], [(0, 0, 0), (0, 0, 1), (1, 0, 0)], [(1, 0, 0), (0, 0, 1), (0, 1, 0)]], f32)
    quad = np.array([[(-1, 0, -1), (-1, 0, 1), (1, 0, 1)], [(-1, 0, -1), (1, 0, 1), (1, 0, -1)]], f32)
    cube = np.concatenate([np.roll(np.concatenate([quad + (0, s, 0) for s in (-1, 1)]), k, axis=2) for k in range(3)]).astype(f32)
    objects = []
    for _ in range(n):
        M = np.zeros((3, 4), f32); M[:, :3] = np.diag(rng.uniform(0.05, 0.2, 3)); M[:, 3] = rng.uniform(-4, 4, 3) * (1, 0.1, 1)
        objects.append((0, M))
    G = np.zeros((3, 4), f32); G[:, :3] = np.diag((5, 1, 5)); G[1, 3] = -0.5
    E = np.zeros((3, 4), f32); E[:, :3] = np.diag((6, 6, 6))
    return [tet, quad, cube], objects[:n // 2] + [(1, G)] + objects[n // 2:] + [(2, E)], n // 2


def tags(fn):
    """the parts named in the AssertionError fn() raises ('' when it passes)"""
    try:
        fn()
    except AssertionError as e:
        return "".join(sorted({line.split("[")[1][0] for line in str(e).splitlines() if "[" in line}))
    return ""


def full_check(lay, buf, parts="abcdefg"):
    return bvhref.check(lay, buf, blas_params, TLAS, parts=parts)


# ---------------------------------------------------------------------------------------------
# sound trees pass
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "flat_grid", "identical", "small", "field"])
def test_the_restated_tree_passes_both_checkers(name):
    if name == "field":
        meshes, objects, ground = field()
    else:
        meshes, objects = [{"soup": soup(300), "flat_grid": flat_grid(), "identical": identical(), "small": soup(31, 2)}[name]], [(0, IDENTITY)]
    lay, buf, trees = assemble(meshes, objects)
    bvh_check.check_blob(lay, buf, leaf_rule)
    res = full_check(lay, buf)
    for T, r, _ in list(res["trees"].values()) + [res["tlas"] + (None,)]:
        assert r["cost"] <= r["optimum"] * (1 + 1e-12) and r["cost"] >= r["optimum"] * (1 - 1e-12), (r, "the tree read off the tables costs what the tables say")
    T = trees["blas"][0][0]
    if name == "identical":
        assert len(set(T.keys.tolist())) == 1                       # every key equal: the positional tree
        assert np.array_equal(T.order, np.arange(T.n))              # and a stable sort
        n = T.nleaves
        assert all(T.first[i] >> (T.first[i] ^ T.last[i]).bit_length() == T.last[i] >> (T.first[i] ^ T.last[i]).bit_length() for i in range(n - 1))
        assert T.height == int(np.ceil(np.log2(n)))
    if name == "field":
        TT = trees["tlas"][0]
        assert TT.large.sum() == 2 and TT.large[ground] and TT.large[-1]
        assert (TT.keys[TT.large] >> np.uint64(62) == 1).all() and (TT.keys[~TT.large] >> np.uint64(62) == 0).all()


def test_empty_instance_boxes_take_cell_zero():
    """an inverted (empty) box has a NaN centre: cell 0 on every axis, never large, and it moves no scene bound"""
    lo = np.array([(1, 1, 1), (np.inf,) * 3, (2, 3, 4)], f32); hi = np.array([(2, 2, 2), (-np.inf,) * 3, (3, 4, 5)], f32)
    keys, large = bvhref.morton_keys(lo, hi, TLAS)
    assert int(keys[1]) == 0 and not large[1] and int(keys[2]) & ((1 << 62) - 1) != 0
    k2, _ = bvhref.morton_keys(lo[[0, 2]], hi[[0, 2]], TLAS)
    assert keys[[0, 2]].tolist() == k2.tolist()
    T = bvhref.Tree(lo, hi, TLAS)
    assert T.order.tolist() == [1, 0, 2] and T.optimum > 0 and np.isfinite(T.optimum)      # (the other two are large); the empty box costs nothing


# ---------------------------------------------------------------------------------------------
# every single mutation is noticed by the check named for it
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sound():
    tris = soup(300)
    lay, buf, trees = assemble([tris], [(0, IDENTITY)])
    full_check(lay, buf)
    return tris, lay, buf, trees


def mutated(tris, **hooks):
    lay, buf, _ = assemble([tris], [(0, IDENTITY)], blas_hooks=hooks)
    bvh_check.check_blob(lay, buf, leaf_rule)                      # still a valid tree: the weaker check has nothing to say
    return lay, buf


def test_packets_swapped_across_leaves(sound):
    tris, lay, buf, trees = sound
    T, item_at, slot_at = trees["blas"][0]
    # Two single leaves under ONE wide node are dealt to their slots by their boxes alone: exchanging them changes nothing at all. So: the
    # first pair of Morton neighbours that the damaged build still files under different wide nodes.
    def swapper(i):
        def swap(order):
            order[[i, i + 1]] = order[[i + 1, i]]
            return order
        return swap
    for i in range(T.n - 1):
        _, item2, _, slot2 = bvhref.build(tris.min(1), tris.max(1), blas_params(len(tris)), order_hook=swapper(i))
        where = {int(it): int(sl) // 8 for it, sl in zip(item2, slot2)}
        if where[int(T.order[i])] != where[int(T.order[i + 1])]:
            break
    swap = swapper(i)
    lay2, buf2 = mutated(tris, order_hook=swap)
    assert tags(lambda: full_check(lay2, buf2)) == "a"
    full_check(lay2, buf2, parts="bcdefg")


def test_a_key_that_lost_an_axis(sound):
    tris, lay, buf, trees = sound
    T = trees["blas"][0][0]
    victim = int(T.order[T.n // 2])

    def lose_x(keys):
        keys[victim] &= ~np.uint64(0x4924924924924924)            # every third bit from bit 2: the x cell
        return keys
    assert int(T.keys[victim]) & 0x4924924924924924
    lay2, buf2 = mutated(tris, keys_hook=lose_x)
    assert "a" in tags(lambda: full_check(lay2, buf2))
    full_check(lay2, buf2, parts="defg")                           # the tree is sound in itself: boxes, slots and exponents follow its own order


def test_a_dearer_collapse_decision(sound, capsys):
    tris, lay, buf, trees = sound
    T = trees["blas"][0][0]
    c0, c1 = T.cost[T.left[0]], T.cost[T.right[0]]
    k = max(range(1, 8), key=lambda k: c0[k - 1] + c1[7 - k])
    assert k != T.split[0][8]
    lay2, buf2 = mutated(tris, force={(0, 8): k})
    with pytest.raises(AssertionError, match=r"\[c\]") as e:
        full_check(lay2, buf2)
    assert tags(lambda: full_check(lay2, buf2)) == "c"
    ratio = (c0[k - 1] + c1[7 - k] - T.dist8[0]) / T.optimum
    with capsys.disabled():
        print(f"\n[rules] root dealt {k} + {8 - k} roots instead of {T.split[0][8]} + {8 - T.split[0][8]}: cost ratio - 1 = {ratio:.3e} = {ratio / bvhref.eps_of(T.height):.0f} eps  ({str(e.value).splitlines()[0]})")
    assert ratio > 100 * bvhref.eps_of(T.height)


def test_a_stale_cost_table(sound, capsys):
    tris, lay, buf, trees = sound
    T = trees["blas"][0][0]
    stale = T.left[0] if T.left[0] >= 0 else T.right[0]
    lay2, buf2 = mutated(tris, stale=stale)
    with pytest.raises(AssertionError, match=r"\[c\]") as e:
        full_check(lay2, buf2)
    assert tags(lambda: full_check(lay2, buf2)) == "c"
    r = float(re.search(r": (\S+) above it", str(e.value)).group(1))
    with capsys.disabled():
        print(f"\n[rules] the root decided on a zeroed table of node {stale}: cost ratio - 1 = {r:.3e} = {r / bvhref.eps_of(T.height):.0f} eps")
    assert r > 100 * bvhref.eps_of(T.height)


def blas_nodes(lay, buf):
    inst, nodes, tris, order = bvh_check.split(lay, buf)
    return nodes[int(inst[0]["nodeBase"]):]


def test_an_exponent_one_too_large(sound):
    tris, lay, buf, trees = sound
    d = buf.copy()
    n = blas_nodes(lay, d)
    n["exp"][0, 0] += 1                                             # requantised to the coarser grid, outward: still contains everything
    occ = n["meta"][0] != 0
    n["qlox"][0, occ] = n["qlox"][0, occ] // 2
    n["qhix"][0, occ] = (n["qhix"][0, occ].astype(np.int64) + 1) // 2
    bvh_check.check_blob(lay, d, leaf_rule)
    assert tags(lambda: full_check(lay, d)) == "d"
    assert tags(lambda: full_check(lay, d, parts="d")) == "d" and "fits 0..255 at" in _message(lambda: full_check(lay, d))


def _message(fn):
    with pytest.raises(AssertionError) as e:
        fn()
    return str(e.value)


def test_a_box_two_quanta_out(sound):
    tris, lay, buf, trees = sound
    d = buf.copy()
    n = blas_nodes(lay, d)
    w, s = next((w, s) for w in range(len(n)) for s in range(8) if n["meta"][w, s] and n["qhiy"][w, s] <= 253)
    n["qhiy"][w, s] += 2
    bvh_check.check_blob(lay, d, leaf_rule)
    assert tags(lambda: full_check(lay, d)) == "e"
    assert "more than a quantum" in _message(lambda: full_check(lay, d))


def test_an_unpadded_box():
    # far from the origin the padding (1e-5 of the coordinate) is many quanta of a node; near it a quantum hides it
    tris = (soup(300) * f32(0.25) + np.array([4096.5, -2048.25, 1024.125])).astype(f32)
    lay, buf, _ = assemble([tris], [(0, IDENTITY)])
    full_check(lay, buf)
    lay2, buf2 = mutated(tris, unpad_leaf=17)
    msg = _message(lambda: full_check(lay2, buf2))
    assert "[e]" in msg and "sticks out" in msg
    full_check(lay2, buf2, parts="abcfg")


def test_two_slots_exchanged(sound):
    tris, lay, buf, trees = sound
    lay2, buf2 = mutated(tris, swap_slots=(0, 1, 4))
    assert tags(lambda: full_check(lay2, buf2)) == "f"
    full_check(lay2, buf2, parts="abcdeg")


def test_the_large_flag_dropped_for_the_ground():
    meshes, objects, ground = field()

    def drop(keys):
        assert int(keys[ground]) >> 62 == 1
        keys[ground] &= ~(np.uint64(1) << np.uint64(62))
        return keys
    lay, buf, _ = assemble(meshes, objects)
    full_check(lay, buf)
    lay2, buf2, _ = assemble(meshes, objects, tlas_hooks=dict(keys_hook=drop))
    bvh_check.check_blob(lay2, buf2, leaf_rule)
    msg = _message(lambda: full_check(lay2, buf2))
    assert "top level" in msg and "[a]" in msg


# ---------------------------------------------------------------------------------------------
# the restatement against itself
# ---------------------------------------------------------------------------------------------
def karras(keys):
    """Karras 2012, figure 4, node by node, with delta(i, j) = common prefix of (key, position): a transcription used ONLY here, to
    cross-check the top-down construction. -> {(first, last): split}"""
    n = len(keys)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        x = int(keys[i]) ^ int(keys[j])
        return 64 - x.bit_length() if x else 64 + 32 - (i ^ j).bit_length()
    out = {}
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t, div = 0, (l + 1) // 2, 2
        while True:
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t == 1:
                break
            div *= 2; t = (l + div - 1) // div
        gamma = i + s * d + min(d, 0)
        out[(min(i, j), max(i, j))] = gamma + 1
    return out


@pytest.mark.parametrize("seed", range(6))
def test_the_top_down_radix_tree_is_karras_tree(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 400))
    pool = rng.integers(0, 1 << 63, max(2, n // (1 + seed)), dtype=np.uint64)           # seed 0: few duplicates ... seed 5: mostly duplicates
    keys = np.sort(pool[rng.integers(0, len(pool), n)])
    if seed == 5:
        keys[:] = keys[0]
    first, last, left, right = bvhref.radix_tree(keys)
    mine = {(first[i], last[i]): (right[i] if right[i] < 0 else None, first[right[i]] if right[i] >= 0 else ~right[i]) for i in range(len(first))}
    assert {k: v[1] for k, v in mine.items()} == karras(keys)
    assert len(first) == n - 1


@pytest.mark.parametrize("name", ["soup", "flat_grid", "identical", "field"])
def test_the_optimum_is_no_dearer_than_the_greedy_collapse(name, capsys):
    if name == "field":
        meshes, objects, _ = field()
        _, _, trees = assemble(meshes, objects)
        T = trees["tlas"][0]
    else:
        t = {"soup": soup(300), "flat_grid": flat_grid(), "identical": identical()}[name]
        T = bvhref.Tree(t.min(1), t.max(1), blas_params(len(t)))
    g = T.greedy_cost()
    with capsys.disabled():
        print(f"\n[rules] {name}: optimum {T.optimum:.6g}, greedy collapse {g:.6g}")
    assert T.optimum <= g
    assert all(T.cost[n][i] <= T.cost[n][i - 1] for n in range(len(T.first)) for i in range(1, 7))     # more roots never cost more
